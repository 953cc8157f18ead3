"""The shapes test_gpu_field_geometry.py (GPU) and test_field_geometry_host.py (CPU) share: the kernels that sweep a whole
flow field -- camera motion (motion_model.hip), flow weights (lloyd_weighted.hip), blob keys (blobs.hip), per-cell cluster
counts (grid_labels.hip) -- at the launch geometry a full-size clip gives them, on fields small enough for a test.

Why: the tests of those kernels are exact but tiny.  There a moment work-group takes one share and the solve adds at most
23 partials; the weight and key kernels never start their grid-stride second pass; the grid counts never leave their first
65 535-frame chunk.  Every path named in PATHS below is what a 1080p clip or the benchmark runs and no other test does.

The references are the existing ones: camera_motion_cases for the moments, the fit and the subtraction, numpy's f32
expression for the weights and the threshold keys, ofc_lloyd_step_dev for the model keys, motion_grid_cases.model_counts
for the grid counts (restated here over all frames at once, and held to model_counts by the host test).  numpy only at
import."""
import numpy as np

from tests import camera_motion_cases as CC

# ---------------------------------------------------------------------------------------------------------------------
# 1. the motion kernels
# ---------------------------------------------------------------------------------------------------------------------
MOTION_SHARE = 2048                 # vectors of a share (csrc/motion_model.h)
SOLVE_LANES = 64                    # k_motion_solve: one wave per pair, a lane adds every 64th partial
THRESHOLDS = CC.DEFAULT_THRESHOLDS

PATHS = ("several shares per group",            # per > 1: the loop over shares, the accumulators carried, MmWalk restarted
         "short last group",                    # the last used group takes fewer than per shares
         "empty groups",                        # trailing groups with no share still write an all-zero partial
         "every group full",                    # per > 1 and neither of the two above
         "more than 64 partials",               # k_motion_solve's loop runs more than once per lane
         "2048 / npair groups",                 # the branch of the group formula that needs npair >= 9
         "floor of 16 groups",                  # and its floor, npair >= 128
         "narrow frame over several shares")    # W < 64: dy >= 1 in the walk, restarted at every share


def cdiv(a, b):
    return -(-a // b)


class MotionShape:
    """W x H x npair, the kinds it is fitted with, the geometry it was chosen for as (nshare, groups, per, used groups,
    shares of the last used group) and the paths it is in the table for"""

    def __init__(self, W, H, npair, kinds, geometry, reaches, seed=3):
        self.W, self.H, self.npair, self.kinds, self.geometry, self.reaches, self.seed = W, H, npair, kinds, geometry, reaches, seed
        self.name = f"{W}x{H}x{npair}"

    def __repr__(self):
        return self.name

    # which distinct field pair i carries: 0..3 the four backgrounds in turn, 4 the specials, 5 all outside
    def layout(self):
        idx = np.arange(self.npair) % 4
        if self.npair > 1:
            idx[5], idx[self.npair - 2] = 4, 5
        return idx

    def distinct(self):
        """the fields the pairs cycle through, (4 or 6, H, W, 2) f32"""
        if self.npair == 1:
            return background(self.W, self.H, self.seed)[None]
        four = [background(self.W, self.H, self.seed + 100 * s) for s in range(4)]
        return np.stack(four + [specials(self.W, self.H, self.seed + 400), CC._all_outside(self.W, self.H, 0)])


def background(W, H, seed):
    return CC.background(W, H, seed=seed)


def specials(W, H, seed):
    """one background with the non-finite vectors of camera_motion_cases' "non-finite" and the range limits of its
    "range-limit" together"""
    f, g = CC._non_finite(W, H, seed), CC._range_limit(W, H, seed)
    for y, x in ((3, 5), (3, 6), (4, 5), (4, 6), (10, 7)):
        f[y, x] = g[y, x]
    return f


SPECIALS_OUTSIDE = 6 + 3            # vectors of `specials` that are not valid: six non-finite, 1024, -1024, (below, 1024)

# Least margin (the least distance of a valid residual from a round's threshold, over the shape's distinct fields and
# kinds; the bar is CC.MARGIN = 2^-20 = 9.5e-7) and largest kappa_inf (the bar is CC.KAPPA_MAX = 2^20) beside each shape,
# as test_field_geometry_host.py measures them.  The seed is 3 unless that test failed with it (then the next that passes).
MOTION_SHAPES = [
    MotionShape(449, 457, 1, ("affine",), (101, 101, 1, 101, 1),                                     # margin 9.56e-1, kappa 1.46
                ("more than 64 partials",)),
    MotionShape(1031, 512, 1, ("affine", "translation"), (258, 256, 2, 129, 2),                     # margin 1.58e-5 affine, 2.06e-6 translation; kappa 2.35
                ("several shares per group", "empty groups", "more than 64 partials")),
    MotionShape(131, 523, 9, ("affine",), (34, 34, 1, 34, 1),                                        # margin 4.38e-1, kappa 2.11
                ("2048 / npair groups",), seed=7),
    MotionShape(131, 523, 128, ("affine", "translation"), (34, 16, 3, 12, 1),                       # margin 4.38e-1 affine, 5.40e-6 translation; kappa 2.11 (seeds 3 .. 5: translation below the bar)
                ("several shares per group", "short last group", "empty groups", "floor of 16 groups"), seed=7),
    MotionShape(257, 255, 128, ("affine",), (32, 16, 2, 16, 2),                                      # margin 3.68e-1, kappa 2.05
                ("several shares per group", "every group full", "floor of 16 groups")),
    MotionShape(48, 2731, 1, ("affine",), (65, 65, 1, 65, 1),                                        # margin 9.56e-1, kappa 3.00
                ("narrow frame over several shares", "more than 64 partials")),
]
MOTION_BY_NAME = {s.name: s for s in MOTION_SHAPES}
MOTION_CASES = [(s, kind) for s in MOTION_SHAPES for kind in s.kinds]
# the batch whose pairs are also fitted one call each: 16 groups of 3 shares in the batch, 34 groups of 1 share alone
ONE_BY_ONE = "131x523x128"


def motion_case_id(case):
    return f"{case[0].name}-{case[1]}"


def paths_of(W, H, npair, geometry):
    """the PATHS a launch reaches, from what ofc_motion_launch_geometry reports for it: (groups, per, used, last)"""
    groups, per, used, last = geometry
    nshare = cdiv(W * H, MOTION_SHARE)
    out = set()
    if per > 1:
        out.add("several shares per group")
        if last < per:
            out.add("short last group")
        if used < groups:
            out.add("empty groups")
        if last == per and used == groups:
            out.add("every group full")
    if groups > SOLVE_LANES:
        out.add("more than 64 partials")
    if npair >= 9 and 2048 // npair < 256 and groups == min(nshare, max(16, 2048 // npair)):
        out.add("2048 / npair groups")
        if 2048 // npair <= 16 and groups == 16:
            out.add("floor of 16 groups")
    if W < 64 and nshare > 1:
        out.add("narrow frame over several shares")
    return out


_cache = {}


def motion_reference(shape, kind):
    """(the distinct fields, [CC.fit(...) per distinct field], layout), computed once and shared: read-only"""
    key = (shape.name, kind)
    if key not in _cache:
        if ("fields", shape.name) not in _cache:
            d = shape.distinct()
            d.setflags(write=False)
            _cache["fields", shape.name] = d
        d = _cache["fields", shape.name]
        _cache[key] = (d, [CC.fit(f, CC.KIND[kind], THRESHOLDS) for f in d], shape.layout())
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the stream's camera where the flush gets another geometry than the full batch
# ---------------------------------------------------------------------------------------------------------------------
STREAM_W, STREAM_H, STREAM_BATCH, STREAM_PUSHES, STREAM_GRID = 449, 457, 24, 28, (3, 4)
STREAM_FLUSH = (STREAM_PUSHES - 1) % STREAM_BATCH                   # 3 pairs
STREAM_GEOMETRY = {STREAM_BATCH: (85, 2), STREAM_FLUSH: (101, 1)}    # pairs of a batch -> (groups, per)
STREAM_PARAMS = (256, 8.0)
STREAM_CENTRES = np.array([[0.0137, 0.0211], [0.5113, -0.2891], [2.9931, -2.0117]])


def stream_clip():
    """(28, 457, 449) u8: a texture under a slow pan that changes from frame to frame, and a block of it that moves on its
    own by (3, -2) px per frame on top of the pan"""
    from opticalflowclustering_amd import synth
    p = synth.texture_params(21)
    W, H, n = STREAM_W, STREAM_H, STREAM_PUSHES
    step = np.random.default_rng(8).uniform(0.2, 0.9, (n, 2)) * (1.0, -0.6)
    pan = np.cumsum(step, axis=0) - step[0]
    yy, xx = np.mgrid[0:H, 0:W]
    block = (yy >= 150) & (yy < 290) & (xx >= 120) & (xx < 270)
    out = []
    for t in range(n):
        dx = np.where(block, pan[t, 0] + 3.0 * t, pan[t, 0])
        dy = np.where(block, pan[t, 1] - 2.0 * t, pan[t, 1])
        out.append(synth.frame(W, H, dx, dy, p))
    return np.stack(out).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# 3. flow weights and blob keys past their grid caps
# ---------------------------------------------------------------------------------------------------------------------
WEIGHTS_PASS = 4 * 256 * 4096                   # vectors of one pass of k_flow_weights: 4096 work-groups, 256 lanes, 4 each
WEIGHTS_N = WEIGHTS_PASS + 1027                 # a full pass, a partial second one, and a scalar tail of 3
KEYS_PASS_VEC = 4 * 256 * 8192                  # one pass of k_blob_keys with four vectors per lane ...
KEYS_PASS_ONE = 256 * 8192                      # ... and with one
KEYS_N = KEYS_PASS_VEC + 4 * 256 * 3 + 2        # a partial second pass and a tail of 2; four passes and a bit without VEC
KEYS_W, KEYS_H, KEYS_PAIRS = 322757, 13, 2      # W * H * pairs = KEYS_N = 2 * 13 * 322757, the last one prime
THR = 0.5


def big_field(n, seed, boundaries):
    """(n, 2) f32: small finite vectors around the threshold THR, and at the first index, the last ones and either side of
    every index in `boundaries` the specials of the threshold tests: NaN, inf, zeros, and vectors whose u*u + v*v is the
    f32 just below, at and just above THR*THR"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, 2), dtype=np.float32)
    f *= np.float32(THR)
    t = np.float32(THR)
    below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(np.inf))
    special = np.array([[np.nan, 0], [0, np.inf], [0, 0], [-0.0, 0.0], [t, 0], [0, -below], [above, 0], [-np.inf, np.nan]], np.float32)
    for b in sorted(set([0, n]) | set(boundaries)):
        lo, hi = max(b - 8, 0), min(b + 8, n)
        f[lo:hi] = np.resize(special, (hi - lo, 2))
    return f


def weights_field():
    return big_field(WEIGHTS_N, 31, (WEIGHTS_PASS, WEIGHTS_PASS + 1024))


def keys_field():
    """(KEYS_PAIRS, KEYS_H, KEYS_W, 2) f32"""
    bounds = [KEYS_PASS_VEC, KEYS_PASS_VEC + 4 * 256 * 3] + [KEYS_PASS_ONE * i for i in (1, 2, 3, 4)] + [KEYS_W * KEYS_H]
    return big_field(KEYS_N, 32, bounds).reshape(KEYS_PAIRS, KEYS_H, KEYS_W, 2)


KEYS_K = 5
KEYS_MEAN = np.array([0.0625, -0.125])
KEYS_CENTRES_C = np.array([[0.0, 0.0], [0.7, 0.1], [-0.6, 0.5], [0.2, -0.8], [-0.4, -0.5]])      # centred, as the kernels take them
KEYS_SELECT = 0b10101               # clusters 0, 2 and 4: holes at 1 and 3

# ---------------------------------------------------------------------------------------------------------------------
# 4. grid counts across the 65 535-frame chunk of gridDim.y
# ---------------------------------------------------------------------------------------------------------------------
GRID_CHUNK = 65535
GRID_FRAMES, GRID_W, GRID_H, GRID_ROWS, GRID_COLS = GRID_CHUNK + 2, 4, 3, 2, 2
GRID_KS = (3, 9)                    # the 5- and the 16-cluster instantiation


def grid_labels(k, seed=0):
    return np.random.default_rng(seed + k).integers(0, k, (GRID_FRAMES, GRID_H, GRID_W)).astype(np.uint8)


def grid_flow(seed=77):
    return (np.random.default_rng(seed).standard_normal((GRID_FRAMES, GRID_H, GRID_W, 2)) * 3).astype(np.float32)


def counts_all_frames(labels, k, rows, cols, flow=None, absolute=False):
    """motion_grid_cases.model_counts over every frame at once: one-hot labels summed over each cell's pixels.  A cell
    here has so few pixels that the f64 sum of their f32 values in any order is exact, as math.fsum's is (the host test
    compares the two on the frames either side of the chunk)"""
    labels = np.asarray(labels, np.uint8)
    n, H, W = labels.shape
    ys, xs = H // rows, W // cols
    assert ys * xs <= 4
    lab = labels[:, :rows * ys, :cols * xs].reshape(n, rows, ys, cols, xs).transpose(0, 1, 3, 2, 4).reshape(n, rows * cols, ys * xs)
    hot = lab[..., None] == np.arange(k, dtype=np.uint8)                               # (n, cells, px, k)
    counts = hot.sum(axis=2).astype(np.int32)
    if flow is None:
        return counts
    fl = np.asarray(flow, np.float64)
    if absolute:
        fl = np.abs(fl)
    fl = fl[:, :rows * ys, :cols * xs].reshape(n, rows, ys, cols, xs, 2).transpose(0, 1, 3, 2, 4, 5).reshape(n, rows * cols, ys * xs, 2)
    sums = np.zeros((n, rows * cols, k, 2))
    for p in range(ys * xs):                                                           # at most 4 terms, added in pixel order
        sums += np.where(hot[:, :, p, :, None], fl[:, :, p, None, :], 0.0)
    return counts, sums
