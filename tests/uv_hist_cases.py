"""The (u,v) histogram (include/ofc.h "Histogram of flow vectors", uv_hist.hip, uvhist.py): its numpy model, the fields and
the case tables of test_uv_hist_host.py (which proves the cases well-conditioned on the CPU) and test_gpu_uv_hist.py."""
import numpy as np

from opticalflowclustering_amd import _lib

SHARE, MAX_GRID = _lib.UV_HIST_SHARE, _lib.UV_HIST_MAX_GRID
PARAMS = ((16, 2.0 ** -4), (256, 8.0), (1024, 32.0), (2048, 1024.0))
SMALL_SIZES = (1, 63, 64, 65, 255, 257, 4099)
SHARE_SIZES = (SHARE - 1, SHARE, SHARE + 1)                       # either side of one work-group's share
GRID_SIZES = (SHARE * MAX_GRID - 1, SHARE * MAX_GRID, SHARE * MAX_GRID + 1)   # ... and of a whole grid's first round
PATTERNS = ("one-bin", "own-bin", "two-alternating", "63-and-1", "wave-boundary", "staggered", "uniform")


def table_len(bins):
    return 3 * bins * bins + 1


def model(flow, bins, rng, table=None):
    """the definition: f32 add, exact power-of-two scale, floor, np.add.at on int64.  -> a new table (added to `table`)"""
    f = np.ascontiguousarray(flow, np.float32).reshape(-1, 2)
    B, R, scale = int(bins), np.float32(rng), np.float32(bins / (2.0 * rng))
    with np.errstate(all="ignore"):
        t = (f + R) * scale
        ok = (t[:, 0] >= 0) & (t[:, 0] < B) & (t[:, 1] >= 0) & (t[:, 1] < B)
    idx = np.floor(t[ok, 1]).astype(np.int64) * B + np.floor(t[ok, 0]).astype(np.int64)
    q = np.rint(f[ok].astype(np.float64) * 65536.0).astype(np.int64)
    tab = np.zeros(table_len(B), np.int64) if table is None else np.array(table, np.int64)
    np.add.at(tab, idx, 1)
    np.add.at(tab, B * B + idx, q[:, 0])
    np.add.at(tab, 2 * B * B + idx, q[:, 1])
    tab[-1] += np.count_nonzero(~ok)
    return tab


def bin_of(flow, bins, rng):
    """bin index per vector, -1 outside (the model's arithmetic)"""
    f = np.ascontiguousarray(flow, np.float32).reshape(-1, 2)
    B, R, scale = int(bins), np.float32(rng), np.float32(bins / (2.0 * rng))
    with np.errstate(all="ignore"):
        t = (f + R) * scale
        ok = (t[:, 0] >= 0) & (t[:, 0] < B) & (t[:, 1] >= 0) & (t[:, 1] < B)
    out = np.full(len(f), -1, np.int64)
    out[ok] = np.floor(t[ok, 1]).astype(np.int64) * B + np.floor(t[ok, 0]).astype(np.int64)
    return out


def bin_value(iu, iv, bins, rng, frac=0.5):
    """(n,2) f32: the point `frac` of a bin width above the lower edge of bin (iu, iv) on both axes; exact in f32 for
    dyadic frac (edges and widths are powers of two times integers)"""
    w = 2.0 * rng / bins
    u = -rng + (np.asarray(iu, np.float64) + frac) * w
    v = -rng + (np.asarray(iv, np.float64) + frac) * w
    return np.stack(np.broadcast_arrays(u, v), -1).astype(np.float32)


def pattern(name, n, bins, rng, seed=0):
    """(n,2) f32 in range, laid out against the kernel's waves of 64 consecutive vectors.  Values move inside their bins
    (eighths of a width) and every pattern has bins below zero, so sums are not multiples of one value and go negative."""
    r = np.random.default_rng(seed)
    i = np.arange(n)
    frac = (r.integers(0, 8, n) + 0.5) / 8.0
    B = bins
    if name == "one-bin":                                   # the contention path: every lane of every wave
        iu, iv = np.full(n, B // 2 - 3), np.full(n, B // 4 + 1)
    elif name == "own-bin":                                 # 64 distinct bins per wave, 4096 before one repeats
        j = i % min(B * B, 4096)
        iu, iv = j % B, (j // B + 3 * (j % B)) % B
    elif name == "two-alternating":
        iu, iv = np.where(i & 1, B - 1, 0), np.where(i & 1, 0, B - 1)
    elif name == "63-and-1":                                # lane 17 of every wave elsewhere
        odd = (i % 64) == 17
        iu, iv = np.where(odd, 5, B // 2), np.where(odd, B - 2, B // 2)
    elif name == "wave-boundary":                           # a new bin for every wave of 64, 37 of them in turn
        w = (i // 64) % 37
        iu, iv = (B // 2 + w) % B, (B // 2 - w) % B
    elif name == "staggered":                               # lane l changes bin every 1 + l % 4 waves, five bins in turn:
        w = ((i // 64) // (1 + (i % 64) % 4)) % 5           # lanes that share a bin are at different points of their runs
        iu, iv = B // 2 - 2 + w, B // 2 + 1 - w
    elif name == "uniform":
        iu, iv = r.integers(0, B, n), r.integers(0, B, n)
    else:
        raise KeyError(name)
    w = 2.0 * rng / B
    u = -rng + (iu + frac) * w
    v = -rng + (iv + frac[::-1]) * w
    return np.stack([u, v], -1).astype(np.float32)


def mixed_field(n, bins, rng, seed=1):
    """a cheap field for the large sizes: three compact clusters and a still background, 1 in 64 vectors outside"""
    r = np.random.default_rng(seed)
    which = r.integers(0, 4, n)
    cen = np.array([[0.0, 0.0], [0.31, -0.22], [-0.55, 0.4], [0.12, 0.62]]) * rng
    f = cen[which] + r.standard_normal((n, 2)) * (rng / 64.0)
    f[r.integers(0, 64, n) == 0] *= 40.0
    return f.astype(np.float32)


def special_values(bins, rng):
    """u values whose fate the arithmetic decides: the range's ends, zeros, denormals, non-finite, huge"""
    R = np.float32(rng)
    tiny = np.float32(1e-45)
    big = np.finfo(np.float32).max
    return np.array([-R, R, np.nextafter(R, np.float32(0)), np.nextafter(-R, np.float32(-np.inf)), 0.0, -0.0, tiny, -tiny,
                     np.float32(1.1e-38), np.nan, np.inf, -np.inf, big, -big, np.float32(0.75) * R, np.float32(-0.75) * R],
                    np.float32)


def edge_values(bins, rng):
    """every bin edge of a row, the value just below it and the value just above: 3 * (bins + 1) f32"""
    e = (-rng + np.arange(bins + 1) * (2.0 * rng / bins)).astype(np.float32)
    return np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))])


def in_one_axis(values, axis, other):
    """(n,2) f32 with `values` on one axis and the benign `other` on the other"""
    f = np.full((len(values), 2), other, np.float32)
    f[:, axis] = values
    return f


# ---- the fit: four well-separated blobs ----
FIT_BINS, FIT_RANGE, FIT_K, FIT_N = 256, 8.0, 4, 20000
BLOBS = np.array([[-3.0, -2.0], [2.5, 0.5], [0.0, 3.0], [4.0, -3.0]])
FIT_INIT = BLOBS + np.array([[0.3, -0.2], [-0.25, 0.3], [0.2, 0.2], [-0.3, -0.1]])
FIT_WIDTH = 2.0 * FIT_RANGE / FIT_BINS                         # 1/16 px


def lattice_field(seed=5):
    """(FIT_N,2) f32 on the lattice of bin centres: one distinct value per bin, so every bin mean is that value exactly.
    Blob b holds (b + 2) / 14 of the vectors, within +-8 bins of its centre."""
    r = np.random.default_rng(seed)
    which = r.choice(FIT_K, FIT_N, p=np.arange(2, 2 + FIT_K) / np.arange(2, 2 + FIT_K).sum())
    off = r.integers(-8, 9, (FIT_N, 2))
    base = np.floor((BLOBS + FIT_RANGE) / FIT_WIDTH).astype(np.int64)            # the bin of each blob centre
    ij = base[which] + off
    return bin_value(ij[:, 0], ij[:, 1], FIT_BINS, FIT_RANGE)


def off_lattice_field(seed=6):
    """the same blobs with continuous values: +-0.5 px around each centre, f32"""
    r = np.random.default_rng(seed)
    which = r.choice(FIT_K, FIT_N, p=np.arange(2, 2 + FIT_K) / np.arange(2, 2 + FIT_K).sum())
    return (BLOBS[which] + r.uniform(-0.5, 0.5, (FIT_N, 2))).astype(np.float32)


def lloyd(X, C0, w=None, max_iter=300):
    """plain float64 Lloyd to a fixed point (tol = 0): -> (centres, labels, n_iter), n_iter as sklearn counts it"""
    X, C = np.asarray(X, np.float64), np.array(C0, np.float64)
    w = np.ones(len(X)) if w is None else np.asarray(w, np.float64)
    lab = None
    for it in range(1, max_iter + 1):
        d = ((X[:, None, :] - C[None]) ** 2).sum(-1)
        new = d.argmin(1)
        if lab is not None and np.array_equal(new, lab):
            return C, lab, it
        lab = new
        C = np.stack([(X[lab == j] * w[lab == j, None]).sum(0) / w[lab == j].sum() for j in range(len(C))])
    return C, lab, max_iter


def boundary_margin(X, centres):
    """per vector: its distance to the nearest Voronoi boundary of `centres` (the bisector of its two nearest centres)"""
    X, C = np.asarray(X, np.float64), np.asarray(centres, np.float64)
    d2 = ((X[:, None, :] - C[None]) ** 2).sum(-1)
    order = np.argsort(d2, 1)
    a, b = order[:, 0], order[:, 1]
    gap = np.linalg.norm(C[a] - C[b], axis=1)
    return (d2[np.arange(len(X)), b] - d2[np.arange(len(X)), a]) / (2.0 * gap)


# ---- the stream: 64 x 48 frames, batch_pairs 2 ----
STREAM_W, STREAM_H, STREAM_BATCH, STREAM_GRID = 64, 48, 2, (2, 3)
STREAM_PARAMS = (256, 8.0)
STREAM_CENTRES = np.array([[0.0137, 0.0211], [0.5113, -0.2891], [1.0931, -0.4117]])


def stream_clip(n_frames=6):
    """(n, 48, 64) u8: a texture that steps by a different amount between every two frames"""
    from opticalflowclustering_amd import synth
    p = synth.texture_params(21)
    xs, ys = np.cumsum([0.0, 0.5, 0.8, 1.1, 0.3, 0.9]), np.cumsum([0.0, -0.3, -0.6, 0.2, -0.4, 0.1])
    return np.stack([synth.frame(STREAM_W, STREAM_H, xs[t], ys[t], p) for t in range(n_frames)]).astype(np.uint8)
