"""Shared by test_oracle_lloyd_tiles.py and test_gpu_lloyd_tile_patterns.py: the fields that drive csrc/lloyd_tiles.hip
through every walk pattern, mode switch, k and edge input, each with its seed, and a float64 numpy model of what the
tile sweeps decide -- the box test of TileCtx::box_label and the mode rules of k_lloyd_update.

The model cannot reproduce the device's last bits (no FMA in numpy, another order for the mean), so it is only asked
about tiles whose verdict does not depend on them: a tile is BORDERLINE when its verdict changes for some margin factor
in [1e-13, 1e-11] around the kernel's 1e-12, and every case must have none (asserted by the CPU module).  The verdict is
then the same for any rounding of the ~1e-15 kind, and the device's counts must equal the model's exactly.
"""
import functools

import numpy as np

from oracle import oracle as O

TILE = 64
FULL, PRUNED, PROBE = 0, 1, 2          # LLOYD_TILES_* (lloyd_common.h), the numbers the trace line prints
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the model
def tile_boxes(X):
    """boxes of the full 64-sample tiles of a float32 (N, 2) field -> lo (NT, 2), hi (NT, 2) as float64"""
    assert X.dtype == np.float32 and X.ndim == 2 and X.shape[1] == 2
    NT = len(X) // TILE
    T = X[: NT * TILE].reshape(NT, TILE, 2)
    return T.min(1).astype(np.float64), T.max(1).astype(np.float64)


def box_verdict(lo, hi, mean, cc, factor=1e-12):
    """TileCtx::box_label for every tile: cc are the CENTRED centres (k, 2).  -> candidate label (NT,), pure (NT,) bool"""
    cc = np.asarray(cc, np.float64)
    lo, hi = lo - mean, hi - mean
    cn = (cc * cc).sum(1)
    D = cn[None, :] - 2.0 * (lo[:, 1:2] * cc[None, :, 1] + lo[:, 0:1] * cc[None, :, 0])
    j = np.argmin(D, axis=1)                                  # first minimum at the low corner: the candidate
    cj, cnj = cc[j], cn[j]
    ax, ay = np.maximum(np.abs(lo[:, 0]), np.abs(hi[:, 0])), np.maximum(np.abs(lo[:, 1]), np.abs(hi[:, 1]))
    pure = np.ones(len(lo), bool)
    for q in range(len(cc)):
        gx, gy = cc[q, 0] - cj[:, 0], cc[q, 1] - cj[:, 1]
        wmax = (cnj - cn[q]) + 2.0 * (np.maximum(lo[:, 0] * gx, hi[:, 0] * gx) + np.maximum(lo[:, 1] * gy, hi[:, 1] * gy))
        mag = (np.abs(cnj) + abs(cn[q])) + 4.0 * (ax * (abs(cc[q, 0]) + np.abs(cj[:, 0])) + ay * (abs(cc[q, 1]) + np.abs(cj[:, 1])))
        pure &= (j == q) | (wmax < -factor * mag)
    return j, pure


def tile_report(X, mean, cc):
    """-> (pure mask at the kernel's margin, number of borderline tiles)"""
    lo, hi = tile_boxes(X)
    pure = box_verdict(lo, hi, mean, cc)[1]
    loose, tight = box_verdict(lo, hi, mean, cc, 1e-13)[1], box_verdict(lo, hi, mean, cc, 1e-11)[1]
    return pure, int(((loose != tight) | (loose != pure)).sum())


def argmin_gap_ok(X, mean, cc, tied=None):
    """the condition of test_oracle_lloyd_independent.py on every sample outside `tied`: its two smallest squared distances
    differ by at least 2 max(B_j1, B_j2), B = (d + 4) u (|x|^2 + |c|^2 + 2 sum |x_f c_f|).  The gap is evaluated in float64,
    itself within B of the exact one, hence the factor 3 here.  -> (all ok, smallest gap / bound)"""
    cc = np.asarray(cc, np.float64)
    if len(cc) < 2:
        return True, np.inf
    x = X.astype(np.float64) - mean
    if tied is not None:
        x = x[~tied]
    d2 = ((x[:, None, :] - cc[None]) ** 2).sum(2)
    B = 6 * U * ((x * x).sum(1)[:, None] + (cc * cc).sum(1)[None] + 2 * (np.abs(x)[:, None, :] * np.abs(cc)[None]).sum(2))
    o = np.argsort(d2, axis=1, kind="stable")[:, :2]
    r = np.arange(len(x))
    gap = d2[r, o[:, 1]] - d2[r, o[:, 0]]
    bound = 3 * np.maximum(B[r, o[:, 0]], B[r, o[:, 1]])
    ratio = float((gap / bound).min()) if len(x) else np.inf
    return ratio >= 1.0, ratio


def replay(policy, pure, NT):
    """the rules of k_tile_decide and k_lloyd_update (cool-down 6, doubling) on the model's pure counts per iteration
    (pure[0] is also what the probe before iteration 0 sees: it tests every tile of a field this small).
    -> modes per sweep, final_pruned, and the (share, threshold) pairs that fed a decision"""
    mode = PRUNED if policy == 3 or pure[0] >= 0.45 * NT else FULL
    off = mode == FULL
    fed = [] if policy == 3 else [(pure[0] / NT, 0.45)]
    cooldown = backoff = 6
    modes = []
    for p in pure:
        modes.append(mode)
        frac = p / NT
        if policy == 3:
            continue
        if mode == PRUNED:
            fed.append((frac, 0.30))
            if frac < 0.3:
                mode, cooldown, backoff = FULL, backoff, backoff * 2
        elif mode == PROBE:
            fed.append((frac, 0.45))
            mode, cooldown, backoff = (PRUNED if frac >= 0.45 else FULL), backoff, backoff * 2
        elif not off:
            cooldown -= 1
            if cooldown <= 0:
                mode = PROBE
    return modes, mode == PRUNED, fed


class Plan:
    """what one policy makes of a case's pure counts"""

    def __init__(self, ex, policy):
        self.ex = ex
        self.modes, self.final_pruned, self.fed = replay(policy, ex.pure, ex.NT)
        self.pruned_sweeps, self.probe_sweeps = self.modes.count(PRUNED), self.modes.count(PROBE)

    def trace(self, world=1):
        """(tiles_mode, tested, pure) per iteration, as OFC_LLOYD_TRACE prints them"""
        return [(m, self.ex.NT * world if m != FULL else 0, p * world if m != FULL else 0)
                for m, p in zip(self.modes, self.ex.pure)]

    def margins_ok(self):
        return all(abs(s - t) >= 0.05 for s, t in self.fed)

    def letters(self):
        return "".join("FPB"[m] for m in self.modes)


@functools.lru_cache(maxsize=None)
def _cut_fit(base, max_iter):
    """the oracle's fit of a field cut after max_iter iterations (shared by the cases that are prefixes of one fit)"""
    X, C0 = field(base)
    return O.kmeans_fit(X, C0, max_iter, CASES[base].get("tol", 1e-4))


@functools.lru_cache(maxsize=None)
def _report(base, i):
    """tile_report against the centres sweep i labels: the initial ones, or the fit cut after i iterations"""
    X, C0 = field(base)
    mean = X.astype(np.float64).mean(0)
    return tile_report(X, mean, (np.asarray(C0, np.float64) if i == 0 else _cut_fit(base, i)[0]) - mean)


class Expect:
    """the oracle's fit of a case and what the model says of every sweep"""

    def __init__(self, name):
        c = CASES[name]
        base = c.get("base", name)
        self.X, self.C0 = field(base)
        self.cen, self.lab, self.inertia, self.n_iter = _cut_fit(base, c.get("max_iter", 300))
        self.mean = self.X.astype(np.float64).mean(0)
        self.NT = len(self.X) // TILE
        # the centres sweep i labels against: the fit cut after i iterations; the final E-step: after n_iter
        self.centres = [np.asarray(self.C0, np.float64)] + [_cut_fit(base, i)[0] for i in range(1, self.n_iter)]
        rep = [_report(base, i) for i in range(self.n_iter + 1)]
        self.pure_masks = [r[0] for r in rep[:-1]]
        self.pure = [int(r[0].sum()) for r in rep[:-1]]
        self.final_pure = int(rep[-1][0].sum())
        self.borderline = sum(r[1] for r in rep)
        self.plans = {}

    def plan(self, policy):
        if policy not in self.plans:
            self.plans[policy] = Plan(self, policy)
        return self.plans[policy]


@functools.lru_cache(maxsize=None)
def expect(name):
    return Expect(name)


@functools.lru_cache(maxsize=None)
def field(name):
    c = CASES[name]
    X, C0 = c["build"](**c["args"])
    X.setflags(write=False)
    return X, C0


# ------------------------------------------------------------------------------------------------ A. walk patterns
REJECTED_COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
PLACEMENTS = ("first", "last", "alternating", "random")
MINORITY = (1, 63, 2, 32, 17, 5, 62, 31)      # samples of population 0 in a rejected tile; 1/63 and 63/1 come first


def rejected_lanes(count, placement, rng):
    if placement == "first":
        return np.arange(count)
    if placement == "last":
        return np.arange(64 - count, 64)
    if placement == "alternating":      # every other lane rejected (or, past 32, every other lane pure)
        return np.arange(0, 2 * count, 2) if count <= 32 else np.setdiff1d(np.arange(64), np.arange(1, 2 * (64 - count), 2))
    return np.sort(rng.permutation(64)[:count])


def walk_field(placement, reverse, extra_tiles, extra_samples, seed):
    """k = 2, populations at (-1, 0) and (+1, 0), noise 0.05.  One group of 64 tiles per rejected count; a pure tile holds one
    population, a rejected one both.  -> X, C0, rejected mask per tile"""
    rng = np.random.default_rng(seed)
    groups = []
    for count in (REJECTED_COUNTS[::-1] if reverse else REJECTED_COUNTS):
        g = np.zeros(64, bool)
        g[rejected_lanes(count, placement, rng)] = True
        groups.append(g)
    tail = np.zeros(extra_tiles, bool)
    tail[::-2] = True                   # the field's last tile is a rejected one
    rej = np.concatenate(groups + [tail])
    NT = len(rej)
    N = NT * TILE + extra_samples
    pop = np.empty(N, np.int64)
    pop[: NT * TILE] = np.repeat(rng.integers(0, 2, NT), TILE)
    for n, t in enumerate(np.flatnonzero(rej)):
        s = np.ones(TILE, np.int64)
        s[rng.permutation(TILE)[: MINORITY[n % len(MINORITY)]]] = 0
        pop[t * TILE: (t + 1) * TILE] = s
    pop[NT * TILE:] = rng.integers(0, 2, extra_samples)
    X = (np.array([[-1.0, 0.0], [1.0, 0.0]])[pop] + 0.05 * rng.standard_normal((N, 2))).astype(np.float32)
    return X, np.array([[-0.9, 0.1], [1.1, -0.05]]), rej


def _walk(**kw):
    return walk_field(**kw)[:2]


# placement, reversed, tiles behind the last whole group (mod 64 in {1, 63, 2, 0}: mod 4 in {1, 3, 2, 0}), samples behind the
# last tile (N mod 64 in {0, 1, 63})
WALKS = [("first", False, 1, 0), ("first", True, 63, 63), ("last", False, 2, 1), ("last", True, 1, 63),
         ("alternating", False, 63, 1), ("alternating", True, 0, 0), ("random", False, 63, 0), ("random", True, 2, 63)]


# ------------------------------------------------------------------------------------------------ B. mode switches
def rotating_field(NT, horizontal, vertical, v_range, u_range, eps, seed, point_noise=0.01):
    """tiles of three kinds, shuffled: horizontal segments (u uniform on [-1, 1] at one v), vertical segments (v uniform on
    [-v_range, v_range] at one u in [-u_range, u_range]) and points.  The initial centres (-+eps, -+0.3) cut the field
    along v = 0, where the horizontal segments and the points are pure; the longer axis is u, so Lloyd turns the cut
    through the diagonal (almost every segment straddles it) to u = 0, where the vertical segments and the points are."""
    rng = np.random.default_rng(seed)
    nh, nv = int(horizontal * NT), int(vertical * NT)
    kinds = rng.permutation(np.r_[np.zeros(nh), np.ones(nv), 2 * np.ones(NT - nh - nv)]).astype(int)
    X = np.empty((NT, TILE, 2))
    for t, kind in enumerate(kinds):
        if kind == 0:
            X[t, :, 0], X[t, :, 1] = rng.uniform(-1, 1, TILE), rng.uniform(-v_range, v_range)
        elif kind == 1:
            X[t, :, 0], X[t, :, 1] = rng.uniform(-u_range, u_range), rng.uniform(-v_range, v_range, TILE)
        else:
            X[t] = np.r_[rng.uniform(-1, 1), rng.uniform(-v_range, v_range)] + point_noise * rng.standard_normal((TILE, 2))
    return X.reshape(-1, 2).astype(np.float32), np.array([[-eps, -0.3], [eps, 0.3]])


RECOVER = dict(NT=2048, horizontal=0.48, vertical=0.44, v_range=0.5, u_range=0.5, eps=0.002, seed=1)
STAY_FULL = dict(NT=4096, horizontal=0.7, vertical=0.15, v_range=0.66, u_range=0.6, eps=0.01, seed=0, point_noise=0.3)


# ------------------------------------------------------------------------------------------------ C. every k
def coherent_k(k, N, seed, centre=(0.0, 0.0), radius=4.0, noise=0.05, run=700):
    """k populations on a circle, long runs of consecutive samples in one population (a flow field's rows)"""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * (np.arange(k) + 0.25) / k
    vel = np.asarray(centre) + radius * np.stack([np.cos(ang), np.sin(ang)], 1) * (k > 1)
    runs = np.r_[rng.permutation(k), rng.integers(0, k, N // run + 2)]      # every population is there
    pop = np.repeat(runs, run)[:N]
    X = (vel[pop] + noise * rng.standard_normal((N, 2))).astype(np.float32)
    return X, vel + 0.3 * radius / 4.0 * rng.uniform(-1, 1, vel.shape)


# ------------------------------------------------------------------------------------------------ D. edge inputs
def tie_field(n0, seed):
    """integer coordinates, mean exactly (0, 0), centres (-4, 0) and (4, 0) that the first M-step reproduces exactly: n0
    tiles at u = -8, 2 n0 tiles at u = 4 and n0 tiles ON u = 0, every sample of which is exactly equidistant from both
    centres (label 0, the first minimum) -- at iteration 0 and, the centres being a fixed point, at the final E-step.
    Every tile's box has zero extent in u; v runs over -8..8 and sums to zero in every tile."""
    rng = np.random.default_rng(seed)
    u = rng.permutation(np.r_[np.full(n0, -8.0), np.full(2 * n0, 4.0), np.zeros(n0)])
    v = np.r_[np.arange(-8, 0), np.arange(1, 9)].repeat(4).astype(np.float64)
    X = np.stack([np.repeat(u, TILE), np.concatenate([rng.permutation(v) for _ in u])], 1).astype(np.float32)
    return X, np.array([[-4.0, 0.0], [4.0, 0.0]])


def tied_tiles(X):
    return X[::TILE, 0] == 0.0


def constant_field(N, k):
    X = np.tile(np.array([[3.5, -1.25]], np.float32), (N, 1))
    return X, np.array([[3.5, -1.25], [4.0, 0.0]])[:k]


def offset_field(N, seed):
    """three populations 0.25 apart around (1e4, -1e4) (float32 spacing there: 9.8e-4), spread 1e-2"""
    return coherent_k(3, N, seed, centre=(1e4, -1e4), radius=0.25, noise=1e-2)


# ------------------------------------------------------------------------------------------------ the table
CASES = {}
for _i, (_p, _r, _t, _s) in enumerate(WALKS):
    CASES["walk-%s-%s-t%d-s%d" % (_p, "rev" if _r else "fwd", _t, _s)] = dict(
        family="walk", build=_walk, args=dict(placement=_p, reverse=_r, extra_tiles=_t, extra_samples=_s, seed=100 + _i))
CASES["switch-recover"] = dict(family="switch", build=rotating_field, args=RECOVER, tol=0.0)
# the same fit cut by max_iter inside its FULL stretch, on its PROBE and inside the PRUNED stretch behind it
CASES["switch-recover-cut-full"] = dict(family="switch", base="switch-recover", tol=0.0, max_iter=15)
CASES["switch-recover-cut-probe"] = dict(family="switch", base="switch-recover", tol=0.0, max_iter=19)
CASES["switch-recover-cut-pruned"] = dict(family="switch", base="switch-recover", tol=0.0, max_iter=22)
CASES["switch-stay-full"] = dict(family="switch", build=rotating_field, args=STAY_FULL, tol=0.0)
for _k in range(1, 9):
    CASES["k%d" % _k] = dict(family="k", build=coherent_k, args=dict(k=_k, N=64 * 600 + 37, seed=200 + _k))
CASES["tie"] = dict(family="edge", build=tie_field, args=dict(n0=40, seed=300))
CASES["const-k1"] = dict(family="edge", build=constant_field, args=dict(N=64 * 40 + 5, k=1))
CASES["const-k2"] = dict(family="edge", build=constant_field, args=dict(N=64 * 40 + 5, k=2))
CASES["offset1e4"] = dict(family="edge", build=offset_field, args=dict(N=64 * 300 + 21, seed=301))

WALK_CASES = [n for n in CASES if CASES[n]["family"] == "walk"]
SWITCH_CASES = [n for n in CASES if CASES[n]["family"] == "switch"]
K_CASES = [n for n in CASES if CASES[n]["family"] == "k"]
EDGE_CASES = [n for n in CASES if CASES[n]["family"] == "edge"]


def walk_rejected(name):
    return walk_field(**CASES[name]["args"])[2]


# the cases of lloyd_edge_goldens.npz the tile sweeps accept (f32, d = 2, k <= 8, N >= 64)
def golden_tile_cases(Z):
    names = sorted({k.split("/")[0] for k in Z.files if "/" in k})
    return [c for c in names if Z[c + "/X"].dtype == np.float32 and Z[c + "/X"].shape[1] == 2
            and len(Z[c + "/C0"]) <= 8 and len(Z[c + "/X"]) >= 64]


def nan_field(bad, seed=400):
    """a coherent k = 2 field with one non-finite sample in tile 17"""
    X, C0 = coherent_k(2, 64 * 64 + 5, seed)
    X = X.copy()
    X[17 * TILE + 29, 1] = bad
    return X, C0
