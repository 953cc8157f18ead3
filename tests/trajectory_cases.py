"""The trajectories of include/ofc.h twice over -- a numpy reference vectorised over the points and an independent per-point
loop in plain Python integers that shares nothing with it -- and the table of cases that test_trajectory_host.py proves on
the CPU and test_gpu_trajectories.py runs on the device."""
import math

import numpy as np

from tests import consistency_cases as CC

RAN, UNTRUSTED, LEAVES, INVALID = 0, 1, 2, 3
ONE = 65536
Q = 1.0 / ONE                     # one quantum in px
ALMOST = CC.ALMOST
SPECIALS = CC.SPECIALS            # nan, inf, -inf, 1024, -1024 (not vectors) and 1023.99994 (the largest valid one)
THREADS = 256                     # OFC_TRAJ_THREADS
ONE_LAUNCH_POINTS, DENSE_PAIRS = 1 << 19, 16      # OFC_TRAJ_ONE_LAUNCH_POINTS, OFC_TRAJ_DENSE_PAIRS


def keep_mask(states):
    if isinstance(states, (int, np.integer)):
        return int(states)
    k = 0
    for s in states:
        k |= 1 << int(s)
    return k


# ---- the reference: numpy, all points at a time ----
def _quantise(f):
    f = np.asarray(f, np.float32)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(f).all(-1) & (np.abs(f) < np.float32(1024)).all(-1)
        q = np.rint(np.where(valid[..., None], f, np.float32(0)).astype(np.float64) * 65536.0).astype(np.int64)
    return valid, q


def reference(flow, seeds, state=None, keep=1):
    """(n,H,W,2) f32, (P,2) int32, (n,H,W) u8 or None, the set keep -> pos (n+1,P,2) int32, len (P,) int32, why (P,) u8"""
    n, H, W = flow.shape[:3]
    P = len(seeds)
    xmax, ymax = (W - 1) << 16, (H - 1) << 16
    X, Y = seeds[:, 0].astype(np.int64), seeds[:, 1].astype(np.int64)
    live, length, why = np.ones(P, bool), np.zeros(P, np.int32), np.zeros(P, np.uint8)
    pos = np.empty((n + 1, P, 2), np.int32)
    pos[0] = seeds
    for t in range(n):
        valid, q = _quantise(flow[t])
        inside = (X >= 0) & (X <= xmax) & (Y >= 0) & (Y <= ymax)
        Xc, Yc = np.clip(X, 0, xmax), np.clip(Y, 0, ymax)                 # only indexes; an inside point is unchanged
        trusted = np.ones(P, bool)
        if state is not None:
            s = state[t][(Yc + 32768) >> 16, (Xc + 32768) >> 16].astype(np.int64)
            trusted = (s <= 3) & (((np.int64(keep) >> np.minimum(s, 16)) & 1) == 1)
        ix, iy, fx, fy = Xc >> 16, Yc >> 16, Xc & 65535, Yc & 65535
        ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
        S, ok = np.zeros((P, 2), np.int64), np.ones(P, bool)
        for tx, ty, w in ((ix, iy, (ONE - fx) * (ONE - fy)), (ix1, iy, fx * (ONE - fy)), (ix, iy1, (ONE - fx) * fy), (ix1, iy1, fx * fy)):
            S += w[:, None] * q[ty, tx]
            ok &= valid[ty, tx]
        D = (S + (1 << 31)) >> 32
        Xn, Yn = Xc + D[:, 0], Yc + D[:, 1]
        lands = (Xn >= 0) & (Xn <= xmax) & (Yn >= 0) & (Yn <= ymax)
        reason = np.select([~inside, ~trusted, ~ok, ~lands], [LEAVES, UNTRUSTED, INVALID, LEAVES], RAN)
        step = live & (reason == RAN)
        why[live & ~step] = reason[live & ~step]
        X, Y = np.where(step, Xn, X), np.where(step, Yn, Y)
        length += step
        live = step
        pos[t + 1, :, 0], pos[t + 1, :, 1] = X, Y
    return pos, length, why


# ---- the same definition as a loop over the points in Python integers.  Shares nothing with the numpy above. ----
def _q(u):
    u = float(u)
    if not math.isfinite(u) or not abs(u) < 1024.0:
        return None
    return int(round(u * 65536.0))              # exact product; round() goes to even on ties, as llrint does


def _qvec(vec):
    a, b = _q(vec[0]), _q(vec[1])
    return None if a is None or b is None else (a, b)


def loop(flow, seeds, state=None, keep=1, bounds=None):
    """the same outputs; `bounds`, a dict, takes the largest |S|, |D| and coordinate met"""
    n, H, W = flow.shape[:3]
    f = flow.tolist()
    st = state.tolist() if state is not None else None
    xmax, ymax = (W - 1) * 65536, (H - 1) * 65536
    pos = [[None] * len(seeds) for _ in range(n + 1)]
    length, why = [], []
    big = dict(S=0, D=0, X=0)
    for p, (X, Y) in enumerate(seeds.tolist()):
        steps, reason = 0, RAN
        pos[0][p] = (X, Y)
        for t in range(n):
            if reason == RAN:
                reason = _step_reason(f[t], st[t] if st else None, keep, X, Y, W, H, xmax, ymax, big)
                if isinstance(reason, tuple):
                    X, Y = reason
                    reason = RAN
                    steps += 1
            pos[t + 1][p] = (X, Y)
        length.append(steps)
        why.append(reason)
    if bounds is not None:
        bounds.update(big)
    return np.array(pos, np.int32).reshape(n + 1, len(seeds), 2), np.array(length, np.int32), np.array(why, np.uint8)


def _step_reason(f, st, keep, X, Y, W, H, xmax, ymax, big):
    """-> the new (X, Y), or why the point ends"""
    if not (0 <= X <= xmax and 0 <= Y <= ymax):
        return LEAVES
    if st is not None:
        s = st[(Y + 32768) // 65536][(X + 32768) // 65536]
        if s > 3 or not (keep >> s) & 1:
            return UNTRUSTED
    ix, fx, iy, fy = X // 65536, X % 65536, Y // 65536, Y % 65536
    ix1, iy1 = min(ix + 1, W - 1), min(iy + 1, H - 1)
    taps = [_qvec(f[iy][ix]), _qvec(f[iy][ix1]), _qvec(f[iy1][ix]), _qvec(f[iy1][ix1])]
    if any(t is None for t in taps):
        return INVALID
    wts = [(65536 - fx) * (65536 - fy), fx * (65536 - fy), (65536 - fx) * fy, fx * fy]
    assert sum(wts) == 2 ** 32
    S = [sum(w * t[c] for w, t in zip(wts, taps)) for c in (0, 1)]
    D = [(s + 2 ** 31) // 2 ** 32 for s in S]                     # floor division: the arithmetic shift
    Xn, Yn = X + D[0], Y + D[1]
    big["S"], big["D"], big["X"] = max(big["S"], abs(S[0]), abs(S[1])), max(big["D"], abs(D[0]), abs(D[1])), max(big["X"], abs(Xn), abs(Yn))
    if not (0 <= Xn <= xmax and 0 <= Yn <= ymax):
        return LEAVES
    return (Xn, Yn)


# ---- the cases ----
class Case:
    def __init__(self, name, flow, seeds, state=None, keep=(0,), marks=None):
        self.name, self.keep = name, keep_mask(keep)
        self.flow = np.ascontiguousarray(flow, np.float32)
        self.seeds = np.ascontiguousarray(seeds, np.int32)
        self.state = None if state is None else np.ascontiguousarray(state, np.uint8)
        assert self.flow.ndim == 4 and self.flow.shape[3] == 2 and self.seeds.ndim == 2 and self.seeds.shape[1] == 2
        assert self.state is None or self.state.shape == self.flow.shape[:3]
        for a in (self.flow, self.seeds) + (() if self.state is None else (self.state,)):
            a.setflags(write=False)
        self.marks = marks or {}                  # named points (indices into seeds) the host test asks about
        self._ref = None

    def __repr__(self):
        return self.name

    @property
    def shape(self):
        return self.flow.shape[:3]

    def reference(self):
        if self._ref is None:                     # computed once, shared, never written
            self._ref = reference(self.flow, self.seeds, self.state, self.keep)
            for a in self._ref:
                a.setflags(write=False)
        return self._ref


def spread_seeds(W, H, seed, extra=64):
    """every half pixel of the frame, then `extra` random points of which some lie outside it"""
    r = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:2 * H - 1, 0:2 * W - 1]
    grid = np.stack([xs.ravel() * 32768, ys.ravel() * 32768], 1)
    rnd = np.stack([r.integers(-ONE, W * ONE, extra), r.integers(-ONE, H * ONE, extra)], 1)
    return np.concatenate([grid, rnd]).astype(np.int32)


def _smooth(n, H, W, seed=11, specials=True):
    """consistency_cases' fields with its own state map: (flow, state)"""
    fwd, bwd = CC.smooth_fields(seed, n, H, W, specials)
    return fwd, CC.reference(fwd, bwd)[0]


KEEPS = ((0,), (0, 1), (0, 1, 2), (0, 1, 2, 3), 0)
SMOOTH = ((7, 13, 17), (5, 48, 64))               # n, H, W: all four reasons and every length occur on both


def _smooth_cases():
    out = []
    for n, H, W in SMOOTH:
        flow, state = _smooth(n, H, W)
        seeds = spread_seeds(W, H, 3)
        out.append(Case(f"smooth-{W}x{H}-n{n}", flow, seeds))
        for keep in KEEPS if (W, H) == (17, 13) else KEEPS[:1]:
            tag = "none" if keep == 0 else "".join(str(s) for s in keep)
            out.append(Case(f"smooth-{W}x{H}-n{n}-keep-{tag}", flow, seeds, state, keep))
    return out


def _degenerate_cases():
    """frames of one pixel in a direction: the component along that side is exactly 0, so that points survive"""
    out = []
    for (W, H), n in (((1, 1), 1), ((1, 9), 2), ((9, 1), 9), ((2, 2), 7)):
        flow, state = _smooth(n, H, W, seed=21, specials=(W, H) != (2, 2))       # in 2x2 one unusable value ends every point
        flow = flow.copy()
        flow[np.isfinite(flow) & (np.abs(flow) < 1024)] *= np.float32(0.125)
        if W == 1:
            flow[..., 0] = 0
        if H == 1:
            flow[..., 1] = 0
        seeds = spread_seeds(W, H, 5, extra=16)
        out.append(Case(f"degenerate-{W}x{H}-n{n}", flow, seeds))
        out.append(Case(f"degenerate-{W}x{H}-n{n}-state", flow, seeds, state, (0, 1)))
    return out


EDGE_W, EDGE_H, EDGE_N = 12, 10, 3


def _edge_case():
    """hand-made: a field that is zero but for the vectors named below, a state map that is 0 but for the bytes named below"""
    W, H, n = EDGE_W, EDGE_H, EDGE_N
    xmax, ymax = (W - 1) << 16, (H - 1) << 16
    flow, state = np.zeros((n, H, W, 2), np.float32), np.zeros((n, H, W), np.uint8)
    seeds, marks = [], {}

    def seed(name, X, Y):
        marks[name] = len(seeds)
        seeds.append((X, Y))

    def put(t, y, x, u, v):
        flow[t, y, x] = (u, v)
        assert float(flow[t, y, x, 0]) == u and float(flow[t, y, x, 1]) == v       # representable: the quantum is not lost
    seed("seed-outside-left", -1, 3 << 16)
    seed("seed-outside-right", xmax + 1, 3 << 16)
    seed("seed-outside-top", 3 << 16, -1)
    seed("seed-outside-bottom", 3 << 16, ymax + 1)
    seed("seed-int32-min", -2 ** 31, 2 ** 31 - 1)
    seed("seed-corner", xmax, ymax)                                     # both "+1" taps are clamped and have weight 0
    put(0, 0, 3, W - 1 - 3, 0.0)
    seed("onto-border", 3 << 16, 0)                                     # lands exactly on the last column, then rests there
    put(0, 0, 4, W - 1 - 4 + Q, 0.0)
    seed("past-border", 4 << 16, 0)                                     # one quantum past it: ends at step 0 and does not move
    put(0, 1, 3, -3.0, 0.0)
    seed("onto-column-0", 3 << 16, 1 << 16)
    put(0, 1, 5, -5.0 - Q, 0.0)
    seed("before-column-0", 5 << 16, 1 << 16)
    put(n - 1, 2, 2, 0.0, -2.0 - Q)
    seed("ends-at-the-last-step", 2 << 16, 2 << 16)
    # the nearest-pixel seam of rule 2: state 1 at (6, 3) is not in keep = {0}
    state[:, 3, 6] = 1
    seed("seam-32767", (5 << 16) + 32767, 3 << 16)
    seed("seam-32768", (5 << 16) + 32768, 3 << 16)
    state[:, 4, 2], state[:, 4, 4], state[1, 4, 6] = 4, 255, 17
    seed("state-byte-4", 2 << 16, 4 << 16)
    seed("state-byte-255", 4 << 16, 4 << 16)
    seed("state-byte-17-at-step-1", 6 << 16, 4 << 16)
    # ties of (S + 2^31) >> 32 with negative S: fx = 1/2, taps -q and 0 give S = -q * 2^31
    put(0, 5, 1, -Q, 0.0)
    seed("tie-minus-half", (1 << 16) + 32768, 5 << 16)                 # S = -2^31: D = 0
    put(0, 5, 4, -3 * Q, 0.0)
    seed("tie-minus-three-halves", (4 << 16) + 32768, 5 << 16)         # S = -3 * 2^31: D = -1
    put(0, 6, 1, 0.0, 3 * Q)
    seed("tie-plus-three-halves", (1 << 16) + 32768, 6 << 16)          # S = 3 * 2^31: D = 2
    seed("all-four-valid", (8 << 16) + 12345, (7 << 16) + 54321)
    return Case("edges-12x10-n3", flow, np.array(seeds, np.int64).astype(np.int32), state, (0,), marks)


VALID_W, VALID_H = 40, 7


def _validity_case():
    """every special value in u or v of one pixel each, met as the tap of weight zero (the seed sits on the pixel to its left)
    and of weight 1/2 (the seed sits half a pixel to its left): an unusable tap ends the point whatever its weight; the
    largest valid vector moves it out of the frame only where it has weight"""
    W, H = VALID_W, VALID_H
    flow = np.zeros((1, H, W, 2), np.float32)
    seeds, marks = [], {}
    for j, s in enumerate(SPECIALS):
        x, y, c = 3 + 6 * j, 3, j % 2
        flow[0, y, x, c] = s
        marks[f"special-{j}-weight-0"] = len(seeds)
        seeds.append(((x - 1) << 16, y << 16))
        marks[f"special-{j}-weight-half"] = len(seeds)
        seeds.append((((x - 1) << 16) + 32768, y << 16))
        marks[f"special-{j}-below-weight-0"] = len(seeds)
        seeds.append((x << 16, (y - 1) << 16))
    return Case("validity-40x7-n1", flow, np.array(seeds, np.int32), marks=marks)


def _many_points_case():
    """more points than the device holds lanes at once: 600 000 random seeds, a few of them outside"""
    n, H, W = 3, 48, 64
    flow, state = _smooth(n, H, W)
    r = np.random.default_rng(9)
    P = 600_000
    seeds = np.stack([r.integers(-2048, W * ONE - ONE + 2048, P), r.integers(-2048, H * ONE - ONE + 2048, P)], 1).astype(np.int32)
    return Case("many-600000-64x48-n3", flow, seeds, state, (0, 1))


CASES = _smooth_cases() + _degenerate_cases() + [_edge_case(), _validity_case()]
MANY = _many_points_case
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
POINT_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)


def chunks(n):
    """the pairs_per_launch every case runs at: automatic, 1, 2, one short of all, all, more than all"""
    return sorted({0, 1, 2, max(n - 1, 1), n, n + 5})


def geometry(npair, P):
    """what ofc_traj_launch_geometry documents: pairs per launch, work-groups per launch, launches, lanes per work-group"""
    chunk = npair if P <= ONE_LAUNCH_POINTS else min(npair, DENSE_PAIRS)
    return chunk, -(-P // THREADS), -(-npair // chunk), THREADS
