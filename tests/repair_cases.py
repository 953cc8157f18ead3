"""The repair of include/ofc.h (masked median fill, median smoothing) twice over -- a vectorised numpy model and a plain
per-pixel restatement in Python -- and the table of cases that test_repair_host.py proves on the CPU and test_gpu_repair.py
runs on the device.  Every case is laid out from ofc_repair_tile, so its holes sit on the seams of whatever tile the sweep
kernel takes."""
import ctypes as C
import functools
import math
import os

import numpy as np
import torch  # noqa: F401  (before libofc.so is loaded, as in test_consistency_host.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, MISMATCH, LEAVES, INVALID = 0, 1, 2, 3
UNFILLED = 255
BELOW = float(np.nextafter(np.float32(1024), np.float32(0)))      # the largest magnitude a valid component has
SPECIALS = (float("nan"), float("inf"), float("-inf"), 1024.0, -1024.0, 3.0e38)
QUANT = np.array([-1.5, -0.0, 0.0, 0.25, 2.0, 1e-40], np.float32)   # few values: heavy ties, both zeros, a denormal


def tile(radius):
    """(TX, TY) of the sweep kernel at this radius: ofc_repair_tile, host only"""
    from opticalflowclustering_amd import _lib
    out = (C.c_int * 2)()
    _lib.load().ofc_repair_tile(int(radius), C.byref(out))
    return int(out[0]), int(out[1])


# ---- the model: numpy, whole fields at a time ----
def valid(f):
    with np.errstate(invalid="ignore"):
        return np.isfinite(f).all(-1) & (np.abs(f) < np.float32(1024)).all(-1)


def sources(flow, state, keep):
    """V_0 of one pair or of a stack of pairs"""
    v = valid(flow)
    if state is not None:
        st = state.astype(np.int64)
        v &= (st < 4) & (((keep >> np.minimum(st, 4)) & 1) == 1)
    return v


def window(F, V, r):
    """(H,W,2) f32 and (H,W) bool -> the lower median over the window's pixels in V, (H,W,2) f32 (meaningless where the
    count is 0), and that count (H,W): pad with a sentinel, stack the shifted views, sort along the stack, take the index"""
    H, W = V.shape
    pad = np.full((H + 2 * r, W + 2 * r, 2), np.inf, np.float32)
    pad[r:r + H, r:r + W] = np.where(V[..., None], F, np.float32(np.inf))
    pv = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    pv[r:r + H, r:r + W] = V
    stack = np.stack([pad[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)])
    cnt = sum(pv[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1))
    stack = np.sort(stack, axis=0)                                   # the sentinels go last
    idx = np.broadcast_to((np.maximum(cnt, 1) - 1) // 2, (2, H, W)).transpose(1, 2, 0)[None]
    return np.take_along_axis(stack, idx, axis=0)[0], cnt


def model_pair(flow, state, keep, r, rounds, min_count, smooth):
    F = np.array(flow, np.float32)
    V = sources(F, state, keep)
    filled = np.where(V, 0, UNFILLED).astype(np.uint8)
    for g in range(1, rounds + 1):
        med, cnt = window(F, V, r)
        new = ~V & (cnt >= min_count)
        F[new] = med[new]
        filled[new] = g
        V = V | new
    if smooth:
        med, _ = window(F, V, r)
        F[V] = med[V]
    counts = np.array([(filled == 0).sum(), ((filled > 0) & (filled < UNFILLED)).sum(), (filled == UNFILLED).sum()], np.int64)
    st_out = None if state is None else np.where((filled > 0) & (filled < UNFILLED), OK, state).astype(np.uint8)
    return F, filled, counts, st_out


def model(flow, state, keep=1, r=1, rounds=8, min_count=1, smooth=False):
    """(n,H,W,2) f32, (n,H,W) u8 or None -> out (n,H,W,2) f32, filled (n,H,W) u8, counts (n,3) int64, state_out or None"""
    res = [model_pair(flow[t], None if state is None else state[t], keep, r, rounds, min_count, smooth) for t in range(len(flow))]
    out = [np.stack([p[j] for p in res]) for j in range(3)]
    return out[0], out[1], out[2], None if state is None else np.stack([p[3] for p in res])


# ---- the definition once more, pixel by pixel in plain Python.  Shares nothing with the numpy above. ----
def _usable(u, v):
    return math.isfinite(u) and math.isfinite(v) and abs(u) < 1024.0 and abs(v) < 1024.0


def loop_pair(flow, state, keep, r, rounds, min_count, smooth):
    H, W = len(flow), len(flow[0])
    F = [[(float(flow[y][x][0]), float(flow[y][x][1])) for x in range(W)] for y in range(H)]
    V = [[_usable(*F[y][x]) and (state is None or (int(state[y][x]) <= 3 and bool(keep >> int(state[y][x]) & 1))) for x in range(W)]
         for y in range(H)]
    filled = [[0 if V[y][x] else UNFILLED for x in range(W)] for y in range(H)]

    def lower_median(F, V, x, y, comp):
        vals = sorted(F[qy][qx][comp] for qy in range(max(y - r, 0), min(y + r, H - 1) + 1)
                      for qx in range(max(x - r, 0), min(x + r, W - 1) + 1) if V[qy][qx])
        return vals, (vals[(len(vals) - 1) // 2] if vals else None)

    for g in range(1, rounds + 1):
        Fn, Vn = [row[:] for row in F], [row[:] for row in V]
        for y in range(H):
            for x in range(W):
                if V[y][x]:
                    continue
                us, mu = lower_median(F, V, x, y, 0)
                _, mv = lower_median(F, V, x, y, 1)
                if len(us) >= min_count:
                    Fn[y][x], Vn[y][x], filled[y][x] = (mu, mv), True, g
        F, V = Fn, Vn
    if smooth:
        Fn = [row[:] for row in F]
        for y in range(H):
            for x in range(W):
                if V[y][x]:
                    Fn[y][x] = (lower_median(F, V, x, y, 0)[1], lower_median(F, V, x, y, 1)[1])
        F = Fn
    return F, filled


# ---- the cases ----
class Params:
    def __init__(self, keep=1, r=1, rounds=8, min_count=1, smooth=False):
        self.keep, self.r, self.rounds, self.min_count, self.smooth = keep, r, rounds, min_count, smooth

    def args(self):
        return self.keep, self.r, self.rounds, self.min_count, int(self.smooth)

    def __repr__(self):
        return "keep%d-r%d-g%d-m%d-%s" % (self.keep, self.r, self.rounds, self.min_count, "smooth" if self.smooth else "fill")


class Case:
    """flow (n,H,W,2) f32, state (n,H,W) u8 or None, the parameter sets it runs with, and what it is for: `claims`, a set of
    'seam' (targets on both sides of a vertical and of a horizontal tile seam), 'round3' (a pixel filled in round >= 3),
    'unfilled', 'even' (a filled pixel whose window held an even count), 'tie' (... equal values around its median),
    'split' (u and v taken from different neighbours), 'mincount' (neighbouring targets with min_count - 1 and min_count
    sources), 'all_source', 'all_target'.  test_repair_host.py holds every case to its claims at its first parameter set."""

    def __init__(self, name, flow, state, params, claims=()):
        self.name, self.flow, self.state, self.params, self.claims = name, np.ascontiguousarray(flow, np.float32), state, tuple(params), set(claims)
        self.flow.setflags(write=False)
        if state is not None:
            self.state = np.ascontiguousarray(state, np.uint8)
            self.state.setflags(write=False)
        self.shape = self.flow.shape[:3]

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def reference(self, p):
        """the model at one of the case's parameter sets, computed once and read-only"""
        out = model(self.flow, self.state, *p.args())
        for a in out:
            if a is not None:
                a.setflags(write=False)
        return out


def _field(rng, n, H, W, kind):
    if kind == "quant":
        return QUANT[rng.integers(0, len(QUANT), (n, H, W, 2))]
    if kind == "big":
        return (rng.choice(np.array([BELOW, -BELOW, 1000.0, -3.0], np.float32), (n, H, W, 2))).astype(np.float32)
    return (rng.standard_normal((n, H, W, 2)) * 3).astype(np.float32)


def _build():
    rng = np.random.default_rng(20240611)
    cases = []

    def add(name, flow, state, params, claims=()):
        cases.append(Case(name, flow, state, params, claims))

    # the smallest frames: every window is clipped on all sides
    for W, H, n, r in ((1, 1, 1, 1), (1, 7, 2, 1), (7, 1, 3, 2), (2, 2, 1, 2), (2, 2, 1, 1)):
        f = _field(rng, n, H, W, "quant")
        st = rng.choice(np.array([OK, OK, MISMATCH], np.uint8), (n, H, W))
        st.reshape(n, -1)[:, 0] = OK if W * H > 1 else MISMATCH
        add(f"tiny-{W}x{H}-n{n}-r{r}", f, st, [Params(r=r), Params(r=r, smooth=True), Params(r=r, rounds=0, smooth=True)])
        add(f"tiny-nostate-{W}x{H}-n{n}-r{r}", f, None, [Params(r=r, rounds=1), Params(r=r, rounds=0, smooth=True)])
    for r in (1, 2):
        TX, TY = tile(r)
        side = 2 * (3 * r) + 1
        # one pixel short of a tile's width, one row past its height: single pixels, the corners, the borders, a checkerboard
        W, H, n = TX - 1, TY + 1, 2
        f = _field(rng, n, H, W, "random")
        st = np.zeros((n, H, W), np.uint8)
        st[0, H // 2, W // 2] = MISMATCH
        st[0, TY, 3] = LEAVES                                              # a single pixel below the seam
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            st[0, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = MISMATCH     # 2x2 in each corner
        st[0, 0, 10:20] = st[0, H - 1, 10:20] = st[0, 5:9, 0] = st[0, 5:9, W - 1] = MISMATCH
        yy, xx = np.mgrid[0:H, 0:W]
        st[1] = np.where((yy + xx) % 2 == 0, OK, MISMATCH)
        add(f"edges-{W}x{H}-n{n}-r{r}", f, st, [Params(r=r), Params(r=r, rounds=1, smooth=True), Params(r=r, rounds=0, smooth=True),
                                                 Params(r=r, rounds=3, min_count=(2 * r + 1) ** 2 // 2)], {"even", "split"})
        # two tiles and a pixel wide, a tile and three rows high, odd W*H, three pairs: a hole across both seams and a square
        # one that takes three rounds in pair 0, all sources in pair 1, all targets in pair 2
        W, H, n = 2 * TX + 1, TY + 3, 3
        assert (W * H) % 2 == 1 and side <= TY
        for kind in ("random", "quant"):
            f = _field(rng, n, H, W, kind)
            st = np.zeros((n, H, W), np.uint8)
            st[0, TY - 2:TY + 2, TX - 3:TX + 3] = MISMATCH                 # spans the vertical seam at TX and the horizontal at TY
            st[0, 1:1 + side, TX + 8:TX + 8 + side] = INVALID
            st[0, 0:TY, 2 * TX - 1:2 * TX + 1] = LEAVES                    # a slit along the second vertical seam
            st[2] = MISMATCH
            claims = {"seam", "round3", "all_source", "all_target", "even"} | ({"tie"} if kind == "quant" else {"split"})
            add(f"seams-{kind}-{W}x{H}-n{n}-r{r}", f, st,
                [Params(r=r), Params(r=r, smooth=True), Params(r=r, rounds=0, smooth=True), Params(keep=1 | 1 << LEAVES, r=r, rounds=2),
                 Params(keep=15, r=r, rounds=1)], claims)
        # a hole the rounds cannot close
        W, H, n = TX + 5, TY + 2, 1
        f = _field(rng, n, H, W, "random")
        st = np.zeros((n, H, W), np.uint8)
        st[0, 1:H - 1, 2:W - 2] = MISMATCH
        add(f"open-{W}x{H}-n{n}-r{r}", f, st, [Params(r=r, rounds=2), Params(r=r, rounds=2, smooth=True), Params(r=r, rounds=1, min_count=3)],
            {"unfilled", "seam"})
        # exactly min_count - 1 and min_count sources: three sources in a row in a frame of targets
        W, H, n = 12, 9, 1
        f = _field(rng, n, H, W, "random")
        st = np.full((n, H, W), MISMATCH, np.uint8)
        st[0, 4, 4:7] = OK
        add(f"mincount-{W}x{H}-n{n}-r{r}", f, st, [Params(r=r, rounds=2, min_count=3), Params(r=r, rounds=4, min_count=2)], {"mincount", "unfilled"})
        # what is not a source whatever its state says, states that are in no set, several sets, values next to the limit
        W, H, n = TX + 3, 7, 2
        f = _field(rng, n, H, W, "big")
        f[1] = _field(rng, 1, H, W, "quant")[0]
        st = rng.integers(0, 4, (n, H, W)).astype(np.uint8)
        flat, sflat = f.reshape(-1, 2), st.reshape(-1)
        for j, s in enumerate(SPECIALS):
            for comp in (0, 1):
                at = 11 + 17 * (2 * j + comp)
                flat[at, comp], sflat[at] = s, OK
        sflat[5::23] = rng.choice(np.array([4, 7, 128, 255], np.uint8), len(sflat[5::23]))
        add(f"values-{W}x{H}-n{n}-r{r}", f, st, [Params(keep=k, r=r, rounds=3, smooth=sm) for k, sm in ((1, False), (5, True), (10, False), (15, True))]
            + [Params(keep=2, r=r, rounds=0, smooth=True)], {"even"})
        add(f"values-nostate-{W}x{H}-n{n}-r{r}", f, None, [Params(r=r, rounds=2), Params(r=r, rounds=2, smooth=True), Params(r=r, rounds=0, smooth=True)])
    return tuple(cases)


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
RUNS = tuple((c, p) for c in CASES for p in c.params)
