"""The tracklets of include/ofc.h twice over -- a numpy model that keeps the pool as arrays and takes the step from
trajectory_cases.reference one pair at a time, and an independent loop over frames and tracks in plain Python integers that
shares nothing with it -- and the table of cases that test_tracklet_host.py proves on the CPU and test_gpu_tracklets.py runs
on the device."""
import numpy as np

from tests import trajectory_cases as TC

RAN, UNTRUSTED, LEAVES, INVALID, FULL = 0, 1, 2, 3, 4
UNUSED = 255
ONE = TC.ONE
THREADS = 256                     # OFC_TRACKLET_THREADS: the cells of a work-group of the two birth kernels, the ids of one of the step
keep_mask = TC.keep_mask


def grid(W, H, cell):
    cols, rows = -(-W // cell), -(-H // cell)
    return cols, rows, cols * rows


# ---- the model: numpy, the whole pool at a time ----
def model(flow, cell, L, M, state=None, keep=1):
    """(n,H,W,2) f32, cell, L, M, (n,H,W) u8 or None, the set keep ->
    pos (L+1,M,2) int32, birth (M,) int32, len (M,) int32, why (M,) u8, frames (n,3) int32"""
    n, H, W = flow.shape[:3]
    cols, rows, cells = grid(W, H, cell)
    idx = np.arange(cells)
    seeds = np.stack([np.minimum((idx % cols * cell << 16) + (cell << 15), (W - 1) << 16),
                      np.minimum((idx // cols * cell << 16) + (cell << 15), (H - 1) << 16)], 1).astype(np.int32)
    pos = np.full((L + 1, M, 2), -1, np.int32)
    birth, length, why = np.full(M, -1, np.int32), np.zeros(M, np.int32), np.full(M, UNUSED, np.uint8)
    frames = np.zeros((n, 3), np.int32)
    used = 0
    for t in range(n):
        live = np.flatnonzero(why[:used] == RAN)
        at = pos[length[live], live].astype(np.int64)
        occupied = np.zeros(cells, bool)
        occupied[(at[:, 1] >> 16) // cell * cols + (at[:, 0] >> 16) // cell] = True
        ok = np.ones(cells, bool)
        if state is not None:
            s = state[t][(seeds[:, 1] + 32768) >> 16, (seeds[:, 0] + 32768) >> 16].astype(np.int64)
            ok = (s <= 3) & (((np.int64(keep) >> np.minimum(s, 16)) & 1) == 1)
        empty = np.flatnonzero(~occupied & ok)
        born = min(len(empty), M - used)
        frames[t] = len(empty), born, (~occupied & ~ok).sum()
        ids = used + np.arange(born)
        pos[0, ids], birth[ids], length[ids], why[ids] = seeds[empty[:born]], t, 0, RAN
        used += born
        live = np.flatnonzero(why[:used] == RAN)
        if len(live) == 0:
            continue
        after, took, reason = TC.reference(flow[t:t + 1], pos[length[live], live], None if state is None else state[t:t + 1], keep)
        moved = live[took == 1]
        pos[length[moved] + 1, moved] = after[1][took == 1]
        length[moved] += 1
        why[live[took == 0]] = reason[took == 0]
        why[moved[length[moved] >= L]] = FULL
    return pos, birth, length, why, frames


# ---- the same definition as a loop over frames, cells and tracks in Python integers.  Shares nothing with the model above
# (its step is trajectory_cases' per-point one, which shares nothing with trajectory_cases.reference). ----
def loop(flow, cell, L, M, state=None, keep=1):
    n, H, W = flow.shape[:3]
    f = flow.tolist()
    st = state.tolist() if state is not None else None
    xmax, ymax = (W - 1) * 65536, (H - 1) * 65536
    cols, rows = (W + cell - 1) // cell, (H + cell - 1) // cell
    tracks = []                                        # [birth, [positions], why or None while live]
    live = []
    frames = []
    big = dict(S=0, D=0, X=0)
    for t in range(n):
        occupied = set()
        for k in live:
            X, Y = tracks[k][1][-1]
            occupied.add((Y // 65536 // cell) * cols + X // 65536 // cell)
        empty = born = blocked = 0
        for c in range(rows * cols):
            if c in occupied:
                continue
            X0 = min((c % cols) * cell * 65536 + cell * 32768, xmax)
            Y0 = min((c // cols) * cell * 65536 + cell * 32768, ymax)
            if st is not None:
                s = st[t][(Y0 + 32768) // 65536][(X0 + 32768) // 65536]
                if s > 3 or not (keep >> s) & 1:
                    blocked += 1
                    continue
            empty += 1
            if len(tracks) < M:
                born += 1
                live.append(len(tracks))
                tracks.append([t, [(X0, Y0)], None])
        frames.append((empty, born, blocked))
        still = []
        for k in live:
            tr = tracks[k]
            X, Y = tr[1][-1]
            r = TC._step_reason(f[t], st[t] if st else None, keep, X, Y, W, H, xmax, ymax, big)
            if isinstance(r, tuple):
                tr[1].append(r)
                if len(tr[1]) - 1 == L:
                    tr[2] = FULL
                else:
                    still.append(k)
            else:
                tr[2] = r
        live = still
    pos = np.full((L + 1, M, 2), -1, np.int32)
    birth, length, why = np.full(M, -1, np.int32), np.zeros(M, np.int32), np.full(M, UNUSED, np.uint8)
    for k, (b, p, w) in enumerate(tracks):
        pos[:len(p), k] = p
        birth[k], length[k], why[k] = b, len(p) - 1, RAN if w is None else w
    return pos, birth, length, why, np.array(frames, np.int32).reshape(n, 3)


DTYPES = (np.int32, np.int32, np.int32, np.uint8, np.int32)


def same(got, want):
    for g, w, dt, name in zip(got, want, DTYPES, ("pos", "birth", "len", "why", "frames")):
        assert g.dtype == dt and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


# ---- the fields ----
def shift(n, H, W, u=3.25, v=0.5):
    f = np.empty((n, H, W, 2), np.float32)
    f[..., 0], f[..., 1] = u, v
    return f


def _radial(n, H, W, gain):
    ys, xs = np.mgrid[0:H, 0:W]
    f = np.empty((n, H, W, 2), np.float32)
    f[..., 0], f[..., 1] = gain * (xs - W / 2), gain * (ys - H / 2)     # the centre is (W/2, H/2)
    return f


def sink(n, H, W):
    return _radial(n, H, W, -0.2)


def source(n, H, W):
    return _radial(n, H, W, 0.2)


# ---- the cases ----
class Case:
    def __init__(self, name, flow, cell, L, M, state=None, keep=(0,)):
        self.name, self.cell, self.L, self.M, self.keep = name, cell, L, M, keep_mask(keep)
        self.flow = np.ascontiguousarray(flow, np.float32)
        self.state = None if state is None else np.ascontiguousarray(state, np.uint8)
        assert self.flow.ndim == 4 and self.flow.shape[3] == 2 and (self.state is None or self.state.shape == self.flow.shape[:3])
        for a in (self.flow,) + (() if self.state is None else (self.state,)):
            a.setflags(write=False)
        self._model = None

    def __repr__(self):
        return self.name

    @property
    def shape(self):
        return self.flow.shape[:3]

    @property
    def cells(self):
        return grid(self.shape[2], self.shape[1], self.cell)[2]

    def model(self):
        if self._model is None:                       # computed once, shared, never written
            self._model = model(self.flow, self.cell, self.L, self.M, self.state, self.keep)
            for a in self._model:
                a.setflags(write=False)
        return self._model

    def used(self):
        return int(self.model()[4][:, 1].sum())


def _state_case():
    """a state map with a column of seeds that may not stand (state 1, not in keep = {0}), one seed on a byte that is no state
    at all, and a stripe further right that ends the tracks that drift into it"""
    n, H, W = 6, 24, 40
    state = np.zeros((n, H, W), np.uint8)
    state[:, :, 12] = 1                               # the seeds of column cx = 1 stand on x = 12
    state[:, 4, 20] = 200                             # the seed of cell (2, 0)
    state[2:, :, 30:32] = 2                           # from frame 2 on
    return Case("state-40x24-c8-L4", shift(n, H, W, 1.75, 0.25), 8, 4, 400, state, (0,))


def _specials_case():
    """a patch of values that are no vectors: the tracks that reach it end INVALID"""
    n, H, W = 6, 24, 40
    f = shift(n, H, W, 2.5, 0.0)
    for j, s in enumerate(TC.SPECIALS):
        f[:, 3 + 3 * j, 20 + (j % 3), j % 2] = s
    return Case("specials-40x24-c4-L5", f, 4, 5, 2000)


def _seam_cases():
    """one row of cells: counts at the seams of the bitmap's words (32), the wave's ballot (64) and the work-group (256).  With
    L = 2 the step's id window starts at first[t-1], which these counts put either side of a multiple of 256, as they do
    `used`"""
    out = []
    for cells in (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513):
        W = 2 * cells - 1                             # the last cell is one px wide: a clamped seed
        out.append(Case(f"seam-{cells}-cells", shift(4, 2, W, 1.5, -0.125), 2, 2, 4 * cells))
    return out


def _scan_cases():
    """256 and 257 work-groups of cells: either side of one work-group per lane of the last work-group's scan"""
    return [Case(f"scan-{W}x256-c1", shift(2, 256, W, 0.75, 0.25), 1, 2, 140000) for W in (256, 257)]


def _exact_pool_case():
    """max_tracks equal to the births of shift-40x24 with a pool that never runs out"""
    free = Case("unbounded", shift(9, 24, 40), 8, 4, 1000)
    return Case("exact-pool-40x24-c8-L4", free.flow, 8, 4, free.used())


N = 9
TABLE = [
    Case("shift-40x24-c8-L4", shift(N, 24, 40), 8, 4, 1000),
    Case("shift-37x19-c5-L3", shift(N, 19, 37), 5, 3, 1000),
    Case("sink-40x24-c8-L20", sink(N, 24, 40), 8, 20, 40),
    Case("source-40x24-c8-L20", source(N, 24, 40), 8, 20, 40),
    Case("shift-67x35-c1-L2", shift(4, 35, 67), 1, 2, 20000),
    Case("shift-9x7-c16-L3", shift(5, 7, 9), 16, 3, 100),
]
EXTRA = [
    _state_case(),
    _specials_case(),
    Case("shift-37x16-c5-L3", shift(N, 16, 37, -2.25, -0.5), 5, 3, 1000),      # the last row is 1 px high: its seeds are clamped too
    Case("one-pair-40x24-c8",shift(1, 24, 40), 8, 4, 100),
    Case("one-step-40x24-c8-L1", shift(5, 24, 40), 8, 1, 200),
    _exact_pool_case(),
]
CASES = TABLE + EXTRA + _seam_cases() + _scan_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def default_max_tracks(W, H, n, cell, length):
    cells = grid(W, H, cell)[2]
    return min(cells * (1 + -(-2 * n // length)), cells * n)
