"""Point trajectories: points followed through a clip's flow fields (csrc/trajectories.hip; include/ofc.h has the definition).
The reference has no counterpart: its motion signature over time was a per-cell mean (drawGridsAndOutputCSV.py), it never
followed a point.

Points are seeded on a grid, at blob centroids or anywhere, in 1/65536 px.  Each is carried from pair to pair by the bilinearly
interpolated flow at its sub-pixel position and stops where it would leave the frame (LEAVES), where one of the four vectors
under it is not a usable number (INVALID), or, with the state map of a check, where the nearest pixel's state is not in
`keep` (UNTRUSTED).  All of it is done in integers, so every result is exact and does not depend on the order the device
worked in, nor on how the pairs were cut into launches.

follow() carries a fixed set of points; follow_dense() (csrc/tracklets.hip) keeps a pool of tracks instead: every frame each
grid cell without a live track gets a new one, and a track is cut after a fixed number of steps."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check as _check
from ._lib import load, ptr

RAN, UNTRUSTED, LEAVES, INVALID = _lib.TRAJ_RAN, _lib.TRAJ_UNTRUSTED, _lib.TRAJ_LEAVES, _lib.TRAJ_INVALID
WHY_NAMES = ("ran", "untrusted", "leaves", "invalid")
ONE = 65536


def check_args(W, H, n, P, keep=0, pairs_per_launch=0):
    """the library's own decision on the arguments (ofc_traj_check, host only): ValueError or OfcError as it refuses"""
    _check(load().ofc_traj_check(int(W), int(H), int(n), int(P), int(keep), int(pairs_per_launch)))


def launch_geometry(W, H, n, P):
    """ofc_traj_launch_geometry (host only) -> (pairs per launch, work-groups per launch, launches, lanes per work-group):
    how pairs_per_launch=0 cuts n pairs of P points into launches"""
    out = (C.c_int * 4)()
    _check(load().ofc_traj_launch_geometry(int(W), int(H), int(n), int(P), C.byref(out)))
    return tuple(out)


def grid_seeds(W, H, step=8, offset=None):
    """-> int32 (P, 2): (X, Y) in 1/65536 px of the grid points offset + i * step that lie inside the W x H frame, row by
    row.  step and offset in px (floats allowed; offset defaults to step / 2, the centre of every step x step cell; one
    value or (ox, oy))."""
    step = float(step)
    if not (np.isfinite(step) and step > 0):
        raise ValueError(f"step = {step!r}: a positive number of pixels")
    ox, oy = (step / 2, step / 2) if offset is None else np.broadcast_to(np.asarray(offset, np.float64), (2,))
    sq = int(round(step * ONE))
    if sq < 1:
        raise ValueError(f"step = {step!r}: at least 1/65536 px")

    def axis(o, size):
        o = int(round(float(o) * ONE))
        last = (int(size) - 1) * ONE
        first = o if o >= 0 else o + (-o + sq - 1) // sq * sq
        return np.arange(first, last + 1, sq, dtype=np.int64)
    xs, ys = axis(ox, W), axis(oy, H)
    out = np.empty((len(ys), len(xs), 2), np.int32)
    out[..., 0], out[..., 1] = xs[None, :], ys[:, None]
    return out.reshape(-1, 2)


def _seeds(seeds, W, H, step):
    s = grid_seeds(W, H, step) if seeds is None else np.ascontiguousarray(seeds, np.int32)
    if s.ndim != 2 or s.shape[1] != 2 or len(s) < 1:
        raise ValueError(f"seeds should be an int32 (P, 2) array of (X, Y) in 1/65536 px with P >= 1, got shape {s.shape}")
    return s


def seeds_from_px(xy):
    """float (P, 2) positions in px -> int32 (P, 2) seeds in 1/65536 px, rounded to the nearest"""
    return np.ascontiguousarray(np.rint(np.asarray(xy, np.float64) * ONE), np.int32)


class Trajectories:
    """pos: (n+1, P, 2) int32, time-major, (X, Y) in 1/65536 px: pos[0] the seeds, pos[t+1] the positions after pair t (an
    ended point stays where it ended); length: (P,) int32, the steps every point took, 0 .. n; why: (P,) u8, RAN for a point
    that took all n steps, else UNTRUSTED, LEAVES or INVALID."""

    def __init__(self, pos, length, why):
        self.pos, self.length, self.why = pos, length, why

    def __len__(self):
        return self.pos.shape[1]

    @property
    def n_pairs(self):
        return len(self.pos) - 1

    def xy(self):
        """(n+1, P, 2) f64: the positions in px"""
        return self.pos / float(ONE)

    def displacement(self):
        """(P, 2) f64 px: from the seed to where the point is at the end"""
        return (self.pos[-1].astype(np.int64) - self.pos[0]) / float(ONE)

    def alive(self):
        """(n+1,) int64: the points that have taken t steps or more, for t = 0 .. n (the points live at frame t)"""
        return (self.length[None, :] >= np.arange(self.n_pairs + 1)[:, None]).sum(1).astype(np.int64)

    def shapes(self, L):
        """the trajectory-shape descriptor of the dense-trajectories literature: for the m points with at least L steps, the
        first L step vectors divided by the sum of their lengths -> (rows (m, 2L) f64, the m point indices).  A row is what
        cluster.KMeans takes.  The row of a point that never moved is zeros."""
        L = int(L)
        if not 1 <= L <= self.n_pairs:
            raise ValueError(f"L = {L}: 1 .. {self.n_pairs}")
        idx = np.flatnonzero(self.length >= L)
        p = self.pos[:L + 1, idx].astype(np.int64)
        d = (p[1:] - p[:-1]) / float(ONE)                       # (L, m, 2)
        total = np.sqrt((d ** 2).sum(2)).sum(0)                 # (m,)
        rows = np.zeros((len(idx), 2 * L))
        moved = total > 0
        rows[moved] = (d[:, moved] / total[moved][None, :, None]).transpose(1, 0, 2).reshape(-1, 2 * L)
        return rows, idx


def follow(flow, seeds=None, step=8, state=None, keep=(0,), pairs_per_launch=0, device=0):
    """flow ((n,)H,W,2 f32): pair t's field on frame t's grid; seeds int32 (P,2) in 1/65536 px (None: grid_seeds(W, H, step));
    state ((n,)H,W u8, optional): the state map of a check, with `keep` the states a point may stand on
    (consistency.keep_mask; an int is taken as the set itself) -> Trajectories (ofc_traj).  pairs_per_launch: 0 lets the
    library's cost model cut the pairs into launches, a positive value forces it; the result is the same bits."""
    from .blobs import _stack_flow
    from .consistency import keep_mask
    f = _stack_flow(flow)
    n, H, W = f.shape[:3]
    s = _seeds(seeds, W, H, step)
    P = len(s)
    kp = int(keep) if isinstance(keep, (int, np.integer)) else keep_mask(keep)
    st = None
    if state is not None:
        st = np.ascontiguousarray(state, np.uint8)
        if st.shape not in ((n, H, W), (H, W) if n == 1 else None):
            raise ValueError(f"state {st.shape} does not match flow {f.shape}")
    check_args(W, H, n, P, kp, pairs_per_launch)
    pos, length, why = np.empty((n + 1, P, 2), np.int32), np.empty(P, np.int32), np.empty(P, np.uint8)
    _check(load().ofc_traj(device, ptr(f), ptr(st), W, H, n, ptr(s), P, kp, int(pairs_per_launch), ptr(pos), ptr(length), ptr(why)))
    return Trajectories(pos, length, why)


def follow_dev(flow_ptr, W, H, n, seeds, state_ptr=None, keep=(0,), pairs_per_launch=0, device=0):
    """ofc_traj_dev on a field (and a state map) that are on the device; seeds is a host int32 (P,2) array.  The table is
    built on the device with the seeds as its row 0 and downloaded -> Trajectories"""
    from .consistency import keep_mask
    s = _seeds(seeds, W, H, 8)
    P = len(s)
    kp = int(keep) if isinstance(keep, (int, np.integer)) else keep_mask(keep)
    check_args(W, H, n, P, kp, pairs_per_launch)
    pos = _lib.DeviceBuffer((n + 1) * P * 8, device)
    ln = _lib.DeviceBuffer(P * 4, device)
    why = _lib.DeviceBuffer(P, device)
    try:
        pos.upload(s)
        _check(load().ofc_traj_dev(device, C.c_void_p(flow_ptr), C.c_void_p(state_ptr) if state_ptr else None, int(W), int(H), int(n),
                                   C.c_void_p(pos.ptr), P, kp, int(pairs_per_launch), C.c_void_p(pos.ptr), C.c_void_p(ln.ptr),
                                   C.c_void_p(why.ptr)))
        return Trajectories(pos.download((n + 1, P, 2), np.int32), ln.download((P,), np.int32), why.download((P,), np.uint8))
    finally:
        for b in (pos, ln, why):
            b.free()


# ---- tracklets: dense trajectories with reseeding (csrc/tracklets.hip; the definition is in include/ofc.h) ----
FULL = _lib.TRAJ_FULL
TRACKLET_WHY_NAMES = WHY_NAMES + ("full",)


def grid_cells(W, H, cell):
    """-> (cols, rows) of the tracklets' grid of cell x cell px"""
    cell = int(cell)
    if cell < 1:
        raise ValueError(f"cell = {cell}: at least 1 px")
    return -(-int(W) // cell), -(-int(H) // cell)


def default_max_tracks(W, H, n, cell, length):
    """the pool follow_dense takes when max_tracks is None: cells * (1 + ceil(2 n / length)), at most cells * n.  Every cell
    turns its track over once in `length` frames in the steady state; the factor of two is a guess, not tuned.  It matters
    little: a pool that runs out shows in the outputs (Tracklets.overflowed)."""
    cols, rows = grid_cells(W, H, cell)
    cells, n, length = cols * rows, int(n), max(int(length), 1)
    return min(cells * (1 + -(-2 * n // length)), cells * n)


def check_dense_args(W, H, n, cell, length, max_tracks, keep=0):
    """the library's own decision on the arguments (ofc_tracklets_check, host only): ValueError or OfcError as it refuses"""
    _check(load().ofc_tracklets_check(int(W), int(H), int(n), int(cell), int(length), int(max_tracks), int(keep)))


class Tracklets:
    """The T tracks a clip of n pairs gave.  pos: (L+1, T, 2) int32, step-major, (X, Y) in 1/65536 px: pos[k, i] is track i
    after k steps, (-1, -1) above its length; birth: (T,) int32, the frame it was seeded at; length: (T,) int32, the steps it
    took, 0 .. L; why: (T,) u8: RAN for a track still live when the clip ended, FULL for one that took all L steps, else
    UNTRUSTED, LEAVES or INVALID; empty, born, blocked: (n,) int32 per frame: the cells without a live track whose seed may
    stand, the tracks born, and the cells whose seed the state map refused; max_tracks: the pool the call had."""

    def __init__(self, pos, birth, length, why, frames, max_tracks):
        frames = np.asarray(frames)
        T = int(frames[:, 1].sum())
        self.pos, self.birth, self.length, self.why = (np.ascontiguousarray(a) for a in (pos[:, :T], birth[:T], length[:T], why[:T]))
        self.empty, self.born, self.blocked = (np.ascontiguousarray(frames[:, j]) for j in range(3))
        self.max_tracks = int(max_tracks)

    def __len__(self):
        return self.pos.shape[1]

    @property
    def n_pairs(self):
        return len(self.born)

    @property
    def max_len(self):
        return len(self.pos) - 1

    @property
    def overflowed(self):
        """True iff the pool ran out: some frame seeded fewer tracks than it had empty cells"""
        return bool((self.born < self.empty).any())

    def xy(self):
        """(L+1, T, 2) f64: the positions in px, nan above a track's length"""
        out = self.pos / float(ONE)
        out[self.pos < 0] = np.nan
        return out

    def _live(self, t):
        age = int(t) - self.birth
        return (age >= 0) & (age <= self.length) & (age < self.max_len)

    def alive(self):
        """(n,) int64: the tracks that are live at frame t after its births, i.e. that take or try pair t's step"""
        return np.array([self._live(t).sum() for t in range(self.n_pairs)], np.int64)

    def at(self, t):
        """-> (ids (m,), pos (m, 2) int32): the tracks live at frame t after its births, and where they stand in frame t"""
        t = int(t)
        if not 0 <= t < self.n_pairs:
            raise ValueError(f"t = {t}: 0 .. {self.n_pairs - 1}")
        ids = np.flatnonzero(self._live(t))
        return ids, self.pos[t - self.birth[ids], ids]

    def shapes(self, L=None, min_length=None):
        """the descriptor of Trajectories.shapes over the tracks with at least L steps (None: max_len, the full tracks) ->
        (rows (m, 2L) f64, the m track ids).  min_length (px): only tracks whose L steps sum to at least this length, which
        drops the static ones."""
        L = self.max_len if L is None else int(L)
        if not 1 <= L <= self.max_len:
            raise ValueError(f"L = {L}: 1 .. {self.max_len}")
        idx = np.flatnonzero(self.length >= L)
        p = self.pos[:L + 1, idx].astype(np.int64)
        d = (p[1:] - p[:-1]) / float(ONE)                       # (L, m, 2)
        total = np.sqrt((d ** 2).sum(2)).sum(0)                 # (m,)
        if min_length is not None:
            sel = total >= float(min_length)
            idx, d, total = idx[sel], d[:, sel], total[sel]
        rows = np.zeros((len(idx), 2 * L))
        moved = total > 0
        rows[moved] = (d[:, moved] / total[moved][None, :, None]).transpose(1, 0, 2).reshape(-1, 2 * L)
        return rows, idx


def _dense_args(W, H, n, cell, length, max_tracks, keep):
    from .consistency import keep_mask
    cell, length = int(cell), int(length)
    M = default_max_tracks(W, H, n, cell, length) if max_tracks is None else int(max_tracks)
    kp = int(keep) if isinstance(keep, (int, np.integer)) else keep_mask(keep)
    check_dense_args(W, H, n, cell, length, M, kp)
    return cell, length, M, kp


def follow_dense(flow, cell=8, length=15, max_tracks=None, state=None, keep=(0,), device=0):
    """flow ((n,)H,W,2 f32): pair t's field on frame t's grid -> Tracklets (ofc_tracklets).  Every frame each cell x cell
    grid cell without a live track gets a new one at its centre, and a track is cut after `length` steps.  state
    ((n,)H,W u8, optional): the state map of a check, with `keep` the states a track may stand on and be seeded on.
    max_tracks: the pool; None takes default_max_tracks, which is a guess and not tuned -- look at Tracklets.overflowed."""
    from .blobs import _stack_flow
    f = _stack_flow(flow)
    n, H, W = f.shape[:3]
    cell, L, M, kp = _dense_args(W, H, n, cell, length, max_tracks, keep)
    st = None
    if state is not None:
        st = np.ascontiguousarray(state, np.uint8)
        if st.shape not in ((n, H, W), (H, W) if n == 1 else None):
            raise ValueError(f"state {st.shape} does not match flow {f.shape}")
    pos, birth, ln, why = np.empty((L + 1, M, 2), np.int32), np.empty(M, np.int32), np.empty(M, np.int32), np.empty(M, np.uint8)
    frames = np.empty((n, 3), np.int32)
    _check(load().ofc_tracklets(device, ptr(f), ptr(st), W, H, n, cell, L, M, kp, ptr(pos), ptr(birth), ptr(ln), ptr(why), ptr(frames)))
    return Tracklets(pos, birth, ln, why, frames, M)


def follow_dense_dev(flow_ptr, W, H, n, cell=8, length=15, max_tracks=None, state_ptr=None, keep=(0,), device=0):
    """ofc_tracklets_dev on a field (and a state map) that are on the device; the outputs are built there and downloaded
    -> Tracklets"""
    cell, L, M, kp = _dense_args(W, H, n, cell, length, max_tracks, keep)
    bufs = [_lib.DeviceBuffer(b, device) for b in ((L + 1) * M * 8, M * 4, M * 4, M, n * 12)]
    pos, birth, ln, why, frames = bufs
    try:
        _check(load().ofc_tracklets_dev(device, C.c_void_p(flow_ptr), C.c_void_p(state_ptr) if state_ptr else None, int(W), int(H), int(n),
                                        cell, L, M, kp, *(C.c_void_p(b.ptr) for b in bufs)))
        fr = frames.download((n, 3), np.int32)
        return Tracklets(pos.download((L + 1, M, 2), np.int32), birth.download((M,), np.int32), ln.download((M,), np.int32),
                         why.download((M,), np.uint8), fr, M)
    finally:
        for b in bufs:
            b.free()
