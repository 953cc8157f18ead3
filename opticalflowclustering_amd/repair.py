"""Repair of a flow field: a masked median fill of the vectors that are not trusted, and a median smoothing pass
(csrc/flow_repair.hip; include/ofc.h has the definition).  The reference has no counterpart: it trusted every vector of
cv2.calcOpticalFlowFarneback alike (computeOpticalFlowModule.py:20-22).

The two checks (consistency.py, photometric.py) say which vectors to trust; so far an untrusted one could only be thrown
away, which punches holes into moving objects along their leading and trailing edges.  Here such a vector (a target) is
replaced by the component-wise lower median of the trusted vectors (sources) in its 3x3 or 5x5 window, round after round,
every round reading only the result of the one before, until the hole is closed or the rounds run out.  A smoothing pass, the
same median over every pixel that has a value, can follow: what cv2.medianBlur does to one channel, with the window clipped
at the border.  A median only selects, so every result is one of the input numbers, exactly, whatever order the device
worked in."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check as _check
from ._lib import load, ptr
from .consistency import CONSISTENT, INVALID, LEAVES, MISMATCH, keep_mask  # noqa: F401

NCOUNT = _lib.REPAIR_NCOUNT
UNFILLED = _lib.REPAIR_UNFILLED     # filled[p] of a target that no round filled
SOURCES, FILLED, UNFILLED_COUNT = 0, 1, 2     # the columns of counts
ROUNDS, MIN_COUNT = 8, 1            # a convention, not tuned on any footage here


def tile(radius=1):
    """(TX, TY): the tile of a frame one work-group of the sweep kernel takes at this radius (ofc_repair_tile)"""
    out = (C.c_int * 2)()
    load().ofc_repair_tile(int(radius), C.byref(out))
    return int(out[0]), int(out[1])


def check_args(W, H, n, keep=1, radius=1, rounds=ROUNDS, min_count=MIN_COUNT, smooth=False):
    """the library's own decision on the arguments (ofc_repair_check, host only): ValueError or OfcError as it refuses.
    keep is the 4-bit set (keep_mask)."""
    _check(load().ofc_repair_check(int(W), int(H), int(n), int(keep), int(radius), int(rounds), int(min_count), int(smooth)))


class Repaired:
    """flow: (n,H,W,2) f32, the repaired field (None where it stayed on the device); filled: (n,H,W) u8, 0 for a source, g
    for a target filled in round g, 255 (UNFILLED) for a target never filled; counts: (n,3) int64, every pair's sources,
    filled and unfilled pixels; state: (n,H,W) u8, the input state map with the filled targets CONSISTENT, or None when no
    state was given."""

    def __init__(self, flow, filled, counts, state):
        self.flow, self.filled, self.state = flow, filled, state
        self.counts = np.asarray(counts, np.int64).reshape(-1, NCOUNT)

    def __len__(self):
        return len(self.counts)

    def share(self):
        """(n,3) f64: the share of every pair's pixels that are sources, filled and unfilled"""
        return self.counts / self.counts.sum(1, keepdims=True).astype(np.float64)


def fill(flow, state=None, keep=(CONSISTENT,), radius=1, rounds=ROUNDS, min_count=MIN_COUNT, smooth=False, device=0):
    """flow ((n,)H,W,2 f32) and the state map of one of the checks ((n,)H,W u8) or None, with which only vectors that are not
    usable numbers are targets -> Repaired.  rounds and min_count default to 8 and 1, a convention: they are not tuned on
    anything here."""
    from .blobs import _stack_flow
    f = _stack_flow(flow)
    n, H, W = f.shape[:3]
    st = None
    if state is not None:
        st = np.ascontiguousarray(state, np.uint8).reshape((-1,) + np.shape(state)[-2:])
        if st.shape != (n, H, W):
            raise ValueError(f"state should be ({n},{H},{W}) u8 for flow {f.shape}, got shape {np.shape(state)}")
    kp = keep_mask(keep)
    check_args(W, H, n, kp, radius, rounds, min_count, smooth)
    out, filled, counts = np.empty_like(f), np.empty((n, H, W), np.uint8), np.empty((n, NCOUNT), np.int64)
    st_out = np.empty((n, H, W), np.uint8) if st is not None else None
    _check(load().ofc_repair(device, ptr(f), ptr(st), W, H, n, kp, int(radius), int(rounds), int(min_count), int(bool(smooth)),
                             ptr(out), ptr(filled), ptr(st_out), ptr(counts)))
    return Repaired(out, filled, counts, st_out)


def median(flow, radius=1, device=0):
    """the median filter of a flow field, per component, window clipped at the border (lower median where the clipped
    window holds an even number of vectors); a vector that is not a usable number is left as it is and not read ->
    ((n,)H,W,2) f32 of flow's shape"""
    return fill(flow, None, radius=radius, rounds=0, smooth=True, device=device).flow.reshape(np.shape(flow))


def fill_dev(flow_ptr, state_ptr, W, H, n, out_ptr=None, filled_ptr=None, state_out_ptr=None, keep=1, radius=1, rounds=ROUNDS,
             min_count=MIN_COUNT, smooth=False, device=0):
    """ofc_repair_dev on a field that is on the device: out_ptr defaults to flow_ptr (in place); state_ptr, filled_ptr and
    state_out_ptr (may be state_ptr) may each be None; keep is the 4-bit set (keep_mask).  Only the counts leave the device
    -> (n,3) int64.  The defaults of rounds and min_count are a convention, not tuned on anything here."""
    check_args(W, H, n, keep, radius, rounds, min_count, smooth)
    cnt = _lib.DeviceBuffer(n * NCOUNT * 8, device)
    try:
        vp = lambda p: C.c_void_p(p) if p else None     # noqa: E731
        _check(load().ofc_repair_dev(device, C.c_void_p(flow_ptr), vp(state_ptr), W, H, n, int(keep), int(radius), int(rounds),
                                     int(min_count), int(bool(smooth)), C.c_void_p(out_ptr if out_ptr else flow_ptr), vp(filled_ptr),
                                     vp(state_out_ptr), C.c_void_p(cnt.ptr)))
        return cnt.download((n, NCOUNT), np.int64)
    finally:
        cnt.free()
