"""Which vectors of a flow field can be trusted: the forward-backward check (csrc/fb_check.hip; include/ofc.h has the
definition).  The reference has no counterpart: it trusted every vector of cv2.calcOpticalFlowFarneback alike
(computeOpticalFlowModule.py:20-22), although Farneback flow is wrong in known places: where something is uncovered or
occluded, at motion boundaries, and where a pixel leaves the frame.

A pixel of frame t is followed by its forward vector into frame t+1; the backward field (frame t+1 -> t) is read there,
bilinearly, and the two should cancel: |f + b|^2 <= alpha (|f|^2 + |b|^2) + beta.  All of it is done in integers of 1/65536
px, so every result is exact and does not depend on the order the device worked in.  A pixel's state is one of
CONSISTENT, MISMATCH, LEAVES (it lands outside the frame) and INVALID (its vector, or one it lands on, is not a usable
number)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check as _check
from ._lib import load, ptr

CONSISTENT, MISMATCH, LEAVES, INVALID = _lib.CONSIST_OK, _lib.CONSIST_MISMATCH, _lib.CONSIST_LEAVES, _lib.CONSIST_INVALID
NSTATE = _lib.CONSIST_STATES
STATE_NAMES = ("consistent", "mismatch", "leaves", "invalid")
ALPHA, BETA = 0.01, 0.5       # the convention of the literature (alpha 0.01, beta 0.5 px^2); not tuned on any footage here
ONE = 65536


def quantise(alpha=ALPHA, beta=BETA):
    """-> (alpha_q, beta_q), the two integers the library takes: alpha in 16-bit fixed point (0 .. 65536, so alpha in
    0 .. 1), beta in px^2 in units of 2^-32 (0 .. 2^62, so beta in 0 .. 2^30).  ValueError outside those limits or for a
    value that is not finite.  The defaults give (655, 2^31)."""
    if not (np.isfinite(alpha) and np.isfinite(beta)):
        raise ValueError(f"alpha and beta must be finite, got {alpha!r}, {beta!r}")
    alpha_q, beta_q = int(round(float(alpha) * ONE)), int(round(float(beta) * 2.0 ** 32))
    if not 0 <= alpha_q <= _lib.CONSIST_ALPHA_MAX:
        raise ValueError(f"alpha = {alpha!r}: 0 .. 1")
    if not 0 <= beta_q <= _lib.CONSIST_BETA_MAX:
        raise ValueError(f"beta = {beta!r}: 0 .. 2^30 px^2")
    return alpha_q, beta_q


def check_args(W, H, n, alpha_q=655, beta_q=1 << 31):
    """the library's own decision on the arguments (ofc_consist_check, host only): ValueError or OfcError as it refuses"""
    _check(load().ofc_consist_check(int(W), int(H), int(n), int(alpha_q), int(beta_q)))


def keep_mask(states):
    """an iterable of states -> the 4-bit set ofc_consist_mask_dev takes"""
    keep = 0
    for s in states:
        if not 0 <= int(s) < NSTATE:
            raise ValueError(f"state {s!r}: 0 .. {NSTATE - 1}")
        keep |= 1 << int(s)
    return keep


class Consistency:
    """state: (n,H,W) u8, one of CONSISTENT, MISMATCH, LEAVES, INVALID per pixel; counts: (n,4) int64, the pixels of every
    pair in each state; residual: (n,H,W,2) f64 px, f + b where the state is CONSISTENT or MISMATCH and 0 elsewhere, or
    None when it was not asked for (residual_q holds the integers, 1/65536 px); alpha_q, beta_q: what it was decided by."""

    def __init__(self, state, counts, residual_q, alpha_q, beta_q):
        self.state, self.counts, self.residual_q, self.alpha_q, self.beta_q = state, counts, residual_q, alpha_q, beta_q

    def __len__(self):
        return len(self.state)

    @property
    def residual(self):
        return None if self.residual_q is None else self.residual_q / float(ONE)

    def share(self):
        """(n,4) f64: the share of every pair's pixels in each state"""
        return self.counts / self.counts.sum(1, keepdims=True).astype(np.float64)


def check(fwd, bwd, alpha=ALPHA, beta=BETA, residual=False, bwd_reversed=False, device=0):
    """fwd ((n,)H,W,2 f32): pair t is the flow frame t -> t+1 on frame t's grid; bwd, of the same shape: the flow frame
    t+1 -> t on frame t+1's grid, pair t's at bwd[t], or at bwd[n-1-t] with bwd_reversed (what a flow engine leaves when it
    is run over the reversed clip) -> Consistency.  alpha and beta default to the convention of the literature (0.01 and
    0.5 px^2); they are not tuned here."""
    from .blobs import _stack_flow
    f, b = _stack_flow(fwd), _stack_flow(bwd)
    if f.shape != b.shape:
        raise ValueError(f"bwd {b.shape} does not match fwd {f.shape}")
    alpha_q, beta_q = quantise(alpha, beta)
    n, H, W = f.shape[:3]
    check_args(W, H, n, alpha_q, beta_q)
    state, counts = np.empty((n, H, W), np.uint8), np.empty((n, NSTATE), np.int64)
    resid = np.empty((n, H, W, 2), np.int32) if residual else None
    _check(load().ofc_consist(device, ptr(f), ptr(b), W, H, n, int(bool(bwd_reversed)), alpha_q, beta_q, ptr(state), ptr(counts),
                              ptr(resid)))
    return Consistency(state, counts, resid, alpha_q, beta_q)


def check_dev(fwd_ptr, bwd_ptr, W, H, n, state_ptr, alpha_q=655, beta_q=1 << 31, bwd_reversed=False, residual=False, device=0):
    """ofc_consist_dev on fields that are on the device: the state map u8 [n][H][W] stays there, at state_ptr; only the
    counts, and the residual when asked for, leave it -> (counts (n,4) int64, residual (n,H,W,2) int32 or None)"""
    check_args(W, H, n, alpha_q, beta_q)
    cnt = _lib.DeviceBuffer(n * NSTATE * 8, device)
    res = _lib.DeviceBuffer(n * W * H * 8, device) if residual else None
    try:
        _check(load().ofc_consist_dev(device, C.c_void_p(fwd_ptr), C.c_void_p(bwd_ptr), W, H, n, int(bool(bwd_reversed)), alpha_q,
                                      beta_q, C.c_void_p(state_ptr), C.c_void_p(cnt.ptr), C.c_void_p(res.ptr) if residual else None))
        return cnt.download((n, NSTATE), np.int64), res.download((n, H, W, 2), np.int32) if residual else None
    finally:
        cnt.free()
        if res is not None:
            res.free()


def mask_dev(state_ptr, n, keep=(CONSISTENT,), keys_ptr=None, w_ptr=None, device=0):
    """ofc_consist_mask_dev: where a pixel's state is not in `keep`, its key becomes 255 (the background of a blob key map)
    and its weight 0; n states at state_ptr, u8 keys at keys_ptr and f32 weights at w_ptr, each optional, on the device"""
    _check(load().ofc_consist_mask_dev(device, C.c_void_p(state_ptr), int(n), keep_mask(keep),
                                       C.c_void_p(keys_ptr) if keys_ptr else None, C.c_void_p(w_ptr) if w_ptr else None))


def frames_reverse_dev(frames_ptr, W, H, n_frames, out_ptr, device=0):
    """ofc_frames_reverse_dev: the u8 clip [n_frames][H][W] at frames_ptr, its frames in reverse order, into out_ptr"""
    _check(load().ofc_frames_reverse_dev(device, C.c_void_p(frames_ptr), int(W), int(H), int(n_frames), C.c_void_p(out_ptr)))
