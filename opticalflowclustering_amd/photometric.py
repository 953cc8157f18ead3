"""Which vectors of a flow field agree with the frames they were computed from: the photometric (brightness-constancy)
check (csrc/photo_check.hip; include/ofc.h has the definition).  The reference has no counterpart: it trusted every vector of
cv2.calcOpticalFlowFarneback alike (computeOpticalFlowModule.py:20-22).

A pixel of frame t is followed by its vector into frame t+1; that frame is read there, bilinearly, and the grey value found
should be the pixel's own: |J - I0| <= tau + kappa * c, with c the contrast (max - min) of the four pixels it was read from,
which forgives the sub-pixel error of a vector that sits on an edge.  All of it is done in integers (positions in 1/65536 px,
grey values in 1/256 levels), so every result is exact and does not depend on the order the device worked in.  The check needs
no backward field, so it costs one sweep and also exists on a FlowStream; it says little where the image has no texture, so
it complements the forward-backward check (consistency.py) and does not replace it.  A pixel's state is one of that check's
codes: CONSISTENT, MISMATCH, LEAVES (it lands outside the frame) and INVALID (its vector is not a usable number), so every
consumer of a state map takes this one unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check as _check
from ._lib import load, ptr
from .consistency import CONSISTENT, INVALID, LEAVES, MISMATCH, NSTATE, STATE_NAMES, keep_mask  # noqa: F401

NSTAT = _lib.PHOTO_NSTAT
TAU, KAPPA = 8.0, 0.5         # grey levels, and grey levels per grey level of contrast: a convention, not tuned on any footage here
LEVEL = 256                   # J, e and tau_q are in 1/256 grey levels; kappa_q in 1/256


def quantise(tau=TAU, kappa=KAPPA):
    """-> (tau_q, kappa_q), the two integers the library takes: tau in 1/256 grey levels (0 .. 65280, so tau in 0 .. 255),
    kappa in 1/256 (0 .. 1024, so kappa in 0 .. 4).  ValueError outside those limits or for a value that is not finite.
    The defaults, a convention that is not tuned on anything here, give (2048, 128)."""
    if not (np.isfinite(tau) and np.isfinite(kappa)):
        raise ValueError(f"tau and kappa must be finite, got {tau!r}, {kappa!r}")
    tau_q, kappa_q = int(round(float(tau) * LEVEL)), int(round(float(kappa) * LEVEL))
    if not 0 <= tau_q <= _lib.PHOTO_TAU_MAX:
        raise ValueError(f"tau = {tau!r}: 0 .. 255 grey levels")
    if not 0 <= kappa_q <= _lib.PHOTO_KAPPA_MAX:
        raise ValueError(f"kappa = {kappa!r}: 0 .. 4")
    return tau_q, kappa_q


def check_args(W, H, n, tau_q=2048, kappa_q=128):
    """the library's own decision on the arguments (ofc_photo_check, host only): ValueError or OfcError as it refuses"""
    _check(load().ofc_photo_check(int(W), int(H), int(n), int(tau_q), int(kappa_q)))


class Photometric:
    """state: (n,H,W) u8, one of CONSISTENT, MISMATCH, LEAVES, INVALID per pixel (None where it stayed on the device);
    counts: (n,4) int64, the pixels of every pair in each state; abs_error: (n,) int64, the sum of |J - 256 I0| over the
    pair's compared pixels (states CONSISTENT and MISMATCH), in 1/256 grey levels; warped: (n,H,W) u16, frame t+1 read where
    frame t's pixels land, in 1/256 grey levels, 0 where the state is LEAVES or INVALID, or None when it was not asked
    for; tau_q, kappa_q: what it was decided by."""

    def __init__(self, state, stats, warped, tau_q, kappa_q):
        stats = np.asarray(stats, np.int64).reshape(-1, NSTAT)
        self.state, self.stats, self.warped, self.tau_q, self.kappa_q = state, stats, warped, tau_q, kappa_q
        self.counts, self.abs_error = stats[:, :NSTATE], stats[:, NSTATE]

    def __len__(self):
        return len(self.stats)

    def mean_abs_error(self):
        """(n,) f64: every pair's mean |J - I0| in grey levels over its compared pixels, NaN where it has none"""
        compared = self.counts[:, CONSISTENT] + self.counts[:, MISMATCH]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(compared > 0, self.abs_error / (float(LEVEL) * compared), np.nan)

    def share(self):
        """(n,4) f64: the share of every pair's pixels in each state"""
        return self.counts / self.counts.sum(1, keepdims=True).astype(np.float64)


def _stack(frames, flow):
    from .blobs import _stack_flow
    f = _stack_flow(flow)
    g = np.ascontiguousarray(frames, np.uint8)
    if g.ndim != 3 or g.shape != (f.shape[0] + 1,) + f.shape[1:3]:
        raise ValueError(f"frames should be ({f.shape[0] + 1},{f.shape[1]},{f.shape[2]}) u8 for flow {f.shape}, got shape {g.shape}")
    return g, f


def check(frames, flow, tau=TAU, kappa=KAPPA, warped=False, device=0):
    """frames ((n+1),H,W u8) and flow ((n,)H,W,2 f32; with a single field, two frames): pair t is the flow frame t -> t+1
    on frame t's grid -> Photometric.  tau and kappa default to 8 grey levels and 0.5, a convention: they are not tuned on
    anything here."""
    g, f = _stack(frames, flow)
    tau_q, kappa_q = quantise(tau, kappa)
    n, H, W = f.shape[:3]
    check_args(W, H, n, tau_q, kappa_q)
    state, stats = np.empty((n, H, W), np.uint8), np.empty((n, NSTAT), np.int64)
    out = np.empty((n, H, W), np.uint16) if warped else None
    _check(load().ofc_photo(device, ptr(g), ptr(f), W, H, n, tau_q, kappa_q, ptr(state), ptr(stats), ptr(out)))
    return Photometric(state, stats, out, tau_q, kappa_q)


def check_dev(frames_ptr, flow_ptr, W, H, n, state_ptr, tau_q=2048, kappa_q=128, warped=False, device=0):
    """ofc_photo_dev on frames and a field that are on the device: the state map u8 [n][H][W] stays there, at state_ptr;
    only the stats, and the warped frames when asked for, leave it -> (stats (n,5) int64, warped (n,H,W) u16 or None).
    tau_q, kappa_q: quantise's; the defaults are a convention, not tuned on anything here."""
    check_args(W, H, n, tau_q, kappa_q)
    st = _lib.DeviceBuffer(n * NSTAT * 8, device)
    wd = _lib.DeviceBuffer(n * W * H * 2, device) if warped else None
    try:
        _check(load().ofc_photo_dev(device, C.c_void_p(frames_ptr), C.c_void_p(flow_ptr), W, H, n, tau_q, kappa_q,
                                    C.c_void_p(state_ptr), C.c_void_p(st.ptr), C.c_void_p(wd.ptr) if warped else None))
        return st.download((n, NSTAT), np.int64), wd.download((n, H, W), np.uint16) if warped else None
    finally:
        st.free()
        if wd is not None:
            wd.free()
