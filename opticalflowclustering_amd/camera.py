"""Per-pair camera motion: fit a translation or an affine model to a frame pair's flow field and remove it
(csrc/motion_model.hip; include/ofc.h has the definition).  Everything after the flow -- the clip-wide Lloyd fit and its
'moving' / 'magnitude' weights, the (u,v) histogram, a stream's model -- assumes a fixed camera; on hand-held or panning
footage the background moves, and these calls give them the field they assume.

The model is about the frame centre: u^ = p0 + p1 X/2 + p2 Y/2, v^ = p3 + p4 X/2 + p5 Y/2 with X = 2x - (W-1),
Y = 2y - (H-1).  It is fitted by least squares over every valid vector (finite, |u|, |v| < 1024), then re-fitted over the
vectors within thresholds[t] px of the model of the round before, once per threshold.  The default thresholds
(4.0, 2.0, 1.0) are a guess: they were not tuned on any footage."""
import collections
import ctypes as C

import numpy as np

from ._lib import check, load, ptr

KINDS = {"translation": 1, "affine": 2}
DEFAULT_THRESHOLDS = (4.0, 2.0, 1.0)     # px; a guess, not tuned on any footage
MAX_ROUNDS = 8
NMOM = 13

CameraMotion = collections.namedtuple("CameraMotion", "params status inliers outside")
CameraMotion.__doc__ = """params (n,6) f64: p0..p5 per pair; status (n,) int32: 0 every round solved, 1 a later round could
not be and params are the round before's, 2 round 0 could not be and params are zeros; inliers (n,) int64: the pixels the
model was solved from; outside (n,) int64: the pair's vectors that are not valid"""


def camera_args(model, thresholds=DEFAULT_THRESHOLDS):
    """-> (kind, thresholds as a C-contiguous f64 array, T), checked as the library checks them"""
    if model not in KINDS:
        raise ValueError(f"model should be 'translation' or 'affine', got {model!r}")
    thr = np.ascontiguousarray(thresholds, np.float64).reshape(-1)
    if len(thr) > MAX_ROUNDS:
        raise ValueError(f"{len(thr)} thresholds, at most {MAX_ROUNDS}")
    if not (np.isfinite(thr).all() and (thr > 0).all()):
        raise ValueError(f"thresholds must be finite and positive, got {tuple(thr)}")
    return KINDS[model], thr, len(thr)


def parse_camera(camera):
    """None | 'translation' | 'affine' | (kind, thresholds) -> None or (model, thresholds)"""
    if camera is None or camera == "none":
        return None
    model, thr = (camera, DEFAULT_THRESHOLDS) if isinstance(camera, str) else camera
    camera_args(model, thr)
    return model, tuple(float(t) for t in thr)


def solve(moments, model="affine"):
    """the library's least-squares solve on thirteen integer moments (ofc_motion_solve; host only, the function the kernel
    runs) -> (p (6,) f64, status: 0 solved, 1 not)"""
    m = np.ascontiguousarray(moments, np.int64)
    if m.shape != (NMOM,) or model not in KINDS:
        raise ValueError(f"solve takes {NMOM} moments and 'translation' or 'affine'")
    p, st = np.zeros(6), C.c_int()
    check(load().ofc_motion_solve(ptr(m), KINDS[model], ptr(p), C.byref(st)))
    return p, st.value


def motion_launch_geometry(W, H, npair=1):
    """(groups, per, used, last): the work-groups per pair of the moment kernel and the subtraction over npair fields of
    W x H, the 2048-vector shares each takes, the groups that get at least one share, and the shares of the last of those
    (ofc_motion_launch_geometry); needs no device"""
    out = (C.c_int * 4)()
    check(load().ofc_motion_launch_geometry(W, H, npair, out))
    return tuple(out)


def motion_from_history(params, status, moments, model):
    """CameraMotion from a fit's outputs and its moment history (T+1, n, 13): the inliers are the n of the last round that
    solved, which the host solve decides as the device did"""
    n = len(status)
    inliers = np.zeros(n, np.int64)
    for i in range(n):
        for m in moments[:, i]:
            if solve(m, model)[1] != 0:
                break
            inliers[i] = m[0]
    return CameraMotion(params, status, inliers, moments[0, :, 12].copy())


def _stack(flow):
    flow = np.ascontiguousarray(flow, np.float32)
    if flow.ndim == 3:
        flow = flow[None]
    if flow.ndim != 4 or flow.shape[3] != 2 or flow.shape[0] < 1:
        raise ValueError(f"flow should be (H,W,2) or (n,H,W,2), got shape {flow.shape}")
    return flow


def _fit(flow, model, thresholds, device, residual):
    f = _stack(flow)
    n, H, W = f.shape[:3]
    kind, thr, T = camera_args(model, thresholds)
    params, status = np.zeros((n, 6)), np.zeros(n, np.int32)
    moments = np.zeros((T + 1, n, NMOM), np.int64)
    if residual:
        out = np.empty_like(f)
        check(load().ofc_motion_compensate(device, ptr(f), W, H, n, kind, ptr(thr), T, ptr(out), ptr(params), ptr(status),
                                           None, ptr(moments)))
    else:
        out = None
        check(load().ofc_motion_fit(device, ptr(f), W, H, n, kind, ptr(thr), T, ptr(params), ptr(status), None, ptr(moments)))
    return out, motion_from_history(params, status, moments, model)


def estimate_camera_motion(flow, model="affine", thresholds=DEFAULT_THRESHOLDS, device=0):
    """flow (H,W,2) or (n,H,W,2) f32 -> CameraMotion, one row per pair (ofc_motion_fit).  model: 'translation' or 'affine'.
    thresholds: up to 8 inlier radii in px, one re-fit each; () fits once over every valid vector.  The default
    (4.0, 2.0, 1.0) is a guess and was not tuned on any footage."""
    return _fit(flow, model, thresholds, device, False)[1]


def compensate(flow, model="affine", thresholds=DEFAULT_THRESHOLDS, device=0):
    """-> (residual, CameraMotion): the field minus every pair's fitted model (ofc_motion_compensate), in the shape it came
    in.  Vectors with a non-finite component pass through unchanged."""
    out, cm = _fit(flow, model, thresholds, device, True)
    return (out[0] if np.ndim(flow) == 3 else out), cm


def evaluate(params, W, H):
    """the field a model describes: params (6,) -> (H,W,2) f64, (n,6) -> (n,H,W,2).  Plain numpy: each product and sum is
    rounded on its own, where the device runs one fma chain, so the two may differ in the last bit."""
    p = np.asarray(params, np.float64)
    if p.shape[-1:] != (6,) or p.ndim not in (1, 2):
        raise ValueError(f"params should be (6,) or (n,6), got shape {p.shape}")
    q = p.reshape(-1, 6)[:, :, None, None]
    hx = (0.5 * (2 * np.arange(W) - (W - 1)))[None, None, :]
    hy = (0.5 * (2 * np.arange(H) - (H - 1)))[None, :, None]
    out = np.stack([q[:, 0] + q[:, 1] * hx + q[:, 2] * hy, q[:, 3] + q[:, 4] * hx + q[:, 5] * hy], -1)
    return out[0] if p.ndim == 1 else out
