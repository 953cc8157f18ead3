"""Farneback flow engine (libofc ofc_flow_*): the device-side replacement of
cv2.calcOpticalFlowFarneback as called at computeOpticalFlowModule.py:20-22, and calcOpticalFlowFarneback itself
with cv2's call shape."""
import ctypes as C
import threading
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import FbParams, check, load, ptr


class FlowEngine:
    """one engine per (device, resolution); owns all device scratch for `max_batch` frame pairs"""

    def __init__(self, W, H, params=None, max_batch=1, device=0):
        self.W, self.H, self.device, self.max_batch = int(W), int(H), device, int(max_batch)
        self.params = params or FbParams()
        h = C.c_void_p()
        check(load().ofc_flow_create(device, self.W, self.H, C.byref(self.params), self.max_batch, C.byref(h)))
        self._h = h

    def calc(self, prev_gray, next_gray, out=None):
        """one isolated pair, host arrays -> HxWx2 float32 (u = x-displacement, v = y-displacement); `out`: a
        C-contiguous HxWx2 float32 array to write the flow into (returned)"""
        prev_gray = np.ascontiguousarray(prev_gray, np.uint8)
        next_gray = np.ascontiguousarray(next_gray, np.uint8)
        if prev_gray.shape != (self.H, self.W) or next_gray.shape != (self.H, self.W):
            raise ValueError(f"expected two {self.H}x{self.W} uint8 images")
        if out is None:
            out = np.empty((self.H, self.W, 2), np.float32)
        elif not _is_flow_buffer(out, self.H, self.W):
            raise ValueError(f"out must be a writeable C-contiguous {self.H}x{self.W}x2 float32 array")
        check(load().ofc_flow_calc(self._h, ptr(prev_gray), ptr(next_gray), ptr(out)))
        return out

    def push(self, gray):
        """streaming: returns None for the first frame, then the flow prev->gray"""
        gray = np.ascontiguousarray(gray, np.uint8)
        if gray.shape != (self.H, self.W):
            raise ValueError(f"expected a {self.H}x{self.W} uint8 image")
        flow = np.empty((self.H, self.W, 2), np.float32)
        rc = load().ofc_flow_push_gray(self._h, ptr(gray), ptr(flow))
        if rc == _lib.OFC_ENOTREADY:
            return None
        check(rc)
        return flow

    def calc_frames_dev(self, frames_ptr, n_frames, flow_ptr, sync=True, uv_sum_ptr=None):
        """device pointers: n_frames resident u8 frames -> n_frames-1 flows (async unless sync); uv_sum_ptr: device address
        of two doubles that receive sum(u), sum(v) of those flows (from the last iteration's epilogue)"""
        if uv_sum_ptr:
            check(load().ofc_flow_calc_frames_dev_stats(self._h, C.c_void_p(frames_ptr), n_frames, C.c_void_p(flow_ptr),
                                                        C.c_void_p(uv_sum_ptr)))
        else:
            check(load().ofc_flow_calc_frames_dev(self._h, C.c_void_p(frames_ptr), n_frames, C.c_void_p(flow_ptr)))
        if sync:
            self.sync()

    def calc_frames_dev_bidir(self, frames_ptr, n_frames, fwd_ptr, bwd_ptr, sync=True, uv_sum_ptr=None):
        """device pointers: n_frames resident u8 frames -> n_frames-1 forward flows at fwd_ptr and n_frames-1 backward flows
        at bwd_ptr from one front end (ofc_flow_calc_frames_dev_bidir): bwd[t] is the flow from frame t+1 to frame t, stored
        at t (consistency.check_dev takes it with bwd_reversed=False).  The buffers may not overlap.  uv_sum_ptr: device
        address of two doubles that receive sum(u), sum(v) of the forward flows"""
        if uv_sum_ptr:
            check(load().ofc_flow_calc_frames_dev_bidir_stats(self._h, C.c_void_p(frames_ptr), n_frames, C.c_void_p(fwd_ptr),
                                                              C.c_void_p(bwd_ptr), C.c_void_p(uv_sum_ptr)))
        else:
            check(load().ofc_flow_calc_frames_dev_bidir(self._h, C.c_void_p(frames_ptr), n_frames, C.c_void_p(fwd_ptr),
                                                        C.c_void_p(bwd_ptr)))
        if sync:
            self.sync()

    def sync(self):
        check(load().ofc_flow_sync(self._h))

    def front_overlap(self):
        """True when the engine runs the coarse levels' front end on a side stream beside the level-0 expansion, False when
        it runs the levels in series (OFC_FLOW_FRONT_OVERLAP=0 or OFC_FLOW_GRAPH=1 at creation, no coarse level, or per-level
        scratch beyond 1.5 x the shared buffers); the results are the same bits either way"""
        on = C.c_int(-1)
        check(load().ofc_flow_front_overlap(self._h, C.byref(on)))
        return bool(on.value)

    def pyramid_fused(self):
        """True when one launch per batch writes the level images of all coarse levels (overlap on, at most three coarse
        levels, all exact decimations, OFC_PYRAMID_FUSED=0 not set at creation); the images are the same bits either way"""
        on = C.c_int(-1)
        check(load().ofc_flow_pyramid_fused(self._h, C.byref(on)))
        return bool(on.value)

    def close(self):
        if getattr(self, "_h", None):
            load().ofc_flow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _is_flow_buffer(a, H, W):
    return (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (H, W, 2)
            and a.flags.c_contiguous and a.flags.writeable)


# ---- cv2.calcOpticalFlowFarneback ----
OPTFLOW_USE_INITIAL_FLOW = 4        # cv2's flag values; neither is implemented: the library refuses both
OPTFLOW_FARNEBACK_GAUSSIAN = 256

_FB_CACHE_MAX = 4                   # engines kept alive (each owns its device scratch); least recently used goes first
_fb_engines = OrderedDict()         # (device, W, H, parameters) -> FlowEngine
_fb_lock = threading.Lock()         # engine handles are not thread-safe (ofc.h)


def _gray_arg(a, name):
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError(f"{name} must be a 2-D uint8 array (one grey frame)")
    return np.ascontiguousarray(a)


def calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags,
                             device=0):
    """cv2.calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    on the GPU.  prev / next: HxW uint8 frames.  Returns the HxWx2 float32 flow: written into `flow` (and that object
    returned) when it is a writeable C-contiguous HxWx2 float32 array, a new array otherwise.  winsize odd, 5 .. 255
    (wider raises OfcError OFC_EUNSUPPORTED, even OFC_EINVAL); poly_n 5 or 7; flags must be 0
    (OPTFLOW_USE_INITIAL_FLOW / OPTFLOW_FARNEBACK_GAUSSIAN raise OfcError OFC_EUNSUPPORTED).  One engine per (device,
    size, parameters) is kept between calls; parameters the library refuses leave none behind."""
    prev = _gray_arg(prev, "prev")
    next = _gray_arg(next, "next")
    if prev.shape != next.shape:
        raise ValueError(f"prev {prev.shape} and next {next.shape} differ in shape")
    H, W = prev.shape
    out = flow if _is_flow_buffer(flow, H, W) else np.empty((H, W, 2), np.float32)
    key = (int(device), W, H, float(pyr_scale), int(levels), int(winsize), int(iterations), int(poly_n),
           float(poly_sigma), int(flags))
    with _fb_lock:
        eng = _fb_engines.get(key)
        if eng is None:
            eng = FlowEngine(W, H, FbParams(*key[3:]), max_batch=1, device=key[0])
            _fb_engines[key] = eng
            while len(_fb_engines) > _FB_CACHE_MAX:
                _fb_engines.popitem(last=False)[1].close()
        else:
            _fb_engines.move_to_end(key)
        eng.calc(prev, next, out)
    return out


def clear_farneback_cache():
    """close the engines calcOpticalFlowFarneback keeps (frees their device memory)"""
    with _fb_lock:
        while _fb_engines:
            _fb_engines.popitem()[1].close()
