"""The cases of test_gpu_flow_iter_schedule.py and tests/golden/make_flow_iter_digests.py: the smallest shapes at which the
store and wait paths of the fused flow iteration's march differ.  numpy only; the inputs are generated, never stored.

  250x190        one column tile plus a sliver; the height is no multiple of 4: two waves of the last step store nothing
  496x264 x 3    every level an exact half: levels 2, 1, 0 start from the x2 upsample; three pairs in one batch (pair map)
  726x414        several strips per tile, each with its own warm-up; rows clamped at both image edges
  499x301 l2     odd width: the per-pixel store path; inexact halves: the general upsample
  322x198 l0 i4  no pyramid: the plain form only, from a zeroed start
  640x360 w13/w5 other window widths (other instantiations)
The batch is also run with the column sums (the form the last level-0 iteration of a clip takes)."""
import hashlib
import json
import os

import numpy as np

from opticalflowclustering_amd import synth

DIGESTS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_iter_digests.json")

# name -> (W, H, frames, FbParams keywords)
CASES = {
    "250x190": (250, 190, 2, {}),
    "496x264_batch3": (496, 264, 4, {}),
    "726x414": (726, 414, 2, {}),
    "499x301_levels2": (499, 301, 2, {"levels": 2}),
    "322x198_levels0_iterations4": (322, 198, 2, {"levels": 0, "iterations": 4}),
    "640x360_winsize13": (640, 360, 2, {"winsize": 13}),
    "640x360_winsize5": (640, 360, 2, {"winsize": 5}),
}
BATCH = "496x264_batch3"
REL_BAR, MAX_BAR = 1e-4, 1e-3          # the project's end-to-end bars against oracle/farneback_ref.c


def frames(name):
    """uint8 [frames][H][W]: a texture under a smooth non-rigid motion that grows with the frame index (every vector of the
    field differs, at every level)"""
    W, H, n, _ = CASES[name]
    p = synth.texture_params(len(name))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    dx = 2.0 * np.sin(2 * np.pi * yy / H) * np.cos(np.pi * xx / W) + 0.6
    dy = 1.2 * np.cos(2 * np.pi * xx / W) - 0.4
    out = np.stack([synth.frame(W, H, t * dx, t * dy, p) for t in range(n)])
    out.setflags(write=False)
    return out


def digest(flow):
    flow = np.ascontiguousarray(flow, np.float32)
    return hashlib.sha256(flow.tobytes()).hexdigest()


def run(name, sums=False):
    """the flows of a case on the GPU, [pairs][H][W][2] float32 (and the two column sums when asked): single pairs through
    FlowEngine.calc, the batch through calc_frames_dev"""
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.flow import FlowEngine
    W, H, n, kw = CASES[name]
    fr = frames(name)
    eng = FlowEngine(W, H, _lib.FbParams(**kw), max_batch=n - 1)
    try:
        if n == 2 and not sums:
            return eng.calc(fr[0], fr[1])[None]
        fd = _lib.DeviceBuffer(fr.nbytes).upload(fr)
        od = _lib.DeviceBuffer((n - 1) * H * W * 8)
        sd = _lib.DeviceBuffer(16)
        _lib.check(_lib.load().ofc_memset(0, od.ptr, 0xFF, od.nbytes))
        _lib.check(_lib.load().ofc_memset(0, sd.ptr, 0xFF, sd.nbytes))
        eng.calc_frames_dev(fd.ptr, n, od.ptr, uv_sum_ptr=sd.ptr if sums else None)
        flows = od.download((n - 1, H, W, 2), np.float32)
        uv = sd.download((2,), np.float64)
        for b in (fd, od, sd):
            b.free()
        return (flows, uv) if sums else flows
    finally:
        eng.close()


def load_digests():
    with open(DIGESTS_PATH) as f:
        return json.load(f)["sha256"]
