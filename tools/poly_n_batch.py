"""driver for tools/poly_n_profile.sh: one 64-pair 1080p batch (FlowEngine(1920, 1080, params, max_batch=64).calc_frames_dev,
bench.py's launch geometry) per poly_n given, after one warm-up batch; `reps` timed batches each.
usage: python3 tools/poly_n_batch.py [reps] [poly_n ...]      (default: 3 batches, poly_n 5 7; sigma 1.2 for 5, 1.5 for 7)"""
import os
import sys
import time
import ctypes as C

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflowclustering_amd import _lib                                     # noqa: E402
from opticalflowclustering_amd._lib import FbParams, check, load               # noqa: E402
from opticalflowclustering_amd.flow import FlowEngine                          # noqa: E402

W, H, P = 1920, 1080, 64
SIGMA = {5: 1.2, 7: 1.5}
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ns = [int(a) for a in sys.argv[2:]] or [5, 7]
frames = _lib.DeviceBuffer((P + 1) * W * H)
flows = _lib.DeviceBuffer(P * H * W * 8)
check(load().ofc_synth_frames_dev(0, C.c_void_p(frames.ptr), W, H, P + 1, 0, 0))
for n in ns:
    eng = FlowEngine(W, H, FbParams(poly_n=n, poly_sigma=SIGMA[n]), max_batch=P)
    eng.calc_frames_dev(frames.ptr, P + 1, flows.ptr)                          # warm-up
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.calc_frames_dev(frames.ptr, P + 1, flows.ptr)
    ms = (time.perf_counter() - t0) * 1e3 / reps
    print("poly_n=%d sigma=%.1f: %.2f ms per %d-pair batch (host wall clock, synchronised)" % (n, SIGMA[n], ms, P))
    eng.close()
frames.free()
flows.free()
