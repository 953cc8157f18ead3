"""winsize sweep of the flow engine: one 1080p engine per window (FlowEngine(1920, 1080, FbParams(winsize=ws),
max_batch=64)) over 65 resident synthetic frames (ofc_synth_frames_dev), `warmup` untimed batches, then `reps` batches
timed one by one (host wall clock around a synchronised calc_frames_dev).  One JSON line per window: median / min / max ms
per 64-pair batch and the median per pair.  winsize 15 runs the fused k_flow_iter, 17 k_box_solve<8>, 19 and wider
k_box_solve_wide (the staged kernels).
usage: python3 tools/winsize_bench.py [--reps N] [--warmup N] [ws ...]      (default: 10 reps, 2 warm-up, 15 17 19 31 61
127 255)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflowclustering_amd import _lib                                     # noqa: E402
from opticalflowclustering_amd._lib import FbParams, check, load               # noqa: E402
from opticalflowclustering_amd.flow import FlowEngine                          # noqa: E402

W, H, P = 1920, 1080, 64
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("ws", type=int, nargs="*", default=[15, 17, 19, 31, 61, 127, 255])
args = ap.parse_args()
frames = _lib.DeviceBuffer((P + 1) * W * H)
flows = _lib.DeviceBuffer(P * H * W * 8)
check(load().ofc_synth_frames_dev(0, C.c_void_p(frames.ptr), W, H, P + 1, 0, 0))
for ws in args.ws:
    eng = FlowEngine(W, H, FbParams(winsize=ws), max_batch=P)
    for _ in range(args.warmup):
        eng.calc_frames_dev(frames.ptr, P + 1, flows.ptr)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        eng.calc_frames_dev(frames.ptr, P + 1, flows.ptr)               # synchronised
        ts.append((time.perf_counter() - t0) * 1e3)
    eng.close()
    ts.sort()
    med = ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])
    print(json.dumps({"winsize": ws, "W": W, "H": H, "pairs": P, "reps": args.reps, "warmup": args.warmup,
                      "ms_per_batch_median": round(med, 3), "ms_per_batch_min": round(ts[0], 3),
                      "ms_per_batch_max": round(ts[-1], 3), "ms_per_pair_median": round(med / P, 4)}), flush=True)
frames.free()
flows.free()
