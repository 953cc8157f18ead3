"""ClipPipeline.cell_clusters over the bench clip, in one session, after run_kmeans(INIT): ms per call of
ofc_grid_label_counts_dev counts-only (1 B/px read) and with sums (9 B/px read) into preallocated buffers, of the
Python method around it (buffers, the call, the download of the table), and of ofc_flow_weights_dev over the same
field as the yardstick (a plain 12 B/sample stream).  The three alternate over --reps rounds so that drift shows as
spread.  Beside them the route the call replaces: one pair's labels and vectors copied to the host and counted by the
numpy model, scaled to the clip.  One JSON line at the end.  --frames shortens the clip (default: the bench clip)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CLIP_FRAMES, H, INIT, W, auto_batch      # noqa: E402
from opticalflowclustering_amd import _lib, stages      # noqa: E402
from opticalflowclustering_amd.pipeline import ClipPipeline      # noqa: E402
from tests.motion_grid_cases import model_counts      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=CLIP_FRAMES)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--rows", type=int, default=14)
ap.add_argument("--cols", type=int, default=25)
args = ap.parse_args()

pipe = ClipPipeline(W, H, args.frames, batch_pairs=auto_batch(args.frames - 1), n_engines=2)
pipe.synth(0)
pipe.run_flow()
n, P = pipe.n_pairs, W * H
N = n * P
centers, _, _ = pipe.run_kmeans(INIT)
k, cells = len(centers), args.rows * args.cols
lib = _lib.load()
cnt, sm, w32 = _lib.DeviceBuffer(n * cells * k * 4), _lib.DeviceBuffer(n * cells * k * 16), _lib.DeviceBuffer(N * 4)
L, F = C.c_void_p(pipe.labels.ptr), C.c_void_p(pipe.flows.ptr)


def timed(fn):
    """ms per call over --iters calls that each return after the device finished"""
    _lib.check(lib.ofc_device_sync(0))
    t0 = time.perf_counter()
    for _ in range(args.iters):
        fn()
    return 1e3 * (time.perf_counter() - t0) / args.iters


calls = {
    "counts": lambda: _lib.check(lib.ofc_grid_label_counts_dev(0, L, None, W, H, n, args.rows, args.cols, k, C.c_void_p(cnt.ptr), None)),
    "counts_sums": lambda: _lib.check(lib.ofc_grid_label_counts_dev(0, L, F, W, H, n, args.rows, args.cols, k, C.c_void_p(cnt.ptr),
                                                                    C.c_void_p(sm.ptr))),
    "flow_weights": lambda: stages.flow_weights_dev(pipe.flows.ptr, N, "magnitude", 0.0, w32.ptr),
    "method_counts": lambda: pipe.cell_clusters(args.rows, args.cols),
    "method_counts_sums": lambda: pipe.cell_clusters(args.rows, args.cols, sums=True),
}
for fn in calls.values():       # warm every kernel
    fn()
ms = {name: [] for name in calls}
for _ in range(args.reps):
    for name, fn in calls.items():
        ms[name].append(timed(fn))
med = {name: float(np.median(v)) for name, v in ms.items()}

# the host route for one pair (the middle one), and what the device says about the same pair
mid = n // 2
t0 = time.perf_counter()
lab = pipe.labels.download((1, H, W), np.uint8, offset=mid * P)
t_copy_l = 1e3 * (time.perf_counter() - t0)
t0 = time.perf_counter()
flo = pipe.flows.download((1, H, W, 2), np.float32, offset=mid * P * 8)
t_copy_f = 1e3 * (time.perf_counter() - t0)
t0 = time.perf_counter()
mc = model_counts(lab, k, args.rows, args.cols)
t_count = 1e3 * (time.perf_counter() - t0)
t0 = time.perf_counter()
mc2, msums = model_counts(lab, k, args.rows, args.cols, flo)
t_count_sums = 1e3 * (time.perf_counter() - t0)
dc, ds = pipe.cell_clusters(args.rows, args.cols, sums=True)

bytes_per = {"counts": 1, "counts_sums": 9, "flow_weights": 12}
out = {
    "frames": args.frames, "pairs": n, "pixels": N, "k": k, "grid": [args.rows, args.cols], "iters": args.iters,
    "ms": {name: [round(x, 4) for x in v] for name, v in ms.items()}, "ms_median": med,
    "GBps": {name: N * b / 1e6 / med[name] for name, b in bytes_per.items()},
    "ns_per_GB": {name: med[name] * 1e6 / (N * b / 1e9) for name, b in bytes_per.items()},
    "time_per_byte_counts_sums_over_flow_weights": (med["counts_sums"] / 9) / (med["flow_weights"] / 12),
    "host_route_one_pair_ms": {"copy_labels": t_copy_l, "copy_vectors": t_copy_f, "numpy_counts": t_count, "numpy_counts_sums": t_count_sums},
    "host_route_clip_ms": {"counts": (t_copy_l + t_count) * n, "counts_sums": (t_copy_l + t_copy_f + t_count_sums) * n},
    "device_equals_model_on_that_pair": bool(np.array_equal(dc[mid], mc[0]) and np.array_equal(mc2, mc)),
    "largest_sum_difference_on_that_pair": float(np.abs(ds[mid] - msums[0]).max()),
}
print(json.dumps(out), flush=True)
for b in (cnt, sm, w32):
    b.free()
pipe.close()
