"""Applying a model to the resident bench clip, in one session, after run_flow(): ms per call of
  (a) the two-pass route: ClipPipeline.assign(C) then cell_clusters() -- labels written (8 B/px read, 1 written), then
      counted (1 B/px read, 9 with sums): 10 B/px, 18 with sums;
  (b) the fused route: cell_clusters(centers=C) -- ofc_grid_assign_counts_dev, 8 B/px read, nothing written per pixel;
  (c) ofc_flow_weights_dev over the same field, the per-byte yardstick (a plain 12 B/sample stream).
All five alternate over --reps rounds in one process so that drift shows as spread; every figure is the mean of --iters
calls that each return after the device finished.  (a) and (b) are the Python methods, so both carry their buffers, the
column mean and the download of the table.  One JSON line at the end.  --frames shortens the clip (default: the bench
clip)."""
import argparse
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
centres = np.asarray(INIT, np.float64)          # k = 5: the bench's initial centres serve as the model
lib = _lib.load()
w32 = _lib.DeviceBuffer(N * 4)


def timed(fn):
    """ms per call over --iters calls that each return after the device finished"""
    _lib.check(lib.ofc_device_sync(0))
    t0 = time.perf_counter()
    for _ in range(args.iters):
        fn()
    return 1e3 * (time.perf_counter() - t0) / args.iters


def route(sums):
    pipe.assign(centres)
    return pipe.cell_clusters(args.rows, args.cols, sums=sums)


calls = {
    "route": lambda: route(False),
    "fused": lambda: pipe.cell_clusters(args.rows, args.cols, centers=centres),
    "route_sums": lambda: route(True),
    "fused_sums": lambda: pipe.cell_clusters(args.rows, args.cols, sums=True, centers=centres),
    "flow_weights": lambda: stages.flow_weights_dev(pipe.flows.ptr, N, "magnitude", 0.0, w32.ptr),
}
first = {name: fn() for name, fn in calls.items()}       # warm every kernel, and keep what the routes say
ms = {name: [] for name in calls}
for _ in range(args.reps):
    for name, fn in calls.items():
        ms[name].append(timed(fn))
med = {name: float(np.median(v)) for name, v in ms.items()}
spread = {name: [float(min(v)), float(max(v))] for name, v in ms.items()}

same_counts = bool(np.array_equal(first["route"], first["fused"]) and np.array_equal(first["route_sums"][0], first["fused_sums"][0]))
same_sums = bool(np.array_equal(first["route_sums"][1].view(np.int64), first["fused_sums"][1].view(np.int64)))
out = {
    "frames": args.frames, "pairs": n, "pixels": N, "k": len(centres), "grid": [args.rows, args.cols], "iters": args.iters,
    "ms": {name: [round(x, 4) for x in v] for name, v in ms.items()}, "ms_median": med, "ms_min_max": spread,
    "fused_over_route": {"counts": med["fused"] / med["route"], "counts_sums": med["fused_sums"] / med["route_sums"]},
    "fused_not_slower": {"counts": med["fused"] <= med["route"], "counts_sums": med["fused_sums"] <= med["route_sums"]},
    "GBps_at_8_B_per_px": {name: N * 8 / 1e6 / med[name] for name in ("fused", "fused_sums")},
    "GBps_flow_weights_at_12_B": N * 12 / 1e6 / med["flow_weights"],
    "time_per_byte_over_flow_weights": {name: (med[name] / 8) / (med["flow_weights"] / 12) for name in ("fused", "fused_sums")},
    "fused_equals_route": {"counts": same_counts, "sums_bits": same_sums},
}
print(json.dumps(out), flush=True)
w32.free()
pipe.close()
