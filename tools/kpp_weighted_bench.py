"""The k-means++ seeding with sample weights next to the unit-weight seeding over the bench clip's resident (u,v) field, in
one session: wall ms of the whole call at k = 5 (cluster.kmeans_plusplus_dev: ofc_kpp_seed_dev without weights,
ofc_kpp_seed_dev_w with f32 weights |(u,v)| and with the same values as f64).  Per sample and step the sweep moves 24 B
without weights (X 8, closest read 8 and write 8), 28 B with f32 and 32 B with f64 weights.  The three calls alternate over
--reps rounds after one warm-up round, so that drift shows as spread.  One JSON line at the end.  --frames shortens the clip
(default: the bench clip)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import CLIP_FRAMES, H, K_CLUSTERS, W, auto_batch      # noqa: E402
from opticalflowclustering_amd import _lib, stages      # noqa: E402
from opticalflowclustering_amd.cluster import kmeans_plusplus_dev      # noqa: E402
from opticalflowclustering_amd.pipeline import ClipPipeline      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=CLIP_FRAMES)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

pipe = ClipPipeline(W, H, args.frames, batch_pairs=auto_batch(args.frames - 1), n_engines=2)
pipe.synth(0)
pipe.run_flow()
N = pipe.n_pairs * W * H
colsum = pipe._colsum()

w32 = _lib.DeviceBuffer(N * 4)
stages.flow_weights_dev(pipe.flows.ptr, N, "magnitude", 0.0, w32.ptr)
w64 = _lib.DeviceBuffer(N * 8)
CH = 1 << 26
for o in range(0, N, CH):
    n = min(CH, N - o)
    w64.upload(w32.download((n,), np.float32, offset=o * 4).astype(np.float64), offset=o * 8)

LEGS = {"unit": (None, _lib.F32), "w_f32": (w32.ptr, _lib.F32), "w_f64": (w64.ptr, _lib.F64)}
ms = {k: [] for k in LEGS}
idx = {}
for rep in range(args.reps + 1):
    for name, (wp, wdt) in LEGS.items():
        _lib.check(_lib.load().ofc_device_sync(0))
        t0 = time.perf_counter()
        _, idx[name] = kmeans_plusplus_dev(pipe.flows.ptr, _lib.F32, N, 2, K_CLUSTERS, args.seed, colsum=colsum,
                                           weights_ptr=wp, weight_dtype=wdt)       # returns after the stream synchronised
        if rep:
            ms[name].append(1e3 * (time.perf_counter() - t0))

med = {k: float(np.median(v)) for k, v in ms.items()}
spread = (max(ms["unit"]) - min(ms["unit"])) / med["unit"]
out = {
    "frames": args.frames, "samples": N, "k": K_CLUSTERS, "reps": args.reps,
    "seed_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}, "seed_ms_median": med,
    "unit_spread_rel": spread,
    "ratio_f32_over_unit": med["w_f32"] / med["unit"], "byte_ratio_f32": 28 / 24,
    "ratio_f64_over_unit": med["w_f64"] / med["unit"], "byte_ratio_f64": 32 / 24,
    "within_bar_f32": med["w_f32"] / med["unit"] <= 28 / 24 + spread,
    "within_bar_f64": med["w_f64"] / med["unit"] <= 32 / 24 + spread,
    "indices": {k: [int(i) for i in v] for k, v in idx.items()},
    "same_rows_f32_f64": bool(np.array_equal(idx["w_f32"], idx["w_f64"])),
}
print(json.dumps(out), flush=True)
for b in (w32, w64):
    b.free()
pipe.close()
