"""What a model costs the streaming ingest: the configs[4] shape of tools/stream_bench.py (4K grey frames pushed from host
memory through FlowStream, batch_pairs = 8, 14 x 25 grid) without a model and with one (k = 8, counts, and counts + sums),
the variants alternating over --reps rounds in one session on streams that were warmed first.  PCIe-inclusive Mpixels/s
per variant and round, and the difference of the medians.  One JSON line.

    python tools/stream_model_bench.py [frames per pass, default 200] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflowclustering_amd import synth      # noqa: E402
from opticalflowclustering_amd.stream import FlowStream      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("frames", type=int, nargs="?", default=200)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

W, H, n = 3840, 2160, args.frames
p = synth.texture_params(0)
base = [synth.frame(W, H, 0.9 * t, -0.5 * t, p).astype(np.uint8) for t in range(8)]
ang = np.arange(8) * (2 * np.pi / 8)
centres = np.stack([1.3 * np.cos(ang) + 0.4, 1.3 * np.sin(ang) - 0.2], -1)       # k = 8 around the clip's step (0.9, -0.5)
streams = {"no_model": FlowStream(W, H, batch_pairs=8),
           "counts": FlowStream(W, H, batch_pairs=8, centers=centres),
           "counts_sums": FlowStream(W, H, batch_pairs=8, centers=centres, sums=True)}


def one_pass(name):
    fs = streams[name]
    t0 = time.perf_counter()
    for t in range(n):
        fs.push(base[t % 8])
    res = fs.finish() if name == "no_model" else fs.finish_clusters()
    return (n - 1) * W * H / (time.perf_counter() - t0) / 1e6, res


for name in streams:                            # first pass warms up allocations
    one_pass(name)
mpx = {name: [] for name in streams}
for _ in range(args.reps):
    for name in streams:
        rate, res = one_pass(name)
        mpx[name].append(rate)
med = {name: float(np.median(v)) for name, v in mpx.items()}
print(json.dumps({
    "frames": n, "pairs": n - 1, "width": W, "height": H, "batch_pairs": 8, "k": len(centres),
    "mpx_s": {name: [round(x, 1) for x in v] for name, v in mpx.items()}, "mpx_s_median": med,
    "ms_per_frame_median": {name: W * H / 1e3 / med[name] for name in med},
    "model_costs_percent": {name: 100 * (1 - med[name] / med["no_model"]) for name in ("counts", "counts_sums")},
}), flush=True)
for fs in streams.values():
    fs.close()
