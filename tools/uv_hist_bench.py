"""ms per launch of the (u,v) histogram kernel (ofc_bench_uv_hist, bins 1024, range 32) beside the full label-less Lloyd
sweep that reads the same 8 B per vector (ofc_bench_lloyd_sweep what=0), on the bench clip's resident field (299 pairs of
1080p) and on a field of as many uniformly random vectors, where every lane of a wave has its own bin.  Also what the
coherent field looks like to the kernel: non-empty bins, and distinct bins per wave of 64 consecutive vectors (sampled)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import CLIP_FRAMES, H, INIT, W, auto_batch
from opticalflowclustering_amd import _lib, stages
from opticalflowclustering_amd.pipeline import ClipPipeline

BINS, RANGE, REPS, ITERS = 1024, 32.0, 5, 10

pipe = ClipPipeline(W, H, CLIP_FRAMES, batch_pairs=auto_batch(CLIP_FRAMES - 1), n_engines=2)
pipe.synth(0)
pipe.run_flow()
N = pipe.n_pairs * W * H
centers = np.asarray(INIT, np.float64)
mean = np.zeros(2)


def measure(name):
    hist = [stages.bench_uv_hist(pipe.flows.ptr, N, BINS, RANGE, ITERS) for _ in range(REPS)]
    sweep = [stages.bench_lloyd_sweep(pipe.flows.ptr, N, centers, mean, 0, ITERS) for _ in range(REPS)]
    h, s = float(np.median(hist)), float(np.median(sweep))
    print("%s: uv_hist %s ms (median %.3f, %.0f GB/s) | lloyd what=0 %s ms (median %.3f) | ratio %.2f"
          % (name, " ".join("%.3f" % x for x in hist), h, N * 8 / h / 1e6, " ".join("%.3f" % x for x in sweep), s, h / s),
          flush=True)


measure("coherent (synthetic clip, %d vectors)" % N)
h = pipe.uv_histogram(BINS, RANGE)
print("coherent: %d non-empty bins, %d outside, largest bin holds %.1f %% of the vectors"
      % (np.count_nonzero(h.counts), h.outside, 100.0 * h.counts.max() / max(h.n, 1)), flush=True)
P = W * H
sample = pipe.flows.download((4 * P, 2), np.float32, offset=(pipe.n_pairs // 2) * P * 8)
t = np.floor((sample + np.float32(RANGE)) * np.float32(BINS / (2 * RANGE))).astype(np.int64)
b = (t[:, 1] * BINS + t[:, 0]).reshape(-1, 64)
d = np.array([len(np.unique(r)) for r in b[::16]])
print("coherent: distinct bins per wave of 64 vectors (4 frames, every 16th wave): mean %.1f, median %d, max %d, one bin in %.1f %%"
      % (d.mean(), np.median(d), d.max(), 100.0 * (d == 1).mean()), flush=True)

rng = np.random.default_rng(0)
chunk = 1 << 24
for o in range(0, N, chunk):
    m = min(chunk, N - o)
    pipe.flows.upload(rng.uniform(-RANGE, RANGE, (m, 2)).astype(np.float32), offset=o * 8)
measure("uniformly random (%d vectors)" % N)
pipe.close()
