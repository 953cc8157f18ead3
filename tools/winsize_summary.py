"""level-0 kernel times per window from the rocprofv3 kernel traces tools/winsize_profile.sh writes (one output directory
per winsize, each holding tools/winsize_bench.py's 64-pair 1080p batches).  Level 0 = the launches of a kernel with the
largest grid (k_flow_iter, which winsize 15 runs, launches the same persistent grid at every level, so its row keeps
only the per-batch total).  Per window: the median per-launch time of the level-0 box-mean/solve kernel (k_flow_iter at winsize <= 15,
where update-matrices is fused in) and of k_update_matrices, their sum per iteration, the box kernel's bandwidth at its
28 B/px algorithmic traffic (20 B of M read, 8 B of flow written) and its fraction of the 8 TB/s HBM peak, and the GPU time
per batch (all kernels).
usage: python3 tools/winsize_summary.py <dir of winsize_<ws> trace dirs> [out.csv]"""
import csv
import glob
import os
import re
import sys
from collections import defaultdict

PEAK = 8.0e12
BATCHES = 4                     # winsize_profile.sh: 1 warm-up + 3 timed batches per window
out = []
for d in [p for p in glob.glob(os.path.join(sys.argv[1], "winsize_*")) if os.path.isdir(p)]:
    ws = int(re.search(r"winsize_(\d+)$", d).group(1))
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not f:
        continue
    per = defaultdict(list)
    total = 0.0
    for r in csv.DictReader(open(f[0])):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        total += us
        grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
        name = r["Kernel_Name"]
        kind = ("box" if re.search(r"k_box_solve|k_flow_iter", name) else "um" if "k_update_matrices" in name else None)
        if kind:
            per[kind].append((grid, us, re.sub(r"\(.*", "", name)))
    row = dict(winsize=ws)
    for kind in ("box", "um"):
        if not per[kind] or ws <= 15:
            row[kind + "_kernel"], row[kind + "_l0_launches"], row[kind + "_l0_us"] = "", 0, 0.0
            continue
        g0 = max(g for g, _, _ in per[kind])
        ts = sorted(us for g, us, _ in per[kind] if g == g0)
        row[kind + "_kernel"] = [n for g, _, n in per[kind] if g == g0][0]
        row[kind + "_l0_launches"] = len(ts)
        row[kind + "_l0_us"] = round(ts[len(ts) // 2], 1)
    row["l0_us_per_iteration"] = round(row["box_l0_us"] + row["um_l0_us"], 1) if ws > 15 else ""
    px = 1920 * 1080 * 64
    row["box_GBps"] = round(28 * px / (row["box_l0_us"] * 1e-6) / 1e9, 1) if ws > 15 else ""
    row["box_frac_of_8TBps"] = round(28 * px / (row["box_l0_us"] * 1e-6) / PEAK, 3) if ws > 15 else ""
    row["gpu_ms_per_batch"] = round(total / BATCHES / 1e3, 2)
    out.append(row)
out.sort(key=lambda r: r["winsize"])
w = csv.DictWriter(open(sys.argv[2], "w", newline="") if len(sys.argv) > 2 else sys.stdout, fieldnames=list(out[0]))
w.writeheader()
w.writerows(out)
