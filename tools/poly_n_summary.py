"""per-image time of every k_polyexp form in a rocprofv3 kernel trace of tools/poly_n_batch.py, per pyramid level, and
the poly_n=7 / poly_n=5 ratio.  usage: python3 tools/poly_n_summary.py <rocprofv3 output dir> [out.csv]"""
import csv
import glob
import re
import sys
from collections import defaultdict

rows = list(csv.DictReader(open(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0])))
acc = defaultdict(list)
for r in rows:
    m = re.search(r"k_polyexp<(\d+), (true|false), (true|false), (\d+)>", r["Kernel_Name"])
    if not m:
        continue
    form = "u8in" if m.group(2) == "true" else "f32"
    tiles_x = int(r["Grid_Size_X"]) // int(r.get("Workgroup_Size_X", 256))   # 240-column strips: 8, 4, 2, 1 at 1080p levels 0..3
    acc[(form, int(m.group(4)), tiles_x, int(r["Grid_Size_Z"]))].append(
        (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
out = []
for (form, n, tx, nimg), d in sorted(acc.items(), key=lambda kv: (kv[0][0], -kv[0][2], kv[0][1])):
    d = sorted(d)
    out.append(dict(form=form, poly_n=n, tiles_x=tx, images=nimg, launches=len(d), median_us=round(d[len(d) // 2], 2),
                    us_per_image=round(d[len(d) // 2] / nimg, 3)))
for o in out:
    five = [p for p in out if p["form"] == o["form"] and p["tiles_x"] == o["tiles_x"] and p["poly_n"] == 5]
    o["ratio_to_poly5"] = round(o["us_per_image"] / five[0]["us_per_image"], 3) if five else ""
w = csv.DictWriter(open(sys.argv[2], "w", newline="") if len(sys.argv) > 2 else sys.stdout, fieldnames=list(out[0]))
w.writeheader()
w.writerows(out)
