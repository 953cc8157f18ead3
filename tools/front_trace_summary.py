"""Front-end figures per flow batch ("Front end beside the level-0 expansion") from kernel traces of
bench.py at 1080p, where a batch's front end is 7 launches (three k_level_dec, three k_polyexp<0,false>, one
k_polyexp<0,true>) or, with the level images from one launch, 5 (k_pyramid_dec in place of the three k_level_dec), taken in
dispatch order: `rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py
--steps 5 --warmup 2 [--engines 1]`, one directory per run.  Medians over the batches of the timed steps (the first 2/7 of the
batches are the warm-up).  profiles/frontoverlap_trace_summary.txt was written from its output.
usage: front_trace_summary.py label=DIR ..."""
import csv
import glob
import gzip
import re
import statistics as st
import sys

FRONT = re.compile(r"k_level_dec<|k_pyramid_dec<|k_polyexp<")
U8 = re.compile(r"k_polyexp<0,\s*true")


def short(n):
    m = re.search(r"(k_level_dec<[^>]*>|k_pyramid_dec<[^>]*>|k_polyexp<[^>]*>)", n)
    return m.group(1).replace(" ", "") if m else n[:30]


def load(d):
    f = glob.glob(d + "/**/*kernel_trace.csv*", recursive=True)[0]
    rows = list(csv.DictReader(gzip.open(f, "rt") if f.endswith(".gz") else open(f)))
    key = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Correlation_Id"
    rows.sort(key=lambda r: int(r[key]))
    return rows


def union_len(iv):
    iv = sorted(iv)
    tot, cs, ce = 0, None, None
    for s, e in iv:
        if ce is None or s > ce:
            if ce is not None:
                tot += ce - cs
            cs, ce = s, e
        else:
            ce = max(ce, e)
    return tot + (ce - cs if ce is not None else 0)


def overlap_with(iv, a, b):
    return union_len([(max(s, a), min(e, b)) for s, e in iv if min(e, b) > max(s, a)])


for arg in sys.argv[1:]:
    label, d = arg.split("=")
    rows = load(d)
    fe = [(short(r["Kernel_Name"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Stream_Id", r.get("Queue_Id", "?")))
          for r in rows if FRONT.search(r["Kernel_Name"])]
    per_batch = 5 if any("k_pyramid_dec" in k[0] for k in fe) else 7
    groups = [fe[i:i + per_batch] for i in range(0, len(fe) - per_batch + 1, per_batch)]
    bad = [i for i, g in enumerate(groups) if sum(1 for k in g if U8.search(k[0])) != 1]
    print(f"== {label}: {len(rows)} dispatches, {len(fe)} front-end launches, {len(groups)} batches, {len(bad)} irregular groups; "
          f"streams/queues of the front end: {sorted({k[3] for k in fe})}")
    if bad:
        print("   first irregular group:", [k[0] for k in groups[bad[0]]])
        continue
    groups = groups[len(groups) * 2 // 7:]          # drop the two warm-up steps of seven
    span, busy, summ, ovl, u8, side_span = [], [], [], [], [], []
    per = {}
    for g in groups:
        u = [k for k in g if U8.search(k[0])][0]
        side = [(k[1], k[2]) for k in g if k is not u]
        span.append((max(k[2] for k in g) - min(k[1] for k in g)) / 1e3)
        busy.append(union_len([(k[1], k[2]) for k in g]) / 1e3)
        summ.append(sum(k[2] - k[1] for k in g) / 1e3)
        ovl.append(overlap_with(side, u[1], u[2]) / 1e3)
        u8.append((u[2] - u[1]) / 1e3)
        side_span.append((max(e for _, e in side) - min(s for s, _ in side)) / 1e3)
        for k in g:
            per.setdefault(k[0], []).append((k[2] - k[1]) / 1e3)
    med = st.median
    print(f"   per batch, median over {len(groups)} batches (us): front-end kernels' sum {med(summ):.1f}, union of their intervals {med(busy):.1f}, "
          f"first start to last end {med(span):.1f}")
    # a step's batches differ in size (bench.py: 299 pairs in 5 batches), so the batch-to-batch range is taken per position
    # in the step
    for pos in range(5):
        b = busy[pos::5]
        print(f"   union, batch {pos} of a step: median {med(b):.1f}, min {min(b):.1f}, max {max(b):.1f}, range {max(b) - min(b):.1f}  n {len(b)}")
    print(f"   coarse chain ({per_batch - 4} level-image launch(es) + 3 expansions): first start to last end {med(side_span):.1f}; of it inside the level-0 expansion's interval {med(ovl):.1f}")
    print(f"   level-0 expansion k_polyexp<0,true>: {med(u8):.1f} (min {min(u8):.1f}, max {max(u8):.1f})")
    for k, v in sorted(per.items()):
        print(f"     {k:34s} median {med(v):7.1f}  min {min(v):7.1f}  max {max(v):7.1f}  n {len(v)}")
    # whole-step view: all kernels, per-kernel exclusive totals per step over the timed steps
    tot = {}
    for r in rows:
        n = r["Kernel_Name"]
        m = re.search(r"(k_\w+)", n)
        tot.setdefault(m.group(1) if m else n[:24], 0)
        tot[m.group(1) if m else n[:24]] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    top = sorted(tot.items(), key=lambda kv: -kv[1])[:6]
    print("   kernel time summed over the run (ms): " + ", ".join(f"{k} {v / 1e6:.1f}" for k, v in top))
