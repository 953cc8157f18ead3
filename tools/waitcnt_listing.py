#!/usr/bin/env python3
"""Condense one kernel's assembly to its synchronisation skeleton: every s_waitcnt, s_barrier and s_setprio in program order,
with the labels and branch targets that give the loops their shape, and between them the COUNTS of global loads, global
stores, LDS instructions and everything else.  What it is for: seeing which outstanding memory operations a wait at a loop
head covers ("Waits that reach into the stores").

    hipcc <the Makefile's CXXFLAGS> -S --cuda-device-only flow_iter.hip -o flow_iter.s
    python tools/waitcnt_listing.py flow_iter.s 'k_flow_iterILi7ELi0ELb0ELb0E'

The second argument is a substring of the kernel's (mangled) symbol; the assembly is the compiler's -S output.  The kernel's
register and occupancy figures (.vgpr_count, .vgpr_spill_count, .private_segment_fixed_size of its metadata record) are printed
under the listing."""
import re
import sys


def kernel_body(lines, key):
    """the instruction lines of the first function whose label contains `key`"""
    start = None
    for i, ln in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if m and key in m.group(1) and not m.group(1).startswith("."):
            start, sym = i + 1, m.group(1)
            break
    if start is None:
        sys.exit("no function label contains %r" % key)
    body = []
    for ln in lines[start:]:
        if ln.startswith(".Lfunc_end"):
            break
        body.append(ln)
    return sym, body


def classify(op):
    if op.startswith("global_load"):
        return "gload"
    if op.startswith("global_store"):
        return "gstore"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def listing(body):
    out, counts = [], {"gload": 0, "gstore": 0, "lds": 0, "other": 0}

    def flush():
        if any(counts.values()):
            out.append("    [%s]" % ", ".join("%d %s" % (counts[k], k) for k in ("gload", "gstore", "lds", "other") if counts[k]))
            for k in counts:
                counts[k] = 0

    for ln in body:
        s = ln.split(";")[0].strip()
        if not s or s.startswith((".", "//")) and not s.startswith(".LBB"):
            continue
        if s.startswith(".LBB") and s.endswith(":"):
            flush()
            out.append(s)
            continue
        op = s.split()[0]
        if op in ("s_waitcnt", "s_barrier", "s_setprio"):
            flush()
            out.append("  " + " ".join(s.split()))
        elif ".LBB" in s:                   # a branch: it counts as an instruction and its target is shown
            counts["other"] += 1
            flush()
            out.append("    -> " + s.split()[-1])
        else:
            counts[classify(op)] += 1
    flush()
    return out


def metadata(lines, sym):
    """the figures of the kernel's record in the amdhsa metadata"""
    want = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
            ".group_segment_fixed_size", ".max_flat_workgroup_size")
    rec, recs = {}, []
    for ln in lines:
        s = ln.strip()
        if s.startswith("- .") or s.startswith("- .args"):
            if rec:
                recs.append(rec)
            rec = {}
            s = s[2:]
        m = re.match(r"^(\.\w+):\s*(\S+)$", s)
        if m:
            rec[m.group(1)] = m.group(2)
    if rec:
        recs.append(rec)
    for r in recs:
        if r.get(".name") == sym:
            return {k: r[k] for k in want if k in r}
    return {}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with open(sys.argv[1]) as f:
        lines = f.read().splitlines()
    sym, body = kernel_body(lines, sys.argv[2])
    print("kernel", sym)
    print("\n".join(listing(body)))
    md = metadata(lines, sym)
    if md:
        print("metadata", " ".join("%s=%s" % (k[1:], v) for k, v in md.items()))
        v = int(md.get(".vgpr_count", 0)) + 0
        if v:
            # gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8 (the unified file; AGPRs count)
            alloc = -(-v // 8) * 8
            print("waves_per_simd_by_vgprs", min(8, 512 // alloc))


if __name__ == "__main__":
    main()
