#!/usr/bin/env python3
"""Say whether two sets of device assembly hold the same kernels: per mangled kernel name, the instruction stream (comments
stripped, local .L labels renumbered in order of appearance) and the .amdhsa_* descriptor lines (register counts, LDS and
private segment sizes among them).  For refactors that move kernels between files and must not change an instruction.

    hipcc <the Makefile's CXXFLAGS> -S --cuda-device-only flow_iter.hip -o new/flow_iter.s        (and so on, both sides)
    python tools/kernel_asm_equal.py old/*.s -- new/*.s

Exit status 1 on any difference, or on a kernel that only one side has."""
import re
import sys


def kernels(paths):
    """{kernel name: (instruction lines, descriptor lines)} of the compiler's -S outputs"""
    out = {}
    for path in paths:
        lines = [ln.split(";")[0].strip() for ln in open(path)]
        for i, ln in enumerate(lines):
            if not ln.startswith(".amdhsa_kernel "):
                continue
            name = ln.split()[1]
            start = max(j for j in range(i) if lines[j] == name + ":")
            end = lines.index(".end_amdhsa_kernel", i)
            labels = {}
            body = [re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), b)
                    for b in lines[start + 1:i] if b]
            out[name] = (body, lines[i + 1:end])
    return out


def main():
    if "--" not in sys.argv:
        sys.exit(__doc__)
    cut = sys.argv.index("--")
    a, b = kernels(sys.argv[1:cut]), kernels(sys.argv[cut + 1:])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            verdict = "only on the %s side" % ("first" if name in a else "second")
        elif a[name][0] != b[name][0]:
            verdict = "INSTRUCTIONS DIFFER (%d against %d lines)" % (len(a[name][0]), len(b[name][0]))
        elif a[name][1] != b[name][1]:
            verdict = "DESCRIPTOR DIFFERS: " + "; ".join(x + " / " + y for x, y in zip(a[name][1], b[name][1]) if x != y)
        else:
            verdict = "equal"
        bad += verdict != "equal"
        print("%-9s %s" % (verdict if verdict == "equal" else "DIFF", name) + ("" if verdict == "equal" else "\n    " + verdict))
    print("%d kernels on the first side, %d on the second, %d differ" % (len(a), len(b), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
