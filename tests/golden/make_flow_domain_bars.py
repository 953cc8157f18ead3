"""Writes flow_domain_bars.json: for every stage case of tests/flow_domain_cases.py (fused iteration x window x seam width
x iteration count, box mean + solve x window x seam width) the largest absolute difference between the CPU oracle and a
float64 numpy restatement of the same operation on the same float32 inputs -- what float32 against float64 alone costs
on that input.  test_gpu_flow_domain.py derives each case's bar from it; test_oracle_flow_domain.py recomputes the values
and fails when this file is stale.  Run from the repository root:  python tests/golden/make_flow_domain_bars.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import flow_domain_cases as D  # noqa: E402

if __name__ == "__main__":
    d = D.measure_stage_distances()
    with open(D.BARS_PATH, "w") as f:
        json.dump({"what": "max |oracle (float32) - float64 restatement| per stage case, pixels",
                   "max_abs_oracle_minus_float64": d}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(d)} cases, largest {max(d.values()):.3e} -> {D.BARS_PATH}")
