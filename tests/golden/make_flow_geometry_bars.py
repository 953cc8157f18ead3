"""Writes flow_geometry_bars.json: for every stage case of tests/flow_geometry_cases.py (fused iteration x window x frame
height x iteration count) the largest absolute difference between the CPU oracle and a float64 numpy restatement of the
same iterations on the same float32 inputs -- make_flow_domain_bars.py's method on that table.
test_gpu_flow_geometry.py derives the 16-row run's bar from it; test_flow_geometry_host.py recomputes the values and fails
when this file is stale.  Run from the repository root:  python tests/golden/make_flow_geometry_bars.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import flow_geometry_cases as G  # noqa: E402

if __name__ == "__main__":
    d = G.measure_stage_distances()
    with open(G.BARS_PATH, "w") as f:
        json.dump({"what": "max |oracle (float32) - float64 restatement| per stage case, pixels",
                   "max_abs_oracle_minus_float64": d}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(d)} cases, largest {max(d.values()):.3e} -> {G.BARS_PATH}")
