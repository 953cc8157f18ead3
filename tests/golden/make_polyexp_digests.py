"""Writes polyexp_digests.json: the SHA-256 of the expansion of every case of tests/polyexp_layout_cases.py, at poly_n 5 and
7, as the library in the tree computes it on the GPU.  A change to k_polyexp that only moves its LDS staging or evaluates
the u8 blur another exact way leaves every digest as it is (test_gpu_polyexp_layout.py).  The file names the commit whose
build it was recorded from; regenerate only when the arithmetic is meant to change.  Needs a GPU; run from the repository
root:  python tests/golden/make_polyexp_digests.py COMMIT [OUT.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import polyexp_layout_cases as K  # noqa: E402

if __name__ == "__main__":
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else K.DIGESTS_PATH
    d = {K.case_id(c, n): K.digest(K.run(c, n)) for c in K.CASES for n in K.POLY}
    with open(out, "w") as f:
        json.dump({"what": "sha256 of the float32 expansion [H][W][5] of each case", "recorded_from": commit, "sha256": d},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    for name, h in d.items():
        print(name, h[:16])
