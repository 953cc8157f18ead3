"""Writes flow_iter_digests.json: the SHA-256 of the flow fields of the cases of tests/flow_iter_sched_cases.py as the
library in the tree computes them on the GPU.  A change to the fused flow iteration that only reschedules it leaves every
digest as it is (test_gpu_flow_iter_schedule.py); the file was recorded from the commit before the march's waits were
moved off its stores.  Regenerate only when the arithmetic is meant to change.  Needs a GPU; run from the repository
root:  python tests/golden/make_flow_iter_digests.py [OUT.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import flow_iter_sched_cases as K  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else K.DIGESTS_PATH
    d = {name: K.digest(K.run(name)) for name in K.CASES}
    with open(out, "w") as f:
        json.dump({"what": "sha256 of the float32 flow field(s) [pairs][H][W][2] of each case", "sha256": d}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    for name, h in d.items():
        print(name, h[:16])
