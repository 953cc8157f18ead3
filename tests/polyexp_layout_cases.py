"""The cases of test_gpu_polyexp_layout.py and tests/golden/make_polyexp_digests.py: the smallest frames at which the
polynomial expansion's output staging (a wave stages its output row in the moments row it has just consumed) and the
integer 3x3 blur of its u8 form can go wrong.  numpy only; the inputs are generated, never stored.

  236x8      one partial column tile, one chunk, one strip
  244x24     a full 240-column tile plus a 4-pixel tail tile; three 8-row strips: the top and the bottom one take the
             reflected any-row path of the u8 form
  250x17     W % 4 != 0: the scalar store path, which must leave the staging alone; ragged last strip
  484x40     three tiles; the strips from rows 8 and 16 (poly_n 5) / row 8 (poly_n 7) take the interior path of the u8 form,
             with row sums carried from chunk to chunk
  4x2        the smallest frame the u8 form accepts: every tap reflected, the weight word's positions coincide
             (f32 form: 1x1, the smallest it accepts)
  244x8192   1 024 work-groups, so the strips stay 16 rows high (the benchmark's height): two chunks per strip, the second
             chunk's moments overwrite staged rows.  Digest only.
Contents: u8 all 255 (the integer sums at their maximum, 4 080), a 0/255 checkerboard, seeded random bytes; f32 seeded
random floats in [0, 255) and the same scaled by 1e4.  Every case runs with poly_n 5 and 7."""
import hashlib
import json
import os

import numpy as np

DIGESTS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polyexp_digests.json")

SMALL = [(236, 8), (244, 24), (250, 17), (484, 40)]         # checked against the oracle as well
TINY_U8, TINY_F32 = (4, 2), (1, 1)
TALL = (244, 8192)                                           # digest only
U8_CONTENTS = ("all255", "checker", "random")
F32_CONTENTS = ("random", "random_x1e4")
POLY = {5: 1.2, 7: 1.5}                                      # poly_n -> poly_sigma (the values cv2 documents)

# (form, W, H, content)
CASES = [("u8", W, H, c) for (W, H) in SMALL + [TINY_U8, TALL] for c in U8_CONTENTS] + \
        [("f32", W, H, c) for (W, H) in SMALL + [TINY_F32, TALL] for c in F32_CONTENTS]


def case_id(case, n):
    form, W, H, content = case
    return "%s_%dx%d_%s_n%d" % (form, W, H, content, n)


def frame(case):
    """the input of a case: uint8 [H][W] for the u8 form, float32 [H][W] for the f32 form (read-only)"""
    form, W, H, content = case
    rng = np.random.default_rng(W * 100003 + H * 17 + len(content))
    if form == "u8":
        if content == "all255":
            a = np.full((H, W), 255, np.uint8)
        elif content == "checker":
            yy, xx = np.mgrid[0:H, 0:W]
            a = (((yy + xx) & 1) * 255).astype(np.uint8)
        else:
            a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    else:
        a = (rng.random((H, W)) * 255).astype(np.float32)
        if content == "random_x1e4":
            a = a * np.float32(1e4)
    a.setflags(write=False)
    return a


def level0(gray):
    """pyramid level 0 of a u8 frame, float32: the [1/4 1/2 1/4] blur along x then y with BORDER_REFLECT_101, in integers
    (every sum is exact in f32, so this is the image any f32 evaluation of the taps gives); any size with W, H >= 2"""
    g = np.pad(gray.astype(np.int32), 1, mode="reflect")
    h = g[:, :-2] + 2 * g[:, 1:-1] + g[:, 2:]
    v = h[:-2] + 2 * h[1:-1] + h[2:]
    return (v.astype(np.float32) * np.float32(0.0625)).astype(np.float32)


def run(case, n):
    """the expansion of a case on the GPU, float32 [H][W][5]"""
    from opticalflowclustering_amd import stages
    f = stages.polyexp_u8 if case[0] == "u8" else stages.polyexp
    return f(frame(case), n, POLY[n])


def digest(R):
    return hashlib.sha256(np.ascontiguousarray(R, np.float32).tobytes()).hexdigest()


def load_digests():
    with open(DIGESTS_PATH) as f:
        return json.load(f)["sha256"]
