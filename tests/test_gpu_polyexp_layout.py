"""k_polyexp after its output staging moved into the moments tile (no separate scratch array: a wave stages its output row
in the moments row it has just consumed) and the u8 form's 3x3 blur moved to integers (a byte dot product per row, a
shift-add per column, one conversion): neither changes a bit of the output.  The cases (tests/polyexp_layout_cases.py) are the
smallest frames at which either can go wrong, each at poly_n 5 and 7.

Bars:
  1. digest: the SHA-256 of every expansion equals the one recorded from the commit before the change
     (tests/golden/polyexp_digests.json, written by tests/golden/make_polyexp_digests.py).
  2. u8 against staged f32: the u8 form equals the level-0 image followed by the f32 form, bit for bit (every case but the
     tall one).  The level-0 image comes from stages.level_image where it accepts the frame (W, H >= 16) and must then
     equal the integer statement of the blur in the cases file, which serves the smaller frames.
  3. oracle: on the four small shapes max|d| <= 2e-5 * max|oracle|, test_polyexp's bar, so that the digests are not the only
     anchor.  Frames whose level-0 image is constant have a zero expansion and no such scale; _flat_bar says what they
     are held to instead.
The tall case also pins the strip height it is there for: 16 rows, two chunks per strip."""
import numpy as np
import pytest

import polyexp_layout_cases as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ALL = [(c, n) for c in K.CASES for n in K.POLY]
_ids = [K.case_id(c, n) for c, n in ALL]


@pytest.fixture(scope="module")
def digests():
    return K.load_digests()


@pytest.fixture(scope="module")
def results():
    """every expansion computed once on the GPU, shared read-only"""
    out = {}
    for c, n in ALL:
        R = K.run(c, n)
        R.setflags(write=False)
        out[K.case_id(c, n)] = R
    return out


def test_tall_case_runs_at_the_benchmark_strip_height():
    from opticalflowclustering_amd import stages
    W, H = K.TALL
    assert stages.flow_launch_geometry(W, H // 2, 1)[2] == 16        # the same 1 024 work-groups, over two images


@pytest.mark.parametrize("case,n", ALL, ids=_ids)
def test_expansion_keeps_its_bits(case, n, results, digests):
    name = K.case_id(case, n)
    R = results[name]
    assert R.shape == (case[2], case[1], 5) and np.isfinite(R).all()
    assert K.digest(R) == digests[name], name


@pytest.mark.parametrize("case,n", [(c, n) for c, n in ALL if c[0] == "u8" and (c[1], c[2]) != K.TALL],
                         ids=[i for (c, n), i in zip(ALL, _ids) if c[0] == "u8" and (c[1], c[2]) != K.TALL])
def test_u8_form_equals_level_image_then_f32_form(case, n, results):
    from opticalflowclustering_amd import stages
    _, W, H, _ = case
    gray = K.frame(case)
    lvl = K.level0(gray)
    if W >= 16 and H >= 16:
        dev = stages.level_image(gray, 0)
        assert np.array_equal(dev, lvl)
        lvl = dev
    want = stages.polyexp(lvl, n, K.POLY[n])
    assert np.array_equal(results[K.case_id(case, n)], want)


def _flat_bar(c, n):
    """the bar of a frame whose level-0 image is the constant c (all 255; the checkerboard, which blurs to 127.5).  Its
    exact expansion is zero, and max|oracle| is then the oracle's own rounding error (5.4e-6 at c = 255, poly_n 5), not a
    scale: the exact answer itself would miss 2e-5 of it.  What is left of either side is the cancellation
    b1 * ig03 + b5 * ig33 of two terms of size c * |ig03|, each b a (2n+1)-tap sum of (2n+1)-tap f32 sums with relative error
    <= 2 (2n+1) 2^-24, so each side is within 2 * 2 (2n+1) 2^-24 * c |ig03| of zero and the two within twice that of each
    other (4.6e-4 at c = 255, poly_n 5; measured 6.1e-6)."""
    ig03 = abs(float(O.polyexp_setup(n, K.POLY[n])[3][1]))
    return 2 * (2 * 2 * (2 * n + 1) * 2.0 ** -24 * c * ig03)


@pytest.mark.parametrize("case,n", [(c, n) for c, n in ALL if (c[1], c[2]) in K.SMALL],
                         ids=[i for (c, n), i in zip(ALL, _ids) if (c[1], c[2]) in K.SMALL])
def test_expansion_agrees_with_the_oracle(case, n, results):
    img = K.frame(case)
    if case[0] == "u8":
        img = K.level0(img)
    want = O.polyexp(img, n, K.POLY[n])
    got = results[K.case_id(case, n)]
    err, top = np.abs(got - want).max(), np.abs(want).max()
    print("%s: max|d| %.3e, max|oracle| %.3e, ratio %.3e" % (K.case_id(case, n), err, top, err / top))
    if img.min() == img.max():
        assert err <= _flat_bar(float(img.max()), n), (err, _flat_bar(float(img.max()), n))
    else:
        assert err <= 2e-5 * top
