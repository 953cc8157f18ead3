"""ofc_grid_label_counts_dev (csrc/grid_labels.hip) through vis.grid_label_counts and the C ABI, against the numpy model
of tests/motion_grid_cases.py (itself checked by hand in test_motion_grids_host.py).

Bars: counts equal the model exactly, always.  Sums of integer-valued flows equal the model bit for bit (every partial
sum is an exact integer, so no order of summation rounds).  Sums of real-valued flows are within n 2^-53 sum|x| of the
exact sum per entry (n its count): the bound of any order of f64 summation.  Entries nobody is counted in are +0.0."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import motion_grid_cases as MC

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def case(geom, k, kind="uniform", flow="integer"):
    """labels, flow and the model's answer for one case, computed once"""
    rows, cols, W, H, n = MC.GEOMETRIES[geom]
    seed = sorted(MC.GEOMETRIES).index(geom) * 100 + k
    lab = MC.random_labels(seed, n, H, W, k, kind)
    fl = (MC.integer_flow if flow == "integer" else MC.real_flow)(seed + 50, n, H, W)
    counts, sums = MC.model_counts(lab, k, rows, cols, fl)
    for a in (lab, fl, counts, sums):
        a.setflags(write=False)
    return lab, fl, counts, sums


def run(geom, lab, k, fl=None):
    from opticalflowclustering_amd.vis import grid_label_counts
    rows, cols = MC.GEOMETRIES[geom][:2]
    return grid_label_counts(lab, k, rows, cols, flow=fl)


def check_exact(geom, k, kind="uniform"):
    lab, fl, counts, sums = case(geom, k, kind)
    got_c, got_s = run(geom, lab, k, fl)
    assert got_c.dtype == np.int32 and got_c.shape == counts.shape and got_s.shape == sums.shape
    assert np.array_equal(got_c, counts)
    assert np.array_equal(bits(got_s), bits(sums))                  # integer-valued flow: bit for bit, +0.0 included
    assert np.array_equal(run(geom, lab, k), counts)                # the counts-only kernel
    return counts


@pytest.mark.parametrize("geom", sorted(MC.GEOMETRIES))
def test_every_geometry(geom):
    rows, cols, W, H, n = MC.GEOMETRIES[geom]
    counts = check_exact(geom, 5)
    assert (counts.sum(axis=(1, 2)) == (W // cols) * cols * (H // rows) * rows).all()
    if geom == "whole-frame":
        assert (counts.sum(axis=(1, 2)) == W * H).all()


@pytest.mark.parametrize("geom", ["remainders-odd-frame", "smaller-than-wave"])
@pytest.mark.parametrize("k", MC.KS)
def test_every_k(geom, k):
    check_exact(geom, k)


@pytest.mark.parametrize("k", [2, 5, 9])
def test_absent_cluster(k):
    counts = check_exact("remainders-odd-frame", k, "absent")
    assert (counts[..., 1] == 0).all() and counts[..., 0].any()


@pytest.mark.parametrize("k", [1, 5, 8, 16])
def test_unassigned_labels_are_counted_nowhere(k):
    rows, cols, W, H, n = MC.GEOMETRIES["remainders-odd-frame"]
    counts = check_exact("remainders-odd-frame", k, "unassigned")
    assert (counts.sum(axis=(1, 2)) < (W // cols) * cols * (H // rows) * rows).all()


@pytest.mark.parametrize("k", [1, 5, 6, 9, 16])
def test_labels_out_of_range_only(k):
    lab, fl, counts, sums = case("remainders-odd-frame", k, "out-of-range")
    assert not counts.any()
    got_c, got_s = run("remainders-odd-frame", lab, k, fl)
    assert not got_c.any()
    assert np.array_equal(bits(got_s), np.zeros(got_s.shape, np.int64))            # every entry exactly +0.0


@pytest.mark.parametrize("geom,k", [("remainders-odd-frame", 5), ("remainders-odd-frame", 16), ("wider-than-group", 8),
                                    ("whole-frame", 5), ("reference-1080p", 5)])
def test_real_valued_sums_within_the_f64_bound(geom, k):
    rows, cols = MC.GEOMETRIES[geom][:2]
    lab, fl, counts, sums = case(geom, k, "unassigned", "real")
    got_c, got_s = run(geom, lab, k, fl)
    assert np.array_equal(got_c, counts)
    bound = MC.sum_bound(counts, MC.model_abs_sums(lab, k, rows, cols, fl))
    err = np.abs(got_s - sums)
    print("largest error / bound:", (err[bound > 0] / bound[bound > 0]).max())
    assert (err <= bound).all()
    empty = np.broadcast_to((counts == 0)[..., None], got_s.shape)
    assert np.array_equal(bits(got_s)[empty], np.zeros(empty.sum(), np.int64))     # +0.0, not -0.0
    again = run(geom, lab, k, fl)[1]
    assert np.array_equal(bits(again), bits(got_s))                                # the same call twice: the same bits


@pytest.mark.parametrize("k", [5, 16])
def test_a_frame_does_not_depend_on_the_others(k):
    lab, fl, counts, _ = case("remainders-odd-frame", k, "uniform", "real")
    c3, s3 = run("remainders-odd-frame", lab, k, fl)
    c1, s1 = run("remainders-odd-frame", lab[1:2], k, fl[1:2])
    assert np.array_equal(c1[0], c3[1]) and np.array_equal(bits(s1[0]), bits(s3[1]))
    c2d, s2d = run("remainders-odd-frame", lab[1], k, fl[1])                       # a single 2-D / 3-D frame
    assert np.array_equal(c2d, c1) and np.array_equal(bits(s2d), bits(s1))


def test_refusals_leave_the_outputs_untouched():
    from opticalflowclustering_amd import _lib
    W, H, n, rows, cols, k = 40, 9, 2, 3, 4, 5
    lab = MC.random_labels(1, n, H, W, k)
    fl = MC.integer_flow(2, n, H, W)
    pat_c = np.full(n * H * W * 16, 0x5A5A5A5A, np.int32)          # room for every grid tried below
    pat_s = np.full(n * H * W * 32, -7.25, np.float64)
    bufs = [_lib.DeviceBuffer(a.nbytes).upload(a) for a in (lab, fl, pat_c, pat_s)]
    L, F, Cn, S = (C.c_void_p(b.ptr) for b in bufs)
    fn = _lib.load().ofc_grid_label_counts_dev
    EINVAL, EUNSUP = _lib.OFC_EINVAL, _lib.OFC_EUNSUPPORTED
    refused = {
        "no labels": ((0, None, F, W, H, n, rows, cols, k, Cn, S), EINVAL),
        "no counts": ((0, L, F, W, H, n, rows, cols, k, None, S), EINVAL),
        "flow without sums": ((0, L, F, W, H, n, rows, cols, k, Cn, None), EINVAL),
        "sums without flow": ((0, L, None, W, H, n, rows, cols, k, Cn, S), EINVAL),
        "no frames": ((0, L, F, W, H, 0, rows, cols, k, Cn, S), EINVAL),
        "negative frames": ((0, L, F, W, H, -1, rows, cols, k, Cn, S), EINVAL),
        "rows 0": ((0, L, F, W, H, n, 0, cols, k, Cn, S), EINVAL),
        "rows > H": ((0, L, F, W, H, n, H + 1, cols, k, Cn, S), EINVAL),
        "cols 0": ((0, L, F, W, H, n, rows, 0, k, Cn, S), EINVAL),
        "cols > W": ((0, L, F, W, H, n, rows, W + 1, k, Cn, S), EINVAL),
        "k 0": ((0, L, F, W, H, n, rows, cols, 0, Cn, S), EUNSUP),
        "k 17": ((0, L, F, W, H, n, rows, cols, 17, Cn, S), EUNSUP),
        "k 17, counts only": ((0, L, None, W, H, n, rows, cols, 17, Cn, None), EUNSUP),
    }
    try:
        for name, (args, want) in refused.items():
            assert fn(*args) == want, name
            assert _lib.load().ofc_last_error(), name
            assert np.array_equal(bufs[2].download(pat_c.shape, np.int32), pat_c), name
            assert np.array_equal(bits(bufs[3].download(pat_s.shape, np.float64)), bits(pat_s)), name
        # and the same buffers accept the call at the limits: rows = H, cols = W, k = 16
        assert fn(0, L, F, W, H, n, H, W, 16, Cn, S) == _lib.OFC_OK
        counts, sums = MC.model_counts(lab, 16, H, W, fl)
        assert np.array_equal(bufs[2].download(counts.shape, np.int32), counts)
        assert np.array_equal(bits(bufs[3].download(sums.shape, np.float64)), bits(sums))
        with pytest.raises(ValueError):                                            # the Python hook raises on the same
            from opticalflowclustering_amd.vis import grid_label_counts
            grid_label_counts(lab, k, rows=H + 1, cols=cols)
    finally:
        for b in bufs:
            b.free()
