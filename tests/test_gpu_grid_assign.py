"""ofc_grid_assign_counts_dev (k_grid_assign_counts of csrc/grid_labels.hip) through vis.grid_assign_counts, the C ABI and
ClipPipeline.cell_clusters(centers=), against the numpy model of tests/grid_assign_cases.py (checked by hand in
test_grid_assign_host.py).

Bars.  On the lattice fields no label is ambiguous (the two nearest centres of EVERY lattice point are >= 1e-3 apart in
squared distance, asserted on the CPU), so the counts equal the direct-form float64 argmin's, and the sums, whose every
partial sum is dyadic and exact, equal math.fsum's bit for bit.  On an arbitrary field the labels to count are those of
ofc_lloyd_step_dev on the same buffer (existing code, held to its definition by its own tests): counts equal, sums within
n 2^-53 sum|x| of the exact sum per entry (n its count), the bound of any order of f64 summation.  Entries nobody is
counted in are +0.0."""
import ctypes as C

import numpy as np
import pytest

from tests import grid_assign_cases as GA
from tests import motion_grid_cases as MC

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run(geom, fl, cen, mean=None, sums=True):
    from opticalflowclustering_amd.vis import grid_assign_counts
    rows, cols = MC.GEOMETRIES[geom][:2]
    return grid_assign_counts(fl, cen, rows, cols, mean=mean, sums=sums)


def check_exact(geom, k, mean=None):
    fl, cen, lab, counts, sums = GA.case(geom, k)
    got_c, got_s = run(geom, fl, cen, mean)
    assert got_c.dtype == np.int32 and got_c.shape == counts.shape and got_s.shape == sums.shape
    assert np.array_equal(got_c, counts)
    assert np.array_equal(bits(got_s), bits(sums))                  # dyadic flow: bit for bit, +0.0 included
    assert np.array_equal(run(geom, fl, cen, mean, sums=False), got_c)      # the counts-only kernel
    return lab, got_c


@pytest.mark.parametrize("geom", sorted(MC.GEOMETRIES))
def test_every_geometry(geom):
    rows, cols, W, H, n = MC.GEOMETRIES[geom]
    lab, counts = check_exact(geom, 5)
    assert (counts.sum(axis=(1, 2)) == (W // cols) * cols * (H // rows) * rows).all()
    if geom == "one-px-cells":                                      # a cell is a pixel: the counts are the one-hot labels
        assert np.array_equal(np.argmax(counts, -1).reshape(n, H, W), lab) and (counts.sum(-1) == 1).all()


@pytest.mark.parametrize("mean", [None, GA.DYADIC_MEAN], ids=["mean-zero", "mean-dyadic"])
@pytest.mark.parametrize("geom", ["remainders-odd-frame", "smaller-than-wave"])
@pytest.mark.parametrize("k", MC.KS)
def test_every_k(geom, k, mean):
    check_exact(geom, k, mean)


def test_exact_ties_go_to_the_first_minimum():
    """centres (1, 0), (-1, 0), (0, 1), mean (0, 0), on the lattice: cn = 1 and every product is exact, so the expanded
    form is exact in f64 and a tie is an exact tie; one-pixel cells show every label"""
    fl = GA.field("one-px-cells", seed=21)
    fl[0, 0, :6] = [[0, 0], [0, -1], [1.5, 1.5], [-2, 2], [0, 0.125], [-0.125, 0]]      # the host test's hand-made ties
    want = GA.expanded_labels(fl, GA.TIE_CENTRES)
    d = np.sort(MC.direct_sqdist(fl.reshape(-1, 2), GA.TIE_CENTRES), axis=1)
    assert (d[:, 0] == d[:, 1]).sum() >= 4
    counts = run("one-px-cells", fl, GA.TIE_CENTRES, sums=False)
    assert (counts.sum(-1) == 1).all()
    assert np.array_equal(np.argmax(counts, -1).reshape(want.shape), want)
    assert want[0, 0, :6].tolist() == [0, 0, 0, 1, 2, 1]


def step_labels(fl, k, mean, cen_c):
    """ofc_lloyd_step_dev(accumulate = 0) on the field: the labels the fused kernel has to count"""
    from opticalflowclustering_amd import _lib
    n, H, W = fl.shape[:3]
    X, L = _lib.DeviceBuffer(fl.nbytes).upload(fl), _lib.DeviceBuffer(n * H * W)
    try:
        _lib.check(_lib.load().ofc_lloyd_step_dev(0, C.c_void_p(X.ptr), _lib.F32, n * H * W, 2, k, _lib.ptr(mean),
                                                  _lib.ptr(cen_c), C.c_void_p(L.ptr), 0, None))
        return L.download((n, H, W), np.uint8)
    finally:
        X.free()
        L.free()


@pytest.mark.parametrize("geom,k", [("remainders-odd-frame", 5), ("remainders-odd-frame", 16), ("wider-than-group", 8),
                                    ("whole-frame", 2)])
def test_against_the_e_step_on_an_arbitrary_field(geom, k):
    rows, cols, W, H, n = MC.GEOMETRIES[geom]
    rng = np.random.default_rng(500 + k)
    fl = MC.real_flow(400 + k, n, H, W)
    cen, mean = rng.uniform(-4, 4, (k, 2)), rng.uniform(-0.5, 0.5, 2)
    lab = step_labels(fl, k, mean, np.ascontiguousarray(cen - mean))
    counts, sums = MC.model_counts(lab, k, rows, cols, fl)
    got_c, got_s = run(geom, fl, cen, mean)
    assert np.array_equal(got_c, counts)
    bound = MC.sum_bound(counts, MC.model_abs_sums(lab, k, rows, cols, fl))
    err = np.abs(got_s - sums)
    print("largest error / bound:", (err[bound > 0] / bound[bound > 0]).max())
    assert (err <= bound).all()
    empty = np.broadcast_to((counts == 0)[..., None], got_s.shape)
    assert np.array_equal(bits(got_s)[empty], np.zeros(empty.sum(), np.int64))     # +0.0, not -0.0
    again_c, again_s = run(geom, fl, cen, mean)
    assert np.array_equal(again_c, got_c) and np.array_equal(bits(again_s), bits(got_s))      # twice: the same bits


@pytest.mark.parametrize("k", [5, 16])
def test_a_frame_does_not_depend_on_the_others(k):
    rows, cols, W, H, n = MC.GEOMETRIES["remainders-odd-frame"]
    fl, cen = MC.real_flow(31 + k, n, H, W), GA.centres(k)
    c3, s3 = run("remainders-odd-frame", fl, cen)
    c1, s1 = run("remainders-odd-frame", fl[1:2], cen)
    assert np.array_equal(c1[0], c3[1]) and np.array_equal(bits(s1[0]), bits(s3[1]))
    c2d, s2d = run("remainders-odd-frame", fl[1], cen)                             # a single (H, W, 2) frame
    assert np.array_equal(c2d, c1) and np.array_equal(bits(s2d), bits(s1))


def test_refusals_leave_the_outputs_untouched():
    from opticalflowclustering_amd import _lib
    W, H, n, rows, cols, k = 40, 9, 2, 3, 4, 5
    fl = GA.field("one-px-high")
    assert fl.shape == (n, H, W, 2)
    cen = np.ascontiguousarray(GA.centres(16))
    mean = np.zeros(2)
    pat_c = np.full(n * H * W * 16, 0x5A5A5A5A, np.int32)          # room for every grid tried below
    pat_s = np.full(n * H * W * 32, -7.25, np.float64)
    bufs = [_lib.DeviceBuffer(a.nbytes).upload(a) for a in (fl, pat_c, pat_s)]
    F, Cn, S = (C.c_void_p(b.ptr) for b in bufs)
    M, Ce = _lib.ptr(mean), _lib.ptr(cen)

    def bad(i, v, what=cen):
        a = np.array(what, np.float64)
        a.flat[i] = v
        return a

    bad_arrays = [bad(0, np.nan), bad(9, np.inf), bad(3, -np.inf), bad(0, np.nan, mean), bad(1, np.inf, mean)]
    fn = _lib.load().ofc_grid_assign_counts_dev
    EINVAL, EUNSUP = _lib.OFC_EINVAL, _lib.OFC_EUNSUPPORTED
    refused = {
        "no flow": ((0, None, W, H, n, rows, cols, k, M, Ce, Cn, S), EINVAL),
        "no centres": ((0, F, W, H, n, rows, cols, k, M, None, Cn, S), EINVAL),
        "no counts": ((0, F, W, H, n, rows, cols, k, M, Ce, None, S), EINVAL),
        "nan centre": ((0, F, W, H, n, rows, cols, k, M, _lib.ptr(bad_arrays[0]), Cn, S), EINVAL),
        "inf centre": ((0, F, W, H, n, rows, cols, k, M, _lib.ptr(bad_arrays[1]), Cn, S), EINVAL),
        "-inf centre": ((0, F, W, H, n, rows, cols, k, M, _lib.ptr(bad_arrays[2]), Cn, S), EINVAL),
        "nan mean": ((0, F, W, H, n, rows, cols, k, _lib.ptr(bad_arrays[3]), Ce, Cn, S), EINVAL),
        "inf mean": ((0, F, W, H, n, rows, cols, k, _lib.ptr(bad_arrays[4]), Ce, Cn, S), EINVAL),
        "no frames": ((0, F, W, H, 0, rows, cols, k, M, Ce, Cn, S), EINVAL),
        "negative frames": ((0, F, W, H, -1, rows, cols, k, M, Ce, Cn, S), EINVAL),
        "rows 0": ((0, F, W, H, n, 0, cols, k, M, Ce, Cn, S), EINVAL),
        "rows > H": ((0, F, W, H, n, H + 1, cols, k, M, Ce, Cn, S), EINVAL),
        "cols 0": ((0, F, W, H, n, rows, 0, k, M, Ce, Cn, S), EINVAL),
        "cols > W": ((0, F, W, H, n, rows, W + 1, k, M, Ce, Cn, S), EINVAL),
        "k 0": ((0, F, W, H, n, rows, cols, 0, M, Ce, Cn, S), EUNSUP),
        "k 17": ((0, F, W, H, n, rows, cols, 17, M, Ce, Cn, S), EUNSUP),
        "k 17, counts only": ((0, F, W, H, n, rows, cols, 17, M, Ce, Cn, None), EUNSUP),
        "W*H = 2^31": ((0, F, 65536, 32768, 1, rows, cols, k, M, Ce, Cn, S), EUNSUP),
    }
    try:
        for name, (args, want) in refused.items():
            assert fn(*args) == want, name
            assert _lib.load().ofc_last_error(), name
            assert np.array_equal(bufs[1].download(pat_c.shape, np.int32), pat_c), name
            assert np.array_equal(bits(bufs[2].download(pat_s.shape, np.float64)), bits(pat_s)), name
        # and the same buffers accept the call at the limits: rows = H, cols = W, k = 16, no mean (= (0, 0)), no sums
        lab = GA.model_labels(fl, cen)
        counts, sums = MC.model_counts(lab, 16, H, W, fl)
        assert fn(0, F, W, H, n, H, W, 16, None, Ce, Cn, None) == _lib.OFC_OK
        assert np.array_equal(bufs[1].download(counts.shape, np.int32), counts)
        assert np.array_equal(bits(bufs[2].download(pat_s.shape, np.float64)), bits(pat_s))      # sums_dev NULL: not written
        assert fn(0, F, W, H, n, H, W, 16, M, Ce, Cn, S) == _lib.OFC_OK
        assert np.array_equal(bits(bufs[2].download(sums.shape, np.float64)), bits(sums))
        from opticalflowclustering_amd.vis import grid_assign_counts
        with pytest.raises(ValueError):                                            # the Python hook raises on the same
            grid_assign_counts(fl, cen[:5], rows=H + 1, cols=cols)
        with pytest.raises(ValueError):
            grid_assign_counts(fl, bad(0, np.nan)[:5])
        with pytest.raises(ValueError):
            grid_assign_counts(fl[..., :1], cen[:5])
    finally:
        for b in bufs:
            b.free()


def test_cell_clusters_with_centres_is_assign_then_cell_clusters():
    from opticalflowclustering_amd.pipeline import ClipPipeline
    from opticalflowclustering_amd.vis import bgr2gray
    clip = np.stack([bgr2gray(f) for f in MC.moving_blobs_clip()])
    T, H, W = clip.shape
    rows, cols, k = 3, 4, 3
    pipe = ClipPipeline(W, H, T, batch_pairs=2)
    try:
        pipe.upload_frames(clip)
        pipe.run_flow()
        with pytest.raises(ValueError, match="run_kmeans"):             # without centres it still needs labels
            pipe.cell_clusters(rows, cols)
        C0, _ = pipe.seed_kmeans(k, random_state=0)
        centers, _, _ = pipe.run_kmeans(C0)
        before = pipe.labels_host()
        fit_c = MC.model_counts(before, k, rows, cols)
        models = (centers, centers + np.array([0.21, -0.13]))           # the fit's own, and one from elsewhere
        got = [pipe.cell_clusters(rows, cols, sums=True, centers=cen) for cen in models]
        assert np.array_equal(pipe.labels_host(), before) and pipe._label_k == k      # the labels: neither needed nor touched
        assert np.array_equal(pipe.cell_clusters(rows, cols), fit_c)    # ... and still those of the fit
        for cen, (got_c, got_s) in zip(models, got):
            assert np.array_equal(pipe.cell_clusters(rows, cols, centers=cen), got_c)
            pipe.assign(cen)
            want_c, want_s = pipe.cell_clusters(rows, cols, sums=True)
            assert got_c.dtype == np.int32 and np.array_equal(got_c, want_c)
            assert np.array_equal(bits(got_s), bits(want_s))
            assert (got_c.sum(axis=(1, 2)) == (W // cols) * cols * (H // rows) * rows).all()
        with pytest.raises(ValueError):
            pipe.cell_clusters(rows, cols, centers=np.zeros((3, 3)))
        pipe.run_flow()                                                 # no labels any more: the fused route does not care
        assert np.array_equal(pipe.cell_clusters(rows, cols, centers=models[1]), got[1][0])
    finally:
        pipe.close()
