"""Camera motion on the device (motion_model.hip): the moment reduction, the chained fit, the subtraction, and their way up
through ClipPipeline, FlowStream and the motionGrids command line.

The moments are integers, so they are compared with array_equal against the numpy reference of
tests/camera_motion_cases.py; test_camera_motion_host.py proves the cases well-conditioned.  Models are held to the solve
bound against the exact solution, and to equal bits against the host's ofc_motion_solve on the device's own moments."""
import ctypes as C

import numpy as np
import pytest

from tests import camera_motion_cases as CC
from tests import motion_grid_cases as MC
from tests import uv_hist_cases as UC

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.int64)


def _dev(f):
    L = _L()
    f = np.ascontiguousarray(f, np.float32)
    return L.DeviceBuffer(max(f.nbytes, 8)).upload(f)


def moments_dev(f, models=None, c=None):
    """ofc_motion_moments_dev on a fresh device copy of f (n,H,W,2) -> (n,13) int64"""
    L = _L()
    n, H, W = f.shape[:3]
    fd = _dev(f)
    out = np.full((n, CC.NMOM), -7, np.int64)
    m = None if models is None else np.ascontiguousarray(models, np.float64)
    cc = None if c is None else np.ascontiguousarray(np.broadcast_to(np.float64(c), (n,)))
    try:
        L.check(L.load().ofc_motion_moments_dev(0, C.c_void_p(fd.ptr), W, H, n, L.ptr(m), L.ptr(cc), L.ptr(out)))
    finally:
        fd.free()
    return out


def fit_dev(f, kind, thresholds):
    """ofc_motion_fit_dev -> (models (n,6), status (n,), history models (T+1,n,6), history moments (T+1,n,13))"""
    L = _L()
    n, H, W = f.shape[:3]
    T = len(thresholds)
    thr = np.ascontiguousarray(thresholds, np.float64)
    fd = _dev(f)
    models, status = np.full((n, 6), 9.0), np.full(n, -1, np.int32)
    hm, hq = np.full((T + 1, n, 6), 9.0), np.full((T + 1, n, CC.NMOM), -7, np.int64)
    try:
        L.check(L.load().ofc_motion_fit_dev(0, C.c_void_p(fd.ptr), W, H, n, kind, L.ptr(thr), T, L.ptr(models), L.ptr(status),
                                            L.ptr(hm), L.ptr(hq)))
        assert np.array_equal(bits(fd.download(f.shape, np.float32)), bits(f))  # a fit leaves the field alone
    finally:
        fd.free()
    return models, status, hm, hq


def subtract_dev(f, models, in_place):
    L = _L()
    n, H, W = f.shape[:3]
    fd = _dev(f)
    dd = fd if in_place else L.DeviceBuffer(max(f.nbytes, 8))
    m = np.ascontiguousarray(models, np.float64)
    try:
        L.check(L.load().ofc_motion_subtract_dev(0, C.c_void_p(fd.ptr), W, H, n, L.ptr(m), C.c_void_p(dd.ptr)))
        if not in_place:
            assert np.array_equal(bits(fd.download(f.shape, np.float32)), bits(f))
        return dd.download(f.shape, np.float32)
    finally:
        fd.free()
        if not in_place:
            dd.free()


def host_solve(m, kind):
    L = _L()
    mm, p, st = np.ascontiguousarray(m, np.int64), np.zeros(6), C.c_int()
    L.check(L.load().ofc_motion_solve(L.ptr(mm), kind, L.ptr(p), C.byref(st)))
    return p, st.value


@pytest.mark.parametrize("case", CC.CASES, ids=repr)
def test_moments_equal_the_reference_in_every_round(case):
    f, fits = CC.reference(case)
    got = moments_dev(f)
    assert np.array_equal(got, np.array([ref["full"][0] for ref in fits], dtype=np.int64))
    for t, c in enumerate(case.thresholds, start=1):
        models = np.stack([ref["models"][t - 1] for ref in fits])
        got = moments_dev(f, models, c)
        for i, ref in enumerate(fits):
            if t < len(ref["full"]):                                             # the rounds the pair takes
                assert np.array_equal(got[i], np.array(ref["full"][t], dtype=np.int64)), (case, t, i)
            assert got[i, 12] == ref["full"][0][12]                              # outside does not depend on the selection


@pytest.mark.parametrize("case", CC.CASES, ids=repr)
def test_fit_history_status_and_models(case):
    f, fits = CC.reference(case)
    models, status, hm, hq = fit_dev(f, case.kind, case.thresholds)
    assert np.array_equal(hq, np.stack([ref["moments"] for ref in fits], 1))
    assert np.array_equal(status, [ref["status"] for ref in fits])
    assert np.array_equal(bits(models), bits(hm[-1]))
    for i, ref in enumerate(fits):
        kept, solved = np.zeros(6), 0
        for t in range(len(case.thresholds) + 1):
            p, st = host_solve(hq[t, i], case.kind) if t < len(ref["full"]) else (None, 1)
            if st == 0:                                                          # host and device run one function
                kept, solved = p, solved + 1
                want, kappa = CC.solve_exact([int(v) for v in hq[t, i]], case.kind)
                err, bound = np.abs(hm[t, i] - want).max(), CC.solve_bound(kappa, want)
                assert err <= bound, (case, t, i, err, bound)
            assert np.array_equal(bits(hm[t, i]), bits(kept)), (case, t, i)
        assert solved == len(ref["kappa"])


@pytest.mark.parametrize("case", CC.CASES, ids=repr)
def test_subtraction_within_one_ulp_and_in_place_equals_out_of_place(case):
    f, _ = CC.reference(case)
    models = fit_dev(f, case.kind, case.thresholds)[0]
    out = subtract_dev(f, models, in_place=False)
    assert np.array_equal(bits(subtract_dev(f, models, in_place=True)), bits(out))
    finite = np.isfinite(f).all(-1)
    for i in range(case.npair):
        eu, ev = CC.predict(models[i], case.W, case.H)
        with np.errstate(invalid="ignore", over="ignore"):
            want = np.stack([f[i, ..., 0].astype(np.float64) - eu, f[i, ..., 1].astype(np.float64) - ev], -1)
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            # the reference's own error: it rounds every product and sum of u - (p0 + p1 X/2 + p2 Y/2) where the definition
            # is one fma chain, at most 2^-52 of the terms' magnitudes; it shows only where the residual cancels to nothing
            m = np.abs(models[i])
            hx, hy = np.abs(CC.predict(np.array([0, 1, 0, 0, 0, 1.0]), case.W, case.H))
            own = 2.0 ** -52 * np.stack([m[0] + m[1] * hx + m[2] * hy, m[3] + m[4] * hx + m[5] * hy], -1)
            own = own + 2.0 ** -52 * np.abs(np.where(np.isfinite(f[i]), f[i], 0)).astype(np.float64)
        ok = finite[i]
        assert (np.abs(out[i][ok].astype(np.float64) - want[ok]) <= ulp[ok] + own[ok]).all(), case
        assert np.array_equal(bits(out[i][~ok]), bits(f[i][~ok]))                # a non-finite vector passes through, both parts
    if case.name == "non-finite":
        assert (~finite).sum() == 6 and np.isfinite(out[~finite]).any()
    if case.name == "range-limit":                                               # finite, not valid: subtracted all the same
        assert finite.all() and np.abs(out[0, 3, 5, 0] - (1024.0 - CC.predict(models[0], 64, 48)[0][3, 5])) < 1e-3


@pytest.mark.parametrize("name", ["64x48-x3", "67x45-x3-translation", "all-outside-in-the-middle"])
def test_three_pairs_equal_three_calls_of_one(name):
    case = CC.BY_NAME[name]
    f, fits = CC.reference(case)
    m3, s3, hm3, hq3 = fit_dev(f, case.kind, case.thresholds)
    q3 = moments_dev(f, m3, 2.0)
    out3 = subtract_dev(f, m3, in_place=True)
    for i in range(3):
        m1, s1, hm1, hq1 = fit_dev(f[i:i + 1], case.kind, case.thresholds)
        assert np.array_equal(bits(m1[0]), bits(m3[i])) and s1[0] == s3[i]
        assert np.array_equal(bits(hm1[:, 0]), bits(hm3[:, i])) and np.array_equal(hq1[:, 0], hq3[:, i])
        assert np.array_equal(moments_dev(f[i:i + 1], m3[i:i + 1], 2.0)[0], q3[i])
        assert np.array_equal(bits(subtract_dev(f[i:i + 1], m3[i:i + 1], in_place=False)[0]), bits(out3[i]))


def test_python_fronts_agree_with_the_device_calls():
    from opticalflowclustering_amd import camera as cam
    for name in ("64x48-x3", "67x45-x3-translation", "starved-in-round-2", "all-outside-in-the-middle"):
        case = CC.BY_NAME[name]
        f, fits = CC.reference(case)
        models, status, hm, hq = fit_dev(f, case.kind, case.thresholds)
        cm = cam.estimate_camera_motion(f, case.model, case.thresholds)
        assert np.array_equal(bits(cm.params), bits(models)) and np.array_equal(cm.status, status)
        assert np.array_equal(cm.outside, hq[0, :, 12])
        assert np.array_equal(cm.inliers, [ref["moments"][len(ref["kappa"]) - 1][0] if ref["kappa"] else 0 for ref in fits])
        res, cm2 = cam.compensate(f, case.model, case.thresholds)
        assert np.array_equal(bits(res), bits(subtract_dev(f, models, in_place=False)))
        assert all(np.array_equal(a, b) for a, b in zip(cm, cm2))
        one, cm1 = cam.compensate(f[0], case.model, case.thresholds)            # (H,W,2) in, (H,W,2) out
        assert one.shape == f[0].shape and np.array_equal(bits(one), bits(res[0])) and len(cm1.status) == 1
    f = CC.reference(CC.BY_NAME["64x48"])[0]
    d = cam.estimate_camera_motion(f)                                            # the defaults: affine, (4, 2, 1)
    assert np.array_equal(bits(d.params), bits(fit_dev(f, 2, (4.0, 2.0, 1.0))[0]))
    once = cam.estimate_camera_motion(f, thresholds=())                          # T = 0: one fit over every valid pixel
    assert once.inliers[0] == 64 * 48 and np.array_equal(bits(once.params), bits(fit_dev(f, 2, ())[0]))


def test_refusals_are_decided_on_the_host():
    L = _L()
    lib = L.load()
    f = CC.reference(CC.BY_NAME["64x48"])[0]
    fd = _dev(f)
    fp = C.c_void_p(fd.ptr)
    thr = np.array([4.0, 2.0, 1.0] * 3)
    models, status, mom = np.full((1, 6), 9.0), np.full(1, -1, np.int32), np.full((1, 13), -7, np.int64)
    res, ms = np.full(f.shape, 5.0, np.float32), C.c_float(-1.0)
    mp, sp, tp = L.ptr(models), L.ptr(status), L.ptr(thr)

    def fit(dev=0, flow=fp, W=64, H=48, n=1, kind=2, t=tp, T=3, m=mp, s=sp):
        return lib.ofc_motion_fit_dev(dev, flow, W, H, n, kind, t, T, m, s, None, None)
    for kw in (dict(kind=0), dict(kind=3), dict(T=9), dict(T=-1), dict(t=None), dict(flow=None), dict(m=None), dict(s=None),
               dict(n=0), dict(W=0), dict(W=1, H=64), dict(flow=C.c_void_p(fd.ptr + 4))):
        assert fit(**kw) == L.OFC_EINVAL, kw
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        t = np.array([4.0, bad, 1.0])
        assert fit(t=L.ptr(t)) == L.OFC_EINVAL, bad
        assert lib.ofc_motion_fit(0, L.ptr(f), 64, 48, 1, 2, L.ptr(t), 3, mp, sp, None, None) == L.OFC_EINVAL
        assert lib.ofc_motion_compensate(0, L.ptr(f), 64, 48, 1, 2, L.ptr(t), 3, L.ptr(res), mp, sp, None, None) == L.OFC_EINVAL
    assert "threshold" in lib.ofc_last_error().decode()
    assert fit(W=8192, H=8192) == L.OFC_EUNSUPPORTED and fit(n=65536) == L.OFC_EUNSUPPORTED
    assert fit(dev=99) == L.OFC_ENODEV
    assert fit(T=0, t=None) == L.OFC_OK and status[0] == 0                       # T = 0 needs no thresholds
    models[:], status[:] = 9.0, -1
    for args in ((None, 64, 48, 1, 2, tp, 3, mp, sp), (L.ptr(f), 64, 48, 1, 2, tp, 3, None, sp), (L.ptr(f), 64, 48, 1, 2, tp, 3, mp, None),
                 (L.ptr(f), 64, 48, 1, 5, tp, 3, mp, sp), (L.ptr(f), 64, 48, 1, 2, tp, 9, mp, sp), (L.ptr(f), 64, 48, 0, 2, tp, 3, mp, sp)):
        assert lib.ofc_motion_fit(0, *args, None, None) == L.OFC_EINVAL
        assert lib.ofc_motion_compensate(0, *args[:7], L.ptr(res), *args[7:], None, None) == L.OFC_EINVAL
    assert lib.ofc_motion_compensate(0, L.ptr(f), 64, 48, 1, 2, tp, 3, None, mp, sp, None, None) == L.OFC_EINVAL
    one = np.zeros((1, 6))
    c = np.array([4.0])
    for args in ((None, 64, 48, 1, L.ptr(one), L.ptr(c), L.ptr(mom)), (fp, 64, 48, 1, L.ptr(one), None, L.ptr(mom)),
                 (fp, 64, 48, 1, L.ptr(one), L.ptr(c), None), (fp, 64, 48, 0, None, None, L.ptr(mom)),
                 (fp, 64, 48, 1, L.ptr(one), L.ptr(np.array([0.0])), L.ptr(mom)),
                 (fp, 64, 48, 1, L.ptr(np.full((1, 6), np.nan)), L.ptr(c), L.ptr(mom))):
        assert lib.ofc_motion_moments_dev(0, *args) == L.OFC_EINVAL
    assert lib.ofc_motion_moments_dev(0, fp, 8192, 8192, 1, None, None, L.ptr(mom)) == L.OFC_EUNSUPPORTED
    for args in ((None, 64, 48, 1, L.ptr(one), fp), (fp, 64, 48, 1, None, fp), (fp, 64, 48, 1, L.ptr(one), None),
                 (fp, 64, 48, 1, L.ptr(one), C.c_void_p(fd.ptr + 4)), (fp, 64, 48, 1, L.ptr(np.full((1, 6), np.inf)), fp),
                 (fp, 0, 48, 1, L.ptr(one), fp)):
        assert lib.ofc_motion_subtract_dev(0, *args) == L.OFC_EINVAL
    for args in ((None, 64, 48, 1, 0, 1, C.byref(ms)), (fp, 64, 48, 1, 5, 1, C.byref(ms)), (fp, 64, 48, 1, 0, 0, C.byref(ms)),
                 (fp, 64, 48, 1, 0, 1, None), (fp, 1, 48, 1, 0, 1, C.byref(ms))):
        assert lib.ofc_bench_motion(0, *args) == L.OFC_EINVAL
    # nothing was written by any refused call, and the field is as it was
    assert (models == 9.0).all() and (status == -1).all() and (mom == -7).all() and (res == 5.0).all() and ms.value == -1.0
    assert np.array_equal(bits(fd.download(f.shape, np.float32)), bits(f))
    for what in range(5):
        assert lib.ofc_bench_motion(0, fp, 64, 48, 1, what, 2, C.byref(ms)) == L.OFC_OK and ms.value > 0
    assert np.array_equal(bits(fd.download(f.shape, np.float32)), bits(f))      # the hook subtracts into its own buffer
    fd.free()


# ---- ClipPipeline ----
def test_clip_pipeline_compensate_camera():
    from opticalflowclustering_amd import camera as cam
    from opticalflowclustering_amd.cluster import KMeans
    from opticalflowclustering_amd.pipeline import ClipPipeline
    pipe = ClipPipeline(CC.CLIP_W, CC.CLIP_H, CC.CLIP_FRAMES, batch_pairs=2)
    try:
        pipe.synth()
        pipe.run_flow()
        C0, _ = pipe.seed_kmeans(3, random_state=5)
        pipe.run_kmeans(C0)
        assert pipe.cell_clusters(3, 4).shape == (3, 12, 3)
        before = pipe.flows_host()
        cm = pipe.compensate_camera()
        after = pipe.flows_host()
        want, cm_host = cam.compensate(before)
        assert np.array_equal(bits(after), bits(want)) and not np.array_equal(bits(after), bits(before))
        assert all(np.array_equal(a, b) for a, b in zip(cm, cm_host)) and cm.params.shape == (3, 6)
        with pytest.raises(ValueError, match="run_kmeans"):                      # the labels were the old field's
            pipe.cell_clusters(3, 4)
        assert not pipe._sums_valid                                              # and so were the engine's column sums
        X = after.reshape(-1, 2)
        C1 = np.array([[0.0, 0.0], [0.5, -0.25], [-0.5, 0.5]])
        centers, inertia, n_iter = pipe.run_kmeans(C1)
        km = KMeans(3, init=C1).fit(X)
        assert np.array_equal(bits(centers), bits(km.cluster_centers_)) and n_iter == km.n_iter_
        assert np.array_equal(pipe.labels_host().ravel(), km.labels_)
        assert pipe.cell_clusters(3, 4).sum() == 3 * 64 * 48
        tr = pipe.compensate_camera("translation", (2.0,))                       # again, on the residual, with other arguments
        want2, tr_host = cam.compensate(after, "translation", (2.0,))
        assert np.array_equal(bits(pipe.flows_host()), bits(want2)) and not tr.params[:, [1, 2, 4, 5]].any()
        assert all(np.array_equal(a, b) for a, b in zip(tr, tr_host))
        with pytest.raises(ValueError, match="model should be"):
            pipe.compensate_camera("projective")
    finally:
        pipe.close()


# ---- the stream ----
def _stream(**kw):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(UC.STREAM_W, UC.STREAM_H, batch_pairs=CC.STREAM_BATCH, rows=CC.STREAM_GRID[0], cols=CC.STREAM_GRID[1], **kw)


@pytest.fixture(scope="module")
def clip():
    """five frames, their four pairwise fields (the engine's, one pair at a time), what compensate makes of them, and what a
    plain stream delivers: read-only"""
    from types import SimpleNamespace
    from opticalflowclustering_amd import camera as cam
    from opticalflowclustering_amd.flow import FlowEngine
    from opticalflowclustering_amd.vis import grid_assign_counts
    frames = UC.stream_clip(CC.STREAM_FRAMES)
    eng = FlowEngine(UC.STREAM_W, UC.STREAM_H, max_batch=1)
    fields = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    eng.close()
    residual, motion = cam.compensate(fields, "affine")
    st = _stream(centers=UC.STREAM_CENTRES, histogram=UC.STREAM_PARAMS)
    for f in frames:
        st.push(f)
    cells, counts = st.finish_clusters()
    table = st.histogram().table
    st.close()
    res_counts = grid_assign_counts(residual, UC.STREAM_CENTRES, *CC.STREAM_GRID)
    for a in (frames, fields, residual, cells, counts, table, res_counts):
        a.setflags(write=False)
    return SimpleNamespace(frames=frames, fields=fields, residual=residual, motion=motion, cells=cells, counts=counts,
                           table=table, res_counts=res_counts)


@pytest.mark.parametrize("n_frames", (5, 4), ids=["two-batches", "a-batch-and-the-flush"])
def test_stream_with_a_camera_sees_the_residual_field(clip, n_frames):
    from opticalflowclustering_amd.stream import grid_cell_mean_flow
    from opticalflowclustering_amd.uvhist import uv_histogram
    n = n_frames - 1
    st = _stream(camera="affine", centers=UC.STREAM_CENTRES, histogram=UC.STREAM_PARAMS)
    assert st.camera == ("affine", (4.0, 2.0, 1.0))
    for f in clip.frames[:n_frames]:
        st.push(f)
    cells, counts = st.finish_clusters()
    cm = st.camera_motion()
    assert np.array_equal(bits(cm.params), bits(clip.motion.params[:n])) and np.array_equal(cm.status, clip.motion.status[:n])
    assert np.abs(cm.params[:, [0, 3]]).max() > 0.2                              # the clip does pan
    want = np.stack([grid_cell_mean_flow(clip.residual[i], *CC.STREAM_GRID) for i in range(n)])
    assert np.array_equal(bits(cells), bits(want))
    assert np.array_equal(counts, clip.res_counts[:n])
    assert np.array_equal(st.histogram().table, uv_histogram(clip.residual[:n], *UC.STREAM_PARAMS).table)
    assert np.array_equal(bits(st.camera_motion().params), bits(cm.params))      # still there until frames arrive
    st.close()


def test_stream_set_camera_preconditions_and_removal(clip):
    L = _L()
    st = _stream(centers=UC.STREAM_CENTRES, histogram=UC.STREAM_PARAMS)
    with pytest.raises(ValueError, match="no camera"):
        st.camera_motion()
    st.set_camera("translation", (3.0,))
    assert st.camera == ("translation", (3.0,))
    st.push(clip.frames[0])
    for cam_arg in ("affine", None):
        with pytest.raises(ValueError, match="holds frames"):                    # refused while frames are held
            st.set_camera(cam_arg)
    with pytest.raises(ValueError, match="holds frames"):
        st.camera_motion()
    assert st.camera == ("translation", (3.0,))
    for f in clip.frames[1:]:
        st.push(f)
    cells, counts = st.finish_clusters()
    from opticalflowclustering_amd import camera as cam
    res, motion = cam.compensate(clip.fields, "translation", (3.0,))
    assert np.array_equal(bits(st.camera_motion().params), bits(motion.params))
    assert not np.array_equal(bits(cells), bits(clip.cells))
    small = np.zeros((1, 6))
    assert L.load().ofc_stream_read_camera(st._h, L.ptr(small), None, 1) == L.OFC_EINVAL and not small.any()
    assert L.load().ofc_stream_read_camera(st._h, None, None, 4) == L.OFC_OK
    thr = np.array([4.0, 0.0])
    for kind, t, T in ((3, thr, 1), (2, thr, 2), (2, thr, 9), (2, None, 1), (-1, thr, 1)):
        assert L.load().ofc_stream_set_camera(st._h, kind, L.ptr(t) if t is not None else None, T) == L.OFC_EINVAL
    assert L.load().ofc_stream_set_camera(None, 2, L.ptr(thr), 1) == L.OFC_EINVAL
    assert L.load().ofc_stream_read_camera(None, None, None, 0) == L.OFC_EINVAL
    st.histogram()                                                               # start the table over
    st.set_camera(None)                                                          # removed: today's output, bit for bit
    assert st.camera is None
    for f in clip.frames:
        st.push(f)
    cells, counts = st.finish_clusters()
    assert np.array_equal(bits(cells), bits(clip.cells)) and np.array_equal(counts, clip.counts)
    assert np.array_equal(st.histogram().table, clip.table)
    with pytest.raises(ValueError, match="no camera"):
        st.camera_motion()
    st.close()


def test_stream_camera_fits_grow_past_their_first_allocation(clip):
    """frames cycling through 4 distinct images, 261 pushes at batch_pairs = 8: the 33rd batch takes the per-pair records
    past their 256 pairs.  Pair t is (image t % 4, image (t + 1) % 4), so its fit equals that of pair t % 4"""
    from opticalflowclustering_amd import camera as cam
    from opticalflowclustering_amd.flow import FlowEngine
    from opticalflowclustering_amd.stream import FlowStream
    images = clip.frames[:4]
    eng = FlowEngine(UC.STREAM_W, UC.STREAM_H, max_batch=1)
    fields = np.stack([eng.calc(images[t], images[(t + 1) % 4]) for t in range(4)])
    eng.close()
    residual, motion = cam.compensate(fields, "affine")
    assert len(np.unique(motion.params, axis=0)) == 4                            # the four pairs differ: a misplaced row shows
    st = FlowStream(UC.STREAM_W, UC.STREAM_H, batch_pairs=8, rows=2, cols=3, camera="affine")
    for t in range(261):
        st.push(images[t % 4])
    cells = st.finish()
    cm = st.camera_motion()
    assert cm.params.shape == (260, 6) and len(cells) == 260
    assert np.array_equal(bits(cm.params), bits(motion.params[np.arange(260) % 4]))
    assert np.array_equal(cm.status, motion.status[np.arange(260) % 4])
    st.close()


# ---- the command line ----
def test_motion_grids_camera_on_the_resident_route_and_on_the_stream(tmp_path):
    from opticalflowclustering_amd import camera as cam
    from opticalflowclustering_amd import motionGrids as G
    from opticalflowclustering_amd.flow import FlowEngine
    from opticalflowclustering_amd.vis import bgr2gray, grid_assign_counts
    names = ("clip.npy", "fit.csv", "model.npy", "res.csv", "stream.csv", "cam_fit.npy", "cam_res.npy", "cam_stream.npy", "plain.csv")
    clip_path, fit_csv, model, res_csv, stream_csv, cam_fit, cam_res, cam_stream, plain_csv = (str(tmp_path / n) for n in names)
    frames = MC.moving_blobs_clip()
    frames = np.stack([np.roll(fr, (t, 2 * t), (0, 1)) for t, fr in enumerate(frames)])      # a pan on top of the blobs
    np.save(clip_path, frames)
    gray = np.stack([bgr2gray(f) for f in frames])
    eng = FlowEngine(gray.shape[2], gray.shape[1], max_batch=1)
    fields = np.stack([eng.calc(gray[t], gray[t + 1]) for t in range(len(gray) - 1)])
    eng.close()
    residual, motion = cam.compensate(fields, "affine", (3.0, 1.5))
    base = ["--path", clip_path, "-c", "3", "--rows", "3", "--cols", "4", "--camera", "affine", "--camera-thresholds", "3,1.5"]
    _, centres = G.main(base + ["-f", fit_csv, "--seed", "5", "--save-model", model, "--camera-out", cam_fit])
    res_counts, _ = G.main(base + ["-f", res_csv, "--model", model, "--camera-out", cam_res])
    stream_counts, _ = G.main(base + ["-f", stream_csv, "--model", model, "--stream", "--batch-pairs", "3", "--camera-out", cam_stream])
    for path in (cam_fit, cam_res, cam_stream):                                  # every route removed the same camera
        assert np.array_equal(bits(np.load(path)), bits(motion.params))
    assert np.abs(motion.params[:, 0] - 2.0).max() < 0.5 and np.abs(motion.params[:, 3] - 1.0).max() < 0.5
    assert np.array_equal(stream_counts, grid_assign_counts(residual, centres, 3, 4))
    # the two labelling routes centre differently (README): pixels on a border between two centres may differ, cells do not
    assert open(res_csv).read() == open(stream_csv).read()
    assert np.abs(res_counts.astype(np.int64) - stream_counts).sum() <= 0.001 * stream_counts.sum()
    plain_counts, _ = G.main(base[:8] + ["-f", plain_csv, "--model", model, "--stream", "--batch-pairs", "3"])
    assert np.array_equal(plain_counts, grid_assign_counts(fields, centres, 3, 4))   # without --camera: as before
    assert not np.array_equal(plain_counts, stream_counts)
