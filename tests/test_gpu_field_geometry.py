"""The kernels that sweep a whole flow field at the launch geometry of full-size clips: k_motion_moments, k_motion_solve and
k_motion_subtract over several shares per work-group, short and empty groups and more than 64 partials; the stream's camera
where the flush gets another geometry than the full batch; k_flow_weights and k_blob_keys past their grid caps; the grid
counts across the 65 535-frame chunk of gridDim.y.  The shapes, and why each is there, are tests/field_geometry_cases.py's;
test_field_geometry_host.py proves on the CPU, through ofc_motion_launch_geometry, that they reach what they claim and that
every motion case is well-conditioned.

No new bar: the moments are integers and compared with array_equal against camera_motion_cases' reference, models to the
solve bound and to equal bits against the host solve, the subtraction to one f32 ulp plus the reference's own rounding
(test_gpu_camera_motion.py's bars and helpers); 'moving' weights and threshold keys equal numpy's f32 expression,
'magnitude' within 1 ulp of it (test_gpu_lloyd_weighted.py); model keys equal ofc_lloyd_step_dev's bytes
(test_gpu_blobs.py's bar and helpers); counts equal motion_grid_cases' model, sums within its f64 bound."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import camera_motion_cases as CC
from tests import field_geometry_cases as F
from tests import motion_grid_cases as MC
from tests.test_gpu_blobs import keys_dev, moving_weights, step_labels
from tests.test_gpu_camera_motion import bits, fit_dev, host_solve, moments_dev, subtract_dev

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------------
# the motion kernels
# ---------------------------------------------------------------------------------------------------------------------
def motion_case(case):
    """the batch (npair, H, W, 2), the reference fit of every distinct field, and which field each pair carries"""
    shape, kind = case
    fields, fits, layout = F.motion_reference(shape, kind)
    return shape, CC.KIND[kind], fields[layout], fits, layout


@pytest.mark.parametrize("case", F.MOTION_CASES, ids=F.motion_case_id)
def test_moments_equal_the_reference_in_every_round(case):
    shape, kind, f, fits, layout = motion_case(case)
    got = moments_dev(f)
    assert np.array_equal(got, np.array([fits[l]["full"][0] for l in layout], dtype=np.int64))
    for t, c in enumerate(F.THRESHOLDS, start=1):
        got = moments_dev(f, np.stack([fits[l]["models"][t - 1] for l in layout]), c)
        taken = np.array([t < len(fits[l]["full"]) for l in layout])                     # the rounds the pair takes
        want = np.array([fits[l]["full"][t] if t < len(fits[l]["full"]) else [0] * CC.NMOM for l in layout], dtype=np.int64)
        assert np.array_equal(got[taken], want[taken]), (case, t)
        assert np.array_equal(got[:, 12], [fits[l]["full"][0][12] for l in layout])      # outside does not depend on the selection


@pytest.mark.parametrize("case", F.MOTION_CASES, ids=F.motion_case_id)
def test_fit_history_status_and_models(case):
    shape, kind, f, fits, layout = motion_case(case)
    models, status, hm, hq = fit_dev(f, kind, F.THRESHOLDS)
    assert np.array_equal(hq, np.stack([fits[l]["moments"] for l in layout], 1))
    assert np.array_equal(status, [fits[l]["status"] for l in layout])
    assert np.array_equal(bits(models), bits(hm[-1]))
    for i in [int(np.argmax(layout == l)) for l in range(len(fits))]:                    # one pair of every distinct field ...
        ref = fits[layout[i]]
        kept, solved = np.zeros(6), 0
        for t in range(len(F.THRESHOLDS) + 1):
            p, st = host_solve(hq[t, i], kind) if t < len(ref["full"]) else (None, 1)
            if st == 0:                                                                  # host and device run one function
                kept, solved = p, solved + 1
                want, kappa = CC.solve_exact([int(v) for v in hq[t, i]], kind)
                err, bound = np.abs(hm[t, i] - want).max(), CC.solve_bound(kappa, want)
                assert err <= bound, (case, t, i, err, bound)
            assert np.array_equal(bits(hm[t, i]), bits(kept)), (case, t, i)
        assert solved == len(ref["kappa"])
        same = np.flatnonzero(layout == layout[i])                                       # ... and the others are its bits
        assert np.array_equal(bits(hm[:, same]), np.broadcast_to(bits(hm[:, i])[:, None], (len(hm), len(same), 6))), (case, i)


@pytest.mark.parametrize("case", F.MOTION_CASES, ids=F.motion_case_id)
def test_subtraction_within_one_ulp_and_in_place_equals_out_of_place(case):
    shape, kind, f, fits, layout = motion_case(case)
    models = fit_dev(f, kind, F.THRESHOLDS)[0]
    out = subtract_dev(f, models, in_place=False)
    assert np.array_equal(bits(subtract_dev(f, models, in_place=True)), bits(out))
    for l in range(len(fits)):
        i = int(np.argmax(layout == l))
        finite = np.isfinite(f[i]).all(-1)
        eu, ev = CC.predict(models[i], shape.W, shape.H)
        with np.errstate(invalid="ignore", over="ignore"):
            want = np.stack([f[i, ..., 0].astype(np.float64) - eu, f[i, ..., 1].astype(np.float64) - ev], -1)
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            # the reference's own error, as test_gpu_camera_motion.py states it: at most 2^-52 of the terms' magnitudes
            m = np.abs(models[i])
            hx, hy = np.abs(CC.predict(np.array([0, 1, 0, 0, 0, 1.0]), shape.W, shape.H))
            own = 2.0 ** -52 * np.stack([m[0] + m[1] * hx + m[2] * hy, m[3] + m[4] * hx + m[5] * hy], -1)
            own = own + 2.0 ** -52 * np.abs(np.where(np.isfinite(f[i]), f[i], 0)).astype(np.float64)
        assert (np.abs(out[i][finite].astype(np.float64) - want[finite]) <= ulp[finite] + own[finite]).all(), (case, l)
        assert np.array_equal(bits(out[i][~finite]), bits(f[i][~finite]))                # a non-finite vector passes through
        if l == 4:
            assert (~finite).sum() == 6 and np.isfinite(out[i][~finite]).any()
        if l == 5:                                                                       # status 2: the zero model, the field's bits
            assert not models[i].any() and np.array_equal(bits(out[i][finite]), bits(f[i][finite]))
        same = np.flatnonzero(layout == l)                                               # equal fields, equal models: equal bits
        assert np.array_equal(bits(models[same]), np.broadcast_to(bits(models[i]), (len(same), 6)))
        assert all(np.array_equal(bits(out[j]), bits(out[i])) for j in same), (case, l)


def test_a_pair_of_the_batch_equals_a_call_on_it_alone():
    """16 groups of 3 shares in the batch, 34 groups of 1 share alone: the partial layout does not leak into results"""
    shape = F.MOTION_BY_NAME[F.ONE_BY_ONE]
    for kind in shape.kinds:
        _, k, f, fits, layout = motion_case((shape, kind))
        mb, sb, hmb, hqb = fit_dev(f, k, F.THRESHOLDS)
        qb = moments_dev(f, mb, 2.0)
        outb = subtract_dev(f, mb, in_place=True)
        for i in range(shape.npair):
            m1, s1, hm1, hq1 = fit_dev(f[i:i + 1], k, F.THRESHOLDS)
            assert np.array_equal(bits(m1[0]), bits(mb[i])) and s1[0] == sb[i], (kind, i)
            assert np.array_equal(bits(hm1[:, 0]), bits(hmb[:, i])) and np.array_equal(hq1[:, 0], hqb[:, i]), (kind, i)
            assert np.array_equal(moments_dev(f[i:i + 1], mb[i:i + 1], 2.0)[0], qb[i]), (kind, i)
            assert np.array_equal(bits(subtract_dev(f[i:i + 1], mb[i:i + 1], in_place=False)[0]), bits(outb[i])), (kind, i)


# ---------------------------------------------------------------------------------------------------------------------
# the stream's camera: a full batch of 24 pairs (85 groups of 2 shares) and a flush of 3 (101 groups of 1)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    """the frames, their pairwise fields (the engine's, one pair at a time) and what compensate makes of them: read-only"""
    from opticalflowclustering_amd import camera as cam
    from opticalflowclustering_amd.flow import FlowEngine
    frames = F.stream_clip()
    eng = FlowEngine(F.STREAM_W, F.STREAM_H, max_batch=1)
    fields = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    eng.close()
    residual, motion = cam.compensate(fields, "affine")
    for a in (frames, fields, residual):
        a.setflags(write=False)
    return SimpleNamespace(frames=frames, fields=fields, residual=residual, motion=motion)


def test_stream_camera_across_a_flush_that_changes_the_geometry(clip):
    from opticalflowclustering_amd.stream import FlowStream, grid_cell_mean_flow
    from opticalflowclustering_amd.uvhist import uv_histogram
    from opticalflowclustering_amd.vis import grid_assign_counts
    n = F.STREAM_PUSHES - 1
    st = FlowStream(F.STREAM_W, F.STREAM_H, batch_pairs=F.STREAM_BATCH, rows=F.STREAM_GRID[0], cols=F.STREAM_GRID[1],
                    camera="affine", centers=F.STREAM_CENTRES, histogram=F.STREAM_PARAMS)
    try:
        for fr in clip.frames:
            st.push(fr)
        cells, counts = st.finish_clusters()
        cm = st.camera_motion()
        table = st.histogram().table
    finally:
        st.close()
    assert cm.params.shape == (n, 6) and len(cells) == n == F.STREAM_BATCH + F.STREAM_FLUSH
    assert np.array_equal(bits(cm.params), bits(clip.motion.params)) and np.array_equal(cm.status, clip.motion.status)
    assert not clip.motion.status.any() and np.abs(cm.params[:, [0, 3]]).max() > 0.2   # the clip does pan, every pair is fitted
    assert len(np.unique(cm.params, axis=0)) == n                                        # no two pairs alike: a misplaced row shows
    want = np.stack([grid_cell_mean_flow(clip.residual[i], *F.STREAM_GRID) for i in range(n)])
    assert np.array_equal(bits(cells), bits(want))
    assert np.array_equal(counts, grid_assign_counts(clip.residual, F.STREAM_CENTRES, *F.STREAM_GRID))
    assert np.array_equal(table, uv_histogram(clip.residual, *F.STREAM_PARAMS).table)


# ---------------------------------------------------------------------------------------------------------------------
# flow weights and blob keys past their grid caps
# ---------------------------------------------------------------------------------------------------------------------
def test_flow_weights_past_the_grid_cap():
    from opticalflowclustering_amd import stages
    L = _L()
    n = F.WEIGHTS_N
    f = F.weights_field()
    u, v = f[:, 0], f[:, 1]
    with np.errstate(invalid="ignore"):
        s = u * u + v * v                                                                # f32, every operation rounded
        thr = np.float32(F.THR)
        moving, mag = (s >= thr * thr).astype(np.float32), np.sqrt(s)
    fb = L.DeviceBuffer(f.nbytes).upload(f)
    wb = L.DeviceBuffer(n * 4 + 16)
    try:
        for kind, t in (("moving", float(thr)), ("magnitude", 0.0)):
            L.check(L.load().ofc_memset(0, C.c_void_p(wb.ptr), 0x55, wb.nbytes))
            stages.flow_weights_dev(fb.ptr, n, kind, t, wb.ptr)
            got = wb.download((n,), np.float32)
            assert (wb.download((16,), np.uint8, offset=n * 4) == 0x55).all()           # nothing past the last weight
            if kind == "moving":
                bad = np.flatnonzero(got != moving)
                assert not len(bad), (len(bad), bad[:8], bad[:8] // F.WEIGHTS_PASS)
            else:
                fin = np.isfinite(mag)
                assert np.array_equal(np.isnan(got), np.isnan(mag)) and np.array_equal(np.isinf(got), np.isinf(mag))
                bad = np.flatnonzero(np.abs(got[fin].astype(np.float64) - mag[fin]) > np.spacing(mag[fin]).astype(np.float64))
                assert not len(bad), (len(bad), np.flatnonzero(fin)[bad[:8]])
        assert np.array_equal(bits(fb.download(f.shape, np.float32)), bits(f))           # the field is only read
    finally:
        fb.free()
        wb.free()
    # every part of the sweep held something to get wrong: both passes and the tail carry 0s and 1s and the specials
    for lo, hi in ((0, F.WEIGHTS_PASS), (F.WEIGHTS_PASS, n - 3), (n - 3, n)):
        assert 0 < moving[lo:hi].sum() < hi - lo, (lo, hi)
    assert np.isnan(mag[[0, F.WEIGHTS_PASS, n - 8]]).all() and np.isinf(mag[[1, F.WEIGHTS_PASS + 1, n - 7]]).all()


@pytest.fixture(scope="module")
def keys_case():
    """the field past the key kernel's cap, its f32 squared lengths, and the same field with its non-finite vectors set to
    zero for the model (the E-step kernels are not specified on NaN): read-only"""
    f = F.keys_field()
    with np.errstate(invalid="ignore"):
        s = f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]
    finite = np.where(np.isfinite(f).all(-1, keepdims=True), f, np.float32(0))
    for a in (f, s, finite):
        a.setflags(write=False)
    return SimpleNamespace(f=f, s=s, finite=finite)


def test_threshold_keys_past_the_grid_cap(keys_case):
    f, s = keys_case.f, keys_case.s
    keys = keys_dev(f, thr=F.THR)                                                        # 16-byte aligned: four vectors per lane
    one = keys_dev(f, thr=F.THR, shift=1)                                                # shifted: one per lane, four passes
    t2 = np.float32(F.THR) * np.float32(F.THR)
    with np.errstate(invalid="ignore"):
        want = np.where(s >= t2, 0, 255).astype(np.uint8)
    for got in (keys, one):
        bad = np.flatnonzero(got.ravel() != want.ravel())
        assert not len(bad), (len(bad), bad[:8], bad[:8] // F.KEYS_PASS_ONE)
    assert np.array_equal(keys == 0, moving_weights(f, F.THR) == 1.0)
    flat = want.ravel()
    for lo, hi in ((0, F.KEYS_PASS_ONE), (3 * F.KEYS_PASS_ONE, F.KEYS_PASS_VEC), (F.KEYS_PASS_VEC, F.KEYS_N - 2), (F.KEYS_N - 2, F.KEYS_N)):
        assert (flat[lo:hi] == 0).any() and (flat[lo:hi] == 255).any(), (lo, hi)         # every pass has both keys to write


@pytest.mark.parametrize("merge", [0, 1])
def test_model_keys_past_the_grid_cap(keys_case, merge):
    f = keys_case.finite
    k, mean, cen = F.KEYS_K, F.KEYS_MEAN, np.ascontiguousarray(F.KEYS_CENTRES_C)
    lab = step_labels(f, k, mean, cen)
    assert set(np.unique(lab)) == set(range(k))
    chosen = ((F.KEYS_SELECT >> lab.astype(np.int64)) & 1).astype(bool)
    assert 0.2 < chosen.mean() < 0.9
    want = np.where(chosen, 0 if merge else lab, 255).astype(np.uint8)
    for shift in (0, 1):
        got = keys_dev(f, k=k, mean=mean, centers_c=cen, select=F.KEYS_SELECT, merge=merge, shift=shift)
        bad = np.flatnonzero(got.ravel() != want.ravel())
        assert not len(bad), (shift, len(bad), bad[:8], bad[:8] // F.KEYS_PASS_ONE)
    with np.errstate(invalid="ignore"):
        moving = keys_case.s >= np.float32(F.THR) * np.float32(F.THR)                    # zeros where f was not finite
    moving = moving & np.isfinite(keys_case.f).all(-1)
    got = keys_dev(f, thr=F.THR, k=k, mean=mean, centers_c=cen, select=F.KEYS_SELECT, merge=merge, shift=merge)
    assert np.array_equal(got, np.where(moving, want, 255))


# ---------------------------------------------------------------------------------------------------------------------
# grid counts across the 65 535-frame chunk
# ---------------------------------------------------------------------------------------------------------------------
def _edges_differ(counts, sums):
    edge = [0, F.GRID_CHUNK - 1, F.GRID_CHUNK, F.GRID_CHUNK + 1]                         # frames 0, 65534, 65535, 65536
    for a in edge + [F.GRID_CHUNK - 2]:
        for b in edge:
            if a != b:
                assert not np.array_equal(counts[a], counts[b]) and not np.array_equal(sums[a], sums[b]), (a, b)


def _check_counts(got_c, got_s, only_c, counts, sums, abs_sums):
    bad = np.flatnonzero((got_c != counts).any(axis=(1, 2)))
    assert not len(bad), (len(bad), bad[:8])
    assert np.array_equal(only_c, counts)                                                # the counts-only kernel
    bound = MC.sum_bound(counts, abs_sums)
    late = np.flatnonzero((np.abs(got_s - sums) > bound).any(axis=(1, 2, 3)))
    assert not len(late), (len(late), late[:8])
    empty = np.broadcast_to((counts == 0)[..., None], got_s.shape)
    assert not got_s.view(np.int64)[empty].any()                                         # +0.0 where nobody is counted


@pytest.mark.parametrize("k", F.GRID_KS)
def test_grid_label_counts_across_the_frame_chunk(k):
    from opticalflowclustering_amd.vis import grid_label_counts
    rows, cols = F.GRID_ROWS, F.GRID_COLS
    lab, fl = F.grid_labels(k), F.grid_flow()
    counts, sums = F.counts_all_frames(lab, k, rows, cols, fl)
    _edges_differ(counts, sums)
    got_c, got_s = grid_label_counts(lab, k, rows, cols, flow=fl)
    _check_counts(got_c, got_s, grid_label_counts(lab, k, rows, cols), counts, sums,
                  F.counts_all_frames(lab, k, rows, cols, fl, absolute=True)[1])


@pytest.mark.parametrize("k", F.GRID_KS)
def test_grid_assign_counts_across_the_frame_chunk(k):
    from opticalflowclustering_amd.vis import grid_assign_counts
    rows, cols = F.GRID_ROWS, F.GRID_COLS
    fl = F.grid_flow()
    rng = np.random.default_rng(900 + k)
    cen, mean = rng.uniform(-4, 4, (k, 2)), rng.uniform(-0.5, 0.5, 2)
    lab = step_labels(fl, k, mean, np.ascontiguousarray(cen - mean))                     # the labels the fused kernel has to count
    counts, sums = F.counts_all_frames(lab, k, rows, cols, fl)
    _edges_differ(counts, sums)
    got_c, got_s = grid_assign_counts(fl, cen, rows, cols, mean=mean, sums=True)
    _check_counts(got_c, got_s, grid_assign_counts(fl, cen, rows, cols, mean=mean), counts, sums,
                  F.counts_all_frames(lab, k, rows, cols, fl, absolute=True)[1])


def test_a_stream_batch_cannot_pass_a_grid_dimension():
    """k_grid_cell_mean_flow and the motion kernels take a stream's batch in gridDim.y: the engine behind the stream keeps
    a batch to 4096 pairs, decided on the host"""
    L = _L()
    h = C.c_void_p()
    for batch in (4097, 65536):
        assert L.load().ofc_stream_create(0, 64, 48, None, batch, 2, 3, C.byref(h)) == L.OFC_EINVAL and not h.value
        assert "max_batch" in L.load().ofc_last_error().decode()
