"""The photometric check on the device (photo_check.hip): the state map, the stats and the warped frames on every case and
every threshold pair of tests/photometric_cases.py, on host buffers and on device buffers whose bases do not allow the wide
accesses, and the way up through photometric.py, ClipPipeline, FlowStream and the motionGrids command line.

Every output is an integer, so everything is compared with array_equal against the numpy reference of the case table;
test_photometric_host.py proves that reference against a per-pixel loop and that the table reaches what it is meant to."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import photometric_cases as PC

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _K():
    from opticalflowclustering_amd import photometric
    return photometric


def _B():
    from opticalflowclustering_amd import blobs
    return blobs


def _fill(buf, byte=0x55):
    L = _L()
    L.check(L.load().ofc_memset(0, C.c_void_p(buf.ptr), byte, buf.nbytes))


def same(got, want, warped=True):
    state, stats, wd = got
    ws, wt, ww = want
    assert state.dtype == np.uint8 and np.array_equal(state, ws), np.argwhere(state != ws)[:5]
    assert stats.dtype == np.int64 and np.array_equal(stats, wt), (stats, wt)
    if warped:
        assert wd.dtype == np.uint16 and np.array_equal(wd, ww), np.argwhere(wd != ww)[:5]
    else:
        assert wd is None


def photo_host(c, tau_q, kappa_q, warped):
    """ofc_photo: host buffers, whole chain"""
    L = _L()
    n, H, W = c.shape
    state, stats = np.full((n, H, W), 0x55, np.uint8), np.full((n, 5), -1, np.int64)
    wd = np.full((n, H, W), 0x5555, np.uint16) if warped else None
    L.check(L.load().ofc_photo(0, L.ptr(c.frames), L.ptr(c.fwd), W, H, n, tau_q, kappa_q, L.ptr(state), L.ptr(stats), L.ptr(wd)))
    return state, stats, wd


@pytest.mark.parametrize("case", PC.CASES, ids=repr)
def test_host_buffers_equal_the_reference_with_and_without_warped(case):
    for tau_q, kappa_q in case.thresholds():
        want = case.reference(tau_q, kappa_q)
        same(photo_host(case, tau_q, kappa_q, True), want)
        same(photo_host(case, tau_q, kappa_q, False), want, warped=False)
    same(photo_host(case, PC.TAU_Q, PC.KAPPA_Q, True), case.reference())         # a second call gives the same


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", PC.CASES, ids=repr)
def test_device_buffers_equal_the_reference_at_both_alignments(case, shift):
    """ofc_photo_dev; shift = 1 puts the field 8 bytes, the frames and the state map 1 byte and the warped frames 2 bytes past
    their buffers' starts, where the kernel can take neither four vectors, four grey values, four states nor four warped
    values at a time.  Checks that the inputs are left alone and that nothing is written in front of or past the outputs."""
    L = _L()
    n, H, W = case.shape
    N = n * H * W
    gd = L.DeviceBuffer(case.frames.nbytes + 16).upload(case.frames, offset=shift)
    fd = L.DeviceBuffer(case.fwd.nbytes + 16).upload(case.fwd, offset=8 * shift)
    sd, td, wd = L.DeviceBuffer(N + 16), L.DeviceBuffer(n * 40 + 16), L.DeviceBuffer(N * 2 + 32)
    try:
        for tau_q, kappa_q in case.thresholds():
            for warped in (True, False):
                for b in (sd, td, wd):
                    _fill(b)
                L.check(L.load().ofc_photo_dev(0, C.c_void_p(gd.ptr + shift), C.c_void_p(fd.ptr + 8 * shift), W, H, n, tau_q, kappa_q,
                                               C.c_void_p(sd.ptr + shift), C.c_void_p(td.ptr),
                                               C.c_void_p(wd.ptr + 2 * shift) if warped else None))
                raw = sd.download((N + 16,), np.uint8)
                assert (raw[:shift] == 0x55).all() and (raw[shift + N:] == 0x55).all()
                assert (td.download((16,), np.uint8, offset=n * 40) == 0x55).all()
                wraw = wd.download((N * 2 + 32,), np.uint8)
                if warped:
                    assert (wraw[:2 * shift] == 0x55).all() and (wraw[2 * shift + N * 2:] == 0x55).all()
                else:
                    assert (wraw == 0x55).all()
                got_w = wraw[2 * shift:2 * shift + N * 2].copy().view(np.uint16).reshape(n, H, W) if warped else None
                same((raw[shift:shift + N].reshape(n, H, W).copy(), td.download((n, 5), np.int64), got_w),
                     case.reference(tau_q, kappa_q), warped=warped)
        assert np.array_equal(gd.download(case.frames.shape, np.uint8, offset=shift), case.frames)
        assert np.array_equal(fd.download(case.fwd.shape, np.float32, offset=8 * shift).view(np.uint32), case.fwd.view(np.uint32))
    finally:
        for b in (gd, fd, sd, td, wd):
            b.free()


def test_check_takes_a_single_field_and_floats_and_says_what_it_used():
    K = _K()
    c = PC.BY_NAME["small-smooth-100x62-n2"]
    out = K.check(c.frames[:2], c.fwd[0], warped=True)
    assert (out.tau_q, out.kappa_q) == (PC.TAU_Q, PC.KAPPA_Q) and len(out) == 1
    want = tuple(a[:1] for a in c.reference())
    same((out.state, out.stats, out.warped), want)
    assert np.array_equal(out.counts, want[1][:, :4]) and np.array_equal(out.abs_error, want[1][:, 4])
    compared = want[1][0, 0] + want[1][0, 1]
    assert compared > 0 and out.mean_abs_error()[0] == want[1][0, 4] / (256.0 * compared)
    out = K.check(c.frames, c.fwd, tau=0.0, kappa=4.0)
    assert out.warped is None
    same((out.state, out.stats, None), c.reference(0, 1024), warped=False)


def test_the_device_calls_refuse_what_the_check_refuses_and_touch_nothing():
    L = _L()
    c = PC.BY_NAME["mixed-random-5x3-n3"]
    n, H, W = c.shape
    gd, fd = L.DeviceBuffer(c.frames.nbytes + 16).upload(c.frames), L.DeviceBuffer(c.fwd.nbytes + 16).upload(c.fwd)
    sd, td, wd = L.DeviceBuffer(256), L.DeviceBuffer(n * 40 + 8), L.DeviceBuffer(256)
    try:
        def call(frames=gd.ptr, fwd=fd.ptr, W=W, H=H, npair=n, tau_q=2048, kappa_q=128, state=sd.ptr, stats=td.ptr, warped=wd.ptr):
            return L.load().ofc_photo_dev(0, C.c_void_p(frames) if frames else None, C.c_void_p(fwd) if fwd else None, W, H, npair,
                                          tau_q, kappa_q, C.c_void_p(state) if state else None,
                                          C.c_void_p(stats) if stats else None, C.c_void_p(warped) if warped else None)

        assert call() == L.OFC_OK
        for b in (sd, td, wd):
            _fill(b)
        assert call(frames=None) == L.OFC_EINVAL and call(fwd=None) == L.OFC_EINVAL and call(state=None) == L.OFC_EINVAL
        assert call(stats=None) == L.OFC_EINVAL
        assert call(fwd=fd.ptr + 4) == L.OFC_EINVAL and call(stats=td.ptr + 4) == L.OFC_EINVAL and call(warped=wd.ptr + 1) == L.OFC_EINVAL
        assert call(W=0) == L.OFC_EINVAL and call(H=0) == L.OFC_EINVAL and call(npair=0) == L.OFC_EINVAL
        assert call(npair=65536) == L.OFC_EINVAL and call(W=16385) == L.OFC_EUNSUPPORTED and call(H=16385) == L.OFC_EUNSUPPORTED
        assert call(tau_q=-1) == L.OFC_EINVAL and call(tau_q=65281) == L.OFC_EINVAL
        assert call(kappa_q=-1) == L.OFC_EINVAL and call(kappa_q=1025) == L.OFC_EINVAL
        for b in (sd, wd):
            assert (b.download((256,), np.uint8) == 0x55).all()
        assert (td.download((n * 40 + 8,), np.uint8) == 0x55).all()                # not even the clear of the stats
        host = np.full(8, 0x55, np.uint8)
        lib = L.load()
        assert lib.ofc_photo(0, None, L.ptr(c.fwd), W, H, n, 2048, 128, L.ptr(host), L.ptr(host), None) == L.OFC_EINVAL
        assert lib.ofc_photo(0, L.ptr(c.frames), L.ptr(c.fwd), W, H, n, 2048, 1025, L.ptr(host), L.ptr(host), None) == L.OFC_EINVAL
        assert (host == 0x55).all()
        ms = C.c_float(-1.0)
        assert lib.ofc_bench_photo(0, C.c_void_p(gd.ptr), C.c_void_p(fd.ptr), W, H, n, 2, 1, C.byref(ms)) == L.OFC_EINVAL
        assert lib.ofc_bench_photo(0, C.c_void_p(gd.ptr), C.c_void_p(fd.ptr), W, H, 0, 0, 1, C.byref(ms)) == L.OFC_EINVAL
        assert ms.value == -1.0
        for what in (0, 1):
            L.check(lib.ofc_bench_photo(0, C.c_void_p(gd.ptr), C.c_void_p(fd.ptr), W, H, n, what, 2, C.byref(ms)))
            assert ms.value > 0
    finally:
        for b in (gd, fd, sd, td, wd):
            b.free()


# ---- ClipPipeline ----
PW, PH = 96, 64


def gray_clip(n):
    from tests import motion_grid_cases as MC
    return np.ascontiguousarray(MC.moving_blobs_clip(n, PW, PH)[..., 0])


def moving_keys(f, thr):
    s = f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]
    return np.where(s >= np.float32(thr) * np.float32(thr), 0, 255).astype(np.uint8)


def same_blobs(got, want, labels=True):
    assert np.array_equal(got.found, want.found) and len(got.records) == len(want.records)
    for a, b in zip(got.records, want.records):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    if labels:
        assert np.array_equal(got.labels, want.labels)


def test_pipeline_photometric_and_its_consumers():
    from opticalflowclustering_amd.pipeline import ClipPipeline
    B, K = _B(), _K()
    T = 6
    frames = gray_clip(T)
    n, P = T - 1, PW * PH
    pipe = ClipPipeline(PW, PH, T, batch_pairs=2)
    try:
        pipe.upload_frames(frames)
        pipe.run_flow()
        for call in (lambda: pipe.blobs(consistent=True), lambda: pipe.run_kmeans(np.zeros((2, 2)), consistent=True)):
            with pytest.raises(ValueError, match="consistency"):                  # the existing text, unchanged
                call()
        fwd = pipe.flows_host()
        for warped in (False, True):
            got = pipe.photometric(warped=warped)
            want = PC.reference(frames, fwd)
            same((got.state, got.stats, got.warped), want, warped=warped)
            assert np.array_equal(pipe.state.download((n, PH, PW), np.uint8), want[0])
        assert (got.tau_q, got.kappa_q) == (PC.TAU_Q, PC.KAPPA_Q) and (got.counts.sum(1) == P).all()
        assert np.array_equal(pipe.flows_host().view(np.uint32), fwd.view(np.uint32))
        assert np.array_equal(pipe.frames.download((T, PH, PW), np.uint8), frames)
        # whichever check ran last owns the map
        pipe.run_backward_flow()
        fb = pipe.consistency()
        assert np.array_equal(pipe.state.download((n, PH, PW), np.uint8), fb.state)
        strict = pipe.photometric(tau=2.0, kappa=0.25)
        tau_q, kappa_q = K.quantise(2.0, 0.25)
        want = PC.reference(frames, fwd, tau_q, kappa_q)
        same((strict.state, strict.stats, None), want, warped=False)
        state = want[0]
        assert np.array_equal(pipe.state.download((n, PH, PW), np.uint8), state) and not np.array_equal(state, fb.state)
        # blobs(consistent=True): the components of the host-masked keys
        plain = pipe.blobs(by="moving", thr=0.25)
        assert np.array_equal(plain.keys, moving_keys(fwd, 0.25))
        masked = np.where(state == PC.OK, plain.keys, 255).astype(np.uint8)
        assert (masked != plain.keys).any() and (masked == 0).any()
        got_b = pipe.blobs(by="moving", thr=0.25, consistent=True)
        assert np.array_equal(got_b.keys, masked)
        same_blobs(got_b, B.connected_components(masked, flow=fwd))
        # run_kmeans(consistent=True): the fit with the same weights zeroed on the host
        C0 = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, -2.0]])
        pipe.run_kmeans(C0, sample_weight=("moving", 0.5))
        w = pipe.weights.download((n * P,), np.float32)
        cen, inertia, n_iter = pipe.run_kmeans(C0, sample_weight=("moving", 0.5), consistent=True)
        wm = np.where(state.ravel() == PC.OK, w, np.float32(0))
        assert np.array_equal(pipe.weights.download((n * P,), np.float32), wm) and (wm != w).any() and wm.any()
        cen2, inertia2, n_iter2 = pipe.run_kmeans(C0, sample_weight=wm)
        assert np.array_equal(cen, cen2) and inertia == inertia2 and n_iter == n_iter2
        seeds, _ = pipe.seed_kmeans(3, 5, sample_weight=("moving", 0.5), consistent=True)
        seeds2, _ = pipe.seed_kmeans(3, 5, sample_weight=wm)
        assert np.array_equal(seeds, seeds2)
        with pytest.raises(ValueError, match="tau"):
            pipe.photometric(tau=256.0)
        pipe.compensate_camera("translation")
        with pytest.raises(ValueError, match="compensate_camera"):
            pipe.photometric()
        assert np.array_equal(pipe.state.download((n, PH, PW), np.uint8), state)  # the refusal left the map alone
        pipe.run_flow()
        assert pipe.state is None
        with pytest.raises(ValueError, match="consistency"):
            pipe.blobs(consistent=True)
    finally:
        pipe.close()


# ---- FlowStream ----
ST, THR = 9, 1.0
STRICT = dict(tau=2.0, kappa=0.25)


@pytest.fixture(scope="module")
def clip():
    """nine frames, their eight pairwise fields (the engine's, one pair at a time, as test_gpu_stream_clusters.py obtains the
    fields a stream saw) and the reference on them: once, read-only"""
    from opticalflowclustering_amd.flow import FlowEngine
    frames = gray_clip(ST)
    eng = FlowEngine(PW, PH, max_batch=1)
    fields = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(ST - 1)])
    eng.close()
    tau_q, kappa_q = _K().quantise(**STRICT)
    ref, strict = PC.reference(frames, fields), PC.reference(frames, fields, tau_q, kappa_q)
    for a in (frames, fields) + ref + strict:
        a.setflags(write=False)
    return SimpleNamespace(frames=frames, fields=fields, ref=ref, strict=strict)


def _stream(batch_pairs, **kw):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(PW, PH, batch_pairs=batch_pairs, rows=2, cols=3, **kw)


def _run(st, frames):
    for f in frames:
        st.push(f)
    return st.finish()


def test_stream_stats_equal_the_reference_whatever_the_batches_and_the_camera(clip):
    got = {}
    for batch in (3, 8):                                                          # 3 + 3 and a flush of 2; one full batch
        st = _stream(batch, photometric=True)
        assert st.photo_args == (PC.TAU_Q, PC.KAPPA_Q, 1)
        cells = _run(st, clip.frames)
        got[batch] = st.photometric_stats()
        assert got[batch].dtype == np.int64 and got[batch].shape == (ST - 1, 5)
        assert np.array_equal(st.photometric_stats(), got[batch])                 # still there until frames arrive
        plain = _stream(batch)                                                    # the cell means never depended on the check
        assert np.array_equal(_run(plain, clip.frames).view(np.uint32), cells.view(np.uint32))
        plain.close()
        st.set_camera("affine")                                                   # the check runs before the subtraction
        _run(st, clip.frames)
        assert np.array_equal(st.photometric_stats(), got[batch])
        _run(st, clip.frames[:5])                                                 # a second, shorter clip on the same stream
        assert np.array_equal(st.photometric_stats(), clip.ref[1][:4])
        st.close()
    assert np.array_equal(got[3], got[8]) and np.array_equal(got[3], clip.ref[1])
    assert (clip.ref[1][:, :4].sum(1) == PW * PH).all() and clip.ref[1][:, 0].min() > 0 and clip.ref[1][:, 4].min() > 0


@pytest.mark.parametrize("batch", (3, 8))
def test_stream_blobs_are_those_of_the_masked_key_maps_and_the_check_can_be_removed(clip, batch):
    from opticalflowclustering_amd import camera
    B = _B()
    spec = dict(thr=THR, connectivity=8, min_area=4, max_blobs=256)
    keys = moving_keys(clip.fields, THR)
    unmasked = B.connected_components(keys, min_area=4, max_blobs=256, flow=clip.fields)
    st = _stream(batch, blobs=spec)
    _run(st, clip.frames)
    same_blobs(st.blobs(), unmasked, labels=False)
    for keep, kept in (((0,), clip.strict[0] == PC.OK), ((0, 2), (clip.strict[0] == PC.OK) | (clip.strict[0] == PC.LEAVES))):
        st.set_photometric(keep=keep, **STRICT)
        _run(st, clip.frames)
        masked = np.where(kept, keys, 255).astype(np.uint8)
        assert (masked != keys).any() and (masked == 0).any()
        same_blobs(st.blobs(), B.connected_components(masked, min_area=4, max_blobs=256, flow=clip.fields), labels=False)
        assert np.array_equal(st.photometric_stats(), clip.strict[1])
    st.set_camera("translation", (3.0,))                                          # the states of the whole flow, the keys of the residual
    _run(st, clip.frames)
    res, _ = camera.compensate(clip.fields, "translation", (3.0,))
    masked = np.where(kept, moving_keys(res, THR), 255).astype(np.uint8)
    same_blobs(st.blobs(), B.connected_components(masked, min_area=4, max_blobs=256, flow=res), labels=False)
    assert np.array_equal(st.photometric_stats(), clip.strict[1])
    st.set_camera(None)
    st.set_photometric(on=False)                                                  # back to what it delivered before
    assert st.photo_args is None
    _run(st, clip.frames)
    same_blobs(st.blobs(), unmasked, labels=False)
    with pytest.raises(ValueError, match="no photometric"):
        st.photometric_stats()
    st.close()


def test_stream_set_photo_and_read_photo_refusals(clip):
    L = _L()
    lib = L.load()
    st = _stream(3)
    host = np.full((ST, 5), -7, np.int64)
    assert lib.ofc_stream_read_photo(st._h, L.ptr(host), ST) == L.OFC_EINVAL      # without the check
    assert "no photometric" in lib.ofc_last_error().decode()
    for on, tau_q, kappa_q, keep, rc in ((1, -1, 128, 1, L.OFC_EINVAL), (1, 65281, 128, 1, L.OFC_EINVAL), (1, 2048, -1, 1, L.OFC_EINVAL),
                                         (1, 2048, 1025, 1, L.OFC_EINVAL), (1, 2048, 128, 0, L.OFC_EINVAL),
                                         (1, 2048, 128, 16, L.OFC_EINVAL)):
        assert lib.ofc_stream_set_photo(st._h, on, tau_q, kappa_q, keep) == rc
    assert lib.ofc_stream_set_photo(None, 1, 2048, 128, 1) == L.OFC_EINVAL and lib.ofc_stream_read_photo(None, None, 0) == L.OFC_EINVAL
    assert lib.ofc_stream_read_photo(st._h, L.ptr(host), ST) == L.OFC_EINVAL      # the refusals set nothing
    st.set_photometric()
    st.push(clip.frames[0])
    with pytest.raises(ValueError, match="holds frames"):                         # in mid-clip: refused, nothing changes
        st.set_photometric(tau=1.0)
    with pytest.raises(ValueError, match="holds frames"):
        st.set_photometric(on=False)
    with pytest.raises(ValueError, match="holds frames"):
        st.photometric_stats()
    assert st.photo_args == (PC.TAU_Q, PC.KAPPA_Q, 1)
    for f in clip.frames[1:]:
        st.push(f)
    st.finish()
    assert lib.ofc_stream_read_photo(st._h, L.ptr(host), ST - 2) == L.OFC_EINVAL and (host == -7).all()      # too small: nothing written
    assert "delivered 8" in lib.ofc_last_error().decode()
    L.check(lib.ofc_stream_read_photo(st._h, L.ptr(host), ST))
    assert np.array_equal(host[:ST - 1], clip.ref[1]) and (host[ST - 1] == -7).all()                     # the run went on unharmed
    with pytest.raises(ValueError):
        st.set_photometric(keep=(4,))
    with pytest.raises(ValueError, match="kappa"):
        st.set_photometric(kappa=5.0)
    assert np.array_equal(st.photometric_stats(), clip.ref[1])
    st.close()


def test_motion_grids_photometric_on_both_routes(clip, tmp_path):
    from opticalflowclustering_amd import motionGrids as G
    names = ("clip.npy", "model.npy", "res.csv", "stream.csv", "fit.csv", "res.npy", "stream.npy", "fit.npy", "b_res.csv", "b_stream.csv")
    clip_path, model, res_csv, stream_csv, fit_csv, res_npy, stream_npy, fit_npy, b_res, b_stream = (str(tmp_path / n) for n in names)
    np.save(clip_path, clip.frames)
    np.save(model, np.array([[0.0, 0.0], [3.0, 0.0], [0.0, -2.0]]))
    base = ["--path", clip_path, "-c", "3", "--rows", "2", "--cols", "3", "--photometric", "--photo-tau", "2", "--photo-kappa", "0.25",
            "--blob-thr", "1.0", "--blob-min-area", "4"]
    G.main(base + ["-f", res_csv, "--init", model, "--photo-counts", res_npy, "--blobs", b_res])
    G.main(base + ["-f", stream_csv, "--model", model, "--stream", "--batch-pairs", "3", "--photo-counts", stream_npy, "--blobs", b_stream])
    G.main(base + ["-f", fit_csv, "--fit-stream", "--hist-bins", "256", "--hist-range", "8", "--photo-counts", fit_npy])
    for path in (res_npy, stream_npy, fit_npy):
        got = np.load(path)
        assert got.dtype == np.int64 and np.array_equal(got, clip.strict[1]), path
    for path in (res_csv, stream_csv, fit_csv):
        assert len(open(path).read().splitlines()) == ST
    # the stream's rows are those of the masked key maps, keyed by the model's labels
    B = _B()
    cen = np.load(model)
    want = B.cluster_blobs(clip.fields, cen, thr=1.0, min_area=4, max_blobs=G.MAX_BLOBS)
    masked = np.where(clip.strict[0] == PC.OK, want.keys, 255).astype(np.uint8)
    rows = B.connected_components(masked, min_area=4, max_blobs=G.MAX_BLOBS, flow=clip.fields).rows()
    assert open(b_stream).read().splitlines()[1:] == [",".join(str(v) for v in r) for r in rows] and len(rows) >= ST - 1
    assert len(open(b_res).read().splitlines()) > 1
