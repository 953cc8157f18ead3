"""The repair on the device (flow_repair.hip): the field, the filled map, the counts and the updated states on every case and
parameter set of tests/repair_cases.py, on host buffers and on device buffers at both alignments, out of place, in place and
with the state map updated in place, and the way up through repair.py, ClipPipeline, FlowStream and the motionGrids command
line.

Nothing here carries a tolerance: the counts, the maps and the states are integers, and every value of the field is one of the
input's numbers, compared with == (which sign a zero carries is not promised), while sources and pixels never filled are
compared by their bytes.  test_repair_host.py proves the model against a per-pixel restatement and the table against its
claims."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import photometric_cases as PC
from tests import repair_cases as RC

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _K():
    from opticalflowclustering_amd import repair
    return repair


def _B():
    from opticalflowclustering_amd import blobs
    return blobs


def _fill(buf, byte=0x55):
    L = _L()
    L.check(L.load().ofc_memset(0, C.c_void_p(buf.ptr), byte, buf.nbytes))


def same(case, p, got, with_state=True):
    """out by == where it was written and by bytes where it must be the input's own; filled, counts, state_out exactly"""
    out, filled, counts, st_out = got
    wo, wf, wc, ws = case.reference(p)
    copied = (wf == RC.UNFILLED) | ((wf == 0) & (not p.smooth))
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32)[copied], case.flow.view(np.uint32)[copied])
    with np.errstate(invalid="ignore"):
        assert (out[~copied] == wo[~copied]).all(), np.argwhere(~copied & ~(out == wo).all(-1))[:5]
    if filled is not None:
        assert filled.dtype == np.uint8 and np.array_equal(filled, wf), np.argwhere(filled != wf)[:5]
    assert counts.dtype == np.int64 and np.array_equal(counts, wc), (counts, wc)
    if with_state and case.state is not None:
        assert st_out.dtype == np.uint8 and np.array_equal(st_out, ws), np.argwhere(st_out != ws)[:5]


def repair_host(flow, state, p, filled=True, state_out=True):
    """ofc_repair: host buffers, whole chain"""
    L = _L()
    n, H, W = flow.shape[:3]
    out, counts = np.full((n, H, W, 2), np.float32(-7)), np.full((n, 3), -1, np.int64)
    fl = np.full((n, H, W), 0x55, np.uint8) if filled else None
    so = np.full((n, H, W), 0x55, np.uint8) if state is not None and state_out else None
    L.check(L.load().ofc_repair(0, L.ptr(flow), L.ptr(state), W, H, n, *p.args(), L.ptr(out), L.ptr(fl), L.ptr(so), L.ptr(counts)))
    return out, fl, counts, so


@pytest.mark.parametrize("case", RC.CASES, ids=repr)
def test_host_buffers_equal_the_model(case):
    for p in case.params:
        same(case, p, repair_host(case.flow, case.state, p))
    p = case.params[0]
    same(case, p, repair_host(case.flow, case.state, p, filled=False), with_state=True)      # the optional outputs left out
    same(case, p, repair_host(case.flow, case.state, p, filled=False, state_out=False), with_state=False)
    n = case.shape[0]
    if n > 1:                                                                     # a batch is its pairs, one at a time
        for t in range(n):
            one = repair_host(case.flow[t:t + 1], None if case.state is None else case.state[t:t + 1], p)
            want = case.reference(p)
            with np.errstate(invalid="ignore"):
                eq = (one[0][0] == want[0][t]) | (one[0][0].view(np.uint32) == case.flow[t].view(np.uint32))
            assert eq.all() and np.array_equal(one[1][0], want[1][t]) and np.array_equal(one[2][0], want[2][t])


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", RC.CASES, ids=repr)
def test_device_buffers_equal_the_model_out_of_place_and_in_place(case, shift):
    """ofc_repair_dev; shift = 1 puts the field and the output 8 bytes and the three maps 1 byte past their buffers' starts,
    where the kernels can take neither two vectors nor four map bytes at a time.  Out of place the inputs are left alone; in
    place the field and the state map are their own outputs.  Nothing is written in front of or past an output."""
    L = _L()
    lib = L.load()
    n, H, W = case.shape
    N = n * H * W
    st = case.state
    fd, od = L.DeviceBuffer(N * 8 + 32), L.DeviceBuffer(N * 8 + 32)
    sd, ld, ud, cd = L.DeviceBuffer(N + 16), L.DeviceBuffer(N + 16), L.DeviceBuffer(N + 16), L.DeviceBuffer(n * 24 + 16)
    fp, op, sp, lp, up = fd.ptr + 8 * shift, od.ptr + 8 * shift, sd.ptr + shift, ld.ptr + shift, ud.ptr + shift

    def field(buf):
        raw = buf.download((N * 8 + 32,), np.uint8)
        assert (raw[:8 * shift] == 0x55).all() and (raw[8 * shift + N * 8:] == 0x55).all()
        return raw[8 * shift:8 * shift + N * 8].copy().view(np.float32).reshape(n, H, W, 2)

    def bytemap(buf):
        raw = buf.download((N + 16,), np.uint8)
        assert (raw[:shift] == 0x55).all() and (raw[shift + N:] == 0x55).all()
        return raw[shift:shift + N].reshape(n, H, W).copy()

    def counts():
        assert (cd.download((16,), np.uint8, offset=n * 24) == 0x55).all()
        return cd.download((n, 3), np.int64)

    try:
        for p in case.params:
            for b in (fd, od, sd, ld, ud, cd):
                _fill(b)
            fd.upload(case.flow, offset=8 * shift)
            if st is not None:
                sd.upload(st, offset=shift)
            vp = C.c_void_p
            # out of place, every output its own buffer
            L.check(lib.ofc_repair_dev(0, vp(fp), vp(sp) if st is not None else None, W, H, n, *p.args(), vp(op), vp(lp),
                                       vp(up) if st is not None else None, vp(cd.ptr)))
            same(case, p, (field(od), bytemap(ld), counts(), bytemap(ud) if st is not None else None))
            assert np.array_equal(field(fd).view(np.uint32), case.flow.view(np.uint32))
            if st is not None:
                assert np.array_equal(bytemap(sd), st)
            else:
                assert (bytemap(ud) == 0x55).all()
            # in place: the field onto itself, the states onto themselves, no filled map
            _fill(cd)
            L.check(lib.ofc_repair_dev(0, vp(fp), vp(sp) if st is not None else None, W, H, n, *p.args(), vp(fp), None,
                                       vp(sp) if st is not None else None, vp(cd.ptr)))
            same(case, p, (field(fd), None, counts(), bytemap(sd) if st is not None else None))
    finally:
        for b in (fd, od, sd, ld, ud, cd):
            b.free()


def test_a_batch_of_more_than_one_chunk_equals_its_pairs_alone():
    """two pairs of more than half a chunk's pixels each go through the chunk loop one after the other"""
    L, K = _L(), _K()
    W, H, n = 4096, 1030, 2
    assert 2 * W * H > 1 << 23 >= W * H
    rng = np.random.default_rng(5)
    flow = rng.integers(-8, 9, (n, H, W, 2)).astype(np.float32)
    state = (rng.integers(0, 16, (n, H, W)) == 0).astype(np.uint8)
    state[1, 100:130, 4000:4096] = PC.LEAVES
    both = K.fill(flow, state, rounds=2, smooth=True)
    assert (both.counts.sum(1) == W * H).all() and both.counts[:, 1].min() > 0 and both.counts[1, 2] > 0
    for t in range(n):
        one = K.fill(flow[t], state[t], rounds=2, smooth=True)
        assert np.array_equal(one.flow[0], both.flow[t]) and np.array_equal(one.filled[0], both.filled[t])
        assert np.array_equal(one.counts[0], both.counts[t]) and np.array_equal(one.state[0], both.state[t])


def test_median_equals_a_numpy_median_filter_with_a_clipped_window():
    K = _K()
    rng = np.random.default_rng(11)
    H, W = 21, RC.tile(1)[0] + 6
    f = np.round(rng.standard_normal((2, H, W, 2)) * 4).astype(np.float32) / 2
    for r in (1, 2):
        want = np.empty_like(f)
        for y in range(H):
            for x in range(W):
                win = f[:, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].reshape(2, -1, 2)
                want[:, y, x] = np.sort(win, axis=1)[:, (win.shape[1] - 1) // 2]
        got = K.median(f, radius=r)
        assert got.shape == f.shape and got.dtype == np.float32 and (got == want).all()
        assert (K.median(f[0], radius=r) == want[0]).all()


def test_fill_takes_a_single_field_and_says_what_it_did():
    K = _K()
    c = RC.BY_NAME["open-%dx%d-n1-r1" % (RC.tile(1)[0] + 5, RC.tile(1)[1] + 2)]
    p = c.params[0]
    got = K.fill(c.flow[0], c.state[0], radius=1, rounds=2)
    same(c, p, (got.flow, got.filled, got.counts, got.state))
    assert len(got) == 1 and got.counts[0, K.UNFILLED_COUNT] > 0 and np.allclose(got.share().sum(1), 1)
    assert K.fill(c.flow, None, rounds=1).state is None


def test_the_device_calls_refuse_what_the_check_refuses_and_touch_nothing():
    L = _L()
    lib = L.load()
    c = RC.BY_NAME["mincount-12x9-n1-r1"]
    n, H, W = c.shape
    N = n * H * W
    fd, sd = L.DeviceBuffer(N * 8 + 16).upload(c.flow), L.DeviceBuffer(N + 16).upload(c.state)
    od, ld, ud, cd = L.DeviceBuffer(N * 8 + 16), L.DeviceBuffer(N + 16), L.DeviceBuffer(N + 16), L.DeviceBuffer(n * 24 + 8)
    try:
        def call(flow=fd.ptr, state=sd.ptr, W=W, H=H, npair=n, keep=1, radius=1, rounds=2, min_count=1, smooth=0, out=od.ptr, filled=ld.ptr,
                 state_out=ud.ptr, counts=cd.ptr):
            vp = lambda p: C.c_void_p(p) if p else None      # noqa: E731
            return lib.ofc_repair_dev(0, vp(flow), vp(state), W, H, npair, keep, radius, rounds, min_count, smooth, vp(out), vp(filled),
                                      vp(state_out), vp(counts))

        assert call() == L.OFC_OK
        for b in (od, ld, ud, cd):
            _fill(b)
        assert call(flow=None) == L.OFC_EINVAL and call(out=None) == L.OFC_EINVAL and call(counts=None) == L.OFC_EINVAL
        assert call(state=None) == L.OFC_EINVAL and "state_out" in lib.ofc_last_error().decode()          # state_out without state
        assert call(flow=fd.ptr + 4) == L.OFC_EINVAL and call(out=od.ptr + 4) == L.OFC_EINVAL and call(counts=cd.ptr + 4) == L.OFC_EINVAL
        assert call(out=fd.ptr + 8) == L.OFC_EINVAL and "overlaps" in lib.ofc_last_error().decode()
        assert call(W=0) == L.OFC_EINVAL and call(H=0) == L.OFC_EINVAL and call(npair=0) == L.OFC_EINVAL and call(npair=65536) == L.OFC_EINVAL
        assert call(W=16385) == L.OFC_EUNSUPPORTED and call(H=16385) == L.OFC_EUNSUPPORTED
        assert call(keep=0) == L.OFC_EINVAL and call(keep=16) == L.OFC_EINVAL and call(radius=0) == L.OFC_EINVAL and call(radius=3) == L.OFC_EINVAL
        assert call(rounds=-1) == L.OFC_EINVAL and call(rounds=255) == L.OFC_EINVAL and call(rounds=0) == L.OFC_EINVAL
        assert call(min_count=0) == L.OFC_EINVAL and call(min_count=10) == L.OFC_EINVAL and call(radius=2, min_count=26) == L.OFC_EINVAL
        assert call(smooth=2) == L.OFC_EINVAL and call(smooth=-1) == L.OFC_EINVAL
        for b in (od, ld, ud, cd):
            assert (b.download((b.nbytes,), np.uint8) == 0x55).all()                # not even the clear of the counts
        assert np.array_equal(fd.download(c.flow.shape, np.float32).view(np.uint32), c.flow.view(np.uint32))
        host = np.full(8, 0x55, np.uint8)
        assert lib.ofc_repair(0, None, None, W, H, n, 1, 1, 2, 1, 0, L.ptr(host), None, None, L.ptr(host)) == L.OFC_EINVAL
        assert lib.ofc_repair(0, L.ptr(c.flow), None, W, H, n, 1, 1, 2, 1, 0, L.ptr(host), None, L.ptr(host), L.ptr(host)) == L.OFC_EINVAL
        assert lib.ofc_repair(0, L.ptr(c.flow), None, W, H, n, 1, 3, 2, 1, 0, L.ptr(host), None, None, L.ptr(host)) == L.OFC_EINVAL
        assert (host == 0x55).all()
        ms = C.c_float(-1.0)
        assert lib.ofc_bench_repair(0, C.c_void_p(fd.ptr), C.c_void_p(sd.ptr), W, H, n, 3, 1, C.byref(ms)) == L.OFC_EINVAL
        assert lib.ofc_bench_repair(0, C.c_void_p(fd.ptr), None, W, H, 0, 0, 1, C.byref(ms)) == L.OFC_EINVAL
        assert ms.value == -1.0
        for what in (0, 1, 2):
            for state in (C.c_void_p(sd.ptr), None):
                L.check(lib.ofc_bench_repair(0, C.c_void_p(fd.ptr), state, W, H, n, what, 2, C.byref(ms)))
                assert ms.value > 0
        assert np.array_equal(fd.download(c.flow.shape, np.float32).view(np.uint32), c.flow.view(np.uint32))   # the hook writes its own
    finally:
        for b in (fd, sd, od, ld, ud, cd):
            b.free()


# ---- ClipPipeline ----
PW, PH = 96, 64
STRICT = dict(tau=2.0, kappa=0.25)
SPEC = dict(radius=1, rounds=3, min_count=2)


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


def test_pipeline_repair_after_either_check_equals_fill_on_the_downloaded_field():
    from opticalflowclustering_amd.pipeline import ClipPipeline
    B, K = _B(), _K()
    T = 5
    frames = gray_clip(T)
    n = T - 1
    pipe = ClipPipeline(PW, PH, T, batch_pairs=2)
    try:
        pipe.upload_frames(frames)
        pipe.run_flow()
        with pytest.raises(ValueError, match="state map of a check"):
            pipe.repair()
        with pytest.raises(ValueError, match="no filled map"):
            pipe.filled_host()
        fwd = pipe.flows_host()
        for which, spec in (("photometric", dict(SPEC)), ("consistency", dict(SPEC, smooth=True, keep=(0, 2)))):
            pipe.run_flow()                                                        # the field as the engine left it, no state map
            assert np.array_equal(pipe.flows_host().view(np.uint32), fwd.view(np.uint32)) and pipe.state is None
            if which == "consistency":
                pipe.run_backward_flow()
                state = pipe.consistency().state
            else:
                state = pipe.photometric(**STRICT).state
            want = K.fill(fwd, state, **spec)
            assert want.counts[:, 1].min() > 0                                     # the check flagged pixels and the fill closed some
            counts = pipe.repair(**spec)
            assert counts.dtype == np.int64 and np.array_equal(counts, want.counts)
            got = pipe.flows_host()
            assert np.array_equal(got.view(np.uint32), want.flow.view(np.uint32))   # the same code on the same bits
            assert np.array_equal(pipe.filled_host(), want.filled)
            assert np.array_equal(pipe.state.download((n, PH, PW), np.uint8), want.state)
            # blobs(consistent=True) afterwards: the filled pixels are back in the key map, those never filled are not
            after = pipe.blobs(by="moving", thr=0.25, consistent=True)
            keys = np.where(want.state == PC.OK, moving_keys(got, 0.25), 255).astype(np.uint8)
            assert np.array_equal(after.keys, keys)
            was_filled = (want.filled > 0) & (want.filled < K.UNFILLED)
            assert (after.keys[was_filled] == 0).any() and (after.keys[want.filled == K.UNFILLED] == 255).all()
            same_blobs(after, B.connected_components(keys, flow=got))
        with pytest.raises(ValueError, match="rounds"):
            pipe.repair(rounds=255)
        pipe.compensate_camera("translation")
        with pytest.raises(ValueError, match="compensate_camera"):
            pipe.repair()
        pipe.run_flow()
        assert pipe.state is None and pipe.filled is None
        stateless = pipe.repair(need_state=False)                                  # nothing but unusable vectors to fill
        assert np.array_equal(stateless, K.fill(fwd).counts) and pipe.state is None
    finally:
        pipe.close()


# ---- FlowStream ----
ST, THR = 9, 1.0
BLOB = dict(thr=THR, connectivity=8, min_area=4, max_blobs=256)


@pytest.fixture(scope="module")
def clip():
    """nine frames, their eight pairwise fields (the engine's, one pair at a time, as test_gpu_photometric.py obtains the fields
    a stream saw), the strict photometric reference on them and the model's repair of that: once, read-only"""
    from opticalflowclustering_amd.flow import FlowEngine
    from opticalflowclustering_amd import photometric
    frames = gray_clip(ST)
    eng = FlowEngine(PW, PH, max_batch=1)
    fields = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(ST - 1)])
    eng.close()
    strict = PC.reference(frames, fields, *photometric.quantise(**STRICT))
    repaired = RC.model(fields, strict[0], 1, SPEC["radius"], SPEC["rounds"], SPEC["min_count"], False)
    for a in (frames, fields) + strict + repaired:
        a.setflags(write=False)
    return SimpleNamespace(frames=frames, fields=fields, strict=strict, repaired=repaired)


def _stream(batch_pairs, **kw):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(PW, PH, batch_pairs=batch_pairs, rows=2, cols=3, **kw)


def _run(st, frames):
    for f in frames:
        st.push(f)
    return st.finish()


@pytest.mark.parametrize("batch", (3, 8))
def test_stream_repair_equals_the_resident_route_and_can_be_removed(clip, batch):
    from opticalflowclustering_amd.pipeline import ClipPipeline
    from opticalflowclustering_amd.stream import grid_cell_mean_flow
    B = _B()
    out, filled, counts, state = clip.repaired
    assert counts[:, 1].min() > 0 and counts[:, 2].sum() > 0                      # some filled in every pair, some left over
    # the resident route on the same frames and parameters
    pipe = ClipPipeline(PW, PH, ST, batch_pairs=batch)
    try:
        pipe.upload_frames(clip.frames)
        pipe.run_flow()
        assert np.array_equal(pipe.flows_host().view(np.uint32), clip.fields.view(np.uint32))
        pipe.photometric(**STRICT)
        res_counts = pipe.repair(**SPEC)
        res_field = pipe.flows_host()
        res_blobs = pipe.blobs(by="moving", labels=False, consistent=True, **BLOB)
    finally:
        pipe.close()
    assert np.array_equal(res_counts, counts) and (res_field == out).all()
    st = _stream(batch, photometric=dict(STRICT), repair=dict(SPEC), blobs=BLOB)
    assert st.repair_args == (1, SPEC["radius"], SPEC["rounds"], SPEC["min_count"], 0)
    cells = _run(st, clip.frames)
    got = st.repair_stats()
    assert got.dtype == np.int64 and got.shape == (ST - 1, 3) and np.array_equal(got, res_counts)
    assert np.array_equal(st.repair_stats(), got)                                 # still there until frames arrive
    same_blobs(st.blobs(), res_blobs, labels=False)
    assert np.array_equal(st.photometric_stats(), clip.strict[1])                 # the check saw the field before the repair
    # everything downstream sees the repaired field: the cell means are those of the resident route's field
    want_cells = np.stack([grid_cell_mean_flow(res_field[t], 2, 3) for t in range(ST - 1)])
    assert np.array_equal(np.asarray(cells).reshape(want_cells.shape).view(np.uint32), want_cells.view(np.uint32))
    # the blobs are those of the repaired field under the updated states
    keys = np.where(state == PC.OK, moving_keys(res_field, THR), 255).astype(np.uint8)
    same_blobs(st.blobs(), B.connected_components(keys, min_area=4, max_blobs=256, flow=res_field), labels=False)
    _run(st, clip.frames[:5])                                                     # a second, shorter clip on the same stream
    assert np.array_equal(st.repair_stats(), counts[:4])
    # on = 0: back to what a stream with the check alone delivers
    st.set_repair(on=False)
    assert st.repair_args is None
    plain_cells = _run(st, clip.frames)
    masked = np.where(clip.strict[0] == PC.OK, moving_keys(clip.fields, THR), 255).astype(np.uint8)
    same_blobs(st.blobs(), B.connected_components(masked, min_area=4, max_blobs=256, flow=clip.fields), labels=False)
    with pytest.raises(ValueError, match="no repair"):
        st.repair_stats()
    st.close()
    never = _stream(batch, photometric=dict(STRICT), blobs=BLOB)
    assert np.array_equal(_run(never, clip.frames).view(np.uint32), plain_cells.view(np.uint32))
    never.close()
    # without a check the state is NULL: only unusable vectors are targets, and the engine leaves none
    alone = _stream(batch, repair=True)
    _run(alone, clip.frames)
    assert np.array_equal(alone.repair_stats(), RC.model(clip.fields, None)[2])
    alone.close()


def test_stream_photometric_stats_and_repair_counts_grow_past_their_first_allocation(clip):
    """frames cycling through 4 images, 261 pushes at batch_pairs = 8: the 33rd batch takes both tables past their 256 pairs.
    Pair t is (image t % 4, image (t + 1) % 4), so its rows equal those of pair t % 4: the reference's, from the pairwise
    fields of the four cyclic pairs, not a second stream's"""
    from opticalflowclustering_amd.flow import FlowEngine
    from opticalflowclustering_amd import photometric
    images = clip.frames[:4]
    eng = FlowEngine(PW, PH, max_batch=1)
    fields = np.stack([eng.calc(images[t], images[(t + 1) % 4]) for t in range(4)])
    eng.close()
    state, want_stats, _ = PC.reference(images[[0, 1, 2, 3, 0]], fields, *photometric.quantise(**STRICT))
    want_counts = RC.model(fields, state)[2]                                      # repair=True: the model's defaults
    for want in (want_stats, want_counts):
        assert len({r.tobytes() for r in want}) == 4                              # the four pairs differ: a misplaced row shows
    st = _stream(8, photometric=dict(STRICT), repair=True)
    for t in range(261):
        st.push(images[t % 4])
    assert len(st.finish()) == 260
    stats, counts = st.photometric_stats(), st.repair_stats()
    st.close()
    assert stats.shape == (260, 5) and counts.shape == (260, 3)
    for t in range(260):
        assert np.array_equal(stats[t], want_stats[t % 4]), t
        assert np.array_equal(counts[t], want_counts[t % 4]), t


def test_stream_set_repair_and_read_repair_refusals(clip):
    L = _L()
    lib = L.load()
    st = _stream(3)
    host = np.full((ST, 3), -7, np.int64)
    assert lib.ofc_stream_read_repair(st._h, L.ptr(host), ST) == L.OFC_EINVAL     # without the repair
    assert "no repair" in lib.ofc_last_error().decode()
    for args in ((0, 1, 8, 1, 0), (16, 1, 8, 1, 0), (1, 0, 8, 1, 0), (1, 3, 8, 1, 0), (1, 1, -1, 1, 0), (1, 1, 255, 1, 0), (1, 1, 0, 1, 0),
                 (1, 1, 8, 0, 0), (1, 1, 8, 10, 0), (1, 2, 8, 26, 0), (1, 1, 8, 1, 2)):
        assert lib.ofc_stream_set_repair(st._h, 1, *args) == L.OFC_EINVAL, args
    assert lib.ofc_stream_set_repair(None, 1, 1, 1, 8, 1, 0) == L.OFC_EINVAL and lib.ofc_stream_read_repair(None, None, 0) == L.OFC_EINVAL
    assert lib.ofc_stream_read_repair(st._h, L.ptr(host), ST) == L.OFC_EINVAL     # the refusals set nothing
    st.set_repair(**SPEC)
    st.push(clip.frames[0])
    with pytest.raises(ValueError, match="holds frames"):                         # in mid-clip: refused, nothing changes
        st.set_repair(radius=2)
    with pytest.raises(ValueError, match="holds frames"):
        st.set_repair(on=False)
    with pytest.raises(ValueError, match="holds frames"):
        st.repair_stats()
    for f in clip.frames[1:]:
        st.push(f)
    st.finish()
    assert lib.ofc_stream_read_repair(st._h, L.ptr(host), ST - 2) == L.OFC_EINVAL and (host == -7).all()     # too small: nothing written
    assert "delivered 8" in lib.ofc_last_error().decode()
    L.check(lib.ofc_stream_read_repair(st._h, L.ptr(host), ST))
    assert (host[:ST - 1].sum(1) == PW * PH).all() and (host[ST - 1] == -7).all()
    with pytest.raises(ValueError):
        st.set_repair(keep=(4,))
    st.close()


def test_motion_grids_repair_writes_its_counts_on_every_route(clip, tmp_path):
    from opticalflowclustering_amd import motionGrids as G
    names = ("clip.npy", "model.npy", "res.csv", "stream.csv", "fit.csv", "res.npy", "stream.npy", "fit.npy", "alone.csv", "alone.npy")
    clip_path, model, res_csv, stream_csv, fit_csv, res_npy, stream_npy, fit_npy, alone_csv, alone_npy = (str(tmp_path / n) for n in names)
    np.save(clip_path, clip.frames)
    np.save(model, np.array([[0.0, 0.0], [3.0, 0.0], [0.0, -2.0]]))
    base = ["--path", clip_path, "-c", "3", "--rows", "2", "--cols", "3", "--photometric", "--photo-tau", "2", "--photo-kappa", "0.25",
            "--repair", "1:3"]
    G.main(base + ["-f", res_csv, "--init", model, "--repair-counts", res_npy])
    G.main(base + ["-f", stream_csv, "--model", model, "--stream", "--batch-pairs", "3", "--repair-counts", stream_npy])
    G.main(base + ["-f", fit_csv, "--fit-stream", "--hist-bins", "256", "--hist-range", "8", "--repair-counts", fit_npy])
    want = RC.model(clip.fields, clip.strict[0], 1, 1, 3, 1, False)[2]
    for path in (res_npy, stream_npy, fit_npy):
        got = np.load(path)
        assert got.dtype == np.int64 and np.array_equal(got, want), path
    for path in (res_csv, stream_csv, fit_csv):
        assert len(open(path).read().splitlines()) == ST
    # without a check: only unusable vectors, of which the engine leaves none
    G.main(["--path", clip_path, "-c", "3", "--rows", "2", "--cols", "3", "--repair", "2", "--repair-smooth", "-f", alone_csv, "--init", model,
            "--repair-counts", alone_npy])
    assert np.array_equal(np.load(alone_npy), RC.model(clip.fields, None, 1, 2, 8, 1, True)[2])
