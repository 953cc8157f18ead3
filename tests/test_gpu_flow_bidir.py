"""The bidirectional flow batch on the GPU.  FlowEngine.calc_frames_dev_bidir against a forward-only engine on the palindrome
clip, bit for bit (tests/flow_bidir_cases.py says why that is a fair demand, test_flow_bidir_host.py that the case table
reaches what it names); the same engine called forward-only, bidirectionally and forward-only again; what the entry point
refuses; FlowStream(consistency=...) against the staged route; ClipPipeline.run_flow_bidirectional."""
import ctypes as C

import numpy as np
import pytest

import flow_bidir_cases as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _forward(frames, kw, max_batch):
    """a fresh forward-only engine over the whole clip in one call -> (n-1, H, W, 2)"""
    from opticalflowclustering_amd.flow import FlowEngine
    L = _L()
    n, H, W = frames.shape
    eng = FlowEngine(W, H, params=L.FbParams(**kw), max_batch=max_batch)
    fd = L.DeviceBuffer(frames.nbytes).upload(frames)
    od = L.DeviceBuffer((n - 1) * H * W * 8)
    eng.calc_frames_dev(fd.ptr, n, od.ptr)
    out = od.download((n - 1, H, W, 2), np.float32)
    eng.close()
    return out


def _bidir(frames, kw, split=False, eng=None):
    """calc_frames_dev_bidir over the whole clip -> (fwd, bwd); max_batch is exactly the clip's pair count.  split: the two
    fields in allocations of their own instead of one block"""
    from opticalflowclustering_amd.flow import FlowEngine
    L = _L()
    n, H, W = frames.shape
    own = eng is None
    if own:
        eng = FlowEngine(W, H, params=L.FbParams(**kw), max_batch=n - 1)
    fd = L.DeviceBuffer(frames.nbytes).upload(frames)
    half = (n - 1) * H * W * 8
    if split:
        bd, od = L.DeviceBuffer(half), L.DeviceBuffer(half)
        fwd_ptr, bwd_ptr = od.ptr, bd.ptr
    else:
        od = L.DeviceBuffer(2 * half)
        fwd_ptr, bwd_ptr = od.ptr, od.ptr + half
    eng.calc_frames_dev_bidir(fd.ptr, n, fwd_ptr, bwd_ptr)
    fwd = od.download((n - 1, H, W, 2), np.float32)
    bwd = bd.download((n - 1, H, W, 2), np.float32) if split else od.download((n - 1, H, W, 2), np.float32, offset=half)
    if own:
        eng.close()
    return fwd, bwd


def _assert_is_the_palindrome_run(fwd, bwd, ref):
    n = fwd.shape[0]
    assert ref.shape[0] == 2 * n
    f_idx, b_idx = B.palindrome_pairs(n)
    assert np.isfinite(ref).all()
    for t in range(n):
        assert np.array_equal(fwd[t], ref[f_idx[t]]), ("fwd", t, np.abs(fwd[t] - ref[f_idx[t]]).max())
        assert np.array_equal(bwd[t], ref[b_idx[t]]), ("bwd", t, np.abs(bwd[t] - ref[b_idx[t]]).max())


# ---- a. the engine against the existing engine, bit for bit ----
@pytest.mark.parametrize("name,W,H,kw,n", B.CASES, ids=[c[0] for c in B.CASES])
def test_both_directions_are_the_palindrome_runs_pairs(name, W, H, kw, n):
    frames = B.clip(W, H, n + 1)
    ref = _forward(B.palindrome(frames), kw, 2 * n)
    fwd, bwd = _bidir(frames, kw)
    _assert_is_the_palindrome_run(fwd, bwd, ref)
    fwd2, bwd2 = _bidir(frames, kw, split=True)             # level 0 through two base pointers that are not neighbours
    assert np.array_equal(fwd2, fwd) and np.array_equal(bwd2, bwd)


@pytest.mark.parametrize("var,value", B.FRONT_END_ENV, ids=[f"{k}={v}" for k, v in B.FRONT_END_ENV])
def test_front_end_paths_in_a_fresh_engine(monkeypatch, var, value):
    from opticalflowclustering_amd.flow import FlowEngine
    L = _L()
    name, W, H, kw, n = B.case(B.FRONT_END_CASE)
    frames = B.clip(W, H, n + 1)
    ref = _forward(B.palindrome(frames), kw, 2 * n)           # the default front end
    monkeypatch.setenv(var, value)
    eng = FlowEngine(W, H, params=L.FbParams(**kw), max_batch=n)
    if var == "OFC_FLOW_FRONT_OVERLAP":
        assert not eng.front_overlap()
    if var == "OFC_PYRAMID_FUSED":
        assert eng.front_overlap() and not eng.pyramid_fused()
    fwd, bwd = _bidir(frames, kw, eng=eng)
    eng.close()
    if var == "OFC_FLOW_STAGED":      # the staged kernels are another arithmetic: against their own forward-only run
        ref = _forward(B.palindrome(frames), kw, 2 * n)
    _assert_is_the_palindrome_run(fwd, bwd, ref)


def test_against_the_oracle_on_the_clip_and_on_the_reversed_clip():
    """the project's bars (1e-4 relative L2, 1e-3 px) on one case: the palindrome demand above cannot see a wrong pair map
    that both engines share"""
    import flow_domain_cases as D
    name, W, H, kw, n = B.case("ws15-odd-size-UPS1-251x67-2pairs")
    frames = B.clip(W, H, n + 1)
    fwd, bwd = _bidir(frames, kw)
    po = D.oracle_params(kw)
    for t in range(n):
        for got, want in ((fwd[t], O.farneback(frames[t], frames[t + 1], po)), (bwd[t], O.farneback(frames[t + 1], frames[t], po))):
            r, m = D.rel(got, want), np.abs(got - want).max()
            print(f"pair {t}: rel {r:.3e} max|d| {m:.3e}")
            assert r <= 1e-4 and m <= 1e-3, (t, r, m)
    assert np.abs(fwd + bwd).mean() < 0.1 < np.abs(fwd).mean()          # a translation: the two nearly cancel


@pytest.mark.parametrize("name", ["ws15-two-column-tiles-272x80-2pairs", "ws17-staged-box8-272x80-2pairs"])
@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph-replay"])
def test_forward_only_calls_around_a_bidirectional_one(monkeypatch, name, graph):
    """forward-only, bidirectional, forward-only on ONE engine: the grown scratch and the R slices leave the forward-only
    results as they were, with graph replay on as well (the bidirectional call makes plain launches and drops the graphs
    that hold the old scratch)"""
    from opticalflowclustering_amd.flow import FlowEngine
    L = _L()
    _, W, H, kw, n = B.case(name)
    frames = B.clip(W, H, n + 1)
    want = _forward(frames, kw, n)
    if graph:
        monkeypatch.setenv("OFC_FLOW_GRAPH", "1")
    eng = FlowEngine(W, H, params=L.FbParams(**kw), max_batch=n)
    fd = L.DeviceBuffer(frames.nbytes).upload(frames)
    od = L.DeviceBuffer(n * H * W * 8)

    def forward():
        od.zero()
        eng.calc_frames_dev(fd.ptr, n + 1, od.ptr)
        return od.download((n, H, W, 2), np.float32)

    for _ in range(3 if graph else 1):          # the third call with one argument set replays a captured graph
        assert np.array_equal(forward(), want)
    fwd, bwd = _bidir(frames, kw, eng=eng)
    assert np.array_equal(fwd, want)             # (the strips are sized for 2n pairs here: the same bits on these frames)
    for _ in range(3 if graph else 1):
        assert np.array_equal(forward(), want)
    fwd2, bwd2 = _bidir(frames[:2], kw, eng=eng)            # fewer pairs than max_batch, after the scratch has grown
    ref = _forward(B.palindrome(frames[:2]), kw, 2)
    _assert_is_the_palindrome_run(fwd2, bwd2, ref)
    eng.close()


def test_refusals_of_the_entry_point():
    from opticalflowclustering_amd.flow import FlowEngine
    L = _L()
    lib = L.load()
    W, H, n = 96, 64, 2
    P = W * H
    eng = FlowEngine(W, H, max_batch=n)
    fd = L.DeviceBuffer(P * (n + 2))
    fd.zero()
    od = L.DeviceBuffer(2 * n * P * 8)
    od.upload(np.full(2 * n * P * 2, -7.0, np.float32))
    half = n * P * 8
    call = lib.ofc_flow_calc_frames_dev_bidir
    vp = C.c_void_p
    ok = (eng._h, vp(fd.ptr), n + 1, vp(od.ptr), vp(od.ptr + half))
    for bad in ((None,) + ok[1:], (ok[0], None) + ok[2:], ok[:3] + (None, ok[4]), ok[:4] + (None,),
                ok[:2] + (1,) + ok[3:], ok[:2] + (0,) + ok[3:], ok[:2] + (n + 2,) + ok[3:],
                ok[:4] + (vp(od.ptr),), ok[:4] + (vp(od.ptr + half - 8),), ok[:3] + (vp(od.ptr + 8), vp(od.ptr))):
        assert call(*bad) == L.OFC_EINVAL, bad
    sums = L.DeviceBuffer(16)
    assert lib.ofc_flow_calc_frames_dev_bidir_stats(*ok, None) == L.OFC_EINVAL
    eng.sync()
    assert (od.download((2 * n * P * 2,), np.float32) == -7.0).all()        # a refusal writes nothing
    # one pair of a two-pair engine: the halves of the smaller batch touch, which is no overlap
    assert call(eng._h, vp(fd.ptr), 2, vp(od.ptr), vp(od.ptr + P * 8)) == L.OFC_OK
    assert lib.ofc_flow_calc_frames_dev_bidir_stats(*ok, vp(sums.ptr)) == L.OFC_OK
    eng.sync()
    assert np.isfinite(od.download((2 * n * P * 2,), np.float32)).all()
    eng.close()


def test_column_sums_of_the_forward_field():
    from opticalflowclustering_amd.flow import FlowEngine
    L = _L()
    _, W, H, kw, n = B.case("ws15-two-column-tiles-272x80-2pairs")
    frames = B.clip(W, H, n + 1)
    eng = FlowEngine(W, H, params=L.FbParams(**kw), max_batch=n)
    fd = L.DeviceBuffer(frames.nbytes).upload(frames)
    od, sd = L.DeviceBuffer(2 * n * H * W * 8), L.DeviceBuffer(16)
    eng.calc_frames_dev_bidir(fd.ptr, n + 1, od.ptr, od.ptr + n * H * W * 8, uv_sum_ptr=sd.ptr)
    fwd = od.download((n, H, W, 2), np.float32)
    got, want = sd.download((2,), np.float64), fwd.astype(np.float64).reshape(-1, 2).sum(0)
    eng.close()
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())      # test_flow_column_sums_without_the_epilogue's


# ---- b. the stream against the staged route ----
def _SC():
    from tests import stream_compose_cases as SC
    return SC


STREAM_CHECK = dict(alpha=0.01, beta=0.5, keep=(0,))
STREAM_NAMES = ("consist_counts", "repair_counts", "records", "found", "links", "nlinks")


def _stream_spec(SC, **kw):
    return dict(consistency=STREAM_CHECK, repair=SC.REPAIR, blobs=SC.BLOBS, **kw)


def _run_stream(st, frames):
    import types
    for f in frames:
        st.push(f)
    cells = st.finish()
    r = types.SimpleNamespace(cells=cells, consist_counts=None, repair_counts=None, records=None, found=None, links=None, nlinks=None)
    if st.consist_args:
        r.consist_counts = st.consistency_stats()
    if st.repair_args:
        r.repair_counts = st.repair_stats()
    if st.blob_args:
        b = st.blobs()
        r.records, r.found, r.links, r.nlinks = b.records, b.found, b.links, b.nlinks
    return r


@pytest.fixture(scope="module")
def staged():
    """the clip of stream_compose_cases through the staged route, once: calc_frames_dev_bidir over the whole clip,
    consistency.check_dev on the two fields, and the resident pipeline (proved against exactly those in the pipeline tests
    below) for the repair, the blobs and their links.  Read-only."""
    import types
    from opticalflowclustering_amd import consistency as K
    from opticalflowclustering_amd.pipeline import ClipPipeline
    from opticalflowclustering_amd.stream import grid_cell_mean_flow
    SC, L = _SC(), _L()
    frames = SC.clip()
    n = len(frames) - 1
    fwd, bwd = _bidir(frames, B.DEFAULTS)
    P = SC.W * SC.H
    fd, bd, sd = (L.DeviceBuffer(n * P * 8).upload(fwd), L.DeviceBuffer(n * P * 8).upload(bwd), L.DeviceBuffer(n * P))
    counts, _ = K.check_dev(fd.ptr, bd.ptr, SC.W, SC.H, n, sd.ptr, *K.quantise(STREAM_CHECK["alpha"], STREAM_CHECK["beta"]))
    state = sd.download((n, SC.H, SC.W), np.uint8)
    blob = SC.BLOBS
    pipe = ClipPipeline(SC.W, SC.H, len(frames), batch_pairs=n, n_engines=1)
    try:
        pipe.upload_frames(frames)
        pipe.run_flow_bidirectional()
        assert np.array_equal(pipe.flows_host(), fwd) and np.array_equal(pipe.flows_bwd_host(), bwd)
        cons = pipe.consistency(STREAM_CHECK["alpha"], STREAM_CHECK["beta"])
        assert np.array_equal(cons.counts, counts) and np.array_equal(cons.state, state)
        repair_counts = pipe.repair(**SC.REPAIR)
        b = pipe.blobs(by="moving", consistent=True, links=blob["max_links"], labels=False, thr=blob["thr"],
                       connectivity=blob["connectivity"], min_area=blob["min_area"], max_blobs=blob["max_blobs"])
        repaired = pipe.flows_host()
    finally:
        pipe.close()
    cells = np.stack([grid_cell_mean_flow(repaired[t], SC.ROWS, SC.COLS) for t in range(n)])
    ref = types.SimpleNamespace(frames=frames, n=n, consist_counts=counts, repair_counts=repair_counts, records=b.records,
                                found=b.found, links=b.links, nlinks=b.nlinks, cells=cells)
    # the clip makes the stage bite: flagged vectors, filled ones, blobs, and links across what will be batch borders
    assert (counts[:, 1:].sum(1) > 0).all() and counts.sum(1).tolist() == [P] * n
    assert repair_counts[:, 1].sum() > 0 and b.found.sum() > 0 and b.nlinks.sum() > 0
    return ref


def _same(SC, got, want, names=STREAM_NAMES):
    for name in names:
        g, w = getattr(got, name), getattr(want, name)
        if isinstance(w, (list, tuple)):
            assert len(g) == len(w), name
            for t, (a, b) in enumerate(zip(g, w)):
                assert np.array_equal(a, b), (name, t)
        else:
            assert np.array_equal(g, w), name


@pytest.mark.parametrize("batch_pairs", (1, 3, 16))
def test_stream_equals_the_staged_route_at_every_batching(staged, batch_pairs):
    """per-pair counts, repair counts, blob records and the links (those across a batch border included) integer-equal; the
    cell means, which follow the repaired field, bit for bit as in test_gpu_stream_compose.py (a pair's field does not
    depend on its batch)"""
    from opticalflowclustering_amd.stream import FlowStream
    SC = _SC()
    st = FlowStream(SC.W, SC.H, batch_pairs=batch_pairs, rows=SC.ROWS, cols=SC.COLS, **_stream_spec(SC))
    try:
        got = _run_stream(st, staged.frames)
    finally:
        st.close()
    assert got.consist_counts.shape == (staged.n, 4) and got.consist_counts.dtype == np.int64
    assert len(got.links) == staged.n - 1
    _same(SC, got, staged)
    assert np.array_equal(got.cells.view(np.uint32), staged.cells.view(np.uint32))


def test_stream_reuse_growth_and_turning_the_stage_off(staged):
    """one stream: the clip, the clip again after the finish, a clip of more pairs than the first tables held (256), the
    stage off (a plain stream's cells), and on again"""
    from opticalflowclustering_amd.stream import FlowStream
    SC = _SC()
    frames = staged.frames
    plain_st = FlowStream(SC.W, SC.H, batch_pairs=3, rows=SC.ROWS, cols=SC.COLS)
    try:
        plain = _run_stream(plain_st, frames)
    finally:
        plain_st.close()
    st = FlowStream(SC.W, SC.H, batch_pairs=3, rows=SC.ROWS, cols=SC.COLS, **_stream_spec(SC))
    try:
        for _ in range(2):
            _same(SC, _run_stream(st, frames), staged)
        st.set_repair(on=False)
        st.set_blobs(connectivity=None)
        # a palindrome walk over the clip, 264 pairs: the counts table doubles from 256 rows
        walk = np.concatenate([frames, frames[-2:0:-1]])
        long = np.concatenate([walk] * (264 // (len(walk)) + 1) + [walk[:1]])[:265]
        got = _run_stream(st, long)
        assert got.consist_counts.shape == (264, 4) and (got.consist_counts.sum(1) == SC.W * SC.H).all()
        assert np.array_equal(got.consist_counts[:staged.n], staged.consist_counts)
        period = len(walk)
        assert np.array_equal(got.consist_counts[period:period + staged.n], staged.consist_counts)     # rows written after the growth
        st.push(frames[0])
        with pytest.raises(ValueError):
            st.consistency_stats()                                   # frames held: not idle
        for f in frames[1:]:
            st.push(f)
        st.finish()
        st.set_consistency(on=False)
        assert st.consist_args is None
        with pytest.raises(ValueError):
            st.consistency_stats()
        off = _run_stream(st, frames)
        assert off.consist_counts is None and np.array_equal(off.cells.view(np.uint32), plain.cells.view(np.uint32))
        st.set_consistency(**STREAM_CHECK)
        st.set_repair(**SC.REPAIR)
        st.set_blobs(**SC.BLOBS)
        _same(SC, _run_stream(st, frames), staged)
    finally:
        st.close()


def test_stream_refusals():
    from opticalflowclustering_amd.stream import FlowStream
    SC, L = _SC(), _L()
    lib = L.load()
    host = np.full((4, 4), -7, np.int64)
    with pytest.raises(ValueError):
        FlowStream(SC.W, SC.H, batch_pairs=2, photometric=True, consistency=True)
    st = FlowStream(SC.W, SC.H, batch_pairs=2, rows=SC.ROWS, cols=SC.COLS)
    try:
        assert lib.ofc_stream_read_consist(st._h, L.ptr(host), 4) == L.OFC_EINVAL        # without the check
        for args in ((1, -1, 1 << 31, 1), (1, 65537, 1 << 31, 1), (1, 655, -1, 1), (1, 655, (1 << 62) + 1, 1), (1, 655, 1 << 31, 0),
                     (1, 655, 1 << 31, 16)):
            assert lib.ofc_stream_set_consist(st._h, *args) == L.OFC_EINVAL, args
        assert lib.ofc_stream_set_consist(None, 1, 655, 1 << 31, 1) == L.OFC_EINVAL
        assert lib.ofc_stream_read_consist(None, None, 0) == L.OFC_EINVAL
        assert lib.ofc_stream_read_consist(st._h, L.ptr(host), 4) == L.OFC_EINVAL        # the refusals set nothing
        st.set_consistency()
        with pytest.raises(ValueError):
            st.set_photometric()                                     # one state map per stream, whichever comes second
        assert st.photo_args is None
        st.set_consistency(on=False)
        st.set_photometric()
        with pytest.raises(ValueError):
            st.set_consistency()
        assert st.consist_args is None
        st.set_photometric(on=False)
        st.set_consistency()
        frames = SC.clip()[:4]
        st.push(frames[0])
        with pytest.raises(ValueError):
            st.set_consistency(on=False)                             # not idle
        for f in frames[1:]:
            st.push(f)
        st.finish()
        assert lib.ofc_stream_read_consist(st._h, L.ptr(host), 2) == L.OFC_EINVAL and (host == -7).all()     # too small
        L.check(lib.ofc_stream_read_consist(st._h, L.ptr(host), 4))
        assert (host[:3].sum(1) == SC.W * SC.H).all() and (host[3] == -7).all()
    finally:
        st.close()


# ---- c. the pipeline ----
def test_pipeline_bidirectional_route_and_the_reversed_one(staged):
    """run_flow_bidirectional() + consistency() against consistency.check_dev on what calc_frames_dev_bidir gives for the
    pipeline's own batches (1 + 4 + 4 pairs on two engines); run_backward_flow() after it, and it after that; the consumers
    of the state map see it after either"""
    from opticalflowclustering_amd import consistency as K
    from opticalflowclustering_amd.flow import FlowEngine
    from opticalflowclustering_amd.pipeline import ClipPipeline, batch_schedule
    SC, L = _SC(), _L()
    frames, n, P = staged.frames, staged.n, SC.W * SC.H
    schedule = batch_schedule(n, 4)
    assert schedule == [1, 4, 4]
    fwd, bwd = np.empty((n, SC.H, SC.W, 2), np.float32), np.empty((n, SC.H, SC.W, 2), np.float32)
    eng = FlowEngine(SC.W, SC.H, max_batch=4)
    p0 = 0
    for m in schedule:
        fwd[p0:p0 + m], bwd[p0:p0 + m] = _bidir(frames[p0:p0 + m + 1], B.DEFAULTS, eng=eng)
        p0 += m
    eng.close()
    fd, bd, sd = (L.DeviceBuffer(n * P * 8).upload(fwd), L.DeviceBuffer(n * P * 8).upload(bwd), L.DeviceBuffer(n * P))
    counts, _ = K.check_dev(fd.ptr, bd.ptr, SC.W, SC.H, n, sd.ptr)
    state = sd.download((n, SC.H, SC.W), np.uint8)
    pipe = ClipPipeline(SC.W, SC.H, len(frames), batch_pairs=4, n_engines=2)
    try:
        pipe.upload_frames(frames)
        pipe.run_flow()
        forward = pipe.flows_host()
        for _ in range(2):
            pipe.run_flow_bidirectional()
            assert pipe.bwd_reversed is False
            assert np.array_equal(pipe.flows_host(), fwd) and np.array_equal(pipe.flows_bwd_host(), bwd)
            assert np.array_equal(fwd, forward)                      # run_flow()'s field, as run_flow() leaves it
            c = pipe.consistency()
            assert np.array_equal(c.counts, counts) and np.array_equal(c.state, state)
            sums = pipe.uv_sums.download((len(schedule), 2), np.float64).sum(0)
            want = fwd.astype(np.float64).reshape(-1, 2).sum(0)
            assert pipe._sums_valid and np.abs(sums - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
            b = pipe.blobs(consistent=True, thr=SC.BLOBS["thr"], min_area=SC.BLOBS["min_area"], max_blobs=SC.BLOBS["max_blobs"])
            assert ((b.keys != 255) <= (state == 0)).all() and (b.keys != 255).any()
            km = pipe.run_kmeans(SC.CENTRES, max_iter=5, consistent=True)
            assert km is not None
            # the reversed route still works behind it, and leaves its own order
            pipe.run_backward_flow()
            assert pipe.bwd_reversed is True
            rev = pipe.flows_bwd_host()
            c2 = pipe.consistency()
            assert c2.counts.sum(1).tolist() == [P] * n
            # both are backward fields of the same pairs (another batching of another clip: no bit equality is promised)
            assert np.abs(rev[::-1] - bwd).max() <= 1e-3
            assert np.array_equal(c2.counts, K.check(forward, rev, bwd_reversed=True).counts)
    finally:
        pipe.close()
