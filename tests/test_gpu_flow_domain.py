"""The flow engine over the parameter domain it accepts, against the CPU oracle: the fused iteration at each of its six
windows and the staged box mean + solve at each of its seven with widths on their tile seams, the level image on all four
launch paths at pyramid scales other than 0.5, a table of parameters x sizes end to end (all three upsample variants of
the first iteration included), and the edge of the domain -- what is refused, with which code, and that it is refused when
the engine is created.  The cases are tests/flow_domain_cases.py's; test_oracle_flow_domain.py proves on the CPU that each
of them is well-conditioned, so a failure here is the kernels'."""
import ctypes as C

import numpy as np
import pytest

import flow_domain_cases as D
from opticalflowclustering_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    from opticalflowclustering_amd import stages
    return stages


@pytest.fixture(scope="module")
def d64():
    return D.recorded_stage_distances()


# ---- 1. the fused iteration and the staged box mean + solve, every window, widths on the seams ----
@pytest.mark.parametrize("ws,name,W,H", D.ITER_CASES, ids=[D.iter_case_id(*c, "1-3") for c in D.ITER_CASES])
def test_fused_iteration_every_window_on_its_seams(st, d64, ws, name, W, H):
    """k_flow_iter<M, 0> after 1, 2 and 3 iterations against the oracle's unrolled loop.  Bar per case: the larger of the
    winsize-15 bar (2e-5 * max(1, |want|) up to two iterations, 5e-5 from three) and 4 x the oracle's own recorded distance
    from float64 on that input (itself at most 10 x the winsize-15 bar, asserted on the CPU)"""
    R0, R1, flow = D.iter_inputs(W, H, seed=W + ws)
    want = D.oracle_iterations(R0, R1, flow, max(D.ITER_COUNTS), ws)
    for it in D.ITER_COUNTS:
        got = st.flow_iterate(R0, R1, flow, it, winsize=ws, mode=0)
        bar, _ = D.stage_bar(D.iter_base_bar(it), d64[D.iter_case_id(ws, name, W, H, it)], want[it - 1])
        err = np.abs(got - want[it - 1])
        print(f"{D.iter_case_id(ws, name, W, H, it)}: max|d| {err.max():.3e} bar {bar:.3e}")
        assert np.isfinite(got).all()
        assert err.max() <= bar, (it, err.max(), bar, np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("ws,name,W,H", D.BOX_CASES, ids=[D.box_case_id(*c) for c in D.BOX_CASES])
def test_box_solve_every_window_on_its_seams(st, d64, ws, name, W, H):
    """k_box_solve<M> (tile of 256 - 2M columns, as the fused iteration's) against the oracle; bar as above on
    test_box_solve's 1e-5 * max(1, |want|)"""
    M = D.box_input(W, H)
    want = D.oracle_box_solve(M, ws)
    got = st.box_solve(M, ws)
    bar, _ = D.stage_bar(D.BOX_BASE_BAR, d64[D.box_case_id(ws, name, W, H)], want)
    err = np.abs(got - want)
    print(f"{D.box_case_id(ws, name, W, H)}: max|d| {err.max():.3e} bar {bar:.3e}")
    assert np.isfinite(got).all()
    assert err.max() <= bar, (err.max(), bar, np.unravel_index(err.argmax(), err.shape))


# ---- 2. level images at other pyramid scales, all four launch paths ----
_LEVEL_CASES = D.level_cases()


def test_level_image_sweep_reaches_every_launch_path():
    seen = {c[0].rsplit("-", 1)[1] for c in _LEVEL_CASES}
    assert seen == set(D.LEVEL_PATHS), seen


@pytest.mark.parametrize("cid,ps,lv,W,H,k", _LEVEL_CASES, ids=[c[0] for c in _LEVEL_CASES])
def test_level_image_bit_exact_at_other_scales(st, cid, ps, lv, W, H, k):
    from opticalflowclustering_amd._lib import FbParams
    rng = np.random.default_rng(W + H)
    gray = rng.integers(0, 256, (H, W), dtype=np.uint8)
    po = D.oracle_params(dict(pyr_scale=ps, levels=lv))
    assert 0 <= k <= O.pyramid_levels(W, H, po)
    w, h, ksize, _ = O.level_geometry(W, H, k, po)
    assert cid.endswith(D.level_path(W, H, w, h, ksize))      # the id names the path the launch conditions give
    got, want = st.level_image(gray, k, FbParams(pyr_scale=ps, levels=lv)), O.level_image(gray, k, po)
    assert got.shape == want.shape == (h, w)
    assert np.array_equal(got, want), (k, np.abs(got - want).max())


# ---- 3. the engine over a table of parameters and sizes ----
@pytest.mark.parametrize("name,kw,W,H", D.ENGINE_CASES, ids=[c[0] for c in D.ENGINE_CASES])
def test_engine_parameter_table(name, kw, W, H):
    """BASELINE.md section 5's bars: ||d||2 / ||ref||2 <= 1e-4 and max|d| <= 1e-3 px"""
    from opticalflowclustering_amd._lib import FbParams
    from opticalflowclustering_amd.flow import FlowEngine
    a, b = synth.translated_pair(W, H, *D.ENGINE_MOTION)
    want = O.farneback(a, b, D.oracle_params(kw))
    eng = FlowEngine(W, H, params=FbParams(**kw))
    got = eng.calc(a, b)
    eng.close()
    r, m = D.rel(got, want), np.abs(got - want).max()
    print(f"{name}: rel {r:.3e} max|d| {m:.3e}")
    assert np.isfinite(got).all()
    assert r <= 1e-4, r
    assert m <= 1e-3, m


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("name", D.ENGINE_BATCHED)
def test_batched_path_equals_pairwise_at_other_parameters(name, T):
    """calc_frames_dev on T resident frames (max_batch 3): each field bit for bit the pairwise calc's, and the two column
    sums of the stats form against float64 sums of the downloaded fields"""
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.flow import FlowEngine
    _, kw, W, H = D.engine_case(name)
    p = synth.texture_params(3)
    frames = np.stack([synth.frame(W, H, 0.8 * t, -0.4 * t, p) for t in range(T)])
    eng = FlowEngine(W, H, params=_lib.FbParams(**kw), max_batch=3)
    fd = _lib.DeviceBuffer(frames.nbytes).upload(frames)
    od = _lib.DeviceBuffer((T - 1) * H * W * 8)
    sd = _lib.DeviceBuffer(16)
    eng.calc_frames_dev(fd.ptr, T, od.ptr)
    flows = od.download((T - 1, H, W, 2), np.float32)
    for t in range(T - 1):
        assert np.array_equal(flows[t], eng.calc(frames[t], frames[t + 1])), t
    od.zero()
    eng.calc_frames_dev(fd.ptr, T, od.ptr, uv_sum_ptr=sd.ptr)
    assert np.array_equal(od.download((T - 1, H, W, 2), np.float32), flows)
    got = sd.download((2,), np.float64)
    want = flows.astype(np.float64).reshape(-1, 2).sum(0)
    eng.close()
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())      # test_flow_column_sums_without_the_epilogue's


# ---- 4. the edge of the domain ----
def _create(W, H, max_batch=1, **kw):
    """ofc_flow_create through the C ABI -> (code, message, handle)"""
    from opticalflowclustering_amd import _lib
    h = C.c_void_p()
    p = _lib.FbParams(**kw)
    rc = _lib.load().ofc_flow_create(0, W, H, C.byref(p), max_batch, C.byref(h))
    return rc, _lib.load().ofc_last_error().decode(), h


EINVAL, EUNSUPPORTED, OK = -1, -6, 0        # include/ofc.h

# (id, W, H, max_batch, parameters, code): every clause of check_frame_and_fb_params and ofc_flow_create, the value just
# outside and the value just inside.  The 16384 side is tested through refusals only (no 16384^2 engine is allocated).
EDGE = [("W15", 15, 64, 1, {}, EINVAL), ("H15", 64, 15, 1, {}, EINVAL), ("16x16", 16, 16, 1, {}, OK),
        ("W16385", 16385, 64, 1, {}, EINVAL), ("H16385", 64, 16385, 1, {}, EINVAL),
        ("pyr_scale0", 64, 64, 1, dict(pyr_scale=0.0), EINVAL), ("pyr_scale1", 64, 64, 1, dict(pyr_scale=1.0), EINVAL),
        ("pyr_scale-0.5", 64, 64, 1, dict(pyr_scale=-0.5), EINVAL), ("pyr_scaleNaN", 64, 64, 1, dict(pyr_scale=float("nan")), EINVAL),
        ("pyr_scale0.99", 64, 64, 1, dict(pyr_scale=0.99), OK),
        ("levels-1", 64, 64, 1, dict(levels=-1), EINVAL), ("levels17", 64, 64, 1, dict(levels=17), EINVAL),
        ("levels0", 64, 64, 1, dict(levels=0), OK), ("levels16", 64, 64, 1, dict(levels=16), OK),
        ("iterations0", 64, 64, 1, dict(iterations=0), EINVAL), ("iterations65", 64, 64, 1, dict(iterations=65), EINVAL),
        ("iterations1", 64, 64, 1, dict(iterations=1), OK), ("iterations64", 64, 64, 1, dict(iterations=64), OK),
        ("winsize3", 64, 64, 1, dict(winsize=3), EINVAL), ("winsize6", 64, 64, 1, dict(winsize=6), EINVAL),
        ("winsize16", 64, 64, 1, dict(winsize=16), EINVAL), ("winsize256", 64, 64, 1, dict(winsize=256), EINVAL),
        ("winsize257", 64, 64, 1, dict(winsize=257), EUNSUPPORTED),
        ("winsize5", 64, 64, 1, dict(winsize=5), OK), ("winsize255", 64, 64, 1, dict(winsize=255), OK),
        ("poly_n3", 64, 64, 1, dict(poly_n=3), EUNSUPPORTED), ("poly_n9", 64, 64, 1, dict(poly_n=9), EUNSUPPORTED),
        ("poly_n6", 64, 64, 1, dict(poly_n=6), EUNSUPPORTED),
        ("poly_n5", 64, 64, 1, dict(poly_n=5), OK), ("poly_n7", 64, 64, 1, dict(poly_n=7), OK),
        ("flags4", 64, 64, 1, dict(flags=4), EUNSUPPORTED), ("flags256", 64, 64, 1, dict(flags=256), EUNSUPPORTED),
        ("max_batch0", 64, 64, 0, {}, EINVAL), ("max_batch4097", 64, 64, 4097, {}, EINVAL),
        ("max_batch1", 64, 64, 1, {}, OK), ("max_batch4096", 16, 16, 4096, {}, OK),
        # what the launches refuse, refused at create: the fused iteration's 32-bit offsets, W * H * 5 >= 2^30
        ("16384x13108-fused-offsets", 16384, 13108, 1, {}, EUNSUPPORTED)]


@pytest.mark.parametrize("cid,W,H,mb,kw,code", EDGE, ids=[c[0] for c in EDGE])
def test_edge_of_the_domain(cid, W, H, mb, kw, code):
    from opticalflowclustering_amd import _lib
    rc, msg, h = _create(W, H, mb, **kw)
    try:
        assert rc == code, (rc, msg)
        if code == OK:
            assert h.value
        else:
            assert not h.value and msg
    finally:
        if h.value:
            _lib.load().ofc_flow_destroy(h)


# a level whose blur would be wider than 31 taps: (W, H, parameters refused, the engine-table case with fewer levels)
BLUR = [("scale0.5-levels4-512x512", 512, 512, dict(pyr_scale=0.5, levels=4), "edge-512x512-levels3-of-scale0.5", "level 4"),
        ("scale0.06-levels1-640x640", 640, 640, dict(pyr_scale=0.06, levels=1), "edge-640x640-levels0-of-scale0.06", "level 1")]


@pytest.mark.parametrize("cid,W,H,bad,good,level", BLUR, ids=[c[0] for c in BLUR])
def test_level_blur_limit_is_refused_at_create(cid, W, H, bad, good, level):
    """refused by ofc_flow_create with the level and the limit in the message; the same parameters with fewer levels are
    accepted and run (test_engine_parameter_table's case `good`, same W x H)"""
    from opticalflowclustering_amd import _lib
    _, kw, gw, gh = D.engine_case(good)
    assert (gw, gh) == (W, H) and kw["pyr_scale"] == bad["pyr_scale"] and kw["levels"] == bad["levels"] - 1
    rc, msg, h = _create(W, H, **bad)
    assert rc == EUNSUPPORTED and not h.value, (rc, msg)
    assert level in msg and "31" in msg and f"levels <= {kw['levels']}" in msg, msg
    rc, msg, h = _create(W, H, **{k: kw[k] for k in ("pyr_scale", "levels")})
    assert rc == OK and h.value, msg
    _lib.load().ofc_flow_destroy(h)
    if bad["pyr_scale"] == 0.5:     # one pixel short of reaching level 4, the 32-pixel rule clamps levels=4 to 3: accepted
        rc, msg, h = _create(W - 1, H, **bad)
        assert rc == OK and h.value, msg
        _lib.load().ofc_flow_destroy(h)


def test_every_front_end_refuses_before_anything_is_stored():
    """ofc_stream_create, FlowEngine, ComputeOpticalFLow and calcOpticalFlowFarneback all go through ofc_flow_create"""
    from opticalflowclustering_amd import _lib, calcOpticalFlowFarneback, flow
    from opticalflowclustering_amd.computeOpticalFlowModule import ComputeOpticalFLow
    from opticalflowclustering_amd.flow import FlowEngine
    bad = _lib.FbParams(pyr_scale=0.5, levels=4)
    with pytest.raises(_lib.OfcError) as e:
        FlowEngine(512, 512, params=bad)
    assert e.value.code == EUNSUPPORTED
    h = C.c_void_p()
    rc = _lib.load().ofc_stream_create(0, 512, 512, C.byref(bad), 2, 14, 25, C.byref(h))
    assert rc == EUNSUPPORTED and not h.value and "level 4" in _lib.load().ofc_last_error().decode()
    g = np.zeros((512, 512), np.uint8)
    flow.clear_farneback_cache()
    with pytest.raises(_lib.OfcError) as e:
        calcOpticalFlowFarneback(g, g, None, 0.5, 4, 15, 3, 5, 1.2, 0)
    assert e.value.code == EUNSUPPORTED and not flow._fb_engines
    with pytest.raises(_lib.OfcError) as e:
        ComputeOpticalFLow(np.zeros((512, 512, 3), np.uint8), params=bad)      # refused before the first frame is stored
    assert e.value.code == EUNSUPPORTED
