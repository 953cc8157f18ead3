"""Farneback windows wider than 17 px (winsize 19 .. OFC_WINSIZE_MAX = 255) through every layer: k_box_solve_wide stage by
stage against the oracle's box mean + solve (windows wider than the frame included), the flow engine end to end and in
every entry point that runs it (single pair, 64-pair batches, the _stats form, push, ComputeOpticalFLow, ofc_stream),
calcOpticalFlowFarneback, computeOpticalFlow.py --winsize, and the refusals above the bound.  The oracle's wide-window
semantics are pinned by test_oracle_farneback_wide_window.py.  Bars as in test_gpu_flow.py."""
import csv
import ctypes as C

import numpy as np
import pytest

from opticalflowclustering_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.linalg.norm((a - b).ravel().astype(np.float64)) / max(np.linalg.norm(b.ravel().astype(np.float64)), 1e-30)


def oracle_params(**kw):
    p = O.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def assert_flow_bars(got, want):
    assert rel(got, want) <= 1e-4, rel(got, want)
    assert np.abs(got - want).max() <= 1e-3, np.abs(got - want).max()


# ---- 1. stage parity: box mean + solve ----
def _box_case(W, H, ws):
    from opticalflowclustering_amd import stages
    rng = np.random.default_rng(W * 7 + H + ws)
    M = rng.random((H, W, 5)).astype(np.float32) + np.float32([1, 0, 1, 0, 0])
    z5 = np.zeros((H, W, 5), np.float32)
    want, _ = O.update_flow_blur(z5, z5, np.zeros((H, W, 2), np.float32), M, ws, False)
    got = stages.box_solve(M, ws)
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (W, H, ws)
    return got, want


@pytest.mark.parametrize("ws", [19, 21, 31, 61, 101, 255])
@pytest.mark.parametrize("W,H", [(130, 60), (963, 541)])
def test_box_solve_wide(W, H, ws):
    _box_case(W, H, ws)


@pytest.mark.parametrize("W,H,ws", [(1920, 1080, 61), (40, 24, 61), (17, 200, 255), (16, 16, 255), (1100, 37, 19)])
def test_box_solve_wide_odd_geometry(W, H, ws):
    """1080p (several tiles and strips), and windows wider than the frame in one or both directions"""
    _box_case(W, H, ws)


def test_box_solve_wide_is_not_the_narrow_window():
    rng = np.random.default_rng(3)
    M = rng.random((60, 130, 5)).astype(np.float32) + np.float32([1, 0, 1, 0, 0])
    from opticalflowclustering_amd import stages
    assert np.abs(stages.box_solve(M, 19) - stages.box_solve(M, 17)).max() > 1e-4


# ---- 2. the engine against the oracle ----
def _t(W, H):
    return synth.translated_pair(W, H, 2.5, -1.25)


def _nr(W, H):
    return synth.nonrigid_pair(W, H)[:2]


ENGINE_CASES = [("ws21_t", 480, 270, dict(winsize=21), _t),
                ("ws31_nonrigid", 480, 270, dict(winsize=31), _nr),
                ("ws61_t", 480, 270, dict(winsize=61), _t),
                ("ws61_nonrigid", 480, 270, dict(winsize=61), _nr),
                ("ws41_odd", 963, 541, dict(winsize=41), _t),
                ("ws31_1080p_nonrigid", 1920, 1080, dict(winsize=31), _nr),
                ("ws31_levels0", 480, 270, dict(winsize=31, levels=0), lambda W, H: synth.translated_pair(W, H, 0.8, 0.4)),
                ("ws31_scale08_levels4", 500, 300, dict(winsize=31, pyr_scale=0.8, levels=4), _t),
                ("ws31_poly7", 480, 270, dict(winsize=31, poly_n=7, poly_sigma=1.5), _nr)]


@pytest.mark.parametrize("name,W,H,kw,gen", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_flow_wide_window_end_to_end(name, W, H, kw, gen):
    from opticalflowclustering_amd._lib import FbParams
    from opticalflowclustering_amd.flow import FlowEngine
    a, b = gen(W, H)
    want = O.farneback(a, b, oracle_params(**kw))
    eng = FlowEngine(W, H, params=FbParams(**kw))
    got = eng.calc(a, b)
    eng.close()
    assert_flow_bars(got, want)


@pytest.fixture
def fb():
    from opticalflowclustering_amd import flow
    flow.clear_farneback_cache()
    yield flow
    flow.clear_farneback_cache()


def test_calc_optical_flow_farneback_ws31(fb):
    from opticalflowclustering_amd import calcOpticalFlowFarneback
    W, H = 640, 360
    a, b = synth.translated_pair(W, H, 3.0, -1.5)
    got = calcOpticalFlowFarneback(a, b, None, 0.5, 3, 31, 3, 5, 1.2, 0)
    assert_flow_bars(got, O.farneback(a, b, oracle_params(winsize=31)))
    assert len(fb._fb_engines) == 1
    got2 = fb.calcOpticalFlowFarneback(b, a, None, 0.5, 2, 61, 2, 7, 1.5, 0)
    assert_flow_bars(got2, O.farneback(b, a, oracle_params(levels=2, winsize=61, iterations=2, poly_n=7, poly_sigma=1.5)))


# ---- 3. batch geometry: 64 pairs in one call equal the single-pair results ----
@pytest.mark.parametrize("W,H", [(640, 360), (1920, 1080)])
def test_flow_wide_window_64_pair_batch(W, H):
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd._lib import FbParams, check, load
    from opticalflowclustering_amd.flow import FlowEngine
    P = 64
    frames = _lib.DeviceBuffer((P + 1) * W * H)
    flows = _lib.DeviceBuffer(P * H * W * 8)
    try:
        check(load().ofc_synth_frames_dev(0, C.c_void_p(frames.ptr), W, H, P + 1, 0, 0))
        eng = FlowEngine(W, H, FbParams(winsize=31), max_batch=P)
        eng.calc_frames_dev(frames.ptr, P + 1, flows.ptr)
        for t in range(P):
            pair = frames.download((2, H, W), np.uint8, offset=t * W * H)
            got = flows.download((H, W, 2), np.float32, offset=t * H * W * 8)
            assert np.array_equal(got, eng.calc(pair[0], pair[1])), t
            if t == 17:
                assert_flow_bars(got, O.farneback(pair[0], pair[1], oracle_params(winsize=31)))
        eng.close()
    finally:
        frames.free()
        flows.free()


# ---- 4. the _stats form ----
def test_flow_wide_window_stats_form():
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd._lib import FbParams, check, load
    from opticalflowclustering_amd.flow import FlowEngine
    W, H, P = 480, 270, 6
    frames = _lib.DeviceBuffer((P + 1) * W * H)
    flows = _lib.DeviceBuffer(P * H * W * 8)
    sums = _lib.DeviceBuffer(16)
    try:
        check(load().ofc_synth_frames_dev(0, C.c_void_p(frames.ptr), W, H, P + 1, 1, 3))
        eng = FlowEngine(W, H, FbParams(winsize=31), max_batch=P)
        eng.calc_frames_dev(frames.ptr, P + 1, flows.ptr, uv_sum_ptr=sums.ptr)
        fl = flows.download((P, H, W, 2), np.float32)
        got = sums.download((2,), np.float64)
        want = fl.astype(np.float64).reshape(-1, 2).sum(0)
        assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(fl).astype(np.float64).sum())
        allf = frames.download((P + 1, H, W), np.uint8)
        assert_flow_bars(fl[2], O.farneback(allf[2], allf[3], oracle_params(winsize=31)))
        eng.close()
    finally:
        frames.free()
        flows.free()
        sums.free()


# ---- 5. streaming forms ----
def make_video(W=480, H=270, T=3, seed=5):
    p = synth.texture_params(seed)
    frames = []
    for t in range(T):
        g = synth.frame(W, H, 1.9 * t, -0.8 * t, p)
        frames.append(np.stack([g, np.roll(g, 3, 1), 255 - g], -1).astype(np.uint8))
    return np.stack(frames)


def test_flow_engine_push_ws31():
    from opticalflowclustering_amd._lib import FbParams
    from opticalflowclustering_amd.flow import FlowEngine
    W, H = 480, 270
    v = make_video(W, H, T=3)
    g = [O.bgr2gray(f) for f in v]
    eng = FlowEngine(W, H, FbParams(winsize=31))
    assert eng.push(g[0]) is None
    for t in (1, 2):
        assert_flow_bars(eng.push(g[t]), O.farneback(g[t - 1], g[t], oracle_params(winsize=31)))
    eng.close()


def test_compute_optical_flow_class_ws31():
    from opticalflowclustering_amd._lib import FbParams
    from opticalflowclustering_amd.computeOpticalFlowModule import ComputeOpticalFLow
    v = make_video()
    cf = ComputeOpticalFLow(v[0], params=FbParams(winsize=31))
    for t in range(1, len(v)):
        _, flow = cf.compute(v[t], return_flow=True)
        assert_flow_bars(flow, O.farneback(O.bgr2gray(v[t - 1]), O.bgr2gray(v[t]), oracle_params(winsize=31)))
    cf.close()


def test_flow_stream_ws31():
    from opticalflowclustering_amd._lib import FbParams
    from opticalflowclustering_amd.stream import FlowStream
    W, H, T = 500, 280, 6
    p = synth.texture_params(2)
    frames = [synth.frame(W, H, 1.3 * t, -0.7 * t, p) for t in range(T)]
    st = FlowStream(W, H, batch_pairs=3, params=FbParams(winsize=31))
    for f in frames:
        st.push(f)
    cells = st.finish()
    st.close()
    assert cells.shape == (T - 1, 350, 2)
    xs, ys = W // 25, H // 14
    for t in range(T - 1):
        fl = O.farneback(frames[t], frames[t + 1], oracle_params(winsize=31))
        want = fl[:ys * 14, :xs * 25].reshape(14, ys, 25, xs, 2).astype(np.float64).mean((1, 3)).reshape(350, 2)
        assert np.abs(cells[t] - want).max() <= 2e-4, t


# ---- 6. refusals ----
def test_winsize_above_the_bound_is_refused(fb):
    from opticalflowclustering_amd import stages
    from opticalflowclustering_amd._lib import OFC_EUNSUPPORTED, FbParams, OfcError
    from opticalflowclustering_amd.flow import FlowEngine
    a, b = synth.translated_pair(64, 48, 1.0, 0.0)
    for ws in (257, 301):
        with pytest.raises(OfcError) as e:
            fb.calcOpticalFlowFarneback(a, b, None, 0.5, 3, ws, 3, 5, 1.2, 0)
        assert e.value.code == OFC_EUNSUPPORTED and "255" in str(e.value)
        with pytest.raises(OfcError) as e:
            FlowEngine(64, 48, FbParams(winsize=ws))
        assert e.value.code == OFC_EUNSUPPORTED
        with pytest.raises(OfcError) as e:
            stages.box_solve(np.ones((48, 64, 5), np.float32), ws)
        assert e.value.code == OFC_EUNSUPPORTED
    assert len(fb._fb_engines) == 0
    for ws in (20, 32, 256):                                    # OFC_EINVAL, as before
        with pytest.raises(ValueError, match="odd"):
            fb.calcOpticalFlowFarneback(a, b, None, 0.5, 3, ws, 3, 5, 1.2, 0)
    assert len(fb._fb_engines) == 0
    got = fb.calcOpticalFlowFarneback(a, b, None, 0.5, 3, 255, 3, 5, 1.2, 0)   # the bound itself is implemented
    assert_flow_bars(got, O.farneback(a, b, oracle_params(winsize=255)))


# ---- 7. computeOpticalFlow.py --winsize ----
def test_compute_optical_flow_cli_winsize(tmp_path, monkeypatch):
    from opticalflowclustering_amd import computeOpticalFlow
    from opticalflowclustering_amd.computeOpticalFlowModule import ComputeOpticalFLow
    seen = []

    class Spy(ComputeOpticalFLow):
        def __init__(self, *a, params=None, **kw):
            seen.append((params.winsize, params.poly_n, params.poly_sigma))
            super().__init__(*a, params=params, **kw)

    monkeypatch.setattr(computeOpticalFlow, "ComputeOpticalFLow", Spy)
    v = make_video()
    src = str(tmp_path / "clip.npy")
    np.save(src, v)
    computeOpticalFlow.main(["-i", src, "--winsize", "31"])
    assert seen == [(31, 5, 1.2)]
    rows = list(csv.reader(open(src + "_opticalFlow.csv")))[1:]
    assert len(rows) == len(v) - 1
    for t, r in enumerate(rows):
        want = O.flow_to_bgr(O.farneback(O.bgr2gray(v[t]), O.bgr2gray(v[t + 1]), oracle_params(winsize=31)))[1]
        assert abs(float(r[2]) - want) <= 1e-5 * want
    computeOpticalFlow.main(["-i", src])                      # the documented command keeps the reference's window
    assert seen[-1] == (15, 5, 1.2)
