"""The three strip-marching flow kernels at every strip height their cost models pick (tests/flow_geometry_cases.py;
test_flow_geometry_host.py proves on the CPU what the tables reach and that bit equality is a fair demand on the inputs).
  stage level   k_flow_iter<M, 0> through ofc_flow_iterate mode 0 at every multiple of 16 rows: the same bits as at 16 rows,
                which is itself held to the oracle
  engine level  one batch of up to 256 pairs of a small frame, which moves k_flow_iter (all three upsample forms),
                k_box_solve<8> and k_polyexp through the heights production runs: every pair the same bits as the same clip
                computed three pairs at a time (16-row strips everywhere), three pairs against the oracle"""
import ctypes as C

import numpy as np
import pytest

import flow_domain_cases as D
import flow_geometry_cases as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    from opticalflowclustering_amd import stages
    return stages


@pytest.fixture(scope="module")
def d64():
    return G.recorded_stage_distances()


# ---- 1. the fused iteration at every strip height ----
@pytest.mark.parametrize("ws,W,H", G.STAGE_CASES, ids=[f"ws{c[0]}-M{c[0] // 2}-{c[1]}x{c[2]}" for c in G.STAGE_CASES])
def test_fused_iteration_is_bit_identical_at_every_strip_height(st, d64, ws, W, H):
    R0, R1, flow = G.stage_inputs(ws, W, H)
    want = D.oracle_iterations(R0, R1, flow, max(G.STAGE_ITERS), ws)
    auto = st.flow_launch_geometry(W, H, 1, ws)[0]
    assert auto in G.stage_rows(H)
    for it in G.STAGE_ITERS:
        base = st.flow_iterate(R0, R1, flow, it, winsize=ws, mode=0, rows_per_block=G.SUPER_STEP)
        bar, _ = D.stage_bar(D.iter_base_bar(it), d64[G.stage_case_id(ws, W, H, it)], want[it - 1])
        err = np.abs(base - want[it - 1])
        print(f"{G.stage_case_id(ws, W, H, it)}: 16-row strips max|d| {err.max():.3e} bar {bar:.3e}")
        assert np.isfinite(base).all()
        assert err.max() <= bar, (it, err.max(), bar, np.unravel_index(err.argmax(), err.shape))
        for rows in G.stage_rows(H)[1:]:
            got = st.flow_iterate(R0, R1, flow, it, winsize=ws, mode=0, rows_per_block=rows)
            diff = got != base
            assert not diff.any(), (it, rows, int(diff.sum()), np.argwhere(diff.any(-1))[:4].tolist(),
                                    float(np.abs(got - base).max()))
        # 0 = the cost model's height, the one the hook reports
        assert np.array_equal(st.flow_iterate(R0, R1, flow, it, winsize=ws, mode=0, rows_per_block=0),
                              st.flow_iterate(R0, R1, flow, it, winsize=ws, mode=0, rows_per_block=auto))


def test_negative_strip_height_is_refused(st):
    from opticalflowclustering_amd import _lib
    R0, R1, flow = G.stage_inputs(15, 64, 48)
    out = np.empty_like(flow)
    rc = _lib.load().ofc_flow_iterate(0, _lib.ptr(R0), _lib.ptr(R1), _lib.ptr(flow), 64, 48, 15, 1, 0, -16, _lib.ptr(out))
    assert rc == _lib.OFC_EINVAL and "rows_per_block" in _lib.load().ofc_last_error().decode()
    with pytest.raises(ValueError):
        st.flow_iterate(R0, R1, flow, 1, winsize=15, mode=0, rows_per_block=-1)


# ---- 2. the engine at the heights a large batch gets ----
_oracle_cache = {}      # (case, pair) -> the oracle's flow: frame t of the clip does not depend on the batch it is part of


def _oracle_flow(name, kw, a, b, t):
    if (name, t) not in _oracle_cache:
        _oracle_cache[(name, t)] = O.farneback(a, b, D.oracle_params(kw))
    return _oracle_cache[(name, t)]


def _fill(buf, value):
    from opticalflowclustering_amd import _lib
    _lib.check(_lib.load().ofc_memset(0, C.c_void_p(buf.ptr), value, buf.nbytes))


def _pair_chunks(n, P):
    """(first pair, pairs) chunks of at most ~32 MB of flow vectors: only what is compared is on the host at a time"""
    step = max(1, (32 << 20) // (8 * P))
    return [(t, min(step, n - t)) for t in range(0, n, step)]


@pytest.mark.parametrize("name,kw,W,H,n", G.ENGINE_RUNS, ids=[G.engine_run_id(c[0], c[4]) for c in G.ENGINE_RUNS])
def test_large_batch_equals_the_clip_three_pairs_at_a_time(st, name, kw, W, H, n):
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.flow import FlowEngine
    P = W * H
    frames = _lib.DeviceBuffer((n + 1) * P)
    got_d = _lib.DeviceBuffer(n * P * 8 + G.SLACK_BYTES)
    ref_d = _lib.DeviceBuffer(n * P * 8)
    sums_d = _lib.DeviceBuffer(16)
    big = FlowEngine(W, H, params=_lib.FbParams(**kw), max_batch=n)
    small = FlowEngine(W, H, params=_lib.FbParams(**kw), max_batch=G.REF_BATCH)
    try:
        _lib.check(_lib.load().ofc_synth_frames_dev(0, C.c_void_p(frames.ptr), W, H, n + 1, 0, 0))
        heights = [st.flow_launch_geometry(w, h, n, kw["winsize"]) for w, h in G.engine_levels(W, H, kw)]
        # the reference: the same clip three pairs at a time
        for t in range(0, n, G.REF_BATCH):
            m = min(G.REF_BATCH, n - t)
            small.calc_frames_dev(frames.ptr + t * P, m + 1, ref_d.ptr + t * P * 8, sync=False)
        small.sync()
        # one batch of n pairs, plain and with the column sums
        for stats in (False, True):
            _fill(got_d, 0xFF)
            _fill(sums_d, 0xFF)
            big.calc_frames_dev(frames.ptr, n + 1, got_d.ptr, uv_sum_ptr=sums_d.ptr if stats else None)
            want_sum = np.zeros(2)
            for t0, m in _pair_chunks(n, P):
                got = got_d.download((m, H, W, 2), np.float32, offset=t0 * P * 8)
                ref = ref_d.download((m, H, W, 2), np.float32, offset=t0 * P * 8)
                diff = got != ref
                assert not diff.any(), (stats, heights, [t0 + int(t) for t in np.unique(np.argwhere(diff)[:, 0])][:8],
                                        int(diff.sum()), float(np.abs(got - ref).max()))
                want_sum += got.astype(np.float64).reshape(-1, 2).sum(0)
            slack = got_d.download((G.SLACK_BYTES,), np.uint8, offset=n * P * 8)
            assert (slack == 0xFF).all(), stats
            if stats:
                got_sum = sums_d.download((2,), np.float64)
                assert np.abs(got_sum - want_sum).max() <= G.SUM_BAR * max(1.0, np.abs(want_sum).max()), (got_sum, want_sum)
        # three pairs against the oracle
        worst = (0.0, 0.0)
        for t in G.anchor_pairs(n):
            a, b = frames.download((2, H, W), np.uint8, offset=t * P)
            got = got_d.download((H, W, 2), np.float32, offset=t * P * 8)
            want = _oracle_flow(name, kw, a, b, t)
            r, m = D.rel(got, want), float(np.abs(got - want).max())
            worst = (max(worst[0], r), max(worst[1], m))
            assert np.isfinite(got).all()
            assert r <= G.ANCHOR_REL and m <= G.ANCHOR_ABS, (t, r, m)
        print(f"{G.engine_run_id(name, n)}: (iteration, box, expansion) rows per level {heights}, against the oracle "
              f"rel {worst[0]:.3e} max|d| {worst[1]:.3e}")
    finally:
        big.close()
        small.close()
        for b in (frames, got_d, ref_d, sums_d):
            b.free()
