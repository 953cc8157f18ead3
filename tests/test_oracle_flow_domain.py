"""CPU side of test_gpu_flow_domain.py: every case of tests/flow_domain_cases.py is well-conditioned -- the oracle (OpenCV's
float32 / float64 mix) and a float64 numpy restatement of the same operation agree far inside the bar the GPU test applies
-- so that a case can fail on the GPU only because the kernels are wrong; the stage bars recorded in
golden/flow_domain_bars.json are current; and the tables cover what they claim to cover."""
import numpy as np
import pytest

import flow_domain_cases as D
from opticalflowclustering_amd import synth
from oracle import oracle as O
from test_oracle_farneback_independent import farneback_f64


@pytest.fixture(scope="module")
def measured():
    return D.measure_stage_distances()


def test_recorded_stage_distances_are_current(measured):
    """tests/golden/make_flow_domain_bars.py rewrites the fixture"""
    rec = D.recorded_stage_distances()
    assert set(rec) == set(measured)
    for k, v in measured.items():
        assert abs(rec[k] - v) <= 1e-6 * v + 1e-12, (k, rec[k], v)


def test_stage_tables_cover_every_window_seam_and_height():
    for cases, windows in ((D.ITER_CASES, D.ITER_WINDOWS), (D.BOX_CASES, D.BOX_WINDOWS)):
        for ws in windows:
            T = 256 - (ws - 1)
            mine = [(W, H) for w, _, W, H in cases if w == ws]
            assert {W for W, _ in mine} == {T - 1, T, T + 1, 2 * T, 2 * T + 1, 17}
            assert {H for _, H in mine} == set(D.HEIGHTS)


@pytest.mark.parametrize("ws", D.ITER_WINDOWS)
def test_fused_iteration_cases_are_well_conditioned(measured, ws):
    """float32 against float64 alone stays under the cap, 10 x the winsize-15 bar, on every case of this window"""
    for w, name, W, H in D.ITER_CASES:
        if w != ws:
            continue
        R0, R1, flow = D.iter_inputs(W, H, seed=W + ws)
        want = D.oracle_iterations(R0, R1, flow, max(D.ITER_COUNTS), ws)
        for it in D.ITER_COUNTS:
            d = measured[D.iter_case_id(ws, name, W, H, it)]
            bar, cap = D.stage_bar(D.iter_base_bar(it), d, want[it - 1])
            assert d <= cap, (name, W, H, it, d, cap)
            assert bar <= D.F32_FACTOR * cap


@pytest.mark.parametrize("ws", D.BOX_WINDOWS)
def test_box_solve_cases_are_well_conditioned(measured, ws):
    for w, name, W, H in D.BOX_CASES:
        if w != ws:
            continue
        d = measured[D.box_case_id(ws, name, W, H)]
        _, cap = D.stage_bar(D.BOX_BASE_BAR, d, D.oracle_box_solve(D.box_input(W, H), ws))
        assert d <= cap, (name, W, H, d, cap)


def test_level_image_cases_reach_every_launch_path_and_match_the_oracle_geometry():
    cases = D.level_cases()
    assert {c[0].rsplit("-", 1)[1] for c in cases} == set(D.LEVEL_PATHS)
    assert {c[1] for c in cases} >= {0.25, 0.3, 0.7, 0.8, 0.9}
    coarsest_32 = 0
    for ps, lv, W, H in D.LEVEL_FRAMES:
        po = D.oracle_params(dict(pyr_scale=ps, levels=lv))
        n = D.pyramid_levels(W, H, ps, lv)
        assert n == O.pyramid_levels(W, H, po)
        for k in range(n + 1):
            w, h, ksize, sigma = D.level_geometry(W, H, ps, k)
            assert (w, h, ksize) == O.level_geometry(W, H, k, po)[:3]
            assert ksize <= 31                          # the deepest blur the engine implements
        coarsest_32 += D.level_geometry(W, H, ps, n)[0] == 32
    assert coarsest_32 >= 1
    # both tiles of the general path on each side of sx = 2.5 within one pyramid
    for ps in (0.7, 0.8):
        tiles = {c[0].rsplit("-", 1)[1] for c in cases if c[1] == ps}
        assert {"general64x16", "general32x8"} <= tiles


def test_engine_table_covers_what_the_issue_lists():
    kws = [kw for _, kw, _, _ in D.ENGINE_CASES]
    sizes = {(W, H) for _, _, W, H in D.ENGINE_CASES}
    assert 40 <= len(D.ENGINE_CASES) <= 60 and len({c[0] for c in D.ENGINE_CASES}) == len(D.ENGINE_CASES)
    assert {kw["winsize"] for kw in kws} >= {5, 7, 9, 11, 13, 15, 17} and any(kw["winsize"] >= 19 for kw in kws)
    assert {kw["pyr_scale"] for kw in kws} >= {0.3, 0.5, 0.7, 0.8, 0.9}
    assert {kw["levels"] for kw in kws} >= {0, 1, 2, 3, 6, 16}
    assert {kw["iterations"] for kw in kws} >= {1, 2, 3, 4, 10, 64}
    assert any(kw["iterations"] == 1 and kw["levels"] >= 1 for kw in kws)
    assert {kw["poly_n"] for kw in kws} == {5, 7} and {kw["poly_sigma"] for kw in kws} >= {0.0, 1.1, 1.2, 1.5}
    assert sizes >= {(16, 16), (16, 300), (300, 16), (64, 64), (63, 65), (65, 63), (243, 131), (500, 300), (1921, 1081)}
    # levels=16 is clamped by the 32-pixel rule; every upsample variant of the first iteration is reached by a fused window
    assert any(kw["levels"] == 16 and D.pyramid_levels(W, H, kw["pyr_scale"], 16) < 16 for _, kw, W, H in D.ENGINE_CASES)
    ups = set()
    for _, kw, W, H in D.ENGINE_CASES:
        if kw["winsize"] <= 15:
            n = D.pyramid_levels(W, H, kw["pyr_scale"], kw["levels"])
            ups.add(0)
            for k in range(n):
                (w, h), (cw, ch) = D.level_geometry(W, H, kw["pyr_scale"], k)[:2], D.level_geometry(W, H, kw["pyr_scale"], k + 1)[:2]
                ups.add(2 if (cw / w == 0.5 and ch / h == 0.5) else 1)          # launch_flow_iter's choice
    assert ups == {0, 1, 2}
    assert len(D.ENGINE_BATCHED) == 5 and all(D.engine_case(n)[1] != D.DEFAULTS for n in D.ENGINE_BATCHED)


@pytest.mark.parametrize("name,kw,W,H", D.ENGINE_CASES, ids=[c[0] for c in D.ENGINE_CASES])
def test_engine_cases_are_well_conditioned(name, kw, W, H):
    """oracle against the independent float64 Farneback: rel <= 1e-5 and max|d| <= 2e-4 px, a fifth of the GPU bar"""
    a, b = synth.translated_pair(W, H, *D.ENGINE_MOTION)
    got = O.farneback(a, b, D.oracle_params(kw)).astype(np.float64)
    ref = farneback_f64(a, b, **kw)
    assert D.rel(got, ref) <= 1e-5, D.rel(got, ref)
    assert np.abs(got - ref).max() <= 2e-4, np.abs(got - ref).max()
