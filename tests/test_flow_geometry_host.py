"""CPU side of test_gpu_flow_geometry.py.  The tables of tests/flow_geometry_cases.py are checked against the C cost models
themselves (ofc_flow_launch_geometry, which touches no device) and not against a restatement of them: they reach every
class of strip height and strip count named below, and every class the bench's own batches run at 1080p, so a retuned
model fails here instead of quietly shrinking what the GPU test covers.  And the stage inputs are fit for a bit-for-bit
demand: on them the f64 window sums the kernels carry down a strip do not depend on the order of summation, so two strip
heights can differ only if the kernel is wrong."""
import numpy as np
import pytest

import flow_domain_cases as D
import flow_geometry_cases as G
from oracle import oracle as O


@pytest.fixture(scope="module")
def geometry():
    from opticalflowclustering_amd import stages
    return stages.flow_launch_geometry


def _engine_rows(geometry, which):
    """[(case, n pairs, level, (w, h), rows)] over the engine table: what model `which` (0 fused iteration, 1 box mean +
    solve, 2 expansion) picks, for the cases that run that kernel"""
    out = []
    for name, kw, W, H, pairs in G.ENGINE_CASES:
        if (which == 0 and kw["winsize"] > 15) or (which == 1 and kw["winsize"] != 17):
            continue
        for n in pairs:
            for k, (w, h) in enumerate(G.engine_levels(W, H, kw)):
                out.append((name, n, k, (w, h), geometry(w, h, n, kw["winsize"])[which]))
    return out


def _fused_classes(geometry, winsize=None):
    """{(height class, strip-count class): an example} over the stage table and the fused cases of the engine table (at
    one window, or at all of them)"""
    seen = {}
    for ws, W, H in G.STAGE_CASES:
        for rows in G.stage_rows(H) if winsize in (None, ws) else ():
            rows = G.cdiv(rows, G.SUPER_STEP) * G.SUPER_STEP
            seen.setdefault(G.geometry_class(rows, H), f"stage ws{ws} {W}x{H} rows {rows}")
    for name, n, k, (w, h), rows in _engine_rows(geometry, 0):
        if winsize in (None, dict((c[0], c[1]) for c in G.ENGINE_CASES)[name]["winsize"]):
            seen.setdefault(G.geometry_class(rows, h), f"engine {name} {n} pairs level {k} {w}x{h} rows {rows}")
    return seen


def test_hook_answers_without_a_device_and_refuses_bad_arguments(geometry):
    import ctypes as C
    from opticalflowclustering_amd import _lib
    for W, H, n, ws in ((16, 16, 1, 5), (250, 190, 22, 15), (1920, 1080, 64, 15), (3840, 2160, 32, 15), (500, 300, 171, 17)):
        it, box, pe = geometry(W, H, n, ws)
        assert it % G.SUPER_STEP == 0 and G.SUPER_STEP <= it <= G.cdiv(H, G.SUPER_STEP) * G.SUPER_STEP if ws <= 15 else it == 0
        assert box in (16, 32, 64, 128) and pe in (4, 8, 16), (box, pe)
    assert geometry(500, 300, 8, 31)[0] == 0            # a wide window runs staged, at k_box_solve_wide's fixed height
    assert geometry(500, 300, 8, 31)[1] == geometry(64, 64, 300, 31)[1]
    out = (C.c_int * 3)()
    for W, H, n, ws in ((0, 16, 1, 15), (16, 0, 1, 15), (16, 16, 0, 15), (16, 16, 1, 14), (16, 16, 1, 3), (16, 16, 1, 257)):
        assert _lib.load().ofc_flow_launch_geometry(W, H, n, ws, out) == _lib.OFC_EINVAL, (W, H, n, ws)
    assert _lib.load().ofc_flow_launch_geometry(16, 16, 1, 15, None) == _lib.OFC_EINVAL


def test_engine_levels_are_the_oracles(geometry):
    for name, kw, W, H, _ in G.ENGINE_CASES:
        po = D.oracle_params(kw)
        lv = G.engine_levels(W, H, kw)
        assert len(lv) == O.pyramid_levels(W, H, po) + 1 >= 3, name
        for k, wh in enumerate(lv):
            assert wh == tuple(O.level_geometry(W, H, k, po)[:2])


def test_reference_batch_runs_the_geometry_the_rest_of_the_suite_anchors(geometry):
    """three pairs at a time: 16-row strips of the iteration (fused or staged) and 8-row strips of the expansion, at every
    level of every engine case"""
    for name, kw, W, H, _ in G.ENGINE_CASES:
        for w, h in G.engine_levels(W, H, kw):
            for n in range(1, G.REF_BATCH + 1):
                it, box, pe = geometry(w, h, n, kw["winsize"])
                assert (it if kw["winsize"] <= 15 else box) == 16 and pe == 8, (name, w, h, n, it, box, pe)


def test_tables_reach_every_class_of_the_fused_iteration(geometry):
    seen = _fused_classes(geometry)
    for cls, ex in sorted(seen.items()):
        print(cls, "<-", ex)
    assert {s for _, s in seen} >= {"1", "2", "3+partial"}
    assert {h for h, _ in seen} == set(G.HEIGHT_CLASSES)
    # the engine table alone (whole pyramids, the upsample forms, the batch's pair map) reaches them as well
    eng = {G.geometry_class(rows, h) for _, _, _, (_, h), rows in _engine_rows(geometry, 0)}
    assert {s for _, s in eng} >= {"1", "2", "3+partial"} and {h for h, _ in eng} == set(G.HEIGHT_CLASSES), sorted(eng)
    # the x2 upsample form (a level that is exactly half of the next finer one) marches more than one super-step too
    ups2 = 0
    for name, kw, W, H, pairs in G.ENGINE_CASES:
        lv = G.engine_levels(W, H, kw)
        for n in pairs:
            for k in range(len(lv) - 1):
                rows = geometry(*lv[k], n, kw["winsize"])[0]
                ups2 += kw["winsize"] <= 15 and lv[k] == (2 * lv[k + 1][0], 2 * lv[k + 1][1]) and rows >= 64
    assert ups2 >= 3, ups2


def test_stage_table_is_what_the_issue_lists():
    assert {ws for ws, _, _ in G.STAGE_CASES} == set(D.ITER_WINDOWS)
    for ws in D.ITER_WINDOWS:
        assert {(W, H) for w, W, H in G.STAGE_CASES if w == ws} >= {(D.tile_width(ws) + 1, H) for H in G.STAGE_HEIGHTS}
    assert G.STAGE_HEIGHTS == (190, 77, 48) and G.STAGE_ITERS == (1, 3)
    for _, _, H in G.STAGE_CASES:
        rows, single = G.stage_rows(H), G.cdiv(H, 16) * 16
        assert set(range(16, single + 1, 16)) <= set(rows) and max(rows) > max(H, single)
    assert len({G.stage_case_id(*c, it) for c in G.STAGE_CASES for it in G.STAGE_ITERS}) == 2 * len(G.STAGE_CASES)
    assert not set(G.recorded_stage_distances()) & set(D.recorded_stage_distances())


def test_engine_table_reaches_every_box_and_expansion_height(geometry):
    box = _engine_rows(geometry, 1)
    for name, n, k, wh, rows in box:
        print(f"{name} {n} pairs level {k} {wh}: box rows {rows}")
    assert {r for *_, r in box} == {16, 32, 64, 128}
    assert {r for _, _, k, _, r in box if k == 0} == {16, 32, 64, 128}
    # the expansion at both of its heights on ONE shape (level 0 of the poly_n 7 case), and on the default poly_n 5 as well
    for poly_n in (5, 7):
        per_shape = {}
        for name, kw, W, H, pairs in G.ENGINE_CASES:
            if kw["poly_n"] == poly_n:
                for n in pairs:
                    per_shape.setdefault((name, W, H), set()).add(geometry(W, H, n, kw["winsize"])[2])
        assert any(v == {8, 16} for v in per_shape.values()), (poly_n, per_shape)


def test_every_geometry_the_bench_runs_is_represented(geometry):
    """the (strip height class, strip count class) of every level of every batch bench.py cuts its clip into, at the bench's
    own window"""
    import bench
    from opticalflowclustering_amd.pipeline import batch_schedule
    n_pairs = bench.CLIP_FRAMES - 1
    schedule = batch_schedule(n_pairs, bench.auto_batch(n_pairs))
    assert sum(schedule) == n_pairs and len(set(schedule)) >= 2        # a short first batch and the full ones
    seen = _fused_classes(geometry, D.DEFAULTS["winsize"])
    for n in sorted(set(schedule)):
        for k, (w, h) in enumerate(G.engine_levels(bench.W, bench.H, D.DEFAULTS)):
            rows = geometry(w, h, n, D.DEFAULTS["winsize"])[0]
            cls = G.geometry_class(rows, h)
            print(f"bench batch of {n} pairs, level {k} {w}x{h}: rows {rows} x {G.cdiv(h, rows)} strips -> {cls}: "
                  f"{seen.get(cls, 'NOT COVERED')}")
            assert cls in seen, (n, k, rows, cls)


# ---- the 16-row run's oracle bars ----
@pytest.fixture(scope="module")
def measured():
    return G.measure_stage_distances()


def test_recorded_stage_distances_are_current_and_the_cases_well_conditioned(measured):
    """tests/golden/make_flow_geometry_bars.py rewrites the fixture; float32 against float64 alone stays under
    flow_domain_cases' cap (10 x the winsize-15 bar) on every case"""
    rec = G.recorded_stage_distances()
    assert set(rec) == set(measured)
    for k, v in measured.items():
        assert abs(rec[k] - v) <= 1e-6 * v + 1e-12, (k, rec[k], v)
    for ws, W, H in G.STAGE_CASES:
        R0, R1, flow = G.stage_inputs(ws, W, H)
        want = D.oracle_iterations(R0, R1, flow, max(G.STAGE_ITERS), ws)
        for it in G.STAGE_ITERS:
            d = measured[G.stage_case_id(ws, W, H, it)]
            bar, cap = D.stage_bar(D.iter_base_bar(it), d, want[it - 1])
            assert d <= cap and bar <= D.F32_FACTOR * cap, (ws, W, H, it, d, cap)


# ---- the precondition of bit equality across strip heights ----
@pytest.mark.parametrize("ws,W,H", G.STAGE_CASES, ids=[f"ws{c[0]}-{c[1]}x{c[2]}" for c in G.STAGE_CASES])
def test_window_sums_of_the_stage_inputs_do_not_depend_on_the_order(ws, W, H):
    """A strip of k_flow_iter sums its first window top to bottom and then runs + new row - old row in f64; where a strip
    begins decides which of the two a given row gets.  On these inputs both give the same bits as a fresh sum in reverse
    order, for every pixel, channel and iteration (the f64 sums of these float32 entries are exact), so the flow cannot
    legitimately depend on the strip height: a difference in test_gpu_flow_geometry.py is the kernel's."""
    R0, R1, flow = G.stage_inputs(ws, W, H)
    M = O.update_matrices(R0, R1, flow)
    for i in range(max(G.STAGE_ITERS)):
        running = G.window_sums_running(M, ws // 2)
        for reverse in (True, False):
            fresh = G.window_sums_fresh(M, ws // 2, reverse)
            assert np.isfinite(fresh).all()
            differing = int((running != fresh).sum())
            assert differing == 0, (i, reverse, differing, np.abs(running - fresh).max())
        flow, M = O.update_flow_blur(R0, R1, flow, M, ws, True)
