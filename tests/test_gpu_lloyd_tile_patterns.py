"""The tile sweeps (csrc/lloyd_tiles.hip) and the mode rules of k_lloyd_update at every walk pattern, mode switch, k and edge
input of lloyd_tile_cases.py.  The reference of every fit is the CPU oracle (pinned by test_oracle_lloyd_independent.py)
under the bars of test_gpu_lloyd_tiles.same_fit; test_oracle_lloyd_tiles.py proves that no case has a borderline tile, so
the `tested` / `pure` counts and the mode of every sweep -- read from the OFC_LLOYD_TRACE line and from prune_stats() --
must equal the float64 model's exactly.

Measured on an MI355X in one run: this module 2.5 s (98 tests), test_gpu_lloyd_tiles.py 2.2 s (26 tests).
"""
import os
import re

import numpy as np
import pytest

import lloyd_tile_cases as T
from lloyd_tile_cases import PRUNED
from test_gpu_lloyd_tiles import fit, same_fit

pytestmark = pytest.mark.gpu
ZE = np.load(os.path.join(os.path.dirname(__file__), "golden", "lloyd_edge_goldens.npz"))
TRACE = re.compile(r"\[ofc lloyd\] it (\d+) tiles_mode (-?\d+) tested (\d+) pure (\d+) ")


def traced_fit(X, C0, policy, monkeypatch, capfd, **kw):
    """-> fitted KMeans, prune_stats(), [(tiles_mode, tested, pure)] per iteration from the library's trace line"""
    monkeypatch.setenv("OFC_LLOYD_PRUNE", str(policy))
    monkeypatch.setenv("OFC_LLOYD_TRACE", "1")
    capfd.readouterr()
    km, st = fit(X, C0, **kw)
    rows = [tuple(int(v) for v in m.groups()) for m in TRACE.finditer(capfd.readouterr().err)]
    assert [r[0] for r in rows] == list(range(len(rows)))
    return km, st, [r[1:] for r in rows]


def run_case(name, policy, monkeypatch, capfd):
    """fit a case of the table and hold it to the oracle and to the model's account of every sweep"""
    c, ex = T.CASES[name], T.expect(name)
    plan = ex.plan(policy)
    km, st, rows = traced_fit(ex.X, ex.C0, policy, monkeypatch, capfd, max_iter=c.get("max_iter", 300), tol=c.get("tol", 1e-4))
    same_fit(km, ex.cen, ex.lab, ex.inertia, ex.n_iter)
    assert rows == plan.trace()
    assert st["tile_sweeps"] == ex.n_iter and st["final_pruned"] == plan.final_pruned, st
    assert st["pruned_sweeps"] == plan.pruned_sweeps and st["probe_sweeps"] == plan.probe_sweeps, st
    assert st["tiles_tested"] == ex.NT * plan.pruned_sweeps, st
    assert st["tiles_pure"] == sum(p for m, p in zip(plan.modes, ex.pure) if m == PRUNED), st
    return km, st


def unpruned(name, monkeypatch):
    c, ex = T.CASES[name], T.expect(name)
    monkeypatch.setenv("OFC_LLOYD_PRUNE", "0")
    km, st = fit(ex.X, ex.C0, max_iter=c.get("max_iter", 300), tol=c.get("tol", 1e-4))
    assert st["tile_sweeps"] == 0
    same_fit(km, ex.cen, ex.lab, ex.inertia, ex.n_iter)
    return km


# ------------------------------------------------------------------------------------------------ A. walk patterns
@pytest.mark.parametrize("name", T.WALK_CASES)
def test_walk_patterns(name, monkeypatch, capfd):
    """1..64 rejected tiles of a 64-tile group on the first, last, alternating and random lanes, groups of 0, 1, 2 and 63
    tiles and 0, 1 and 63 samples at the field's end: iteration 0, iteration 1 and the final E-step all run pruned and
    walk exactly the designed tiles; the labels localise a wrong row -> tile mapping to the tile"""
    km, st = run_case(name, 3, monkeypatch, capfd)
    assert st["final_pruned"] and st["pruned_sweeps"] == km.n_iter_
    rej = T.walk_rejected(name)
    assert st["tiles_pure"] == km.n_iter_ * int((~rej).sum())
    assert np.abs(km.cluster_centers_ - unpruned(name, monkeypatch).cluster_centers_).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ B. mode switches
@pytest.mark.parametrize("name", T.SWITCH_CASES)
def test_mode_switches(name, monkeypatch, capfd):
    """PRUNED -> FULL x 6 -> PROBE -> PRUNED, the same fit cut by max_iter in its FULL stretch, on its PROBE and in the PRUNED
    stretch behind it, and PRUNED -> FULL x 6 -> PROBE -> FULL x 12 -> PROBE: the records of pruned, full and counting
    sweeps mix in one fit, which must stop in the oracle's iteration and take its final E-step's form from the last status"""
    km, st = run_case(name, 2, monkeypatch, capfd)
    assert st["probe_sweeps"] >= 1 or name == "switch-recover-cut-full"
    if "cut" not in name:
        assert np.abs(km.cluster_centers_ - unpruned(name, monkeypatch).cluster_centers_).max() <= 1e-12


def test_mode_switches_in_a_loopback_world(monkeypatch, capfd):
    """two emulated ranks with the same shard: the all-reduced tile counts are doubled, the shares and so the sequence are
    not; sums and counts double exactly, so the centres are the single rank's and the inertia twice its"""
    from opticalflowclustering_amd._lib import check, load
    ex = T.expect("switch-recover")
    plan = ex.plan(2)
    check(load().ofc_dist_loopback(2))
    try:
        km, st, rows = traced_fit(ex.X, ex.C0, 2, monkeypatch, capfd, tol=0.0)
    finally:
        check(load().ofc_dist_loopback(1))
    same_fit(km, ex.cen, ex.lab, 2.0 * ex.inertia, ex.n_iter)
    assert rows == plan.trace(world=2)
    assert st["probe_sweeps"] == 1 and st["pruned_sweeps"] == plan.pruned_sweeps and st["final_pruned"], st


# ------------------------------------------------------------------------------------------------ C. every k
@pytest.mark.parametrize("policy", [2, 3])
@pytest.mark.parametrize("name", T.K_CASES)
def test_every_k(name, policy, monkeypatch, capfd):
    km, st = run_case(name, policy, monkeypatch, capfd)
    assert st["final_pruned"] and 0.5 < st["skip_fraction"] <= 1.0
    if name == "k1":                  # every tile passes: no sample is read after k_tile_meta, the inertia is all tsq
        assert st["skip_fraction"] == 1.0


# ------------------------------------------------------------------------------------------------ D. edge inputs
@pytest.mark.parametrize("policy", [2, 3])
@pytest.mark.parametrize("name", T.golden_tile_cases(ZE))
def test_edge_goldens_with_tile_sweeps(name, policy, monkeypatch):
    """every case of lloyd_edge_goldens.npz the tile sweeps accept: max_iter cuts and stops on the window boundaries,
    k = 1, 2, 8, duplicate initial rows (an empty cluster at iteration 0), a tol that stops at once"""
    monkeypatch.setenv("OFC_LLOYD_PRUNE", str(policy))
    X, C0 = ZE[name + "/X"], ZE[name + "/C0"]
    km, st = fit(X, C0, max_iter=int(ZE[name + "/max_iter"]), tol=float(ZE[name + "/tol"]))
    same_fit(km, ZE[name + "/centers"], ZE[name + "/labels"], float(ZE[name + "/inertia"]), int(ZE[name + "/n_iter"]))
    assert st["tile_sweeps"] >= 1 or name == "tie_dupC0_f32_k3"        # (stalls on its empty cluster at iteration 0)


@pytest.mark.parametrize("policy", [2, 3])
@pytest.mark.parametrize("name", [n for n in T.EDGE_CASES if n != "const-k2"])
def test_built_edge_inputs(name, policy, monkeypatch, capfd):
    """whole tiles of exactly tied samples (never counted pure: the trace's count is the untied tiles'), boxes of zero
    extent, constant data, an offset of 1e4 with spread 1e-2"""
    km, st = run_case(name, policy, monkeypatch, capfd)
    if name == "tie":
        assert st["tiles_pure"] == int((~T.tied_tiles(T.expect(name).X)).sum()) and st["final_pruned"]


@pytest.mark.parametrize("policy", [2, 3])
def test_constant_field_with_an_empty_cluster(policy, monkeypatch, capfd):
    """k = 2 on constant data: iteration 0's tile sweep meets the empty cluster (its status carries no tile counts) and the
    fit goes on labelled, relocating as sklearn does"""
    ex = T.expect("const-k2")
    km, st, rows = traced_fit(ex.X, ex.C0, policy, monkeypatch, capfd)
    same_fit(km, ex.cen, ex.lab, ex.inertia, ex.n_iter)
    assert rows[0] == (-1, 0, 0) and not st["final_pruned"]


# ------------------------------------------------------------------------------------------------ E. non-finite samples
def same_where_it_can_be(a, b):
    """centres of an unpruned and a pruned fit of a field with a non-finite sample: the poisoned coordinates hold the same
    non-finite value, the others meet the pruned-against-unpruned bar (the two paths sum in different orders, so they are
    not bit-equal: measured 2.2e-16 to 1.3e-15 on these fields)"""
    fin = np.isfinite(a)
    print("finite coordinates:", int(fin.sum()), "largest difference:", np.abs(a[fin] - b[fin]).max() if fin.any() else 0.0)
    assert not fin.all() and np.array_equal(fin, np.isfinite(b))
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True)
    assert not fin.any() or np.abs(a[fin] - b[fin]).max() <= 1e-12


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_sample_with_a_finite_mean(bad, monkeypatch):
    """sklearn refuses such input, so there is no reference: the requirement is that the pruned path returns what the
    unpruned kernels return.  The column sums are handed in by the caller (as the flow engine does), here those of the
    field with the bad sample zeroed: the mean and the centres stay finite and only the one tile is poisoned -- its box
    must fail the test (NaN sums: k_tile_meta empties the box; an infinite corner: mag is infinite), so that its samples
    are labelled one by one as the unpruned kernels label them.  (Through KMeans.fit the sample poisons the column mean
    and with it every centred sample: all labels are 0 on either path and the tile test decides nothing.)"""
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.cluster import kmeans_fit_dev, prune_stats
    X, C0 = T.nan_field(bad)
    colsum = np.where(np.isfinite(X), X, 0).astype(np.float64).sum(0)
    buf = _lib.DeviceBuffer(X.nbytes, 0).upload(X)
    lab = _lib.DeviceBuffer(len(X), 0)
    out = []
    for policy in (0, 3):
        monkeypatch.setenv("OFC_LLOYD_PRUNE", str(policy))
        cen, inertia, n_iter = kmeans_fit_dev(buf.ptr, _lib.F32, len(X), 2, C0, max_iter=1, labels_ptr=lab.ptr, colsum=colsum)
        st = prune_stats()
        out.append((cen, lab.download((len(X),), np.uint8).copy(), n_iter))
        if policy == 3:
            assert st["pruned_sweeps"] == 1 and 0 < st["tiles_pure"] < st["tiles_tested"] == len(X) // 64, st
    buf.free()
    lab.free()
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert np.isfinite(out[0][0]).sum() == 3          # one centre coordinate is poisoned, the fit is not
    same_where_it_can_be(out[0][0], out[1][0])
