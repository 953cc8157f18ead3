"""CPU proof that the cases of lloyd_tile_cases.py are what they claim to be, so that test_gpu_lloyd_tile_patterns.py may
hold the tile sweeps (csrc/lloyd_tiles.hip, k_lloyd_update's mode rules) to exact counts and mode sequences.

Conditions on every case (conditions, not measurements -- a case that loses one is changed, never the bar):
  * no borderline tile in any sweep or in the final E-step: the box verdict is the same for every margin factor in
    [1e-13, 1e-11], so the device's `pure` count must equal the model's whatever its last bits are;
  * every pure share that feeds a mode decision is at least 0.05 away from the threshold it is compared with (0.45 for the
    probe before iteration 0 and for a PROBE sweep, 0.30 for a PRUNED sweep);
  * every sample that is not an exact, designed tie keeps the argmin gap test_oracle_lloyd_independent.py requires of the
    expanded distance form, against the centres of every sweep and the final ones.
The mode sequences, walk patterns and ties are asserted as designed, and the model's constants are checked against the
kernel sources.

Wall time of this file: 13 s on one CPU thread (measured), most of it the oracle fits cut after 1, 2, ... iterations.
"""
import os
import re

import numpy as np
import pytest

import lloyd_tile_cases as T
from lloyd_tile_cases import FULL, PROBE, PRUNED

CSRC = os.path.join(os.path.dirname(__file__), "..", "opticalflowclustering_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ the model itself
def test_model_constants_are_the_kernels():
    tiles, kern, api = src("lloyd_tiles.hip"), src("lloyd_kernels.hip"), src("lloyd_fit.cpp")
    assert "wmax < -1e-12 * mag" in tiles
    assert "pure >= 0.45 * tested" in tiles
    assert "if (frac < 0.3)" in kern and "frac >= 0.45 ? LLOYD_TILES_PRUNED : LLOYD_TILES_FULL" in kern
    assert "st->prune_cooldown = st->prune_backoff = 6;" in kern and kern.count("st->prune_backoff *= 2;") == 2
    assert re.search(r"LLOYD_TILES_FULL = 0,.*\n\s*LLOYD_TILES_PRUNED = 1,.*\n\s*LLOYD_TILES_PROBE = 2", src("lloyd_common.h"))
    assert (FULL, PRUNED, PROBE) == (0, 1, 2)
    # the line the GPU module parses ("What holds the tile sweeps")
    assert '"[ofc lloyd] it %d tiles_mode %d tested %.0f pure %.0f shift %.3e empty %d\\n"' in api


def test_box_model_on_hand_made_tiles():
    cc = np.array([[-1.0, 0.0], [1.0, 0.0]])
    lo = np.array([[0.5, -3.0], [-2.0, -1.0], [-0.5, 0.0], [0.0, -1.0], [1e-13, 0.0], [1e-9, 0.0]])
    hi = np.array([[2.0, 3.0], [-0.1, 1.0], [0.5, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 0.0]])
    j, pure = T.box_verdict(lo, hi, np.zeros(2), cc)
    assert list(j) == [1, 0, 0, 0, 1, 1]
    # inside cell 1, inside cell 0, across the edge, ON the edge (wmax == 0: rejected, label = first minimum),
    # closer to the edge than the margin (mag = 2 + 8 ax: 1e-12 * 10 against 4e-13), clear of it
    assert list(pure) == [True, True, False, False, False, True]
    assert T.box_verdict(lo, hi, np.zeros(2), cc[:1])[1].all()                    # k = 1: every tile passes
    assert not T.box_verdict(lo, hi, np.zeros(2), cc[[0, 0, 1]])[1][[1, 2, 3]].any()    # a duplicate of the candidate: tie
    X = np.zeros((130, 2), np.float32)
    X[:64, 0], X[64:128, 0], X[128:] = 1.0, np.linspace(-1, 1, 64), 50.0
    pure, borderline = T.tile_report(X, np.zeros(2), cc)
    assert list(pure) == [True, False] and borderline == 0                        # the samples behind the last tile: no box
    X[0, 0] = 2e-12                                                               # wmax = -8e-12, mag = 10: inside the band
    assert T.tile_report(X, np.zeros(2), cc)[1] == 1


def test_replay_follows_the_update_rules():
    NT = 100
    modes, final, fed = T.replay(2, [60] * 3 + [20] + [10] * 6 + [50] + [60] * 2, NT)
    assert "".join("FPB"[m] for m in modes) == "PPPP" + "F" * 6 + "B" + "PP" and final
    assert fed[0] == (0.6, 0.45) and fed[4] == (0.2, 0.30) and fed[5] == (0.5, 0.45)      # FULL sweeps feed nothing
    modes, final, _ = T.replay(2, [60, 20] + [10] * 6 + [40] + [10] * 12 + [44] + [10] * 24 + [45, 46], NT)
    assert "".join("FPB"[m] for m in modes) == "PP" + "F" * 6 + "B" + "F" * 12 + "B" + "F" * 24 + "BP" and final
    modes, final, fed = T.replay(2, [44] + [90] * 40, NT)          # the probe before iteration 0 turns the policy off for good
    assert set(modes) == {FULL} and not final and fed == [(0.44, 0.45)]
    modes, final, fed = T.replay(3, [0] * 9, NT)
    assert set(modes) == {PRUNED} and final and fed == []
    assert T.replay(2, [60, 20], NT)[1] is False and T.replay(2, [60, 20] + [0] * 6, NT)[0][-1] == FULL
    assert T.replay(2, [60, 20] + [0] * 7, NT)[0][-1] == PROBE


def test_no_field_is_above_the_size_cap():
    assert max(len(T.field(CASES_BASE(n))[0]) for n in T.CASES) <= 64 * 4096


def CASES_BASE(n):
    return T.CASES[n].get("base", n)


# ------------------------------------------------------------------------------------------------ conditions on every case
def tied_samples(name, ex):
    if name == "tie":
        return np.repeat(T.tied_tiles(ex.X), T.TILE)
    if name == "const-k2":            # the relocated centre lands on the one point there is: both centres equal it
        return np.ones(len(ex.X), bool)
    return None


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_conditions(name):
    ex = T.expect(name)
    assert ex.borderline == 0
    for policy in (2, 3):
        assert ex.plan(policy).margins_ok(), ex.plan(policy).fed
    # the probe before iteration 0 (k_tile_probe) tests every tile: its stride is 1 while a step of 4 tiles per wave
    # covers the field, which replay() relies on
    nblocks = max(1, min(-(-(len(ex.X) // 4) // 256), 1024))
    assert (ex.NT + 3) // 4 <= 4 * min(nblocks, 256)
    tied = tied_samples(name, ex)
    for cen in ex.centres + [ex.cen]:
        ok, ratio = T.argmin_gap_ok(ex.X, ex.mean, cen - ex.mean, tied)
        assert ok, ratio
    if T.CASES[name].get("max_iter"):
        assert ex.n_iter == T.CASES[name]["max_iter"]
    elif name != "const-k2":
        assert np.bincount(ex.lab, minlength=len(ex.C0)).min() > 0


# ------------------------------------------------------------------------------------------------ A. walk patterns
@pytest.mark.parametrize("name", T.WALK_CASES)
def test_walk_case_is_as_designed(name):
    a = T.CASES[name]["args"]
    ex, rej = T.expect(name), T.walk_rejected(name)
    groups = rej[: 64 * len(T.REJECTED_COUNTS)].reshape(-1, 64)
    counts = T.REJECTED_COUNTS[::-1] if a["reverse"] else T.REJECTED_COUNTS
    assert tuple(groups.sum(1)) == counts
    for g, c in zip(groups, counts):
        lanes = np.flatnonzero(g)
        if a["placement"] == "first":
            assert list(lanes) == list(range(c))
        elif a["placement"] == "last":
            assert list(lanes) == list(range(64 - c, 64))
        elif a["placement"] == "alternating" and 0 < c <= 32:
            assert lanes[0] == 0 and (np.diff(lanes) == 2).all()
        elif a["placement"] == "alternating" and 32 < c < 64:
            assert (np.diff(np.flatnonzero(~g)) == 2).all() and not g[1]
    assert ex.NT == len(rej) and ex.NT % 64 == a["extra_tiles"] and len(ex.X) % 64 == a["extra_samples"]
    assert a["extra_tiles"] == 0 or rej[-1]                       # the field ends on a tile that is walked
    # every sweep and the final E-step see exactly the designed tiles as pure
    assert ex.n_iter >= 2 and len(ex.pure_masks) == ex.n_iter
    for m in ex.pure_masks:
        assert np.array_equal(m, ~rej)
    assert ex.final_pure == int((~rej).sum())
    # a rejected tile holds both populations, in splits that include 1/63 and 63/1; a pure one holds one
    per_tile = (ex.X[: ex.NT * 64, 0] < 0).reshape(-1, 64).sum(1)
    assert set(per_tile[~rej]) == {0, 64} and {1, 63} <= set(per_tile[rej]) and not {0, 64} & set(per_tile[rej])
    assert ex.plan(3).letters() == "P" * ex.n_iter and ex.plan(3).final_pruned


def test_walk_cases_cover_every_field_end():
    args = [T.CASES[n]["args"] for n in T.WALK_CASES]
    assert {(a["placement"], a["reverse"]) for a in args} == {(p, r) for p in T.PLACEMENTS for r in (False, True)}
    assert {1, 63} <= {a["extra_tiles"] % 64 for a in args} and {1, 2, 3} <= {a["extra_tiles"] % 4 for a in args}
    assert {0, 1, 63} <= {a["extra_samples"] for a in args}
    assert T.REJECTED_COUNTS == (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)


# ------------------------------------------------------------------------------------------------ B. mode switches
SEQUENCES = {"switch-recover": ("P" * 12 + "F" * 6 + "B" + "P" * 9, True),
             "switch-recover-cut-full": ("P" * 12 + "F" * 3, False),
             "switch-recover-cut-probe": ("P" * 12 + "F" * 6 + "B", True),
             "switch-recover-cut-pruned": ("P" * 12 + "F" * 6 + "B" + "P" * 3, True),
             "switch-stay-full": ("P" * 8 + "F" * 6 + "B" + "F" * 12 + "B", False)}


@pytest.mark.parametrize("name", T.SWITCH_CASES)
def test_switch_case_keeps_its_transitions(name):
    ex = T.expect(name)
    plan = ex.plan(2)
    assert (plan.letters(), plan.final_pruned) == SEQUENCES[name]
    assert len(plan.letters()) == ex.n_iter <= 40
    assert plan.probe_sweeps == SEQUENCES[name][0].count("B") and plan.pruned_sweeps == SEQUENCES[name][0].count("P")
    # with tol = 0 the fit stops on equal labels; the stop must not coincide with a change of the sweep's form, which
    # alone would move the sums by an ulp (a cut fit does not stop)
    if "cut" not in name:
        assert np.array_equal(ex.pure_masks[-1], ex.pure_masks[-2])
        assert plan.modes[-2] != PRUNED or plan.modes[-1] == PRUNED


# ------------------------------------------------------------------------------------------------ C. every k
@pytest.mark.parametrize("name", T.K_CASES)
def test_k_case(name):
    ex = T.expect(name)
    k = T.CASES[name]["args"]["k"]
    assert len(ex.C0) == k and len(ex.X) == 64 * 600 + 37 and ex.n_iter >= 2
    # no cluster is empty at any iteration (the fit would leave the tile sweeps for the labelled ones)
    assert min(np.bincount(T._cut_fit(name, i)[1], minlength=k).min() for i in range(1, ex.n_iter + 1)) > 0
    for policy in (2, 3):
        assert set(ex.plan(policy).modes) == {PRUNED} and ex.plan(policy).final_pruned
    if k == 1:
        assert ex.pure == [ex.NT] * ex.n_iter and ex.final_pure == ex.NT
    else:
        assert 0.5 * ex.NT < min(ex.pure) and max(ex.pure) < ex.NT          # both kinds of tile in every sweep


# ------------------------------------------------------------------------------------------------ D. edge inputs
def test_tie_case_is_exactly_tied():
    ex = T.expect("tie")
    X = ex.X.astype(np.float64)
    assert np.array_equal(X, np.round(X)) and np.array_equal(ex.mean, [0.0, 0.0])
    tied = np.repeat(T.tied_tiles(ex.X), 64)
    assert tied.sum() == 64 * 40
    for cen in (ex.C0, ex.cen):                                    # integers: exact in float64, in any order
        assert np.array_equal(cen, [[-4.0, 0.0], [4.0, 0.0]])
        d = ((X[:, None, :] - cen[None]) ** 2).sum(2)
        assert np.array_equal(d[:, 0] == d[:, 1], tied)
    assert ex.n_iter == 1 and not ex.lab[tied].any()               # the first minimum
    assert not ex.pure_masks[0][T.tied_tiles(ex.X)].any() and ex.pure_masks[0][~T.tied_tiles(ex.X)].all()
    lo, hi = T.tile_boxes(ex.X)
    assert np.array_equal(lo[:, 0], hi[:, 0])                      # zero extent in u, every tile


def test_constant_and_offset_cases():
    for name in ("const-k1", "const-k2"):
        lo, hi = T.tile_boxes(T.expect(name).X)
        assert np.array_equal(lo, hi)
    assert T.expect("const-k1").pure == [40]
    assert T.expect("const-k2").pure[0] == 40                      # before the empty cluster is met: (3.5, -1.25) is centre 0
    ex = T.expect("offset1e4")
    assert np.abs(np.abs(ex.X) - 1e4).max() < 0.5 and np.abs(ex.X - ex.cen[ex.lab]).max() < 0.06
    assert 0 < min(ex.pure) < ex.NT


def test_golden_subset_for_the_tile_sweeps():
    Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "lloyd_edge_goldens.npz"))
    names = T.golden_tile_cases(Z)
    assert len(names) == 29
    fam = {n.split("_")[0] for n in names}
    # duplicate initial rows are there (tie_dupC0_f32_k3); exact ties, constant data and the 1e4 magnitude are not
    # (N < 64 or d = 4), hence the cases "tie", "const-*" and "offset1e4"; no late-empty golden is f32 with d = 2
    assert fam == {"cov", "maxit", "prec", "stop", "tie"} and [n for n in names if n.startswith("tie")] == ["tie_dupC0_f32_k3"]
    assert [n for n in names if n.startswith("prec")] == ["prec_tol_stops_at_1_f32"]
