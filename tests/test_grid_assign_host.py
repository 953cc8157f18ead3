"""Host side of the fused label-and-count (ofc_grid_assign_counts_dev, FlowStream's model, motionGrids --stream): the
centre sets of tests/grid_assign_cases.py leave no lattice point ambiguous, so the GPU tests may demand every label; the
numpy model is what one counts by hand; the parser knows the new options."""
import numpy as np
import pytest

from tests import grid_assign_cases as GA
from tests import motion_grid_cases as MC


@pytest.mark.parametrize("k", MC.KS)
def test_centre_sets_leave_no_lattice_point_ambiguous(k):
    """best and second-best direct-form squared distance >= 1e-3 apart at EVERY lattice point (the minimum over all k is
    1.35e-3): some 1e12 times the rounding of any float64 way of forming them, the expanded form centred by any mean
    included.  Translation by the dyadic mean keeps the gap, and that is asserted too, not assumed"""
    cen = GA.centres(k)
    assert cen.shape == (k, 2) and np.abs(cen).max() <= 3.6 and np.array_equal(cen, np.round(cen, 4))
    gap, shifted = GA.lattice_gap(cen), GA.lattice_gap(cen, GA.DYADIC_MEAN)
    print("k = %d: smallest gap %.4e, shifted by the mean %.4e" % (k, gap, shifted))
    assert gap >= GA.GAP and shifted >= GA.GAP
    if k > 1:
        assert abs(gap - shifted) <= 1e-9
    L = MC.lattice()
    assert np.array_equal((L - GA.DYADIC_MEAN) + GA.DYADIC_MEAN, L)          # x - mean is exact on the lattice


def test_fields_are_on_the_lattice_and_meet_every_cluster():
    for geom, (rows, cols, W, H, n) in MC.GEOMETRIES.items():
        if geom == "reference-1080p":
            continue
        F = GA.field(geom)
        assert F.dtype == np.float32 and F.shape == (n, H, W, 2)
        assert np.array_equal(F * 8, np.round(F * 8)) and np.abs(F).max() <= 4
    fl, cen, lab, counts, sums = GA.case("remainders-odd-frame", 5)
    assert len(np.unique(lab)) == 5 and counts.shape == (3, 12, 5) and sums.shape == (3, 12, 5, 2)
    assert np.array_equal(GA.field("whole-frame", 7)[0, :48, :64], MC.assign_field(7)[0])      # drawn as assign_field draws


def test_model_on_a_hand_made_frame():
    """4 x 6, 2 x 2 cells of 2 x 3 px, centres (2, 0), (-2, 0), (0, 3); labels and sums counted by hand"""
    cen = np.array([[2.0, 0.0], [-2.0, 0.0], [0.0, 3.0]])
    u = np.array([[2, 1, -2, 0, 0, 3],
                  [-1, 2, 0, -3, 1, 0],
                  [0, 0, 0, -1, -1, -1],
                  [1, 1, -1, 0, 2, -2]], np.float64)
    v = np.array([[0, 0, 0, 3, 2.5, 0],
                  [0, 1, 4, 0, 0, 2],
                  [3, 2, 1.5, 0, 0, 0],
                  [0, 0, 0, 2.5, 0, 0]], np.float64)
    flow = np.stack([u, v], -1).astype(np.float32)[None]
    want = np.array([[0, 0, 1, 2, 2, 0],
                     [1, 0, 2, 1, 0, 2],
                     [2, 2, 2, 1, 1, 1],
                     [0, 0, 1, 2, 0, 1]], np.uint8)
    lab = GA.model_labels(flow, cen)
    assert np.array_equal(lab[0], want)
    assert np.array_equal(GA.expanded_labels(flow, cen)[0], want)          # no tie on this frame: both forms agree
    counts, sums = MC.model_counts(lab, 3, 2, 2, flow)
    assert counts[0].tolist() == [[3, 2, 1], [2, 1, 3], [2, 1, 3], [1, 4, 1]]
    assert sums[0, 0].tolist() == [[5, 1], [-3, 0], [0, 4]]
    assert sums[0, 3].tolist() == [[2, 0], [-5, 0], [0, 2.5]]


def test_tie_centres_tie_exactly():
    """(1, 0), (-1, 0), (0, 1): cn = 1 and x.c = +-u or v, so the expanded form is exact in float64 and ties where u = 0,
    u = v or -u = v are exact ties: the first minimum is the lowest index"""
    flow = np.array([[[0.0, 0.0], [0.0, -1.0], [1.5, 1.5], [-2.0, 2.0], [0.0, 0.125], [-0.125, 0.0]]], np.float32)[None]
    assert GA.expanded_labels(flow, GA.TIE_CENTRES)[0, 0].tolist() == [0, 0, 0, 1, 2, 1]
    d = np.sort(MC.direct_sqdist(MC.lattice(), GA.TIE_CENTRES), axis=1)
    # the nearest centre is tied on the half-line u = 0, v <= 0 (33 points) and the diagonals |u| = v > 0 (32 each)
    assert (d[:, 1] == d[:, 0]).sum() == 97


def test_cli_parser_stream_options():
    from opticalflowclustering_amd import motionGrids as G
    a = G.parse_arguments(["--path", "clip.npy", "-c", "5", "-f", "out.csv"])
    assert a.stream is False and a.batch_pairs == 8
    a = G.parse_arguments(["--path", "v", "-c", "3", "-f", "o.csv", "--model", "m.npy", "--stream"])
    assert a.stream is True and a.batch_pairs == 8 and a.model == "m.npy"
    a = G.parse_arguments(["--path", "v", "-c", "3", "-f", "o.csv", "--model", "m.npy", "--stream", "--batch-pairs", "3"])
    assert a.batch_pairs == 3
    for bad in (["--stream"], ["--stream", "--init", "c0.npy"], ["--model", "m.npy", "--stream", "--batch-pairs", "0"],
                ["--model", "m.npy", "--stream", "--batch-pairs", "x"]):
        with pytest.raises(SystemExit):                                      # --stream needs a model: there is no fit on a stream
            G.parse_arguments(["--path", "v", "-c", "3", "-f", "o"] + bad)
