"""CPU side of test_gpu_flow_sequences.py: the two clips of tests/flow_sequence_cases.py are fit for what the GPU module
uses them for.  The anchor pairs are well-conditioned (the oracle and the independent float64 Farneback agree far inside
the bar the GPU is held to), any two pairs of a clip differ by far more than any bar (so a stale, repeated or mispaired
frame cannot pass), no grid cell's mean cancels (so the cell-mean bar, which scales with |mean|, stays meaningful), and the
case tables hold what they claim."""
import numpy as np
import pytest

import flow_sequence_cases as S
from oracle import oracle as O
from test_oracle_farneback_independent import farneback_f64


@pytest.fixture(scope="module")
def table():
    fr = S.clip()
    return fr, [O.farneback(fr[t], fr[t + 1]) for t in range(len(fr) - 1)]


def test_clip_geometry_is_what_the_cases_assume():
    assert O.pyramid_levels(S.W, S.H) == 1                      # two pyramid levels: 0 and 1
    assert O.pyramid_levels(S.GROW_W, S.GROW_H) == 0            # one
    assert (S.H // S.FINE_GRID[0], S.W // S.FINE_GRID[1]) == (6, 6)
    for rows, cols, w, h in (S.GRID + (S.W, S.H), S.FINE_GRID + (S.W, S.H), S.GROW_GRID + (S.GROW_W, S.GROW_H)):
        assert (h // rows) * (w // cols) <= 1 << 12             # what cell_mean_bar's second term assumes
    assert S.N_FRAMES >= max(T for _, T in S.STREAM_CASES) + 1
    steps = np.array([S.step(t) for t in range(S.N_FRAMES - 1)])
    d = np.abs(steps[:, None] - steps[None]).max(-1)
    assert d[~np.eye(len(d), dtype=bool)].min() >= 0.1          # the true motions already differ by twice DISTINCT_PX


def test_anchor_pairs_are_well_conditioned(table):
    """oracle against the independent float64 Farneback on the pairs the GPU module anchors to: inside 1 / 20 of the
    GPU bars, so the ANCHOR_MARGIN the GPU has to keep is not used up by the oracle's own float32 arithmetic"""
    fr, tab = table
    assert len(set(S.ANCHOR_PAIRS)) == 3 and S.ANCHOR_PAIRS[0] == 0 and S.ANCHOR_PAIRS[-1] == len(tab) - 1
    for t in S.ANCHOR_PAIRS:
        got, ref = tab[t].astype(np.float64), farneback_f64(fr[t], fr[t + 1])
        assert S.rel(got, ref) <= S.ANCHOR_REL / 20, (t, S.rel(got, ref))
        assert np.abs(got - ref).max() <= S.ANCHOR_ABS / 20, (t, np.abs(got - ref).max())


@pytest.mark.parametrize("grid", [S.GRID, S.FINE_GRID])
def test_every_two_pairs_of_the_clip_differ_and_no_cell_cancels(table, grid):
    _, tab = table
    means = np.stack([S.cell_means(f, *grid) for f in tab])
    assert S.min_pair_distance(means) > S.DISTINCT_PX
    assert min(S.cancellation(f, *grid) for f in tab) >= S.CANCEL_FLOOR
    # the bar a stream's cell mean is held to is five orders of magnitude below that distance
    assert max(S.cell_mean_bar(f, *grid).max() for f in tab) <= 1e-5 * S.DISTINCT_PX


def test_staged_window_rows_differ_too():
    """the winsize-31 stream case reads the first 8 frames"""
    fr = S.clip()[:8]
    p = O.default_params()
    p.winsize = 31
    tab = [O.farneback(fr[t], fr[t + 1], p) for t in range(7)]
    assert S.min_pair_distance(np.stack([S.cell_means(f, *S.GRID) for f in tab])) > S.DISTINCT_PX
    assert min(S.cancellation(f, *S.GRID) for f in tab) >= S.CANCEL_FLOOR


def test_growth_clip_never_repeats_a_pair():
    fr = S.grow_clip()
    assert len(fr) == S.GROW_FRAMES and len({f.tobytes() for f in fr}) == S.GROW_FRAMES
    means = np.stack([S.cell_means(O.farneback(fr[t], fr[t + 1]), *S.GROW_GRID) for t in range(len(fr) - 1)])
    assert S.min_pair_distance(means) > S.GROW_DISTINCT_PX
    # 7 pairs per batch: the 37th batch is the first that does not fit 256 rows, and it is neither the first nor the
    # last batch of the clip: rows 0 .. 251 are written before the growth, 259 .. 298 after it
    assert 36 * 7 <= 256 < 37 * 7 < S.GROW_FRAMES - 1


def test_case_tables():
    for B in S.STREAM_BATCHES:
        Ts = S.stream_lengths(B)
        assert set(Ts) == {1, 2, B, B + 1, B + 2, 2 * B + 1, 2 * B + 2, 3 * B + 1, 3 * B + 2} and len(set(Ts)) == len(Ts)
    assert [n for _, n, _ in S.SEQ_WINDOWS][:5] == [5, 1, 3, 5, 2]
    assert [s for _, _, s in S.SEQ_WINDOWS][:5] == [False, True, False, True, False]
    assert all(f0 + n + 1 <= S.SEQ_FRAMES and 1 <= n <= S.SEQ_MAX_BATCH for f0, n, _ in S.SEQ_WINDOWS)
    assert {p for f0, n, _ in S.SEQ_WINDOWS for p in range(f0, f0 + n)} == set(range(S.SEQ_FRAMES - 1))
    a = S.gray_as_bgr(np.arange(256, dtype=np.uint8).reshape(16, 16))
    assert np.array_equal(O.bgr2gray(a), a[..., 0])
    b = S.bgr_frame(0, S.clip())
    assert not np.array_equal(O.bgr2gray(b), b[..., 0]) and not np.array_equal(O.bgr2gray(b), b[..., 1])
