"""Host side of the (u,v) histogram (uvhist.py, motionGrids --fit-stream): the numpy model is what one counts by hand, the
cases of tests/uv_hist_cases.py are proven well-conditioned here so that test_gpu_uv_hist.py may demand equal integers and
the derived bound, UVHistogram's arithmetic and refusals, the seeds of n_init restarts, and the parser's new options."""
import os
import re

import numpy as np
import pytest

from tests import uv_hist_cases as UC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "ofc.h")).read()
    assert int(re.search(r"#define OFC_UV_HIST_SHARE (\d+)", text).group(1)) == UC.SHARE
    assert int(re.search(r"#define OFC_UV_HIST_MAX_GRID (\d+)", text).group(1)) == UC.MAX_GRID
    assert UC.SHARE % 256 == 0


def test_model_by_hand():
    """bins 16, range 2: bins 1/4 px wide, scale 4.  Six vectors counted by hand, two of them outside:
    (0, 0) -> (8, 8); (0.1, -0.1) -> floor(8.4), floor(7.6) = (8, 7); (0.2, -0.2) -> floor(8.8), floor(7.2) = (8, 7);
    (2, 0): u = R, outside; (-2, -2) -> (0, 0); (0, NaN): outside"""
    f = np.array([[0.0, 0.0], [0.1, -0.1], [0.2, -0.2], [2.0, 0.0], [-2.0, -2.0], [0.0, np.nan]], np.float32)
    tab = UC.model(f, 16, 2.0)
    B2 = 256

    def q(x):
        return int(np.rint(np.float64(np.float32(x)) * 65536))

    want = np.zeros(3 * B2 + 1, np.int64)
    want[[8 * 16 + 8, 7 * 16 + 8, 0]] = 1, 2, 1
    want[B2 + 7 * 16 + 8], want[2 * B2 + 7 * 16 + 8] = q(0.1) + q(0.2), q(-0.1) + q(-0.2)
    want[B2], want[2 * B2] = -131072, -131072
    want[-1] = 2
    assert np.array_equal(tab, want) and q(-0.1) < 0
    again = UC.model(f, 16, 2.0, tab)
    assert np.array_equal(again, 2 * want) and np.array_equal(tab, want)        # added to a copy


@pytest.mark.parametrize("bins,rng", UC.PARAMS)
def test_special_values_fall_where_the_arithmetic_says(bins, rng):
    R = np.float32(rng)
    vals = UC.special_values(bins, rng)
    for axis in (0, 1):
        b = UC.bin_of(UC.in_one_axis(vals, axis, 0.25 * rng), bins, rng)
        inside = b >= 0
        # -R, +-0, denormals and +-0.75 R are in; R, the value below R (its sum rounds up to 2R), the value below -R,
        # NaN, +-inf and +-FLT_MAX are out
        assert inside.tolist() == [True, False, False, False, True, True, True, True, True, False, False, False, False, False,
                                   True, True]
        other = int(np.floor((0.25 * rng + rng) * bins / (2 * rng)))
        coord = b[inside] % bins if axis == 0 else b[inside] // bins
        assert coord.tolist() == [0, bins // 2, bins // 2, bins // 2, bins // 2, bins // 2, bins // 8 * 7, bins // 8]
        assert ((b[inside] // bins if axis == 0 else b[inside] % bins) == other).all()
    assert np.float32(np.nextafter(R, np.float32(0)) + R) == np.float32(2) * R   # "outside, by the arithmetic"


@pytest.mark.parametrize("bins,rng", UC.PARAMS)
def test_edge_values_take_the_bin_above_the_edge(bins, rng):
    e = UC.edge_values(bins, rng)
    b = UC.bin_of(UC.in_one_axis(e, 0, 0.0), bins, rng)
    n = bins + 1
    on, below, above = b[:n] % bins, b[n:2 * n], b[2 * n:]
    assert np.array_equal(on[:-1], np.arange(bins)) and b[n - 1] == -1           # the last edge is R
    assert below[0] == -1 and (below[1:] >= 0).sum() >= bins - 1                 # below -R is outside
    assert (above[:-1] >= 0).all() and above[-1] == -1


@pytest.mark.parametrize("bins,rng", UC.PARAMS)
@pytest.mark.parametrize("name", UC.PATTERNS)
def test_patterns_are_in_range_and_laid_out_as_named(name, bins, rng):
    f = UC.pattern(name, 4099, bins, rng)
    b = UC.bin_of(f, bins, rng)
    assert (b >= 0).all()                                                        # nothing meant to be in range is outside
    waves = [b[i:i + 64] for i in range(0, 4096, 64)]
    distinct = [len(np.unique(w)) for w in waves]
    if name == "one-bin":
        assert len(np.unique(b)) == 1
    elif name == "own-bin":
        assert min(distinct) == 64
    elif name == "two-alternating":
        assert set(distinct) == {2} and (b[0::2] == b[0]).all() and (b[1::2] == b[1]).all()
    elif name == "63-and-1":
        assert set(distinct) == {2} and all((w == w[17]).sum() == 1 for w in waves)
    elif name == "wave-boundary":
        assert set(distinct) == {1} and all(waves[i][0] != waves[i + 1][0] for i in range(63))
    tab = UC.model(f, bins, rng)
    assert tab[-1] == 0 and tab[:bins * bins].sum() == 4099
    assert (tab[bins * bins:-1] < 0).any()                                       # negative sums occur


def test_lattice_field_has_one_value_per_bin_and_clear_boundaries():
    X = UC.lattice_field()
    b = UC.bin_of(X, UC.FIT_BINS, UC.FIT_RANGE)
    assert (b >= 0).all()
    for u in np.unique(b):
        assert len(np.unique(X[b == u], axis=0)) == 1
    assert np.array_equal(np.rint(X.astype(np.float64) * 65536) / 65536, X)      # the fixed-point step loses nothing here
    cen, lab, _ = UC.lloyd(X, UC.FIT_INIT)
    margin = UC.boundary_margin(X, cen).min()
    print("lattice: smallest distance to a Voronoi boundary %.3f px, bin diagonal %.3f px" % (margin, UC.FIT_WIDTH * 2 ** 0.5))
    assert margin > UC.FIT_WIDTH * 2 ** 0.5
    assert np.bincount(lab, minlength=UC.FIT_K).min() > 1000


def test_off_lattice_field_is_in_range_with_clear_boundaries():
    X = UC.off_lattice_field()
    assert (UC.bin_of(X, UC.FIT_BINS, UC.FIT_RANGE) >= 0).all()
    cen, _, _ = UC.lloyd(X, UC.FIT_INIT)
    assert UC.boundary_margin(X, cen).min() > UC.FIT_WIDTH * 2 ** 0.5            # no bin straddles a boundary


def test_histogram_fit_equals_the_full_fit_on_the_cpu():
    """the claim the GPU test repeats with the library's Lloyd: on the lattice the two fits agree to rounding with equal
    n_iter and labels; off it, within the fixed-point bound of 2^-17 px"""
    from opticalflowclustering_amd.uvhist import UVHistogram
    for X, bar in ((UC.lattice_field(), 1e-9), (UC.off_lattice_field(), 2.0 ** -17)):
        h = UVHistogram(UC.FIT_BINS, UC.FIT_RANGE, UC.model(X, UC.FIT_BINS, UC.FIT_RANGE))
        P, w = h.points()
        assert h.n == len(X) and h.outside == 0 and w.sum() == len(X)
        full, lab, it = UC.lloyd(X, UC.FIT_INIT)
        hist, hlab, hit = UC.lloyd(P, UC.FIT_INIT, w)
        print("|histogram fit - full fit| = %.3e px" % np.abs(full - hist).max())
        assert np.abs(full - hist).max() <= bar and it == hit
        order = np.flatnonzero(h.counts.ravel())                                 # points() is in bin order
        assert np.array_equal(hlab[np.searchsorted(order, UC.bin_of(X, UC.FIT_BINS, UC.FIT_RANGE))], lab)


def test_points_merge_and_refusals():
    from opticalflowclustering_amd.uvhist import UVHistogram, check_params, table_len
    f = UC.pattern("uniform", 500, 16, 2.0, seed=3)
    g = UC.mixed_field(700, 16, 2.0)
    a, b = UVHistogram(16, 2.0, UC.model(f, 16, 2.0)), UVHistogram(16, 2.0, UC.model(g, 16, 2.0))
    both = UVHistogram(16, 2.0, UC.model(np.concatenate([f, g]), 16, 2.0))
    assert np.array_equal((a + b).table, both.table) and np.array_equal(a.merge(b).table, both.table)
    assert a.counts.shape == (16, 16) and a.counts.dtype == np.int64 and a.n == 500 and a.outside == 0
    assert b.outside > 0 and b.n + b.outside == 700
    P, w = both.points()
    idx = np.flatnonzero(both.counts.ravel())
    assert P.shape == (len(idx), 2) and P.dtype == np.float64 and w.dtype == np.float64
    assert np.array_equal(w, both.counts.ravel()[idx])
    bins_of_means = UC.bin_of(P, 16, 2.0)                                        # a bin's mean lies in that bin
    assert np.array_equal(bins_of_means, idx)
    assert np.allclose(P[:, 0] * w * 65536, both.table[256:512][idx], rtol=1e-13, atol=1e-9)
    assert np.allclose(P[:, 1] * w * 65536, both.table[512:768][idx], rtol=1e-13, atol=1e-9)
    with pytest.raises(ValueError, match="differ"):
        a.merge(UVHistogram(32, 2.0, np.zeros(table_len(32), np.int64)))
    with pytest.raises(ValueError, match="differ"):
        a + UVHistogram(16, 4.0, np.zeros(table_len(16), np.int64))
    with pytest.raises(TypeError):
        a.merge(a.table)
    with pytest.raises(ValueError, match="entries"):
        UVHistogram(16, 2.0, np.zeros(5, np.int64))
    for bins, rng in ((8, 2.0), (4096, 2.0), (48, 2.0), (16.5, 2.0), (16, 3.0), (16, 2.0 ** -5), (16, 2048.0), (16, np.nan), (16, -2.0)):
        with pytest.raises(ValueError, match="power of two"):
            check_params(bins, rng)
    with pytest.raises(ValueError, match="empty"):
        UVHistogram(16, 2.0, np.zeros(table_len(16), np.int64)).fit(2)


def test_restart_seeds_are_sklearns():
    """sklearn's KMeans.fit: seeds = random_state.randint(np.iinfo(np.int32).max, size=n_init)"""
    from opticalflowclustering_amd.uvhist import restart_seeds
    for rs in (0, 7, 12345):
        want = np.random.RandomState(rs).randint(np.iinfo(np.int32).max, size=5)
        assert np.array_equal(restart_seeds(rs, 5), want)
        assert np.array_equal(restart_seeds(rs, 3), want[:3])                    # a prefix: more restarts never change earlier ones
    assert np.array_equal(restart_seeds(np.random.RandomState(4), 2), np.random.RandomState(4).randint(2 ** 31 - 1, size=2))


def test_cli_parser_fit_stream_options():
    from opticalflowclustering_amd import motionGrids as G
    base = ["--path", "v", "-c", "3", "-f", "o.csv"]
    a = G.parse_arguments(base)
    assert a.fit_stream is False and a.hist_bins == 1024 and a.hist_range == 32.0 and a.n_init == 1
    a = G.parse_arguments(base + ["--fit-stream"])
    assert a.fit_stream is True and a.stream is False and a.model is None and a.batch_pairs == 8
    a = G.parse_arguments(base + ["--fit-stream", "--hist-bins", "256", "--hist-range", "8", "--n-init", "4", "--seed", "3",
                                  "--init", "c0.npy", "--batch-pairs", "2"])
    assert (a.hist_bins, a.hist_range, a.n_init, a.seed, a.init, a.batch_pairs) == (256, 8.0, 4, 3, "c0.npy", 2)
    for bad in (["--fit-stream", "--model", "m.npy"], ["--fit-stream", "--stream"], ["--fit-stream", "--stream", "--model", "m.npy"],
                ["--fit-stream", "--weights", "magnitude"], ["--fit-stream", "--hist-bins", "100"],
                ["--fit-stream", "--hist-range", "3"], ["--fit-stream", "--n-init", "0"], ["--fit-stream", "--hist-bins", "x"],
                ["--stream"]):                                                   # --stream alone still needs a model
        with pytest.raises(SystemExit):
            G.parse_arguments(base + bad)
