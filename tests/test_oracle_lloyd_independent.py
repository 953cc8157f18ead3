"""The Lloyd oracle (oracle/lloyd_ref.c, oracle.kpp_candidates) pinned twice more.

a. Against scikit-learn at the edges lloyd_goldens.npz does not reach (tests/golden/make_lloyd_edge_goldens.py, written
   by scikit-learn 1.7.2): every dtype x d in 1..4 x k in {1, 2, 8, 9, 16}, max_iter cuts and natural stops on and next to
   the driver's window boundaries (iterations 3/4, 11/12, 27/28), exact ties, duplicate init rows, empty clusters at
   iteration 0, at iterations 0-4 of one fit (the latest emptying a scan of 40 000 small duplicate-heavy u8 problems
   found is at iteration 4; nothing later turned up), with the farthest distance 0, N == k, constant data, a tol that
   stops at once, data offset by 1e6 and of magnitude 1e4.  The bars are test_oracle_lloyd.py's.

b. Against a definition that shares no algebra with it.  The oracle and the HIP kernels both label with the EXPANDED form
   D_j = |c_j|^2 - 2 x.c_j (FMA chains over centred data), so a mistake in that restatement would pass every parity
   test.  Here the label is the argmin of the DIRECT form sum_f (x_f - m_f - c_f)^2 evaluated exactly (fractions.Fraction
   on the binary values of x, m, c), sums are math.fsum's, counts are integers.

   Rounding bound of the expanded form, u = 2^-53, x the centred sample fl(x_f - m_f) (one IEEE subtraction, at most
   u |x_f| away from the exact x_f - m_f, which moves |x - c|^2 by at most 2 u sum |x_f| |x_f - c_f| <= 2 u (|x|^2 +
   sum |x_f c_f|)); the dot product is a chain of d FMAs, error <= d u sum |x_f c_f|, doubled by the factor 2; |c_j|^2
   likewise <= d u |c|^2; the final subtraction adds u (|c|^2 + 2 sum |x_f c_f|).  Together, and |x|^2 + D_j being
   the squared distance:   | (|x|^2 + D_j) - |x - c_j|^2 |  <=  (d + 4) u (|x|^2 + |c_j|^2 + 2 sum_f |x_f c_f|) =: B_j.
   A sample whose two smallest exact distances differ by less than 2 max(B_j1, B_j2) may legitimately go either way
   and is LEFT OUT; the left-out share is asserted to stay below 1e-3 (measured: 0 on every input used here) -- on the
   exact-tie inputs nothing is left out and the lower index is required.
   k-means++ uses the same expanded form plus |x|^2, ((-2 c.x + |c|^2) + |x|^2): at most d + 2 roundings on each product,
   within the same B.

   Sums.  A recursive (or tree) sum of n floats t_i in any order is within (n - 1) u sum |t_i| of the exact sum (each of
   the n - 1 additions rounds a partial sum that is at most sum |t_i|; first order in u).  The terms themselves -- fl(x_f
   - m_f), and the direct-form squared distance of a sample in sklearn's grouping -- are single IEEE expressions that
   numpy reproduces bit for bit, so the reference is math.fsum over those terms.

Correction to the issue's fixed-point check: a centre equals the mean of its FINAL members only after a strict stop (or a
zero shift).  After a tol stop sklearn re-labels against the last centres, so members have moved since the means were
taken; the check therefore runs with tol = 0 and skips fits cut by max_iter.

Wall time of this file: 17 s on one CPU thread (measured; the exact arithmetic is single-threaded Python).
"""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "lloyd_edge_goldens.npz"))
CASES = sorted({k.split("/")[0] for k in Z.files if "/" in k})
TIE_CASES = [c for c in CASES if c.startswith(("tie_int", "tie_half"))]
U = 2.0 ** -53
LEFT_OUT_CAP = 1e-3


# ------------------------------------------------------------------------------------------------ a. sklearn edges
def test_golden_file_is_what_the_generator_describes():
    assert str(Z["sklearn_version"]) == "1.7.2"
    assert len(CASES) == 105 and sum(c.startswith("cov_") for c in CASES) == 60
    assert {int(Z[c + "/n_iter"]) for c in CASES if c.startswith("stop_")} == {4, 5, 12, 13, 28, 29}
    assert sorted(int(Z[c + "/n_iter"]) for c in CASES if c.startswith("maxit_") and "free" not in c) == \
        [1, 2, 3, 4, 5, 8, 11, 12, 13, 28, 29]
    assert "latest at iteration 4" in str(Z["late_empty_report"])


@pytest.mark.parametrize("name", CASES)
def test_fit_matches_sklearn(name):
    X, C0 = Z[name + "/X"], Z[name + "/C0"]
    cen, lab, inertia, n_iter = O.kmeans_fit(X, C0, int(Z[name + "/max_iter"]), float(Z[name + "/tol"]))
    assert n_iter == int(Z[name + "/n_iter"])
    assert np.array_equal(lab, Z[name + "/labels"])            # bit-exact labels
    # sklearn's own thread-order noise is 6e-14 on data within 0..255, for which the absolute bar 1e-11 was set; the one
    # input beyond that range (prec_mag1e4: |x| up to 4e4, where a single rounding of a centre is 7e-12) gets the same
    # bar in units of its range
    scale = max(1.0, float(np.abs(X.astype(np.float64)).max()) / 255.0) if name.startswith("prec_mag1e4") else 1.0
    assert np.abs(cen - Z[name + "/centers"]).max() <= 1e-11 * scale
    assert abs(inertia - float(Z[name + "/inertia"])) <= 1e-12 * float(Z[name + "/inertia"])


@pytest.mark.parametrize("name", CASES)
def test_predict_matches_sklearn(name):
    X = Z[name + "/X"]
    assert np.array_equal(O.kmeans_predict(X, Z[name + "/centers"]), Z[name + "/predict"])


# ------------------------------------------------------------------------------------------------ the exact definition
def frac_rows(A):
    A = np.asarray(A)
    if A.dtype == np.uint8:
        return [[Fraction(int(v)) for v in row] for row in A]
    return [[Fraction(float(v)) for v in row] for row in A.astype(np.float64)]      # f32 -> f64 is exact


def exact_d2(X, mean, C):
    """[N][k] exact squared distances sum_f (x_f - m_f - c_f)^2; C holds CENTRED centres"""
    m = [Fraction(float(v)) for v in mean]
    Cf = frac_rows(np.asarray(C, np.float64))
    out = []
    for row in frac_rows(X):
        xc = [a - b for a, b in zip(row, m)]
        out.append([sum((a - b) ** 2 for a, b in zip(xc, c)) for c in Cf])
    return out


def expanded_bound(X, mean, C):
    """B[i][j] of the module docstring, (N, k) f64"""
    xc = np.asarray(X, np.float64) - np.asarray(mean, np.float64)
    C = np.asarray(C, np.float64)
    d = xc.shape[1]
    cross = np.abs(xc)[:, None, :] * np.abs(C)[None, :, :]
    return (d + 4) * U * ((xc * xc).sum(1)[:, None] + (C * C).sum(1)[None, :] + 2 * cross.sum(2))


def exact_labels(X, mean, C, ties_exact=False):
    """-> (lowest-index exact argmin (N,) i32, left-out mask (N,), number of exactly tied samples).  A tie between two
    bit-identical centre rows is never left out: their expanded distances are the same number, the lower index wins."""
    C = np.asarray(C, np.float64)
    D = exact_d2(X, mean, C)
    B = expanded_bound(X, mean, C)
    lab = np.empty(len(D), np.int32)
    out = np.zeros(len(D), bool)
    tied = 0
    for i, row in enumerate(D):
        order = sorted(range(len(row)), key=lambda j: (row[j], j))
        lab[i] = order[0]
        if len(row) > 1:
            gap = row[order[1]] - row[order[0]]
            tied += gap == 0
            same = gap == 0 and np.array_equal(C[order[0]], C[order[1]])   # bit-identical centres: bit-identical D_j
            if not ties_exact and not same:
                out[i] = gap < 2 * max(B[i, order[0]], B[i, order[1]])
    return lab, out, tied


def exact_labels_wide(X, mean, C):
    """the same rule for inputs too large for Fractions: direct form in 64-bit-mantissa long double, whose own rounding
    ((d + 2) 2^-64 relative) is a thousandth of B and is added to the threshold"""
    assert np.finfo(np.longdouble).nmant >= 63
    xc = np.asarray(X, np.longdouble) - np.asarray(mean, np.longdouble)
    C = np.asarray(C, np.longdouble)
    D = np.zeros((len(xc), len(C)), np.longdouble)
    for f in range(xc.shape[1]):
        D += (xc[:, f, None] - C[None, :, f]) ** 2
    lab = np.argmin(D, axis=1).astype(np.int32)
    if len(C) == 1:
        return lab, np.zeros(len(xc), bool)
    B = expanded_bound(X, mean, C)
    assert len(np.unique(np.asarray(C, np.float64), axis=0)) == len(C), "duplicate centres: use exact_labels"
    part = np.partition(D, 1, axis=1)
    thr = 2 * B.max(axis=1) * (1 + 2.0 ** -8)
    return lab, np.asarray(part[:, 1] - part[:, 0] < thr)


def sum_bound(terms):
    """(n - 1) u sum |t_i|, see the module docstring"""
    terms = np.asarray(terms, np.float64)
    return max(len(terms) - 1, 0) * U * math.fsum(np.abs(terms))


def direct_terms(X, mean, C, labels):
    """per-sample squared distance to the labelled centre as ONE IEEE expression in sklearn's grouping
    (_euclidean_dense_dense: left to right within a group of four) -- the terms whose sum is the inertia"""
    t = (np.asarray(X, np.float64) - mean) - np.asarray(C, np.float64)[labels]
    t = t * t
    r = t[:, 0].copy()
    for f in range(1, t.shape[1]):
        r = r + t[:, f]
    return r


def column_mean(X):
    return np.array([math.fsum(col) / len(X) for col in np.asarray(X, np.float64).T])


def check_record(rec, X, mean, C, labels_before, labels_after, what=""):
    """a step record [k*d sums | k counts | n_changed] against fsum / integers, given the labels the step produced"""
    k, d = np.asarray(C).shape
    xc = np.asarray(X, np.float64) - mean
    assert rec.shape == (k * d + k + 1,)
    assert np.array_equal(rec[k * d:k * d + k], np.bincount(labels_after, minlength=k)[:k].astype(np.float64)), what
    assert rec[k * d + k] == float(np.count_nonzero(labels_before != labels_after)), what
    for j in range(k):
        mem = xc[labels_after == j]
        for f in range(d):
            want, tol = math.fsum(mem[:, f]), sum_bound(mem[:, f])
            assert abs(rec[j * d + f] - want) <= tol, (what, j, f, rec[j * d + f], want, tol)


LABEL_INPUTS = [c for c in CASES if c.startswith(("cov_", "prec_", "empty_it0", "tie_dup"))] + ["maxit_05", "stop_12_tol_seed0_k5"]


# ------------------------------------------------------------------------------------------------ b. independent pin
def test_partials_labels_sums_counts_against_the_exact_definition():
    """O.lloyd_partials at the initial and at the fitted centres of the golden inputs: labels = exact argmin outside the
    left-out set (share asserted and printed), counts exact, centred sums within the summation bound, n_changed = N from
    unassigned labels and 0 on the second call"""
    n_all = n_out = 0
    for name in LABEL_INPUTS:
        X = Z[name + "/X"]
        mean = column_mean(X)
        for C in (Z[name + "/C0"] - mean, Z[name + "/centers"] - mean):
            want, out, _ = exact_labels(X, mean, C)
            lab = np.full(len(X), -1, np.int32)
            rec = O.lloyd_partials(X, mean, C, lab)
            assert np.array_equal(lab[~out], want[~out]), name
            check_record(rec, X, mean, C, np.full(len(X), -1), lab, name)
            again = lab.copy()
            rec2 = O.lloyd_partials(X, mean, C, again)
            assert np.array_equal(again, lab) and rec2[-1] == 0.0 and np.array_equal(rec2[:-1], rec[:-1]), name
            n_all += len(X)
            n_out += int(out.sum())
    print("lloyd_partials: %d of %d samples left out (share %.2e)" % (n_out, n_all, n_out / n_all))
    assert n_out / n_all <= LEFT_OUT_CAP


@pytest.mark.parametrize("name", TIE_CASES)
def test_partials_exact_ties_go_to_the_lower_index(name):
    """integer data, column sums divisible by N, cluster sizes powers of two: every operation of the expanded form is
    exact, so nothing is left out and an equidistant sample must take the lower index"""
    X, C0 = Z[name + "/X"], Z[name + "/C0"]
    assert np.all(X.astype(np.int64).sum(0) % len(X) == 0)
    mean = X.astype(np.float64).sum(0) / len(X)
    want, out, tied = exact_labels(X, mean, C0 - mean, ties_exact=True)
    assert tied >= 1 and not out.any()
    lab = np.full(len(X), -1, np.int32)
    rec = O.lloyd_partials(X, mean, C0 - mean, lab)
    assert np.array_equal(lab, want)
    assert np.array_equal(lab, Z[name + "/labels"])                   # and sklearn agrees
    k, d = C0.shape
    for j in range(k):                                                 # exact sums: the centres are the members' means
        assert np.array_equal(rec[j * d:(j + 1) * d], (C0[j] - mean) * rec[k * d + j])


def test_partials_raw_u8_column_sums_are_exact_integers():
    for name in [c for c in CASES if "uint8" in c or "_u8" in c]:
        X = Z[name + "/X"]
        d = X.shape[1]
        rec = O.lloyd_partials(X, np.zeros(d), np.zeros((1, d)), np.full(len(X), -1, np.int32))
        assert np.array_equal(rec[:d], X.astype(np.int64).sum(0).astype(np.float64)), name
        assert rec[d] == len(X) and rec[d + 1] == len(X)


def test_partials_n_changed_after_moving_one_centre():
    name = "cov_float32_d2_k8"
    X = Z[name + "/X"]
    mean = column_mean(X)
    C = Z[name + "/centers"] - mean
    lab = np.full(len(X), -1, np.int32)
    O.lloyd_partials(X, mean, C, lab)
    C2 = C.copy()
    C2[3] = 0.5 * (C[3] + C[5])
    w0, o0, _ = exact_labels(X, mean, C)
    w1, o1, _ = exact_labels(X, mean, C2)
    assert not o0.any() and not o1.any()
    before = lab.copy()
    rec = O.lloyd_partials(X, mean, C2, lab)
    assert 0 < np.count_nonzero(w0 != w1) == rec[-1]
    check_record(rec, X, mean, C2, before, w1, name)


def kpp_inputs():
    rng = np.random.default_rng(31)
    for name in ("cov_uint8_d4_k8", "cov_float32_d2_k9", "cov_float64_d3_k16", "cov_uint8_d1_k2", "prec_mag1e4_f32_k6"):
        X = Z[name + "/X"]
        for n_cand in (1, 8):
            cand = rng.choice(len(X), n_cand, replace=False).astype(np.int64)
            cand[-1] = cand[0] if n_cand == 8 else cand[-1]                         # a repeated candidate
            yield name, X, cand
    yield "one_sample", np.array([[3.0, 4.0]]), np.array([0], np.int64)
    X = near_duplicates(257, 3)
    yield "near_duplicates", X, np.arange(8, dtype=np.int64)


def near_duplicates(N, d):
    """f64 rows of magnitude 1e3 that repeat eight base rows to within a few ulp: the expanded form of their distance to
    the base row is rounding noise of either sign, so a missing clamp shows as a negative distance"""
    rng = np.random.default_rng(N + d)
    base = rng.uniform(500, 1500, (8, d))
    X = base[np.arange(N) % 8] * (1 + 2.0 ** -52 * rng.integers(-3, 4, (N, d)))
    X[:8] = base
    return X


def test_near_duplicates_drive_the_unclamped_expanded_form_negative():
    """the input does what it is for, shown without any code under test: plain numpy, no clamp"""
    X = near_duplicates(257, 3)
    xc = X - column_mean(X)
    neg = 0
    for c in range(8):
        dot = xc[:, 0] * xc[c, 0]
        cc, xx = xc[c, 0] * xc[c, 0], xc[:, 0] * xc[:, 0]
        for f in range(1, 3):
            dot, cc, xx = dot + xc[:, f] * xc[c, f], cc + xc[c, f] * xc[c, f], xx + xc[:, f] * xc[:, f]
        neg += int(np.count_nonzero((-2.0 * dot + cc) + xx < 0))
    assert neg >= 20


def check_kpp(out, pots, X, mean, cand, closest, what="", own_exact=False):
    """out[c][i] against the exact direct form (minimum with `closest`), never negative, pots against fsum of the row.
    own_exact: a candidate's own entry is exactly 0.  That holds for the device kernel (its three products c.x, |c|^2,
    |x|^2 are the same numbers when x is c) but not for sklearn's form, which the oracle restates: there the dot product
    is BLAS's and the norms are numpy's, so the own entry is rounding noise clamped at 0 -- within B like every other."""
    Xc = np.asarray(X, np.float64) - mean
    B = expanded_bound(X, mean, Xc[cand])
    D = exact_d2(X, mean, Xc[cand]) if len(X) <= 5000 else None
    for c, ci in enumerate(cand):
        if D is not None:
            want = np.array([float(D[i][c]) for i in range(len(X))])
        else:
            want = np.asarray(((np.asarray(X, np.longdouble) - np.asarray(mean, np.longdouble) - Xc[ci].astype(np.longdouble)) ** 2)
                              .sum(1), np.float64)
        if closest is not None:
            want = np.minimum(want, closest)
            assert np.all(out[c] <= closest), what
        assert np.all(np.abs(out[c] - want) <= B[:, c] + U * want), (what, c, np.abs(out[c] - want).max())
        assert np.all(out[c] >= 0.0), what
        if own_exact:
            assert out[c][ci] == 0.0, (what, c, out[c][ci])
        assert abs(pots[c] - math.fsum(out[c])) <= sum_bound(out[c]), (what, c)


def test_kpp_candidates_against_exact_distances():
    for name, X, cand in kpp_inputs():
        mean = column_mean(X)
        out, pots = O.kpp_candidates(X, mean, cand)
        check_kpp(out, pots, X, mean, cand, None, name)
        closest = out[0] * np.random.default_rng(len(X)).uniform(0.2, 1.8, len(X))
        out2, pots2 = O.kpp_candidates(X, mean, cand, closest)
        check_kpp(out2, pots2, X, mean, cand, closest, name + " closest")


FIXED_POINT_INPUTS = ["cov_uint8_d4_k8", "cov_uint8_d1_k16", "cov_float32_d2_k9", "cov_float32_d3_k2", "cov_float64_d4_k16",
                      "cov_float64_d1_k1", "maxit_free_seed2", "stop_13_strict_seed10_k3", "maxit_12", "tie_int_d2_k3_uint8"]


def test_fit_is_an_exact_fixed_point_with_the_inertia_of_its_labels():
    """at the centres O.kmeans_fit returns (tol = 0): every label outside the left-out set is the exact argmin, each centre
    is the exact mean of its members to n u max|x| unless max_iter cut the fit, the inertia is the fsum of the members'
    direct-form distances"""
    n_all = n_out = 0
    for name in FIXED_POINT_INPUTS:
        X, C0, max_iter = Z[name + "/X"], Z[name + "/C0"], int(Z[name + "/max_iter"])
        cen, lab, inertia, n_iter = O.kmeans_fit(X, C0, max_iter, 0.0)
        mean = column_mean(X)
        want, out, _ = exact_labels(X, mean, cen - mean, ties_exact=name.startswith("tie_int"))
        assert np.array_equal(lab[~out], want[~out]), name
        n_all += len(X)
        n_out += int(out.sum())
        if n_iter < max_iter:
            rows = frac_rows(X)
            xmax = float(np.abs(X.astype(np.float64)).max())
            for j in range(len(cen)):
                mem = [rows[i] for i in np.flatnonzero(lab == j)]
                assert mem, name
                for f in range(X.shape[1]):
                    exact = sum(r[f] for r in mem) / len(mem)
                    assert abs(Fraction(float(cen[j, f])) - exact) <= len(mem) * U * xmax, (name, j, f)
        terms = direct_terms(X, mean, cen - mean, lab)
        # the oracle centres with its own column mean and un-centres the result: one more rounding of u |x| on each side
        slack = 4 * U * float(np.abs(X.astype(np.float64)).max()) * math.fsum(np.sqrt(terms))
        assert abs(inertia - math.fsum(terms)) <= sum_bound(terms) + slack, (name, inertia, math.fsum(terms))
    print("fixed point: %d of %d samples left out (share %.2e)" % (n_out, n_all, n_out / n_all))
    assert n_out / n_all <= LEFT_OUT_CAP
