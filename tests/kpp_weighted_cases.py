"""Shared by test_kpp_weighted_host.py and test_gpu_kpp_weighted.py (no test in here): the end-to-end cases of the
k-means++ seeding with sample weights, and the host route through the CPU oracle that the device route must reproduce
index for index.  The host route also reports how far every draw lies from the nearest boundary of its cumulative sum and
how far the winning potential lies from the others: that is what makes "index for index" a fair demand.

What the weights change in sklearn 1.7.2's _kmeans_plusplus (_kmeans.py:174-272):
  first centre     rs.choice(N, p=w / w.sum()): ONE random_sample(), looked up with side='right' in cumsum(p)    :224
  later draws      searchsorted(cumsum(w * closest), uniform * current_pot), clipped to N - 1                   :242-247
  potentials       min(closest, d(., cand)) @ w, the first minimum wins                                         :250-259
closest itself, the centring (unweighted column mean) and the distances are those of the unit-weight seeding."""
import numpy as np

from oracle import oracle as O
from tests import kpp_seed_cases as KC

CH = KC.CH
DTYPES = KC.DTYPES
WKINDS = ("wf32", "w01", "wint")      # f32 random, f32 0/1 (about 70 % zeros), f64 small integers


def _cases():
    out = []
    for dt in DTYPES:
        for d in (1, 2, 4):
            for k in (1, 2, 8, 16):
                for N in (4 * k, CH + 1, 3 * CH + 7):      # 4k, not k: see make_w
                    for wk in WKINDS:
                        out.append(("rand", dt, d, k, N, wk))
    # fewer distinct rows than k, N == k, zero weights: the potential reaches zero before the last centre.  Exact data
    # (kpp_seed_cases.make_X's 'dup') with small-integer weights: every product and sum is exact in any order
    for dt in DTYPES:
        for k, N in ((8, 8), (8, CH + 1), (16, 3 * CH + 7)):
            out.append(("dup", dt, 2, k, N, "wint"))
    return out


CASES = _cases()
assert max(c[4] for c in CASES) <= 20000


# Cases whose default seed (their position in CASES) leaves a draw or a potential inside the conditioning bar of
# test_kpp_weighted_host.py get another one here.  All of them so far are small (N = 4k) with few rows of weight left at the
# end: two such rows that are each other's nearest centre give two candidates the same potential up to the order of summation.
RESEED = {"rand-u8-1-8-32-w01": 1007, "rand-u8-1-16-64-w01": 1025, "rand-u8-2-2-8-w01": 1000, "rand-u8-4-8-32-w01": 1001,
          "rand-u8-4-16-64-w01": 1000, "rand-f32-1-8-32-w01": 1001, "rand-f32-1-16-64-wint": 1000, "rand-f32-2-8-32-w01": 1000,
          "rand-f32-2-16-64-w01": 1000, "rand-f64-1-16-64-w01": 1000, "rand-f64-2-8-32-w01": 1000, "rand-f64-2-8-32-wint": 1000,
          "rand-f64-2-16-64-w01": 1002, "rand-f64-4-16-64-w01": 1000}


def case_id(c):
    return "-".join(str(v) for v in c)


def case_seed(c):
    return RESEED.get(case_id(c), CASES.index(c))


def make_X(c):
    kind, dt, d, k, N, _ = c
    if kind == "dup":
        return KC.make_X(("dup", dt, 2, k, N))
    rng = np.random.default_rng(5000 + CASES.index(c))
    if dt == "u8":
        return rng.integers(0, 256, (N, d)).astype(np.uint8)
    return (rng.normal(size=(N, d)) * 3 + rng.integers(0, 4, (N, 1)) * 5).astype(DTYPES[dt])


def make_w(c):
    """For random data the smallest N is 4k: with N == k the seeding uses up the rows of positive weight and the later
    potentials are rounding noise, which no two summation orders agree on.  The exact 'dup' data covers that ground."""
    kind, _, _, k, N, wk = c
    rng = np.random.default_rng(9000 + CASES.index(c))
    if wk == "wf32":
        return (rng.random(N) * 3 + 0.05).astype(np.float32)
    if wk == "w01":
        w = (rng.random(N) < 0.3).astype(np.float32)
        w[rng.integers(0, N)] = 1.0
        return w
    w = rng.integers(0, 4, N).astype(np.float64)
    if kind == "dup":
        w[: N // 8] = 0          # a leading run of zero weights
    w[rng.integers(N // 2, N)] = 2.0
    return w


def first_index(w, u_first):
    """what rs.choice(N, p=w / w.sum()) returns for the random_sample() u_first (numpy/random/mtrand.pyx: cdf = p.cumsum(),
    cdf /= cdf[-1], searchsorted(side='right'))"""
    w = np.asarray(w, np.float64)
    cdf = (w / w.sum()).cumsum()
    cdf /= cdf[-1]
    return int(np.searchsorted(cdf, u_first, side="right"))


def host_seed(X, w, k, u_first, u):
    """sklearn's _kmeans_plusplus with sample weights on pre-drawn numbers, the CPU oracle as the distance step (what
    cluster.kmeans_plusplus(..., sample_weight=w, _step=O.kpp_candidates) computes).
    -> indices,
       gaps: per draw (distance to the nearest cumulative-sum boundary, potential; for the first draw: the weight sum),
       seps: per step and losing candidate of another row value (|its potential - the winner's|, the larger of the two),
       pots_before: the potential each further centre was drawn from"""
    N = len(X)
    w = np.asarray(w, np.float64)
    mean = KC.host_mean(X)
    idx = np.full(k, -1, np.int64)
    W = float(w.sum())
    cumw = np.cumsum(w)
    idx[0] = first_index(w, u_first)
    gaps = [(float(np.abs(cumw - u_first * W).min()), W)]
    seps, pots_before = [], []
    out, _ = O.kpp_candidates(X, mean, idx[:1])
    closest = out[0]
    pot = float(closest @ w)
    for c in range(1, k):
        rv = u[c - 1] * pot
        cum = np.cumsum(w * closest, dtype=np.float64)
        ids = np.searchsorted(cum, rv)
        np.clip(ids, None, N - 1, out=ids)
        gaps += [(float(np.abs(cum - r).min()), pot) for r in rv]
        pots_before.append(pot)
        out, _ = O.kpp_candidates(X, mean, ids, closest)
        pots = out @ w
        best = int(np.argmin(pots))
        for j in range(len(ids)):
            if not np.array_equal(X[ids[j]], X[ids[best]]):
                seps.append((float(abs(pots[j] - pots[best])), float(max(pots[j], pots[best]))))
        pot, closest = float(pots[best]), out[best]
        idx[c] = ids[best]
    return idx, gaps, seps, pots_before
