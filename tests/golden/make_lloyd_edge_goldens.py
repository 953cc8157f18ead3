"""Generates tests/golden/lloyd_edge_goldens.npz with the installed scikit-learn: the edges of Lloyd's k-means that
lloyd_goldens.npz does not reach (see make_lloyd_goldens.py for the call that is recorded and the keys of a case).
Only the vectors travel; sklearn is never imported by a test.  Every case stores X itself.

Families (the prefix of a case name):
  cov_      every dtype in {u8, f32, f64} x d in 1..4 x k in {1, 2, 8, 9, 16}
  maxit_    one data set whose free run takes more than 29 iterations, cut at max_iter in MAX_ITERS, tol = 0
  stop_     natural stops exactly on iterations 4, 5, 12, 13, 28, 29 (n_iter_), strict (tol = 0) and by tol, found by
            the seeded scan in find_stops(); the seeds found are kept in STOPS so that a rerun does not scan again
  tie_      integer data whose column sums are divisible by N, integer / half-integer centres that are the exact means
            of their members, samples exactly equidistant from two and from three centres (the lower index wins), and
            duplicate rows in C0 (the second copy is empty at iteration 0 and is relocated)
  empty_    empty clusters: at iteration 0 (a far-away centre), at later iterations, several times in one fit, and with the
            farthest distance 0 (relocation skipped: the empty cluster takes the place of the biggest one, with
            _average_centers' in-place quirk on either side of it)
  prec_     N == k, constant data, a tol that stops at n_iter = 1, f64 data offset by 1e6, f32 data of magnitude 1e4

Late emptying.  find_late_empty() scans small duplicate-heavy u8 problems with sklearn's own iteration
(lloyd_iter_chunked_dense: the E-step alone shows the empty cluster before it is relocated) under the budget
LATE_BUDGET = 40 000 problems (23 s); fits that do not converge within 40 iterations or have fewer distinct rows than
clusters are left out (there sklearn relocates on rounding noise until max_iter).  The cases kept are the latest emptying
found and the fit with the most emptying iterations.  The public API confirms them: KMeans(max_iter=m, tol=0).fit leaves
in labels_ the E-step of iteration m, whose bincount shows the empty cluster.  Found with scikit-learn 1.7.2: E-steps
with an empty cluster at iteration 0: 25180, 1: 6566, 2: 1454, 3: 109, 4: 2, none later; one problem (family 1, seed
1755: N = 63, d = 1, k = 8) empties a cluster in each of the iterations 0, 1, 2, 3 and 4 and converges with n_iter_ = 7.
It holds both records, so it is the one late case.  The report is stored in the npz as `late_empty_report`.
"""
import os
import time
import warnings
from fractions import Fraction

import numpy as np
import sklearn
from sklearn.cluster import KMeans
from sklearn.cluster._k_means_lloyd import lloyd_iter_chunked_dense

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lloyd_edge_goldens.npz")
MAX_ITERS = (1, 2, 3, 4, 5, 8, 11, 12, 13, 28, 29)
STOP_TARGETS = (4, 5, 12, 13, 28, 29)
# (n_iter, kind) -> (seed, k, tol) as find_stops() found them with scikit-learn 1.7.2; None = scan again
STOPS = {(4, 'strict'): (3764, 3, 0.0), (4, 'tol'): (1, 3, 0.001), (5, 'strict'): (73, 3, 0.0), (5, 'tol'): (6, 3, 0.0001),
         (12, 'strict'): (9, 5, 0.0), (12, 'tol'): (0, 5, 0.001), (13, 'strict'): (10, 3, 0.0), (13, 'tol'): (1, 5, 0.001),
         (28, 'strict'): (12, 5, 0.0), (28, 'tol'): (33, 5, 0.001), (29, 'strict'): (11, 3, 0.0), (29, 'tol'): (2, 5, 0.0001)}
LATE_BUDGET = 40000          # problems scanned by find_late_empty()
# (family, seed) of the latest emptying and of the most emptying iterations in one fit, as find_late_empty() found them with
# scikit-learn 1.7.2 (one problem holds both records); None = scan again
LATE = [(1, 1755), (1, 1755)]
LATE_REPORT = ("40000 problems scanned; emptying E-steps by iteration {0: 25180, 1: 6566, 2: 1454, 3: 109, 4: 2}; "
               "latest at iteration 4 (1, 1755); most emptying iterations in one fit 5 (1, 1755)")


def fit(X, C0, max_iter=300, tol=1e-4):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return KMeans(n_clusters=C0.shape[0], init=np.asarray(C0, np.float64), n_init=1, max_iter=max_iter,
                      tol=tol).fit(X.astype(np.float64))


def run(name, X, C0, store, max_iter=300, tol=1e-4):
    Xd = X.astype(np.float64)
    km = fit(X, C0, max_iter, tol)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pred = km.predict(Xd)
    store[f"{name}/X"] = X
    store[f"{name}/C0"] = np.asarray(C0, np.float64)
    store[f"{name}/centers"] = km.cluster_centers_
    store[f"{name}/labels"] = km.labels_.astype(np.int32)
    store[f"{name}/predict"] = pred.astype(np.int32)
    store[f"{name}/inertia"] = np.float64(km.inertia_)
    store[f"{name}/n_iter"] = np.int32(km.n_iter_)
    store[f"{name}/max_iter"] = np.int32(max_iter)
    store[f"{name}/tol"] = np.float64(tol)
    print(name, X.shape, X.dtype, "k", len(C0), "n_iter", km.n_iter_, "inertia", km.inertia_,
          "counts", np.bincount(km.labels_, minlength=len(C0)))
    return km


# ------------------------------------------------------------------------------------------------ coverage
def coverage(S):
    for ti, dtype in enumerate((np.uint8, np.float32, np.float64)):
        for d in (1, 2, 3, 4):
            for k in (1, 2, 8, 9, 16):
                rng = np.random.default_rng(1000 * ti + 100 * d + k)
                N = 256 + 16 * d + (k + ti) % 4 + (1 if dtype is np.uint8 else 0)     # N % 4 takes every value
                cen = rng.uniform(20, 235, (k, d))
                X = cen[rng.integers(0, k, N)] + rng.normal(0, 9, (N, d))
                X = np.clip(X, 0, 255).astype(dtype)
                uniq = np.unique(X, axis=0)
                C0 = uniq[rng.choice(len(uniq), k, replace=False)].astype(np.float64) + rng.uniform(0.05, 0.45, (k, d))
                run(f"cov_{np.dtype(dtype).name}_d{d}_k{k}", X, C0, S)


# ------------------------------------------------------------------------------------------------ max_iter cuts
def blob_problem(seed, N=1500, k=5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, 2)).astype(np.float32)
    return X, X[:k].astype(np.float64)


def max_iter_cuts(S):
    seed = next(s for s in range(300) if fit(*blob_problem(s), tol=0.0).n_iter_ > 40)
    X, C0 = blob_problem(seed)
    free = run(f"maxit_free_seed{seed}", X, C0, S, tol=0.0)
    assert free.n_iter_ > 29
    for m in MAX_ITERS:
        km = run(f"maxit_{m:02d}", X, C0, S, max_iter=m, tol=0.0)
        assert km.n_iter_ == m


# ------------------------------------------------------------------------------------------------ natural stops
def stop_problem(seed, k):
    rng = np.random.default_rng(50_000 + seed)
    X = rng.standard_normal((600, 2)).astype(np.float32)
    return X, X[:k].astype(np.float64)


def find_stops():
    """first (seed, k, tol) per target iteration and kind.  A stop with tol > 0 counts as a tol stop only if the same
    problem with tol = 0 runs longer (otherwise the labels stopped it first)."""
    found = {}
    want = {(t, kind) for t in STOP_TARGETS for kind in ("strict", "tol")}
    for seed in range(4000):
        for k in (3, 5):
            X, C0 = stop_problem(seed, k)
            n0 = fit(X, C0, tol=0.0).n_iter_
            if (n0, "strict") in want and (n0, "strict") not in found:
                found[(n0, "strict")] = (seed, k, 0.0)
            if n0 > min(STOP_TARGETS):
                for tol in (1e-2, 1e-3, 1e-4):
                    n = fit(X, C0, tol=tol).n_iter_
                    if n < n0 and (n, "tol") in want and (n, "tol") not in found:
                        found[(n, "tol")] = (seed, k, tol)
        if len(found) == len(want):
            break
    return found


def natural_stops(S):
    stops = STOPS if STOPS is not None else find_stops()
    print("STOPS =", stops)
    for (n, kind), (seed, k, tol) in sorted(stops.items()):
        X, C0 = stop_problem(seed, k)
        km = run(f"stop_{n:02d}_{kind}_seed{seed}_k{k}", X, C0, S, tol=tol)
        assert km.n_iter_ == n
    for t in STOP_TARGETS:
        assert (t, "strict") in stops or (t, "tol") in stops, t
    assert any(kd == "strict" for _, kd in stops) and any(kd == "tol" for _, kd in stops)


# ------------------------------------------------------------------------------------------------ exact ties
def exact_labels(X, C):
    """argmin of the exact squared distances, lowest index on ties; also the number of exactly tied samples"""
    lab, ties = [], 0
    for x in X:
        dist = [sum((Fraction(int(a)) - Fraction(float(c))) ** 2 for a, c in zip(x, cj)) for cj in C]
        lab.append(dist.index(min(dist)))
        ties += dist.count(min(dist)) > 1
    return np.array(lab), ties


def tie_problem(C, members):
    """clusters given by their members: integer rows whose mean is the centre, tie samples listed with the LOWER index.
    Every cluster size is a power of two and every column sum is divisible by N, so centring, the expanded distances
    and the averaging are exact in binary floating point and C is a fixed point reached in one iteration."""
    C = np.asarray(C, np.float64)
    X = np.concatenate([np.asarray(m, np.int64).reshape(-1, C.shape[1]) for m in members])
    lab = np.concatenate([np.full(len(m), j) for j, m in enumerate(members)])
    assert np.all(X.sum(0) % len(X) == 0), "column sums not divisible by N"
    assert all(len(m) & (len(m) - 1) == 0 for m in members), "cluster sizes must be powers of two"
    perm = np.random.default_rng(len(X)).permutation(len(X))       # ties spread over the lanes
    X, lab = X[perm], lab[perm]
    got, n_tied = exact_labels(X, C)
    assert np.array_equal(got, lab), "the listed members are not the lowest-index argmin"
    for j in range(len(C)):
        assert np.all(X[lab == j].sum(0) == C[j] * (lab == j).sum()), "a centre is not the mean of its members"
    return X, C, lab, n_tied


def ties(S):
    # d = 2, integer centres.  (8,8) is equidistant from all three; (8,6) from c0, c1; (6,8) from c0, c2; (10,10) from c1, c2
    C = [[6, 6], [10, 6], [6, 10]]
    members = [[[8, 8], [4, 4], [8, 6], [4, 6], [6, 8], [6, 4], [5, 7], [7, 5]],
               [[10, 10], [10, 2], [11, 5], [9, 7]],
               [[5, 11], [7, 9], [6, 10], [6, 10]]]
    X, C, lab, n_tied = tie_problem(C, members)
    assert n_tied == 4
    for dtype in (np.uint8, np.float32, np.float64):
        km = run(f"tie_int_d2_k3_{np.dtype(dtype).name}", X.astype(dtype), C, S, tol=0.0)
        assert np.array_equal(km.labels_, lab) and km.n_iter_ == 1
    # d = 1, half-integer centres: 3 is equidistant from 1.5 and 4.5
    C = [[1.5], [4.5], [8.5]]
    members = [[[0], [3], [1], [2], [1], [2], [1], [2]], [[4], [5], [4], [5]], [[8], [9], [7], [10]]]
    X, C, lab, n_tied = tie_problem(C, members)
    assert n_tied == 1
    for dtype in (np.uint8, np.float64):
        km = run(f"tie_half_d1_k3_{np.dtype(dtype).name}", X.astype(dtype), C, S, tol=0.0)
        assert np.array_equal(km.labels_, lab) and km.n_iter_ == 1
    # d = 4, k = 9 (clusters 8.. use the masked lanes of the 16-wide instantiation): centres (4j+4, 8, 8, 8); cluster j < 8
    # owns the midpoint to its right neighbour, balanced by two samples on its left
    C = [[4 * j + 4, 8, 8, 8] for j in range(9)]
    members = [[[4 * j + 6, 8, 8, 8], [4 * j + 3, 9, 8, 8], [4 * j + 3, 7, 8, 8], [4 * j + 4, 8, 8, 8]] for j in range(8)]
    members.append([[36, 9, 8, 7], [36, 7, 8, 9], [36, 8, 8, 8], [36, 8, 8, 8]])
    X, C, lab, n_tied = tie_problem(C, members)
    assert n_tied == 8
    for dtype in (np.uint8, np.float32):
        km = run(f"tie_int_d4_k9_{np.dtype(dtype).name}", X.astype(dtype), C, S, tol=0.0)
        assert np.array_equal(km.labels_, lab) and km.n_iter_ == 1
    # duplicate rows in C0: the second copy is empty at iteration 0 and takes the farthest sample
    rng = np.random.default_rng(77)
    Xf = rng.standard_normal((515, 2)).astype(np.float32)
    C0 = np.stack([Xf[0], Xf[0], Xf[1]]).astype(np.float64)
    km = run("tie_dupC0_f32_k3", Xf, C0, S)
    assert np.bincount(km.labels_, minlength=3).min() > 0
    Xu = np.clip(rng.normal(128, 40, (1027, 4)), 0, 255).astype(np.uint8)
    C0 = np.stack([Xu[0], Xu[1], Xu[1], Xu[2], Xu[0]]).astype(np.float64)      # two pairs of duplicates
    km = run("tie_dupC0_u8_d4_k5", Xu, C0, S)
    assert np.bincount(km.labels_, minlength=5).min() > 0


# ------------------------------------------------------------------------------------------------ empty clusters
def sk_empty_iterations(X, C0, max_iter=40):
    """iterations (0-based) of sklearn's own Lloyd loop whose E-step leaves a cluster empty, and n_iter.  tol = 0."""
    Xd = np.ascontiguousarray(X, np.float64)
    mean = Xd.mean(axis=0)
    Xc = Xd - mean
    k = len(C0)
    sw = np.ones(len(Xc))
    cen, new = np.ascontiguousarray(C0 - mean), np.zeros((k, Xc.shape[1]))
    w, shift = np.zeros(k), np.zeros(k)
    lab, old, probe = np.full(len(Xc), -1, np.int32), np.full(len(Xc), -1, np.int32), np.full(len(Xc), -1, np.int32)
    empties = []
    for i in range(max_iter):
        lloyd_iter_chunked_dense(Xc, sw, cen, cen, w, probe, shift, 1, update_centers=False)
        if np.bincount(probe, minlength=k).min() == 0:
            empties.append(i)
        lloyd_iter_chunked_dense(Xc, sw, cen, new, w, lab, shift, 1)
        cen, new = new, cen
        if np.array_equal(lab, old) or (shift ** 2).sum() <= 0:
            break
        old[:] = lab
    return empties, i + 1


def late_problem(family, seed):
    rng = np.random.default_rng(900_000 * family + seed)
    if family == 0:        # few distinct u8 rows, many clusters, rows of X as the init
        N, d, k = int(rng.integers(20, 60)), int(rng.integers(1, 3)), int(rng.integers(4, 9))
        X = rng.integers(0, 6, (N, d)).astype(np.uint8) * 40
        C0 = X[rng.choice(N, k, replace=False)].astype(np.float64) + rng.uniform(-3, 3, (k, d))
    else:                  # the same with a duplicated init row: one cluster is empty at iteration 0 already
        N, d, k = int(rng.integers(24, 80)), int(rng.integers(1, 3)), int(rng.integers(4, 9))
        X = (rng.integers(0, 5, (N, d)) * 50 + rng.integers(0, 3, (N, d))).astype(np.uint8)
        C0 = X[rng.choice(N, k, replace=False)].astype(np.float64) + rng.uniform(-3, 3, (k, d))
        C0[k - 1] = C0[0]
    return X, C0


def find_late_empty():
    latest, most = (-1, None), (0, None)
    n_scanned, t0 = 0, time.time()
    hist = {}
    for family in (0, 1):
        for seed in range(LATE_BUDGET // 2):
            X, C0 = late_problem(family, seed)
            e, n = sk_empty_iterations(X, C0)
            n_scanned += 1
            if n >= 40 or len(np.unique(X, axis=0)) < len(C0):
                continue      # fewer distinct rows than clusters: sklearn relocates on rounding noise until max_iter
            for i in e:
                hist[i] = hist.get(i, 0) + 1
            if e and e[-1] > latest[0]:
                latest = (e[-1], (family, seed))
            if len(e) > most[0]:
                most = (len(e), (family, seed))
    print(f"scan took {time.time() - t0:.0f} s")
    report = (f"{n_scanned} problems scanned; emptying E-steps by iteration {dict(sorted(hist.items()))}; "
              f"latest at iteration {latest[0]} {latest[1]}; most emptying iterations in one fit {most[0]} {most[1]}")
    return [latest[1], most[1]], report


def confirm_empty_with_public_api(X, C0, iteration):
    """labels_ of KMeans(max_iter=m, tol=0) is the E-step of iteration m (0-based)"""
    if iteration == 0:
        return True
    km = fit(X, C0, max_iter=iteration, tol=0.0)
    return km.n_iter_ == iteration and np.bincount(km.labels_, minlength=len(C0)).min() == 0


def empties(S):
    rng = np.random.default_rng(5)
    B = rng.standard_normal((1027, 3))
    run("empty_it0_far_f64_d3_k4", B, np.array([[0, 0, 0], [1, 1, 1], [400, 400, 0], [-1, 0.5, 0.0]]), S)
    if LATE is not None:
        picks, report = LATE, LATE_REPORT
    else:
        picks, report = find_late_empty()
    print("LATE =", picks, "\n", report)
    S["late_empty_report"] = np.array(report)
    for tag, pick in zip(("latest", "most"), picks):
        if pick is None or (tag == "most" and pick == picks[0]):
            continue
        X, C0 = late_problem(*pick)
        e, n = sk_empty_iterations(X, C0)
        assert all(confirm_empty_with_public_api(X, C0, i) for i in e), (pick, e)
        run(f"empty_{tag}_at{'_'.join(map(str, e))}_fam{pick[0]}_seed{pick[1]}", X, C0, S, tol=0.0)
    # farthest distance 0: two distinct rows, both of them centres, and one far-away centre that stays empty.  It takes the
    # biggest cluster's entry of centers_new: already averaged when that cluster comes first, still the SUM when it comes
    # later (_average_centers works in place)
    X = np.array([[10, 20, 30, 40]] * 5 + [[200, 100, 50, 0]] * 11, np.uint8)[np.random.default_rng(1).permutation(16)]
    a, b, far = [10, 20, 30, 40], [200, 100, 50, 0], [255, 255, 255, 255]
    run("empty_dist0_after_biggest_u8", X, np.array([a, b, far], np.float64), S)
    run("empty_dist0_before_biggest_u8", X, np.array([far, a, b], np.float64), S)
    run("empty_dist0_two_empty_f64", X.astype(np.float64), np.array([far, a, [0, 255, 0, 255], b], np.float64), S)


# ------------------------------------------------------------------------------------------------ tolerance, precision
def precision(S):
    rng = np.random.default_rng(9)
    X = rng.uniform(0, 100, (16, 3))
    run("prec_N_eq_k_f64_k16", X, X[rng.permutation(16)] + rng.uniform(-0.1, 0.1, (16, 3)), S)
    X = rng.integers(0, 256, (5, 2)).astype(np.uint8)
    run("prec_N_eq_k_u8_k5", X, X[::-1].astype(np.float64) + 0.25, S)
    run("prec_const_u8_k2", np.full((203, 4), 7, np.uint8), np.array([[7, 7, 7, 7], [9, 9, 9, 9.0]]), S)
    run("prec_const_f32_k1", np.full((37, 2), 0.1, np.float32), np.array([[3.0, -2.0]]), S)
    B = rng.standard_normal((1001, 2)).astype(np.float32)
    km = run("prec_tol_stops_at_1_f32", B, B[:4].astype(np.float64), S, tol=10.0)
    assert km.n_iter_ == 1
    X = 1e6 + rng.standard_normal((1003, 3))
    run("prec_offset1e6_f64_k4", X, X[:4].copy(), S)
    X = (1e4 * rng.standard_normal((1002, 4))).astype(np.float32)
    run("prec_mag1e4_f32_k6", X, X[:6].astype(np.float64), S)


def main():
    S = {}
    coverage(S)
    max_iter_cuts(S)
    natural_stops(S)
    ties(S)
    empties(S)
    precision(S)
    S["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(OUT, **S)
    print(OUT, os.path.getsize(OUT), "bytes,", len({k.split('/')[0] for k in S if '/' in k}), "cases")
    assert os.path.getsize(OUT) < 1_000_000


if __name__ == "__main__":
    main()
