"""Generates tests/golden/lloyd_weighted_goldens.npz with the installed scikit-learn (1.7.2): Lloyd's k-means with sample
weights.  The call recorded is, as in make_lloyd_edge_goldens.py,

    KMeans(n_clusters=k, init=C0, n_init=1, max_iter=m, tol=t, algorithm='lloyd')
        .fit(X.astype(float64), sample_weight=w.astype(float64))

Only the vectors travel; sklearn is never imported by a test.  Keys of a case: X, w (in their storage dtypes), C0, centers,
labels, inertia, n_iter, max_iter, tol.  N <= 400 everywhere.

Families (the prefix of a case name):
  cov_     storage dtype u8 / f32 / f64 x d in 1..4 x k in {1, 2, 8, 9, 16} x weight dtype f32 / f64, uniform weights in [0.1, 3)
  int_     the same grid at d = 2 with integer weights 0..3
  size_    N mod 4 = 0, 1, 2, 3; N = k; N = 3
  maxit_   one fit cut at max_iter = 1, 2, 3, 5 (tol = 0)
  stop_    the same data stopped by tol = 1e-2 and 1e-3 before its labels settle
  reloc_   empty clusters: at iteration 0 with a relocated sample of weight 2.5; a cluster that owns only zero-weight samples
           (also cut at max_iter = 3); a relocated sample of weight 0; two empty clusters in one iteration; largest distance 0
  wide_    weights spanning 1e-6 .. 1e6

Every case is checked while it is generated: the float64 numpy model of tests/lloyd_weighted_cases.py reproduces sklearn
(labels, n_iter, centres, inertia), and the fit is well-conditioned (no sample of any E-step inside the rounding bound of
the expanded distance, every shift-against-tol decision a factor 2 from equality).  A case that fails the conditioning is
drawn again with the next seed.
"""
import os
import sys
import warnings

import numpy as np
import sklearn
from sklearn.cluster import KMeans

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lloyd_weighted_cases as M       # noqa: E402

OUT = os.path.join(HERE, "lloyd_weighted_goldens.npz")
DTYPES = (np.uint8, np.float32, np.float64)


def fit(X, w, C0, max_iter, tol):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return KMeans(n_clusters=len(C0), init=np.asarray(C0, np.float64), n_init=1, max_iter=max_iter, tol=tol,
                      algorithm="lloyd").fit(X.astype(np.float64), sample_weight=w.astype(np.float64))


def well_conditioned(X, w, C0, max_iter, tol):
    out, factor = M.conditioning(X, w, C0, max_iter, tol)
    return out == 0 and factor >= 2


def run(name, make, S, max_iter=300, tol=1e-4, accept=None):
    """make(seed) -> X, w, C0; the first seed whose fit is well-conditioned (and that accept(km) takes) is stored"""
    for seed in range(200):
        X, w, C0 = make(seed)
        C0 = np.asarray(C0, np.float64)
        if well_conditioned(X, w, C0, max_iter, tol) and (accept is None or accept(fit(X, w, C0, max_iter, tol))):
            break
    else:
        raise RuntimeError(f"{name}: no well-conditioned draw in 200 seeds")
    km = fit(X, w, C0, max_iter, tol)
    cen, lab, inertia, n_iter = M.model_fit(X, w, C0, max_iter, tol)
    assert n_iter == km.n_iter_ and np.array_equal(lab, km.labels_), name
    assert np.abs(cen - km.cluster_centers_).max() <= 1e-9 and abs(inertia - km.inertia_) <= 1e-10 * km.inertia_, name
    for key, v in (("X", X), ("w", w), ("C0", C0), ("centers", km.cluster_centers_), ("labels", km.labels_.astype(np.int32)),
                   ("inertia", np.float64(km.inertia_)), ("n_iter", np.int32(km.n_iter_)), ("max_iter", np.int32(max_iter)),
                   ("tol", np.float64(tol))):
        S[f"{name}/{key}"] = v
    print(name, X.shape, X.dtype, w.dtype, "k", len(C0), "seed", seed, "n_iter", km.n_iter_, "inertia", km.inertia_,
          "wk", np.round(np.bincount(km.labels_, weights=w.astype(np.float64), minlength=len(C0)), 3))
    return km, (X, w, C0)


def blobs(rng, N, d, k, dtype, spread=9.0):
    cen = rng.uniform(20, 235, (k, d))
    X = np.clip(cen[rng.integers(0, k, N)] + rng.normal(0, spread, (N, d)), 0, 255).astype(dtype)
    uniq = np.unique(X, axis=0)
    C0 = uniq[rng.choice(len(uniq), k, replace=False)].astype(np.float64) + rng.uniform(0.05, 0.45, (k, d))
    return X, C0


def coverage(S):
    for ti, dtype in enumerate(DTYPES):
        for d in (1, 2, 3, 4):
            for k in (1, 2, 8, 9, 16):
                for wdt in (np.float32, np.float64):
                    def make(seed, ti=ti, dtype=dtype, d=d, k=k, wdt=wdt):
                        rng = np.random.default_rng(100_000 * seed + 1000 * ti + 100 * d + k)
                        N = 64 + 8 * d + (k + ti) % 4 + (1 if dtype is np.uint8 else 0)      # N % 4 takes every value
                        X, C0 = blobs(rng, N, d, k, dtype)
                        return X, rng.uniform(0.1, 3.0, N).astype(wdt), C0
                    run(f"cov_{np.dtype(dtype).name}_d{d}_k{k}_w{np.dtype(wdt).name}", make, S)
    for ti, dtype in enumerate(DTYPES):
        for k in (1, 2, 8, 9, 16):
            for wdt in (np.float32, np.float64):
                def make(seed, ti=ti, dtype=dtype, k=k, wdt=wdt):
                    rng = np.random.default_rng(100_000 * seed + 7000 + 1000 * ti + k)
                    X, C0 = blobs(rng, 80 + (k + ti) % 4, 2, k, dtype)
                    return X, rng.integers(0, 4, len(X)).astype(wdt), C0
                run(f"int_{np.dtype(dtype).name}_d2_k{k}_w{np.dtype(wdt).name}", make, S)


def sizes(S):
    for N, k, tag in ((200, 3, "Nmod0"), (201, 3, "Nmod1"), (202, 3, "Nmod2"), (203, 3, "Nmod3"), (5, 5, "N_eq_k"), (3, 2, "N3")):
        def make(seed, N=N, k=k):
            rng = np.random.default_rng(100_000 * seed + 31 * N + k)
            X = rng.uniform(-50, 50, (N, 2)).astype(np.float32)
            C0 = X[rng.choice(N, k, replace=False)].astype(np.float64) + rng.uniform(0.05, 0.45, (k, 2))
            return X, rng.uniform(0.1, 3.0, N).astype(np.float32), C0
        run(f"size_{tag}", make, S)


def cuts_and_stops(S):
    def make(seed):
        rng = np.random.default_rng(100_000 * seed + 424242)
        X = rng.standard_normal((400, 2)).astype(np.float32)
        return X, rng.uniform(0.1, 3.0, 400), X[:5].astype(np.float64)
    seed0 = next(s for s in range(200) if fit(*make(s), 300, 0.0).n_iter_ > 8)
    free, _ = run("maxit_free", lambda s: make(seed0 + s), S, tol=0.0)
    for m in (1, 2, 3, 5):
        km, _ = run(f"maxit_{m:02d}", lambda s: make(seed0 + s), S, max_iter=m, tol=0.0)
        assert km.n_iter_ == m
    for tol in (1e-2, 1e-3):
        km, _ = run(f"stop_tol{tol:g}", lambda s: make(seed0 + s), S, tol=tol)
        assert km.n_iter_ < free.n_iter_


def relocations(S):
    def two_blobs(rng, n=60):
        a = rng.normal((0, 0), 1.0, (n, 2))
        b = rng.normal((20, 0), 1.0, (n, 2))
        return np.concatenate([a, b])

    def it0(seed):            # C0[2] far away: empty at iteration 0; the farthest sample (row 7) has weight 2.5
        rng = np.random.default_rng(100_000 * seed + 1)
        X = two_blobs(rng)
        X[7] = (-9.0, 6.0)
        w = rng.uniform(0.5, 1.5, len(X))
        w[7] = 2.5
        return X, w, [[0.5, 0.2], [19.0, 0.3], [400.0, 400.0]]
    km, (X, w, C0) = run("reloc_it0_w2p5_f64", it0, S)
    assert np.bincount(km.labels_, minlength=3).min() > 0

    def zero_cluster(seed):   # the third blob has weight 0 throughout: its cluster is empty although it owns samples
        rng = np.random.default_rng(100_000 * seed + 2)
        ab = np.concatenate([rng.normal((0, 0), 2.5, (60, 2)), rng.normal((8, 0), 2.5, (60, 2))])
        X = np.concatenate([ab, rng.normal((4, 30), 1.0, (30, 2))]).astype(np.float32)
        w = rng.uniform(0.5, 1.5, len(X)).astype(np.float32)
        w[120:] = 0
        X[3] = (-12.0, -9.0)
        return X, w, [[-2.0, 1.0], [3.0, -1.0], [4.0, 29.0]]
    seed0 = next(s for s in range(200) if fit(*zero_cluster(s), 300, 1e-4).n_iter_ > 4)      # so that max_iter = 3 cuts it
    km, _ = run("reloc_zero_weight_cluster_f32", lambda s: zero_cluster(seed0 + s), S, accept=lambda km: km.n_iter_ > 4)
    km, _ = run("reloc_zero_weight_cluster_f32_maxit3", lambda s: zero_cluster(seed0 + s), S, max_iter=3)
    assert km.n_iter_ == 3

    def sample_w0(seed):      # the relocated sample itself has weight 0: the cluster stays empty and copies the heaviest
        rng = np.random.default_rng(100_000 * seed + 3)
        X = two_blobs(rng)
        X[11] = (-12.0, 9.0)
        w = rng.uniform(0.5, 1.5, len(X))
        w[11] = 0
        return X, w, [[0.5, 0.2], [19.0, 0.3], [400.0, 400.0]]
    run("reloc_sample_weight0_f64", sample_w0, S)

    def two_empty(seed):      # two far-away centres: the two farthest samples (weights 0.25 and 1.75) move in one iteration
        rng = np.random.default_rng(100_000 * seed + 4)
        X = np.clip(two_blobs(rng) * 4 + 100, 0, 255)
        X[5], X[70] = (40, 160), (250, 30)
        w = rng.uniform(0.5, 1.5, len(X))
        w[5], w[70] = 0.25, 1.75
        return X.astype(np.uint8), w, [[100.5, 100.2], [180.0, 100.3], [255.0, 255.0], [0.0, 255.0]]
    km, _ = run("reloc_two_empty_u8", two_empty, S)
    assert np.bincount(km.labels_, minlength=4).min() > 0

    def dist0(seed):          # two distinct rows, both of them centres, one far-away centre: nothing to relocate
        rng = np.random.default_rng(100_000 * seed + 5)
        perm = rng.permutation(16)
        X = np.array([[10, 20, 30, 40]] * 5 + [[200, 100, 50, 0]] * 11, np.uint8)[perm]
        # weights 0.5 and 1 whose sum per row value is a power of two (4 and 8): the weighted means, hence the zero
        # inertia, are exact
        w = np.array([0.5, 0.5, 1, 1, 1] + [0.5] * 6 + [1.0] * 5)[perm]
        return X, w, [[255, 255, 255, 255], [10, 20, 30, 40], [200, 100, 50, 0]]
    run("reloc_dist0_u8_d4", dist0, S)


def wide(S):
    def make(seed):
        rng = np.random.default_rng(100_000 * seed + 6)
        X, C0 = blobs(rng, 300, 3, 4, np.float64)
        return X, 10.0 ** rng.uniform(-6, 6, 300), C0
    run("wide_1e-6_1e6_f64_d3_k4", make, S)

    def make32(seed):
        rng = np.random.default_rng(100_000 * seed + 7)
        X, C0 = blobs(rng, 300, 2, 5, np.float32)
        return X, (10.0 ** rng.uniform(-6, 6, 300)).astype(np.float32), C0
    run("wide_1e-6_1e6_f32_d2_k5_wf32", make32, S)


def main():
    S = {}
    coverage(S)
    sizes(S)
    cuts_and_stops(S)
    relocations(S)
    wide(S)
    S["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(OUT, **S)
    print(OUT, os.path.getsize(OUT), "bytes,", len({k.split('/')[0] for k in S if '/' in k}), "cases")
    assert os.path.getsize(OUT) < 735_000


if __name__ == "__main__":
    main()
