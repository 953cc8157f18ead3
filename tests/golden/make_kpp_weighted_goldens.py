"""Generates tests/golden/kpp_weighted_goldens.npz with the installed scikit-learn (1.7.2): k-means++ seeding with sample
weights, on the data of make_kpp_goldens.py.  Per case

    indices              _kmeans_plusplus(Xc, k, row_norms(Xc, squared=True), w.astype(float64), RandomState(seed)) on the
                         column-centred X.astype(float64), exactly as KMeans.fit calls it (_kmeans.py:1478-1510)
    centers, labels,     KMeans(n_clusters=k, init='k-means++', n_init=1, random_state=seed)
    inertia, n_iter          .fit(X.astype(float64), sample_weight=w.astype(float64))

X is stored once per family (X/<family>), the weights per case in their storage dtype.  Only the vectors travel; sklearn is
never imported by a test.  Weight kinds:
  mag     magnitude-like, f32: the row's length
  mov     "moving"-like, f32 0/1 with about 70 % zeros
  int     small integers 0..3, f64

Every case is checked while it is generated: the fit from the seeded rows is well-conditioned in the sense of
tests/lloyd_weighted_cases.conditioning -- no sample of any E-step inside the rounding bound of the expanded distance, every
shift-against-tol decision at least 1 % from equality (the shift's own rounding error is some 1e-13 of it; these fits take
tens of iterations, so the factor 2 of the Lloyd goldens would leave no seed for some of them) -- a seed whose fit is not
is passed over for the next one.  The float64 numpy model of the fit reproduces sklearn's fit from the seeded rows."""
import os
import sys
import warnings

import numpy as np
from sklearn.cluster import KMeans
from sklearn.cluster._kmeans import _kmeans_plusplus
from sklearn.utils.extmath import row_norms

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lloyd_weighted_cases as M       # noqa: E402

OUT = os.path.join(HERE, "kpp_weighted_goldens.npz")


def case(name, family, X, w, k, seed, S):
    Xd = X.astype(np.float64)
    wd = w.astype(np.float64)
    Xc = Xd - Xd.mean(axis=0)
    _, idx = _kmeans_plusplus(Xc, k, row_norms(Xc, squared=True), wd, np.random.RandomState(seed))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=k, init="k-means++", n_init=1, random_state=seed).fit(Xd, sample_weight=wd)
    out, factor = M.conditioning(X, w, Xd[idx])
    if not (out == 0 and factor >= 1.01):
        print(name, "not well-conditioned", out, factor, "-- next seed")
        return False
    cen, lab, inertia, n_iter = M.model_fit(X, w, Xd[idx])
    assert n_iter == km.n_iter_ and np.array_equal(lab, km.labels_), name
    assert np.abs(cen - km.cluster_centers_).max() <= 1e-9 and abs(inertia - km.inertia_) <= 1e-10 * km.inertia_, name
    S[f"{name}/family"] = np.array(family)
    S[f"{name}/w"] = w
    S[f"{name}/k"] = np.int32(k)
    S[f"{name}/seed"] = np.int32(seed)
    S[f"{name}/indices"] = idx.astype(np.int64)
    S[f"{name}/centers"] = km.cluster_centers_
    S[f"{name}/labels"] = km.labels_.astype(np.uint8)
    S[f"{name}/inertia"] = np.float64(km.inertia_)
    S[f"{name}/n_iter"] = np.int32(km.n_iter_)
    print(name, X.shape, X.dtype, w.dtype, "zeros", int((w == 0).sum()), "k", k, "seed", seed, "indices", idx, "n_iter", km.n_iter_)
    return True


def main():
    rng = np.random.default_rng(5)
    S = {}
    # the three data sets of make_kpp_goldens.py, drawn in its order
    cell = np.zeros((2601, 4), np.uint8)
    m = rng.random(2601) < 0.3
    cell[m, :3] = rng.integers(30, 256, (m.sum(), 3))
    cell[m, 3] = 255
    cen = np.array([[-3, -3], [-1.5, 1], [0, 0], [1.5, -1], [3, 3]], np.float64)
    blob = (cen[rng.integers(0, 5, 6000)] + 0.35 * rng.standard_normal((6000, 2)))
    img = rng.integers(0, 256, (4096, 4), dtype=np.uint8)
    S["X/cell"], S["X/blob"], S["X/img"] = cell, blob, img

    wr = np.random.default_rng(17)

    def weights(X):
        length = np.sqrt((X.astype(np.float64) ** 2).sum(axis=1))
        mov = (length >= np.quantile(length, 0.7)).astype(np.float32)
        if X is cell:
            mov = (length > 0).astype(np.float32)          # the black background does not move
        return {"mag": length.astype(np.float32), "mov": mov, "int": wr.integers(0, 4, len(X)).astype(np.float64)}

    # per data set and weight kind: the first `count` seeds whose fit is well-conditioned
    for fam, X, k, count in (("cell", cell, 3, 2), ("blob", blob, 5, 1), ("img", img, 3, 1)):
        for kind, w in weights(X).items():
            n = count + (1 if (fam, kind) == ("blob", "mov") else 0)
            for seed in range(100):
                if n and case(f"{fam}_{kind}_k{k}_s{seed}", fam, X, w, k, seed, S):
                    n -= 1
            assert n == 0
    np.savez_compressed(OUT, **S)
    print("wrote", OUT, os.path.getsize(OUT), "bytes", len([k for k in S if k.endswith("/k")]), "cases")


if __name__ == "__main__":
    main()
