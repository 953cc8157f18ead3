"""KMeans -- the subset of sklearn.cluster.KMeans the reference's hot path uses
(color_kmeans.py:66-78, KmeanGrids.py:300-304: KMeans(n_clusters=k) -> .fit(X) -> .cluster_centers_,
.predict(X)), running Lloyd on the MI355X through libofc.

Semantics follow sklearn (cast to float64 math, centring, tol = 1e-4 * mean(var), strict-then-tol
convergence, final E-step, empty-cluster relocation).  One deliberate difference: the reference
constructs KMeans(n_clusters=k) with sklearn's default init='k-means++', random_state=None, i.e. a
non-deterministic seeding.  Here `init` is an explicit (k, d) array, 'seeded-rows'
(the default: k distinct rows of X picked by numpy's default_rng(random_state), seed 0 -- reproducible), or
'k-means++': sklearn's own seeding (_kmeans.py:174-272, on the device: kmeans_plusplus_dev) with numpy-RandomState-compatible draws, so that
KMeans(n_clusters=k, init='k-means++', random_state=s) lands on the centres sklearn finds for the same seed
(random_state=None then means numpy's global RandomState, as in sklearn).  For the reference's documented k=1
the result does not depend on the seeding at all."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, load, ptr

_DT = {np.dtype(np.uint8): _lib.U8, np.dtype(np.float32): _lib.F32, np.dtype(np.float64): _lib.F64}


def _as_supported(X):
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected 2D array, got {X.ndim}D array instead")
    if X.dtype not in _DT:
        X = X.astype(np.float64)          # sklearn: everything that is not f32/f64 becomes f64
    return np.ascontiguousarray(X)


def _as_weights(sample_weight, N):
    """sklearn's _check_sample_weight for KMeans.fit / score: None stays None, a scalar broadcasts, float32 stays float32
    and every other dtype becomes float64; a wrong length, a negative or non-finite weight, or a zero sum raise"""
    if sample_weight is None:
        return None
    w = np.asarray(sample_weight)
    if w.ndim == 0:
        w = np.full(N, w, dtype=w.dtype)
    if w.dtype != np.float32:
        w = w.astype(np.float64)
    if w.ndim != 1:
        raise ValueError("Sample weights must be 1D array or scalar")
    if w.shape != (N,):
        raise ValueError(f"sample_weight.shape == {w.shape}, expected {(N,)}!")
    if not np.isfinite(w).all():
        raise ValueError("Input sample_weight contains NaN or infinity.")
    if (w < 0).any():
        raise ValueError("Negative values in data passed to `sample_weight`")
    if N > 0 and not w.astype(np.float64).sum() > 0:
        raise ValueError("sum of sample weights must be positive")
    return np.ascontiguousarray(w)


def seeded_rows_init(X, k, random_state=0):
    """k distinct rows (by value, when there are enough distinct rows) picked by a seeded rng"""
    rng = np.random.default_rng(random_state)
    X = np.asarray(X)
    uniq = np.unique(X, axis=0)
    if len(uniq) >= k:
        return uniq[rng.choice(len(uniq), k, replace=False)].astype(np.float64)
    return X[rng.choice(len(X), k, replace=len(X) < k)].astype(np.float64)


def check_random_state(seed):
    """sklearn.utils.check_random_state: None -> numpy's global RandomState, int -> RandomState(seed)"""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)):
        return np.random.RandomState(int(seed))
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def kmeans_plusplus(X, n_clusters, random_state=None, n_local_trials=None, device=0, _step=None, sample_weight=None):
    """sklearn's _kmeans_plusplus (_kmeans.py:174-272) as KMeans.fit runs it: on the column-centred data, unit sample
    weights unless sample_weight is given (then, as KMeans.fit(X, sample_weight=) seeds: the weights decide the first
    centre, the distribution of every later draw and every candidate's potential; KMeans(init=C0).fit(X,
    sample_weight=w) from the returned centres is the two-step form of sklearn's weighted k-means++ fit).
    The O(N d trials) part of every step -- distances of all samples to the candidate rows, the minimum
    with the running closest distance, the candidates' potentials -- is one libofc launch (ofc_kpp_candidates); the
    RandomState draws, np.cumsum and searchsorted are numpy's, in sklearn's order.  -> (centres (k,d) f64 rows of X,
    indices).  The distances are not bit-identical to BLAS's (different summation order inside the dot product), so
    agreement with sklearn is exact unless a random value falls within ~1e-16 (relative) of a cumulative-sum
    boundary; tests/golden/kpp_goldens.npz pins it for a spread of seeds and shapes."""
    X = _as_supported(X)
    N, d = X.shape
    rs = check_random_state(random_state)
    if n_local_trials is None:
        n_local_trials = 2 + int(np.log(n_clusters))                              # :217-221
    if n_local_trials > 8:
        raise ValueError("n_local_trials > 8 is not supported")
    mean = X.astype(np.float64).mean(axis=0) if X.dtype != np.float32 else X.mean(axis=0).astype(np.float64)
    w = _as_weights(sample_weight, N)
    weight = np.ones(N, np.float64) if w is None else w.astype(np.float64)
    indices = np.full(n_clusters, -1, dtype=np.int64)
    indices[0] = rs.choice(N, p=weight / weight.sum())                            # :224

    def step(cand, closest):
        cand = np.ascontiguousarray(cand, np.int64)
        if _step is not None:                    # tests: the CPU oracle stands in for the device step
            return _step(X, mean, cand, closest)
        out = np.empty((len(cand), N), np.float64)
        pots = np.empty(len(cand), np.float64)
        check(load().ofc_kpp_candidates(device, ptr(X), _DT[X.dtype], N, d, ptr(mean), ptr(cand), len(cand),
                                        ptr(closest) if closest is not None else None, ptr(out), ptr(pots)))
        return out, pots

    out, pots = step(indices[:1], None)                                           # :233-236
    closest, current_pot = out[0], pots[0] if w is None else out[0] @ weight
    for c in range(1, n_clusters):
        rand_vals = rs.uniform(size=n_local_trials) * current_pot                  # :242
        cum = np.cumsum(closest if w is None else weight * closest, dtype=np.float64)
        candidate_ids = np.searchsorted(cum, rand_vals)                           # :243-245
        np.clip(candidate_ids, None, N - 1, out=candidate_ids)                    # :247
        out, pots = step(candidate_ids, closest)                                  # :250-256
        if w is not None:
            pots = out @ weight                                                   # :256
        best = int(np.argmin(pots))                                               # :259
        current_pot, closest = pots[best], out[best]
        indices[c] = candidate_ids[best]
    return X[indices].astype(np.float64), indices


KPP_CHOICE_MAX = 1 << 24      # largest global N whose first index is drawn with rs.choice (see kpp_draws)


def kpp_draws(rs, N, n_clusters, n_local_trials=None):
    """every random number _kmeans_plusplus consumes, drawn up front in sklearn's order (none of them depends on the
    data): the first index (:224), then uniform(size=n_local_trials) per further centre (:242).
    -> (first, u (n_clusters-1, n_local_trials), n_local_trials).
    Up to KPP_CHOICE_MAX rows the first index is sklearn's own rs.choice(N, p=uniform).  Above that it is
    min(int(rs.random_sample() * N), N - 1): choice draws that same single random_sample() and looks it up in the
    cumulative sum of p -- the same distribution, without three N-long float64 vectors (5 GB each for a clip)."""
    if n_local_trials is None:
        n_local_trials = 2 + int(np.log(n_clusters))                              # :217-221
    if n_local_trials > 8:
        raise ValueError("n_local_trials > 8 is not supported")
    if N <= KPP_CHOICE_MAX:
        weight = np.ones(N, np.float64)
        first = int(rs.choice(N, p=weight / weight.sum()))
    else:
        first = min(int(rs.random_sample() * N), N - 1)
    u = np.empty((n_clusters - 1, n_local_trials), np.float64)
    for c in range(n_clusters - 1):
        u[c] = rs.uniform(size=n_local_trials)
    return first, u, n_local_trials


def kpp_draws_w(rs, n_clusters, n_local_trials=None):
    """kpp_draws for the seeding with sample weights: the first centre is rs.choice(N, p=w / w.sum()), which consumes one
    random_sample() whatever N is and returns searchsorted(cumsum(p), that number, side='right').  That number is handed
    to the device, which looks it up in its own cumulative sum of the weights.
    -> (u_first, u (n_clusters-1, n_local_trials), n_local_trials)"""
    if n_local_trials is None:
        n_local_trials = 2 + int(np.log(n_clusters))                              # :217-221
    if n_local_trials > 8:
        raise ValueError("n_local_trials > 8 is not supported")
    u_first = float(rs.random_sample())
    u = np.empty((n_clusters - 1, n_local_trials), np.float64)
    for c in range(n_clusters - 1):
        u[c] = rs.uniform(size=n_local_trials)
    return u_first, u, n_local_trials


def kmeans_plusplus_dev(X_ptr, dtype, N, d, n_clusters, random_state=None, n_local_trials=None, device=0,
                        colsum=None, n_global=None, weights_ptr=None, weight_dtype=_lib.F32):
    """kmeans_plusplus on device-resident X (this rank's shard when a communicator is active: then n_global is the
    row count over all ranks, and every rank passes the same random_state).  The whole seeding runs in libofc
    (ofc_kpp_seed_dev): the closest distances stay on the device, each further centre costs one sweep over X.
    The draws are kpp_draws'.  colsum as for kmeans_fit_dev.
    weights_ptr: N device-resident sample weights of weight_dtype, as for kmeans_fit_dev: the seeding sklearn's
    fit(X, sample_weight=) runs (ofc_kpp_seed_dev_w, draws: kpp_draws_w); None: unit weights.
    -> (centres (k,d) f64 rows of X, GLOBAL indices)"""
    n_global = int(N if n_global is None else n_global)
    if n_global < 1:
        raise ValueError(f"n_samples={n_global} should be >= n_clusters={n_clusters}.")
    cs = np.ascontiguousarray(colsum, np.float64) if colsum is not None else None
    if cs is not None and cs.shape != (d,):
        raise ValueError(f"colsum must have shape ({d},)")
    centers = np.empty((n_clusters, d), np.float64)
    indices = np.empty(n_clusters, np.int64)
    if weights_ptr:
        u_first, u, n_local_trials = kpp_draws_w(check_random_state(random_state), int(n_clusters), n_local_trials)
        check(load().ofc_kpp_seed_dev_w(device, C.c_void_p(X_ptr), dtype, C.c_void_p(weights_ptr), weight_dtype, N, d,
                                        n_clusters, ptr(cs), u_first, ptr(u), n_local_trials, ptr(centers), ptr(indices)))
        return centers, indices
    first, u, n_local_trials = kpp_draws(check_random_state(random_state), n_global, int(n_clusters), n_local_trials)
    check(load().ofc_kpp_seed_dev(device, C.c_void_p(X_ptr), dtype, N, d, n_clusters, ptr(cs), first, ptr(u),
                                  n_local_trials, ptr(centers), ptr(indices)))
    return centers, indices


class KMeans:
    """n_init is stored for sklearn's signature and ignored: fit() runs once from `init`.  Restarts are offered where they
    cost next to nothing, on the (u,v) histogram of a field: uvhist.UVHistogram.fit(k, n_init=...)."""

    def __init__(self, n_clusters=8, *, init="seeded-rows", n_init=1, max_iter=300, tol=1e-4,
                 random_state=0, device=0, **_ignored):
        self.n_clusters, self.init, self.n_init = int(n_clusters), init, n_init
        self.max_iter, self.tol, self.random_state, self.device = int(max_iter), float(tol), random_state, device

    def _init_centers(self, X):
        if isinstance(self.init, str):
            if self.init == "k-means++":
                return None                      # fit seeds on the uploaded X
            if self.init not in ("seeded-rows", "random"):
                raise ValueError(f"init should be an array, 'k-means++' or 'seeded-rows', got {self.init!r}")
            return seeded_rows_init(X, self.n_clusters, self.random_state if self.random_state is not None else 0)
        C0 = np.ascontiguousarray(self.init, np.float64)
        if C0.shape != (self.n_clusters, X.shape[1]):
            raise ValueError(f"The shape of the initial centers {C0.shape} does not match "
                             f"({self.n_clusters}, {X.shape[1]})")
        return C0

    def fit(self, X, y=None, sample_weight=None):
        X = _as_supported(X)
        N, d = X.shape
        k = self.n_clusters
        if N < k:
            raise ValueError(f"n_samples={N} should be >= n_clusters={k}.")
        w = _as_weights(sample_weight, N)
        if w is not None and isinstance(self.init, str) and self.init == "k-means++":
            raise ValueError("sample_weight together with init='k-means++' is not supported in one call (pass an "
                             "explicit init or 'seeded-rows'; for sklearn's weighted seeding: C0, _ = kmeans_plusplus(X, k, "
                             "random_state=s, sample_weight=w), then KMeans(k, init=C0).fit(X, sample_weight=w))")
        C0 = self._init_centers(X)          # 'seeded-rows' ignores the weights, as sklearn's array init does
        centers = np.empty((k, d), np.float64)
        labels = np.empty(N, np.int32)
        inertia, n_iter = C.c_double(), C.c_int()
        if C0 is None:                           # 'k-means++': one upload serves the seeding and the fit
            Xd = _lib.DeviceBuffer(X.nbytes, self.device)
            Ld = _lib.DeviceBuffer(N, self.device)
            try:
                Xd.upload(X)
                C0, _ = kmeans_plusplus_dev(Xd.ptr, _DT[X.dtype], N, d, k, self.random_state, device=self.device)
                check(load().ofc_kmeans_fit_dev(self.device, C.c_void_p(Xd.ptr), _DT[X.dtype], N, d, k, ptr(C0),
                                                self.max_iter, self.tol, ptr(centers), C.c_void_p(Ld.ptr),
                                                C.byref(inertia), C.byref(n_iter)))
                labels[:] = Ld.download((N,), np.uint8)
            finally:
                Xd.free()
                Ld.free()
        elif w is not None:
            check(load().ofc_kmeans_fit_w(self.device, ptr(X), _DT[X.dtype], ptr(w), _DT[w.dtype], N, d, k, ptr(C0),
                                          self.max_iter, self.tol, ptr(centers), ptr(labels), C.byref(inertia),
                                          C.byref(n_iter)))
        else:
            check(load().ofc_kmeans_fit(self.device, ptr(X), _DT[X.dtype], N, d, k, ptr(C0), self.max_iter,
                                        self.tol, ptr(centers), ptr(labels), C.byref(inertia), C.byref(n_iter)))
        self.cluster_centers_, self.labels_ = centers, labels
        self.inertia_, self.n_iter_ = inertia.value, n_iter.value
        self.n_features_in_ = d
        return self

    def predict(self, X):
        X = _as_supported(X)
        N, d = X.shape
        if d != self.cluster_centers_.shape[1]:
            raise ValueError(f"X has {d} features, but KMeans is expecting {self.cluster_centers_.shape[1]}")
        labels = np.empty(N, np.int32)
        cen = np.ascontiguousarray(self.cluster_centers_, np.float64)
        check(load().ofc_kmeans_predict(self.device, ptr(X), _DT[X.dtype], N, d, self.n_clusters, ptr(cen), ptr(labels)))
        return labels

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_

    def score(self, X, y=None, sample_weight=None):
        """sklearn's KMeans.score: minus the (weighted) inertia of X against cluster_centers_"""
        X = _as_supported(X)
        N, d = X.shape
        if d != self.cluster_centers_.shape[1]:
            raise ValueError(f"X has {d} features, but KMeans is expecting {self.cluster_centers_.shape[1]}")
        w = _as_weights(sample_weight, N)
        cen = np.ascontiguousarray(self.cluster_centers_, np.float64)
        inertia = C.c_double()
        check(load().ofc_kmeans_score(self.device, ptr(X), _DT[X.dtype], ptr(w), _DT[w.dtype] if w is not None else _lib.F32,
                                      N, d, self.n_clusters, ptr(cen), C.byref(inertia)))
        return -inertia.value


def kmeans_fit_dev(X_ptr, dtype, N, d, init, max_iter=300, tol=1e-4, labels_ptr=None, device=0, colsum=None,
                   weights_ptr=None, weight_dtype=_lib.F32, field=None):
    """device-resident X (this rank's shard when a communicator is active).  colsum: this rank's column sums when the
    caller already has them (the flow engine emits sum(u), sum(v) with the field): the fit then skips that sweep.
    weights_ptr: N device-resident sample weights of weight_dtype (F32 or F64; finite, >= 0, not all zero over the ranks),
    sklearn's fit(X, sample_weight=); None: the unweighted fit.
    field=(W, H): X is a stack of N / (W*H) whole float32 (u,v) fields of that size (ofc_kmeans_fit_dev_field): the same
    result, and the tile sweeps cut the fields in 2-D where W % 64 == 0 and H % 8 == 0.  A weighted fit ignores it (its
    sweeps read every sample).
    -> centers (k,d), inertia, n_iter"""
    C0 = np.ascontiguousarray(init, np.float64)
    k = C0.shape[0]
    centers = np.empty((k, d), np.float64)
    inertia, n_iter = C.c_double(), C.c_int()
    cs = np.ascontiguousarray(colsum, np.float64) if colsum is not None else None
    if cs is not None and cs.shape != (d,):
        raise ValueError(f"colsum must have shape ({d},)")
    if weights_ptr:
        check(load().ofc_kmeans_fit_dev_w(device, C.c_void_p(X_ptr), dtype, C.c_void_p(weights_ptr), weight_dtype, N, d, k, ptr(C0),
                                          max_iter, tol, ptr(cs), ptr(centers), C.c_void_p(labels_ptr) if labels_ptr else None,
                                          C.byref(inertia), C.byref(n_iter)))
        return centers, inertia.value, n_iter.value
    if field is not None:
        W, H = (int(v) for v in field)
        if W < 1 or H < 1 or N % (W * H):
            raise ValueError(f"field={field!r}: N={N} is not a whole number of {W}x{H} fields")
        check(load().ofc_kmeans_fit_dev_field(device, C.c_void_p(X_ptr), dtype, N, d, k, ptr(C0), max_iter, tol, ptr(cs),
                                              ptr(centers), C.c_void_p(labels_ptr) if labels_ptr else None, C.byref(inertia),
                                              C.byref(n_iter), W, H, N // (W * H)))
        return centers, inertia.value, n_iter.value
    check(load().ofc_kmeans_fit_dev_stats(device, C.c_void_p(X_ptr), dtype, N, d, k, ptr(C0), max_iter, tol, ptr(cs), ptr(centers),
                                          C.c_void_p(labels_ptr) if labels_ptr else None, C.byref(inertia), C.byref(n_iter)))
    return centers, inertia.value, n_iter.value


def prune_stats(device=0):
    """how the last kmeans_fit_dev on `device` swept its samples (ofc_lloyd_prune_stats): tile sweeps, how many of them
    pruned, how many counting-only (probe), the tiles the pruned sweeps tested and skipped in all, and their share"""
    out = np.zeros(6, np.float64)
    check(load().ofc_lloyd_prune_stats(device, ptr(out)))
    return {"tile_sweeps": int(out[0]), "pruned_sweeps": int(out[1]), "probe_sweeps": int(out[4]), "final_pruned": bool(out[5]),
            "tiles_tested": int(out[2]), "tiles_pure": int(out[3]),
            "skip_fraction": float(out[3] / out[2]) if out[2] > 0 else 0.0}
