"""Shared by the weighted-Lloyd tests and by tests/golden/make_lloyd_weighted_goldens.py (no test in here):

  model_fit        scikit-learn 1.7.2's KMeans(init=C0, n_init=1, algorithm='lloyd').fit(X, sample_weight=w) in float64 numpy
  conditioning     how far a fit stays from the decisions that rounding could flip
  NumpyShard       a numpy-backed weighted shard for sharded.fit_sharded
  large_case       the one generated input that is too large to store

What the weights change (scikit-learn 1.7.2):
  centring, tol    nothing: X.mean(axis=0), mean(var(X)) * tol over the row count       _kmeans.py:1479-1484, :279-287
  E-step           nothing
  M-step           sums[label] += x_c * w (multiply, then add), wk[label] += w          _k_means_lloyd.pyx
  empty cluster    wk[j] == 0 (a cluster of zero-weight samples is empty)               _k_means_common.pyx:165-210
  relocation       farthest samples by UNWEIGHTED distance to their old centre; sums[old] -= x*w, sums[new] = x*w,
                   wk[new] = w, wk[old] -= w; skipped when the largest distance is 0
  average          wk[j] > 0: sums * (1 / wk), else the heaviest cluster's row (in place)   _average_centers
  stop             labels == labels_old, else shift <= tol                              _kmeans.py:716-728
  inertia          sum w_i |x_i - c_label|^2                                            _inertia_dense
"""
import threading

import numpy as np

U = 2.0 ** -53


def np_sum_small(a):
    """numpy's pairwise sum for n <= 128, as sharded._np_sum_small"""
    a = [float(v) for v in a]
    n = len(a)
    if n < 8:
        r = 0.0
        for v in a:
            r += v
        return r
    r = a[:8]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] += a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res += v
    return res


def e_step(Xc, c):
    """labels: first minimum of the expanded distance |c|^2 - 2 x.c"""
    return np.argmin((c * c).sum(1)[None, :] - 2.0 * (Xc @ c.T), axis=1).astype(np.int32)


def sq_dist_grouped(a, b):
    """row-wise squared distance in _euclidean_dense_dense's grouping (four terms at a time, then the rest one by one)"""
    t = (a - b) ** 2
    d = t.shape[1]
    r = np.zeros(len(t))
    f = 0
    while f + 4 <= d:
        r += (t[:, f] + t[:, f + 1] + t[:, f + 2] + t[:, f + 3])
        f += 4
    while f < d:
        r += t[:, f]
        f += 1
    return r


def m_step(Xc, w, labels, k):
    sums = np.stack([np.bincount(labels, weights=Xc[:, f] * w, minlength=k) for f in range(Xc.shape[1])], axis=1)
    return sums, np.bincount(labels, weights=w, minlength=k)


def relocate(Xc, w, c_old, labels, sums, wk):
    """_relocate_empty_clusters_dense.  The n_empty farthest samples in descending order of distance (ties: the lower
    index), which is what argpartition(...)[:-n_empty-1:-1] gives for up to two empty clusters and distinct distances"""
    empty = np.flatnonzero(wk == 0)
    if len(empty) == 0:
        return
    dist = ((Xc - c_old[labels]) ** 2).sum(axis=1)
    if dist.max() == 0:
        return
    far = np.lexsort((np.arange(len(dist)), -dist))[:len(empty)]
    for j, i in zip(empty, far):
        old = labels[i]
        xw = Xc[i] * w[i]
        sums[old] -= xw
        sums[j] = xw
        wk[j] = w[i]
        wk[old] -= w[i]


def average(sums, wk):
    cnew = sums.copy()
    amax = int(np.argmax(wk))
    for j in range(len(wk)):
        if wk[j] > 0:
            cnew[j] = cnew[j] * (1.0 / wk[j])
        else:
            cnew[j] = cnew[amax]
    return cnew


def model_fit(X, w, C0, max_iter=300, tol=1e-4, trace=None):
    """-> centers (k,d), labels (N,) i32, inertia, n_iter.  trace: a list that receives one dict per E-step
    (centred samples, centres) and per stop decision (shift, tol)"""
    Xd = np.asarray(X, np.float64)
    w = np.asarray(w, np.float64)
    C0 = np.asarray(C0, np.float64)
    k = len(C0)
    mean = Xd.mean(axis=0)
    tol_abs = 0.0 if tol == 0 else np.mean(np.var(Xd, axis=0)) * tol
    Xc = Xd - mean
    c = C0 - mean
    labels_old = np.full(len(Xd), -1, np.int32)
    labels = labels_old
    strict, it = False, 0
    for it in range(max_iter):
        if trace is not None:
            trace.append({"kind": "e", "Xc": Xc, "c": c.copy()})
        labels = e_step(Xc, c)
        sums, wk = m_step(Xc, w, labels, k)
        relocate(Xc, w, c, labels, sums, wk)
        cnew = average(sums, wk)
        shift = np_sum_small([np.sqrt(v) ** 2 for v in sq_dist_grouped(cnew, c)])
        c = cnew
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if trace is not None:
            trace.append({"kind": "stop", "shift": shift, "tol": tol_abs})
        if shift <= tol_abs:
            break
        labels_old = labels
    if not strict:
        if trace is not None:
            trace.append({"kind": "e", "Xc": Xc, "c": c.copy()})
        labels = e_step(Xc, c)
    inertia = float(np.sum(sq_dist_grouped(Xc, c[labels]) * w))
    return c + mean, labels, inertia, it + 1


def model_score(X, w, centers):
    """KMeans.score: minus the weighted inertia of the UNCENTRED X against `centers`"""
    Xd = np.asarray(X, np.float64)
    c = np.asarray(centers, np.float64)
    w = np.ones(len(Xd)) if w is None else np.asarray(w, np.float64)
    return -float(np.sum(sq_dist_grouped(Xd, c[e_step(Xd, c)]) * w))


# ------------------------------------------------------------------------------------------------ conditioning
def expanded_bound(xc, C):
    """B[i][j] = (d + 4) u (|x|^2 + |c_j|^2 + 2 sum_f |x_f c_f|): the rounding bound of the expanded distance derived in
    tests/test_oracle_lloyd_independent.py (its expanded_bound, on centred samples)"""
    d = xc.shape[1]
    cross = np.abs(xc)[:, None, :] * np.abs(C)[None, :, :]
    return (d + 4) * U * ((xc * xc).sum(1)[:, None] + (C * C).sum(1)[None, :] + 2 * cross.sum(2))


def left_out(xc, C):
    """samples whose two smallest squared distances to DISTINCT centre rows differ by less than 2 max B (the rule of
    exact_labels_wide, direct form in long double).  Bit-identical centre rows (a still-empty cluster takes a copy of the
    heaviest one's centre) have bit-identical distances: the lower index wins on every implementation."""
    C = np.unique(np.asarray(C, np.float64), axis=0)
    if len(C) < 2:
        return 0
    xl, Cl = np.asarray(xc, np.longdouble), np.asarray(C, np.longdouble)
    D = np.zeros((len(xl), len(Cl)), np.longdouble)
    for f in range(xl.shape[1]):
        D += (xl[:, f, None] - Cl[None, :, f]) ** 2
    part = np.partition(D, 1, axis=1)
    thr = 2 * expanded_bound(np.asarray(xc, np.float64), C).max(axis=1) * (1 + 2.0 ** -8)
    return int(np.count_nonzero(part[:, 1] - part[:, 0] < thr))


def conditioning(X, w, C0, max_iter=300, tol=1e-4):
    """-> (samples left out over all E-steps of the fit, smallest factor between shift and tol over its stop decisions).
    A shift of exactly 0 (equal labels give bit-equal sums) is a decision no rounding can flip: factor inf."""
    trace = []
    model_fit(X, w, C0, max_iter, tol, trace)
    out, factor = 0, np.inf
    for t in trace:
        if t["kind"] == "e":
            out += left_out(t["Xc"], t["c"])
        elif t["shift"] != 0 and t["tol"] != 0:
            factor = min(factor, max(t["shift"] / t["tol"], t["tol"] / t["shift"]))
    return out, factor


# ------------------------------------------------------------------------------------------------ fit_sharded backend
class NumpyShard:
    """the four shard-local passes of sharded.fit_sharded in numpy, with sample weights"""

    def __init__(self, X, w):
        self.Xd, self.w = np.asarray(X, np.float64), np.asarray(w, np.float64)
        self.N, self.d = self.Xd.shape
        self.labels = np.full(self.N, 255, np.int32)

    def colstats(self, mean, pass_):
        return self.Xd.sum(axis=0) if pass_ == 0 else ((self.Xd - mean) ** 2).sum(axis=0)

    def step(self, mean, centers_c, accumulate=True):
        c = np.asarray(centers_c, np.float64)
        k = len(c)
        Xc = self.Xd - mean
        lab = e_step(Xc, c) if self.N else np.zeros(0, np.int32)
        rec = np.zeros(k * self.d + k + 1)
        if accumulate:
            sums, wk = m_step(Xc, self.w, lab, k)
            rec[:k * self.d], rec[k * self.d:k * self.d + k] = sums.ravel(), wk
            rec[k * self.d + k] = np.count_nonzero(lab != self.labels)
        self.labels = lab
        return rec

    def inertia(self, mean, centers_c):
        c = np.asarray(centers_c, np.float64)
        return float(np.sum(sq_dist_grouped(self.Xd - mean, c[self.labels]) * self.w))

    def farthest(self, mean, centers_c, excl):
        c = np.asarray(centers_c, np.float64)
        Xc = self.Xd - mean
        dist = ((Xc - c[self.labels]) ** 2).sum(axis=1)
        dist[list(excl)] = -1
        if self.N == 0 or dist.max() < 0:
            return -1.0, -1, np.zeros(self.d), -1, 0.0
        i = int(np.argmax(dist))
        return float(dist[i]), i, Xc[i], int(self.labels[i]), float(self.w[i])


def threaded_allreduce(world):
    """-> one allreduce(arr, op) per rank for `world` threads of one process (rank order = operand order)"""
    barrier = threading.Barrier(world)
    slots = [None] * world
    fn = {"sum": np.add, "max": np.maximum, "min": np.minimum}

    def make(rank):
        def allreduce(arr, op):
            slots[rank] = np.array(arr, np.float64)
            barrier.wait(timeout=60)
            r = slots[0]
            for q in range(1, world):
                r = fn[op](r, slots[q])
            barrier.wait(timeout=60)
            return r
        return allreduce
    return [make(r) for r in range(world)]


# ------------------------------------------------------------------------------------------------ the large case
LARGE_N = 4 * (262144 + 256 + 37) + 3      # 1024 work-groups x 256 lanes: lanes 0..292 take a second quad, 3 samples remain


def large_case(seed=0):
    """f32, d = 2, k = 3: integer-valued populations far apart, dyadic f32 weights in [0, 3] (a twelfth of them 0).
    -> X (N,2) f32, w (N,) f32, C0 (3,2).  Reseed here if the conditioning test ever fails; never skip there."""
    rng = np.random.default_rng(20_000 + seed)
    pop = rng.integers(0, 3, LARGE_N)
    cen = np.array([[-40, -30], [0, 50], [60, -10]], np.float64)
    X = (cen[pop] + rng.integers(-6, 7, (LARGE_N, 2))).astype(np.float32)
    w = (rng.integers(0, 25, LARGE_N) / 8.0).astype(np.float32)
    w[rng.integers(0, 12, LARGE_N) == 0] = 0
    C0 = np.array([[-30.0, -20.5], [5.25, 35.0], [45.5, 0.75]])
    return X, w, C0
