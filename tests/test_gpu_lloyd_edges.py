"""The Lloyd kernels, their drivers and the k-means++ step at their edges, through the C ABI.

ofc_kmeans_fit / _predict / _fit_dev / _fit_dev_stats run every case of tests/golden/lloyd_edge_goldens.npz (sklearn 1.7.2)
and the oracle, with test_gpu_lloyd.py's bars: labels and n_iter exact, centres <= 1e-9, inertia <= 1e-10 relative.  The
building blocks sharded.py stands on -- ofc_lloyd_colstats_dev, _step_dev, _inertia_dev, _farthest_dev -- and
ofc_kpp_candidates are compared one call at a time with the exact definitions of test_oracle_lloyd_independent.py (direct
form, exact argmin with its left-out rule, math.fsum, integers), not with the oracle's restatement of the same algebra.
A labelling step always runs before inertia / farthest, so every label is below k (the precondition in include/ofc.h).
"""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_oracle_lloyd_independent import (CASES, LEFT_OUT_CAP, TIE_CASES, Z, check_kpp, check_record, direct_terms,
                                                 exact_labels, exact_labels_wide, near_duplicates, sum_bound)

pytestmark = pytest.mark.gpu
NS = (0, 1, 3, 4, 5, 255, 1027, 262_147)
DTYPES = (np.uint8, np.float32, np.float64)


@pytest.fixture(scope="module")
def L():
    from opticalflowclustering_amd import _lib
    _lib.load()
    return _lib


def data(dtype, d, N, seed=0):
    rng = np.random.default_rng(1000 * d + seed + np.dtype(dtype).itemsize)
    if dtype == np.uint8:
        return rng.integers(0, 256, (N, d), dtype=np.uint8)
    cen = rng.uniform(-40, 60, (6, d))
    return (cen[rng.integers(0, 6, N)] + rng.normal(0, 5, (N, d))).astype(dtype)


def centres(X, k, seed=0):
    """k centred centres spread over the data; never on a sample"""
    rng = np.random.default_rng(k + seed)
    lo, hi = (0.0, 255.0) if X.dtype == np.uint8 else (-50.0, 70.0)
    return rng.uniform(lo, hi, (k, X.shape[1])) + 0.123


class Shard:
    """X resident on the device + sharded.DeviceShard (labels start at 0xFF)"""

    def __init__(self, L, X):
        from opticalflowclustering_amd.cluster import _DT
        from opticalflowclustering_amd.sharded import DeviceShard
        self.L, self.X = L, np.ascontiguousarray(X)
        self.buf = L.DeviceBuffer(max(self.X.nbytes, 16))
        if len(self.X):
            self.buf.upload(self.X)
        self.dt = _DT[self.X.dtype]
        self.s = DeviceShard(self.buf.ptr, self.dt, len(self.X), self.X.shape[1])

    def labels(self):
        out = np.empty(len(self.X), np.uint8)
        if len(out):
            self.L.check(self.L.load().ofc_memcpy_d2h(0, self.L.ptr(out), self.s.labels, len(out)))
        return out

    def set_labels(self, lab):
        lab = np.ascontiguousarray(lab, np.uint8)
        if len(lab):
            self.L.check(self.L.load().ofc_memcpy_h2d(0, self.s.labels, self.L.ptr(lab), len(lab)))


def mean_of(X):
    return X.astype(np.float64).sum(0) / max(len(X), 1)


def reference_labels(X, mean, Cc):
    if len(X) == 0:
        return np.zeros(0, np.int32), np.zeros(0, bool)
    if len(X) <= 300:
        lab, out, _ = exact_labels(X, mean, Cc)
        return lab, out
    return exact_labels_wide(X, mean, Cc)


# ------------------------------------------------------------------------------------------------ the fits
@pytest.mark.parametrize("name", CASES)
def test_fit_and_predict_match_sklearn_and_the_oracle(L, name):
    from opticalflowclustering_amd.cluster import KMeans
    X, C0 = Z[name + "/X"], Z[name + "/C0"]
    max_iter, tol = int(Z[name + "/max_iter"]), float(Z[name + "/tol"])
    km = KMeans(n_clusters=len(C0), init=C0, max_iter=max_iter, tol=tol).fit(X)
    pred = km.predict(X)
    want = (Z[name + "/centers"], Z[name + "/labels"], float(Z[name + "/inertia"]), int(Z[name + "/n_iter"]))
    for cen, lab, inertia, n_iter in (want, O.kmeans_fit(X, C0, max_iter, tol)):
        assert km.n_iter_ == n_iter
        assert np.array_equal(km.labels_, lab)
        assert np.abs(km.cluster_centers_ - cen).max() <= 1e-9
        assert abs(km.inertia_ - inertia) <= 1e-10 * inertia
    assert np.array_equal(pred, Z[name + "/predict"])
    assert np.array_equal(pred, O.kmeans_predict(X, km.cluster_centers_))


FIT_DEV_CASES = ["cov_uint8_d4_k16", "cov_float32_d2_k9", "cov_float64_d3_k8", "cov_uint8_d1_k2", "maxit_12", "stop_13_tol_seed1_k5",
                 "tie_dupC0_u8_d4_k5", "prec_offset1e6_f64_k4"] + [c for c in CASES if c.startswith("empty_latest")]


@pytest.mark.parametrize("name", FIT_DEV_CASES)
def test_fit_dev_with_and_without_labels_and_with_supplied_column_sums(L, name):
    from opticalflowclustering_amd.cluster import kmeans_fit_dev
    X, C0 = Z[name + "/X"], Z[name + "/C0"]
    kw = dict(max_iter=int(Z[name + "/max_iter"]), tol=float(Z[name + "/tol"]))
    sh = Shard(L, X)
    N, d = X.shape
    a = kmeans_fit_dev(sh.buf.ptr, sh.dt, N, d, C0, **kw)                                  # labels_dev == NULL
    b = kmeans_fit_dev(sh.buf.ptr, sh.dt, N, d, C0, labels_ptr=sh.s.labels, **kw)
    colsum = sh.s.colstats(None, 0)
    c = kmeans_fit_dev(sh.buf.ptr, sh.dt, N, d, C0, labels_ptr=sh.s.labels, colsum=colsum, **kw)
    for r in (b, c):                                                                        # bit-equal
        assert np.array_equal(r[0], a[0]) and r[1] == a[1] and r[2] == a[2]
    assert a[2] == int(Z[name + "/n_iter"])
    assert np.array_equal(sh.labels().astype(np.int32), Z[name + "/labels"])
    assert np.abs(a[0] - Z[name + "/centers"]).max() <= 1e-9
    assert abs(a[1] - float(Z[name + "/inertia"])) <= 1e-10 * float(Z[name + "/inertia"])


@pytest.mark.parametrize("N,tiled", [((1 << 20) - 1, False), (1 << 20, True)])
def test_tile_sweeps_start_at_two_to_the_twenty_samples(L, monkeypatch, N, tiled):
    """default environment, a coherent (u,v) field: below 2^20 samples no sweep goes tile by tile, from 2^20 on they do;
    either way the fit is the oracle's"""
    from opticalflowclustering_amd.cluster import kmeans_fit_dev, prune_stats
    monkeypatch.delenv("OFC_LLOYD_PRUNE", raising=False)
    rng = np.random.default_rng(20)
    vel = np.array([[-3.0, 0.5], [0.25, 0.0], [2.5, -1.5]])
    region = (np.arange(N) * 3) // N                                   # three contiguous regions: tiles lie inside one cell
    X = (vel[region] + 0.05 * rng.standard_normal((N, 2))).astype(np.float32)
    C0 = vel + np.array([[0.4, -0.3], [-0.2, 0.3], [0.1, 0.2]])
    sh = Shard(L, X)
    cen, inertia, n_iter = kmeans_fit_dev(sh.buf.ptr, sh.dt, N, 2, C0, labels_ptr=sh.s.labels)
    sweeps = prune_stats()["tile_sweeps"]
    assert (sweeps > 0) if tiled else (sweeps == 0)
    ocen, olab, oin, on = O.kmeans_fit(X, C0)
    assert n_iter == on and np.array_equal(sh.labels().astype(np.int32), olab)
    assert np.abs(cen - ocen).max() <= 1e-9 and abs(inertia - oin) <= 1e-10 * oin


# ------------------------------------------------------------------------------------------------ column statistics
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_colstats_against_fsum(L, dtype, d):
    big = data(dtype, d, max(NS))
    for N in NS:
        X = big[:N].copy()
        sh = Shard(L, X)
        s0 = sh.s.colstats(None, 0)
        Xd = X.astype(np.float64)
        mean = s0 / max(N, 1)
        s1 = sh.s.colstats(mean, 1)
        for f in range(d):
            if dtype == np.uint8:
                assert s0[f] == float(X[:, f].astype(np.int64).sum()), (N, f)       # exact integer
            else:
                assert abs(s0[f] - math.fsum(Xd[:, f])) <= sum_bound(Xd[:, f]), (N, f)
            t = Xd[:, f] - mean[f]
            t = t * t
            assert abs(s1[f] - math.fsum(t)) <= sum_bound(t), (N, f, s1[f], math.fsum(t))


# ------------------------------------------------------------------------------------------------ one step
def run_step(L, sh, mean, Cc, accumulate=1, record=None):
    k, d = Cc.shape
    rec = np.zeros(k * d + k + 1) if record is None else record
    L.check(L.load().ofc_lloyd_step_dev(0, C.c_void_p(sh.buf.ptr), sh.dt, len(sh.X), d, k, L.ptr(np.ascontiguousarray(mean)),
                                        L.ptr(np.ascontiguousarray(Cc)), C.c_void_p(sh.s.labels), accumulate, L.ptr(rec)))
    return rec


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_step_labels_record_and_n_changed(L, dtype, d):
    """every k in {1, 8, 9, 16} at every N up to 1027, one k at N = 262 147 (the scalar tail is N % 4 in 1..3)"""
    big = data(dtype, d, max(NS), seed=1)
    n_all = n_out = 0
    for N in NS:
        X = big[:N].copy()
        mean = mean_of(X)
        for k in ((1, 8, 9, 16) if N < max(NS) else ((8, 9, 16, 1)[d - 1],)):
            what = (np.dtype(dtype).name, d, N, k)
            Cc = centres(X, k) - mean
            sh = Shard(L, X)
            want, out = reference_labels(X, mean, Cc)
            rec = run_step(L, sh, mean, Cc)
            got = sh.labels().astype(np.int32)
            assert np.array_equal(got[~out], want[~out]), what
            assert N == 0 or got.max() < k, what
            assert rec[-1] == N, what                                            # from all-0xFF labels
            check_record(rec, X, mean, Cc, np.full(N, 255), got, what)
            rec2 = run_step(L, sh, mean, Cc)
            assert rec2[-1] == 0 and np.array_equal(rec2[:-1], rec[:-1]) and np.array_equal(sh.labels(), got), what
            # accumulate = 0: labels only, the record is not written
            keep = np.full(k * d + k + 1, -7.5)
            run_step(L, sh, mean, Cc, accumulate=0, record=keep)
            assert np.all(keep == -7.5) and np.array_equal(sh.labels(), got), what
            if k > 1:                                                            # move one centre
                C2 = Cc.copy()
                C2[k - 1] = 0.5 * (Cc[k - 1] + Cc[0]) + 0.01
                want2, out2 = reference_labels(X, mean, C2)
                rec3 = run_step(L, sh, mean, C2)
                got2 = sh.labels().astype(np.int32)
                assert np.array_equal(got2[~out2], want2[~out2]), what
                assert rec3[-1] == np.count_nonzero(got2 != got), what
                if not out.any() and not out2.any():
                    assert rec3[-1] == np.count_nonzero(want2 != want), what
                check_record(rec3, X, mean, C2, got, got2, what)
                n_all, n_out = n_all + N, n_out + int(out2.sum())
            n_all, n_out = n_all + N, n_out + int(out.sum())
    print("step %s d=%d: %d of %d samples left out (share %.2e)" % (np.dtype(dtype).name, d, n_out, n_all, n_out / n_all))
    assert n_out / n_all <= LEFT_OUT_CAP


@pytest.mark.parametrize("name", TIE_CASES)
def test_step_exact_ties_go_to_the_lower_index(L, name):
    X, C0 = Z[name + "/X"], Z[name + "/C0"]
    mean = X.astype(np.float64).sum(0) / len(X)
    want, out, tied = exact_labels(X, mean, C0 - mean, ties_exact=True)
    assert tied >= 1
    sh = Shard(L, X)
    rec = run_step(L, sh, mean, C0 - mean)
    assert np.array_equal(sh.labels().astype(np.int32), want)
    check_record(rec, X, mean, C0 - mean, np.full(len(X), 255), want, name)
    # a tie in the scalar tail and in the vector body: the same rows repeated to N % 4 == 3
    Xr = np.concatenate([X] * 8)[: 8 * len(X) - 1]
    wr = np.concatenate([want] * 8)[: len(Xr)]
    shr = Shard(L, Xr)
    run_step(L, shr, mean, C0 - mean)
    assert np.array_equal(shr.labels().astype(np.int32), wr)


# ------------------------------------------------------------------------------------------------ inertia
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_inertia_of_arbitrary_valid_labels_against_fsum(L, dtype, d):
    big = data(dtype, d, max(NS), seed=2)
    for N in NS:
        k = (16, 9, 1, 8)[(d + N) % 4]
        X = big[:N].copy()
        mean = mean_of(X)
        Cc = centres(X, k, seed=3) - mean
        sh = Shard(L, X)
        run_step(L, sh, mean, Cc)                                               # every label < k from here on
        for lab in (sh.labels().astype(np.int64), np.random.default_rng(N).integers(0, k, N)):
            sh.set_labels(lab)
            got = sh.s.inertia(mean, Cc)
            t = direct_terms(X, mean, Cc, lab) if N else np.zeros(0)
            assert abs(got - math.fsum(t)) <= sum_bound(t), (N, k, got, math.fsum(t))


# ------------------------------------------------------------------------------------------------ farthest sample
def far_dist(X, mean, Cc, lab):
    """the kernel's own expression, one IEEE operation after the other: s += ((x - m) - c)^2"""
    t = (X.astype(np.float64) - mean) - Cc[lab]
    s = np.zeros(len(X))
    for f in range(X.shape[1]):
        s = s + t[:, f] * t[:, f]
    return s


@pytest.mark.parametrize("dtype,d,N", [(np.uint8, 4, 1027), (np.float32, 2, 262_147), (np.float64, 3, 5), (np.float32, 1, 255),
                                       (np.float64, 4, 1)])
def test_farthest_unique_maximum(L, dtype, d, N):
    X = data(dtype, d, N, seed=4)
    mean, k = mean_of(X), min(N, 5)
    Cc = centres(X, k, seed=5) - mean
    sh = Shard(L, X)
    run_step(L, sh, mean, Cc)
    lab = sh.labels().astype(np.int64)
    s = far_dist(X, mean, Cc, lab)
    order = np.argsort(-s, kind="stable")
    if N > 1:
        assert s[order[0]] > s[order[1]]
    d2, idx, xc, l = sh.s.farthest(mean, Cc, [])
    assert (idx, d2, l) == (order[0], s[order[0]], lab[order[0]])
    assert np.array_equal(xc, X[idx].astype(np.float64) - mean)
    if N > 1:                                                                 # excluding the winner gives the runner-up
        d2, idx, xc, l = sh.s.farthest(mean, Cc, [int(order[0])])
        assert (idx, d2, l) == (order[1], s[order[1]], lab[order[1]])


def test_farthest_equal_maxima_lowest_index_and_exclusions(L):
    """262 147 u8 samples, one centre at 0 with mean 0: distances are exact integers.  The sweep gives sample i to lane
    i % 256 of work-group (i / 256) % 256 (262 147 / 4 quads over 256 work-groups of 256 lanes).  Equal maxima sit in two lanes of
    one group (5, 200), in another group (300), in the same lane one stride later (5 + 65 536) and at the very end
    (262 146)."""
    N = 262_147
    X = np.random.default_rng(6).integers(0, 100, (N, 1), dtype=np.uint8)
    planted = [5, 200, 300, 5 + 65_536, 70_000, 262_146] + list(range(100_000, 100_000 + 12 * 257, 257))
    X[planted] = 200
    assert len(planted) == 18 and planted[:3] == sorted(planted[:3])
    mean, Cc = np.zeros(1), np.zeros((1, 1))
    sh = Shard(L, X)
    run_step(L, sh, mean, Cc)
    excl, ranked = [], sorted(planted)
    for n in range(17):                                        # n_excl = 0 .. 16: always the lowest index not excluded
        d2, idx, xc, l = sh.s.farthest(mean, Cc, excl)
        assert (d2, idx, xc[0], l) == (40000.0, ranked[n], 200.0, 0), (n, idx)
        excl.append(idx)
    assert len(excl) == 17
    d2, idx = C.c_double(), C.c_int64()
    lab, xc = C.c_int(), np.zeros(1)
    ex = np.array(excl, np.int64)
    rc = L.load().ofc_lloyd_farthest_dev(0, C.c_void_p(sh.buf.ptr), sh.dt, N, 1, 1, L.ptr(mean), L.ptr(Cc), C.c_void_p(sh.s.labels),
                                         L.ptr(ex), 17, C.byref(d2), C.byref(idx), L.ptr(xc), C.byref(lab))
    assert rc == L.OFC_EINVAL and b"exclusion" in L.load().ofc_last_error()
    # the exclusion list in another order, the winner last
    d2v, i, _, _ = sh.s.farthest(mean, Cc, ranked[1:16][::-1] + [ranked[0]])
    assert (d2v, i) == (40000.0, ranked[16])


def test_farthest_with_every_sample_excluded(L):
    X = data(np.float32, 2, 5, seed=7)
    mean = mean_of(X)
    Cc = centres(X, 2) - mean
    sh = Shard(L, X)
    run_step(L, sh, mean, Cc)
    d2, idx, xc, lab = sh.s.farthest(mean, Cc, [4, 2, 0, 1, 3])
    assert (d2, idx, lab) == (-1.0, -1, -1)
    sh0 = Shard(L, X[:0])
    d2, idx, xc, lab = sh0.s.farthest(mean, Cc, [])
    assert (d2, idx, lab) == (-1.0, -1, -1)


def test_farthest_twins_in_two_work_groups_and_the_fit_that_relocates_one(L):
    """4096 f32 samples (4 work-groups) in two tight clusters, and the same far point at indices 100 and 3000, which lie in
    different work-groups.  The third initial centre is where nobody is nearest: the farthest pick must name index 100, and
    the fit relocates the empty cluster onto the far point (sklearn: iteration 0 moves it there, iteration 1 gives it both
    twins, whose mean is the point itself)."""
    from opticalflowclustering_amd.cluster import KMeans
    N, far = 4096, np.array([5.0, 50.0], np.float32)
    rng = np.random.default_rng(12)
    X = (np.array([[0.0, 0.0], [10.0, 0.0]])[np.arange(N) % 2] + 0.01 * rng.standard_normal((N, 2))).astype(np.float32)
    X[[100, 3000]] = far
    C0 = np.array([[0.0, 0.1], [10.0, 0.1], [5.0, -1000.0]])
    mean = mean_of(X)
    sh = Shard(L, X)
    run_step(L, sh, mean, C0 - mean)
    lab = sh.labels()
    assert lab[100] == lab[3000] and 2 not in lab
    d2, idx, xc, l = sh.s.farthest(mean, C0 - mean, [])
    assert np.array_equal(idx, 100) and l == lab[100] and np.array_equal(xc, far.astype(np.float64) - mean)
    d2b, idx, _, _ = sh.s.farthest(mean, C0 - mean, [100])
    assert np.array_equal(idx, 3000) and d2b == d2
    km = KMeans(n_clusters=3, init=C0).fit(X)
    cen, olab, inertia, n_iter = O.kmeans_fit(X, C0)
    assert km.n_iter_ == n_iter and np.array_equal(km.labels_, olab)
    assert np.array_equal(np.flatnonzero(km.labels_ == 2), [100, 3000])
    assert np.abs(km.cluster_centers_ - cen).max() <= 1e-9 and np.abs(km.cluster_centers_[2] - far).max() <= 1e-9
    assert abs(km.inertia_ - inertia) <= 1e-10 * inertia


# ------------------------------------------------------------------------------------------------ k-means++ step
def run_kpp(L, X, mean, cand, closest):
    from opticalflowclustering_amd.cluster import _DT
    out, pots = np.full((len(cand), len(X)), np.nan), np.full(len(cand), np.nan)
    L.check(L.load().ofc_kpp_candidates(0, L.ptr(X), _DT[X.dtype], len(X), X.shape[1], L.ptr(mean), L.ptr(cand), len(cand),
                                        L.ptr(closest) if closest is not None else None, L.ptr(out), L.ptr(pots)))
    return out, pots


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_kpp_candidates_against_exact_distances(L, dtype, d):
    big = data(dtype, d, 100_003, seed=8)
    for N in (1, 257, 100_003):
        X = big[:N].copy()
        mean = mean_of(X)
        rng = np.random.default_rng(N + d)
        combos = [(1, False), (1, True), (8, False), (8, True)] if N == 257 else \
                 [(1, False), (1, True)] if N == 1 else [((1, False), (8, True))[(d + np.dtype(dtype).itemsize) % 2]]
        for n_cand, with_closest in combos:
            cand = rng.integers(0, N, n_cand).astype(np.int64)               # repeats allowed (N = 1: all the same row)
            base, _ = run_kpp(L, X, mean, cand[:1], None)
            closest = base[0] * rng.uniform(0.2, 1.8, N) if with_closest else None
            out, pots = run_kpp(L, X, mean, cand, closest)
            check_kpp(out, pots, X, mean, cand, closest, (np.dtype(dtype).name, d, N, n_cand, with_closest), own_exact=True)


def test_kpp_clamps_the_expanded_form_at_zero(L):
    X = near_duplicates(257, 3)
    mean = mean_of(X)
    cand = np.arange(8, dtype=np.int64)
    out, pots = run_kpp(L, X, mean, cand, None)
    assert np.all(out >= 0.0)
    check_kpp(out, pots, X, mean, cand, None, "near duplicates", own_exact=True)


def test_kpp_refuses_bad_candidate_lists(L):
    X = data(np.float32, 2, 257)
    mean, out, pots = mean_of(X), np.zeros((9, 257)), np.zeros(9)
    lib = L.load()

    def call(cand, n_cand, d=2, Xp=X):
        cand = np.asarray(cand, np.int64)
        return lib.ofc_kpp_candidates(0, L.ptr(Xp), L.F32, 257, d, L.ptr(mean), L.ptr(cand), n_cand, None, L.ptr(out), L.ptr(pots))

    assert call([0], 0) == L.OFC_EINVAL and b"n_cand" in lib.ofc_last_error()
    assert call(list(range(9)), 9) == L.OFC_EINVAL and b"n_cand" in lib.ofc_last_error()
    assert call([257], 1) == L.OFC_EINVAL and b"candidate" in lib.ofc_last_error()
    assert call([3, -1], 2) == L.OFC_EINVAL and b"candidate" in lib.ofc_last_error()
    assert call([0], 1, d=5, Xp=np.zeros((257, 5), np.float32)) == L.OFC_EUNSUPPORTED
    assert call([0], 1) == L.OFC_OK


# ------------------------------------------------------------------------------------------------ refusals
def test_every_entry_point_refuses_what_it_cannot_do(L):
    """d = 5 or k = 17: OFC_EUNSUPPORTED; null pointers and N < k: OFC_EINVAL; each with a message"""
    lib = L.load()
    N = 64
    X5, X2 = np.zeros((N, 5), np.float32), data(np.float32, 2, N)
    dev = L.DeviceBuffer(X5.nbytes).upload(X5)
    labd = L.DeviceBuffer(N)
    L.check(lib.ofc_memset(0, C.c_void_p(labd.ptr), 0, N))
    init, cen = np.zeros((17, 5)), np.zeros((17, 5))
    lab32, lab8 = np.zeros(N, np.int32), C.c_void_p(labd.ptr)
    inertia, n_iter, d2, idx, li = C.c_double(), C.c_int(), C.c_double(), C.c_int64(), C.c_int()
    out, mean, p, X = np.zeros(5 * 17 + 18), np.zeros(5), L.ptr, C.c_void_p(dev.ptr)
    ex = np.zeros(16, np.int64)

    def calls(d, k, Xh=X5, Xd=X, init=init, cen=cen, out=out, lab32=lab32, inertia=C.byref(inertia), d2=C.byref(d2), N=N, mean=mean):
        return {
            "fit": lambda: lib.ofc_kmeans_fit(0, p(Xh), L.F32, N, d, k, p(init), 10, 1e-4, p(cen), p(lab32), inertia, C.byref(n_iter)),
            "predict": lambda: lib.ofc_kmeans_predict(0, p(Xh), L.F32, N, d, k, p(cen), p(lab32)),
            "fit_dev": lambda: lib.ofc_kmeans_fit_dev(0, Xd, L.F32, N, d, k, p(init), 10, 1e-4, p(cen), lab8, inertia, C.byref(n_iter)),
            "fit_dev_stats": lambda: lib.ofc_kmeans_fit_dev_stats(0, Xd, L.F32, N, d, k, p(init), 10, 1e-4, None, p(cen), lab8, inertia,
                                                                  C.byref(n_iter)),
            "colstats": lambda: lib.ofc_lloyd_colstats_dev(0, Xd, L.F32, N, d, p(mean), 1, p(out)),
            "step": lambda: lib.ofc_lloyd_step_dev(0, Xd, L.F32, N, d, k, p(mean), p(cen), lab8, 1, p(out)),
            "inertia": lambda: lib.ofc_lloyd_inertia_dev(0, Xd, L.F32, N, d, k, p(mean), p(cen), lab8, inertia),
            "farthest": lambda: lib.ofc_lloyd_farthest_dev(0, Xd, L.F32, N, d, k, p(mean), p(cen), lab8, p(ex), 0, d2, C.byref(idx), p(out),
                                                           C.byref(li)),
        }

    for d, k in ((5, 3), (2, 17)):
        for name, f in calls(d, k).items():
            if name == "colstats" and d != 5:
                continue
            assert f() == L.OFC_EUNSUPPORTED, (name, d, k)
            assert lib.ofc_last_error(), name
    # null pointers
    for name, kw in (("fit", dict(Xh=None)), ("predict", dict(lab32=None)), ("fit_dev", dict(init=None)), ("fit_dev_stats", dict(cen=None)),
                     ("colstats", dict(out=None)), ("colstats", dict(mean=None)), ("step", dict(out=None)), ("inertia", dict(inertia=None)),
                     ("farthest", dict(d2=None)), ("step", dict(Xd=None))):
        assert calls(2, 3, **kw)[name]() == L.OFC_EINVAL, (name, kw)
        assert lib.ofc_last_error(), name
    # fewer samples than clusters
    dev2 = L.DeviceBuffer(X2.nbytes).upload(X2)
    for name in ("fit", "fit_dev", "fit_dev_stats"):
        assert calls(2, 3, Xh=X2, Xd=C.c_void_p(dev2.ptr), N=2)[name]() == L.OFC_EINVAL, name
        assert b"n_samples=2" in lib.ofc_last_error(), name
    assert calls(2, 3, Xh=X2, Xd=C.c_void_p(dev2.ptr))["fit_dev"]() == L.OFC_OK
