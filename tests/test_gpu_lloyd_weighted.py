"""Lloyd's k-means with sample weights on the MI355X (lloyd_weighted.hip, the weighted paths of lloyd_fit.cpp, cluster.py,
sharded.py, pipeline.py) against scikit-learn 1.7.2's goldens (tests/golden/make_lloyd_weighted_goldens.py) and the float64
numpy model of tests/lloyd_weighted_cases.py, which tests/test_lloyd_weighted_host.py pins to those goldens.

Bars unless a test says otherwise: labels bit-equal, n_iter equal, centres <= 1e-9, inertia <= 1e-10 relative.
Sums of n terms t_i are compared with math.fsum within (n - 1) 2^-53 sum |t_i|, the bound for any summation order
(tests/test_oracle_lloyd_independent.py).

ofc_flow_weights_dev, kind "magnitude": the test asserts 1 f32 ulp against numpy's f32 expression and prints how many
values differ at all.  Measured on the MI355X: 0 of 1 200 003, i.e. bit-equal (the device's sqrtf is correctly rounded).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import lloyd_weighted_cases as M

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "lloyd_weighted_goldens.npz"))
CASES = sorted({k.split("/")[0] for k in Z.files if "/" in k})
U = 2.0 ** -53


def case(name):
    return (Z[name + "/X"], Z[name + "/w"], Z[name + "/C0"], int(Z[name + "/max_iter"]), float(Z[name + "/tol"]))


def assert_golden(name, cen, lab, inertia, n_iter):
    ref = float(Z[name + "/inertia"])
    assert n_iter == int(Z[name + "/n_iter"]), name
    assert np.array_equal(np.asarray(lab, np.int32), Z[name + "/labels"]), name
    assert np.abs(cen - Z[name + "/centers"]).max() <= 1e-9, name
    assert abs(inertia - ref) <= 1e-10 * ref, (name, inertia, ref)


def sum_bound(terms):
    terms = np.asarray(terms, np.float64)
    return max(len(terms) - 1, 0) * U * math.fsum(np.abs(terms))


class Resident:
    """X, w (and a label buffer) on the device"""

    def __init__(self, X, w=None):
        from opticalflowclustering_amd import _lib
        from opticalflowclustering_amd.cluster import _DT
        self.X = np.ascontiguousarray(X if X.dtype in _DT else X.astype(np.float64))
        self.N, self.d = self.X.shape
        self.dtype = _DT[self.X.dtype]
        self.xb = _lib.DeviceBuffer(max(self.X.nbytes, 16)).upload(self.X)
        self.lb = _lib.DeviceBuffer(max(self.N, 1))
        self.wb, self.wdtype = None, _lib.F32
        if w is not None:
            w = np.ascontiguousarray(w)
            self.wdtype = _DT[w.dtype]
            self.wb = _lib.DeviceBuffer(max(w.nbytes, 16)).upload(w)

    @property
    def wptr(self):
        return self.wb.ptr if self.wb is not None else None

    def fit(self, C0, max_iter=300, tol=1e-4):
        from opticalflowclustering_amd.cluster import kmeans_fit_dev
        cen, inertia, n_iter = kmeans_fit_dev(self.xb.ptr, self.dtype, self.N, self.d, C0, max_iter, tol, self.lb.ptr,
                                              weights_ptr=self.wptr, weight_dtype=self.wdtype)
        return cen, self.labels(), inertia, n_iter

    def labels(self):
        return self.lb.download((self.N,), np.uint8)

    def free(self):
        for b in (self.xb, self.lb, self.wb):
            if b is not None:
                b.free()


@pytest.fixture(scope="module")
def large():
    """the large case, its model fit (computed once, read-only) and its device copy"""
    X, w, C0 = M.large_case()
    ref = M.model_fit(X, w, C0, 300, 0.0)
    r = Resident(X, w)
    yield X, w, C0, ref, r
    r.free()


# ------------------------------------------------------------------------------------------------ the goldens
@pytest.mark.parametrize("name", CASES)
def test_kmeans_fit_sample_weight_matches_sklearn(name):
    from opticalflowclustering_amd.cluster import KMeans
    X, w, C0, max_iter, tol = case(name)
    km = KMeans(n_clusters=len(C0), init=C0, max_iter=max_iter, tol=tol).fit(X, sample_weight=w)
    assert_golden(name, km.cluster_centers_, km.labels_, km.inertia_, km.n_iter_)


@pytest.mark.parametrize("name", CASES)
def test_fit_dev_w_matches_sklearn(name):
    X, w, C0, max_iter, tol = case(name)
    r = Resident(X, w)
    try:
        assert_golden(name, *r.fit(C0, max_iter, tol))
    finally:
        r.free()


def test_scalar_weight_broadcasts_and_fit_predict_takes_weights():
    from opticalflowclustering_amd.cluster import KMeans
    X, w, C0, max_iter, tol = case("cov_float32_d2_k8_wfloat32")
    a = KMeans(n_clusters=8, init=C0).fit(X, sample_weight=2.5)
    b = KMeans(n_clusters=8, init=C0).fit(X, sample_weight=np.full(len(X), 2.5))
    assert a.n_iter_ == b.n_iter_ and np.array_equal(a.labels_, b.labels_) and np.array_equal(a.cluster_centers_, b.cluster_centers_)
    assert np.array_equal(KMeans(n_clusters=8, init=C0).fit_predict(X, sample_weight=w), Z["cov_float32_d2_k8_wfloat32/labels"])


# ------------------------------------------------------------------------------------------------ unit weights, no weights
def medium_case():
    rng = np.random.default_rng(3)
    N = 4 * 70_000 + 1                          # several work-groups, a one-sample tail
    cen = np.array([[-3.0, 1.0], [2.0, 2.5], [0.5, -3.0], [5.0, -1.0]])
    X = (cen[rng.integers(0, 4, N)] + rng.normal(0, 0.7, (N, 2))).astype(np.float32)
    return X, cen + rng.uniform(-0.4, 0.4, cen.shape)


@pytest.mark.parametrize("wdtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["medium", "cov_uint8_d4_k16_wfloat32", "cov_float64_d3_k9_wfloat64", "reloc_two_empty_u8",
                                  "maxit_03"])
def test_unit_weights_equal_the_unweighted_fit(monkeypatch, name, wdtype):
    """w = 1 against the plain sweeps (OFC_LLOYD_PRUNE=0): x * 1 is x and the weight sums are the counts, so only the
    order of the adds may differ (it does not: same lanes, same folds; the bar leaves room for the 128-lane shape)"""
    monkeypatch.setenv("OFC_LLOYD_PRUNE", "0")
    X, C0 = medium_case() if name == "medium" else (Z[name + "/X"], Z[name + "/C0"])
    max_iter = 300 if name == "medium" else int(Z[name + "/max_iter"])
    tol = 1e-4 if name == "medium" else float(Z[name + "/tol"])
    a, b = Resident(X), Resident(X, np.ones(len(X), wdtype))
    try:
        ca, la, ia, na = a.fit(C0, max_iter, tol)
        cb, lb, ib, nb = b.fit(C0, max_iter, tol)
    finally:
        a.free()
        b.free()
    assert na == nb and np.array_equal(la, lb)
    assert np.abs(ca - cb).max() <= 1e-12 and abs(ia - ib) <= 1e-12 * ia


def test_null_weights_are_the_unweighted_fit_tile_sweeps_included(monkeypatch):
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.cluster import prune_stats
    from tests.lloyd_tile_cases import coherent_k
    monkeypatch.setenv("OFC_LLOYD_PRUNE", "2")
    X, C0 = coherent_k(3, 64 * 700 + 5, seed=4)
    C0 = np.ascontiguousarray(C0, np.float64)
    r = Resident(X)
    lib = _lib.load()
    out = []
    try:
        for weighted_entry in (False, True):
            cen, inertia, n_iter = np.empty((3, 2)), C.c_double(), C.c_int()
            args = (_lib.ptr(C0), 300, 1e-4, None, _lib.ptr(cen), C.c_void_p(r.lb.ptr), C.byref(inertia), C.byref(n_iter))
            if weighted_entry:
                _lib.check(lib.ofc_kmeans_fit_dev_w(0, C.c_void_p(r.xb.ptr), r.dtype, None, _lib.F32, r.N, 2, 3, *args))
            else:
                _lib.check(lib.ofc_kmeans_fit_dev_stats(0, C.c_void_p(r.xb.ptr), r.dtype, r.N, 2, 3, *args))
            out.append((cen, inertia.value, n_iter.value, r.labels(), prune_stats()))
    finally:
        r.free()
    (c0, i0, n0, l0, s0), (c1, i1, n1, l1, s1) = out
    assert np.array_equal(c0, c1) and i0 == i1 and n0 == n1 and np.array_equal(l0, l1) and s0 == s1
    assert s1["tile_sweeps"] > 0


# ------------------------------------------------------------------------------------------------ the large case
def test_large_case_matches_the_model_and_runs_no_tile_sweeps(large):
    from opticalflowclustering_amd.cluster import prune_stats
    X, w, C0, (cen, lab, inertia, n_iter), r = large
    assert r.N >= 1 << 20                      # an unweighted fit of this stream would go tile by tile
    c, l, i, n = r.fit(C0, 300, 0.0)
    assert prune_stats()["tile_sweeps"] == 0 and not prune_stats()["final_pruned"]
    assert n == n_iter and np.array_equal(l.astype(np.int32), lab)
    assert np.abs(c - cen).max() <= 1e-9 and abs(i - inertia) <= 1e-10 * inertia


# ------------------------------------------------------------------------------------------------ building blocks
def step_w(r, mean, cc):
    from opticalflowclustering_amd import _lib
    k = len(cc)
    rec = np.zeros(k * r.d + k + 1)
    _lib.check(_lib.load().ofc_lloyd_step_dev_w(0, C.c_void_p(r.xb.ptr), r.dtype, C.c_void_p(r.wb.ptr), r.wdtype, r.N, r.d, k,
                                                _lib.ptr(mean), _lib.ptr(cc), C.c_void_p(r.lb.ptr), _lib.ptr(rec)))
    return rec


def check_blocks(X, w, C0, r):
    from opticalflowclustering_amd import _lib
    lib = _lib.load()
    Xd, wd = X.astype(np.float64), w.astype(np.float64)
    N, d = Xd.shape
    k = len(C0)
    mean = Xd.mean(axis=0)
    cc = np.ascontiguousarray(C0 - mean)
    Xc = Xd - mean
    lab = M.e_step(Xc, cc)
    assert M.left_out(Xc, cc) == 0
    _lib.check(lib.ofc_memset(0, C.c_void_p(r.lb.ptr), 0xFF, N))
    rec = step_w(r, mean, cc)
    assert np.array_equal(r.labels(), lab.astype(np.uint8)) and rec[k * d + k] == N
    integer = np.array_equal(wd, np.rint(wd))
    for j in range(k):
        mem = lab == j
        want_w = math.fsum(wd[mem])
        assert rec[k * d + j] == want_w if integer else abs(rec[k * d + j] - want_w) <= sum_bound(wd[mem]), j
        for f in range(d):
            terms = Xc[mem, f] * wd[mem]                     # each product rounded on its own, as the kernel forms it
            assert abs(rec[j * d + f] - math.fsum(terms)) <= sum_bound(terms), (j, f)
    assert step_w(r, mean, cc)[k * d + k] == 0               # the same labels again: none changed
    # inertia
    terms = M.sq_dist_grouped(Xc, cc[lab]) * wd
    got = C.c_double()
    _lib.check(lib.ofc_lloyd_inertia_dev_w(0, C.c_void_p(r.xb.ptr), r.dtype, C.c_void_p(r.wb.ptr), r.wdtype, N, d, k, _lib.ptr(mean),
                                           _lib.ptr(cc), C.c_void_p(r.lb.ptr), C.byref(got)))
    assert abs(got.value - math.fsum(terms)) <= sum_bound(terms)
    # farthest: the distance ignores the weights, the winner's weight comes back
    dist = ((Xc - cc[lab]) ** 2).sum(axis=1)
    excl = np.array([int(np.argmax(dist))], np.int64)
    for ex in (None, excl):
        dd = dist.copy()
        if ex is not None:
            dd[ex] = -1
        i = int(np.argmax(dd))
        d2, idx, labo, wt = C.c_double(), C.c_int64(), C.c_int(), C.c_double()
        xc = np.zeros(d)
        _lib.check(lib.ofc_lloyd_farthest_dev_w(0, C.c_void_p(r.xb.ptr), r.dtype, C.c_void_p(r.wb.ptr), r.wdtype, N, d, k,
                                                _lib.ptr(mean), _lib.ptr(cc), C.c_void_p(r.lb.ptr), _lib.ptr(ex),
                                                0 if ex is None else 1, C.byref(d2), C.byref(idx), _lib.ptr(xc), C.byref(labo),
                                                C.byref(wt)))
        assert idx.value == i and labo.value == lab[i] and wt.value == wd[i] and np.array_equal(xc, Xc[i])
        assert abs(d2.value - dist[i]) <= 1e-12 * dist[i]


@pytest.mark.parametrize("name", ["cov_float32_d2_k8_wfloat32", "int_uint8_d2_k9_wfloat64", "cov_float64_d4_k16_wfloat64",
                                  "cov_uint8_d1_k2_wfloat32", "wide_1e-6_1e6_f64_d3_k4", "reloc_sample_weight0_f64"])
def test_building_blocks_one_call_at_a_time(name):
    X, w, C0, _, _ = case(name)
    r = Resident(X, w)
    try:
        check_blocks(X, w, C0, r)
    finally:
        r.free()


def test_building_blocks_on_the_large_case(large):
    X, w, C0, _, r = large
    check_blocks(X, w, C0, r)


# ------------------------------------------------------------------------------------------------ more than one rank
@pytest.mark.parametrize("name", ["reloc_it0_w2p5_f64", "cov_float32_d2_k8_wfloat32", "reloc_zero_weight_cluster_f32"])
def test_loopback_world_equals_fit_over_two_copies(name):
    from opticalflowclustering_amd._lib import check, load
    X, w, C0, max_iter, tol = case(name)
    both = Resident(np.concatenate([X, X]), np.concatenate([w, w]))
    one = Resident(X, w)
    try:
        cen, lab, inertia, n_iter = both.fit(C0, max_iter, tol)
        check(load().ofc_dist_loopback(2))
        try:
            c, l, i, n = one.fit(C0, max_iter, tol)
        finally:
            check(load().ofc_dist_loopback(1))
    finally:
        both.free()
        one.free()
    assert n == n_iter and np.array_equal(l, lab[:len(X)])
    assert np.abs(c - cen).max() <= 1e-9 and abs(i - inertia) <= 1e-10 * inertia


def _two_rank_weighted_worker(rank, conn, name, cut, q):
    """one of two processes sharing the GPU: the in-library driver over a host transport, this rank's rows and weights"""
    import numpy as np
    from opticalflowclustering_amd import _lib, dist
    from opticalflowclustering_amd.cluster import _DT, kmeans_fit_dev
    Zw = np.load(os.path.join(os.path.dirname(__file__), "golden", "lloyd_weighted_goldens.npz"))
    X, w, C0 = Zw[name + "/X"], Zw[name + "/w"], Zw[name + "/C0"]
    Xs = np.ascontiguousarray(X[:cut] if rank == 0 else X[cut:])
    ws = np.ascontiguousarray(w[:cut] if rank == 0 else w[cut:])
    fn = {"sum": np.add, "max": np.maximum, "min": np.minimum}

    def allreduce(arr, op):
        conn.send(arr)
        other = conn.recv()
        return fn[op](arr, other) if rank == 0 else fn[op](other, arr)     # same operand order on both ranks

    dist.init_host(0, rank, 2, allreduce)
    xb = _lib.DeviceBuffer(Xs.nbytes).upload(Xs)
    wb = _lib.DeviceBuffer(ws.nbytes).upload(ws)
    lab = _lib.DeviceBuffer(len(Xs))
    cen, inertia, n_iter = kmeans_fit_dev(xb.ptr, _DT[Xs.dtype], len(Xs), Xs.shape[1], C0, int(Zw[name + "/max_iter"]),
                                          float(Zw[name + "/tol"]), labels_ptr=lab.ptr, weights_ptr=wb.ptr,
                                          weight_dtype=_DT[ws.dtype])
    labels = lab.download((len(Xs),), np.uint8)
    dist.finalize()
    q.put((rank, cen, inertia, n_iter, labels.astype(np.int32)))


def test_two_processes_in_library_driver_weighted_relocation_on_rank_1():
    """two processes, shards of 5 and 115 rows; the farthest sample of iteration 0 (row 7, weight 2.5) lives on rank 1, which
    broadcasts it with its weight.  Must equal sklearn's fit of the whole data."""
    import multiprocessing as mp
    name, cut = "reloc_it0_w2p5_f64", 5
    assert Z[name + "/w"][7] == 2.5
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    c0, c1 = ctx.Pipe()
    procs = [ctx.Process(target=_two_rank_weighted_worker, args=(r, c, name, cut, q)) for r, c in ((0, c0), (1, c1))]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    labels = np.concatenate([res[0][4], res[1][4]])
    for _, cen, inertia, n_iter, _ in res:
        assert_golden(name, cen, labels, inertia, n_iter)
    assert np.array_equal(res[0][1], res[1][1])


@pytest.mark.parametrize("name", ["reloc_it0_w2p5_f64", "reloc_two_empty_u8", "reloc_sample_weight0_f64",
                                  "reloc_zero_weight_cluster_f32_maxit3", "cov_float64_d4_k16_wfloat32", "stop_tol0.01"])
def test_host_driven_sharded_fit_equals_the_library_fit(name):
    from opticalflowclustering_amd.sharded import DeviceShard, fit_sharded
    X, w, C0, max_iter, tol = case(name)
    r = Resident(X, w)
    try:
        cen, lab, inertia, n_iter = r.fit(C0, max_iter, tol)
        shard = DeviceShard(r.xb.ptr, r.dtype, r.N, r.d, weights_ptr=r.wb.ptr, weight_dtype=r.wdtype)
        c, i, n = fit_sharded(shard, C0, max_iter, tol)
        from opticalflowclustering_amd import _lib
        l = np.empty(r.N, np.uint8)
        _lib.check(_lib.load().ofc_memcpy_d2h(0, _lib.ptr(l), shard.labels, r.N))
    finally:
        r.free()
    assert n == n_iter and np.array_equal(l, lab)
    assert np.abs(c - cen).max() <= 1e-9 and abs(i - inertia) <= 1e-10 * max(inertia, 1e-300)
    assert_golden(name, c, l, i, n)


# ------------------------------------------------------------------------------------------------ weights from the flow
def test_flow_weights_dev(capsys):
    from opticalflowclustering_amd import _lib, stages
    rng = np.random.default_rng(11)
    n = 4 * 300_000 + 3
    F = (rng.standard_normal((n, 2)) * 10.0 ** rng.uniform(-3, 2, (n, 1))).astype(np.float32)
    F[:64] = 0
    F[64:128] = np.float32(0.5) * np.array([[0.6, 0.8]], np.float32)       # lengths next to the threshold 0.5
    fb = _lib.DeviceBuffer(F.nbytes).upload(F)
    wb = _lib.DeviceBuffer(n * 4)
    try:
        u, v = F[:, 0], F[:, 1]
        s = u * u + v * v                                                  # f32, every operation rounded
        thr = np.float32(0.5)
        stages.flow_weights_dev(fb.ptr, n, "moving", float(thr), wb.ptr)
        assert np.array_equal(wb.download((n,), np.float32), (s >= thr * thr).astype(np.float32))
        stages.flow_weights_dev(fb.ptr, n, "magnitude", 0.0, wb.ptr)
        got, want = wb.download((n,), np.float32), np.sqrt(s)
        differ = int(np.count_nonzero(got != want))
        with capsys.disabled():
            print(f"\n[flow weights] magnitude: {differ} of {n} values differ from numpy's f32 sqrt")
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(want).astype(np.float64))
        with pytest.raises(ValueError):
            stages.flow_weights_dev(fb.ptr, n, "speed", 0.0, wb.ptr)
        assert _lib.load().ofc_flow_weights_dev(0, C.c_void_p(fb.ptr), n, 1, C.c_float(-1.0), C.c_void_p(wb.ptr)) == _lib.OFC_EINVAL
    finally:
        fb.free()
        wb.free()


def test_clip_pipeline_weight_kinds_equal_fits_with_numpy_weights():
    from opticalflowclustering_amd.pipeline import ClipPipeline
    pipe = ClipPipeline(64, 48, 3)
    pipe.synth(t0=0, seed=2)
    pipe.run_flow()
    X = pipe.flows_host().reshape(-1, 2)
    s = X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]
    thr = np.float32(np.sqrt(np.median(s)))
    rng = np.random.default_rng(5)
    init = X[rng.choice(len(X), 3, replace=False)].astype(np.float64) + 0.01
    kinds = {"magnitude": np.sqrt(s), "moving": (s >= thr * thr).astype(np.float32),
             "array": rng.uniform(0.1, 2.0, len(X)).astype(np.float32)}
    try:
        for kind, w in kinds.items():
            arg = {"magnitude": "magnitude", "moving": ("moving", float(thr)), "array": w}[kind]
            cen, inertia, n_iter = pipe.run_kmeans(init, sample_weight=arg)
            lab = pipe.labels_host().ravel()
            got_w = pipe.weights.download((len(X),), np.float32)
            assert np.all(np.abs(got_w.astype(np.float64) - w) <= np.spacing(w).astype(np.float64)), kind
            if kind != "magnitude":
                assert np.array_equal(got_w, w), kind
            r = Resident(X, w)                       # the weights numpy built from flows_host()
            try:
                c, l, i, n = r.fit(init)
            finally:
                r.free()
            assert n == n_iter and np.array_equal(l, lab), kind
            assert np.abs(c - cen).max() <= 1e-9 and abs(i - inertia) <= 1e-10 * inertia, kind
        with pytest.raises(ValueError):
            pipe.run_kmeans(init, sample_weight="speed")
        with pytest.raises(ValueError):
            pipe.run_kmeans("k-means++", k=3, sample_weight="magnitude")
    finally:
        pipe.close()


# ------------------------------------------------------------------------------------------------ score
@pytest.mark.parametrize("name", ["cov_float32_d2_k8_wfloat32", "cov_uint8_d4_k16_wfloat64", "int_float64_d2_k9_wfloat32",
                                  "wide_1e-6_1e6_f64_d3_k4"])
def test_score_is_minus_the_weighted_inertia(name):
    from opticalflowclustering_amd.cluster import KMeans
    X, w, C0, max_iter, tol = case(name)
    km = KMeans(n_clusters=len(C0), init=C0, max_iter=max_iter, tol=tol).fit(X, sample_weight=w)
    for weights in (w, None):
        want = M.model_score(X, weights, km.cluster_centers_)
        got = km.score(X, sample_weight=weights)
        assert got <= 0 and abs(got - want) <= 1e-10 * abs(want), (name, got, want)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.cluster import KMeans, kmeans_fit_dev
    X, w, C0, _, _ = case("cov_float32_d2_k2_wfloat32")
    r = Resident(X, w)
    zeros = Resident(X, np.zeros(len(X), np.float32))
    lib = _lib.load()
    try:
        with pytest.raises(ValueError, match="weight dtype"):                    # u8 weights
            kmeans_fit_dev(r.xb.ptr, r.dtype, r.N, 2, C0, weights_ptr=r.wb.ptr, weight_dtype=_lib.U8)
        cen, inertia, n_iter = np.empty((2, 2)), C.c_double(), C.c_int()
        assert lib.ofc_kmeans_fit_w(0, _lib.ptr(X), _lib.F32, _lib.ptr(w), _lib.U8, len(X), 2, 2, _lib.ptr(C0), 300, 1e-4,
                                    _lib.ptr(cen), None, C.byref(inertia), C.byref(n_iter)) == _lib.OFC_EINVAL
        rec = np.zeros(7)
        assert lib.ofc_lloyd_step_dev_w(0, C.c_void_p(r.xb.ptr), r.dtype, C.c_void_p(r.wb.ptr), 3, r.N, 2, 2, _lib.ptr(np.zeros(2)),
                                        _lib.ptr(C0), C.c_void_p(r.lb.ptr), _lib.ptr(rec)) == _lib.OFC_EINVAL
        km = KMeans(n_clusters=2, init=C0)
        with pytest.raises(ValueError, match="sample_weight.shape"):             # wrong length
            km.fit(X, sample_weight=w[:-1])
        for bad in (-1.0, np.nan):                                               # through the C host API as well
            wb = w.copy()
            wb[3] = bad
            with pytest.raises(ValueError):
                km.fit(X, sample_weight=wb)
            assert lib.ofc_kmeans_fit_w(0, _lib.ptr(X), _lib.F32, _lib.ptr(wb), _lib.F32, len(X), 2, 2, _lib.ptr(C0), 300, 1e-4,
                                        _lib.ptr(cen), None, C.byref(inertia), C.byref(n_iter)) == _lib.OFC_EINVAL
            assert lib.ofc_kmeans_score(0, _lib.ptr(X), _lib.F32, _lib.ptr(wb), _lib.F32, len(X), 2, 2, _lib.ptr(C0),
                                        C.byref(inertia)) == _lib.OFC_EINVAL
        with pytest.raises(ValueError, match="must be positive"):                # all zero: host path
            km.fit(X, sample_weight=np.zeros(len(X)))
        assert lib.ofc_kmeans_fit_w(0, _lib.ptr(X), _lib.F32, _lib.ptr(np.zeros(len(X), np.float32)), _lib.F32, len(X), 2, 2,
                                    _lib.ptr(C0), 300, 1e-4, _lib.ptr(cen), None, C.byref(inertia), C.byref(n_iter)) == _lib.OFC_EINVAL
        with pytest.raises(ValueError, match="sum of sample weights must be positive"):      # all zero: device path
            zeros.fit(C0)
        with pytest.raises(ValueError, match="k-means\\+\\+"):
            KMeans(n_clusters=2, init="k-means++").fit(X, sample_weight=w)
        assert_golden("cov_float32_d2_k2_wfloat32", *r.fit(C0))                  # the scratch is fit for use after a refusal
    finally:
        r.free()
        zeros.free()
