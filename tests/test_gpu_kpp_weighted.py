"""k-means++ seeding with sample weights on device-resident samples (ofc_kpp_seed_dev_w, ofc_kpp_sample_dev_w,
cluster.kmeans_plusplus_dev(weights_ptr=), ClipPipeline.seed_kmeans) against sklearn 1.7.2's goldens
(tests/golden/make_kpp_weighted_goldens.py), numpy's cumsum/searchsorted and the host route through the CPU oracle
(tests/kpp_weighted_cases.py, which tests/test_kpp_weighted_host.py proves well-conditioned case by case).

Bars of the two-step fit, as in test_gpu_lloyd_weighted.py: labels bit-equal, n_iter equal, centres <= 1e-9, inertia <= 1e-10
relative."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import kpp_weighted_cases as WC

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "kpp_weighted_goldens.npz"))
GOLDEN = sorted({k.split("/")[0] for k in Z.files if not k.startswith("X/")})


def golden(name):
    return Z["X/" + str(Z[name + "/family"])], Z[name + "/w"], int(Z[name + "/k"]), int(Z[name + "/seed"])


class Resident:
    """X and w (f32 or f64) on the device"""

    def __init__(self, X, w):
        from opticalflowclustering_amd import _lib
        from opticalflowclustering_amd.cluster import _DT
        self.X, self.w = np.ascontiguousarray(X), np.ascontiguousarray(w)
        self.N, self.d = self.X.shape
        self.dtype, self.wdtype = _DT[self.X.dtype], _DT[self.w.dtype]
        self.xb = _lib.DeviceBuffer(max(self.X.nbytes, 16))
        self.wb = _lib.DeviceBuffer(max(self.w.nbytes, 16))
        if self.N:
            self.xb.upload(self.X)
            self.wb.upload(self.w)

    def seed(self, k, random_state, **kw):
        from opticalflowclustering_amd.cluster import kmeans_plusplus_dev
        return kmeans_plusplus_dev(self.xb.ptr, self.dtype, self.N, self.d, k, random_state, weights_ptr=self.wb.ptr,
                                   weight_dtype=self.wdtype, **kw)

    def seed_raw(self, k, u_first, u=None, n_trials=1):
        """ofc_kpp_seed_dev_w on given numbers -> rc, centers, indices"""
        from opticalflowclustering_amd import _lib
        cen, idx = np.full((k, self.d), -1.0), np.full(k, -1, np.int64)
        rc = _lib.load().ofc_kpp_seed_dev_w(0, C.c_void_p(self.xb.ptr), self.dtype, C.c_void_p(self.wb.ptr), self.wdtype,
                                            self.N, self.d, k, None, u_first, _lib.ptr(u) if u is not None else None,
                                            n_trials, _lib.ptr(cen), _lib.ptr(idx))
        return rc, cen, idx

    def free(self):
        self.xb.free()
        self.wb.free()


@pytest.mark.parametrize("name", GOLDEN)
def test_resident_seeding_picks_sklearns_rows_and_the_two_step_fit_is_sklearns(name):
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.cluster import kmeans_fit_dev
    X, w, k, seed = golden(name)
    r = Resident(X, w)
    lb = _lib.DeviceBuffer(len(X))
    try:
        C0, idx = r.seed(k, seed)
        assert np.array_equal(idx, Z[name + "/indices"])
        assert np.array_equal(C0, X[idx].astype(np.float64))
        cen, inertia, n_iter = kmeans_fit_dev(r.xb.ptr, r.dtype, r.N, r.d, C0, labels_ptr=lb.ptr, weights_ptr=r.wb.ptr,
                                              weight_dtype=r.wdtype)
        ref = float(Z[name + "/inertia"])
        assert n_iter == int(Z[name + "/n_iter"])
        assert np.array_equal(lb.download((len(X),), np.uint8), Z[name + "/labels"])
        assert np.abs(cen - Z[name + "/centers"]).max() <= 1e-9
        assert abs(inertia - ref) <= 1e-10 * ref, (inertia, ref)
    finally:
        r.free()
        lb.free()


@pytest.mark.parametrize("case", WC.CASES, ids=WC.case_id)
def test_end_to_end_equals_the_host_route_index_for_index(case):
    """every dtype, d, k and weight kind at the seams of the chunked cumulative sum, the weights stored as f32 and as f64
    (the same values): the rows of the host route through the CPU oracle"""
    from opticalflowclustering_amd.cluster import kpp_draws_w
    k = case[3]
    X, w = WC.make_X(case), WC.make_w(case)
    seed = WC.case_seed(case)
    u_first, u, _ = kpp_draws_w(np.random.RandomState(seed), k)
    want, _, _, _ = WC.host_seed(X, w, k, u_first, u)
    for wt in (np.float32, np.float64):
        assert np.array_equal(w.astype(wt).astype(np.float64), w.astype(np.float64))
        r = Resident(X, w.astype(wt))
        try:
            centers, idx = r.seed(k, seed)
        finally:
            r.free()
        assert np.array_equal(idx, want), wt
        assert np.array_equal(centers, X[want].astype(np.float64))


# ------------------------------------------------------------------------------------------------ the sampling hook
def _sample(w, v, r, side):
    """ofc_kpp_sample_dev_w -> indices, the total the device formed"""
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.cluster import _DT
    w = np.ascontiguousarray(w)
    r = np.ascontiguousarray(r, np.float64)
    wb = _lib.DeviceBuffer(max(w.nbytes, 16)).upload(w)
    vb = _lib.DeviceBuffer(max(8 * len(w), 16)).upload(np.ascontiguousarray(v, np.float64)) if v is not None else None
    try:
        out, total = [], None
        for j in range(0, len(r), 8):
            part = np.ascontiguousarray(r[j:j + 8])
            idx, tot = np.full(len(part), -7, np.int64), np.full(1, -7.0)
            _lib.check(_lib.load().ofc_kpp_sample_dev_w(0, C.c_void_p(wb.ptr), _DT[w.dtype], C.c_void_p(vb.ptr) if vb else None,
                                                        len(w), _lib.ptr(part), len(part), {"left": 0, "right": 1}[side],
                                                        _lib.ptr(idx), _lib.ptr(tot)))
            assert total is None or total == tot[0]
            total = tot[0]
            out.append(idx)
        return np.concatenate(out), total
    finally:
        wb.free()
        if vb:
            vb.free()


def _sample_sizes():
    CH = WC.CH
    return [1, 2, 5, CH - 1, CH, CH + 1, 3 * CH + 7, CH * CH - 1, CH * CH + CH + 3]     # the last: two top-level sums


def _exact_inputs(N, kind, variant, rng):
    """(w, v or None): every product and partial sum is a small multiple of 1/8, exact in any order"""
    w = rng.integers(0, 8, N).astype(np.float64) * (0.25 if variant != "f32" else 1.0)
    if kind == "runs":                      # zero-weight runs: leading, trailing and inside, across chunk borders
        w[: N // 3] = 0
        w[N - max(N // 4, 1):] = 0
        w[N // 2: N // 2 + N // 8] = 0
    if kind == "zeros":
        w[:] = 0
    v = None
    if variant != "f32":
        v = rng.integers(0, 5, N) * 0.5           # zeros among them as well
    return w.astype(np.float32 if variant != "f64v" else np.float64), v


@pytest.mark.parametrize("variant", ["f32", "f32v", "f64v"])
@pytest.mark.parametrize("kind", ["dense", "runs", "zeros"])
@pytest.mark.parametrize("N", _sample_sizes())
def test_sampling_hook_is_searchsorted_of_cumsum_exactly(N, kind, variant):
    """exact inputs, so no tolerance, on either side.  r at 0, at partial sums (where 'left' and 'right' differ), between
    them, at the total and above it"""
    from opticalflowclustering_amd import _lib
    assert _lib.KPP_CHUNK == WC.CH
    CH = WC.CH
    rng = np.random.default_rng(N)
    w, v = _exact_inputs(N, kind, variant, rng)
    cum = np.cumsum(w.astype(np.float64) * (v if v is not None else 1.0))
    at = np.unique(np.concatenate([[0, N // 3, N // 2, N - 1], rng.integers(0, N, 9),
                                   np.clip([CH - 1, CH, CH * CH - 1, CH * CH], 0, N - 1)]))
    r = np.concatenate([[0.0], cum[at], cum[at] + 0.0625, [cum[-1], cum[-1] + 1, cum[-1] * 2 + 10]])
    for side in ("left", "right"):
        got, total = _sample(w, v, r, side)
        assert np.array_equal(got, np.minimum(np.searchsorted(cum, r, side), N - 1)), side
        assert total == cum[-1]


def test_sampling_hook_rounding_stays_inside_the_a_priori_bound():
    """general values: any summation order of N non-negative terms moves a partial sum by < N 2^-53 T"""
    N = (1 << 20) + 1
    rng = np.random.default_rng(4)
    w = (rng.random(N) * np.exp(rng.normal(size=N) * 2)).astype(np.float32)
    w[rng.random(N) < 0.3] = 0
    v = rng.random(N) * np.exp(rng.normal(size=N) * 2)
    t = w.astype(np.float64) * v
    T = math.fsum(t)
    eps = N * 2.0 ** -53 * T
    r = np.concatenate([rng.random(13) * T, [0.0, T * 0.999999, 1e-300]])
    got, total = _sample(w, v, r, "left")
    assert abs(total - T) <= eps
    for i, rj in zip(got, r):
        assert 0 <= i < N
        assert i == 0 or math.fsum(t[:i]) < rj + eps
        assert math.fsum(t[:i + 1]) >= rj - eps
    got, _ = _sample(w, v, r, "right")
    for i, rj in zip(got, r):
        assert 0 <= i < N
        assert i == 0 or math.fsum(t[:i]) <= rj + eps
        assert math.fsum(t[:i + 1]) > rj - eps


# ------------------------------------------------------------------------------------------------ the first centre
@pytest.mark.parametrize("wt", [np.float32, np.float64])
@pytest.mark.parametrize("N", [1, 7, WC.CH, WC.CH + 1, 3 * WC.CH + 7, 2 * WC.CH * WC.CH + 5])
def test_first_centre_is_never_a_zero_weight_row(N, wt):
    """integer weights with leading, inner and trailing zero runs: the cumulative sum, W and u_first * W are exact, so the
    row is searchsorted(cumsum(w), u_first * W, 'right'), and the last row of positive weight where that runs off the
    end.  u_first at 0, just below 1, at cumulative values and one ulp below them"""
    rng = np.random.default_rng(N)
    w = rng.integers(0, 4, N).astype(wt)
    w[: N // 5] = 0
    w[N // 2: N // 2 + N // 7] = 0
    w[N - N // 3:] = 0
    w[N // 3] = 3
    cum = np.cumsum(w.astype(np.float64))
    W = cum[-1]
    last_pos = int(np.nonzero(w)[0][-1])
    X = np.arange(N, dtype=np.float32).reshape(N, 1)
    r = Resident(X, w)
    try:
        at = cum[rng.integers(0, N, 6)] / W
        for u_first in np.concatenate([[0.0, 1.0 - 2.0 ** -53, 0.5, 1.0 / 3], at[at < 1.0], np.nextafter(at, 0)[at > 0]]):
            rc, cen, idx = r.seed_raw(1, float(u_first))
            assert rc == 0
            want = int(np.searchsorted(cum, u_first * W, "right"))
            want = want if want < N else last_pos
            assert idx[0] == want and w[idx[0]] > 0 and cen[0, 0] == want, u_first
    finally:
        r.free()


def test_first_centre_on_general_weights_has_weight_and_brackets_the_draw():
    """random weights, 60 % of them zero, the last tenth all zero: whatever rounding does, the row has positive weight, and
    the exact cumulative sum brackets u_first * T within N 2^-53 T on either side"""
    N = 5 * WC.CH * WC.CH // 4 + 11
    rng = np.random.default_rng(8)
    w = (rng.random(N) * np.exp(rng.normal(size=N) * 2)).astype(np.float32)
    w[rng.random(N) < 0.6] = 0
    w[N - N // 10:] = 0
    wd = w.astype(np.float64)
    T = math.fsum(wd)
    eps = N * 2.0 ** -53 * T
    r = Resident(np.zeros((N, 1), np.uint8), w)
    try:
        for u_first in (0.0, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -30, 0.25, 0.5, 0.9999999, 1e-12):
            rc, _, idx = r.seed_raw(1, u_first)
            i = int(idx[0])
            assert rc == 0 and 0 <= i < N and w[i] > 0, u_first
            assert math.fsum(wd[:i]) <= u_first * T + 2 * eps and math.fsum(wd[:i + 1]) > u_first * T - 2 * eps, u_first
    finally:
        r.free()


@pytest.mark.parametrize("wt", [np.float32, np.float64])
def test_unit_weights_are_the_unweighted_seeding(wt):
    """w = 1: every weighted value, chunk sum and potential is the unweighted one bit for bit, so from the same first
    centre the rows are ofc_kpp_seed_dev's"""
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.cluster import kpp_draws_w
    KPP = np.load(os.path.join(os.path.dirname(__file__), "golden", "kpp_goldens.npz"))
    for name in ("cell_k8_s3", "blob_k5_s11", "img_k3_s2"):
        X, k = KPP[name + "/X"], int(KPP[name + "/k"])
        u_first, u, nt = kpp_draws_w(np.random.RandomState(3), k)
        r = Resident(X, np.ones(len(X), wt))
        try:
            rc, cen_w, idx_w = r.seed_raw(k, u_first, u, nt)
            assert rc == 0 and idx_w[0] == min(int(u_first * len(X)), len(X) - 1)
            cen, idx = np.empty((k, X.shape[1])), np.empty(k, np.int64)
            _lib.check(_lib.load().ofc_kpp_seed_dev(0, C.c_void_p(r.xb.ptr), r.dtype, r.N, r.d, k, None, int(idx_w[0]),
                                                    _lib.ptr(u), nt, _lib.ptr(cen), _lib.ptr(idx)))
            assert np.array_equal(idx, idx_w) and np.array_equal(cen, cen_w)
        finally:
            r.free()


# ------------------------------------------------------------------------------------------------ two ranks
def _two_rank_data(name, split, zero_head):
    X, w, k, seed = golden(name)
    cut = int(len(X) * split)
    if zero_head:
        w = w.copy()
        w[:cut] = 0
    return X, w, k, seed, cut


def _two_rank_seed_worker(rank, conn, name, split, zero_head, q):
    import numpy as np
    from opticalflowclustering_amd import dist
    X, w, k, seed, cut = _two_rank_data(name, split, zero_head)
    sl = slice(0, cut) if rank == 0 else slice(cut, None)
    fn = {"sum": np.add, "max": np.maximum, "min": np.minimum}

    def allreduce(arr, op):
        conn.send(arr)
        other = conn.recv()
        return fn[op](arr, other) if rank == 0 else fn[op](other, arr)     # same operand order on both ranks

    dist.init_host(0, rank, 2, allreduce)
    r = Resident(X[sl], w[sl])
    cen, idx = r.seed(k, seed, n_global=len(X))
    dist.finalize()
    q.put((rank, cen, idx))


@pytest.mark.parametrize("name,split,zero_head", [("blob_mag_k5_s0", 0.5, False), ("cell_mov_k3_s1", 0.37, False),
                                                  ("img_int_k3_s0", 1.0, False), ("blob_int_k5_s0", 0.4, True)])
def test_two_real_ranks_seed_like_one(name, split, zero_head):
    """two processes, uneven shards (the second empty at split 1.0; all of rank 0's weights zero in the last case), the
    per-step exchange over a pipe: both ranks return the single-rank rows -- sklearn's, and where the weights were
    changed, the host route's"""
    import multiprocessing as mp
    from opticalflowclustering_amd.cluster import kmeans_plusplus
    X, w, k, seed, cut = _two_rank_data(name, split, zero_head)
    if zero_head:
        _, want = kmeans_plusplus(X, k, seed, sample_weight=w, _step=O.kpp_candidates)
        assert np.all(want >= cut)
    else:
        want = Z[name + "/indices"]
        if split < 1.0:
            assert np.any(want >= cut) and np.any(want < cut)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    c0, c1 = ctx.Pipe()
    procs = [ctx.Process(target=_two_rank_seed_worker, args=(r, c, name, split, zero_head, q)) for r, c in ((0, c0), (1, c1))]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for _, cen, idx in res:
        assert np.array_equal(idx, want)
        assert np.array_equal(cen, X[want].astype(np.float64))


# ------------------------------------------------------------------------------------------------ ClipPipeline
def test_clip_pipeline_seeds_with_weights_and_keeps_its_refusals():
    from opticalflowclustering_amd.cluster import KMeans, kmeans_plusplus
    from opticalflowclustering_amd.pipeline import ClipPipeline
    pipe = ClipPipeline(64, 48, 3, batch_pairs=2)
    try:
        pipe.synth(0, 1)
        pipe.run_flow()
        uv = pipe.flows_host().reshape(-1, 2)
        N = len(uv)
        length = np.sqrt(uv[:, 0] * uv[:, 0] + uv[:, 1] * uv[:, 1])
        thr = float(np.quantile(length, 0.7))
        for sw in ("magnitude", ("moving", thr)):
            C0, idx = pipe.seed_kmeans(4, random_state=5, sample_weight=sw)
            w = pipe.weights.download((N,), np.float32)
            _, want = kmeans_plusplus(uv, 4, 5, sample_weight=w, _step=O.kpp_candidates)
            assert np.array_equal(idx, want) and np.array_equal(C0, uv[want].astype(np.float64))
            if sw != "magnitude":
                assert np.all(w[idx] == 1) and np.all(length[idx] >= np.float32(thr)) and 0 < np.mean(w) < 0.5
            cen, inertia, n_iter = pipe.run_kmeans(C0, sample_weight=sw)      # the second step of the route
            assert cen.shape == (4, 2) and np.isfinite(inertia) and n_iter >= 1
        # no weights: the seeds run_kmeans('k-means++') starts from
        C0, idx = pipe.seed_kmeans(3, random_state=5)
        _, want = kmeans_plusplus(uv, 3, 5, _step=O.kpp_candidates)
        assert np.array_equal(idx, want)
        a, b = pipe.run_kmeans(C0), pipe.run_kmeans("k-means++", k=3, random_state=5)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        # the one-call forms stay refused, and say where to go
        with pytest.raises(ValueError, match="seed_kmeans"):
            pipe.run_kmeans("k-means++", k=3, sample_weight="magnitude")
        with pytest.raises(ValueError, match=r"k-means\+\+"):
            KMeans(3, init="k-means++").fit(uv, sample_weight=length)
    finally:
        pipe.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_with_a_code_and_a_message_before_any_launch():
    from opticalflowclustering_amd import _lib
    lib = _lib.load()
    X = np.arange(40, dtype=np.float32).reshape(20, 2)
    xb = _lib.DeviceBuffer(X.nbytes).upload(X)
    wb = _lib.DeviceBuffer(80).upload(np.ones(20, np.float32))
    zb = _lib.DeviceBuffer(80)
    zb.zero()
    u = np.full((3, 2), 0.5)
    cen, idx = np.full((4, 2), -1.0), np.full(4, -1, np.int64)
    xp, wp, p = C.c_void_p(xb.ptr), C.c_void_p(wb.ptr), _lib.ptr

    def seed(X_=xp, w_=wp, wdt=_lib.F32, N=20, d=2, k=4, u_first=0.3, u_=u, nt=2, cen_=cen, idx_=idx):
        return lib.ofc_kpp_seed_dev_w(0, X_, _lib.F32, w_, wdt, N, d, k, None, u_first, p(u_) if u_ is not None else None, nt,
                                      p(cen_) if cen_ is not None else None, p(idx_) if idx_ is not None else None)

    def refused(rc, code):
        assert rc == code and len(lib.ofc_last_error()) > 0
        assert np.all(cen == -1.0) and np.all(idx == -1)          # nothing was written

    try:
        for kw in (dict(w_=None), dict(wdt=_lib.U8), dict(wdt=7), dict(w_=C.c_void_p(wb.ptr + 4)), dict(u_first=1.0),
                   dict(u_first=-1e-9), dict(u_first=float("nan")), dict(X_=None), dict(u_=None), dict(cen_=None),
                   dict(idx_=None), dict(N=-1), dict(N=3), dict(nt=0), dict(nt=9), dict(u_=np.array([[0.5, 1.0]] * 3)),
                   dict(u_=np.array([[np.nan, 0.5]] * 3))):
            refused(seed(**kw), _lib.OFC_EINVAL)
        for kw in (dict(k=17), dict(d=5)):
            refused(seed(**kw), _lib.OFC_EUNSUPPORTED)
        refused(seed(w_=C.c_void_p(zb.ptr)), _lib.OFC_EINVAL)       # all weights zero: found on the device
        assert lib.ofc_last_error() == b"sum of sample weights must be positive"
        r, out, tot = np.array([1.0]), np.full(8, -1, np.int64), np.full(1, -1.0)
        for args in ((None, _lib.F32, None, 20, p(r), 1, 0, p(out), p(tot)), (wp, _lib.U8, None, 20, p(r), 1, 0, p(out), p(tot)),
                     (wp, _lib.F32, None, 20, None, 1, 0, p(out), p(tot)), (wp, _lib.F32, None, 20, p(r), 1, 0, None, p(tot)),
                     (wp, _lib.F32, None, 20, p(r), 1, 0, p(out), None), (wp, _lib.F32, None, 20, p(r), 0, 0, p(out), p(tot)),
                     (wp, _lib.F32, None, 20, p(r), 9, 0, p(out), p(tot)), (wp, _lib.F32, None, 0, p(r), 1, 0, p(out), p(tot)),
                     (wp, _lib.F32, None, 20, p(r), 1, 2, p(out), p(tot)), (wp, _lib.F32, None, 20, p(r), 1, -1, p(out), p(tot))):
            assert lib.ofc_kpp_sample_dev_w(0, *args) == _lib.OFC_EINVAL and len(lib.ofc_last_error()) > 0
            assert np.all(out == -1) and tot[0] == -1.0
        # the scratch is usable afterwards, and the call itself works
        assert seed() == _lib.OFC_OK and idx[0] == 6 and np.array_equal(cen, X[idx])
    finally:
        for b in (xb, wb, zb):
            b.free()
