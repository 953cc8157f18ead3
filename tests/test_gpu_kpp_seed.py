"""k-means++ seeding on device-resident samples (ofc_kpp_seed_dev, ofc_kpp_sample_dev, cluster.kmeans_plusplus_dev,
KMeans(init='k-means++'), ClipPipeline.run_kmeans('k-means++')) against sklearn's goldens, numpy's
cumsum/searchsorted and the host route through the CPU oracle."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import kpp_seed_cases as KC

pytestmark = pytest.mark.gpu

KPP = np.load(os.path.join(os.path.dirname(__file__), "golden", "kpp_goldens.npz"))
KPP_CASES = sorted({k.split("/")[0] for k in KPP.files})


def _seed_dev(X, k, seed, **kw):
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.cluster import _DT, kmeans_plusplus_dev
    buf = _lib.DeviceBuffer(max(X.nbytes, 8), 0)
    try:
        buf.upload(X)
        return kmeans_plusplus_dev(buf.ptr, _DT[X.dtype], len(X), X.shape[1], k, seed, **kw)
    finally:
        buf.free()


@pytest.mark.parametrize("name", KPP_CASES)
def test_resident_seeding_picks_sklearns_rows(name):
    X, k, seed = KPP[name + "/X"], int(KPP[name + "/k"]), int(KPP[name + "/seed"])
    centers, idx = _seed_dev(X, k, seed)
    assert np.array_equal(idx, KPP[name + "/indices"])
    assert np.array_equal(centers, X[idx].astype(np.float64))


def _sample(w, r):
    from opticalflowclustering_amd import _lib
    w = np.ascontiguousarray(w, np.float64)
    r = np.ascontiguousarray(r, np.float64)
    buf = _lib.DeviceBuffer(w.nbytes, 0)
    try:
        buf.upload(w)
        out = []
        for j in range(0, len(r), 8):
            part = np.ascontiguousarray(r[j:j + 8])
            idx = np.full(len(part), -7, np.int64)
            _lib.check(_lib.load().ofc_kpp_sample_dev(0, C.c_void_p(buf.ptr), len(w), _lib.ptr(part), len(part), _lib.ptr(idx)))
            out.append(idx)
        return np.concatenate(out)
    finally:
        buf.free()


def _sample_sizes():
    return [1, 2, KC.CH - 1, KC.CH, KC.CH + 1, 3 * KC.CH + 7, KC.CH * KC.CH + KC.CH + 3]   # the last: two second-level sums


def _weights(N, kind, rng):
    if kind == "zeros":
        return np.zeros(N)
    w = rng.integers(0, 1000, N).astype(np.float64)
    if kind == "runs":                      # long zero runs: leading, trailing and inside, across chunk borders
        w[: N // 3] = 0
        w[N - max(N // 4, 1):] = 0
        w[N // 2: N // 2 + N // 8] = 0
    return w


@pytest.mark.parametrize("kind", ["dense", "runs", "zeros"])
@pytest.mark.parametrize("N", _sample_sizes())
def test_sampling_stage_is_searchsorted_of_cumsum_exactly(N, kind):
    """integer-valued weights: every partial sum is exact in any order, so no tolerance.  r at 0, at prefix sums, half
    a unit above them, at the total and above it"""
    from opticalflowclustering_amd import _lib
    assert _lib.KPP_CHUNK == KC.CH
    rng = np.random.default_rng(N)
    w = _weights(N, kind, rng)
    cum = np.cumsum(w)
    at = np.unique(np.concatenate([[0, N // 3, N // 2, N - 1], rng.integers(0, N, 9),
                                   np.clip([KC.CH - 1, KC.CH, KC.CH * KC.CH - 1, KC.CH * KC.CH], 0, N - 1)]))
    r = np.concatenate([[0.0], cum[at], cum[at] + 0.5, [cum[-1], cum[-1] + 1, cum[-1] * 2 + 10]])
    want = np.minimum(np.searchsorted(cum, r), N - 1)
    assert np.array_equal(_sample(w, r), want)


def test_sampling_stage_rounding_stays_inside_the_a_priori_bound():
    """random positive weights: any summation order of N non-negative terms moves a partial sum by < N 2^-53 T"""
    N = (1 << 20) + 1
    rng = np.random.default_rng(3)
    w = rng.random(N) * np.exp(rng.normal(size=N) * 3)
    T = math.fsum(w)
    r = np.concatenate([rng.random(13) * T, [0.0, T * 0.999999, 1e-300]])
    got = _sample(w, r)
    eps = N * 2.0 ** -53 * T
    for i, rj in zip(got, r):
        assert 0 <= i < N
        assert i == 0 or math.fsum(w[:i]) < rj + eps
        assert math.fsum(w[:i + 1]) >= rj - eps


@pytest.mark.parametrize("case", KC.CASES, ids=KC.case_id)
def test_end_to_end_equals_the_host_route_index_for_index(case):
    """every dtype, d, k at the seams of the chunked cumulative sum (test_kpp_seed_host.py proves each case
    well-conditioned): same rows as the host route through the CPU oracle"""
    from opticalflowclustering_amd.cluster import kpp_draws
    _, _, _, k, N = case
    X = KC.make_X(case)
    seed = KC.case_seed(case)
    first, u, _ = kpp_draws(np.random.RandomState(seed), N, k)
    want, _, _ = KC.host_seed(X, k, first, u)
    centers, idx = _seed_dev(X, k, seed)
    assert np.array_equal(idx, want)
    assert np.array_equal(centers, X[want].astype(np.float64))


def _two_rank_seed_worker(rank, conn, name, split, q):
    import numpy as np
    from opticalflowclustering_amd import _lib, dist
    from opticalflowclustering_amd.cluster import _DT, kmeans_plusplus_dev
    X, k, seed = KPP[name + "/X"], int(KPP[name + "/k"]), int(KPP[name + "/seed"])
    cut = int(len(X) * split)
    Xs = np.ascontiguousarray(X[:cut] if rank == 0 else X[cut:])
    fn = {"sum": np.add, "max": np.maximum, "min": np.minimum}

    def allreduce(arr, op):
        conn.send(arr)
        other = conn.recv()
        return fn[op](arr, other) if rank == 0 else fn[op](other, arr)     # same operand order on both ranks

    dist.init_host(0, rank, 2, allreduce)
    buf = _lib.DeviceBuffer(max(Xs.nbytes, 8), 0)
    if len(Xs):
        buf.upload(Xs)
    cen, idx = kmeans_plusplus_dev(buf.ptr, _DT[Xs.dtype], len(Xs), Xs.shape[1], k, seed, n_global=len(X))
    dist.finalize()
    q.put((rank, cen, idx))


@pytest.mark.parametrize("name,split", [("blob_k5_s0", 0.5), ("cell_k8_s3", 0.37), ("img_k3_s2", 1.0), ("cell_k3_s7", 0.5)])
def test_two_real_ranks_seed_like_one(name, split):
    """two processes, uneven shards (one empty at split 1.0), the per-step exchange over a pipe: both ranks return the
    single-process rows, which are sklearn's.  Every case but the empty-shard one has winners on rank 1; in
    cell_k3_s7 the first centre is on rank 0 and both later winners on rank 1"""
    import multiprocessing as mp
    X, want = KPP[name + "/X"], KPP[name + "/indices"]
    cut = int(len(X) * split)
    if split < 1.0:
        assert np.any(want[1:] >= cut) and np.any(want < cut)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    c0, c1 = ctx.Pipe()
    procs = [ctx.Process(target=_two_rank_seed_worker, args=(r, c, name, split, q)) for r, c in ((0, c0), (1, c1))]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for _, cen, idx in res:
        assert np.array_equal(idx, want)
        assert np.array_equal(cen, X[want].astype(np.float64))


def test_kmeans_class_seeds_on_the_uploaded_samples():
    """KMeans(init='k-means++').fit = resident seeding + resident fit: the same model as the fit from the host seeding"""
    from opticalflowclustering_amd.cluster import KMeans, kmeans_plusplus
    name = "cell_k8_s3"
    X, k, seed = KPP[name + "/X"], int(KPP[name + "/k"]), int(KPP[name + "/seed"])
    C0, _ = kmeans_plusplus(X, k, seed, _step=O.kpp_candidates)
    ref = KMeans(n_clusters=k, init=C0).fit(X)
    km = KMeans(n_clusters=k, init="k-means++", random_state=seed).fit(X)
    assert km.n_iter_ == ref.n_iter_ and km.inertia_ == ref.inertia_
    assert np.array_equal(km.labels_, ref.labels_) and np.array_equal(km.cluster_centers_, ref.cluster_centers_)


def test_clip_pipeline_seeds_its_resident_vectors():
    from opticalflowclustering_amd.cluster import kmeans_plusplus
    from opticalflowclustering_amd.pipeline import ClipPipeline
    pipe = ClipPipeline(64, 48, 3, batch_pairs=2)
    try:
        pipe.synth(0, 1)
        pipe.run_flow()
        cen, inertia, n_iter = pipe.run_kmeans("k-means++", k=3, random_state=5)
        uv = pipe.flows_host().reshape(-1, 2)
        C0, _ = kmeans_plusplus(uv, 3, 5, _step=O.kpp_candidates)
        ref = pipe.run_kmeans(C0)              # kmeans_fit_dev on the resident vectors, with the same column sums
        assert n_iter == ref[2] and np.array_equal(cen, ref[0]) and inertia == ref[1]
        with pytest.raises(ValueError):
            pipe.run_kmeans("k-means++")
    finally:
        pipe.close()


def test_refusals_come_with_a_code_and_a_message_before_any_launch():
    from opticalflowclustering_amd import _lib
    lib = _lib.load()
    X = np.arange(40, dtype=np.float32).reshape(20, 2)
    buf = _lib.DeviceBuffer(X.nbytes, 0)
    buf.upload(X)
    u = np.full((3, 2), 0.5)
    cen, idx = np.full((4, 2), -1.0), np.full(4, -1, np.int64)
    xp, p = C.c_void_p(buf.ptr), _lib.ptr

    def seed(X_=xp, N=20, d=2, k=4, first=3, u_=u, nt=2, cen_=cen, idx_=idx):
        return lib.ofc_kpp_seed_dev(0, X_, _lib.F32, N, d, k, None, first, p(u_) if u_ is not None else None, nt,
                                    p(cen_) if cen_ is not None else None, p(idx_) if idx_ is not None else None)

    def refused(rc, code):
        assert rc == code and len(lib.ofc_last_error()) > 0
        assert np.all(cen == -1.0) and np.all(idx == -1)          # nothing ran

    try:
        for kw in (dict(X_=None), dict(u_=None), dict(cen_=None), dict(idx_=None), dict(N=-1), dict(N=3), dict(first=-1),
                   dict(first=20), dict(nt=0), dict(nt=9), dict(u_=np.array([[0.5, 1.0]] * 3)),
                   dict(u_=np.array([[-1e-9, 0.5]] * 3)), dict(u_=np.array([[np.nan, 0.5]] * 3))):
            refused(seed(**kw), _lib.OFC_EINVAL)
        for kw in (dict(k=17), dict(d=5)):
            refused(seed(**kw), _lib.OFC_EUNSUPPORTED)
            assert b"outside the kernels' range" in lib.ofc_last_error()
        w = _lib.DeviceBuffer(64, 0)
        w.upload(np.ones(8))
        r, out = np.array([1.0]), np.full(8, -1, np.int64)
        wp = C.c_void_p(w.ptr)
        for args in ((None, 8, p(r), 1, p(out)), (wp, 8, None, 1, p(out)), (wp, 8, p(r), 1, None), (wp, 8, p(r), 0, p(out)),
                     (wp, 8, p(r), 9, p(out)), (wp, 0, p(r), 1, p(out)), (wp, -1, p(r), 1, p(out))):
            assert lib.ofc_kpp_sample_dev(0, *args) == _lib.OFC_EINVAL and len(lib.ofc_last_error()) > 0
            assert np.all(out == -1)
        w.free()
        assert seed() == _lib.OFC_OK and idx[0] == 3 and np.array_equal(cen, X[idx])       # and the call itself works
    finally:
        buf.free()
