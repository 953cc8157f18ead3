"""Weighted Lloyd on the host: the float64 numpy model of tests/lloyd_weighted_cases.py against scikit-learn's goldens
(tests/golden/make_lloyd_weighted_goldens.py, scikit-learn 1.7.2), the conditioning of every case the GPU tests use, and
sharded.fit_sharded's weighted relocation over a numpy-backed shard.

Bars (the project's GPU-vs-oracle bars): labels bit-equal, n_iter equal, centres <= 1e-9, inertia <= 1e-10
relative.  Holding them here pins the model for the one case that is too large to store.
"""
import os
import threading

import numpy as np
import pytest

from opticalflowclustering_amd.sharded import fit_sharded
from tests import lloyd_weighted_cases as M

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "lloyd_weighted_goldens.npz"))
CASES = sorted({k.split("/")[0] for k in Z.files if "/" in k})
# row at which the two-shard runs cut the data: the relocation winners (make_lloyd_weighted_goldens.py plants them at rows
# 7; 3; 11; 5 and 70) sit on shard 1, for reloc_two_empty one on either shard.  Uneven everywhere.
CUTS = {"reloc_it0_w2p5_f64": 5, "reloc_zero_weight_cluster_f32": 2, "reloc_zero_weight_cluster_f32_maxit3": 2,
        "reloc_sample_weight0_f64": 8, "reloc_two_empty_u8": 40, "reloc_dist0_u8_d4": 6, "cov_float32_d2_k8_wfloat32": 30,
        "int_uint8_d2_k9_wfloat64": 50, "size_N3": 1, "stop_tol0.01": 130}


def case(name):
    return (Z[name + "/X"], Z[name + "/w"], Z[name + "/C0"], int(Z[name + "/max_iter"]), float(Z[name + "/tol"]))


def assert_fit(name, cen, lab, inertia, n_iter):
    ref = float(Z[name + "/inertia"])
    assert n_iter == int(Z[name + "/n_iter"]), name
    assert np.array_equal(lab, Z[name + "/labels"]), name
    assert np.abs(cen - Z[name + "/centers"]).max() <= 1e-9, name
    assert abs(inertia - ref) <= 1e-10 * ref, (name, inertia, ref)


def test_golden_file_is_what_the_generator_describes():
    assert str(Z["sklearn_version"]) == "1.7.2"
    assert len(CASES) == 171 and sum(c.startswith("cov_") for c in CASES) == 120 and sum(c.startswith("int_") for c in CASES) == 30
    assert max(len(Z[c + "/X"]) for c in CASES) <= 400
    assert {len(Z[c + "/X"]) % 4 for c in CASES if c.startswith("size_Nmod")} == {0, 1, 2, 3}
    assert {int(Z[c + "/n_iter"]) for c in CASES if c.startswith("maxit_0")} == {1, 2, 3, 5}
    assert int(Z["reloc_zero_weight_cluster_f32/n_iter"]) > 3 == int(Z["reloc_zero_weight_cluster_f32_maxit3/n_iter"])
    X, w, C0, _, _ = case("reloc_zero_weight_cluster_f32")            # iteration 0: cluster 2 owns 30 samples that weigh nothing
    lab0 = M.e_step(X.astype(np.float64), C0)
    assert np.count_nonzero(lab0 == 2) == 30 and np.all(w[lab0 == 2] == 0) and np.all(w[lab0 != 2] > 0)
    X, w, C0, _, _ = case("reloc_sample_weight0_f64")                 # the farthest sample of iteration 0 weighs nothing
    lab0 = M.e_step(X, C0)
    assert w[np.argmax(((X - C0[lab0]) ** 2).sum(1))] == 0 and np.count_nonzero(w == 0) == 1
    for c in ("wide_1e-6_1e6_f64_d3_k4", "wide_1e-6_1e6_f32_d2_k5_wf32"):
        assert Z[c + "/w"].min() < 1e-5 and Z[c + "/w"].max() > 1e5
    assert {str(Z[c + "/w"].dtype) for c in CASES} == {"float32", "float64"}


def test_rounding_bound_is_the_independent_oracle_tests():
    from tests.test_oracle_lloyd_independent import expanded_bound
    X, _, C0, _, _ = case("cov_float64_d3_k8_wfloat64")
    mean = X.mean(axis=0)
    assert np.array_equal(M.expanded_bound(X - mean, C0 - mean), expanded_bound(X, mean, C0 - mean))


@pytest.mark.parametrize("name", CASES)
def test_model_reproduces_sklearn(name):
    X, w, C0, max_iter, tol = case(name)
    assert_fit(name, *M.model_fit(X, w, C0, max_iter, tol))


@pytest.mark.parametrize("name", CASES)
def test_case_is_well_conditioned(name):
    """no sample of any E-step of the fit inside the rounding bound of the expanded distance (share left out: 0), every
    shift-against-tol decision at least a factor 2 from equality.  A failing case is reseeded in the generator."""
    X, w, C0, max_iter, tol = case(name)
    out, factor = M.conditioning(X, w, C0, max_iter, tol)
    assert out == 0 and factor >= 2, (name, out, factor)


def test_large_case_is_well_conditioned_and_weighted():
    X, w, C0 = M.large_case()
    assert X.shape == (M.LARGE_N, 2) and M.LARGE_N % 4 == 3 and X.dtype == w.dtype == np.float32
    assert np.array_equal(X, np.rint(X)) and 0.05 < np.mean(w == 0) < 0.2 and w.max() == 3.0
    out, factor = M.conditioning(X, w, C0, 300, 0.0)
    assert out == 0 and factor >= 2, (out, factor)
    cen, lab, inertia, n_iter = M.model_fit(X, w, C0, 300, 0.0)
    assert 2 <= n_iter <= 6 and np.bincount(lab).min() > M.LARGE_N // 4
    cen1, _, _, _ = M.model_fit(X, np.ones(len(X)), C0, 300, 0.0)
    assert np.abs(cen - cen1).max() > 1e-6                      # the weights matter to the answer


def test_integer_weights_equal_repeated_rows():
    """tol = 0: fit(X, sample_weight=w) and fit(np.repeat(X, w)) are the same fit (checked for the model here, as the issue
    reports for sklearn)"""
    X, w, C0, _, _ = case("int_float32_d2_k8_wfloat64")
    wi = w.astype(np.int64)
    cen, lab, inertia, n_iter = M.model_fit(X, w, C0, 300, 0.0)
    cen_r, lab_r, inertia_r, n_iter_r = M.model_fit(np.repeat(X, wi, axis=0), np.ones(wi.sum()), C0, 300, 0.0)
    assert n_iter == n_iter_r and np.array_equal(np.repeat(lab, wi), lab_r)
    assert np.abs(cen - cen_r).max() <= 1e-9 and abs(inertia - inertia_r) <= 1e-10 * inertia


@pytest.mark.parametrize("name", CASES)
def test_fit_sharded_one_numpy_shard(name):
    X, w, C0, max_iter, tol = case(name)
    shard = M.NumpyShard(X, w)
    cen, inertia, n_iter = fit_sharded(shard, C0, max_iter, tol)
    assert_fit(name, cen, shard.labels, inertia, n_iter)


@pytest.mark.parametrize("name", sorted(CUTS))
def test_fit_sharded_two_numpy_shards(name):
    """two uneven shards, one thread each, an in-process all-reduce; the relocation winner sits on shard 1"""
    X, w, C0, max_iter, tol = case(name)
    cut = CUTS[name]
    shards = [M.NumpyShard(X[:cut], w[:cut]), M.NumpyShard(X[cut:], w[cut:])]
    reduces = M.threaded_allreduce(2)
    res = [None, None]

    def work(rank):
        try:
            res[rank] = fit_sharded(shards[rank], C0, max_iter, tol, allreduce=reduces[rank], rank=rank)
        except BaseException as e:                             # noqa: BLE001  (reported by the assert below)
            res[rank] = e
    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(isinstance(r, BaseException) or r is None for r in res), res
    labels = np.concatenate([shards[0].labels, shards[1].labels])
    for cen, inertia, n_iter in res:
        assert_fit(name, cen, labels, inertia, n_iter)
    assert np.array_equal(res[0][0], res[1][0])


def test_fit_sharded_keeps_backends_without_weights():
    """a backend whose farthest() returns four values and whose records hold counts (the oracle-backed shard of
    tests/test_dist_gloo.py is one): the relocated sample weighs 1"""
    class Unweighted(M.NumpyShard):
        def farthest(self, mean, centers_c, excl):
            return super().farthest(mean, centers_c, excl)[:4]
    X, w, C0, max_iter, tol = case("reloc_it0_w2p5_f64")
    ones = np.ones(len(X))
    shard = Unweighted(X, ones)
    cen, inertia, n_iter = fit_sharded(shard, C0, max_iter, tol)
    ref_cen, ref_lab, ref_inertia, ref_n = M.model_fit(X, ones, C0, max_iter, tol)
    assert n_iter == ref_n and np.array_equal(shard.labels, ref_lab)
    assert np.abs(cen - ref_cen).max() <= 1e-9 and abs(inertia - ref_inertia) <= 1e-10 * ref_inertia


def test_fit_sharded_refuses_weights_that_sum_to_zero():
    X, w, C0, _, _ = case("size_Nmod1")
    with pytest.raises(ValueError, match="sum of sample weights must be positive"):
        fit_sharded(M.NumpyShard(X, np.zeros(len(X))), C0)


def test_weight_arguments_are_checked_before_the_device_is_touched():
    """KMeans.fit / score: sklearn's _check_sample_weight refusals, the zero sum, and k-means++ with weights"""
    from opticalflowclustering_amd.cluster import KMeans, _as_weights
    X = np.zeros((6, 2), np.float32)
    km = KMeans(n_clusters=2, init=np.zeros((2, 2)))
    for bad, msg in ((np.ones(5), "sample_weight.shape"), (-np.ones(6), "Negative"), (np.full(6, np.nan), "NaN or infinity"),
                     (np.zeros(6), "must be positive"), (np.ones((6, 1)), "1D array")):
        with pytest.raises(ValueError, match=msg):
            km.fit(X, sample_weight=bad)
    with pytest.raises(ValueError, match="k-means\\+\\+"):
        KMeans(n_clusters=2, init="k-means++").fit(X, sample_weight=np.ones(6))
    assert _as_weights(None, 6) is None
    assert _as_weights(2, 3).dtype == np.float64 and np.array_equal(_as_weights(2, 3), [2.0, 2.0, 2.0])
    assert _as_weights(np.ones(4, np.float32), 4).dtype == np.float32
    assert _as_weights(np.ones(4, np.int32), 4).dtype == _as_weights(np.ones(4, np.float16), 4).dtype == np.float64
