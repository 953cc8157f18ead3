"""Host side of the device-resident k-means++ seeding (cluster.kpp_draws / kmeans_plusplus_dev): the random numbers
drawn up front are the ones cluster.kmeans_plusplus draws step by step, and every end-to-end case of
test_gpu_kpp_seed.py is proven well-conditioned, so that "index for index" is a fair demand there."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import kpp_seed_cases as KC

KPP = np.load(os.path.join(os.path.dirname(__file__), "golden", "kpp_goldens.npz"))
KPP_CASES = sorted({k.split("/")[0] for k in KPP.files})


class RecordingState(np.random.RandomState):
    """a RandomState that remembers what kmeans_plusplus drew from it"""

    def __init__(self, seed):
        super().__init__(seed)
        self.first, self.uniforms = None, []

    def choice(self, *a, **kw):
        self.first = super().choice(*a, **kw)
        return self.first

    def uniform(self, *a, **kw):
        v = super().uniform(*a, **kw)
        self.uniforms.append(np.array(v))
        return v


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


@pytest.mark.parametrize("name", KPP_CASES)
def test_up_front_draws_are_the_ones_kmeans_plusplus_makes(name):
    """same first index, same uniforms (hence the same rand_vals = u * current_pot), same RandomState afterwards, and the
    host model on those draws picks sklearn's rows"""
    from opticalflowclustering_amd.cluster import kmeans_plusplus, kpp_draws
    X, k, seed = KPP[name + "/X"], int(KPP[name + "/k"]), int(KPP[name + "/seed"])
    rec = RecordingState(seed)
    _, idx = kmeans_plusplus(X, k, rec, _step=O.kpp_candidates)
    rs = np.random.RandomState(seed)
    first, u, n_trials = kpp_draws(rs, len(X), k)
    assert first == rec.first == idx[0]
    assert n_trials == 2 + int(np.log(k)) and u.shape == (k - 1, n_trials)
    assert np.array_equal(u, np.array(rec.uniforms).reshape(k - 1, n_trials))
    assert _same_state(rs, rec)
    got, rand_vals, _ = KC.host_seed(X, k, first, u)
    assert np.array_equal(got, idx) and np.array_equal(got, KPP[name + "/indices"])
    assert all(np.all((rv >= 0) & np.isfinite(rv)) for rv in rand_vals)


def test_large_n_first_index_consumes_exactly_one_draw():
    """above KPP_CHOICE_MAX rows the first index is min(int(random_sample() * N), N - 1): one draw, as rs.choice makes"""
    from opticalflowclustering_amd.cluster import KPP_CHOICE_MAX, kpp_draws
    assert KPP_CHOICE_MAX == 1 << 24
    N = 620_000_000
    rs, ref = np.random.RandomState(5), np.random.RandomState(5)
    first, u, nt = kpp_draws(rs, N, 8)
    x = ref.random_sample()
    assert first == min(int(x * N), N - 1) and 0 <= first < N
    assert np.array_equal(u, np.array([ref.uniform(size=nt) for _ in range(7)]))
    assert _same_state(rs, ref)
    # at the switch itself rs.choice is still used, and it too takes one draw
    rs, ref = np.random.RandomState(9), np.random.RandomState(9)
    small = 1000
    first, _, _ = kpp_draws(rs, small, 1)
    assert first == ref.choice(small, p=np.full(small, 1.0 / small)) and _same_state(rs, ref)


def test_n_local_trials_above_eight_is_refused():
    from opticalflowclustering_amd.cluster import kpp_draws
    with pytest.raises(ValueError):
        kpp_draws(np.random.RandomState(0), 100, 4, n_local_trials=9)


@pytest.mark.parametrize("case", KC.CASES, ids=KC.case_id)
def test_every_end_to_end_case_is_well_conditioned(case):
    """every rand_val lies at least 16 N 2^-52 of the potential from the nearest cumulative-sum boundary: 16 times what
    any summation order of N non-negative terms can move a partial sum, so the device's chunked sums must find the row
    np.cumsum finds.  (Where the potential has reached 0 -- fewer distinct rows than k -- both are exactly 0.)"""
    from opticalflowclustering_amd.cluster import kpp_draws
    _, dt, d, k, N = case
    assert N <= 20000
    X = KC.make_X(case)
    assert X.shape == (N, d) and X.dtype == KC.DTYPES[dt]
    first, u, _ = kpp_draws(np.random.RandomState(KC.case_seed(case)), N, k)
    idx, _, gaps = KC.host_seed(X, k, first, u)
    assert len(gaps) == (k - 1) * u.shape[1]
    for gap, pot in gaps:
        assert gap >= 16 * N * 2.0 ** -52 * pot, (gap, pot)
    assert np.all((idx >= 0) & (idx < N))
