"""The fused flow iteration after its waits were moved off its own stores: a pure rescheduling, so every flow field keeps
the bits it had before (tests/golden/flow_iter_digests.json, recorded from the commit before the change by
tests/golden/make_flow_iter_digests.py).  The cases (tests/flow_iter_sched_cases.py) are the smallest shapes at which the
march's store and wait paths differ.

Bars:
  1. digest: SHA-256 of the float32 field equals the recorded one.
  2. oracle: relative L2 <= 1e-4 and max|d| <= 1e-3 px against oracle/farneback_ref.c per pair (the project's end-to-end
     bars), so that the test still means something if the golden is ever regenerated.
  3. column sums: the kernel adds the float32 vectors it stores in float64, in its own order; numpy adds the same numbers
     in another.  Each of the two sums of N terms is within N * 2^-53 * sum|x| of the exact one, so they differ by at most
     2 * N * 2^-53 * sum|x|.  The field stored with the sums has the digest of the field stored without."""
import numpy as np
import pytest

import flow_iter_sched_cases as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def digests():
    return K.load_digests()


@pytest.fixture(scope="module")
def batch():
    """the three-pair batch, computed once and shared read-only"""
    flows = K.run(K.BATCH)
    flows.setflags(write=False)
    return flows


def _assert_oracle(name, flows):
    _, _, _, kw = K.CASES[name]
    fr = K.frames(name)
    p = O.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    for t in range(len(flows)):
        want = O.farneback(fr[t], fr[t + 1], p)
        d = flows[t].astype(np.float64) - want
        rel = np.linalg.norm(d.ravel()) / np.linalg.norm(want.ravel().astype(np.float64))
        mx = np.abs(d).max()
        print(f"{name} pair {t}: rel {rel:.3e} max {mx:.3e}")
        assert rel <= K.REL_BAR and mx <= K.MAX_BAR, (name, t, rel, mx)


@pytest.mark.parametrize("name", [n for n in K.CASES if n != K.BATCH])
def test_single_pair_keeps_its_bits(name, digests):
    flows = K.run(name)
    _assert_oracle(name, flows)
    assert K.digest(flows) == digests[name], name


def test_batch_keeps_its_bits(batch, digests):
    _assert_oracle(K.BATCH, batch)
    assert K.digest(batch) == digests[K.BATCH]


def test_batch_with_column_sums(batch, digests):
    flows, uv = K.run(K.BATCH, sums=True)
    assert K.digest(flows) == digests[K.BATCH]
    assert np.array_equal(flows, batch)
    x = flows.astype(np.float64).reshape(-1, 2)
    want, bar = x.sum(0), 2 * len(x) * 2.0 ** -53 * np.abs(x).sum(0)
    print("sums", uv, "numpy", want, "bar", bar)
    assert np.all(np.abs(uv - want) <= bar), (uv, want, bar)
