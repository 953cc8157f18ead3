"""Shared by test_kpp_seed_host.py and test_gpu_kpp_seed.py: the end-to-end seeding cases, and the host route through the
CPU oracle that the device route must reproduce index for index (it also reports how far every draw lies from the
nearest boundary of the cumulative sum, which is what makes that demand fair)."""
import numpy as np

from oracle import oracle as O

CH = 1024           # = _lib.KPP_CHUNK (asserted by the GPU test): the seams of the chunked cumulative sum
DTYPES = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}


def _cases():
    out = []
    for dt in DTYPES:
        for d in (1, 2, 4):
            for k in (1, 2, 8, 16):
                for N in (k, CH + 1, 3 * CH + 7):
                    out.append(("rand", dt, d, k, N))
    for dt in DTYPES:                      # fewer distinct rows than k: the potential reaches zero before the last centre
        for k, N in ((8, 8), (8, CH + 1), (16, 3 * CH + 7)):
            out.append(("dup", dt, 2, k, N))
    return out


CASES = _cases()
assert max(c[4] for c in CASES) <= 20000


def case_id(c):
    return "-".join(str(v) for v in c)


def case_seed(c):
    return CASES.index(c)


def make_X(c):
    kind, dt, d, k, N = c
    rng = np.random.default_rng(1000 + CASES.index(c))
    if kind == "rand":
        if dt == "u8":
            return rng.integers(0, 256, (N, d)).astype(np.uint8)
        return (rng.normal(size=(N, d)) * 3 + rng.integers(0, 4, (N, 1)) * 5).astype(DTYPES[dt])
    # 'dup': three rows and their mirror images about 50 (plus the centre row when N is odd).  The column mean is 50 and
    # every product and sum below is a small multiple of 1/4: exact in any order, on the host and on the device, so the
    # distance of a chosen row to itself is 0 and the zero potential at the end is reached exactly on both routes
    base = np.array([[10, 90], [30, 20], [70, 60]])
    rows = np.concatenate([base, 100 - base])
    pick = rng.integers(0, 3, N // 2)
    X = np.concatenate([base[pick], 100 - base[pick]] + ([[[50, 50]]] if N % 2 else []))
    assert len(np.unique(X, axis=0)) < k and len(X) == N and set(map(tuple, X)) <= set(map(tuple, rows)) | {(50, 50)}
    return np.ascontiguousarray(X[rng.permutation(N)].astype(DTYPES[dt]))


def host_mean(X):
    """the mean cluster.kmeans_plusplus centres by"""
    return X.astype(np.float64).mean(axis=0) if X.dtype != np.float32 else X.mean(axis=0).astype(np.float64)


def host_seed(X, k, first, u):
    """sklearn's _kmeans_plusplus on pre-drawn numbers, the CPU oracle as the distance step (what
    cluster.kmeans_plusplus(..., _step=O.kpp_candidates) computes).
    -> indices, rand_vals per step, and per draw (gap to the nearest cumulative-sum boundary, potential)"""
    N = len(X)
    mean = host_mean(X)
    idx = np.full(k, -1, np.int64)
    idx[0] = first
    out, pots = O.kpp_candidates(X, mean, idx[:1])
    closest, pot = out[0], pots[0]
    rand_vals, gaps = [], []
    for c in range(1, k):
        rv = u[c - 1] * pot
        cum = np.cumsum(closest, dtype=np.float64)
        ids = np.searchsorted(cum, rv)
        np.clip(ids, None, N - 1, out=ids)
        rand_vals.append(rv)
        gaps += [(float(np.abs(cum - r).min()), float(pot)) for r in rv]
        out, pots = O.kpp_candidates(X, mean, ids, closest)
        best = int(np.argmin(pots))
        pot, closest = pots[best], out[best]
        idx[c] = ids[best]
    return idx, rand_vals, gaps
