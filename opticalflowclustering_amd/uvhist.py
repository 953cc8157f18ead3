"""A 2-D histogram of flow vectors, and the motion fit on it.

The table (include/ofc.h, "Histogram of flow vectors") carries per bin of the (u,v) plane an exact count and exact
fixed-point sums of its members.  A weighted Lloyd fit over the non-empty bins -- points = the bin means, weights = the
counts, the existing ofc_kmeans_fit_w and kmeans_plusplus(..., sample_weight=) -- stands in for the fit over the field: its
M-step is exact for every bin that lies inside one Voronoi cell, the only approximation is that a bin is assigned as a
whole, and the only arithmetic one is the fixed-point step (2^-17 px per sample).  The table is built in one pass over the
field where the flow left it (uv_hist.hip), is a few MB whatever the clip's length, and merges by addition, so a fit can
cover footage that is never resident (FlowStream(histogram=...), motionGrids --fit-stream); a fit on it takes so little
that n_init restarts and several k come almost free.

Three producers: uv_histogram(flow) for host arrays, ClipPipeline.uv_histogram() for the resident field,
FlowStream(..., histogram=(bins, range)).histogram() for a frame stream."""
import numpy as np

from ._lib import check, load, ptr
from .cluster import KMeans, check_random_state, kmeans_plusplus

FIXED_ONE = 65536.0            # the sums are in units of 2^-16 px


def table_len(bins):
    return 3 * int(bins) * int(bins) + 1


def check_params(bins, range):
    """bins: a power of two in 16 .. 2048, range: a power of two in 2^-4 .. 2^10 (what the library accepts); ValueError"""
    b, r = int(bins), float(range)
    if b != bins or b < 16 or b > 2048 or b & (b - 1):
        raise ValueError(f"bins = {bins!r} is not a power of two in 16 .. 2048")
    if not (2.0 ** -4 <= r <= 2.0 ** 10) or np.frexp(r)[0] != 0.5:
        raise ValueError(f"range = {range!r} is not a power of two in 2^-4 .. 2^10")
    return b, r


def restart_seeds(random_state, n_init):
    """the per-restart seeds of n_init fits, as sklearn's KMeans.fit draws them (_kmeans.py: one randint per restart from
    the checked random_state)"""
    return check_random_state(random_state).randint(np.iinfo(np.int32).max, size=int(n_init))


class UVHistogram:
    """bins, range and the table of 3*bins^2 + 1 int64 (count, sum_u, sum_v, outside) as the library writes it"""

    def __init__(self, bins, range, table):
        self.bins, self.range = check_params(bins, range)
        table = np.ascontiguousarray(table, np.int64).ravel()
        if table.shape != (table_len(self.bins),):
            raise ValueError(f"the table of {self.bins} bins has {table_len(self.bins)} entries, got {table.size}")
        self.table = table

    @property
    def counts(self):
        """(bins, bins) int64, [iv, iu]"""
        B = self.bins
        return self.table[:B * B].reshape(B, B)

    @property
    def outside(self):
        """vectors that fell outside [-range, range) on either axis, NaN and inf included"""
        return int(self.table[-1])

    @property
    def n(self):
        """vectors in range"""
        return int(self.table[:self.bins * self.bins].sum())

    def points(self):
        """the non-empty bins in bin order -> (P (m,2) f64: the mean (u,v) of each bin's members = sum / count / 65536,
        w (m,) f64: their counts)"""
        B2 = self.bins * self.bins
        cnt = self.table[:B2]
        idx = np.flatnonzero(cnt)
        w = cnt[idx].astype(np.float64)
        P = np.empty((len(idx), 2), np.float64)
        P[:, 0] = self.table[B2:2 * B2][idx] / w / FIXED_ONE
        P[:, 1] = self.table[2 * B2:3 * B2][idx] / w / FIXED_ONE
        return P, w

    def merge(self, other):
        """the table of both inputs together (plain addition).  Same bins and range, or ValueError."""
        if not isinstance(other, UVHistogram):
            raise TypeError(f"cannot merge a UVHistogram with {type(other).__name__}")
        if (other.bins, other.range) != (self.bins, self.range):
            raise ValueError(f"histograms differ: bins {self.bins} / range {self.range} against bins {other.bins} / "
                             f"range {other.range}")
        return UVHistogram(self.bins, self.range, self.table + other.table)

    __add__ = merge

    def fit(self, k, init="k-means++", random_state=0, n_init=1, max_iter=300, tol=1e-4, device=0):
        """weighted Lloyd over the bin means -> (centers (k,2), inertia, n_iter).
        init='k-means++': sklearn's weighted fit in its two-step form, C0, _ = kmeans_plusplus(P, k, random_state,
        sample_weight=w), then KMeans(k, init=C0).fit(P, sample_weight=w).  With n_init > 1 that runs n_init times with
        the seeds sklearn derives (restart_seeds) and the first strictly smallest inertia wins; sklearn's extra test that
        two restarts found the same clustering (_is_same_clustering, which only affects which of two equal results is kept) is
        not reproduced.  An explicit (k,2) init runs once, whatever n_init says.
        The inertia is that of the bin means, not of the vectors: it leaves out every bin's own scatter, which does not
        depend on the centres while a bin stays in one cell, so restarts compare as they would on the vectors.
        ValueError on an empty table, or with fewer non-empty bins than k."""
        P, w = self.points()
        if len(P) == 0:
            raise ValueError("the histogram is empty: no vector in range")
        k = int(k)

        def one(C0):
            km = KMeans(k, init=C0, max_iter=max_iter, tol=tol, device=device).fit(P, sample_weight=w)
            return km.cluster_centers_, km.inertia_, km.n_iter_

        if not isinstance(init, str):
            return one(np.asarray(init, np.float64))
        if init != "k-means++":
            raise ValueError(f"init should be 'k-means++' or a (k,2) array, got {init!r}")
        if len(P) < k:
            raise ValueError(f"n_samples={len(P)} should be >= n_clusters={k}.")
        if int(n_init) < 1:
            raise ValueError(f"n_init = {n_init!r} should be at least 1")
        if int(n_init) == 1:
            return one(kmeans_plusplus(P, k, random_state, device=device, sample_weight=w)[0])
        best = None
        for seed in restart_seeds(random_state, n_init):
            res = one(kmeans_plusplus(P, k, int(seed), device=device, sample_weight=w)[0])
            if best is None or res[1] < best[1]:
                best = res
        return best


def uv_histogram(flow, bins=1024, range=32.0, device=0):
    """the histogram of a host flow field (H,W,2), a stack (n,H,W,2), or any (..., 2) array of (u,v) vectors (ofc_uv_hist)"""
    bins, range = check_params(bins, range)
    flow = np.ascontiguousarray(flow, np.float32)
    if flow.ndim < 2 or flow.shape[-1] != 2:
        raise ValueError(f"expected (u,v) vectors in the last axis, got shape {flow.shape}")
    table = np.empty(table_len(bins), np.int64)
    check(load().ofc_uv_hist(device, ptr(flow), flow.size // 2, bins, range, ptr(table)))
    return UVHistogram(bins, range, table)
