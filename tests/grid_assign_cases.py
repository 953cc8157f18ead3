"""What test_grid_assign_host.py and the GPU files of the fused label-and-count (ofc_grid_assign_counts_dev, the streaming
ingest's model) share: fields on motion_grid_cases' lattice at its geometries, centre sets per k that leave no lattice
point ambiguous, and the numpy model of the answer (the direct-form float64 argmin, counted by MC.model_counts)."""
import functools

import numpy as np

from tests import motion_grid_cases as MC

# seed per k of centres(): found by search, asserted by test_grid_assign_host.py
CENTRE_SEEDS = {1: 0, 2: 0, 5: 2, 6: 6, 8: 0, 9: 14, 16: 6}
GAP = 1e-3                                  # every lattice point's best and second-best squared distance differ by more
DYADIC_MEAN = np.array([0.375, -1.25])      # x - mean is exact in f64 for every lattice point
TIE_CENTRES = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0]])      # the nearest is tied at 97 lattice points


def centres(k):
    """(k, 2) f64, four decimals, inside the lattice's square"""
    return np.round(np.random.default_rng(1000 * k + CENTRE_SEEDS[k]).uniform(-3.6, 3.6, (k, 2)), 4)


def lattice_gap(cen, shift=(0.0, 0.0)):
    """smallest difference between the best and the second-best direct-form squared distance over the whole lattice,
    lattice and centres both moved by -shift (inf for a single centre)"""
    if len(cen) < 2:
        return np.inf
    shift = np.asarray(shift, np.float64)
    d = np.sort(MC.direct_sqdist(MC.lattice() - shift, np.asarray(cen, np.float64) - shift), axis=1)
    return float((d[:, 1] - d[:, 0]).min())


def field(geom, seed=7):
    """(n, H, W, 2) f32 on the lattice at the size of MC.GEOMETRIES[geom], drawn as MC.assign_field draws its field"""
    rows, cols, W, H, n = MC.GEOMETRIES[geom]
    rng = np.random.default_rng(seed)
    return (rng.integers(-32, 33, (n, H, W, 2)) / 8.0).astype(np.float32)


def model_labels(flow, cen):
    """the direct-form float64 argmin (first minimum), (n, H, W) u8"""
    flow = np.asarray(flow)
    return np.argmin(MC.direct_sqdist(flow.reshape(-1, 2), cen), axis=1).astype(np.uint8).reshape(flow.shape[:-1])


def expanded_labels(flow, cen_c, mean=(0.0, 0.0)):
    """numpy's first minimum of cn - 2 x.c in float64: the kernel's own form, for inputs on which every step is exact"""
    x = np.asarray(flow, np.float64).reshape(-1, 2) - np.asarray(mean, np.float64)
    cen_c = np.asarray(cen_c, np.float64)
    cn = cen_c[:, 0] * cen_c[:, 0] + cen_c[:, 1] * cen_c[:, 1]
    d = cn[None] - 2.0 * (x[:, :1] * cen_c[None, :, 0] + x[:, 1:] * cen_c[None, :, 1])
    return np.argmin(d, axis=1).astype(np.uint8).reshape(np.asarray(flow).shape[:-1])


@functools.lru_cache(maxsize=None)
def case(geom, k):
    """field, centres, expected labels, counts and sums of one (geometry, k), computed once and read-only"""
    rows, cols = MC.GEOMETRIES[geom][:2]
    fl, cen = field(geom), centres(k)
    lab = model_labels(fl, cen)
    counts, sums = MC.model_counts(lab, k, rows, cols, fl)
    for a in (fl, cen, lab, counts, sums):
        a.setflags(write=False)
    return fl, cen, lab, counts, sums
