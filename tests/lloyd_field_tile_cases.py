"""Shared by test_lloyd_field_layout_host.py and test_gpu_lloyd_field_tiles.py: the layout of the 2-D tiles that
csrc/lloyd_tiles.hip's field kernels sweep (csrc/lloyd_field.h), mirrored in numpy, a float64 model of their two-level
box test built on lloyd_tile_cases.box_verdict (TileCtx::box_label's arithmetic and margin), and the fields of the tests.

Every field is made of motion populations whose centres are at least 1 apart, with noise of at most 1e-3 around them (or
none), so that a box is either far inside one Voronoi cell or holds samples of two populations: no verdict depends on the
last bits, and the device's counts must equal the model's exactly.
"""
import functools

import numpy as np

from lloyd_tile_cases import box_verdict
from oracle import oracle as O

GROUP_W, GROUP_H = 64, 8            # lloyd_field.h: FIELD_GW, FIELD_GH
POP = np.array([[-2.0, 0.5], [1.0, -1.5], [2.5, 2.0], [-1.0, -3.0]])      # population centres, >= 1 apart
NOISE = 1e-3


# ------------------------------------------------------------------------------------------------ layout
def quad_origins(W, H, n, tile_w=16, tile_h=4):
    """numpy mirror of field_quad_origin: (NT, 16) index of the first of the 4 samples of every quad of every tile of a
    stack of n fields of W x H, tiles numbered group-major"""
    assert W % GROUP_W == 0 and H % GROUP_H == 0 and tile_w * tile_h == 64
    gtx, qpr = GROUP_W // tile_w, tile_w // 4
    g = np.arange(n * (H // GROUP_H) * (W // GROUP_W), dtype=np.int64)
    band, col = g // (W // GROUP_W), g % (W // GROUP_W)
    origin = band * GROUP_H * W + col * GROUP_W                                   # (NG,)
    ti = np.arange(8)
    tile = (ti // gtx) * tile_h * W + (ti % gtx) * tile_w                         # (8,)
    r = np.arange(16)
    quad = (r // qpr) * W + (r % qpr) * 4                                         # (16,)
    return (origin[:, None, None] + tile[None, :, None] + quad[None, None, :]).reshape(-1, 16)


def tile_samples(W, H, n, **kw):
    """(NT, 64) sample indices of every tile"""
    return (quad_origins(W, H, n, **kw)[:, :, None] + np.arange(4)[None, None, :]).reshape(-1, 64)


# ------------------------------------------------------------------------------------------------ the model
def field_report(X, W, H, mean, cc, factor=1e-12):
    """the two-level test of k_lloyd_tiles_field against the CENTRED centres cc: a group's box first, then the boxes of the
    8 tiles of a group that failed.  A box with a NaN in it never passes (k_tile_meta_field poisons it).
    -> dict(tested, pure: the trace line's counts in tiles; group_pass (NG,), tile_pass (NT,): who was not read)"""
    X = np.asarray(X)
    n = len(X) // (W * H)
    T = X[tile_samples(W, H, n)].astype(np.float64)                  # (NT, 64, 2)
    with np.errstate(invalid="ignore"):
        tlo, thi = T.min(1), T.max(1)
        G = T.reshape(-1, 8 * 64, 2)
        glo, ghi = G.min(1), G.max(1)
        tbad, gbad = np.isnan(T).any((1, 2)), np.isnan(G).any((1, 2))
        tp = box_verdict(np.nan_to_num(tlo), np.nan_to_num(thi), mean, cc, factor)[1] & ~tbad
        gp = box_verdict(np.nan_to_num(glo), np.nan_to_num(ghi), mean, cc, factor)[1] & ~gbad
    tile_pass = tp | np.repeat(gp, 8)
    return {"tested": len(T), "pure": int(8 * gp.sum() + tp[~np.repeat(gp, 8)].sum()), "group_pass": gp, "tile_pass": tile_pass,
            "tile_pure_alone": tp}


def borderline(X, W, H, mean, cc):
    """boxes whose verdict changes for a margin factor in [1e-13, 1e-11] (none allowed, as in lloyd_tile_cases)"""
    a, b, c = (field_report(X, W, H, mean, cc, f) for f in (1e-13, 1e-12, 1e-11))
    return int(((a["tile_pure_alone"] != c["tile_pure_alone"]) | (a["tile_pure_alone"] != b["tile_pure_alone"])).sum()
               + ((a["group_pass"] != c["group_pass"]) | (a["group_pass"] != b["group_pass"])).sum())


# ------------------------------------------------------------------------------------------------ fields
def populations(pop, noise=NOISE, seed=0):
    """pop: (n, H, W) integer population of every pixel -> (N, 2) float32 field"""
    rng = np.random.default_rng(seed)
    X = POP[pop] + (noise * rng.uniform(-1, 1, pop.shape + (2,)) if noise else 0.0)
    return np.ascontiguousarray(X.reshape(-1, 2), np.float32)


def grid(W, H, n):
    f, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing="ij")
    return f, y, x


def _vertical(W, H, n):        # edge at x = 40: tile column 2 of group column 0 is mixed in every band
    f, y, x = grid(W, H, n)
    return (x >= 40).astype(int)


def _horizontal(W, H, n):      # edge at y = 5: the lower tile row of band 0 is mixed
    f, y, x = grid(W, H, n)
    return (y >= 5).astype(int)


def _diagonal(W, H, n):
    f, y, x = grid(W, H, n)
    return ((x + 3 * y + 11 * f) >= (W + 3 * H) // 2).astype(int)


def _aligned(W, H, n):         # edges on group borders only: every group passes
    f, y, x = grid(W, H, n)
    return ((x // GROUP_W + y // GROUP_H + f) % 2).astype(int)


def _one_tile(W, H, n):        # one pixel of the other population: exactly one tile of one group is mixed
    pop = np.zeros((n, H, W), int)
    pop[:, :, W // 2:] = 1
    pop[n - 1, H - 6, 21] = 1
    return pop


def _three(W, H, n):           # three populations, k = 3: vertical bands with a slanted border
    f, y, x = grid(W, H, n)
    return np.minimum(2, (3 * x + y + 5 * f) * 3 // (3 * W + H + 5 * n)).astype(int)


def _stripes(W, H, n):         # slanted stripes 100 px wide: dozens of failing groups in every chunk of 64
    f, y, x = grid(W, H, n)
    return (((x + 2 * y + 7 * f) // 100) % 2).astype(int)


def _layout(W, H, n):          # field 0: group-sized blocks, field 1: tile-sized (16 x 4), the others: quad-sized (4 x 1)
    f, y, x = grid(W, H, n)
    by_group, by_tile, by_quad = (x // 64 + y // 8) % 2, (x // 16 + y // 4) % 2, (x // 4 + y) % 2
    return np.where(f == 0, by_group, np.where(f == 1, by_tile, by_quad)).astype(int)


CONTENTS = {"vertical": _vertical, "horizontal": _horizontal, "diagonal": _diagonal, "aligned": _aligned,
            "one-tile": _one_tile, "three": _three, "stripes": _stripes, "layout": _layout}
# name -> (content, W, H, n)
CASES = {
    "one-group": ("vertical", 64, 8, 1),
    "vertical-128x16x3": ("vertical", 128, 16, 3),
    "horizontal-128x16x3": ("horizontal", 128, 16, 3),
    "diagonal-128x16x3": ("diagonal", 128, 16, 3),
    "diagonal-192x24x2": ("diagonal", 192, 24, 2),
    "aligned-128x16x3": ("aligned", 128, 16, 3),
    "one-tile-128x16x3": ("one-tile", 128, 16, 3),
    "three-192x24x2": ("three", 192, 24, 2),
    "layout-128x16x3": ("layout", 128, 16, 3),
    "bench-width-1920x8x2": ("diagonal", 1920, 8, 2),
    "many-chunks-4096x16x2": ("stripes", 4096, 16, 2),        # 256 groups: 4 chunks of 64, several waves
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: the field, its start centres, the oracle's fit, and the model's report of every sweep and of the final
    E-step (computed once, read-only)"""
    content, W, H, n = CASES[name]
    pop = CONTENTS[content](W, H, n)
    X = populations(pop, seed=len(name))
    k = int(pop.max()) + 1
    C0 = POP[:k] + np.array([0.3, -0.2])
    cen, lab, inertia, n_iter = O.kmeans_fit(X, C0)
    mean = X.astype(np.float64).mean(0)
    centres = [C0] + [O.kmeans_fit(X, C0, i)[0] for i in range(1, n_iter)] + [cen]
    reports = [field_report(X, W, H, mean, c - mean) for c in centres]
    X.setflags(write=False)
    return dict(X=X, W=W, H=H, n=n, C0=C0, pop=pop, cen=cen, lab=lab, inertia=inertia, n_iter=n_iter, mean=mean,
                sweeps=reports[:-1], final=reports[-1],
                borderline=sum(borderline(X, W, H, mean, c - mean) for c in centres))


def constant_field(W, H, n):
    """every sample the same vector, k = 1"""
    X = np.empty((n * W * H, 2), np.float32)
    X[:] = (1.25, -0.75)
    return X, np.array([[1.0, -1.0]])


def noise_field(W, H, n, seed=7):
    """white noise over the populations: no two neighbours belong together, almost no box passes"""
    rng = np.random.default_rng(seed)
    return populations(rng.integers(0, 3, (n, H, W)), noise=0.3, seed=seed), POP[:3] + 0.2


def nan_field(W, H, n):
    """two populations split on a group border (every box passes), one NaN sample -> X, C0, index of the bad sample"""
    X = populations(_aligned(W, H, n), seed=3).copy()
    bad = (n - 1) * W * H + 9 * W + 70            # field n-1, row 9, x = 70: band 1, group column 1, tile (0, 0) of its group
    X[bad, 1] = np.nan
    return X, POP[:2] + np.array([0.3, -0.2]), bad
