"""Connected components of a key map (include/ofc.h "Moving objects", blobs.hip, blobs.py): a plain Python reference of the
definition, and the case table test_blobs_host.py (which proves each case has the property it is named for, on the CPU) and
test_gpu_blobs.py share.  The tile size is read from ofc.h, so the seams the cases aim at move with the constants."""
import collections
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "ofc.h")) as _f:
    _H = _f.read()
TW = int(re.search(r"#define\s+OFC_BLOB_TILE_W\s+(\d+)", _H).group(1))
TH = int(re.search(r"#define\s+OFC_BLOB_TILE_H\s+(\d+)", _H).group(1))
NF = int(re.search(r"#define\s+OFC_BLOB_FIELDS\s+(\d+)", _H).group(1))
BG = 255
FIELDS = ("root", "key", "area", "xmin", "ymin", "xmax", "ymax", "sx", "sy", "nvalid", "squ", "sqv")

Case = collections.namedtuple("Case", "name keys flow")
Case.__repr__ = lambda c: c.name


def neighbours(connectivity):
    """the earlier half of a pixel's neighbourhood in raster order, as (dy, dx)"""
    return ((0, -1), (-1, 0)) if connectivity == 4 else ((0, -1), (-1, -1), (-1, 0), (-1, 1))


def label_one(keys, connectivity):
    """(H,W) u8 -> (H,W) int32 label map of the definition, by union-find with the smaller index as the root"""
    H, W = keys.shape
    k = keys.tolist()
    parent = list(range(H * W))

    def find(i):
        r = i
        while parent[r] != r:
            r = parent[r]
        while parent[i] != r:
            parent[i], i = r, parent[i]
        return r

    nb = neighbours(connectivity)
    for y in range(H):
        for x in range(W):
            if k[y][x] == BG:
                continue
            for dy, dx in nb:
                yy, xx = y + dy, x + dx
                if 0 <= yy and 0 <= xx < W and k[yy][xx] == k[y][x]:
                    a, b = find(y * W + x), find(yy * W + xx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    out = np.full(H * W, -1, np.int32)
    for i in range(H * W):
        if k[i // W][i % W] != BG:
            out[i] = find(i)
    return out.reshape(H, W)


def quantise(v):
    """llrint((double)v * 65536) of an f32: the product is exact in f64, Python's round is to nearest even"""
    return round(float(np.float64(v) * 65536.0))


def records_one(keys, labels, flow=None):
    """every component's record, ascending by root: a list of 12 Python ints each"""
    H, W = keys.shape
    rec = {}
    lab, k = labels.tolist(), keys.tolist()
    f = None if flow is None else np.asarray(flow, np.float32)
    for y in range(H):
        for x in range(W):
            r = lab[y][x]
            if r < 0:
                continue
            t = rec.get(r)
            if t is None:
                t = rec[r] = [r, k[y][x], 0, x, y, x, y, 0, 0, 0, 0, 0]
            t[2] += 1
            t[3], t[4], t[5], t[6] = min(t[3], x), min(t[4], y), max(t[5], x), max(t[6], y)
            t[7] += x
            t[8] += y
            if f is not None:
                u, v = f[y, x]
                if np.isfinite(u) and np.isfinite(v) and abs(u) < 1024 and abs(v) < 1024:
                    t[9] += 1
                    t[10] += quantise(u)
                    t[11] += quantise(v)
    return [rec[r] for r in sorted(rec)]


@functools.lru_cache(maxsize=None)
def _reference(name, connectivity):
    c = BY_NAME[name]
    labels = np.stack([label_one(k, connectivity) for k in c.keys])
    recs = [records_one(c.keys[i], labels[i], None if c.flow is None else c.flow[i]) for i in range(len(c.keys))]
    labels.setflags(write=False)
    return labels, recs


def reference(case, connectivity):
    """-> (labels (n,H,W) int32, read-only; per pair the list of all records by root).  Computed once per case."""
    return _reference(case.name, connectivity)


def table(recs, min_area=1, max_blobs=4096):
    """the definition's table of one pair from all its records -> (records (n,12) int64, found)"""
    keep = [r for r in recs if r[2] >= min_area]
    found = len(keep)
    if found > max_blobs:
        keep = []
    return np.array(keep, np.int64).reshape(-1, NF), found


# ---- fields for the sums ----
HALF = 1.0 / 131072.0            # half a unit of the fixed point: odd multiples are ties of llrint
SPECIALS = np.array([[-0.0, 0.0], [np.nan, 1.0], [1.0, np.inf], [-np.inf, -np.inf], [1023.99, -1023.99], [1024.0, 2.0],
                     [3.0, -1024.0], [-HALF, -3 * HALF], [-5 * HALF, 5 * HALF], [3 * HALF, -7 * HALF], [7.0, -3.0]], np.float32)


def field_for(keys, seed):
    """(n,H,W,2) f32: fractional vectors (multiples of 1/256) on even rows, integer-valued ones on odd rows, and SPECIALS
    on every pair's first foreground pixels, so that they fall inside components"""
    r = np.random.default_rng(seed)
    n, H, W = keys.shape
    f = (r.integers(-2048, 2049, (n, H, W, 2)) / 256.0).astype(np.float32)
    f[:, 1::2] = np.rint(f[:, 1::2])
    for i in range(n):
        ys, xs = np.nonzero(keys[i] != BG)
        step = max(1, len(ys) // (2 * len(SPECIALS)))
        for j, s in enumerate(SPECIALS):
            if j * step < len(ys):
                f[i, ys[j * step], xs[j * step]] = s
    return f


# ---- patterns ----
def _blank(W, H, n=1):
    return np.full((n, H, W), BG, np.uint8)


def random_mask(W, H, n, density, seed, keys=(0, 15, 254)):
    r = np.random.default_rng(seed)
    k = np.asarray(keys, np.uint8)[r.integers(0, len(keys), (n, H, W))]
    k[r.random((n, H, W)) >= density] = BG
    return k


def checkerboard(W, H):
    k = _blank(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    k[0][(yy + xx) % 2 == 0] = 0
    return k


def serpentine(W, H):
    """a one-pixel path: every even row in full, joined alternately at its right and left end"""
    k = _blank(W, H)
    k[0, 0::2, :] = 7
    for j, y in enumerate(range(1, H - 1, 2)):
        k[0, y, W - 1 if j % 2 == 0 else 0] = 7
    return k


def comb(W, H):
    k = _blank(W, H)
    k[0, :, 0::2] = 3
    k[0, H - 1, :] = 3
    return k


def u_shape(W, H):
    k = _blank(W, H)
    k[0, :, 1] = 9
    k[0, :, W - 2] = 9
    k[0, H - 1, 1:W - 1] = 9
    return k


def rings(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.minimum(np.minimum(xx, yy), np.minimum(W - 1 - xx, H - 1 - yy))
    return np.array([0, 15, 254, BG], np.uint8)[d % 4][None]


def diagonals(W, H):
    """a diagonal through the tile corner (TW, TH) and an anti-diagonal through (2 TW, TH): connected under 8 only"""
    k = _blank(W, H)
    for t in range(-3, 3):
        k[0, TH + t, TW + t] = 1
    for t in range(-1, 5):                                     # from the image's last column down to the left
        k[0, TH + t, 2 * TW - 1 - t] = 2
    return k


def seam_touch(W, H):
    """equal-key rectangles that meet only across a seam: by an edge over the column seam (key 4), by an edge over the row
    seam (key 15), and by a corner over the column seam (key 6: one component under 8, two under 4)"""
    k = _blank(W, H)
    k[0, 2:7, TW - 5:TW] = 4
    k[0, 6:11, TW:TW + 5] = 4
    k[0, TH - 4:TH, 10:15] = 15
    k[0, TH:TH + 4, 14:19] = 15
    k[0, TH + 6:TH + 9, TW - 3:TW] = 6
    k[0, TH + 9:TH + 12, TW:TW + 3] = 6
    return k


def seam_singles(W, H):
    k = _blank(W, H)
    for x, y in ((TW - 1, 3), (TW, 7), (5, TH - 1), (9, TH), (2 * TW - 1, TH - 1), (2 * TW, TH), (0, 0), (W - 1, 0), (0, H - 1),
                 (W - 1, H - 1)):
        k[0, y, x] = 0
    return k


def stripes(W, H):
    k = _blank(W, H)
    k[0] = np.array([0, 15, 254], np.uint8)[(np.arange(W) // 5) % 3][None, :]
    k[0, H // 2] = 15                                          # a bar that joins the stripes of key 15
    return k


def inter_pair(W, H):
    k = _blank(W, H, 2)
    k[0, H - 1] = 5
    k[1, 0] = 5
    return k


def _cases():
    out = []

    def add(name, keys, flow_seed=None):
        keys = np.ascontiguousarray(keys, np.uint8)
        keys.setflags(write=False)
        flow = None if flow_seed is None else field_for(keys, flow_seed)
        out.append(Case(name, keys, flow))

    add("1x1-fg", np.zeros((1, 1, 1)), 1)
    add("1x1-bg", _blank(1, 1))
    add("1xN", random_mask(1, 2 * TH + 8, 2, 0.6, 2), 2)
    add("Nx1", random_mask(3 * TW + 8, 1, 2, 0.6, 3), 3)
    add("narrow-37x20", random_mask(37, 20, 3, 0.5, 4), 4)
    seed = 10
    for W in (TW - 1, TW, TW + 1, 2 * TW + 1):
        for H in (TH - 1, TH, TH + 1, 2 * TH + 1):
            dens, n = (0.3, 0.5, 0.6)[seed % 3], 1 + seed % 3
            add(f"random-{W}x{H}x{n}-d{dens}", random_mask(W, H, n, dens, seed), seed if seed % 2 else None)
            seed += 1
    W, H = 2 * TW + 1, 2 * TH + 1
    add("all-background", _blank(W, H))
    add("all-foreground", np.zeros((2, H, W)), 30)
    add("corners-and-seam-singles", seam_singles(W, H), 31)
    add("checkerboard", checkerboard(W, H), 32)
    add("diagonals-at-tile-corners", diagonals(W, H))
    add("serpentine-3x3-tiles", serpentine(3 * TW, 3 * TH), 33)
    add("serpentine-flipped", serpentine(3 * TW, 3 * TH)[:, ::-1, ::-1])
    add("comb", comb(W, H), 34)
    add("u-shape", u_shape(W, H))
    add("rings", rings(W, H), 35)
    add("touch-across-seams", seam_touch(W, H), 36)
    add("stripes-of-keys", stripes(W, H), 37)
    add("inter-pair", inter_pair(TW + 1, TH + 1), 38)
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CONNECTIVITIES = (4, 8)
