"""Links between the blobs of consecutive pairs (include/ofc.h "Blob links", blob_links.hip, blobs.py): a numpy reference of
the definition -- moves from a field, areas by bincount, votes by np.unique over packed pairs -- and the case table that
test_blob_links_host.py (which proves the reference against a per-pixel loop, and that each case has the property it is named
for, on the CPU) and test_gpu_blob_links.py share.  Label maps come from tests/blob_cases.py's reference."""
import collections
import functools
import os
import re

import numpy as np

from tests import blob_cases as BC

with open(os.path.join(BC.ROOT, "include", "ofc.h")) as _f:
    _H = _f.read()
LINK_NF = int(re.search(r"#define\s+OFC_BLOB_LINK_FIELDS\s+(\d+)", _H).group(1))
NO_MOVE = np.array([int(re.search(r"#define\s+OFC_BLOB_NO_MOVE\s+0x([0-9a-fA-F]+)u", _H).group(1), 16)], np.uint32).view(np.int32)[0]
SHARE = 2048                     # consecutive pixels of a pair a work-group of the link kernel takes (csrc/blobs.h BLOB_SHARE)
MAXL = 4096

Case = collections.namedtuple("Case", "name keys flow")
Case.__repr__ = lambda c: c.name


# ---- the reference ----
def moves_of(flow):
    """(..., 2) f32 -> (...) int32: the move words of the definition"""
    f = np.asarray(flow, np.float32)
    u, v = f[..., 0], f[..., 1]
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1024) & (np.abs(v) < 1024)
    dx = np.where(valid, np.rint(np.where(valid, u, 0)), 0).astype(np.int64)      # np.rint of an f32: to nearest, ties to even
    dy = np.where(valid, np.rint(np.where(valid, v, 0)), 0).astype(np.int64)
    word = (((dy & 0xffff) << 16) | (dx & 0xffff)).astype(np.uint32).view(np.int32)
    return np.where(valid, word, NO_MOVE).astype(np.int32)


def unpack(moves):
    """(...) int32 -> dx, dy as int64 (both -32768 for NO_MOVE)"""
    w = np.asarray(moves, np.int32).view(np.uint32).astype(np.int64)
    dx, dy = w & 0xffff, w >> 16
    return dx - ((dx & 0x8000) << 1), dy - ((dy & 0x8000) << 1)


def areas_of(labels):
    """(H,W) int32 label map -> (H*W,) int64: the pixel count at every root, 0 elsewhere"""
    lab = labels.ravel()
    return np.bincount(lab[lab >= 0], minlength=lab.size).astype(np.int64)


def links_one(lab_a, moves_a, lab_b, min_area):
    """one transition -> (m,3) int64 rows root_a, root_b, votes, ascending by (root_a, root_b); every distinct link"""
    H, W = lab_a.shape
    area_a, area_b = areas_of(lab_a), areas_of(lab_b)
    yy, xx = np.mgrid[0:H, 0:W]
    dx, dy = unpack(moves_a)
    a = lab_a.astype(np.int64)
    ok = (a >= 0) & (moves_a != NO_MOVE)
    ok &= area_a[np.where(a >= 0, a, 0)] >= min_area
    xt, yt = xx + dx, yy + dy
    ok &= (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
    b = lab_b.astype(np.int64)[np.where(ok, yt, 0), np.where(ok, xt, 0)]
    ok &= b >= 0
    ok &= area_b[np.where(b >= 0, b, 0)] >= min_area
    packed, votes = np.unique((a[ok] << 32) | b[ok], return_counts=True)
    return np.stack([packed >> 32, packed & 0xffffffff, votes], 1).astype(np.int64).reshape(-1, LINK_NF)


def deliver(rows, max_links):
    """the definition's table of one transition from all its links -> (rows, nlinks): none and -1 past max_links"""
    if len(rows) > max_links:
        return np.zeros((0, LINK_NF), np.int64), -1
    return rows, len(rows)


def links_of(labels, moves, min_area=1, max_links=MAXL):
    """label maps (n,H,W), moves (n,H,W) -> (list of n-1 (m_t,3) arrays, nlinks (n-1,) int32)"""
    out = [deliver(links_one(labels[t], moves[t], labels[t + 1], min_area), max_links) for t in range(len(labels) - 1)]
    return [r for r, _ in out], np.array([m for _, m in out], np.int32).reshape(-1)


@functools.lru_cache(maxsize=None)
def _labels(name, connectivity):
    c = BY_NAME[name]
    lab = np.stack([BC.label_one(k, connectivity) for k in c.keys])
    lab.setflags(write=False)
    return lab


def labels_of(case, connectivity):
    """(n,H,W) int32, read-only: blob_cases' reference label maps of the case's key maps.  Computed once."""
    return _labels(case.name, connectivity)


@functools.lru_cache(maxsize=None)
def _moves(name):
    m = moves_of(BY_NAME[name].flow)
    m.setflags(write=False)
    return m


def case_moves(case):
    return _moves(case.name)


@functools.lru_cache(maxsize=None)
def _all_links(name, connectivity, min_area):
    c = BY_NAME[name]
    lab, mv = labels_of(c, connectivity), case_moves(c)
    return tuple(links_one(lab[t], mv[t], lab[t + 1], min_area) for t in range(len(lab) - 1))


def reference(case, connectivity, min_area=1, max_links=MAXL):
    """-> (links, nlinks) of the case under the reference label maps.  The vote count is computed once per argument set."""
    out = [deliver(r, max_links) for r in _all_links(case.name, connectivity, min_area)]
    return [r for r, _ in out], np.array([m for _, m in out], np.int32).reshape(-1)


# ---- fields ----
SPECIALS = np.concatenate([np.array([[0.5, -0.5], [1.5, -1.5], [2.5, -2.5], [-2.5, 3.5], [0.49999997, -0.50000006]], np.float32),
                           BC.SPECIALS])


def small_moves(shape, seed, reach=3):
    """(n,H,W,2) f32: multiples of 1/4 in [-reach, reach], so that halves (ties) are frequent"""
    r = np.random.default_rng(seed)
    return (r.integers(-4 * reach, 4 * reach + 1, shape + (2,)) / 4.0).astype(np.float32)


def with_specials(keys, flow):
    """SPECIALS on every pair's first foreground pixels, spread out so that they fall inside components"""
    f = flow.copy()
    for i in range(len(keys)):
        ys, xs = np.nonzero(keys[i] != BC.BG)
        step = max(1, len(ys) // (2 * len(SPECIALS)))
        for j, s in enumerate(SPECIALS):
            if j * step < len(ys):
                f[i, ys[j * step], xs[j * step]] = s
    return f


def blocks(W, H, n, seed, size=5):
    """key maps of random size x size blocks of three keys and background"""
    r = np.random.default_rng(seed)
    pick = np.array([0, 15, BC.BG, 254], np.uint8)[r.integers(0, 4, (n, -(-H // size), -(-W // size)))]
    return np.ascontiguousarray(np.repeat(np.repeat(pick, size, 1), size, 2)[:, :H, :W])


EDGE_MOVES = {"left": (-1, 0), "right": (1, 0), "top": (0, -1), "bottom": (0, 1), "top-left": (-1, -1), "top-right": (1, -1),
              "bottom-left": (-1, 1), "bottom-right": (1, 1)}


def edge_pixels(W, H):
    """name -> (x, y) of a pixel on that edge or corner"""
    return {"left": (0, H // 2), "right": (W - 1, H // 3), "top": (W // 2, 0), "bottom": (W // 3, H - 1), "top-left": (0, 0),
            "top-right": (W - 1, 0), "bottom-left": (0, H - 1), "bottom-right": (W - 1, H - 1)}


def frame_edges(W, H):
    """all foreground, two keys in vertical halves, three pairs; still but for: the pixel at every edge and corner leaves
    the frame by exactly one pixel (pair 0) and the pixel one step inside lands exactly on the border (pair 0 too); pair 1
    does the same with moves of 1023 px and of the exact distance to the far border"""
    keys = np.zeros((3, H, W), np.uint8)
    keys[:, :, W // 2:] = 15
    f = np.zeros((3, H, W, 2), np.float32)
    for name, (x, y) in edge_pixels(W, H).items():
        dx, dy = EDGE_MOVES[name]
        f[0, y, x] = (dx, dy)                                  # out by one
        f[0, y - dy, x - dx] = (dx, dy)                        # from one step inside onto the border: in by zero
        f[1, y, x] = (1023 * dx, 1023 * dy)
        f[1, y - dy, x - dx] = (-dx * (W - 2) if dx else 0, -dy * (H - 2) if dy else 0)          # onto the far border
    return keys, f


def merge_and_split(W, H):
    """pair 0: two rectangles that move towards each other and land on one rectangle of pair 1, whose halves move apart and
    land on two rectangles of pair 2"""
    keys = BC._blank(W, H, 3)
    f = np.zeros((3, H, W, 2), np.float32)
    keys[0, 10:30, 20:50] = 0
    keys[0, 10:30, 110:140] = 0
    f[0, 10:30, 20:50] = (30.0, 0.0)
    f[0, 10:30, 110:140] = (-30.0, 0.0)
    keys[1, 10:30, 50:110] = 0                                 # both land here
    f[1, 10:30, 50:80] = (-35.0, 4.0)
    f[1, 10:30, 80:110] = (35.0, -4.0)
    keys[2, 14:34, 15:45] = 0
    keys[2, 6:26, 115:145] = 0
    return keys, f


def min_area_blobs(W, H):
    """pair 0: squares of area 9, 16 and 4, all moving by (3, 2); pair 1: where they land, rectangles of area 25, 6 and 4
    (still); pair 2 repeats pair 1"""
    keys = BC._blank(W, H, 3)
    f = np.zeros((3, H, W, 2), np.float32)
    f[0] = (3.0, 2.0)
    keys[0, 5:8, 5:8] = 0
    keys[0, 5:9, 20:24] = 0
    keys[0, 5:7, 40:42] = 0
    keys[1:, 6:11, 7:12] = 0                                   # 25: covers the 9 that lands on (8..10, 7..9)
    keys[1:, 8:10, 23:26] = 0                                  # 6: inside the 16 that lands on (23..26, 7..10)
    keys[1:, 7:9, 43:45] = 0                                   # 4: exactly the 4
    return keys, f


def shifted_then_unlike(W, H, seed):
    """pair 1 is pair 0 shifted by (3, 1), and pair 0's field says so; pair 2 is unlike both, and the fields of pairs 1 and
    2 are random"""
    keys = blocks(W, H, 3, seed, size=4)
    keys[1] = BC.BG
    keys[1, 1:, 3:] = keys[0, :-1, :-3]
    f = small_moves((3, H, W), seed + 1)
    f[0] = (3.0, 1.0)
    return keys, f


def _cases():
    out = []

    def add(name, keys, flow):
        keys = np.ascontiguousarray(keys, np.uint8)
        flow = np.ascontiguousarray(flow, np.float32)
        assert flow.shape == keys.shape + (2,)
        keys.setflags(write=False)
        flow.setflags(write=False)
        out.append(Case(name, keys, flow))

    k = blocks(BC.TW, BC.TH, 3, 1)
    add("specials-64x16", k, with_specials(k, small_moves(k.shape, 2)))
    add("frame-edges-70x33", *frame_edges(70, 33))
    k = BC.random_mask(129, 40, 3, 0.5, 3, keys=(0,))
    add("background-129x40", k, small_moves(k.shape, 4))
    add("merge-and-split-200x50", *merge_and_split(200, 50))
    board = np.repeat(BC.checkerboard(129, 40), 3, 0)
    add("many-links-129x40", board, np.broadcast_to(np.array([2.0, 0.0], np.float32), board.shape + (2,)))
    add("min-area-70x33", *min_area_blobs(70, 33))
    add("pair-isolation-64x16", *shifted_then_unlike(BC.TW, BC.TH, 5))
    k = blocks(BC.TW, BC.TH, 1, 7)
    add("single-pair-64x16", k, small_moves(k.shape, 8))
    k = BC.random_mask(1, 300, 3, 0.7, 9, keys=(0, 15))
    add("1xN", k, with_specials(k, small_moves(k.shape, 10, reach=2)))
    k = BC.random_mask(300, 1, 3, 0.7, 11, keys=(0, 15))
    add("Nx1", k, with_specials(k, small_moves(k.shape, 12, reach=2)))
    k = blocks(200, 50, 3, 13, size=7)
    add("blocks-200x50", k, with_specials(k, small_moves(k.shape, 14, reach=6)))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CONNECTIVITIES = BC.CONNECTIVITIES


# ---- a clip whose tracks are known: two textured rectangles, 3 px per frame each, over a textured background ----
CLIP_W, CLIP_H, CLIP_FRAMES, CLIP_THR, CLIP_MIN_AREA = 128, 80, 6, 1.5, 60
CLIP_RECTS = ((14, 12, 30, 20, 3, 0), (88, 52, 24, 22, 0, -3))         # x, y, w, h in frame 0 of the world; vx, vy per frame
CLIP_PAN = (2, 1)                                                      # the panning camera's step per frame, px


def rect_clip(pan=(0, 0), n_frames=CLIP_FRAMES, W=CLIP_W, H=CLIP_H):
    """(n, H, W) u8.  The camera looks at a larger textured world through a window that moves by `pan` per frame, so the
    background's image moves by -pan and nothing wraps around; each rectangle carries its own texture with it."""
    rng = np.random.default_rng(21)
    M = 32                                                             # margin of the world around the first window
    yy, xx = np.mgrid[0:H + 2 * M, 0:W + 2 * M].astype(np.float64)
    world = 118 + 45 * np.sin(xx * 0.23 + 0.4) * np.cos(yy * 0.19) + 25 * np.sin(xx * 0.07 - yy * 0.11) + rng.integers(-5, 6, xx.shape)
    tex = 128 + 90 * np.sin(xx * 0.8 + yy * 0.5) * np.cos(xx * 0.35 - yy * 0.7)
    clip = np.empty((n_frames, H, W), np.uint8)
    for t in range(n_frames):
        img = world.copy()
        for x, y, w, h, vx, vy in CLIP_RECTS:
            x0, y0 = M + x + vx * t, M + y + vy * t
            img[y0:y0 + h, x0:x0 + w] = tex[M + y:M + y + h, M + x:M + x + w]
        ox, oy = M + pan[0] * t, M + pan[1] * t
        clip[t] = np.clip(img[oy:oy + H, ox:ox + W], 0, 255).astype(np.uint8)
    return clip
