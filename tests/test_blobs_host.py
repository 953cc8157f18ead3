"""Connected components without a GPU: the exports, the host-only check, the proof that the reference of
tests/blob_cases.py is the definition (an independent flood fill) and that every case has the property it is named for, and
the Python and command-line fronts."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libofc.so is loaded, as in bench.py: this file sorts first in the suite, and a process
#               that loads libofc first and torch later holds two HIP runtimes, on which the RCCL tests then fail)

from tests import blob_cases as BC

EXPORTS = ("ofc_blob_check", "ofc_blob_keys_dev", "ofc_blob_label_dev", "ofc_blob_table_dev", "ofc_blob_table_read", "ofc_blobs",
           "ofc_stream_set_blobs", "ofc_stream_read_blobs", "ofc_bench_blobs")


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _B():
    from opticalflowclustering_amd import blobs
    return blobs


def test_the_new_exports_exist_and_the_constants_agree():
    L = _L()
    lib = C.CDLL(L.LIB_PATH)
    missing = [n for n in EXPORTS if not hasattr(lib, n)]
    assert not missing, missing
    assert set(EXPORTS) <= set(L.EXPORTS)
    header = open(L.LIB_PATH.replace("opticalflowclustering_amd/libofc.so", "include/ofc.h")).read()
    assert all(f"int {n}(" in header for n in EXPORTS)
    assert (L.BLOB_TILE_W, L.BLOB_TILE_H, L.BLOB_FIELDS) == (BC.TW, BC.TH, BC.NF)
    assert _B().FIELDS == BC.FIELDS and len(BC.FIELDS) == BC.NF and _B().BACKGROUND == BC.BG


# ---- the reference is the definition ----
def flood_fill(keys, connectivity):
    """(H,W) u8 -> (H,W) int32: breadth-first from every unvisited foreground pixel in raster order, which is therefore
    its component's smallest index.  Shares nothing with blob_cases.label_one."""
    H, W = keys.shape
    out = np.full((H, W), -1, np.int32)
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    for y0 in range(H):
        for x0 in range(W):
            if keys[y0, x0] == BC.BG or out[y0, x0] >= 0:
                continue
            root, key = y0 * W + x0, keys[y0, x0]
            out[y0, x0] = root
            queue = collections.deque([(y0, x0)])
            while queue:
                y, x = queue.popleft()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and out[yy, xx] < 0 and keys[yy, xx] == key:
                        out[yy, xx] = root
                        queue.append((yy, xx))
    return out


@pytest.mark.parametrize("connectivity", BC.CONNECTIVITIES)
@pytest.mark.parametrize("case", BC.CASES, ids=repr)
def test_reference_equals_an_independent_flood_fill(case, connectivity):
    labels, recs = BC.reference(case, connectivity)
    assert labels.dtype == np.int32 and labels.shape == case.keys.shape
    for i, keys in enumerate(case.keys):
        want = flood_fill(keys, connectivity)
        assert np.array_equal(labels[i], want)
        roots, areas = np.unique(want[want >= 0], return_counts=True)
        assert [r[0] for r in recs[i]] == list(roots) and [r[2] for r in recs[i]] == list(areas)
        for r in recs[i]:
            ys, xs = np.nonzero(want == r[0])
            assert r[1] == keys.ravel()[r[0]] and r[3:9] == [xs.min(), ys.min(), xs.max(), ys.max(), xs.sum(), ys.sum()]


def count(name, connectivity, pair=0):
    return len(BC.reference(BC.BY_NAME[name], connectivity)[1][pair])


def test_the_case_table_covers_the_sizes_the_seams_need():
    shapes = {c.keys.shape[1:] for c in BC.CASES}
    for W in (BC.TW - 1, BC.TW, BC.TW + 1, 2 * BC.TW + 1):
        for H in (BC.TH - 1, BC.TH, BC.TH + 1, 2 * BC.TH + 1):
            assert (H, W) in shapes
    assert (1, 1) in shapes and any(w == 1 and h > BC.TH for h, w in shapes) and any(h == 1 and w > BC.TW for h, w in shapes)
    assert any(w < 64 and h > 1 for h, w in shapes)
    assert {len(c.keys) for c in BC.CASES} >= {1, 2, 3}
    assert {0, 15, 254} <= set(np.unique(np.concatenate([c.keys.ravel() for c in BC.CASES])))
    dens = [float((c.keys != BC.BG).mean()) for c in BC.CASES if c.name.startswith("random")]
    assert min(dens) < 0.35 and max(dens) > 0.55


def test_each_case_has_the_property_it_is_named_for():
    board = BC.BY_NAME["checkerboard"].keys[0]
    assert count("checkerboard", 4) == int((board != BC.BG).sum()) > 1000 and count("checkerboard", 8) == 1
    assert count("all-background", 8) == 0 and count("all-foreground", 4) == 1 and count("all-foreground", 4, pair=1) == 1
    assert count("corners-and-seam-singles", 4) == 10 and count("corners-and-seam-singles", 8) == 9
    assert count("diagonals-at-tile-corners", 8) == 2 and count("diagonals-at-tile-corners", 4) == 12
    for name in ("serpentine-3x3-tiles", "serpentine-flipped"):
        k = BC.BY_NAME[name].keys[0]
        assert k.shape == (3 * BC.TH, 3 * BC.TW) and count(name, 4) == 1 and count(name, 8) == 1
        fg = k != BC.BG
        for ty in range(3):                                                     # it passes through every tile
            for tx in range(3):
                assert fg[ty * BC.TH:(ty + 1) * BC.TH, tx * BC.TW:(tx + 1) * BC.TW].any()
        crossings = int((fg[:, BC.TW - 1] & fg[:, BC.TW]).sum() + (fg[:, 2 * BC.TW - 1] & fg[:, 2 * BC.TW]).sum()
                        + (fg[BC.TH - 1] & fg[BC.TH]).sum() + (fg[2 * BC.TH - 1] & fg[2 * BC.TH]).sum())
        assert crossings >= 8
        rec = BC.reference(BC.BY_NAME[name], 4)[1][0][0]
        last = int(np.flatnonzero(fg.ravel())[-1])
        assert rec[0] == int(np.flatnonzero(fg.ravel())[0]) and last - rec[0] > 2 * BC.TH * 3 * BC.TW      # the root is far from the end
    for name in ("comb", "u-shape"):
        k = BC.BY_NAME[name].keys[0]
        assert count(name, 4) == 1 and count(name, 8) == 1
        assert len(np.unique(BC.label_one(k[:-1], 8))) - 1 >= 2                  # only the last row joins the arms
        assert BC.reference(BC.BY_NAME[name], 4)[1][0][0][0] < k.shape[1]        # and the root is in the first row
    assert count("rings", 4) == count("rings", 8) == 13
    assert count("touch-across-seams", 4) == 4 and count("touch-across-seams", 8) == 3
    assert count("inter-pair", 8) == 1 and count("inter-pair", 8, pair=1) == 1
    pair = BC.BY_NAME["inter-pair"].keys
    assert (pair[0, -1] != BC.BG).all() and (pair[1, 0] != BC.BG).all()          # one component if pairs were stacked
    assert len(np.unique(BC.label_one(pair.reshape(-1, pair.shape[2]), 4))) - 1 == 1
    stripes = BC.reference(BC.BY_NAME["stripes-of-keys"], 4)[1][0]
    assert {r[1] for r in stripes} == {0, 15, 254} and max(r[2] for r in stripes if r[1] == 15) > 5 * (2 * BC.TH + 1)


def test_the_fields_exercise_every_rule_of_the_sums():
    S = BC.SPECIALS
    assert np.signbit(S[0, 0]) and S[0, 0] == 0 and np.isnan(S[1, 0]) and np.isposinf(S[2, 1]) and np.isneginf(S[3, 0])
    assert S[4, 0] == np.float32(1023.99) and S[5, 0] == 1024 and S[6, 1] == -1024
    assert [BC.quantise(v) for v in S[7]] == [0, -2] and [BC.quantise(v) for v in S[8]] == [-2, 2]      # ties go to even
    assert [BC.quantise(v) for v in S[9]] == [2, -4]
    case = BC.BY_NAME["all-foreground"]
    rec = BC.reference(case, 8)[1][0][0]
    f = case.flow[0].reshape(-1, 2)
    valid = np.isfinite(f).all(1) & (np.abs(f) < 1024).all(1)
    assert rec[2] == len(f) and rec[9] == valid.sum() == len(f) - 5              # NaN, inf, -inf, 1024 and -1024 are left out
    assert rec[10] == sum(BC.quantise(u) for u in f[valid, 0])
    assert (case.flow[0, 0::2] != np.rint(case.flow[0, 0::2])).mean() > 0.9      # fractional rows
    assert (case.flow[0, 1::2] == np.rint(case.flow[0, 1::2])).mean() > 0.99     # integer-valued rows (but for the specials)


# ---- the host-only check ----
def test_blob_check_accepts_and_refuses_exactly_the_domain():
    L = _L()
    check = L.load().ofc_blob_check
    ok = (64, 48, 1, 8, 1, 4096)
    assert check(*ok) == L.OFC_OK

    def with_(**kw):
        names = ("W", "H", "npair", "connectivity", "min_area", "max_blobs")
        return check(*[kw.get(n, v) for n, v in zip(names, ok)])

    assert with_(W=1, H=1) == L.OFC_OK and with_(W=0) == L.OFC_EINVAL and with_(H=0) == L.OFC_EINVAL and with_(W=-3) == L.OFC_EINVAL
    assert with_(W=2 ** 31 - 1, H=1) == L.OFC_OK and with_(W=1, H=2 ** 31 - 1) == L.OFC_OK          # W*H = 2^31 - 1
    assert with_(W=46341, H=46340) == L.OFC_OK                                                       # 2147441940
    assert with_(W=65536, H=32768) == L.OFC_EUNSUPPORTED and "2^31" in L.load().ofc_last_error().decode()      # 2^31
    assert with_(W=46341, H=46341) == L.OFC_EUNSUPPORTED
    assert with_(npair=1) == L.OFC_OK and with_(npair=65535) == L.OFC_OK
    assert with_(npair=0) == L.OFC_EINVAL and with_(npair=65536) == L.OFC_EUNSUPPORTED
    for conn, rc in ((4, L.OFC_OK), (8, L.OFC_OK), (0, L.OFC_EINVAL), (6, L.OFC_EINVAL), (16, L.OFC_EINVAL), (-8, L.OFC_EINVAL)):
        assert with_(connectivity=conn) == rc
    assert with_(min_area=1) == L.OFC_OK and with_(min_area=2 ** 31 - 1) == L.OFC_OK and with_(min_area=0) == L.OFC_EINVAL
    assert with_(max_blobs=1) == L.OFC_OK and with_(max_blobs=65536) == L.OFC_OK
    assert with_(max_blobs=0) == L.OFC_EINVAL and with_(max_blobs=65537) == L.OFC_EUNSUPPORTED
    B = _B()
    B.check_args(64, 48, 3)
    with pytest.raises(ValueError, match="connectivity"):
        B.check_args(64, 48, 3, connectivity=5)
    with pytest.raises(L.OfcError):
        B.check_args(65536, 32768, 1)


# ---- the Python layer ----
def test_order_records_sorts_by_root_and_applies_the_overflow_rule():
    B = _B()
    recs = BC.reference(BC.BY_NAME["rings"], 4)[1][0]
    want = np.array(recs, np.int64)
    r = np.random.default_rng(0)
    slots = want[r.permutation(len(want))]                                       # the device's order is unspecified
    padded = np.concatenate([slots, np.full((3, BC.NF), -9, np.int64)])          # slots past `found` are not read
    for given in (slots, padded, padded.ravel()):
        out = B.order_records(given, len(want), len(want))
        assert out.dtype == np.int64 and np.array_equal(out, want)
    assert np.array_equal(B.order_records(padded, len(want), 4096), want)
    over = B.order_records(padded, len(want), len(want) - 1)                     # found > max_blobs: none delivered
    assert over.shape == (0, BC.NF)
    assert B.order_records(np.zeros((0, BC.NF)), 0, 1).shape == (0, BC.NF)
    got, found = BC.table(recs, 1, len(want) - 1)
    assert len(got) == 0 and found == len(want)                                  # the reference's rule is the same


def test_select_mask_and_blob_views_and_rows():
    B = _B()
    assert B.select_mask(None, 3) == 0b111 and B.select_mask([0, 2], 3) == 0b101 and B.select_mask([], 3) == 0
    assert B.select_mask(None, 16) == 0xFFFF
    for bad in ([3], [-1]):
        with pytest.raises(ValueError, match="select"):
            B.select_mask(bad, 3)
    W = 100
    rec = np.array([[205, 1, 4, 5, 2, 6, 3, 22, 10, 4, int(1.5 * 65536 * 4), int(-0.25 * 65536 * 4)],
                    [730, 0, 2, 30, 7, 31, 7, 61, 14, 0, 0, 0]], np.int64)
    b = B.Blobs(W, 50, None, [rec, np.zeros((0, BC.NF), np.int64)], np.array([2, 0], np.int32))
    assert len(b) == 2 and np.array_equal(b.boxes(0), [[5, 2, 6, 3], [30, 7, 31, 7]])
    assert b.centroids(0).dtype == np.float64 and np.array_equal(b.centroids(0), [[5.5, 2.5], [30.5, 7.0]])
    mf = b.mean_flow(0)
    assert np.array_equal(mf[0], [1.5, -0.25]) and np.isnan(mf[1]).all()        # no valid vector: no mean
    assert b.boxes(1).shape == (0, 4) and b.centroids(1).shape == (0, 2) and b.mean_flow(1).shape == (0, 2)
    assert b.rows() == [(0, 1, 5, 2, 4, 5, 2, 6, 3, "5.500", "2.500", "1.5000", "-0.2500"),
                        (0, 0, 30, 7, 2, 30, 7, 31, 7, "30.500", "7.000", "nan", "nan")]
    assert len(B.CSV_HEADER) == len(b.rows()[0]) == 13
    assert B.CSV_HEADER[:5] == ("pair", "key", "root_x", "root_y", "area") and B.CSV_HEADER[-2:] == ("mean_u", "mean_v")


def test_blob_csv_format(tmp_path):
    from opticalflowclustering_amd import motionGrids as G
    B = _B()
    rec = np.array([[3, 2, 1, 3, 0, 3, 0, 3, 0, 1, 65536, -32768]], np.int64)
    path = str(tmp_path / "sub" / "blobs.csv")
    G.write_blob_csv(path, B.Blobs(8, 8, None, [np.zeros((0, BC.NF), np.int64), rec], np.array([0, 1], np.int32)))
    assert open(path).read() == ("pair,key,root_x,root_y,area,xmin,ymin,xmax,ymax,cx,cy,mean_u,mean_v\n"
                                 "1,2,3,0,1,3,0,3,0,3.000,0.000,1.0000,-0.5000\n")


def test_motion_grids_blob_arguments():
    from opticalflowclustering_amd import motionGrids as G
    base = ["--path", "clip.npy", "-c", "3", "-f", "out.csv"]
    a = G.parse_arguments(base)                                                  # as before: no blobs, everything else untouched
    assert a.blobs is None and a.blob_spec is None and a.camera_spec is None and not a.stream and a.rows == 14 and a.cols == 25
    a = G.parse_arguments(base + ["--model", "m.npy", "--stream", "--camera", "affine"])
    assert a.blob_spec is None and a.stream and a.camera_spec == ("affine", (4.0, 2.0, 1.0))
    a = G.parse_arguments(base + ["--blobs", "b.csv"])
    assert a.blobs == "b.csv" and a.blob_spec == dict(thr=0.5, connectivity=8, min_area=1, max_blobs=G.MAX_BLOBS)
    a = G.parse_arguments(base + ["--blobs", "b.csv", "--blob-thr", "1.25", "--blob-min-area", "16", "--blob-connectivity", "4",
                                  "--model", "m.npy", "--stream", "--camera", "translation"])
    assert a.blob_spec == dict(thr=1.25, connectivity=4, min_area=16, max_blobs=G.MAX_BLOBS) and a.stream
    assert G.parse_arguments(base + ["--blob-thr", "2"]).blob_spec is None       # the options alone switch nothing on
    for bad in (["--blob-connectivity", "6"], ["--blob-min-area", "0"], ["--blob-thr", "-1"], ["--blob-thr", "nan"],
                ["--blob-thr", "x"], ["--blobs"]):
        with pytest.raises(SystemExit):
            G.parse_arguments(base + bad)
