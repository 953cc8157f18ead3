"""Connected components on the device (blobs.hip): the label map, the table, the key kernel, the refusals, and the way up
through blobs.py, ClipPipeline, FlowStream and the motionGrids command line.

Every output is an integer, so everything is compared with array_equal against the plain Python reference of
tests/blob_cases.py; test_blobs_host.py proves that reference against an independent flood fill and that each case has the
property it is named for."""
import ctypes as C

import numpy as np
import pytest

from tests import blob_cases as BC

pytestmark = pytest.mark.gpu

MAXB = 4096


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _B():
    from opticalflowclustering_amd import blobs
    return blobs


def _dev(a):
    L = _L()
    a = np.ascontiguousarray(a)
    return L.DeviceBuffer(max(a.nbytes, 8)).upload(a)


def label_dev(keys, connectivity, calls=1):
    """ofc_blob_label_dev on a device copy of keys (n,H,W) -> `calls` label maps (n,H,W) int32, into a buffer of 0x55 bytes"""
    L = _L()
    n, H, W = keys.shape
    kd = _dev(keys)
    ld = L.DeviceBuffer(max(keys.size * 4, 8))
    out = []
    try:
        for _ in range(calls):
            L.check(L.load().ofc_memset(0, C.c_void_p(ld.ptr), 0x55, ld.nbytes))
            L.check(L.load().ofc_blob_label_dev(0, C.c_void_p(kd.ptr), W, H, n, connectivity, C.c_void_p(ld.ptr)))
            out.append(ld.download((n, H, W), np.int32))
        assert np.array_equal(kd.download(keys.shape, np.uint8), keys)
    finally:
        kd.free()
        ld.free()
    return out


def table_dev(keys, labels, flow, min_area, max_blobs):
    """ofc_blob_table_dev + ofc_blob_table_read -> (table (n,max_blobs,12), n (n,), found (n,))"""
    L = _L()
    n, H, W = keys.shape
    kd, ld = _dev(keys), _dev(labels)
    fd = None if flow is None else _dev(flow)
    td, cd = L.DeviceBuffer(n * max_blobs * BC.NF * 8), L.DeviceBuffer(max(n * 4, 8))
    table = np.full((n, max_blobs, BC.NF), -7, np.int64)
    cnt, found = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    try:
        L.check(L.load().ofc_blob_table_dev(0, C.c_void_p(kd.ptr), C.c_void_p(ld.ptr), C.c_void_p(fd.ptr) if fd else None, W, H, n,
                                            min_area, max_blobs, C.c_void_p(td.ptr), C.c_void_p(cd.ptr)))
        L.check(L.load().ofc_blob_table_read(0, C.c_void_p(td.ptr), C.c_void_p(cd.ptr), n, max_blobs, L.ptr(table), L.ptr(cnt),
                                             L.ptr(found)))
        assert np.array_equal(ld.download(labels.shape, np.int32), labels)       # the table leaves the label map alone
    finally:
        for b in (kd, ld, fd, td, cd):
            if b is not None:
                b.free()
    return table, cnt, found


def assert_tables(got, want_recs, min_area, max_blobs):
    table, cnt, found = got
    for i, recs in enumerate(want_recs):
        want, nfound = BC.table(recs, min_area, max_blobs)
        assert found[i] == nfound, (i, found[i], nfound)
        assert cnt[i] == len(want)
        assert np.array_equal(table[i, :cnt[i]], want), i
        assert not table[i, cnt[i]:].any()


# ---- the label map ----
@pytest.mark.parametrize("connectivity", BC.CONNECTIVITIES)
@pytest.mark.parametrize("case", BC.CASES, ids=repr)
def test_label_map_equals_the_reference_and_repeats(case, connectivity):
    want, _ = BC.reference(case, connectivity)
    a, b = label_dev(case.keys, connectivity, calls=2)
    assert a.dtype == np.int32 and np.array_equal(a, want)
    assert np.array_equal(b, a)


# ---- the table ----
@pytest.mark.parametrize("connectivity", BC.CONNECTIVITIES)
@pytest.mark.parametrize("case", BC.CASES, ids=repr)
def test_table_equals_the_reference(case, connectivity):
    labels, recs = BC.reference(case, connectivity)
    most = max(max(len(r) for r in recs), 1)
    assert most <= MAXB
    assert_tables(table_dev(case.keys, labels, case.flow, 1, MAXB), recs, 1, MAXB)
    if case.flow is not None:                                                    # without a field the last three are 0
        table, cnt, _ = table_dev(case.keys, labels, None, 1, MAXB)
        for i, r in enumerate(recs):
            want = np.array(r, np.int64).reshape(-1, BC.NF)
            assert np.array_equal(table[i, :cnt[i], :9], want[:, :9]) and not table[i, :, 9:].any()


@pytest.mark.parametrize("name", ["random-65x17x3-d0.6", "rings", "touch-across-seams", "checkerboard", "corners-and-seam-singles"])
def test_min_area_and_max_blobs_at_their_edges(name):
    case = BC.BY_NAME[name]
    labels, recs = BC.reference(case, 4)
    areas = sorted({r[2] for rs in recs for r in rs})
    area = areas[len(areas) // 2]
    for min_area in (area, area + 1, 1):
        assert_tables(table_dev(case.keys, labels, case.flow, min_area, MAXB), recs, min_area, MAXB)
    found = max(BC.table(r, 1)[1] for r in recs)
    assert found >= 2
    assert_tables(table_dev(case.keys, labels, case.flow, 1, found), recs, 1, found)          # all delivered
    got = table_dev(case.keys, labels, case.flow, 1, found - 1)                               # the fullest pair: none
    assert_tables(got, recs, 1, found - 1)
    assert (got[1][[BC.table(r, 1)[1] == found for r in recs]] == 0).all()
    assert np.array_equal(label_dev(case.keys, 4)[0], labels)                                # the label map is complete


# ---- keys ----
def keys_dev(flow, thr=None, k=0, mean=None, centers_c=None, select=0, merge=0, shift=0):
    """ofc_blob_keys_dev; shift = 1 puts the field 8 bytes and the key map 1 byte past their buffers' starts, where the
    kernel cannot take four vectors at a time"""
    L = _L()
    n, H, W = flow.shape[:3]
    flow = np.ascontiguousarray(flow, np.float32)
    fd = L.DeviceBuffer(flow.nbytes + 8).upload(flow, offset=8 * shift)
    kd = L.DeviceBuffer(n * H * W + 8)
    try:
        L.check(L.load().ofc_memset(0, C.c_void_p(kd.ptr), 0x55, kd.nbytes))
        L.check(L.load().ofc_blob_keys_dev(0, C.c_void_p(fd.ptr + 8 * shift), W, H, n, int(thr is not None), float(thr or 0.0), k,
                                           L.ptr(mean), L.ptr(centers_c), select, merge, C.c_void_p(kd.ptr + shift)))
        assert (kd.download((8,), np.uint8, offset=n * H * W) == 0x55)[shift:].all()              # nothing past the map
        return kd.download((n, H, W), np.uint8, offset=shift)
    finally:
        fd.free()
        kd.free()


def moving_weights(flow, thr):
    """ofc_flow_weights_dev kind 1 on the same field -> (n,H,W) f32 of 0 / 1"""
    L = _L()
    fd = _dev(flow)
    wd = L.DeviceBuffer(max(flow.size * 2, 8))
    try:
        L.check(L.load().ofc_flow_weights_dev(0, C.c_void_p(fd.ptr), flow.size // 2, 1, float(thr), C.c_void_p(wd.ptr)))
        return wd.download(flow.shape[:3], np.float32)
    finally:
        fd.free()
        wd.free()


def threshold_field(thr, seed):
    """(2, 9, 67, 2) f32: random vectors, NaN and inf, zeros, and vectors whose u*u + v*v (f32, each operation rounded)
    lies one ulp below, at, and one ulp above thr*thr"""
    r = np.random.default_rng(seed)
    f = (r.standard_normal((2, 9, 67, 2)) * max(thr, 0.25)).astype(np.float32)
    f[0, 0, :4] = [[np.nan, 0], [0, np.inf], [0, 0], [-0.0, 0.0]]
    t2 = np.float32(thr) * np.float32(thr)
    edge = []
    for target in (np.nextafter(t2, np.float32(0)), t2, np.nextafter(t2, np.float32(np.inf))):
        u = np.sqrt(np.float32(target))                                          # (u, 0): u*u rounds near the target
        for cand in (np.nextafter(u, np.float32(0)), u, np.nextafter(u, np.float32(np.inf))):
            edge.append([cand, 0.0])
            edge.append([0.0, -cand])
    f[1, 1, :len(edge)] = np.array(edge, np.float32)
    f[1, 2, 0] = [np.float32(thr), 0.0]
    f[1, 3, :3] = ulp_neighbours(thr)
    return f


def ulp_neighbours(thr):
    """three vectors whose u*u + v*v, as numpy's f32 expression rounds it, is exactly the f32 below thr*thr, thr*thr itself
    and the f32 above it (thr = 0: nothing is below, the first is the zero vector).  Found by search, checked here."""
    one = np.float32(thr)
    t2 = one * one
    if thr == 0:
        tiny = np.float32(2.0 ** -60)                                            # its square, 2^-120, is a normal f32
        return np.array([[0, 0], [0, 0], [tiny, 0]], np.float32)
    out = []
    for target in (np.nextafter(t2, np.float32(0)), t2, np.nextafter(t2, np.float32(np.inf))):
        hit, u = None, one
        for _ in range(4096):                                                    # u from thr downwards, v fills the rest
            rest = np.float32(target) - u * u
            if rest >= 0:
                v0 = np.sqrt(np.float32(rest))
                for v in (np.nextafter(v0, np.float32(0)), v0, np.nextafter(v0, np.float32(np.inf))):
                    if u * u + v * v == target:
                        hit = (u, v)
                        break
            if hit:
                break
            u = np.nextafter(u, np.float32(0))
        assert hit is not None, (thr, target)
        out.append(hit)
    return np.array(out, np.float32)


@pytest.mark.parametrize("thr", [0.0, 0.5, 1.7, 3.0])
def test_threshold_keys_are_the_moving_weights(thr):
    f = threshold_field(thr, 5)
    keys, w = keys_dev(f, thr=thr), moving_weights(f, thr)
    assert np.array_equal(keys_dev(f, thr=thr, shift=1), keys)                   # four vectors per lane or one: equal keys
    assert set(np.unique(keys)) <= {0, 255}
    assert np.array_equal(keys == 0, w == 1.0)
    s = f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]                            # numpy's f32 expression
    with np.errstate(invalid="ignore"):
        assert np.array_equal(keys == 0, s >= np.float32(thr) * np.float32(thr))
    assert s[1, 3, 1] == np.float32(thr) * np.float32(thr) and s[1, 3, 2] > s[1, 3, 1]
    assert list(keys[1, 3, :3]) == [255 if thr > 0 else 0, 0, 0]                 # at thr*thr and above: moving
    if thr > 0:                                                                  # exactly one ulp either side
        assert s[1, 3, 2] == np.nextafter(s[1, 3, 1], np.float32(np.inf))
        assert s[1, 3, 0] == np.nextafter(s[1, 3, 1], np.float32(0))
        assert (keys[1, 1] == 0).any() and (keys[1, 1, :18] == 255).any()        # both sides of the edge are present
    assert keys[0, 0, 0] == 255 and keys[0, 0, 1] == 0                           # NaN fails the comparison; inf passes it


def step_labels(flow, k, mean, cen_c):
    L = _L()
    fd = _dev(flow)
    ld = L.DeviceBuffer(max(flow.size // 2, 8))
    try:
        L.check(L.load().ofc_lloyd_step_dev(0, C.c_void_p(fd.ptr), L.F32, flow.size // 2, 2, k, L.ptr(mean), L.ptr(cen_c),
                                            C.c_void_p(ld.ptr), 0, None))
        return ld.download(flow.shape[:3], np.uint8)
    finally:
        fd.free()
        ld.free()


@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_model_keys_are_the_lloyd_step_bytes_under_select(k):
    r = np.random.default_rng(k)
    f = (r.standard_normal((2, 17, 65, 2)) * 2).astype(np.float32)
    mean = np.array([0.25, -0.5])
    cen_c = np.ascontiguousarray(r.standard_normal((k, 2)) * 2)
    lab = step_labels(f, k, mean, cen_c)
    assert lab.max() < k
    every = (1 << k) - 1
    assert np.array_equal(keys_dev(f, k=k, mean=mean, centers_c=cen_c, select=every), lab)
    odd = every & 0xAAAA | 1
    chosen = ((odd >> lab.astype(np.int64)) & 1).astype(bool)
    assert np.array_equal(keys_dev(f, k=k, mean=mean, centers_c=cen_c, select=odd), np.where(chosen, lab, 255))
    assert np.array_equal(keys_dev(f, k=k, mean=mean, centers_c=cen_c, select=odd, merge=1), np.where(chosen, 0, 255))
    thr = 1.5
    moving = moving_weights(f, thr) == 1.0
    assert np.array_equal(keys_dev(f, thr=thr, k=k, mean=mean, centers_c=cen_c, select=every), np.where(moving, lab, 255))
    assert np.array_equal(keys_dev(f, k=k, mean=None, centers_c=cen_c, select=every), step_labels(f, k, np.zeros(2), cen_c))
    assert np.array_equal(keys_dev(f, thr=thr, k=k, mean=mean, centers_c=cen_c, select=odd, shift=1),
                          np.where(moving & chosen, lab, 255))                   # the one-vector-per-lane form


def test_a_fit_label_buffer_is_a_key_map_without_a_copy():
    """ofc_kmeans_fit_dev leaves u8 labels on the device; ofc_blob_label_dev reads that buffer where it is"""
    L = _L()
    from opticalflowclustering_amd.cluster import kmeans_fit_dev
    W, H, n = BC.TW + 9, BC.TH + 5, 2
    f = np.zeros((n, H, W, 2), np.float32)
    f[:, 3:9, 5:BC.TW + 4] = (2.0, 0.0)                                          # a bar across the column seam
    f[:, 12:BC.TH + 3, 2:6] = (0.0, -2.0)                                        # a bar across the row seam
    fd, kd, ld = _dev(f), L.DeviceBuffer(n * H * W), L.DeviceBuffer(n * H * W * 4)
    try:
        C0 = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, -2.0]])
        kmeans_fit_dev(fd.ptr, L.F32, n * H * W, 2, C0, 10, 1e-4, kd.ptr, 0)
        keys = kd.download((n, H, W), np.uint8)
        assert set(np.unique(keys)) == {0, 1, 2}
        L.check(L.load().ofc_blob_label_dev(0, C.c_void_p(kd.ptr), W, H, n, 8, C.c_void_p(ld.ptr)))
        got = ld.download((n, H, W), np.int32)
    finally:
        for b in (fd, kd, ld):
            b.free()
    assert np.array_equal(got, np.stack([BC.label_one(k, 8) for k in keys]))
    assert len(np.unique(got[0])) == 3                                           # background, and the two bars


# ---- refusals ----
def test_every_refusal_comes_before_any_launch():
    """dimensions beyond the limits with 8-byte buffers: a launch would fault, a refusal returns"""
    L = _L()
    lib = L.load()
    a, b, c, d = (L.DeviceBuffer(64) for _ in range(4))
    pa, pb, pc, pd = (C.c_void_p(x.ptr) for x in (a, b, c, d))
    cen = np.zeros((17, 2))
    host = np.zeros(64, np.int64)
    hp = L.ptr(host)
    try:
        big = (65536, 32768)                                                     # 2^31 pixels
        for W, H, n, conn, rc in ((*big, 1, 8, L.OFC_EUNSUPPORTED), (4, 4, 65536, 8, L.OFC_EUNSUPPORTED),
                                  (0, 4, 1, 8, L.OFC_EINVAL), (4, 0, 1, 8, L.OFC_EINVAL), (4, 4, 0, 8, L.OFC_EINVAL),
                                  (4, 4, 1, 6, L.OFC_EINVAL)):
            assert lib.ofc_blob_label_dev(0, pa, W, H, n, conn, pb) == rc
            if conn == 8:
                assert lib.ofc_blob_keys_dev(0, pa, W, H, n, 1, 0.5, 0, None, None, 0, 0, pb) == rc
                assert lib.ofc_blob_table_dev(0, pa, pb, None, W, H, n, 1, 4, pc, pd) == rc
        assert lib.ofc_blob_table_dev(0, pa, pb, None, 2, 2, 1, 0, 4, pc, pd) == L.OFC_EINVAL
        assert lib.ofc_blob_table_dev(0, pa, pb, None, 2, 2, 1, 1, 0, pc, pd) == L.OFC_EINVAL
        assert lib.ofc_blob_table_dev(0, pa, pb, None, 2, 2, 1, 1, 65537, pc, pd) == L.OFC_EUNSUPPORTED
        assert lib.ofc_blob_table_read(0, pc, pd, 1, 65537, hp, hp, hp) == L.OFC_EUNSUPPORTED
        assert lib.ofc_blob_table_read(0, pc, pd, 0, 4, hp, hp, hp) == L.OFC_EINVAL
        for thr in (-1.0, float("nan"), float("inf")):
            assert lib.ofc_blob_keys_dev(0, pa, 2, 2, 1, 1, thr, 0, None, None, 0, 0, pb) == L.OFC_EINVAL
        assert lib.ofc_blob_keys_dev(0, pa, 2, 2, 1, 0, 0.0, 17, None, L.ptr(cen), 1, 0, pb) == L.OFC_EUNSUPPORTED
        assert lib.ofc_blob_keys_dev(0, pa, 2, 2, 1, 0, 0.0, -1, None, L.ptr(cen), 1, 0, pb) == L.OFC_EUNSUPPORTED
        assert lib.ofc_blob_keys_dev(0, pa, 2, 2, 1, 0, 0.0, 2, None, None, 1, 0, pb) == L.OFC_EINVAL
        bad = np.array([[0.0, np.nan]])
        assert lib.ofc_blob_keys_dev(0, pa, 2, 2, 1, 0, 0.0, 1, None, L.ptr(bad), 1, 0, pb) == L.OFC_EINVAL
        assert lib.ofc_blob_keys_dev(0, C.c_void_p(a.ptr + 4), 2, 2, 1, 1, 0.5, 0, None, None, 0, 0, pb) == L.OFC_EINVAL
        assert lib.ofc_blob_label_dev(0, None, 2, 2, 1, 8, pb) == L.OFC_EINVAL
        assert lib.ofc_blob_label_dev(0, pa, 2, 2, 1, 8, None) == L.OFC_EINVAL
        assert lib.ofc_blobs(0, None, None, 2, 2, 1, 0, 0.0, 0, None, None, 0, 0, 8, 1, 4, None, None, hp, hp, hp) == L.OFC_EINVAL
        assert lib.ofc_blobs(0, hp, None, *big, 1, 0, 0.0, 0, None, None, 0, 0, 8, 1, 4, None, None, hp, hp, hp) == L.OFC_EUNSUPPORTED
        assert lib.ofc_bench_blobs(0, pa, None, *big, 1, 8, 4, 1, C.byref(C.c_float())) == L.OFC_EUNSUPPORTED
        with pytest.raises(ValueError):
            _B().connected_components(np.zeros((4, 4), np.uint8), connectivity=5)
        with pytest.raises(ValueError):
            _B().cluster_blobs(np.zeros((4, 4, 2), np.float32), np.zeros((2, 2)), select=[2])
        with pytest.raises(L.OfcError):
            _B().cluster_blobs(np.zeros((4, 4, 2), np.float32), np.zeros((17, 2)))
    finally:
        for x in (a, b, c, d):
            x.free()


# ---- the Python layer on host arrays ----
@pytest.mark.parametrize("name", ["random-129x33x2-d0.5", "serpentine-3x3-tiles", "stripes-of-keys"])
def test_connected_components_on_host_arrays(name):
    case = BC.BY_NAME[name]
    for conn in BC.CONNECTIVITIES:
        labels, recs = BC.reference(case, conn)
        got = _B().connected_components(case.keys, connectivity=conn, flow=case.flow)
        assert np.array_equal(got.labels, labels)
        for i, r in enumerate(recs):
            assert np.array_equal(got.records[i], np.array(r, np.int64).reshape(-1, BC.NF)) and got.found[i] == len(r)
        if len(recs[0]):
            r0 = np.array(recs[0], np.float64)
            assert np.array_equal(got.centroids(0), r0[:, 7:9] / r0[:, 2:3])
    assert _B().connected_components(case.keys[0], labels=False).labels is None


def pan_with_two_rectangles(W, H):
    """an affine panning background plus two rectangles that move differently against it -> (flow (H,W,2), the boxes)"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    X, Y = xx - (W - 1) / 2, yy - (H - 1) / 2
    f = np.stack([1.5 + 0.004 * X - 0.002 * Y, -0.75 + 0.003 * X + 0.001 * Y], -1)
    boxes = ((10, 5, 10 + 17, 5 + 8), (BC.TW - 6, BC.TH - 3, BC.TW + 12, BC.TH + 9))          # the second spans four tiles
    for (x0, y0, x1, y1), d in zip(boxes, ((3.0, 0.0), (0.0, -4.0))):
        f[y0:y1 + 1, x0:x1 + 1] += d
    return f.astype(np.float32), boxes


def test_compensate_then_moving_blobs_finds_the_two_rectangles():
    from opticalflowclustering_amd import camera
    W, H = 2 * BC.TW + 1, 2 * BC.TH + 1
    f, boxes = pan_with_two_rectangles(W, H)
    res, _ = camera.compensate(f, "affine")
    got = _B().moving_blobs(res, thr=1.0)
    assert got.found[0] == 2 and len(got.records[0]) == 2
    assert np.array_equal(got.boxes(0), np.array(boxes))
    assert np.array_equal(got.records[0][:, 2], [(x1 - x0 + 1) * (y1 - y0 + 1) for x0, y0, x1, y1 in boxes])
    assert np.array_equal(got.keys == 0, got.labels >= 0)
    assert np.abs(got.mean_flow(0) - [[3.0, 0.0], [0.0, -4.0]]).max() < 0.2      # the fit is close to the pan, not equal


def test_cluster_blobs_keeps_touching_motions_apart_and_merge_joins_them():
    W, H = BC.TW + 20, BC.TH + 10
    f = np.zeros((H, W, 2), np.float32)
    f[4:BC.TH + 4, BC.TW - 10:BC.TW] = (2.0, 0.0)                                # two rectangles that share an edge
    f[4:BC.TH + 4, BC.TW:BC.TW + 8] = (0.0, -2.0)                                # ... which lies on the column seam
    cen = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, -2.0]])
    two = _B().cluster_blobs(f, cen, select=[1, 2])
    assert two.found[0] == 2 and np.array_equal(two.records[0][:, 1], [1, 2])
    assert np.array_equal(two.boxes(0), [[BC.TW - 10, 4, BC.TW - 1, BC.TH + 3], [BC.TW, 4, BC.TW + 7, BC.TH + 3]])
    one = _B().cluster_blobs(f, cen, select=[1, 2], merge=True)
    assert one.found[0] == 1 and one.records[0][0, 2] == 18 * BC.TH and one.records[0][0, 1] == 0
    assert _B().cluster_blobs(f, cen, select=[2], thr=1.0).found[0] == 1
    assert _B().cluster_blobs(f, cen).found[0] == 3                              # the still background is a blob too


# ---- ClipPipeline ----
def same_blobs(got, want, labels=True):
    assert np.array_equal(got.found, want.found) and len(got.records) == len(want.records)
    for a, b in zip(got.records, want.records):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    if labels:
        assert np.array_equal(got.labels, want.labels)


def gray_clip(n):
    from tests import motion_grid_cases as MC
    return np.ascontiguousarray(MC.moving_blobs_clip(n)[..., 0])                 # (n, 64, 96): 2 x 4 tiles


def test_pipeline_blobs_equal_the_host_array_route():
    from opticalflowclustering_amd.pipeline import ClipPipeline
    B = _B()
    frames = gray_clip(3)
    H, W = frames.shape[1:]
    assert W > BC.TW and H > BC.TH
    pipe = ClipPipeline(W, H, 3, batch_pairs=2)
    try:
        pipe.upload_frames(frames)
        pipe.run_flow()
        f = pipe.flows_host()
        with pytest.raises(ValueError, match="run_kmeans"):
            pipe.blobs(by="labels")
        thr = 1.0
        s = f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]
        keys = np.where(s >= np.float32(thr) * np.float32(thr), 0, 255).astype(np.uint8)
        got = pipe.blobs(by="moving", thr=thr, min_area=4)
        assert np.array_equal(got.keys, keys) and 2 <= got.found[0] <= 64        # the clip's two discs, and some specks
        same_blobs(got, B.connected_components(keys, min_area=4, flow=f))
        assert np.array_equal(got.labels[0], BC.label_one(keys[0], 8))
        same_blobs(pipe.blobs(by="moving", thr=thr, connectivity=4, labels=False),
                   B.connected_components(keys, connectivity=4, flow=f), labels=False)
        C0 = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, -2.0]])
        centers, _, _ = pipe.run_kmeans(C0)
        lab = pipe.labels_host()
        got = pipe.blobs(by="labels", min_area=9, max_blobs=512)
        same_blobs(got, B.connected_components(lab, min_area=9, max_blobs=512, flow=f))
        assert got.keys is None and got.found.min() >= 2
        mean = pipe._centred_model(centers)[1]
        got = pipe.blobs(by=centers, thr=None, select=[1, 2], min_area=9)
        same_blobs(got, B.cluster_blobs(f, centers, select=[1, 2], mean=mean, min_area=9))
        assert np.array_equal(got.keys, np.where(np.isin(lab, [1, 2]), lab, 255))    # assign's labels are the fit's last E-step
        got = pipe.blobs(by=centers, thr=0.5, merge=True, mean=None)
        same_blobs(got, B.cluster_blobs(f, centers, thr=0.5, merge=True))
        with pytest.raises(ValueError, match="by should be"):
            pipe.blobs(by="colour")
        with pytest.raises(ValueError):
            pipe.blobs(connectivity=6)
    finally:
        pipe.close()


# ---- FlowStream ----
STREAM_THR, STREAM_CENTRES = 1.0, np.array([[0.0, 0.0], [3.0, 0.0], [0.0, -2.0]])


@pytest.fixture(scope="module")
def clip():
    """five frames and their four pairwise fields (the engine's, one pair at a time): read-only"""
    from types import SimpleNamespace
    from opticalflowclustering_amd.flow import FlowEngine
    frames = gray_clip(5)
    eng = FlowEngine(frames.shape[2], frames.shape[1], max_batch=1)
    fields = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    eng.close()
    for a in (frames, fields):
        a.setflags(write=False)
    return SimpleNamespace(frames=frames, fields=fields, W=frames.shape[2], H=frames.shape[1])


def _stream(clip, batch_pairs=2, **kw):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(clip.W, clip.H, batch_pairs=batch_pairs, rows=2, cols=3, **kw)


@pytest.mark.parametrize("n_frames", (5, 4), ids=["two-batches", "a-batch-and-the-flush"])
def test_stream_blobs_equal_the_pairwise_fields(clip, n_frames):
    from opticalflowclustering_amd import camera
    B = _B()
    n = n_frames - 1
    spec = dict(thr=STREAM_THR, connectivity=8, min_area=4, max_blobs=256)
    st = _stream(clip, blobs=spec)
    assert st.blob_args == (8, STREAM_THR, 4, 256)
    for f in clip.frames[:n_frames]:
        st.push(f)
    cells = st.finish()
    got = st.blobs()
    want = B.moving_blobs(clip.fields[:n], STREAM_THR, min_area=4, max_blobs=256)
    assert got.labels is None and len(got) == n and got.found.min() >= 2
    same_blobs(got, want, labels=False)
    same_blobs(st.blobs(), want, labels=False)                                   # still there until frames arrive
    st.set_model(STREAM_CENTRES)                                                 # with a model: keyed by its labels
    for f in clip.frames[:n_frames]:
        st.push(f)
    st.finish_clusters()
    want = B.cluster_blobs(clip.fields[:n], STREAM_CENTRES, thr=STREAM_THR, min_area=4, max_blobs=256)
    same_blobs(st.blobs(), want, labels=False)
    assert {1, 2} <= set(want.records[0][:, 1])
    st.set_model(None)
    st.set_camera("translation", (3.0,))                                         # with a camera: of the residual field
    for f in clip.frames[:n_frames]:
        st.push(f)
    st.finish()
    res, _ = camera.compensate(clip.fields[:n], "translation", (3.0,))
    same_blobs(st.blobs(), B.moving_blobs(res, STREAM_THR, min_area=4, max_blobs=256), labels=False)
    st.close()
    plain = _stream(clip)                                                        # the cell means never depended on the blobs
    for f in clip.frames[:n_frames]:
        plain.push(f)
    assert np.array_equal(plain.finish().view(np.uint32), cells.view(np.uint32))
    plain.close()


def test_stream_set_blobs_preconditions_and_removal(clip):
    L = _L()
    st = _stream(clip)
    with pytest.raises(ValueError, match="no blobs"):
        st.blobs()
    st.set_blobs(thr=2.0, connectivity=4, min_area=2, max_blobs=64)
    st.push(clip.frames[0])
    for conn in (8, None):
        with pytest.raises(ValueError, match="holds frames"):                    # refused while frames are held
            st.set_blobs(connectivity=conn)
    with pytest.raises(ValueError, match="holds frames"):
        st.blobs()
    assert st.blob_args == (4, 2.0, 2, 64)
    for f in clip.frames[1:]:
        st.push(f)
    st.finish()
    want = _B().moving_blobs(clip.fields, 2.0, connectivity=4, min_area=2, max_blobs=64)
    same_blobs(st.blobs(), want, labels=False)
    lib, host = L.load(), np.zeros(4 * 64 * 12, np.int64)
    small = np.full(4, -7, np.int32)
    assert lib.ofc_stream_read_blobs(st._h, L.ptr(host), L.ptr(small), L.ptr(small), 3) == L.OFC_EINVAL and (small == -7).all()
    for conn, thr, min_area, max_blobs, rc in ((6, 1.0, 1, 4, L.OFC_EINVAL), (8, -1.0, 1, 4, L.OFC_EINVAL),
                                               (8, float("nan"), 1, 4, L.OFC_EINVAL), (8, 1.0, 0, 4, L.OFC_EINVAL),
                                               (8, 1.0, 1, 0, L.OFC_EINVAL), (8, 1.0, 1, 65537, L.OFC_EUNSUPPORTED)):
        assert lib.ofc_stream_set_blobs(st._h, conn, thr, min_area, max_blobs) == rc
    assert lib.ofc_stream_set_blobs(None, 8, 1.0, 1, 4) == L.OFC_EINVAL
    assert lib.ofc_stream_read_blobs(None, None, None, None, 0) == L.OFC_EINVAL
    same_blobs(st.blobs(), want, labels=False)                                   # the refusals changed nothing
    st.set_blobs(connectivity=None)
    assert st.blob_args is None
    for f in clip.frames:
        st.push(f)
    st.finish()
    with pytest.raises(ValueError, match="no blobs"):
        st.blobs()
    st.close()


def test_stream_blob_tables_grow_past_their_first_allocation(clip):
    """frames cycling through 4 images, 261 pushes at batch_pairs = 8: the 33rd batch takes the tables past their 256 pairs.
    Pair t is (image t % 4, image (t + 1) % 4), so its table equals that of pair t % 4"""
    from opticalflowclustering_amd.flow import FlowEngine
    images = clip.frames[:4]
    eng = FlowEngine(clip.W, clip.H, max_batch=1)
    fields = np.stack([eng.calc(images[t], images[(t + 1) % 4]) for t in range(4)])
    eng.close()
    want = _B().moving_blobs(fields, STREAM_THR, min_area=4, max_blobs=128, labels=False)
    assert len({r.tobytes() for r in want.records}) == 4                         # the four pairs differ: a misplaced row shows
    st = _stream(clip, batch_pairs=8, blobs=dict(thr=STREAM_THR, min_area=4, max_blobs=128))
    for t in range(261):
        st.push(images[t % 4])
    assert len(st.finish()) == 260
    got = st.blobs()
    assert len(got) == 260
    for t in range(260):
        assert got.found[t] == want.found[t % 4] and np.array_equal(got.records[t], want.records[t % 4]), t
    st.close()


# ---- the command line ----
def test_motion_grids_blobs_on_the_resident_route_and_on_the_stream(tmp_path):
    from opticalflowclustering_amd import camera as cam
    from opticalflowclustering_amd import motionGrids as G
    from opticalflowclustering_amd.flow import FlowEngine
    from tests import motion_grid_cases as MC
    names = ("clip.npy", "fit.csv", "model.npy", "res.csv", "stream.csv", "b_fit.csv", "b_res.csv", "b_stream.csv", "b_plain.csv")
    clip_path, fit_csv, model, res_csv, stream_csv, b_fit, b_res, b_stream, b_plain = (str(tmp_path / n) for n in names)
    frames = MC.moving_blobs_clip()
    frames = np.stack([np.roll(fr, (t, 2 * t), (0, 1)) for t, fr in enumerate(frames)])      # a pan on top of the blobs
    np.save(clip_path, frames)
    from opticalflowclustering_amd.vis import bgr2gray
    gray = np.stack([bgr2gray(f) for f in frames])
    eng = FlowEngine(gray.shape[2], gray.shape[1], max_batch=1)
    fields = np.stack([eng.calc(gray[t], gray[t + 1]) for t in range(len(gray) - 1)])
    eng.close()
    residual, _ = cam.compensate(fields, "affine", (3.0, 1.5))
    blob = ["--blob-thr", "1.0", "--blob-min-area", "9", "--blob-connectivity", "4"]
    base = ["--path", clip_path, "-c", "3", "--rows", "3", "--cols", "4", "--camera", "affine", "--camera-thresholds", "3,1.5"]
    _, centres = G.main(base + blob + ["-f", fit_csv, "--seed", "5", "--save-model", model, "--blobs", b_fit])
    G.main(base + blob + ["-f", res_csv, "--model", model, "--blobs", b_res])
    G.main(base + blob + ["-f", stream_csv, "--model", model, "--stream", "--batch-pairs", "3", "--blobs", b_stream])
    want = _B().cluster_blobs(residual, centres, thr=1.0, connectivity=4, min_area=9)
    text = ",".join(_B().CSV_HEADER) + "\n" + "".join(",".join(str(v) for v in r) + "\n" for r in want.rows())
    assert len(want.rows()) >= 2 * len(fields)
    assert open(b_stream).read() == text and open(b_res).read() == text and open(b_fit).read() == text
    G.main(base[:8] + blob + ["-f", stream_csv, "--model", model, "--stream", "--batch-pairs", "3", "--blobs", b_plain])
    plain = _B().cluster_blobs(fields, centres, thr=1.0, connectivity=4, min_area=9)
    assert open(b_plain).read().splitlines()[1:] == [",".join(str(v) for v in r) for r in plain.rows()] and open(b_plain).read() != text
