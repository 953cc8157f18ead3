"""The tile -> sample map of the Lloyd field sweeps (csrc/lloyd_field.h), through the library's host exports
ofc_lloyd_field_origin / ofc_lloyd_field_origins / ofc_lloyd_field_shape: no device is touched.  The kernels use the same
header functions, so what holds here holds for k_tile_probe_field, k_tile_meta_field, the walk and the label stores."""
import numpy as np
import pytest

import lloyd_field_tile_cases as F
from opticalflowclustering_amd import _lib

SIZES = [(64, 8), (128, 16), (1920, 1080), (3840, 2160)]


def shape():
    import ctypes as C
    v = [C.c_int() for _ in range(4)]
    _lib.load().ofc_lloyd_field_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def origins(W, n_tiles, tile0=0):
    out = np.empty((n_tiles, 16), np.int64)
    _lib.check(_lib.load().ofc_lloyd_field_origins(tile0, n_tiles, W, _lib.ptr(out)))
    return out


def test_shape_is_a_64_sample_tile_under_a_64x8_group():
    tw, th, gw, gh = shape()
    assert tw * th == 64 and (gw, gh) == (F.GROUP_W, F.GROUP_H) and gw % tw == 0 and gh % th == 0 and tw % 4 == 0
    assert (gw // tw) * (gh // th) == 8


@pytest.mark.parametrize("W,H", SIZES)
def test_tiles_partition_the_samples_exactly_once(W, H):
    n = 2 if W * H <= 1920 * 1080 else 1
    N = n * W * H
    q = origins(W, N // 64)
    idx = (q[:, :, None] + np.arange(4)).ravel()
    assert idx.min() == 0 and idx.max() == N - 1
    assert (np.bincount(idx, minlength=N) == 1).all()
    # a quad is 4 consecutive pixels of one image row, inside one field
    x0 = q % W
    assert (x0 % 4 == 0).all() and (x0 + 3 < W).all()


@pytest.mark.parametrize("W,H", SIZES)
def test_a_groups_tiles_are_contiguous_records_and_cover_its_64x8_pixels(W, H):
    tw, th, gw, gh = shape()
    n = 2 if W * H <= 1920 * 1080 else 1
    NG = n * W * H // 512
    q = origins(W, NG * 8).reshape(NG, 8, 16)             # records g*8 .. g*8+7 are group g's tiles
    y, x = q // W, q % W                                   # rows of the stack of fields (n * H of them)
    gy, gx = y[:, 0, 0], x[:, 0, 0]                        # tile 0, quad 0: the group's top left pixel
    assert (gy % gh == 0).all() and (gx % gw == 0).all()
    assert ((y - gy[:, None, None] >= 0) & (y - gy[:, None, None] < gh)).all()
    assert ((x - gx[:, None, None] >= 0) & (x - gx[:, None, None] + 3 < gw)).all()
    # groups run over (field, band, column) in that order: raster order of their top left pixels, each met once
    assert np.array_equal(gy * (W // gw) // gh + gx // gw, np.arange(NG))
    # tile ti of a group sits at (ti // across) * th rows, (ti % across) * tw pixels; quad r at (r // qpr, 4 (r % qpr))
    across, qpr = gw // tw, tw // 4
    ti, r = np.arange(8)[None, :, None], np.arange(16)[None, None, :]
    assert np.array_equal(y - gy[:, None, None], (ti // across) * th + r // qpr + 0 * y)
    assert np.array_equal(x - gx[:, None, None], (ti % across) * tw + (r % qpr) * 4 + 0 * x)
    # a band never straddles two fields
    assert ((gy // H) == ((gy + gh - 1) // H)).all()


@pytest.mark.parametrize("W,H", SIZES[:3])
def test_numpy_mirror_of_the_test_helpers_is_the_librarys_map(W, H):
    tw, th, _, _ = shape()
    n = 2
    assert np.array_equal(F.quad_origins(W, H, n, tile_w=tw, tile_h=th), origins(W, n * W * H // 64))


def test_single_origin_export_and_its_refusals():
    lib = _lib.load()
    q = origins(128, 24)
    for t, r in [(0, 0), (3, 15), (8, 0), (23, 7)]:
        assert lib.ofc_lloyd_field_origin(t, r, 128) == q[t, r]
    for t, r, W in [(-1, 0, 128), (0, 16, 128), (0, -1, 128), (0, 0, 96), (0, 0, 0)]:
        assert lib.ofc_lloyd_field_origin(t, r, W) == -1
    assert lib.ofc_lloyd_field_origins(0, 1, 96, _lib.ptr(np.empty(16, np.int64))) == _lib.OFC_EINVAL
    assert lib.ofc_lloyd_field_origins(0, 1, 128, None) == _lib.OFC_EINVAL
