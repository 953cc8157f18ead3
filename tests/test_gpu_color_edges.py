"""The colour, grid and cosine kernels (csrc/color_kernels.hip, the grid path of csrc/lloyd_batched.hip, csrc/color_api.cpp)
at their edges, through the C ABI: every 8-bit colour, scalar tails, thresholds, octants and hue wrap, several resident
frames per call, grids that do not divide the frame, the LDS limit of the batched fit, long and large-valued cosine
windows.  "bit-exact" = np.array_equal against the oracle (oracle/color_ref.c, itself bounded against the plain
definitions in test_oracle_color_independent.py); these kernels are built with FP contraction off so that this holds."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1), (1, 7), (5, 1), (9, 16), (14, 25), (54, 96)]


@pytest.fixture(scope="module")
def vis():
    from opticalflowclustering_amd import vis
    return vis


@pytest.fixture(scope="module")
def L():
    from opticalflowclustering_amd import _lib
    _lib.load()
    return _lib


def all_colours():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([a & 255, (a >> 8) & 255, a >> 16], 1).astype(np.uint8)


def direction_sweep(kind):
    """as in test_oracle_color_independent.py: 100 003 directions, the eight axis/diagonal directions exactly, +-0.0
    components; magnitudes 0.01 .. 20 ('lin') or 1e-15 .. 1e15 ('log', squares finite and normal in f32)"""
    n = 100_003
    th = 2 * np.pi * np.arange(n) / n
    d = np.stack([np.cos(th), np.sin(th)], 1)
    z = 0.0
    exact = np.array([(1, z), (1, 1), (z, 1), (-1, 1), (-1, z), (-1, -1), (z, -1), (1, -1),
                      (1, -z), (-1, -z), (-z, 1), (-z, -1)], np.float64)
    d = np.concatenate([d, exact, exact, exact])
    ladder = np.linspace(0.01, 20, 257) if kind == "lin" else np.logspace(-15, 15, 61)
    m = ladder[(np.arange(len(d)) * 7) % len(ladder)]
    return (d * m[:, None]).astype(np.float32)


# ---------------------------------------------------------------- ofc_bgr2hsv / ofc_bgr2gray / ofc_preprocess_rgba
def test_bgr2hsv_every_colour(vis):
    """ofc_bgr2hsv, all 2^24 colours in one call: the reciprocal tables, the v==r / v==g tie order, the negative-hue wrap"""
    bgr = all_colours()
    assert np.array_equal(vis.bgr2hsv(bgr), O.bgr2hsv(bgr))


@pytest.mark.parametrize("npix", [1, 255, 256, 257, 65537])
def test_bgr2hsv_block_edges(vis, npix):
    bgr = np.random.default_rng(npix).integers(0, 256, (npix, 3), dtype=np.uint8)
    assert np.array_equal(vis.bgr2hsv(bgr), O.bgr2hsv(bgr))


def test_bgr2gray_every_colour(vis):
    """ofc_bgr2gray, all 2^24 colours as a 4096x4096 frame (the packed 4-pixel path, every byte lane)"""
    bgr = all_colours().reshape(4096, 4096, 3)
    assert np.array_equal(vis.bgr2gray(bgr), O.bgr2gray(bgr))


@pytest.mark.parametrize("W,H", [(1, 1), (2, 1), (3, 1), (5, 1), (1, 7), (1021, 1), (7, 3)])
def test_bgr2gray_scalar_tail(vis, W, H):
    """W*H not a multiple of 4, or below 4: the last lane's scalar loop, and nothing written past the frame"""
    bgr = np.random.default_rng(W * H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    assert np.array_equal(vis.bgr2gray(bgr), O.bgr2gray(bgr))


@pytest.mark.parametrize("thresh", [0, 1, 30, 31, 255, 256])
@pytest.mark.parametrize("npix", [1, 257, 51 * 51, 153 * 154])
def test_preprocess_rgba_thresholds(vis, thresh, npix):
    """ofc_preprocess_rgba: `< thresh`, not `<=`; alpha from the thresholded triple (a pixel like (t-1, t-1, t-1) has a raw
    grey value above 0 and alpha 0); every byte value next to the threshold in every channel"""
    rng = np.random.default_rng(thresh * 7 + npix)
    edge = sorted({0, 1, 2, 3, 4, 5, 254, 255} | {t for t in range(thresh - 2, thresh + 3) if 0 <= t <= 255})
    img = np.array(np.meshgrid(edge, edge, edge)).reshape(3, -1).T.astype(np.uint8)
    img = rng.permutation(np.concatenate([img, rng.integers(0, 256, (npix, 3), dtype=np.uint8)]))[:npix]
    if 2 <= thresh <= 255:
        img[0] = thresh - 1
    want = O.preprocess_rgba(img, thresh)
    if 2 <= thresh <= 255:
        assert O.bgr2gray(img[:1])[0] > 0 and tuple(want[0]) == (0, 0, 0, 0)
    assert np.array_equal(vis.preprocess_rgba(img, thresh), want)


# ---------------------------------------------------------------- ofc_flow_to_bgr
def check_flow_to_bgr(vis, flow):
    got, mm = vis.flow_to_bgr(flow)
    want, wm = O.flow_to_bgr(flow)
    assert np.array_equal(got, want)
    assert abs(mm - wm) <= 1e-6 * abs(wm)
    return got


@pytest.mark.parametrize("kind", ["lin", "log"])
def test_flow_to_bgr_direction_by_magnitude_sweep(vis, kind):
    """every octant, the axes and diagonals, the hue wrap at 360 degrees, V from exactly 0 to exactly 255; 'log' spans
    magnitudes 1e-15 .. 1e15 in one frame (W*H = 100 039, so the last lane takes the scalar path)"""
    got = check_flow_to_bgr(vis, direction_sweep(kind).reshape(1, -1, 2))
    assert got.max() == 255 and len(np.unique(got.reshape(-1, 3), axis=0)) > (1000 if kind == "lin" else 100)


def test_flow_to_bgr_axes_and_diagonals(vis):
    """(+-a, 0), (0, +-a), (+-a, +-a): a over 2^-20 .. 2^20; a few steps apart so that V takes many values on the exact
    axes; and from the smallest to the largest a whose squares (and their sum) are normal and finite in f32"""
    dirs = np.array([(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)], np.float32)
    for a in (2.0 ** np.arange(-20, 21), np.linspace(0.5, 8, 16), [1.1e-19, 1e-10, 1.0, 1e10, 1.2e19]):
        a = np.asarray(a, np.float32)
        check_flow_to_bgr(vis, (a[:, None, None] * dirs[None]).reshape(len(a), 8, 2))


def test_flow_to_bgr_constant_but_one_pixel(vis):
    flow = np.full((37, 53, 2), 0.75, np.float32)
    flow[20, 31] = (-4.0, 2.5)
    got = check_flow_to_bgr(vis, flow)
    assert got[20, 31].max() >= 254 and np.delete(got.reshape(-1, 3), 20 * 53 + 31, 0).max() == 0


@pytest.mark.parametrize("W,H", [(1, 1), (5, 1), (3, 2), (7, 1), (13, 11), (1, 2), (3, 1)])
def test_flow_to_bgr_small_and_ragged_frames(vis, W, H):
    """1x1 (max == min: black) and W*H % 4 in {1, 2, 3}"""
    flow = (np.random.default_rng(W * 31 + H).standard_normal((H, W, 2)) * 3).astype(np.float32)
    check_flow_to_bgr(vis, flow)


@pytest.mark.parametrize("W,H", [(480, 270), (481, 271)])
@pytest.mark.parametrize("n", [2, 5])
def test_flow_to_bgr_dev_many_frames(vis, W, H, n):
    """ofc_flow_to_bgr_dev with n_frames > 1: each frame is normalised by its own min/max and reports its own mean, whatever
    its neighbours hold (ranges from 1e-6 to 1e4, one frame all zero), also when W*H*3 % 4 != 0 so that frames 1.. start
    off a dword boundary; and with mean_mag_dev = NULL"""
    rng = np.random.default_rng(n * W)
    scale = [3.0, 0.0, 1e4, 1e-6, 40.0][:n]
    flows = np.stack([(rng.standard_normal((H, W, 2)) * s).astype(np.float32) for s in scale])
    got, mean = vis.flow_to_bgr_frames(flows)
    for i in range(n):
        one, mm = vis.flow_to_bgr(flows[i])
        assert np.array_equal(got[i], one), i
        assert np.array_equal(one, O.flow_to_bgr(flows[i])[0]), i
        assert mean[i] == np.float32(mm), (i, mean[i], mm)
    got2, none = vis.flow_to_bgr_frames(flows, want_mean=False)
    assert none is None and np.array_equal(got2, got)


# ---------------------------------------------------------------- ofc_grid_cell_means / ofc_grid_cell_mean_flow
def grid_frames(rows, cols):
    return [(W, H) for W, H in [(1281, 719), (64, 48), (cols, rows)] if W >= cols and H >= rows]


@pytest.mark.parametrize("rows,cols", GRIDS)
def test_grid_cell_means_grids(vis, rows, cols):
    """ofc_grid_cell_means: cell sizes that do not divide the frame, rows == 1 / cols == 1 (no white row / column at all),
    cells smaller than one wave down to 1x1 (where every cell but those of the first row and column is all white)"""
    for W, H in grid_frames(rows, cols):
        frame = np.random.default_rng(rows + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        mean, hsv = vis.grid_cell_means(frame, rows, cols)
        om, oh = O.grid_cell_means(frame, rows, cols)
        assert np.array_equal(mean, om) and np.array_equal(hsv, oh), (W, H)


def test_grid_cell_means_rejects_grids_that_do_not_fit(vis):
    frame = np.zeros((48, 64, 3), np.uint8)
    with pytest.raises(ValueError):
        vis.grid_cell_means(frame, 14, 65)           # W < cols
    with pytest.raises(ValueError):
        vis.grid_cell_means(frame, 0, 25)            # rows = 0


@pytest.mark.parametrize("rows,cols", GRIDS)
def test_grid_cell_mean_flow_grids(rows, cols):
    """ofc_grid_cell_mean_flow against the float64 numpy block mean.  The kernel sums in f64 (error ~1e-16 relative, values
    of one sign dominate so nothing cancels) and rounds to f32 once, so it may differ from the f32 rounding of numpy's mean
    only by landing on the other neighbour: one f32 ulp of the result."""
    from opticalflowclustering_amd.stream import grid_cell_mean_flow
    for W, H in grid_frames(rows, cols):
        flow = np.random.default_rng(cols + H).uniform(-2.0, 6.0, (H, W, 2)).astype(np.float32)
        ys, xs = H // rows, W // cols
        want = flow[:ys * rows, :xs * cols].astype(np.float64).reshape(rows, ys, cols, xs, 2).mean((1, 3)).reshape(-1, 2)
        got = grid_cell_mean_flow(flow, rows, cols)
        assert got.shape == want.shape
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all(), (W, H)


# ---------------------------------------------------------------- ofc_grid_kmeans / ofc_grid_kmeans_dev
def maximin_init(X, k):
    seeds = [X[0].astype(np.int64)]
    for _ in range(1, k):
        d = np.min([((X.astype(np.int64) - s) ** 2).sum(1) for s in seeds], 0)
        seeds.append(X[int(np.argmax(d))].astype(np.int64))
    return np.array(seeds, np.float64)


def ref_grid_kmeans(frame, rows, cols, k, channel_order=0, init=None, max_iter=300, tol=1e-4):
    """per cell: extract_cell -> swap if channel_order -> preprocess_rgba -> kmeans_fit -> dominant by bincount(predict),
    first maximum -> rint -> bgr2hsv; -> (dominant centre before rint, after rint, hsv)"""
    raw = np.empty((rows * cols, 4))
    for c in range(rows * cols):
        cell = O.extract_cell(frame, c, rows, cols)
        if channel_order:
            cell = cell[..., ::-1]
        X = O.preprocess_rgba(cell).reshape(-1, 4)
        oc, _, _, _ = O.kmeans_fit(X, maximin_init(X, k) if init is None else init[c], max_iter, tol)
        counts = np.bincount(O.kmeans_predict(X, oc), minlength=k)
        raw[c] = oc[int(np.argmax(counts))]
    cen = np.rint(raw)
    return raw, cen, O.bgr2hsv(cen[:, :3].astype(np.uint8))


def assert_grid_kmeans(got, ref):
    """rint'ed dominant centre and its hsv equal the oracle's, every cell.  One exception, found with this test: a cluster
    of even size often has an exact mean of n + 1/2 in some component (48960 / 384 = 127.5), and sklearn's centred
    arithmetic, the oracle's and the kernel's each deliver it as n + 1/2 -+ 1e-13 depending on the order of their sums,
    so rint lands on either side -- in the reference as well.  A component whose oracle value is within 1e-9 of a half
    (the agreement required of the unrounded centres, test_gpu_color.py) may therefore be either neighbour; the hsv of
    such a cell must be that of the centre the kernel reports.  Such cells are few."""
    (cen, hsv), (raw, ocen, ohsv) = got, ref
    half = np.abs(raw - np.floor(raw) - 0.5) <= 1e-9
    assert np.array_equal(cen[~half], ocen[~half]), np.flatnonzero(((cen != ocen) & ~half).any(1))[:10]
    assert (np.abs(cen[half] - raw[half]) <= 0.5 + 1e-9).all()
    assert np.array_equal(cen, np.rint(cen))
    clean = ~half.any(1)
    assert clean.mean() >= 0.95
    assert np.array_equal(hsv[clean], ohsv[clean])
    assert np.array_equal(hsv, O.bgr2hsv(cen[:, :3].astype(np.uint8)))


def blocky_frame(W, H, seed):
    """a few flat-ish colour populations with noise, dark pixels below the threshold of 30, and two cells (of the 14x25
    grid: cell 0 and an interior one) of one flat colour, so that with the white lines a cell holds two distinct points and
    maximin seeds tie and repeat for k > 2"""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (6, 3))
    pal[0] = (10, 20, 29)
    idx = rng.integers(0, 6, (H // 8 + 1, W // 8 + 1)).repeat(8, 0).repeat(8, 1)[:H, :W]
    f = np.clip(pal[idx] + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
    ys, xs = H // 14, W // 25
    f[:ys, :xs] = (200, 40, 90)
    f[5 * ys:6 * ys, 7 * xs:8 * xs] = (35, 180, 0)
    return f


@pytest.mark.parametrize("k", [1, 2, 4, 5, 8, 9, 16])
def test_grid_kmeans_device_seeding_every_cell(vis, k):
    """ofc_grid_kmeans, k-sweep over the three kernel instantiations (KMAX 4, 8, 16) with maximin seeding on the device,
    every one of the 350 cells of a 640x360 frame (25x25-pixel cells: 625 points, not a multiple of 256)"""
    frame = blocky_frame(640, 360, 1)
    assert_grid_kmeans(vis.grid_kmeans(frame, k=k), ref_grid_kmeans(frame, 14, 25, k))


@pytest.mark.parametrize("rows,cols,W,H", [(3, 4, 640, 360), (14, 25, 1275, 714)])
def test_grid_kmeans_other_geometries(vis, rows, cols, W, H):
    """(3,4) on 640x360: 160x120 = 19 200-point cells; (14,25) on 1275x714: the reference's 51x51 cells"""
    frame = blocky_frame(W, H, rows)
    assert_grid_kmeans(vis.grid_kmeans(frame, k=2, rows=rows, cols=cols), ref_grid_kmeans(frame, rows, cols, 2))


def test_grid_kmeans_channel_swap_with_k3(vis):
    frame = blocky_frame(640, 360, 3)
    cen, hsv = vis.grid_kmeans(frame, k=3, channel_order=1)
    assert_grid_kmeans((cen, hsv), ref_grid_kmeans(frame, 14, 25, 3, channel_order=1))
    assert not np.array_equal(cen, vis.grid_kmeans(frame, k=3)[0])


def test_grid_kmeans_explicit_init_k2(vis):
    frame = blocky_frame(640, 360, 4)
    rng = np.random.default_rng(4)
    init = np.stack([np.array([[0, 0, 0, 0], [180, 180, 180, 255.0]]) + rng.uniform(0, 40, (2, 4)) for _ in range(350)])
    assert_grid_kmeans(vis.grid_kmeans(frame, k=2, init=init), ref_grid_kmeans(frame, 14, 25, 2, init=init))


def test_grid_kmeans_dev_three_frames(vis):
    """ofc_grid_kmeans_dev, n_frames = 3: problem p works on frame p // cells.  Three different resident frames in one
    call equal three single-frame calls (and the oracle)"""
    frames = np.stack([blocky_frame(640, 360, 10 + i) for i in range(3)])
    cen, hsv = vis.grid_kmeans_frames(frames, k=3)
    assert cen.shape == (3, 350, 4) and hsv.shape == (3, 350, 3)
    for i in range(3):
        c1, h1 = vis.grid_kmeans(frames[i], k=3)
        assert np.array_equal(cen[i], c1) and np.array_equal(hsv[i], h1), i
    assert not np.array_equal(cen[0], cen[1]) and not np.array_equal(cen[1], cen[2])
    assert_grid_kmeans((cen[2], hsv[2]), ref_grid_kmeans(frames[2], 14, 25, 3))


def test_grid_kmeans_rejections(vis, L):
    """refused on the host before any launch: fewer points per cell than clusters, a cell beyond the LDS-resident limit"""
    with pytest.raises(ValueError, match="n_samples=4 should be >= n_clusters=5"):
        vis.grid_kmeans(np.zeros((28, 50, 3), np.uint8), k=5)
    with pytest.raises(L.OfcError, match="24576") as e:
        vis.grid_kmeans(np.zeros((200, 200, 3), np.uint8), k=1, rows=1, cols=1)      # one cell of 40 000 pixels
    assert e.value.code == L.OFC_EUNSUPPORTED


# ---------------------------------------------------------------- ofc_kmeans_fit_batched
def rgba_points(rng, n):
    X = np.zeros((n, 4), np.uint8)
    m = rng.random(n) < 0.6
    X[m, :3] = rng.integers(30, 256, (int(m.sum()), 3))
    X[m, 3] = 255
    X[0] = 255
    return X


def spread_init(rng, X, k):
    uniq = np.unique(X, axis=0)
    return uniq[rng.choice(len(uniq), k, replace=False)].astype(np.float64) + np.arange(k)[:, None] * 1e-3


def check_batched(vis, Xs, inits, k, **kw):
    offsets = np.concatenate([[0], np.cumsum([len(X) for X in Xs])])
    cen, counts, labels, n_iter = vis.kmeans_fit_batched(np.concatenate(Xs), offsets, k, np.stack(inits), **kw)
    for p, X in enumerate(Xs):
        oc, ol, _, oi = O.kmeans_fit(X, inits[p], kw.get("max_iter", 300), kw.get("tol", 1e-4))
        assert n_iter[p] == oi, (p, n_iter[p], oi)
        assert np.array_equal(labels[offsets[p]:offsets[p + 1]], ol)
        assert np.abs(cen[p] - oc).max() <= 1e-9
        assert np.array_equal(counts[p], np.bincount(O.kmeans_predict(X, oc), minlength=k))
    return n_iter


def test_batched_at_the_lds_limit(vis, L):
    """24 576 points is the largest problem the LDS-resident kernel takes (5 bytes per point in 120 KiB); 24 577 is refused
    on the host"""
    rng = np.random.default_rng(0)
    X = rgba_points(rng, 24576)
    check_batched(vis, [X, rgba_points(rng, 300)], [spread_init(rng, X, 2)] * 2, 2)
    with pytest.raises(L.OfcError, match="24577") as e:
        vis.kmeans_fit_batched(np.zeros((24577, 4), np.uint8), [0, 24577], 2, np.zeros((1, 2, 4)))
    assert e.value.code == L.OFC_EUNSUPPORTED


def test_batched_max_iter_tol_and_k16(vis):
    """max_iter = 1 and 2 on data that needs more iterations (n_iter, labels and centres are those of the oracle stopped
    at the same point), tol = 0 (runs to strict convergence), k = 16"""
    rng = np.random.default_rng(1)
    Xs = [rgba_points(rng, n) for n in (2601, 977, 5852)]
    inits = [spread_init(rng, X, 5) for X in Xs]
    full = check_batched(vis, Xs, inits, 5)
    assert full.min() > 2
    assert check_batched(vis, Xs, inits, 5, max_iter=1).tolist() == [1, 1, 1]
    assert check_batched(vis, Xs, inits, 5, max_iter=2).tolist() == [2, 2, 2]
    strict = check_batched(vis, Xs, inits, 5, tol=0.0)
    assert (strict >= full).all()
    check_batched(vis, Xs, [spread_init(rng, X, 16) for X in Xs], 16)
    check_batched(vis, Xs, [spread_init(rng, X, 16) for X in Xs], 16, tol=0.0)


@pytest.mark.parametrize("n_mid", [0, 2])
def test_batched_names_the_undersized_problem(vis, n_mid):
    """an empty problem, or one with N < k, between two valid ones: OFC_EINVAL, and the message names its index"""
    rng = np.random.default_rng(2)
    Xs = [rgba_points(rng, 400), rgba_points(rng, n_mid + 1)[:n_mid], rgba_points(rng, 300)]
    offsets = np.concatenate([[0], np.cumsum([len(X) for X in Xs])])
    with pytest.raises(ValueError, match=r"problem 1: n_samples=%d " % n_mid):
        vis.kmeans_fit_batched(np.concatenate(Xs), offsets, 3, np.zeros((3, 3, 4)))


def test_batched_null_labels_and_counts(vis, L):
    """labels = NULL and counts = NULL (the library called directly): the other outputs are unchanged"""
    rng = np.random.default_rng(3)
    Xs = [rgba_points(rng, 700), rgba_points(rng, 2601)]
    X = np.concatenate(Xs)
    offsets = np.array([0, 700, 3301], np.int64)
    init = np.stack([spread_init(rng, x, 3) for x in Xs])
    cen, counts, labels, n_iter = vis.kmeans_fit_batched(X, offsets, 3, init)
    for drop in ("labels", "counts", "both"):
        c2, n2 = np.zeros_like(cen), np.zeros_like(n_iter)
        k2 = np.full_like(counts, -7)
        l2 = np.full_like(labels, -7)
        L.check(L.load().ofc_kmeans_fit_batched(0, L.ptr(X), L.ptr(offsets), 2, 4, 3, L.ptr(init), 300, 1e-4, L.ptr(c2),
                                                None if drop in ("counts", "both") else L.ptr(k2),
                                                None if drop in ("labels", "both") else L.ptr(l2), L.ptr(n2)))
        assert np.array_equal(c2, cen) and np.array_equal(n2, n_iter)
        assert np.array_equal(k2, counts) or (drop != "labels" and (k2 == -7).all())
        assert np.array_equal(l2, labels) or (drop != "counts" and (l2 == -7).all())


# ---------------------------------------------------------------- ofc_sliding_cosine
U = 2.0 ** -53


def exact_cosine(small, large):
    """every window's three sums in exact arithmetic (Python integers through Fraction; a float converts exactly), then
    one correctly rounded conversion per sum, one sqrt per norm, one product, one divide -- the kernel's own tail"""
    a = [Fraction(float(x)) for x in small]
    b = [Fraction(float(y)) for y in large]
    na2 = float(sum(x * x for x in a))
    out = []
    for i in range(len(b) - len(a) + 1):
        w = b[i:i + len(a)]
        dot, nb2 = float(sum(x * y for x, y in zip(a, w))), float(sum(y * y for y in w))
        n1, n2 = math.sqrt(na2), math.sqrt(nb2)
        out.append(0.0 if n1 == 0 or n2 == 0 else dot / (n1 * n2))
    return np.array(out)


def f64_path_bound(n_small):
    """|kernel - exact_cosine| when the sums are accumulated in f64: a sum of n rounded products carries at most n u
    relative to the sum of the absolute products (u = 2^-53, any summation order); for the norms that is n u relative,
    halved by the square root, plus u for the square root itself; for the dot product n u |a|.|b| <= n u |a| |b| by
    Cauchy-Schwarz, i.e. n u absolute on the similarity; the product and the divide add u each: (2 n + 4) u in all, since
    |similarity| <= 1.  exact_cosine rounds its three exact sums once each and shares the tail: 6 u.  Total (2 n + 10) u."""
    return (2 * n_small + 10) * U


def sliding(L, small, large):
    small, large = np.ascontiguousarray(small, np.float64), np.ascontiguousarray(large, np.float64)
    sims = np.full(len(large) - len(small) + 1, np.nan)
    L.check(L.load().ofc_sliding_cosine(0, L.ptr(small), len(small), L.ptr(large), len(large), L.ptr(sims)))
    return sims


@pytest.mark.parametrize("n_small", [1, 255, 256, 257, 1000])
def test_sliding_cosine_hue_columns_are_exact(L, n_small):
    """integer data in 0..179 (what the hue CSVs hold): every sum is an exact integer far below 2^53, so the result
    equals the exact one bit for bit, also when n_small exceeds the work-group (the strided loop) and when
    n_small == n_large (a single window)"""
    rng = np.random.default_rng(n_small)
    small = rng.integers(0, 180, n_small).astype(np.float64)
    for n_large in (n_small, n_small + 37):
        large = rng.integers(0, 180, n_large).astype(np.float64)
        large[:n_small // 2] = 0
        got = sliding(L, small, large)
        assert got.shape == (n_large - n_small + 1,)
        assert np.array_equal(got, exact_cosine(small, large))


def test_sliding_cosine_large_integers(L):
    """What is promised for integer-valued input (include/ofc.h): the sums are exact -- hence the result equal to
    exact_cosine bit for bit -- whenever n_small * max|small| * max|large|, n_small * max|small|^2 and
    n_small * max|large|^2 all stay below 2^63, the range of the integer accumulators; beyond that the sums are
    accumulated in f64 and the result is within f64_path_bound(n_small) of the exact one.  Before this was decided on the
    host, values near 2^31 overflowed the accumulators: small = [2e9, 2e9, 2e9] has sum x^2 = 1.2e19 > 2^63."""
    rng = np.random.default_rng(5)
    # near 2^20 with a long window: 1000 * 2^40 < 2^63, exact
    small = rng.integers(2 ** 20 - 1000, 2 ** 20, 1000).astype(np.float64) * rng.choice([-1, 1], 1000)
    large = rng.integers(2 ** 20 - 1000, 2 ** 20, 1100).astype(np.float64) * rng.choice([-1, 1], 1100)
    assert np.array_equal(sliding(L, small, large), exact_cosine(small, large))
    # near 2^27 with 256 values: the sums pass 2^53 but 256 * 2^54 = 2^62 < 2^63, still exact (one rounding of the sum)
    small = rng.integers(2 ** 27 - 1000, 2 ** 27, 256).astype(np.float64)
    large = rng.integers(2 ** 27 - 1000, 2 ** 27, 300).astype(np.float64)
    assert 256 * small.max() * large.max() < 2 ** 63 and (small ** 2).sum() > 2 ** 53
    assert np.array_equal(sliding(L, small, large), exact_cosine(small, large))
    # near 2^31: two products already pass 2^63
    for small, large in [(np.full(3, 2e9), np.array([2e9, 2e9, 2e9, 1e9, -2e9, 2147483647.0])),
                         (rng.integers(2 ** 31 - 10 ** 6, 2 ** 31, 257).astype(np.float64),
                          rng.integers(-2 ** 31 + 1, 2 ** 31, 400).astype(np.float64))]:
        got, want = sliding(L, small, large), exact_cosine(small, large)
        assert np.abs(got - want).max() <= f64_path_bound(len(small)), (got[:4], want[:4])
    assert abs(sliding(L, np.full(3, 2e9), np.full(3, 2e9))[0] - 1.0) <= f64_path_bound(3)


@pytest.mark.parametrize("n_small", [40, 257, 1000])
def test_sliding_cosine_mixed_input_takes_the_f64_path(L, n_small):
    """one non-integer value anywhere sends everything through the f64 sums; bound: f64_path_bound"""
    rng = np.random.default_rng(n_small)
    small = rng.integers(0, 180, n_small).astype(np.float64)
    large = rng.integers(0, 180, n_small + 64).astype(np.float64)
    large[-1] += 0.5
    got, want = sliding(L, small, large), exact_cosine(small, large)
    assert np.abs(got - want).max() <= f64_path_bound(n_small)
    small, large = rng.standard_normal(n_small) * 50, rng.standard_normal(n_small + 64) * 50
    assert np.abs(sliding(L, small, large) - exact_cosine(small, large)).max() <= f64_path_bound(n_small)


def test_sliding_cosine_rejections(L):
    """n_small > n_large and n_small = 0: OFC_EINVAL from the library itself (the Python wrapper returns an empty array
    for the first before it gets there)"""
    lib = L.load()
    a, b, out = np.ones(5), np.ones(3), np.zeros(8)
    assert lib.ofc_sliding_cosine(0, L.ptr(a), 5, L.ptr(b), 3, L.ptr(out)) == L.OFC_EINVAL
    assert b"n_small" in lib.ofc_last_error()
    assert lib.ofc_sliding_cosine(0, L.ptr(a), 0, L.ptr(b), 3, L.ptr(out)) == L.OFC_EINVAL
    assert not out.any()
