"""The colour oracle (oracle/color_ref.c) against the plain definitions of what it restates, in float64 or exact-integer
numpy that shares no code with it.  The GPU kernels are compared with the oracle bit for bit (test_gpu_color*.py), so an
error in the oracle would be copied silently; these tests bound it.  Parity with cv2 itself stays unpinned (no cv2 here):
what is pinned is that each routine computes its documented formula within the error its number format allows."""
import numpy as np
import pytest

from oracle import oracle as O


def all_colours():
    """every 8-bit (b, g, r), 2^24 x 3 u8; colour i = (i & 255, (i >> 8) & 255, i >> 16)"""
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([a & 255, (a >> 8) & 255, a >> 16], 1).astype(np.uint8)


def direction_sweep(kind):
    """flow vectors (N, 2) f32: 100 003 directions round the circle, then the eight axis/diagonal directions exactly and
    the +-0.0 variants of the axes, each direction with a magnitude that cycles through a ladder co-prime with the count.
    kind 'lin': 257 magnitudes 0.01 .. 20 (a frame as the flow produces); 'log': 61 magnitudes 1e-15 .. 1e15."""
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


def exact_polar(v):
    """float64 magnitude and angle in degrees [0, 360) of f32 vectors; a zero component counts as +0 (cv2's convention:
    the angle of (x, -0.0) is 0 or 180, never 360, and that of the zero vector is 0)"""
    x, y = v[:, 0].astype(np.float64) + 0.0, v[:, 1].astype(np.float64) + 0.0
    ang = np.degrees(np.arctan2(y, x))
    return np.hypot(x, y), np.where(ang < 0, ang + 360.0, ang)


def circ(a, b, period):
    d = np.abs(np.asarray(a, np.float64) - b) % period
    return np.minimum(d, period - d)


def test_bgr2hsv_every_colour_against_the_definition():
    """V = max, S = 255 diff / V, H = 30 (g-b)/diff | 60 + 30 (b-r)/diff | 120 + 30 (r-g)/diff wrapped into [0, 180).
    The oracle multiplies by 12-bit fixed-point reciprocals: a table entry is off by at most 0.5 / 4096, the numerators
    reach 1275 (H, in units of diff/30: |h| <= 5 diff, diff <= 255) and 255 (S), and the result is rounded once, so
    |H - H_exact| <= 0.5 + 1275 * 0.5 / 4096 < 0.66 on the circle of 180 and |S - S_exact| <= 0.5 + 255 * 0.5 / 4096 < 0.54.
    Measured over all 2^24 colours: 0.640 (H), 0.522 (S), largest H 179."""
    bgr = all_colours()
    hsv = O.bgr2hsv(bgr)
    worst_h = worst_s = 0.0
    for lo in range(0, 1 << 24, 1 << 21):
        c = bgr[lo:lo + (1 << 21)].astype(np.float64)
        b, g, r = c[:, 0], c[:, 1], c[:, 2]
        v = c.max(1)
        diff = v - c.min(1)
        safe = np.where(diff > 0, diff, 1.0)
        h = np.where(v == r, 30 * (g - b) / safe, np.where(v == g, 60 + 30 * (b - r) / safe, 120 + 30 * (r - g) / safe))
        h = np.where(diff > 0, h % 180.0, 0.0)
        s = np.where(v > 0, 255 * diff / np.where(v > 0, v, 1.0), 0.0)
        got = hsv[lo:lo + (1 << 21)]
        assert np.array_equal(got[:, 2], v.astype(np.uint8))
        worst_h = max(worst_h, circ(got[:, 0], h, 180).max())
        worst_s = max(worst_s, np.abs(got[:, 1] - s).max())
    print("bgr2hsv: worst |dH| %.4f, worst |dS| %.4f, max H %d" % (worst_h, worst_s, hsv[:, 0].max()))
    assert hsv[:, 0].max() < 180
    assert worst_h <= 0.5 + 1275 * 0.5 / 4096 and worst_s <= 0.5 + 255 * 0.5 / 4096


def test_bgr2gray_every_colour_against_the_definition():
    """gray = 0.114 B + 0.587 G + 0.299 R.  The oracle uses the 15-bit coefficients 3735, 19235, 9798 (sum 2^15, so white
    stays 255) and rounds once: (x + 2^14) >> 15 is off by at most 0.5 from x / 2^15, and x / 2^15 is off from the
    definition by at most 255 * (|3735/2^15 - 0.114| + |19235/2^15 - 0.587| + |9798/2^15 - 0.299|)
    = 255 * (1.68e-5 + 5.62e-6 + 1.12e-5) = 0.0086.  Bound: 0.5086; the worst colour measured is 0.5030 off."""
    bgr = all_colours()
    gray = O.bgr2gray(bgr)
    coef = np.array([0.114, 0.587, 0.299])
    bound = 0.5 + 255 * np.abs(np.array([3735, 19235, 9798]) / 32768.0 - coef).sum()
    worst = 0.0
    for lo in range(0, 1 << 24, 1 << 21):
        want = bgr[lo:lo + (1 << 21)].astype(np.float64) @ coef
        worst = max(worst, np.abs(gray[lo:lo + (1 << 21)] - want).max())
    print("bgr2gray: worst |d| %.5f, bound %.5f" % (worst, bound))
    assert bound < 0.509 and worst <= bound


def f64_hsv2bgr(H, S, V):
    """the sector formula in float64, bytes by truncation: h = H / 30 mod 6, f = frac(h), s = S / 255, v = V / 255,
    table {v, v (1 - s), v (1 - s f), v (1 - s (1 - f))} picked per sector"""
    H, S, V = (np.asarray(a, np.float64) for a in (H, S, V))
    h = (H / 30.0) % 6.0
    sector = np.floor(h).astype(np.int64)
    f, s, v = h - sector, S / 255.0, V / 255.0
    tab = np.stack([v, v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))], 1)
    idx = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector]      # (n, 3): b, g, r
    return np.clip(np.floor(np.take_along_axis(tab, idx, 1) * 255.0), 0, 255).astype(np.int16)


# Share of the 3 * 2^24 output bytes on which the oracle's f32 evaluation and the float64 one truncate to different
# integers, measured with the oracle alone: 0.006347.  The exact channel value is a rational that is an integer, or
# within an f32 rounding of one, for a large family of (S, V) -- every S = 0 or f = 0 pixel has 255 * (V / 255) on the
# boundary -- which is why the rate is 0.6 % and not smaller.
HSV2BGR_FLIP_SHARE = 0.006347


def test_hsv2bgr_every_hsv_against_the_sector_formula():
    """every (H, S, V) in 0..255 each: H >= 180 occurs (the visualisation stores u8(angle / 2), 180 included) and wraps.
    The oracle evaluates the sector formula in f32 and truncates; against float64 a byte can differ only where the value
    sits on an integer boundary and the two roundings fall on different sides, so by 1 and never more.  The share of such
    bytes is capped at twice the measured HSV2BGR_FLIP_SHARE."""
    a = np.arange(1 << 24, dtype=np.uint32)
    hsv = np.stack([a >> 16, (a >> 8) & 255, a & 255], 1).astype(np.uint8)
    got = O.hsv2bgr(hsv)
    differ = 0
    for lo in range(0, 1 << 24, 1 << 21):
        h = hsv[lo:lo + (1 << 21)]
        d = np.abs(got[lo:lo + (1 << 21)].astype(np.int16) - f64_hsv2bgr(h[:, 0], h[:, 1], h[:, 2]))
        assert d.max() <= 1
        differ += int(d.sum())
    share = differ / (3.0 * (1 << 24))
    print("hsv2bgr: share of differing bytes %.6f" % share)
    assert share <= 2 * HSV2BGR_FLIP_SHARE


# Largest error of the oracle's angle against float64 atan2 over both sweeps, where the denominator guard (below) moves
# the angle by less than 1e-5 degrees, measured with the oracle alone.  OpenCV documents "about 0.3 degrees" for
# fastAtan2; the coefficient set restated here is an order of magnitude better than that.
CART_TO_POLAR_WORST_DEG = 0.009554


@pytest.mark.parametrize("kind", ["lin", "log"])
def test_cart_to_polar_against_hypot_and_atan2(kind):
    """magnitude = sqrtf(x*x + y*y) in f32 against the float64 hypot, while the squares stay normal (1e-15 .. 1e15 here).
    Each square and their sum are rounded (2^-24 relative each, at most 2 * 2^-24 on the sum), the square root halves that
    and rounds once more: 2^-23 relative, one ulp of f32 in the relative sense (FLT_EPSILON).  In units of the spacing at
    the result that is between 1 and 2, since the spacing is 2^-24 relative at the top of a binade; the measured worst case is
    1.17 spacings and 0.87 * 2^-23 relative, printed below.
    angle = the 7th-degree odd polynomial of c = min / (max + DBL_EPSILON) in degrees, folded by octant (isometries, so
    the error is that of the first octant) and converted to radians.  Asserted: 1.25 * CART_TO_POLAR_WORST_DEG plus what
    the guard in the denominator is allowed to move the angle, atan(c) - atan(c max / (max + DBL_EPSILON)), which is
    below 1e-5 degrees for max >= 1e-9 and reaches 7.7 degrees at 1e-15 (cv2 adds the same guard; a magnitude that small
    is normalised to V = 0 in any frame that holds a visible one).  The axis and diagonal directions and the +-0.0
    components are in the sweep."""
    v = direction_sweep(kind)
    mag, ang = O.cart_to_polar(v[:, 0], v[:, 1])
    m64, a64 = exact_polar(v)
    rel = np.abs(mag.astype(np.float64) - m64) / m64
    spacings = np.abs(mag.astype(np.float64) - m64) / np.spacing(m64.astype(np.float32)).astype(np.float64)
    err = circ(np.degrees(ang.astype(np.float64)), a64, 360)
    hi, lo = np.abs(v.astype(np.float64)).max(1), np.abs(v.astype(np.float64)).min(1)
    eps = np.finfo(np.float64).eps
    guard = np.degrees(np.arctan(lo / hi) - np.arctan(lo / (hi + eps)))
    big = hi >= 1e-9
    print("cartToPolar[%s]: worst magnitude error %.3f * 2^-23 relative = %.3f spacings, worst angle error %.5f deg where "
          "the guard is idle, %.3f deg overall" % (kind, rel.max() * 2 ** 23, spacings.max(), err[big].max(), err.max()))
    assert rel.max() <= 2.0 ** -23
    assert guard[big].max() < 1e-5
    assert (err <= 1.25 * CART_TO_POLAR_WORST_DEG + guard).all()
    zero = np.zeros(4, np.float32)
    mz, az = O.cart_to_polar(np.array([0.0, -0.0, 0.0, -0.0], np.float32), np.array([0.0, 0.0, -0.0, -0.0], np.float32))
    assert np.array_equal(mz, zero) and np.array_equal(az, zero)


@pytest.mark.parametrize("kind", ["lin", "log"])
def test_flow_to_bgr_against_the_float64_restatement(kind):
    """computeOpticalFlowModule.py:25-33 in float64: H = floor(angle / 2), S = 255, V = floor(255 (m - min) / (max - min)),
    then HSV2BGR.  The polynomial angle (<= 0.3 degrees off) moves H by at most 1 on the circle of 180, the f32
    normalisation moves V by at most 1, so every pixel must be the HSV2BGR (pinned above) of one of the nine (H, V)
    neighbours; S == 255 means the smallest channel is 0."""
    v = direction_sweep(kind)
    bgr, mm = O.flow_to_bgr(v.reshape(1, -1, 2))
    bgr = bgr.reshape(-1, 3)
    m64, a64 = exact_polar(v)
    H = np.floor(a64 / 2).astype(np.int64)
    V = np.floor(255 * (m64 - m64.min()) / (m64.max() - m64.min())).astype(np.int64)
    assert V.min() == 0 and V.max() == 255
    ok = np.zeros(len(v), bool)
    for dh in (-1, 0, 1):
        for dv in (-1, 0, 1):
            cand = np.stack([(H + dh) % 180, np.full(len(v), 255), np.clip(V + dv, 0, 255)], 1).astype(np.uint8)
            ok |= (O.hsv2bgr(cand) == bgr).all(1)
    assert ok.all(), (int((~ok).sum()), v[~ok][:5])
    assert (bgr.min(1) == 0).all()
    assert abs(mm - m64.mean()) <= 1e-6 * m64.mean()


GRIDS = [(1, 1), (1, 7), (5, 1), (14, 25), (9, 16)]


@pytest.mark.parametrize("rows,cols", GRIDS)
@pytest.mark.parametrize("W,H", [(1281, 719), (131, 97)])
def test_grid_cells_against_numpy_slicing(rows, cols, W, H):
    """KmeanGrids.py:52-113: cells of (H // rows) x (W // cols), the remainder ignored; when a cell is averaged its row 0
    is white iff it is not in the first grid row and its column 0 iff not in the first grid column; when it is read back
    for k-means both are white.  mean -> astype(uint8) truncates."""
    rng = np.random.default_rng(rows * 100 + cols + W)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ys, xs = H // rows, W // cols
    mean, hsv = O.grid_cell_means(frame, rows, cols)
    for cell in range(rows * cols):
        cy, cx = divmod(cell, cols)
        c = frame[cy * ys:(cy + 1) * ys, cx * xs:(cx + 1) * xs].astype(np.int64)
        assert c.shape == (ys, xs, 3)
        at_mean = c.copy()
        if cy >= 1:
            at_mean[0] = 255
        if cx >= 1:
            at_mean[:, 0] = 255
        assert np.array_equal(mean[cell], at_mean.sum((0, 1)) // (xs * ys)), cell
        c[0] = 255
        c[:, 0] = 255
        assert np.array_equal(O.extract_cell(frame, cell, rows, cols), c), cell
    assert np.array_equal(hsv, O.bgr2hsv(mean))


@pytest.mark.parametrize("thresh", [0, 1, 30, 255, 256])
def test_preprocess_rgba_against_numpy(thresh):
    """preprocess_image (KmeanGrids.py:269-286): image[image < thresh] = 0 per channel, alpha = 255 where the grey value
    of the THRESHOLDED pixel is > 0.  The grey value rounds 0.114 B + 0.587 G + 0.299 R, which is never within 1e-3 of
    0.5 (114 b + 587 g + 299 r = 500 has no solution), so the float64 definition decides > 0 without ambiguity."""
    rng = np.random.default_rng(thresh)
    edge = sorted({0, 1, 2, 3, 4, 5, 254, 255} | {t for t in range(thresh - 2, thresh + 3) if 0 <= t <= 255})
    img = np.array(np.meshgrid(edge, edge, edge)).reshape(3, -1).T.astype(np.uint8)
    img = np.concatenate([img, rng.integers(0, 256, (4096, 3), dtype=np.uint8)])
    kept = np.where(img < thresh, 0, img)
    alpha = np.where(np.rint(kept.astype(np.float64) @ np.array([0.114, 0.587, 0.299])) > 0, 255, 0)
    want = np.concatenate([kept, alpha[:, None]], 1).astype(np.uint8)
    got = O.preprocess_rgba(img.reshape(1, -1, 3), thresh).reshape(-1, 4)
    assert np.array_equal(got, want)
    raw_alpha = np.rint(img.astype(np.float64) @ np.array([0.114, 0.587, 0.299])) > 0
    if 1 < thresh <= 255:
        assert (raw_alpha & (alpha == 0)).any()          # alpha comes from the thresholded triple, not the raw one
