"""Cases and the reference of the camera-motion tests (test_camera_motion_host.py, test_gpu_camera_motion.py).

The reference is the definition of include/ofc.h in numpy int64, with Python ints for the totals and the solve in
fractions.Fraction, rounded once to float64.  It evaluates a model with plain f64 products and sums where the device runs
one fma chain; test_camera_motion_host.py proves every case well-conditioned (every valid pixel's residual at least 2^-20 px
from every round's threshold), so the two select the same pixels.

A case is a background with dyadic affine coefficients, plus noise on a 2^-8 px lattice, plus a displaced block of 10-15 %
of the frame, except where its builder says otherwise."""
from fractions import Fraction

import numpy as np

NMOM = 13
KIND = {"translation": 1, "affine": 2}
COORD_MOMENTS = (1, 2, 3, 4, 5, 7, 8, 10, 11)          # what a translation fit leaves 0
DEFAULT_THRESHOLDS = (4.0, 2.0, 1.0)
BACKGROUND = (1.5, 2.0 ** -7, -2.0 ** -8, -0.75, 2.0 ** -8, 2.0 ** -7)
MARGIN = 2.0 ** -20
KAPPA_MAX = 2.0 ** 20


# ---- the reference ----
def coords(W, H):
    """X = 2x - (W-1), Y = 2y - (H-1) as (H,W) int64"""
    X = np.broadcast_to(2 * np.arange(W, dtype=np.int64) - (W - 1), (H, W))
    Y = np.broadcast_to((2 * np.arange(H, dtype=np.int64) - (H - 1))[:, None], (H, W))
    return X, Y


def valid(f):
    f = np.asarray(f, np.float32)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(f).all(-1)) & (np.abs(f[..., 0]) < np.float32(1024)) & (np.abs(f[..., 1]) < np.float32(1024))


def predict(p, W, H):
    """(u^, v^) of a model as (H,W) f64 each: plain f64 arithmetic"""
    X, Y = coords(W, H)
    hx, hy = 0.5 * X.astype(np.float64), 0.5 * Y.astype(np.float64)
    return p[0] + p[1] * hx + p[2] * hy, p[3] + p[4] * hx + p[5] * hy


def residual(f, p):
    """sqrt((u-u^)^2 + (v-v^)^2) per pixel, f64; nan where the vector is not valid"""
    H, W = f.shape[:2]
    eu, ev = predict(p, W, H)
    ok = valid(f)
    g = np.where(ok[..., None], f, 0).astype(np.float64)
    return np.where(ok, np.hypot(g[..., 0] - eu, g[..., 1] - ev), np.nan)


def selected(f, p=None, c=None):
    ok = valid(f)
    if p is None:
        return ok
    H, W = f.shape[:2]
    eu, ev = predict(p, W, H)
    g = np.where(ok[..., None], f, 0).astype(np.float64)
    du, dv = g[..., 0] - eu, g[..., 1] - ev
    return ok & (du * du + dv * dv <= c * c)


def moments(f, p=None, c=None):
    """the thirteen moments of one pair's field (H,W,2) f32 over the pixels a round selects -> list of Python ints"""
    f = np.asarray(f, np.float32)
    H, W = f.shape[:2]
    X, Y = coords(W, H)
    ok, S = valid(f), selected(f, p, c)
    q = np.rint(np.where(S[..., None], f, 0).astype(np.float64) * 65536.0).astype(np.int64)
    qu, qv = q[..., 0], q[..., 1]
    Xs, Ys = np.where(S, X, 0), np.where(S, Y, 0)
    terms = (S.astype(np.int64), Xs, Ys, Xs * Xs, Xs * Ys, Ys * Ys, qu, Xs * qu, Ys * qu, qv, Xs * qv, Ys * qv)
    return [sum(int(v) for v in t.sum(axis=1)) for t in terms] + [int((~ok).sum())]


def _ilog2(v):
    return int(v).bit_length() - 1


def coord_scale(sqq, n):
    """the library's power-of-two coordinate scale (include/ofc.h) as a Fraction"""
    if sqq <= 0:
        return Fraction(1)
    e = (_ilog2(sqq) - _ilog2(n)) // 2
    return Fraction(1, 2 ** e) if e >= 0 else Fraction(2 ** -e)


def _inv3(A):
    (a, b, c), (d, e, f), (g, h, i) = A
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
           [d * h - e * g, b * g - a * h, a * e - b * d]]
    return [[v / det for v in row] for row in adj]


def solve_exact(m, kind):
    """-> (p (6,) f64 = the exact least-squares model rounded once, or None when the definition refuses the moments;
    kappa_inf of the scaled normal matrix, exact, as a float)"""
    n = m[0]
    q = Fraction(1, 65536)
    if kind == 1:
        if n < 1:
            return None, 1.0
        return np.array([float(Fraction(m[6], n) * q), 0, 0, float(Fraction(m[9], n) * q), 0, 0]), 1.0
    if n < 3:
        return None, 1.0
    sx, sy = coord_scale(m[3], n), coord_scale(m[5], n)
    A = [[Fraction(n), m[1] * sx, m[2] * sy], [m[1] * sx, m[3] * sx * sx, m[4] * sx * sy], [m[2] * sy, m[4] * sx * sy, m[5] * sy * sy]]
    d1 = A[1][1] - A[0][1] * A[0][1] / A[0][0]
    if d1 <= 0:
        return None, float("inf")
    l21 = (A[1][2] - A[0][2] * A[0][1] / A[0][0]) / d1
    d2 = A[2][2] - A[0][2] * A[0][2] / A[0][0] - l21 * l21 * d1
    if d2 <= 0:
        return None, float("inf")
    Ai = _inv3(A)
    norm = lambda M: max(sum(abs(v) for v in row) for row in M)
    p = []
    for b in ((m[6], m[7] * sx, m[8] * sy), (m[9], m[10] * sx, m[11] * sy)):
        x = [sum(Ai[r][k] * b[k] for k in range(3)) for r in range(3)]
        p += [float(x[0] * q), float(x[1] * sx * 2 * q), float(x[2] * sy * 2 * q)]
    return np.array(p), float(norm(A) * norm(Ai))


def solve_bound(kappa, p):
    """32 kappa_inf(A) 2^-53 |p|_inf per component: Cholesky's backward error for n = 3 times the condition number, with
    about 3x slack for rounding the integer inputs to f64"""
    return 32.0 * kappa * 2.0 ** -53 * np.abs(p).max()


def fit(f, kind, thresholds):
    """the rounds of one pair -> dict(models (T+1,6), moments (T+1,13) int64 as the history reports them, status,
    kappa [per solved round], margin = the least distance of a valid pixel's residual from a round's threshold,
    full [the thirteen moments of every round taken, before a translation fit's zeros])"""
    T = len(thresholds)
    models, moms, kappas, full = np.zeros((T + 1, 6)), np.zeros((T + 1, NMOM), np.int64), [], []
    p, status, margin = np.zeros(6), 0, np.inf
    for t in range(T + 1):
        if status:
            models[t] = p
            continue
        if t == 0:
            m = moments(f)
        else:
            c = thresholds[t - 1]
            m = moments(f, p, c)
            r = residual(f, p)
            if np.isfinite(r).any():
                margin = min(margin, float(np.nanmin(np.abs(r - c))))
        full.append(list(m))
        if kind == 1:
            for k in COORD_MOMENTS:
                m[k] = 0
        new, kappa = solve_exact(m, kind)
        if new is None:
            status = 2 if t == 0 else 1
        else:
            p = new
            kappas.append(kappa)
        models[t], moms[t] = p, m
    return dict(models=models, moments=moms, status=status, kappa=kappas, margin=margin, full=full)


# ---- the cases ----
def background(W, H, p=BACKGROUND, seed=1, noise=8, block=True):
    """the affine field of p plus noise of up to noise / 256 px on the 2^-8 lattice, plus a block of 10-15 % of the frame
    displaced by (6, -5) px"""
    rng = np.random.default_rng(seed)
    eu, ev = predict(np.asarray(p, np.float64), W, H)
    f = np.stack([eu, ev], -1)
    if noise:
        f += rng.integers(-noise, noise + 1, (H, W, 2)) / 256.0
    if block:
        idx = rng.permutation(W * H)[:max(1, int(round(0.125 * W * H)))] if min(W, H) < 8 else None
        if idx is None:
            bh, bw = max(1, int(round(H * 0.35))), max(1, int(round(W * 0.36)))
            y0, x0 = int(rng.integers(0, H - bh + 1)), int(rng.integers(0, W - bw + 1))
            f[y0:y0 + bh, x0:x0 + bw] += (6.0, -5.0)
        else:                                              # a frame too thin for a block: the same share, scattered
            f.reshape(-1, 2)[idx] += (6.0, -5.0)
    return f.astype(np.float32)


def _plain(W, H, seed):
    return background(W, H, seed=seed)


def _tiny(W, H, seed):
    """2 x 2: the exact affine field, no noise and no block (four pixels determine three coefficients and leave no room)"""
    return background(W, H, seed=seed, noise=0, block=False)


def _range_limit(W, H, seed):
    f = background(W, H, seed=seed)
    below = np.nextafter(np.float32(1024), np.float32(0))
    f[3, 5, 0], f[3, 6, 0], f[4, 5, 1], f[4, 6, 1] = 1024.0, below, -1024.0, -below
    f[10, 7] = (below, 1024.0)                             # one component valid, the other not: outside
    return f


def _non_finite(W, H, seed):
    f = background(W, H, seed=seed)
    f[2, 3, 0], f[2, 4, 1], f[5, 6, 0], f[7, 8, 1] = np.nan, np.inf, -np.inf, np.nan
    f[9, 9] = (np.nan, np.inf)
    f[H - 1, W - 1, 0] = np.inf
    return f


def _ties(W, H, seed):
    """no camera motion, no block: vectors on the llrint ties +-2^-17 (to 0), +-3 * 2^-17 (to +-2), all selected in every round"""
    rng = np.random.default_rng(seed)
    f = (rng.integers(-1, 2, (H, W, 2)) * 2.0 + 1.0) * 2.0 ** -17 * rng.choice([-1.0, 1.0], (H, W, 2))
    f[::3, ::2, 0] = 2.0 ** -17
    f[1::3, ::2, 0] = -2.0 ** -17
    return f.astype(np.float32)


def _all_outside(W, H, seed):
    f = np.full((H, W, 2), np.nan, np.float32)
    f[::2, :, 0], f[::2, :, 1] = 1024.0, 0.5
    return f


def _starved(W, H, seed):
    """every pixel's noise is at least 1/4 px long in u, and round 2 selects within 1/16 px: it finds no pixel"""
    rng = np.random.default_rng(seed)
    f = background(W, H, seed=seed, noise=0, block=False).astype(np.float64)
    f[..., 0] += rng.integers(64, 129, (H, W)) / 256.0 * rng.choice([-1.0, 1.0], (H, W))
    return f.astype(np.float32)


def _constant(W, H, seed):
    return np.broadcast_to(np.array([1.25, -0.5], np.float32), (H, W, 2)).copy()


class Case:
    def __init__(self, name, W, H, kind, builders, thresholds=DEFAULT_THRESHOLDS, seed=1):
        self.name, self.W, self.H, self.kind, self.thresholds, self.seed = name, W, H, KIND[kind], tuple(thresholds), seed
        self.model = kind
        self.builders = builders
        self.npair = len(builders)

    def __repr__(self):
        return self.name

    def field(self):
        """(npair, H, W, 2) f32"""
        return np.stack([b(self.W, self.H, self.seed + 100 * i) for i, b in enumerate(self.builders)])


# seeds: 1 unless test_camera_motion_host.py's margin or conditioning proof failed with it (then the next that passes)
CASES = [
    Case("2x2", 2, 2, "affine", [_tiny]),
    Case("3x130", 3, 130, "affine", [_plain]),
    Case("130x3", 130, 3, "affine", [_plain]),
    Case("64x48", 64, 48, "affine", [_plain]),
    Case("64x48-x3", 64, 48, "affine", [_plain] * 3),
    Case("67x45", 67, 45, "affine", [_plain]),
    Case("67x45-x3-translation", 67, 45, "translation", [_plain] * 3),
    Case("257x5", 257, 5, "affine", [_plain]),
    Case("1x64-translation", 1, 64, "translation", [_plain]),
    Case("64x48-translation", 64, 48, "translation", [_plain]),
    Case("1920x24", 1920, 24, "affine", [_plain]),
    Case("range-limit", 64, 48, "affine", [_range_limit]),
    Case("non-finite", 67, 45, "affine", [_non_finite]),
    Case("non-finite-translation", 67, 45, "translation", [_non_finite]),
    Case("ties", 64, 48, "affine", [_ties]),
    Case("all-outside-in-the-middle", 64, 48, "affine", [_plain, _all_outside, _plain]),
    Case("all-outside-translation", 64, 48, "translation", [_all_outside]),
    Case("starved-in-round-2", 64, 48, "affine", [_starved], thresholds=(4.0, 0.0625, 1.0)),
    Case("constant", 64, 48, "affine", [_constant]),
]
BY_NAME = {c.name: c for c in CASES}

_cache = {}


def reference(case):
    """(the case's field, [fit(...) per pair]), computed once and shared: read-only"""
    if case.name not in _cache:
        f = case.field()
        f.setflags(write=False)
        _cache[case.name] = (f, [fit(f[i], case.kind, case.thresholds) for i in range(case.npair)])
    return _cache[case.name]


# ---- the clips of the pipeline, stream and command-line tests ----
CLIP_W, CLIP_H, CLIP_FRAMES = 64, 48, 4
STREAM_FRAMES, STREAM_BATCH, STREAM_GRID = 5, 2, (3, 4)
