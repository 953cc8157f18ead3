"""The photometric check of include/ofc.h twice over -- a vectorised numpy reference and an independent per-pixel loop in
plain Python integers -- and the table of cases that test_photometric_host.py proves on the CPU and
test_gpu_photometric.py runs on the device."""
import math
import os

import numpy as np

from tests.consistency_cases import SPECIALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, MISMATCH, LEAVES, INVALID, NSTATE, NSTAT = 0, 1, 2, 3, 4, 5
SHARE = 2048                      # OFC_PHOTO_SHARE: the pixels of a pair a work-group takes
ONE = 65536
TAU_Q, KAPPA_Q = 2048, 128        # what tau 8 and kappa 0.5 quantise to
TAU_MAX, KAPPA_MAX = 65280, 1024
Q = 1.0 / ONE                     # one quantum in px
FRACS = (0, 1, 32768, 65535)
THRESHOLDS = ((0, 0), (TAU_Q, KAPPA_Q), (TAU_MAX, 0), (0, KAPPA_MAX))


# ---- the reference: numpy, whole fields at a time ----
def core_pair(I0, I1, fwd):
    """one pair: (H,W) u8 twice and (H,W,2) f32 -> valid, inside (H,W) bool, J, e, c (H,W) int64; all but `valid` are
    meaningful only where the pixel is compared (valid and inside)"""
    H, W = I0.shape
    f = np.asarray(fwd, np.float32)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(f).all(-1) & (np.abs(f) < np.float32(1024)).all(-1)
        q = np.rint(np.where(valid[..., None], f, np.float32(0)).astype(np.float64) * 65536.0).astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    X, Y = xx * ONE + q[..., 0], yy * ONE + q[..., 1]
    inside = (X >= 0) & (X <= (W - 1) << 16) & (Y >= 0) & (Y <= (H - 1) << 16)
    ix, iy = np.clip(X >> 16, 0, W - 1), np.clip(Y >> 16, 0, H - 1)
    fx, fy = X & 65535, Y & 65535
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    g = I1.astype(np.int64)
    taps = np.stack([g[iy, ix], g[iy, ix1], g[iy1, ix], g[iy1, ix1]])
    wts = np.stack([(ONE - fx) * (ONE - fy), fx * (ONE - fy), (ONE - fx) * fy, fx * fy])
    S = (wts * taps).sum(0)
    J = (S + (1 << 23)) >> 24
    e = J - 256 * I0.astype(np.int64)
    c = taps.max(0) - taps.min(0)
    return valid, inside, J, e, c


def verdict(core, tau_q, kappa_q):
    """core_pair's result and the two thresholds -> state (H,W) u8, stats (5,) int64, warped (H,W) u16"""
    valid, inside, J, e, c = core
    compared = valid & inside
    good = np.abs(e) <= tau_q + kappa_q * c
    state = np.where(~valid, INVALID, np.where(~inside, LEAVES, np.where(good, OK, MISMATCH))).astype(np.uint8)
    stats = np.concatenate([np.bincount(state.ravel(), minlength=NSTATE), [np.abs(e)[compared].sum()]]).astype(np.int64)
    return state, stats, np.where(compared, J, 0).astype(np.uint16)


def reference(frames, fwd, tau_q=TAU_Q, kappa_q=KAPPA_Q):
    """(n+1,H,W) u8 and (n,H,W,2) f32 -> state (n,H,W) u8, stats (n,5) int64, warped (n,H,W) u16"""
    out = [verdict(core_pair(frames[t], frames[t + 1], fwd[t]), tau_q, kappa_q) for t in range(len(fwd))]
    return tuple(np.stack([o[j] for o in out]) for j in range(3))


# ---- the same definition as a loop over the pixels in Python integers.  Shares nothing with the numpy above. ----
def _q(u):
    """llrint((double)u * 65536) of a valid f32, or None"""
    u = float(u)
    if not math.isfinite(u) or not abs(u) < 1024.0:
        return None
    return int(round(u * 65536.0))              # exact product; round() goes to even on ties, as llrint does


def loop_pair(I0, I1, fwd, tau_q, kappa_q):
    H, W = len(I0), len(I0[0])
    state = [[0] * W for _ in range(H)]
    warped = [[0] * W for _ in range(H)]
    esum, smax = 0, 0
    for y in range(H):
        for x in range(W):
            qu, qv = _q(fwd[y][x][0]), _q(fwd[y][x][1])
            if qu is None or qv is None:
                state[y][x] = INVALID
                continue
            X, Y = x * 65536 + qu, y * 65536 + qv
            if not (0 <= X <= (W - 1) * 65536 and 0 <= Y <= (H - 1) * 65536):
                state[y][x] = LEAVES
                continue
            ix, fx, iy, fy = X // 65536, X % 65536, Y // 65536, Y % 65536
            ix1, iy1 = min(ix + 1, W - 1), min(iy + 1, H - 1)
            a00, a10, a01, a11 = I1[iy][ix], I1[iy][ix1], I1[iy1][ix], I1[iy1][ix1]
            S = (65536 - fx) * (65536 - fy) * a00 + fx * (65536 - fy) * a10 + (65536 - fx) * fy * a01 + fx * fy * a11
            top, bot = a00 * (65536 - fx) + a10 * fx, a01 * (65536 - fx) + a11 * fx
            assert top < 2 ** 24 and bot < 2 ** 24 and S == top * (65536 - fy) + bot * fy      # the form the header allows
            smax = max(smax, S)
            J = (S + 2 ** 23) // 2 ** 24
            assert 0 <= J <= 65280
            e = J - 256 * I0[y][x]
            c = max(a00, a10, a01, a11) - min(a00, a10, a01, a11)
            assert abs(e) <= 65280 and tau_q + kappa_q * c < 2 ** 31
            state[y][x] = OK if abs(e) <= tau_q + kappa_q * c else MISMATCH
            warped[y][x] = J
            esum += abs(e)
    return state, warped, esum, smax


def loop(frames, fwd, tau_q=TAU_Q, kappa_q=KAPPA_Q):
    """-> state, stats, warped as reference(), and the largest S met"""
    g, f = frames.tolist(), fwd.tolist()
    states, warps, stats, smax = [], [], [], 0
    for t in range(len(f)):
        s, w, esum, m = loop_pair(g[t], g[t + 1], f[t], tau_q, kappa_q)
        states.append(s)
        warps.append(w)
        stats.append([sum(row.count(k) for row in s) for k in range(NSTATE)] + [esum])
        smax = max(smax, m)
    n, H, W = fwd.shape[:3]
    return (np.array(states, np.uint8).reshape(n, H, W), np.array(stats, np.int64), np.array(warps, np.uint16).reshape(n, H, W),
            smax)


# ---- the cases ----
class Case:
    def __init__(self, name, frames, fwd, marks=None):
        self.name = name
        self.frames, self.fwd = np.ascontiguousarray(frames, np.uint8), np.ascontiguousarray(fwd, np.float32)
        n, H, W = self.fwd.shape[:3]
        assert self.fwd.ndim == 4 and self.fwd.shape[3] == 2 and self.frames.shape == (n + 1, H, W)
        self.frames.setflags(write=False)
        self.fwd.setflags(write=False)
        self.marks = marks or {}                  # named pixels (pair, y, x) the host test asks about
        self._core, self._ref = None, {}

    def __repr__(self):
        return self.name

    @property
    def shape(self):
        return self.fwd.shape[:3]

    def core(self):
        if self._core is None:                    # computed once, shared, never written
            self._core = [core_pair(self.frames[t], self.frames[t + 1], self.fwd[t]) for t in range(len(self.fwd))]
        return self._core

    def reference(self, tau_q=TAU_Q, kappa_q=KAPPA_Q):
        key = (tau_q, kappa_q)
        if key not in self._ref:
            out = [verdict(c, tau_q, kappa_q) for c in self.core()]
            self._ref[key] = tuple(np.stack([o[j] for o in out]) for j in range(3))
            for a in self._ref[key]:
                a.setflags(write=False)
        return self._ref[key]

    def chosen(self):
        """(pair, y, x) and |e| of one compared pixel with |e| >= 1, the middle one of them in raster order, or None"""
        where = [(t, int(y), int(x)) for t, (valid, inside, _, e, _) in enumerate(self.core())
                 for y, x in np.argwhere(valid & inside & (e != 0))]
        if not where:
            return None
        t, y, x = where[len(where) // 2]
        return (t, y, x), int(abs(self.core()[t][3][y, x]))

    def thresholds(self):
        """the four common pairs, and with a chosen pixel (tau_q, 0) = its |e| exactly and one less: equality passes, one
        less fails"""
        ch = self.chosen()
        return THRESHOLDS + (((ch[1], 0), (ch[1] - 1, 0)) if ch else ())


SIZES = ((1, 1, 1), (1, 7, 2), (7, 1, 3), (5, 3, 3), (6, 3, 2), (64, 32, 1), (64, 32, 3), (89, 23, 2), (683, 3, 2), (100, 62, 2))


# frames: n+1 of them
def frames_random(r, n, H, W):
    return r.integers(0, 256, (n + 1, H, W)).astype(np.uint8)


def frames_smooth(r, n, H, W):
    """a slow texture that slides by about a pixel per frame, with noise: small errors, not all of them zero"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = [128 + 90 * np.sin((xx - 1.2 * t) / 5.0) * np.cos((yy + 0.7 * t) / 4.0) + r.normal(0, 3, (H, W)) for t in range(n + 1)]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def frames_constant(r, n, H, W):
    return np.full((n + 1, H, W), 77, np.uint8)


def frames_black_white(r, n, H, W):
    """all 0 against all 255, alternating: J = 65280 against I0 = 0 and J = 0 against I0 = 255, |e| = 65280 both ways"""
    f = np.zeros((n + 1, H, W), np.uint8)
    f[1::2] = 255
    return f


def frames_checker(r, n, H, W):
    """a 0/255 checkerboard that flips from frame to frame: c = 255 wherever two taps differ"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(((xx + yy + t) & 1) * 255).astype(np.uint8) for t in range(n + 1)])


# fields
def field_zero(r, n, H, W):
    return np.zeros((n, H, W, 2), np.float32)


def field_whole(r, n, H, W):
    """per pair its own whole-pixel translation"""
    f = np.empty((n, H, W, 2), np.float32)
    for t in range(n):
        f[t] = ((1, 0), (-1, 1), (2, -1))[t % 3]
    return f


def field_fractions(r, n, H, W):
    """every combination of the fractions FRACS in x and y, cycling over the pixels, on small whole offsets"""
    k = np.arange(n * H * W).reshape(n, H, W)
    fx, fy = np.array(FRACS)[k % 4], np.array(FRACS)[k // 4 % 4]
    f = np.stack([(k // 16 % 3 - 1) + fx * Q, (k // 48 % 3 - 1) + fy * Q], -1).astype(np.float32)
    assert np.array_equal(np.rint(f.astype(np.float64) * ONE).astype(np.int64) & 65535, np.stack([fx, fy], -1))    # representable
    return f


def field_edges(r, n, H, W):
    """every pixel lands on the last column (row) exactly, or one quantum past it, or on column (row) 0, or one quantum
    before it, in turn; the other component whole or a half"""
    assert W <= 128 and H <= 128                              # 7 + 16 bits: the quantum is representable
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    k = np.arange(n * H * W).reshape(n, H, W)
    kind = k % 8
    u = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [W - 1 - xx, W - 1 - xx + Q, -xx, -xx - Q], (k // 8 % 2) * 0.5)
    v = np.select([kind == 4, kind == 5, kind == 6, kind == 7], [H - 1 - yy, H - 1 - yy + Q, -yy, -yy - Q], (k // 8 % 2) * 0.5)
    f = np.stack([np.broadcast_to(u, k.shape), np.broadcast_to(v, k.shape)], -1).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), np.stack([np.broadcast_to(u, k.shape), np.broadcast_to(v, k.shape)], -1))
    return f


def field_specials(r, n, H, W):
    """every special of SPECIALS in u and in v, cycling over the pixels, over small random vectors"""
    f = r.uniform(-0.75, 0.75, (n, H, W, 2)).astype(np.float32)
    flat = f.reshape(-1, 2)
    where = np.arange(0, len(flat), 2 if len(flat) >= 24 else 1)            # every other pixel, so that clean ones remain
    j = np.arange(len(where))
    flat[where, (j // len(SPECIALS)) % 2] = np.array(SPECIALS, np.float32)[j % len(SPECIALS)]
    return f


def field_random(r, n, H, W):
    return r.uniform(-3.0, 3.0, (n, H, W, 2)).astype(np.float32)


def field_mixed(r, n, H, W):
    """random vectors within +-3 px with a special value in about one vector of forty"""
    f = field_random(r, n, H, W)
    flat = f.reshape(-1, 2)
    where = r.choice(len(flat), max(1, len(flat) // 40), replace=False)
    flat[where, r.integers(0, 2, len(where))] = np.array(SPECIALS, np.float32)[r.integers(0, len(SPECIALS), len(where))]
    return f


def field_small(r, n, H, W):
    """about the motion of frames_smooth, to a fraction of a pixel"""
    return (np.array([1.2, -0.7]) + r.normal(0, 0.15, (n, H, W, 2))).astype(np.float32)


def _make(seed, size, field, frames):
    W, H, n = size
    r = np.random.default_rng(seed)
    return Case(f"{field.__name__[6:]}-{frames.__name__[7:]}-{W}x{H}-n{n}", frames(r, n, H, W), field(r, n, H, W))


def _cases():
    out, seed = [], 1000
    for size in SIZES:                                         # every size: random vectors and specials over random frames
        out.append(_make(seed, size, field_mixed, frames_random))
        seed += 1
    small = [s for s in SIZES if s[0] <= 128]
    for size in small:                                         # the landing edges at every size that can represent them
        out.append(_make(seed, size, field_edges, frames_random))
        seed += 1
    for size in ((5, 3, 3), (64, 32, 3), (683, 3, 2)):
        for field, frames in ((field_zero, frames_random), (field_zero, frames_constant), (field_whole, frames_random),
                              (field_fractions, frames_random), (field_fractions, frames_checker), (field_specials, frames_random),
                              (field_random, frames_black_white), (field_random, frames_checker), (field_small, frames_smooth)):
            out.append(_make(seed, size, field, frames))
            seed += 1
    out.append(_make(seed, (100, 62, 2), field_small, frames_smooth))
    out.append(_make(seed + 1, (100, 62, 2), field_fractions, frames_checker))
    out.append(_make(seed + 2, (6, 3, 2), field_zero, frames_black_white))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
