"""The forward-backward check of include/ofc.h twice over -- a vectorised numpy reference and an independent per-pixel loop
in plain Python integers -- and the table of cases that test_consistency_host.py proves on the CPU and
test_gpu_consistency.py runs on the device."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, MISMATCH, LEAVES, INVALID, NSTATE = 0, 1, 2, 3, 4
SHARE = 2048                      # OFC_CONSIST_SHARE: the pixels of a pair a work-group takes
ONE = 65536
ALPHA_Q, BETA_Q = 655, 1 << 31     # what alpha 0.01 and beta 0.5 quantise to
Q = 1.0 / ONE                     # one quantum in px
ALMOST = float(np.float32(1023.99994))
SPECIALS = (float("nan"), float("inf"), float("-inf"), 1024.0, -1024.0, ALMOST)


# ---- the reference: numpy, whole fields at a time ----
def quantise_field(f):
    """(...,2) f32 -> valid (...) bool, q (...,2) int64 (0 where invalid)"""
    f = np.asarray(f, np.float32)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(f).all(-1) & (np.abs(f) < np.float32(1024)).all(-1)
        q = np.rint(np.where(valid[..., None], f, np.float32(0)).astype(np.float64) * 65536.0).astype(np.int64)
    return valid, q


def reference_pair(fwd, bwd, alpha_q, beta_q):
    """one pair: (H,W,2) f32 twice -> state (H,W) u8, resid (H,W,2) int32"""
    H, W = fwd.shape[:2]
    vf, qf = quantise_field(fwd)
    vb, qb = quantise_field(bwd)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    X, Y = xx * ONE + qf[..., 0], yy * ONE + qf[..., 1]
    inside = (X >= 0) & (X <= (W - 1) << 16) & (Y >= 0) & (Y <= (H - 1) << 16)
    ix, iy = np.clip(X >> 16, 0, W - 1), np.clip(Y >> 16, 0, H - 1)
    fx, fy = X & 65535, Y & 65535
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    taps = ((ix, iy, (ONE - fx) * (ONE - fy)), (ix1, iy, fx * (ONE - fy)), (ix, iy1, (ONE - fx) * fy), (ix1, iy1, fx * fy))
    S, taps_valid = np.zeros((H, W, 2), np.int64), np.ones((H, W), bool)
    for tx, ty, w in taps:
        S += w[..., None] * qb[ty, tx]
        taps_valid &= vb[ty, tx]
    B = (S + (1 << 31)) >> 32
    e = qf + B
    d2 = (e * e).sum(-1)
    m2 = (qf * qf).sum(-1) + (B * B).sum(-1)
    good = d2 <= (m2 >> 16) * np.int64(alpha_q) + np.int64(beta_q)
    state = np.where(~vf, INVALID, np.where(~inside, LEAVES, np.where(~taps_valid, INVALID, np.where(good, OK, MISMATCH))))
    resid = np.where((state <= MISMATCH)[..., None], e, 0)
    return state.astype(np.uint8), resid.astype(np.int32)


def reference(fwd, bwd, alpha_q=ALPHA_Q, beta_q=BETA_Q, bwd_reversed=False):
    """(n,H,W,2) f32 twice -> state (n,H,W) u8, counts (n,4) int64, resid (n,H,W,2) int32"""
    n = len(fwd)
    out = [reference_pair(fwd[t], bwd[n - 1 - t] if bwd_reversed else bwd[t], alpha_q, beta_q) for t in range(n)]
    state, resid = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    counts = np.stack([np.bincount(s.ravel(), minlength=NSTATE) for s in state]).astype(np.int64)
    return state, counts, resid


# ---- the same definition as a loop over the pixels in Python integers.  Shares nothing with the numpy above. ----
def _q(u):
    """llrint((double)u * 65536) of a valid f32, or None"""
    u = float(u)
    if not math.isfinite(u) or not abs(u) < 1024.0:
        return None
    return int(round(u * 65536.0))              # exact product; round() goes to even on ties, as llrint does


def _qvec(vec):
    a, b = _q(vec[0]), _q(vec[1])
    return None if a is None or b is None else (a, b)


def loop_pair(fwd, bwd, alpha_q, beta_q):
    H, W = fwd.shape[:2]
    f, b = fwd.tolist(), bwd.tolist()
    state = [[0] * W for _ in range(H)]
    resid = [[(0, 0)] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            q = _qvec(f[y][x])
            if q is None:
                state[y][x] = INVALID
                continue
            X, Y = x * 65536 + q[0], y * 65536 + q[1]
            if not (0 <= X <= (W - 1) * 65536 and 0 <= Y <= (H - 1) * 65536):
                state[y][x] = LEAVES
                continue
            ix, fx, iy, fy = X // 65536, X % 65536, Y // 65536, Y % 65536
            ix1, iy1 = min(ix + 1, W - 1), min(iy + 1, H - 1)
            taps = [_qvec(b[iy][ix]), _qvec(b[iy][ix1]), _qvec(b[iy1][ix]), _qvec(b[iy1][ix1])]
            if any(t is None for t in taps):
                state[y][x] = INVALID
                continue
            wts = [(65536 - fx) * (65536 - fy), fx * (65536 - fy), (65536 - fx) * fy, fx * fy]
            B = [(sum(w * t[c] for w, t in zip(wts, taps)) + 2 ** 31) // 2 ** 32 for c in (0, 1)]     # floor division: the arithmetic shift
            e = (q[0] + B[0], q[1] + B[1])
            d2 = e[0] ** 2 + e[1] ** 2
            m2 = q[0] ** 2 + q[1] ** 2 + B[0] ** 2 + B[1] ** 2
            assert abs(sum(w * t[0] for w, t in zip(wts, taps))) <= 2 ** 58 and (m2 // 65536) * alpha_q + beta_q < 2 ** 63
            state[y][x] = OK if d2 <= (m2 // 65536) * alpha_q + beta_q else MISMATCH
            resid[y][x] = e
    return np.array(state, np.uint8), np.array(resid, np.int32).reshape(H, W, 2)


def loop(fwd, bwd, alpha_q=ALPHA_Q, beta_q=BETA_Q, bwd_reversed=False):
    n = len(fwd)
    out = [loop_pair(fwd[t], bwd[n - 1 - t] if bwd_reversed else bwd[t], alpha_q, beta_q) for t in range(n)]
    state = np.stack([o[0] for o in out])
    counts = np.array([[int((s == k).sum()) for k in range(NSTATE)] for s in state], np.int64)
    return state, counts, np.stack([o[1] for o in out])


# ---- the cases ----
class Case:
    def __init__(self, name, fwd, bwd, alpha_q=ALPHA_Q, beta_q=BETA_Q, bwd_reversed=False, marks=None):
        self.name, self.alpha_q, self.beta_q, self.bwd_reversed = name, alpha_q, beta_q, bwd_reversed
        self.fwd, self.bwd = np.ascontiguousarray(fwd, np.float32), np.ascontiguousarray(bwd, np.float32)
        assert self.fwd.shape == self.bwd.shape and self.fwd.ndim == 4 and self.fwd.shape[3] == 2
        self.marks = marks or {}                  # named pixels (pair, y, x) the host test asks about
        self._ref = None

    def __repr__(self):
        return self.name

    @property
    def shape(self):
        return self.fwd.shape[:3]

    def reference(self):
        if self._ref is None:                     # computed once, shared, never written
            self._ref = reference(self.fwd, self.bwd, self.alpha_q, self.beta_q, self.bwd_reversed)
            for a in self._ref:
                a.setflags(write=False)
        return self._ref


def smooth_fields(seed, n, H, W, specials=True):
    """per pair its own translation plus a slow wave plus noise; the backward field is the negation of the forward one on
    its own grid, to the size of the wave, plus noise, with patches of other motion and, with specials, some unusable values"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    fwd, bwd = np.empty((n, H, W, 2)), np.empty((n, H, W, 2))
    for t in range(n):
        base = r.uniform(-2.0, 2.0, 2) * (1.0 if min(H, W) > 2 else 0.3)
        wave = 0.4 * np.stack([np.sin(xx / 9.0 + t) * np.cos(yy / 7.0), np.cos(xx / 11.0 - t) * np.sin(yy / 5.0 + 1.0)], -1)
        fwd[t] = base + wave + r.normal(0, 0.02, (H, W, 2))
        bwd[t] = -(base + wave) + r.normal(0, 0.05, (H, W, 2))
        rough = r.random((H, W)) < 0.08
        bwd[t][rough] += r.normal(0, 1.5, (int(rough.sum()), 2))
    fwd, bwd = fwd.astype(np.float32), bwd.astype(np.float32)
    if specials:
        for field in (fwd, bwd):
            flat = field.reshape(-1, 2)
            where = r.choice(len(flat), max(1, len(flat) // 40), replace=False)
            flat[where, r.integers(0, 2, len(where))] = np.array(SPECIALS, np.float32)[r.integers(0, len(SPECIALS), len(where))]
    return fwd, bwd


def _size_cases():
    out, k = [], 0
    for W in (1, 2, 3, 63, 64, 65, 257):
        for H in (1, 2, 17):
            n = (1, 2, 3)[k % 3]
            fwd, bwd = smooth_fields(100 + k, n, H, W)
            rev = bool(k // 3 % 2)                                 # a reversed case holds its backward fields in that order
            out.append(Case(f"size-{W}x{H}-n{n}-rev{int(rev)}", fwd, bwd[::-1] if rev else bwd, bwd_reversed=rev))
            k += 1
    for W, H in ((89, 23), (64, 32), (683, 3)):             # the share minus one, the share, the share plus one
        for rev in (0, 1):
            fwd, bwd = smooth_fields(200 + W + rev, 3, H, W)
            out.append(Case(f"share-{W}x{H}-n3-rev{rev}", fwd, bwd[::-1] if rev else bwd, bwd_reversed=bool(rev)))
    return out


EDGE_W, EDGE_H = 12, 10
FRACS = (0, 1, 32768, 65535)


def _edge_case():
    """pair 0: pixels that land exactly on the last column / row, one quantum past it, exactly on 0, one quantum before it;
    pair 1: every combination of the fractions FRACS in x and y.  The backward field varies from pixel to pixel, so every
    weight matters."""
    W, H = EDGE_W, EDGE_H
    r = np.random.default_rng(7)
    fwd = np.zeros((2, H, W, 2), np.float32)
    bwd = r.uniform(-0.6, 0.6, (2, H, W, 2)).astype(np.float32)
    marks = {}
    x, y = 3, 4
    for name, to in (("last-col", lambda x, y: (W - 1 - x, 0.0)), ("past-last-col", lambda x, y: (W - 1 - x + Q, 0.0)),
                     ("col-0", lambda x, y: (-x, 0.0)), ("before-col-0", lambda x, y: (-x - Q, 0.0)),
                     ("last-row", lambda x, y: (0.0, H - 1 - y)), ("past-last-row", lambda x, y: (0.0, H - 1 - y + Q)),
                     ("row-0", lambda x, y: (0.0, -y)), ("before-row-0", lambda x, y: (0.0, -y - Q)),
                     ("corner", lambda x, y: (W - 1 - x, H - 1 - y)), ("past-corner", lambda x, y: (W - 1 - x + Q, H - 1 - y))):
        u, v = to(x, y)
        fwd[0, y, x] = (u, v)
        assert float(fwd[0, y, x, 0]) == u and float(fwd[0, y, x, 1]) == v           # representable: the quantum is not lost
        marks[name] = (0, y, x)
        x, y = (x + 1, y) if x < 7 else (3, y + 1)
    k = 0
    for fx in FRACS:
        for fy in FRACS:
            y, x = 1 + k // 4 * 2, 1 + k % 4 * 2
            fwd[1, y, x] = (1 + fx * Q, -1 + fy * Q)
            marks[f"frac-{fx}-{fy}"] = (1, y, x)
            k += 1
    return Case("landing-edges-12x10", fwd, bwd, marks=marks)


VALID_W, VALID_H = 40, 13


def _validity_case():
    """pair 0: every special value in u and in v of the forward field, over a backward field that is clean.  Pairs 1 and 2:
    a clean forward field, (0.5, 0.5) and (0, 0), and every special value in u and in v of one backward pixel each, far
    enough apart that the four pixels that have it as their tap 0, 1, 2 and 3 are told apart.  Pair 0 also has a pixel
    that leaves the frame over an unusable corner of the backward field: it is LEAVES, the taps are never looked at."""
    W, H = VALID_W, VALID_H
    fwd, bwd = np.zeros((3, H, W, 2), np.float32), np.zeros((3, H, W, 2), np.float32)
    fwd[1], bwd[1] = 0.5, -0.5
    marks = {}
    for j, s in enumerate(SPECIALS):
        for c in (0, 1):
            x, y = 2 + 3 * (2 * j + c), 3
            fwd[0, y, x, c] = s
            marks[f"fwd-{j}-{c}"] = (0, y, x)
            for pair in (1, 2):
                bwd[pair, y * 2, x, c] = s
                marks[f"tap-{pair}-{j}-{c}"] = (pair, y * 2, x)
    bwd[0, 0, 0] = np.nan
    fwd[0, 0, 0] = (-0.25, 0.0)
    marks["leaves-over-nan"] = (0, 0, 0)
    fwd[0, H - 1, W - 1] = (np.nan, 5.0)                    # invalid and it would leave: invalid comes first
    marks["invalid-and-leaving"] = (0, H - 1, W - 1)
    return Case("validity-40x13", fwd, bwd, marks=marks)


def _threshold_cases():
    W, H = 5, 4
    const = lambda u, v: np.broadcast_to(np.array([u, v], np.float32), (1, H, W, 2))       # noqa: E731
    e2 = 16384 ** 2                                         # f = (1, 0), b = (-0.75, 0): e = (0.25 px, 0), d2 = 2^28
    out = [Case("threshold-beta-equal", const(1, 0), const(-0.75, 0), 0, e2),
           Case("threshold-beta-one-short", const(1, 0), const(-0.75, 0), 0, e2 - 1),
           # f and b at right angles: d2 = m2; with alpha 1 and m2 a multiple of 65536 the two sides are equal
           Case("threshold-alpha-equal", const(1, 0), const(0, 1), 65536, 0),
           # ... and with Q(b) = 65537, m2 = 2^33 + 2^17 + 1 loses its last bit to the shift: d2 = thr + 1
           Case("threshold-alpha-one-short", const(1, 0), const(0, 1 + Q), 65536, 0),
           Case("threshold-all-zero-exact", const(1, 0.5), const(-1, -0.5), 0, 0),
           Case("threshold-all-zero-one-quantum", const(1, 0.5), const(-1, -0.5 + Q), 0, 0)]
    # both fields near +-1024 on a frame wide enough to land inside: the largest d2 and m2 there are
    Wb, Hb = 1100, 2
    fwd, bwd = np.zeros((1, Hb, Wb, 2), np.float32), np.empty((1, Hb, Wb, 2), np.float32)
    fwd[0, :, :70, 0] = ALMOST
    fwd[0, :, 1030:, 0] = -ALMOST
    bwd[0, :, :550], bwd[0, :, 550:] = (-ALMOST, -ALMOST), (ALMOST, ALMOST)
    out.append(Case("threshold-near-1024-alpha1-beta-max", fwd, bwd, 65536, 1 << 62))
    out.append(Case("threshold-near-1024-alpha1-beta0", fwd, bwd, 65536, 0))
    out.append(Case("threshold-near-1024-alpha0-beta0", fwd, bwd, 0, 0))
    return out


TRANS_W, TRANS_H, TRANS = 53, 37, (3.25, -1.5)
RECT = (20, 10, 9, 6)             # x, y, w, h of the patch of other motion in the backward field


def _meaning_cases():
    W, H = TRANS_W, TRANS_H
    fwd = np.broadcast_to(np.array(TRANS, np.float32), (1, H, W, 2)).copy()
    bwd = -fwd
    other = bwd.copy()
    x, y, w, h = RECT
    other[0, y:y + h, x:x + w] = (20.0, -15.0)             # far enough off that the smallest weight, 1/8, shows
    return [Case("translation-53x37", fwd, bwd), Case("translation-53x37-alpha0-beta0", fwd, bwd, 0, 0),
            Case("rectangle-53x37", fwd, other)]


def _random_cases():
    fwd, bwd = smooth_fields(5, 3, 50, 200)
    clean = smooth_fields(6, 2, 40, 129, specials=False)
    return [Case("random-200x50-n3", fwd, bwd), Case("random-200x50-n3-rev", fwd, bwd, bwd_reversed=True),
            Case("random-clean-129x40-n2", *clean)]


CASES = _size_cases() + [_edge_case(), _validity_case()] + _threshold_cases() + _meaning_cases() + _random_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
