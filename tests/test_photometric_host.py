"""The photometric check without a GPU: the exports and the constants, the host-only check of the arguments, the proof that
the reference of tests/photometric_cases.py is the definition (an independent per-pixel loop in Python integers) and that the
case table reaches what it is meant to reach, quantise and the ValueErrors of the Python layer, and the command line's rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libofc.so is loaded, as in test_consistency_host.py)

from tests import photometric_cases as PC

EXPORTS = ("ofc_photo_check", "ofc_photo_dev", "ofc_photo", "ofc_bench_photo", "ofc_stream_set_photo", "ofc_stream_read_photo")


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _K():
    from opticalflowclustering_amd import photometric
    return photometric


def test_the_new_exports_exist_and_the_constants_agree():
    import opticalflowclustering_amd as pkg
    L, K = _L(), _K()
    assert pkg.photometric is K
    lib = C.CDLL(L.LIB_PATH)
    missing = [n for n in EXPORTS if not hasattr(lib, n)]
    assert not missing, missing
    assert set(EXPORTS) <= set(L.EXPORTS)
    header = open(os.path.join(PC.ROOT, "include", "ofc.h")).read()
    assert all(f"int {n}(" in header for n in EXPORTS)
    define = {k: int(v) for k, v in re.findall(r"#define (OFC_PHOTO_\w+) (\d+)", header)}
    assert define == {"OFC_PHOTO_SHARE": 2048, "OFC_PHOTO_TAU_MAX": 65280, "OFC_PHOTO_KAPPA_MAX": 1024, "OFC_PHOTO_NSTAT": 5}
    assert (L.PHOTO_SHARE, L.PHOTO_TAU_MAX, L.PHOTO_KAPPA_MAX, L.PHOTO_NSTAT) == (PC.SHARE, PC.TAU_MAX, PC.KAPPA_MAX, PC.NSTAT)
    assert (K.CONSISTENT, K.MISMATCH, K.LEAVES, K.INVALID, K.NSTATE, K.NSTAT) == (PC.OK, PC.MISMATCH, PC.LEAVES, PC.INVALID, 4, 5)
    assert K.quantise() == (PC.TAU_Q, PC.KAPPA_Q) == (2048, 128) and (K.TAU, K.KAPPA) == (8.0, 0.5)
    assert header.count("No counterpart in the reference") >= header.count("ofc_photo") // 2       # every call of the block says so


def test_photo_check_accepts_every_case_and_refuses_exactly_the_limits():
    L = _L()
    check = L.load().ofc_photo_check
    for c in PC.CASES:
        n, H, W = c.shape
        for tau_q, kappa_q in c.thresholds():
            assert check(W, H, n, tau_q, kappa_q) == L.OFC_OK, (c, tau_q, kappa_q)
    ok = (64, 48, 3, 2048, 128)

    def with_(**kw):
        names = ("W", "H", "npair", "tau_q", "kappa_q")
        return check(*[kw.get(n, v) for n, v in zip(names, ok)])

    assert with_() == L.OFC_OK and with_(W=1, H=1) == L.OFC_OK and with_(W=16384, H=16384) == L.OFC_OK
    assert with_(W=16385) == L.OFC_EUNSUPPORTED and "16384" in L.load().ofc_last_error().decode()
    assert with_(H=16385) == L.OFC_EUNSUPPORTED
    assert with_(W=0) == L.OFC_EINVAL and with_(H=0) == L.OFC_EINVAL
    assert with_(npair=1) == L.OFC_OK and with_(npair=65535) == L.OFC_OK
    assert with_(npair=0) == L.OFC_EINVAL and with_(npair=65536) == L.OFC_EINVAL
    assert with_(tau_q=0) == L.OFC_OK and with_(tau_q=65280) == L.OFC_OK
    assert with_(tau_q=-1) == L.OFC_EINVAL and with_(tau_q=65281) == L.OFC_EINVAL and "tau_q" in L.load().ofc_last_error().decode()
    assert with_(kappa_q=0) == L.OFC_OK and with_(kappa_q=1024) == L.OFC_OK
    assert with_(kappa_q=-1) == L.OFC_EINVAL and with_(kappa_q=1025) == L.OFC_EINVAL
    assert "kappa_q" in L.load().ofc_last_error().decode()
    K = _K()
    K.check_args(64, 48, 3)
    with pytest.raises(ValueError, match="npair"):
        K.check_args(64, 48, 0)
    with pytest.raises(L.OfcError):
        K.check_args(16385, 48, 3)


# ---- the reference is the definition ----
@pytest.mark.parametrize("case", PC.CASES, ids=repr)
def test_reference_equals_an_independent_per_pixel_loop(case):
    n, H, W = case.shape
    for tau_q, kappa_q in case.thresholds():
        state, stats, warped = case.reference(tau_q, kappa_q)
        assert state.shape == (n, H, W) and state.dtype == np.uint8 and stats.shape == (n, 5) and stats.dtype == np.int64
        assert warped.shape == (n, H, W) and warped.dtype == np.uint16
        ls, lt, lw, smax = PC.loop(case.frames, case.fwd, tau_q, kappa_q)
        assert np.array_equal(state, ls) and np.array_equal(stats, lt) and np.array_equal(warped, lw)
        assert smax <= 255 * 2 ** 32 < 2 ** 40 and (stats[:, 4] < 2 ** 44).all() and (stats[:, 4] <= 65280 * H * W).all()
        assert (stats[:, :4].sum(1) == H * W).all() and not warped[state >= PC.LEAVES].any()
    free = PC.reference(case.frames, case.fwd)                                    # the free function is the cached one
    assert all(np.array_equal(a, b) for a, b in zip(free, case.reference()))


def test_the_case_table_has_the_sizes_and_reaches_every_state_and_both_verdicts_at_equality():
    assert {(c.shape[2], c.shape[1], c.shape[0]) for c in PC.CASES} == set(PC.SIZES)
    assert PC.SIZES == ((1, 1, 1), (1, 7, 2), (7, 1, 3), (5, 3, 3), (6, 3, 2), (64, 32, 1), (64, 32, 3), (89, 23, 2), (683, 3, 2),
                        (100, 62, 2))
    assert 64 * 32 == PC.SHARE and 89 * 23 == PC.SHARE - 1 and 683 * 3 == PC.SHARE + 1 and 100 * 62 == 3 * PC.SHARE + 56
    reached = np.zeros(4, np.int64)
    for c in PC.CASES:
        reached += c.reference()[1][:, :4].sum(0)
    assert (reached > 0).all(), reached
    pairs = 0
    for c in PC.CASES:
        ch = c.chosen()
        thr = c.thresholds()
        assert thr[:4] == ((0, 0), (2048, 128), (65280, 0), (0, 1024)) and len(thr) == (6 if ch else 4)
        if ch:
            at, e = ch
            assert 1 <= e <= 65280 and thr[4:] == ((e, 0), (e - 1, 0))
            assert c.reference(e, 0)[0][at] == PC.OK and c.reference(e - 1, 0)[0][at] == PC.MISMATCH    # equality passes, one less fails
            pairs += 1
    assert pairs >= len(PC.CASES) - 6                                                     # all but constant frames and the like
    # the random cases of every size hold compared pixels on both sides of the default thresholds
    for size in PC.SIZES[3:]:
        stats = PC.BY_NAME["mixed-random-%dx%d-n%d" % size].reference()[1]
        assert (stats[:, :2].sum(0) > 0).all() and stats[:, 2].min() > 0, (size, stats)
    assert PC.BY_NAME["mixed-random-683x3-n2"].reference()[1][:, 3].min() > 0


def test_the_extremes_are_reached():
    c = PC.BY_NAME["zero-black_white-6x3-n2"]
    state, stats, warped = c.reference(65279, 0)
    assert (state == PC.MISMATCH).all() and stats[:, 4].tolist() == [65280 * 18] * 2                # |e| = 65280, both signs
    assert warped[0].min() == 65280 and warped[1].max() == 0
    assert (c.reference(65280, 0)[0] == PC.OK).all()
    c = PC.BY_NAME["fractions-checker-64x32-n3"]
    cmax = max(int(core[4][core[0] & core[1]].max()) for core in c.core())
    assert cmax == 255
    state_k, state_0 = c.reference(0, 1024)[0], c.reference(0, 0)[0]
    assert ((state_k == PC.OK) & (state_0 == PC.MISMATCH)).any()                                    # kappa alone forgives
    c = PC.BY_NAME["zero-constant-64x32-n3"]
    assert c.chosen() is None and (c.reference(0, 0)[0] == PC.OK).all() and not c.reference(0, 0)[1][:, 4].any()
    # a whole-pixel translation reads one pixel exactly: J = 256 * I1 there
    c = PC.BY_NAME["whole-random-64x32-n3"]
    state, _, warped = c.reference()
    assert np.array_equal(warped[0][:, :-1], 256 * c.frames[1][:, 1:].astype(np.uint16)) and (state[0][:, -1] == PC.LEAVES).all()


def test_the_fractions_the_edges_and_the_specials_are_what_they_are_named_for():
    c = PC.BY_NAME["fractions-random-64x32-n3"]
    q = np.rint(c.fwd.astype(np.float64) * 65536).astype(np.int64) & 65535
    assert {(int(a), int(b)) for a, b in q.reshape(-1, 2)} == {(a, b) for a in PC.FRACS for b in PC.FRACS}
    for size in [s for s in PC.SIZES if s[0] <= 128]:
        c = PC.BY_NAME["edges-random-%dx%d-n%d" % size]
        W, H, n = size
        state = c.reference()[0]
        k = np.arange(n * H * W).reshape(n, H, W) % 8
        assert (state[(k == 1) | (k == 3) | (k == 5) | (k == 7)] == PC.LEAVES).all()               # one quantum past
        q = np.rint(c.fwd.astype(np.float64) * 65536).astype(np.int64)
        yy, xx = np.mgrid[0:H, 0:W]
        X, Y = xx * 65536 + q[..., 0], yy * 65536 + q[..., 1]
        assert (X[k == 0] == (W - 1) << 16).all() and (X[k == 1] == ((W - 1) << 16) + 1).all() and (X[k == 3] == -1).all()
        assert (Y[k == 4] == (H - 1) << 16).all() and (Y[k == 5] == ((H - 1) << 16) + 1).all() and (Y[k == 7] == -1).all()
        on_edge = (k == 0) | (k == 2)
        assert ((state[on_edge] <= PC.MISMATCH) | (Y[on_edge] > (H - 1) << 16)).all()               # exactly on it: inside
    seen = set()
    for name in ("specials-random-5x3-n3", "specials-random-64x32-n3", "specials-random-683x3-n2"):
        f = PC.BY_NAME[name].fwd.reshape(-1, 2)
        for j, s in enumerate(PC.SPECIALS):
            for comp in (0, 1):
                col = f[:, comp]
                if (np.isnan(col).any() if s != s else (col == np.float32(s)).any()):
                    seen.add((j, comp))
        state = PC.BY_NAME[name].reference()[0]
        bad = ~(np.isfinite(PC.BY_NAME[name].fwd).all(-1) & (np.abs(PC.BY_NAME[name].fwd) < 1024).all(-1))
        assert np.array_equal(state == PC.INVALID, bad) and bad.any() and not bad.all()
    assert seen == {(j, comp) for j in range(len(PC.SPECIALS)) for comp in (0, 1)}


# ---- the Python layer ----
def test_quantise_and_the_value_errors():
    K = _K()
    assert K.quantise(0.0, 0.0) == (0, 0) and K.quantise(255.0, 4.0) == (65280, 1024) and K.quantise(8.0, 0.5) == (2048, 128)
    assert K.quantise(K.TAU, K.KAPPA) == K.quantise()
    tau_q, kappa_q = K.quantise()
    assert (tau_q / 256.0, kappa_q / 256.0) == (K.TAU, K.KAPPA)                                  # the defaults round-trip
    for bad in ((-0.01, 0.5), (255.01, 0.5), (8.0, -0.01), (8.0, 4.01), (float("nan"), 0.5), (8.0, float("inf"))):
        with pytest.raises(ValueError):
            K.quantise(*bad)
    f = np.zeros((4, 5, 2), np.float32)
    with pytest.raises(ValueError, match="frames should be"):
        K.check(np.zeros((3, 4, 5), np.uint8), f)
    with pytest.raises(ValueError, match="frames should be"):
        K.check(np.zeros((2, 5, 4), np.uint8), f)
    with pytest.raises(ValueError, match="should be"):
        K.check(np.zeros((2, 4, 5), np.uint8), np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="tau"):
        K.check(np.zeros((2, 4, 5), np.uint8), f, tau=300.0)
    stats = np.array([[6, 2, 1, 1, 8 * 256 * 3], [0, 0, 10, 0, 0]], np.int64)
    p = K.Photometric(None, stats, None, 2048, 128)
    assert len(p) == 2 and p.warped is None and p.counts.tolist() == [[6, 2, 1, 1], [0, 0, 10, 0]]
    assert p.abs_error.tolist() == [6144, 0] and p.abs_error.dtype == np.int64
    m = p.mean_abs_error()
    assert m[0] == 3.0 and np.isnan(m[1]) and np.allclose(p.share(), [[0.6, 0.2, 0.1, 0.1], [0, 0, 1, 0]])
    for doc in (K.check.__doc__, K.quantise.__doc__, K.check_dev.__doc__):
        assert "not tuned" in doc and "convention" in doc
    from opticalflowclustering_amd.pipeline import ClipPipeline
    from opticalflowclustering_amd.stream import FlowStream
    assert "not tuned" in ClipPipeline.photometric.__doc__ and "not tuned" in FlowStream.set_photometric.__doc__


def test_motion_grids_photometric_arguments():
    from opticalflowclustering_amd import motionGrids as G
    base = ["--path", "clip.npy", "-c", "3", "-f", "out.csv"]
    a = G.parse_arguments(base)
    assert not a.photometric and a.photo_counts is None and (a.photo_tau, a.photo_kappa) == (8.0, 0.5) and a.photo_spec is None
    a = G.parse_arguments(base + ["--photometric", "--photo-tau", "4", "--photo-kappa", "1", "--photo-counts", "n.npy"])
    assert a.photometric and a.photo_spec == dict(tau=4.0, kappa=1.0) and a.photo_counts == "n.npy"
    a = G.parse_arguments(base + ["--photometric", "--stream", "--model", "m.npy", "--blobs", "b.csv"])
    assert a.photometric and a.stream
    a = G.parse_arguments(base + ["--photometric", "--fit-stream", "--camera", "affine"])
    assert a.photometric and a.fit_stream
    for bad in (["--photometric", "--consistent"], ["--photo-counts", "n.npy"], ["--photo-tau", "4"], ["--photo-kappa", "1"],
                ["--photometric", "--photo-tau", "300"], ["--photometric", "--photo-kappa", "-1"],
                ["--photometric", "--photo-tau", "nan"],
                # --consistent keeps its refusals
                ["--consistent", "--stream", "--model", "m.npy"], ["--consistent", "--fit-stream"], ["--fb-counts", "n.npy"]):
        with pytest.raises(SystemExit):
            G.parse_arguments(base + bad)
