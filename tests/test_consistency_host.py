"""The forward-backward check without a GPU: the exports and the constants, the host-only check of the arguments, the proof
that the reference of tests/consistency_cases.py is the definition (an independent per-pixel loop in Python integers) and
that every case has the property it is named for, quantise and the ValueErrors of the Python layer, and the command line's
rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libofc.so is loaded, as in test_blobs_host.py)

from tests import consistency_cases as CC

EXPORTS = ("ofc_consist_check", "ofc_consist_dev", "ofc_consist", "ofc_consist_mask_dev", "ofc_frames_reverse_dev",
           "ofc_bench_consist")


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _K():
    from opticalflowclustering_amd import consistency
    return consistency


def test_the_new_exports_exist_and_the_constants_agree():
    L, K = _L(), _K()
    lib = C.CDLL(L.LIB_PATH)
    missing = [n for n in EXPORTS if not hasattr(lib, n)]
    assert not missing, missing
    assert set(EXPORTS) <= set(L.EXPORTS)
    header = open(os.path.join(CC.ROOT, "include", "ofc.h")).read()
    assert all(f"int {n}(" in header for n in EXPORTS)
    define = dict(re.findall(r"#define (OFC_CONSIST_\w+) (\S+)", header))
    assert [int(define["OFC_CONSIST_" + n]) for n in ("OK", "MISMATCH", "LEAVES", "INVALID", "STATES")] == [0, 1, 2, 3, 4]
    assert (L.CONSIST_OK, L.CONSIST_MISMATCH, L.CONSIST_LEAVES, L.CONSIST_INVALID, L.CONSIST_STATES) == (0, 1, 2, 3, 4)
    assert (K.CONSISTENT, K.MISMATCH, K.LEAVES, K.INVALID, K.NSTATE) == (CC.OK, CC.MISMATCH, CC.LEAVES, CC.INVALID, CC.NSTATE)
    assert len(K.STATE_NAMES) == K.NSTATE
    assert int(define["OFC_CONSIST_SHARE"]) == L.CONSIST_SHARE == CC.SHARE                  # the share the cases aim at
    assert int(define["OFC_CONSIST_MAX_DIM"]) == L.CONSIST_MAX_DIM == 16384
    assert int(define["OFC_CONSIST_ALPHA_MAX"]) == L.CONSIST_ALPHA_MAX == 65536 and L.CONSIST_BETA_MAX == 2 ** 62
    assert "OFC_CONSIST_BETA_MAX ((int64_t)1 << 62)" in header
    assert K.quantise() == (CC.ALPHA_Q, CC.BETA_Q) == (655, 2 ** 31) and (K.ALPHA, K.BETA) == (0.01, 0.5)


def test_consist_check_accepts_and_refuses_exactly_the_domain():
    L = _L()
    check = L.load().ofc_consist_check
    ok = (64, 48, 3, 655, 2 ** 31)
    assert check(*ok) == L.OFC_OK

    def with_(**kw):
        names = ("W", "H", "npair", "alpha_q", "beta_q")
        return check(*[kw.get(n, v) for n, v in zip(names, ok)])

    assert with_(W=1, H=1) == L.OFC_OK and with_(W=16384) == L.OFC_OK and with_(H=16384) == L.OFC_OK
    assert with_(W=16384, H=16384) == L.OFC_OK
    assert with_(W=16385) == L.OFC_EUNSUPPORTED and "16384" in L.load().ofc_last_error().decode()
    assert with_(H=16385) == L.OFC_EUNSUPPORTED and with_(W=2 ** 31 - 1) == L.OFC_EUNSUPPORTED
    assert with_(W=0) == L.OFC_EINVAL and with_(H=0) == L.OFC_EINVAL and with_(W=-5) == L.OFC_EINVAL
    assert with_(npair=1) == L.OFC_OK and with_(npair=65535) == L.OFC_OK
    assert with_(npair=0) == L.OFC_EINVAL and with_(npair=65536) == L.OFC_EINVAL and with_(npair=-1) == L.OFC_EINVAL
    assert with_(alpha_q=0) == L.OFC_OK and with_(alpha_q=65536) == L.OFC_OK
    assert with_(alpha_q=-1) == L.OFC_EINVAL and with_(alpha_q=65537) == L.OFC_EINVAL
    assert with_(beta_q=0) == L.OFC_OK and with_(beta_q=2 ** 62) == L.OFC_OK
    assert with_(beta_q=-1) == L.OFC_EINVAL and with_(beta_q=2 ** 62 + 1) == L.OFC_EINVAL
    assert "beta_q" in L.load().ofc_last_error().decode()
    assert with_(alpha_q=2 ** 32) == L.OFC_EINVAL                                  # the argument is 64 bits wide: no wrap to 0
    K = _K()
    K.check_args(64, 48, 3)
    with pytest.raises(ValueError, match="npair"):
        K.check_args(64, 48, 0)
    with pytest.raises(L.OfcError):
        K.check_args(16385, 48, 3)


# ---- the reference is the definition ----
@pytest.mark.parametrize("case", CC.CASES, ids=repr)
def test_reference_equals_an_independent_per_pixel_loop(case):
    state, counts, resid = case.reference()
    n, H, W = case.shape
    assert state.shape == (n, H, W) and state.dtype == np.uint8 and counts.shape == (n, 4) and counts.dtype == np.int64
    assert resid.shape == (n, H, W, 2) and resid.dtype == np.int32
    ls, lc, lr = CC.loop(case.fwd, case.bwd, case.alpha_q, case.beta_q, case.bwd_reversed)
    assert np.array_equal(state, ls) and np.array_equal(counts, lc) and np.array_equal(resid, lr)
    assert (counts.sum(1) == H * W).all() and not resid[state >= CC.LEAVES].any()


def test_the_case_table_covers_the_sizes_the_pair_counts_and_both_orders():
    shapes = {(c.shape[2], c.shape[1]) for c in CC.CASES}
    assert {(W, H) for W in (1, 2, 3, 63, 64, 65, 257) for H in (1, 2, 17)} <= shapes
    assert {w * h for w, h in shapes} >= {CC.SHARE - 1, CC.SHARE, CC.SHARE + 1}
    assert max(w * h for w, h in shapes) == 200 * 50 and -(-200 * 50 // CC.SHARE) == 5     # several work-groups, the last short
    assert {c.shape[0] for c in CC.CASES} == {1, 2, 3}
    for n in (2, 3):                                                             # both orders, with distinct per-pair fields
        for rev in (False, True):
            some = [c for c in CC.CASES if c.shape[0] == n and c.bwd_reversed == rev]
            assert some
            for c in some:
                assert not np.array_equal(c.bwd[0], c.bwd[-1]) and not np.array_equal(c.fwd[0], c.fwd[-1])
    # with the wrong order the answer is another one: a wrong index shows
    c = CC.BY_NAME["random-200x50-n3-rev"]
    assert not np.array_equal(c.reference()[0], CC.BY_NAME["random-200x50-n3"].reference()[0])
    # the random cases hold every state, and both verdicts in numbers
    for name in ("random-200x50-n3", "share-64x32-n3-rev0", "share-683x3-n3-rev1", "size-257x17-n3-rev0", "size-65x17-n3-rev1"):
        counts = CC.BY_NAME[name].reference()[1]
        assert (counts.sum(0) > 0).all() and counts[:, CC.OK].min() > 50 and counts[:, CC.MISMATCH].min() > 20, (name, counts)
    assert CC.BY_NAME["random-clean-129x40-n2"].reference()[1][:, CC.INVALID].tolist() == [0, 0]


def at(case, name, what=0):
    return case.reference()[what][case.marks[name]]


def test_the_landing_edges_fall_on_the_side_the_definition_says():
    c = CC.BY_NAME["landing-edges-12x10"]
    for name in ("last-col", "col-0", "last-row", "row-0", "corner"):
        assert at(c, name) in (CC.OK, CC.MISMATCH), name
    for name in ("past-last-col", "before-col-0", "past-last-row", "before-row-0", "past-corner"):
        assert at(c, name) == CC.LEAVES, name
    _, q = CC.quantise_field(c.fwd)
    yy, xx = np.mgrid[0:CC.EDGE_H, 0:CC.EDGE_W]
    X, Y = xx * 65536 + q[..., 0], yy * 65536 + q[..., 1]
    pair, y, x = c.marks["past-last-col"]
    assert X[pair, y, x] == ((CC.EDGE_W - 1) << 16) + 1                           # by exactly one quantum
    pair, y, x = c.marks["before-row-0"]
    assert Y[pair, y, x] == -1
    pair, y, x = c.marks["corner"]
    assert (X[pair, y, x], Y[pair, y, x]) == ((CC.EDGE_W - 1) << 16, (CC.EDGE_H - 1) << 16)
    seen = set()
    for fx in CC.FRACS:
        for fy in CC.FRACS:
            pair, y, x = c.marks[f"frac-{fx}-{fy}"]
            assert (X[pair, y, x] & 65535, Y[pair, y, x] & 65535) == (fx, fy) and at(c, f"frac-{fx}-{fy}") <= CC.MISMATCH
            seen.add((fx, fy))
    assert len(seen) == 16


def test_the_validity_case_is_invalid_exactly_where_it_should_be():
    c = CC.BY_NAME["validity-40x13"]
    state = c.reference()[0]
    want = np.zeros_like(state, bool)
    for j, s in enumerate(CC.SPECIALS):
        bad = not (np.isfinite(s) and abs(s) < 1024)
        for comp in (0, 1):
            pair, y, x = c.marks[f"fwd-{j}-{comp}"]
            want[pair, y, x] = bad
            assert (state[pair, y, x] == CC.INVALID) == bad, (j, comp)
            for pair in (1, 2):                                                   # the pixels that have it as tap 0, 1, 2, 3
                _, y, x = c.marks[f"tap-{pair}-{j}-{comp}"]
                for dy, dx in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
                    want[pair, y + dy, x + dx] = bad
    assert sum(not (np.isfinite(s) and abs(s) < 1024) for s in CC.SPECIALS) == 5 and CC.ALMOST < 1024
    assert at(c, "leaves-over-nan") == CC.LEAVES and at(c, "invalid-and-leaving") == CC.INVALID
    want[c.marks["invalid-and-leaving"]] = True
    assert np.array_equal(state == CC.INVALID, want)
    assert (state[2] == CC.INVALID).sum() == 5 * 2 * 4                            # a tap of weight 0 must be valid all the same


def test_the_threshold_cases_sit_on_the_threshold():
    def inner(name):
        c = CC.BY_NAME[name]
        state, _, resid = c.reference()
        inside = state <= CC.MISMATCH
        assert inside.any() and len(set(state[inside].tolist())) == 1
        return c, int(state[inside][0]), resid[inside][0].astype(object)

    c, s, e = inner("threshold-beta-equal")
    assert s == CC.OK and c.alpha_q == 0 and e[0] ** 2 + e[1] ** 2 == c.beta_q                        # d2 == thr
    c, s, e = inner("threshold-beta-one-short")
    assert s == CC.MISMATCH and e[0] ** 2 + e[1] ** 2 == c.beta_q + 1                                 # d2 == thr + 1
    c, s, e = inner("threshold-alpha-equal")
    m2 = 2 * 65536 ** 2
    assert s == CC.OK and e[0] ** 2 + e[1] ** 2 == (m2 >> 16) * 65536 == m2
    c, s, e = inner("threshold-alpha-one-short")
    m2 = 65536 ** 2 + 65537 ** 2
    assert s == CC.MISMATCH and e[0] ** 2 + e[1] ** 2 == m2 == (m2 >> 16) * 65536 + 1
    assert inner("threshold-all-zero-exact")[1] == CC.OK and inner("threshold-all-zero-one-quantum")[1] == CC.MISMATCH
    assert inner("threshold-all-zero-one-quantum")[2].tolist() == [0, 1]
    big = CC.BY_NAME["threshold-near-1024-alpha1-beta-max"]
    state, counts, resid = big.reference()
    fast = np.abs(big.fwd[0, :, :, 0]) > 1023                                     # 2 * 140 pixels, all landing inside
    assert fast.sum() == 2 * 140 and (state[0][fast] == CC.OK).all() and counts[0].tolist() == [2200, 0, 0, 0]
    assert np.abs(resid[0][fast]).min(0).tolist() == [2 * (2 ** 26 - 4), 2 ** 26 - 4]
    assert (CC.BY_NAME["threshold-near-1024-alpha1-beta0"].reference()[0][0][fast] == CC.MISMATCH).all()       # same direction: d2 > m2
    d2 = (resid.astype(object) ** 2).sum(-1).max()
    assert 2 ** 54 < d2 < 2 ** 55                                                                       # the largest there is: it fits


def test_a_translation_and_its_negation_cancel_and_a_patch_of_other_motion_shows():
    W, H = CC.TRANS_W, CC.TRANS_H
    for name in ("translation-53x37", "translation-53x37-alpha0-beta0"):
        state, counts, resid = CC.BY_NAME[name].reference()
        assert not resid.any() and counts.tolist() == [[(W - 4) * (H - 2), 0, W * H - (W - 4) * (H - 2), 0]] == [[1715, 0, 246, 0]]
        assert (state[0, 2:, :W - 4] == CC.OK).all()                              # the band that leaves: right and top
    state, counts, _ = CC.BY_NAME["rectangle-53x37"].reference()
    x, y, w, h = CC.RECT
    touched = np.zeros((H, W), bool)
    _, q = CC.quantise_field(np.array(CC.TRANS, np.float32))
    for py in range(H):
        for px in range(W):
            X, Y = px * 65536 + int(q[0]), py * 65536 + int(q[1])
            if 0 <= X <= (W - 1) << 16 and 0 <= Y <= (H - 1) << 16:
                taps = {(min(X // 65536 + a, W - 1), min(Y // 65536 + b, H - 1)) for a in (0, 1) for b in (0, 1)}
                touched[py, px] = any(x <= tx < x + w and y <= ty < y + h for tx, ty in taps)
    assert touched.sum() == (w + 1) * (h + 1) and np.array_equal(state[0] == CC.MISMATCH, touched)
    assert counts[0, CC.OK] == 1715 - touched.sum()


# ---- the Python layer ----
def test_quantise_and_the_value_errors():
    K = _K()
    assert K.quantise(0.0, 0.0) == (0, 0) and K.quantise(1.0, 2.0 ** 30) == (65536, 2 ** 62)
    assert K.quantise(0.5, 1.0) == (32768, 2 ** 32)
    for bad in ((-0.001, 0.5), (1.001, 0.5), (0.01, -0.1), (0.01, 2.0 ** 30 + 1), (float("nan"), 0.5), (0.01, float("inf"))):
        with pytest.raises(ValueError):
            K.quantise(*bad)
    assert K.keep_mask(()) == 0 and K.keep_mask((K.CONSISTENT,)) == 1 and K.keep_mask((0, 1, 2, 3)) == 15
    with pytest.raises(ValueError):
        K.keep_mask((4,))
    f = np.zeros((4, 5, 2), np.float32)
    with pytest.raises(ValueError, match="does not match"):
        K.check(f, np.zeros((5, 4, 2), np.float32))
    with pytest.raises(ValueError, match="should be"):
        K.check(np.zeros((4, 5), np.float32), f)
    with pytest.raises(ValueError, match="alpha"):
        K.check(f, f, alpha=2.0)
    counts = np.array([[6, 2, 1, 1], [10, 0, 0, 0]], np.int64)
    c = K.Consistency(np.zeros((2, 2, 5), np.uint8), counts, None, 655, 2 ** 31)
    assert c.residual is None and len(c) == 2 and np.allclose(c.share(), [[0.6, 0.2, 0.1, 0.1], [1, 0, 0, 0]])
    c = K.Consistency(None, counts, np.array([[[[65536, -32768]]]], np.int32), 655, 2 ** 31)
    assert c.residual.dtype == np.float64 and c.residual.tolist() == [[[[1.0, -0.5]]]]
    assert "not tuned" in K.check.__doc__ and "literature" in K.check.__doc__


def test_motion_grids_consistent_arguments():
    from opticalflowclustering_amd import motionGrids as G
    base = ["--path", "clip.npy", "-c", "3", "-f", "out.csv"]
    a = G.parse_arguments(base)
    assert not a.consistent and a.fb_counts is None and (a.fb_alpha, a.fb_beta) == (0.01, 0.5)
    a = G.parse_arguments(base + ["--consistent", "--fb-alpha", "0.02", "--fb-beta", "1", "--fb-counts", "n.npy"])
    assert a.consistent and (a.fb_alpha, a.fb_beta, a.fb_counts) == (0.02, 1.0, "n.npy")
    a = G.parse_arguments(base + ["--consistent", "--blobs", "b.csv", "--tracks", "--camera", "affine", "--weights", "moving:0.5"])
    assert a.consistent and a.tracks
    for bad in (["--consistent", "--stream", "--model", "m.npy"], ["--consistent", "--fit-stream"], ["--fb-counts", "n.npy"],
                ["--fb-alpha", "0.02"], ["--fb-beta", "1"], ["--consistent", "--fb-alpha", "1.5"],
                ["--consistent", "--fb-beta", "-1"], ["--consistent", "--fb-alpha", "nan"]):
        with pytest.raises(SystemExit):
            G.parse_arguments(base + bad)
