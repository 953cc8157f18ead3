"""The repair without a GPU: the exports and the constants, the host-only check of the arguments and the tile shape, the proof
that the model of tests/repair_cases.py is the definition (a plain per-pixel restatement in Python) and that every case reaches
what its row in the table claims, the properties a fill has whatever the data, and the rules of the Python layer and the
command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import repair_cases as RC

EXPORTS = ("ofc_repair_check", "ofc_repair_dev", "ofc_repair", "ofc_bench_repair", "ofc_stream_set_repair", "ofc_stream_read_repair")


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _K():
    from opticalflowclustering_amd import repair
    return repair


def test_the_new_exports_exist_and_the_constants_agree():
    import opticalflowclustering_amd as pkg
    L, K = _L(), _K()
    assert pkg.repair is K
    lib = C.CDLL(L.LIB_PATH)
    missing = [n for n in EXPORTS + ("ofc_repair_tile",) if not hasattr(lib, n)]
    assert not missing, missing
    assert set(EXPORTS + ("ofc_repair_tile",)) <= set(L.EXPORTS)
    header = open(os.path.join(RC.ROOT, "include", "ofc.h")).read()
    assert all(f"int {n}(" in header for n in EXPORTS) and "void ofc_repair_tile(int radius, int out[2])" in header
    define = {k: int(v) for k, v in re.findall(r"#define (OFC_REPAIR_\w+) (\d+)", header)}
    assert define["OFC_REPAIR_ROUNDS_MAX"] == L.REPAIR_ROUNDS_MAX == 254 and define["OFC_REPAIR_NCOUNT"] == L.REPAIR_NCOUNT == K.NCOUNT == 3
    assert define["OFC_REPAIR_UNFILLED"] == L.REPAIR_UNFILLED == K.UNFILLED == RC.UNFILLED == 255
    assert (define["OFC_REPAIR_TILE_W"], define["OFC_REPAIR_TILE_H"]) == K.tile(1)
    assert "computeOpticalFlowModule.py:20-22" in header[header.index("Repair of a flow field"):]
    for r in (1, 2):
        TX, TY = K.tile(r)
        assert TX >= 1 and TY >= 1 and (TX, TY) == RC.tile(r)


def test_repair_check_accepts_every_case_and_refuses_exactly_the_limits():
    L = _L()
    check = L.load().ofc_repair_check
    for c, p in RC.RUNS:
        n, H, W = c.shape
        assert check(W, H, n, *p.args()) == L.OFC_OK, (c, p)
    names = ("W", "H", "npair", "keep", "radius", "rounds", "min_count", "smooth")
    ok = (64, 48, 3, 1, 1, 8, 1, 0)

    def with_(**kw):
        return check(*[kw.get(n, v) for n, v in zip(names, ok)])

    def said(word):
        return word in L.load().ofc_last_error().decode()

    assert with_() == L.OFC_OK and with_(W=1, H=1) == L.OFC_OK and with_(W=16384, H=16384) == L.OFC_OK
    assert with_(W=16385) == L.OFC_EUNSUPPORTED and said("16384") and with_(H=16385) == L.OFC_EUNSUPPORTED
    assert with_(W=0) == L.OFC_EINVAL and with_(H=0) == L.OFC_EINVAL
    assert with_(npair=1) == L.OFC_OK and with_(npair=65535) == L.OFC_OK
    assert with_(npair=0) == L.OFC_EINVAL and with_(npair=65536) == L.OFC_EINVAL and said("npair")
    assert with_(keep=1) == L.OFC_OK and with_(keep=15) == L.OFC_OK
    assert with_(keep=0) == L.OFC_EINVAL and with_(keep=16) == L.OFC_EINVAL and said("keep")
    assert with_(radius=1) == L.OFC_OK and with_(radius=2) == L.OFC_OK
    assert with_(radius=0) == L.OFC_EINVAL and with_(radius=3) == L.OFC_EINVAL and said("radius")
    assert with_(rounds=0, smooth=1) == L.OFC_OK and with_(rounds=254) == L.OFC_OK
    assert with_(rounds=-1) == L.OFC_EINVAL and with_(rounds=255) == L.OFC_EINVAL and said("rounds")
    assert with_(rounds=0, smooth=0) == L.OFC_EINVAL and said("smooth")
    assert with_(min_count=1) == L.OFC_OK and with_(min_count=9) == L.OFC_OK and with_(radius=2, min_count=25) == L.OFC_OK
    assert with_(min_count=0) == L.OFC_EINVAL and with_(min_count=10) == L.OFC_EINVAL and with_(radius=2, min_count=26) == L.OFC_EINVAL
    assert said("min_count")
    assert with_(smooth=1) == L.OFC_OK and with_(smooth=-1) == L.OFC_EINVAL and with_(smooth=2) == L.OFC_EINVAL
    assert with_(W=16385, keep=0) == L.OFC_EINVAL                                # a value out of range comes before a size too large
    K = _K()
    K.check_args(64, 48, 3)
    with pytest.raises(ValueError, match="npair"):
        K.check_args(64, 48, 0)
    with pytest.raises(L.OfcError):
        K.check_args(16385, 48, 3)


# ---- the model is the definition ----
def same_numbers(a, b):
    """equal as numbers where both are numbers, the same kind of special elsewhere"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(invalid="ignore"):
        return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("case", RC.CASES, ids=repr)
def test_model_equals_a_plain_per_pixel_restatement(case):
    n, H, W = case.shape
    for p in case.params:
        out, filled, counts, st_out = case.reference(p)
        assert out.shape == (n, H, W, 2) and out.dtype == np.float32 and filled.shape == (n, H, W) and filled.dtype == np.uint8
        assert counts.shape == (n, 3) and counts.dtype == np.int64 and (counts.sum(1) == W * H).all()
        for t in range(n):
            F, fl = RC.loop_pair(case.flow[t].tolist(), None if case.state is None else case.state[t].tolist(), *p.args())
            assert np.array_equal(filled[t], np.array(fl, np.uint8)), (case, p, t)
            assert same_numbers(out[t], np.array(F, np.float64).astype(np.float32)), (case, p, t)
        assert (st_out is None) == (case.state is None)


@pytest.mark.parametrize("case,p", RC.RUNS, ids=repr)
def test_what_holds_for_every_fill(case, p):
    out, filled, counts, st_out = case.reference(p)
    src = RC.sources(case.flow, case.state, p.keep)
    never = filled == RC.UNFILLED
    done = ~src & ~never
    assert np.array_equal(filled == 0, src) and (filled[done] <= p.rounds).all()
    assert np.array_equal(counts, np.stack([src.sum((1, 2)), done.sum((1, 2)), never.sum((1, 2))], 1))
    assert np.array_equal(out.view(np.uint32)[never], case.flow.view(np.uint32)[never])           # never filled: the input's bits
    if not p.smooth:
        assert np.array_equal(out.view(np.uint32)[src], case.flow.view(np.uint32)[src])           # sources are untouched
    # a filled or smoothed component is one of its pair's input components of the same kind
    for t in range(len(out)):
        for comp in (0, 1):
            pool = case.flow[t][..., comp][RC.valid(case.flow[t])]
            assert np.isin(out[t][..., comp][~never[t]], pool).all()
    if case.state is not None:
        assert np.array_equal(st_out, np.where(done, RC.OK, case.state))
    if not never.any() and p.rounds and not p.smooth and case.state is not None and p.keep & 1:
        # idempotent where nothing stayed unfilled: the result with its updated states (a filled pixel is OK, and OK is kept)
        # has no target left
        again = RC.model(out, st_out, *p.args())
        assert np.array_equal(again[0].view(np.uint32), out.view(np.uint32)) and not again[1].any() and (again[2][:, 1:] == 0).all()


@pytest.mark.parametrize("case", [c for c in RC.CASES if c.claims], ids=repr)
def test_each_case_reaches_what_it_is_for(case):
    p = case.params[0]
    n, H, W = case.shape
    TX, TY = RC.tile(p.r)
    out, filled, counts, _ = case.reference(p)
    src = RC.sources(case.flow, case.state, p.keep)
    tgt = ~src
    if "seam" in case.claims:
        assert W > TX and H > TY
        assert (tgt[:, :, TX - 1] & tgt[:, :, TX]).any() and (tgt[:, TY - 1, :] & tgt[:, TY, :]).any()
    if "round3" in case.claims:
        assert ((filled >= 3) & (filled < RC.UNFILLED)).any()
    if "unfilled" in case.claims:
        assert (filled == RC.UNFILLED).any() and ((filled > 0) & (filled < RC.UNFILLED)).any()
    if "all_source" in case.claims:
        assert src.reshape(n, -1).all(1).any()
    if "all_target" in case.claims:
        all_t = tgt.reshape(n, -1).all(1)
        assert all_t.any() and (filled[all_t] == RC.UNFILLED).all() and (counts[all_t, 2] == W * H).all()
    # what the first round saw: the window counts and values of V_0
    first = [RC.window(case.flow[t], src[t], p.r) for t in range(n)]
    cnt = np.stack([f[1] for f in first])
    one = filled == 1
    if "even" in case.claims:
        assert (one & (cnt % 2 == 0)).any() and (one & (cnt % 2 == 1)).any()
    if "mincount" in case.claims:
        a, b = tgt & (cnt == p.min_count - 1), tgt & (cnt == p.min_count)
        beside = (a[:, :, :-1] & b[:, :, 1:]).any() or (a[:, :, 1:] & b[:, :, :-1]).any()
        assert beside or (a[:, :-1] & b[:, 1:]).any() or (a[:, 1:] & b[:, :-1]).any()
        assert not one[a].any() and one[b].all()
    if "tie" in case.claims or "split" in case.claims:
        tie = split = False
        r = p.r
        for t, y, x in np.argwhere(one):
            ys, xs = slice(max(y - r, 0), y + r + 1), slice(max(x - r, 0), x + r + 1)
            m = src[t][ys, xs]
            us, vs = case.flow[t][ys, xs, 0][m], case.flow[t][ys, xs, 1][m]
            tie |= (us == out[t, y, x, 0]).sum() > 1
            split |= not ((us == out[t, y, x, 0]) & (vs == out[t, y, x, 1])).any()
        assert tie or "tie" not in case.claims
        assert split or "split" not in case.claims


def test_the_values_case_holds_what_it_is_named_for():
    c = RC.BY_NAME["values-%dx7-n2-r1" % (RC.tile(1)[0] + 3)]
    f = c.flow.reshape(-1, 2)
    for s in RC.SPECIALS:
        for comp in (0, 1):
            col = f[:, comp]
            assert np.isnan(col).any() if s != s else (col == np.float32(s)).any(), (s, comp)
    assert (np.abs(c.flow) == np.float32(RC.BELOW)).any() and RC.BELOW < 1024.0
    assert (c.state > 3).any() and {p.keep for p in c.params} >= {1, 2, 5, 10, 15}
    bad = ~RC.valid(c.flow)
    assert (bad & (c.state == RC.OK)).any()                                        # not a source, whatever its state says
    for p in c.params:
        src = RC.sources(c.flow, c.state, p.keep)
        assert not src[bad].any() and not src[c.state > 3].any() and src.any()
        assert (c.reference(p)[1][bad] != 0).all()
    q = RC.BY_NAME["seams-quant-%dx%d-n3-r1" % (2 * RC.tile(1)[0] + 1, RC.tile(1)[1] + 3)].flow
    assert (q == 0).any() and np.signbit(q[q == 0]).any() and not np.signbit(q[q == 0]).all()      # both zeros
    assert ((q != 0) & (np.abs(q) < np.finfo(np.float32).tiny)).any()                              # a denormal


def test_the_table_has_the_shapes_and_the_modes():
    shapes = {(c.shape[2], c.shape[1], c.shape[0]) for c in RC.CASES}
    assert {(1, 1, 1), (1, 7, 2), (7, 1, 3), (2, 2, 1)} <= shapes
    for r in (1, 2):
        TX, TY = RC.tile(r)
        assert {(TX - 1, TY + 1, 2), (2 * TX + 1, TY + 3, 3)} <= shapes and ((2 * TX + 1) * (TY + 3)) % 2 == 1
        mine = [(c, p) for c, p in RC.RUNS if p.r == r]
        assert {(p.rounds > 0, p.smooth) for _, p in mine} == {(True, False), (True, True), (False, True)}
        assert {c.state is None for c, _ in mine} == {True, False}
        assert any(c.shape == (1, 2, 2) for c, _ in mine)


# ---- the Python layer ----
def test_the_python_layer_says_what_it_is_and_refuses_bad_shapes():
    K = _K()
    f = np.zeros((4, 5, 2), np.float32)
    with pytest.raises(ValueError, match="state should be"):
        K.fill(f, np.zeros((5, 4), np.uint8))
    with pytest.raises(ValueError, match="should be"):
        K.fill(np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="rounds"):
        K.fill(f, rounds=255)
    with pytest.raises(ValueError, match="smooth"):
        K.fill(f, rounds=0)
    with pytest.raises(ValueError, match="radius"):
        K.median(f, radius=3)
    with pytest.raises(ValueError):
        K.fill(f, np.zeros((4, 5), np.uint8), keep=(4,))
    rep = K.Repaired(None, None, [[6, 3, 1], [10, 0, 0]], None)
    assert len(rep) == 2 and rep.counts.dtype == np.int64 and np.allclose(rep.share(), [[0.6, 0.3, 0.1], [1, 0, 0]])
    assert (K.ROUNDS, K.MIN_COUNT) == (8, 1)
    from opticalflowclustering_amd.pipeline import ClipPipeline
    from opticalflowclustering_amd.stream import FlowStream
    for doc in (K.fill.__doc__, K.fill_dev.__doc__, ClipPipeline.repair.__doc__, FlowStream.set_repair.__doc__):
        assert "not tuned" in doc and "convention" in doc
    assert "computeOpticalFlowModule.py:20-22" in K.__doc__


def test_motion_grids_repair_arguments():
    from opticalflowclustering_amd import motionGrids as G
    base = ["--path", "clip.npy", "-c", "3", "-f", "out.csv"]
    a = G.parse_arguments(base)
    assert a.repair is None and a.repair_spec is None and not a.repair_smooth and a.repair_counts is None
    a = G.parse_arguments(base + ["--repair", "1"])
    assert a.repair_spec == dict(radius=1, rounds=8, smooth=False)
    a = G.parse_arguments(base + ["--repair", "2:3", "--repair-smooth", "--repair-counts", "n.npy", "--photometric"])
    assert a.repair_spec == dict(radius=2, rounds=3, smooth=True) and a.repair_counts == "n.npy" and a.photo_spec
    a = G.parse_arguments(base + ["--repair", "1:0", "--repair-smooth", "--stream", "--model", "m.npy"])
    assert a.repair_spec == dict(radius=1, rounds=0, smooth=True) and a.stream
    assert G.parse_arguments(base + ["--repair", "1", "--fit-stream"]).fit_stream
    assert G.parse_arguments(base + ["--repair", "1", "--consistent"]).consistent
    for bad in (["--repair", "3"], ["--repair", "0"], ["--repair", "1:255"], ["--repair", "1:-1"], ["--repair", "1:0"], ["--repair", "x"],
                ["--repair", "1:2:3"], ["--repair-smooth"], ["--repair-counts", "n.npy"]):
        with pytest.raises(SystemExit):
            G.parse_arguments(base + bad)
