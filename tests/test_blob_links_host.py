"""Blob links without a GPU: the exports, the host-only check, the proof that the reference of tests/blob_link_cases.py is the
definition (an independent per-pixel loop) and that every case has the property it is named for, the host's way from the
device's slots to the table (built stand-alone under the address and undefined-behaviour sanitizers), tracks() on hand-written
link tables, the rows and the CSV with tracks, the command line's rules, and the proof on the CPU oracle that the synthetic
clip of test_gpu_blob_links.py has the two tracks that test asks for."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before libofc.so is loaded, as in test_blobs_host.py)

from tests import blob_cases as BC
from tests import blob_link_cases as LC

EXPORTS = ("ofc_blob_link_check", "ofc_blob_moves_dev", "ofc_blob_links_dev", "ofc_blob_links_read", "ofc_blob_links",
           "ofc_stream_set_blob_links", "ofc_stream_read_blob_links", "ofc_bench_blob_links")


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _B():
    from opticalflowclustering_amd import blobs
    return blobs


def test_the_new_exports_exist_and_the_constants_agree():
    L = _L()
    lib = C.CDLL(L.LIB_PATH)
    names = EXPORTS + ("ofc_blob_links_bytes",)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) <= set(L.EXPORTS)
    header = open(os.path.join(BC.ROOT, "include", "ofc.h")).read()
    assert all(f"int {n}(" in header for n in EXPORTS) and "size_t ofc_blob_links_bytes(" in header
    B = _B()
    assert (L.BLOB_LINK_FIELDS, L.BLOB_NO_MOVE) == (LC.LINK_NF, LC.NO_MOVE) and B.NO_MOVE == LC.NO_MOVE == -0x7fff8000
    assert len(B.LINK_FIELDS) == B.LINK_NF == LC.LINK_NF == 3
    assert B.TRACK_CSV_HEADER == B.CSV_HEADER + ("track",)
    src = open(os.path.join(BC.ROOT, "opticalflowclustering_amd", "csrc", "blobs.h")).read()
    assert f"BLOB_SHARE = {LC.SHARE};" in src                                   # the share the cases aim at


# ---- the host-only check, and the size of the tables ----
def test_blob_link_check_accepts_and_refuses_exactly_the_domain():
    L = _L()
    check = L.load().ofc_blob_link_check
    ok = (64, 48, 3, 1, 4096)
    assert check(*ok) == L.OFC_OK

    def with_(**kw):
        names = ("W", "H", "npair", "min_area", "max_links")
        return check(*[kw.get(n, v) for n, v in zip(names, ok)])

    assert with_(W=1, H=1) == L.OFC_OK and with_(W=0) == L.OFC_EINVAL and with_(H=0) == L.OFC_EINVAL and with_(H=-2) == L.OFC_EINVAL
    assert with_(W=2 ** 31 - 1, H=1) == L.OFC_OK and with_(W=46341, H=46340) == L.OFC_OK
    assert with_(W=65536, H=32768) == L.OFC_EUNSUPPORTED and with_(W=46341, H=46341) == L.OFC_EUNSUPPORTED
    assert with_(npair=1) == L.OFC_OK and with_(npair=65535) == L.OFC_OK           # one pair: zero transitions, allowed
    assert with_(npair=0) == L.OFC_EINVAL and with_(npair=65536) == L.OFC_EUNSUPPORTED
    assert with_(min_area=1) == L.OFC_OK and with_(min_area=2 ** 31 - 1) == L.OFC_OK and with_(min_area=0) == L.OFC_EINVAL
    assert with_(max_links=1) == L.OFC_OK and with_(max_links=65536) == L.OFC_OK
    assert with_(max_links=0) == L.OFC_EINVAL and with_(max_links=-1) == L.OFC_EINVAL
    assert with_(max_links=65537) == L.OFC_EUNSUPPORTED and "max_links" in L.load().ofc_last_error().decode()
    B = _B()
    B.check_link_args(64, 48, 3)
    with pytest.raises(ValueError, match="max_links"):
        B.check_link_args(64, 48, 3, max_links=0)
    with pytest.raises(L.OfcError):
        B.check_link_args(64, 48, 3, max_links=65537)


def test_links_bytes_is_twelve_bytes_a_slot_of_a_power_of_two_capacity():
    size = _L().load().ofc_blob_links_bytes
    for max_links, cap in ((1, 2), (2, 4), (3, 8), (4, 8), (5, 16), (4096, 8192), (4097, 16384), (65536, 131072)):
        assert cap >= 2 * max_links and cap & (cap - 1) == 0 and cap < 4 * max_links
        for ntrans in (0, 1, 7):
            assert size(max_links, ntrans) == 12 * cap * ntrans
    assert size(0, 1) == 0 and size(65537, 1) == 0 and size(4, -1) == 0


# ---- the reference is the definition ----
def loop_links(lab_a, flow_a, lab_b, min_area):
    """one transition by a plain loop over the pixels, from the field itself.  Shares nothing with blob_link_cases' numpy."""
    H, W = lab_a.shape
    la, lb, f = lab_a.tolist(), lab_b.tolist(), np.asarray(flow_a, np.float32)

    def areas(lab):
        out = {}
        for row in lab:
            for r in row:
                out[r] = out.get(r, 0) + 1
        return out

    area_a, area_b = areas(la), areas(lb)
    votes = {}
    for y in range(H):
        for x in range(W):
            a = la[y][x]
            u, v = f[y, x]
            if a < 0 or area_a[a] < min_area:
                continue
            if not (np.isfinite(u) and np.isfinite(v) and abs(u) < 1024 and abs(v) < 1024):
                continue
            xt, yt = x + int(np.rint(u)), y + int(np.rint(v))
            if not (0 <= xt < W and 0 <= yt < H):
                continue
            b = lb[yt][xt]
            if b < 0 or area_b[b] < min_area:
                continue
            votes[(a, b)] = votes.get((a, b), 0) + 1
    return np.array([[a, b, n] for (a, b), n in sorted(votes.items())], np.int64).reshape(-1, LC.LINK_NF)


@pytest.mark.parametrize("connectivity", LC.CONNECTIVITIES)
@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_reference_equals_an_independent_per_pixel_loop(case, connectivity):
    lab = LC.labels_of(case, connectivity)
    for min_area in (1, 7):
        links, nlinks = LC.reference(case, connectivity, min_area, 10 ** 6)
        assert len(links) == len(nlinks) == len(lab) - 1 and nlinks.dtype == np.int32
        for t, got in enumerate(links):
            want = loop_links(lab[t], case.flow[t], lab[t + 1], min_area)
            assert got.dtype == np.int64 and np.array_equal(got, want) and nlinks[t] == len(want)
    direct, n = LC.links_of(lab, LC.case_moves(case), 1, 10 ** 6)                 # the uncached form is the same function
    assert all(np.array_equal(a, b) for a, b in zip(direct, LC.reference(case, connectivity, 1, 10 ** 6)[0]))


def test_moves_follow_every_rounding_rule_and_every_special_value():
    S = LC.SPECIALS
    m = LC.moves_of(S)
    dx, dy = LC.unpack(m)
    got = {tuple(map(float, s)): (int(a), int(b)) if w != LC.NO_MOVE else None for s, w, a, b in zip(S.tolist(), m, dx, dy)}
    assert got[(0.5, -0.5)] == (0, 0) and got[(1.5, -1.5)] == (2, -2) and got[(2.5, -2.5)] == (2, -2)      # ties go to even
    assert got[(-2.5, 3.5)] == (-2, 4)
    assert got[(float(np.float32(0.49999997)), float(np.float32(-0.50000006)))] == (0, -1)               # one ulp either side of a tie
    assert got[(-0.0, 0.0)] == (0, 0) and got[(7.0, -3.0)] == (7, -3)
    assert got[(float(np.float32(1023.99)), float(np.float32(-1023.99)))] == (1024, -1024)              # valid, and fits int16
    assert got[(1024.0, 2.0)] is None and got[(3.0, -1024.0)] is None
    assert m[np.isnan(S).any(1) | np.isinf(S).any(1)].tolist() == [LC.NO_MOVE] * 3
    assert LC.unpack(np.array([LC.NO_MOVE], np.int32))[0][0] == -32768 == LC.unpack(np.array([LC.NO_MOVE], np.int32))[1][0]
    word = LC.moves_of(np.array([[-3.0, 2.0]], np.float32))[0]
    assert int(word) == (2 << 16) | 0xfffd                                        # (uint16)dy << 16 | (uint16)dx
    want = {tuple(v) for v in S.view(np.uint32).tolist()}                        # bit patterns: -0.0 and NaN compare by them
    for name in ("specials-64x16", "blocks-200x50"):                             # the cases carry every one, inside components
        c = BY(name)
        for i in range(len(c.keys)):
            assert want <= {tuple(v) for v in c.flow[i][c.keys[i] != BC.BG].view(np.uint32).tolist()}, (name, i)


def BY(name):
    return LC.BY_NAME[name]


def distinct_per_share(case, connectivity, t=0):
    """the largest number of distinct links among the pixels of one share of transition t"""
    lab, mv = LC.labels_of(case, connectivity), LC.case_moves(case)
    H, W = lab.shape[1:]
    most = 0
    for p0 in range(0, H * W, LC.SHARE):
        a = np.full(H * W, -1, np.int32)
        a[p0:p0 + LC.SHARE] = lab[t].ravel()[p0:p0 + LC.SHARE]
        most = max(most, len(LC.links_one(a.reshape(H, W), mv[t], lab[t + 1], 1)))
    return most


def test_the_case_table_covers_the_sizes_and_the_pair_counts():
    shapes = {c.keys.shape[1:] for c in LC.CASES}
    assert {(16, 64), (33, 70), (40, 129), (50, 200), (300, 1), (1, 300)} <= shapes
    assert (BC.TH, BC.TW) == (16, 64)                                             # 64x16 is one tile, 70x33 ragged against it
    assert max(h * w for h, w in shapes) <= 20000 and {len(c.keys) for c in LC.CASES} == {1, 3}
    assert -(-200 * 50 // LC.SHARE) == 5 and 200 * 50 % LC.SHARE != 0             # five shares, the last one short
    assert {name.rsplit("-", 1)[0] for name in LC.BY_NAME} >= {"specials", "frame-edges", "background", "merge-and-split",
                                                                "many-links", "min-area", "pair-isolation", "single-pair"}


def test_each_case_has_the_property_it_is_named_for():
    # frame edges: each of the eight directions leaves by exactly one pixel, and stays by exactly zero
    c = BY("frame-edges-70x33")
    H, W = c.keys.shape[1:]
    dx, dy = LC.unpack(LC.case_moves(c))
    yy, xx = np.mgrid[0:H, 0:W]
    for pair in (0, 1):
        xt, yt = xx + dx[pair], yy + dy[pair]
        out = {(int(np.sign(a - np.clip(a, 0, W - 1))), int(np.sign(b - np.clip(b, 0, H - 1)))) for a, b in zip(xt.ravel(), yt.ravel())}
        assert out == set(LC.EDGE_MOVES.values()) | {(0, 0)}
        moved = (dx[pair] != 0) | (dy[pair] != 0)
        inside = moved & (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
        assert inside.sum() == 8 and (((xt == 0) | (xt == W - 1) | (yt == 0) | (yt == H - 1))[inside]).all()     # onto the border itself
        assert (moved & ~inside).sum() == 8
    xt, yt = xx + dx[0], yy + dy[0]
    assert int(np.abs(xt - np.clip(xt, 0, W - 1)).max()) == 1 and int(np.abs(yt - np.clip(yt, 0, H - 1)).max()) == 1      # by exactly one
    assert LC.reference(c, 8)[1].tolist() == [2, 4]            # the far-border moves of pair 1 cross between the two halves
    # background: sources on background, targets on background, and votes all the same
    c = BY("background-129x40")
    lab, (dx, dy) = LC.labels_of(c, 8), LC.unpack(LC.case_moves(c))
    H, W = lab.shape[1:]
    yy, xx = np.mgrid[0:H, 0:W]
    xt, yt = np.clip(xx + dx[0], 0, W - 1), np.clip(yy + dy[0], 0, H - 1)
    assert (lab[0] < 0).sum() > 1000 and ((lab[0] >= 0) & (lab[1][yt, xt] < 0)).sum() > 500
    assert sum(int(r[:, 2].sum()) for r in LC.reference(c, 8)[0]) > 2000
    # merge and split
    c = BY("merge-and-split-200x50")
    (first, second), n = LC.reference(c, 8)
    assert n.tolist() == [2, 2]
    assert len(set(first[:, 0])) == 2 and len(set(first[:, 1])) == 1 and (first[:, 2] == 600).all()       # two sources, one target
    assert len(set(second[:, 0])) == 1 and len(set(second[:, 1])) == 2 and (second[:, 2] == 600).all()    # one source, two targets
    assert first[0, 1] == second[0, 0]                                            # the middle pair is target and source
    # many links: every pixel its own blob under 4, one blob under 8; far more links in a share than the LDS table holds
    c = BY("many-links-129x40")
    fg = int((c.keys[0] != BC.BG).sum())
    links, n = LC.reference(c, 4)
    gone = int((c.keys[0][:, -2:] != BC.BG).sum())                               # the last two columns leave the frame
    assert n[0] == len(links[0]) == fg - gone > 2000
    assert (links[0][:, 2] == 1).all() and (links[0][:, 1] == links[0][:, 0] + 2).all()
    assert distinct_per_share(c, 4) >= 1000 and LC.reference(c, 8)[1].tolist() == [1, 1]
    assert n[0] > 2 * 256 * 4                                                     # more than the work-groups' LDS tables hold together
    # min_area: at the area and one above it, on the source side and on the target side
    c = BY("min-area-70x33")
    lab = LC.labels_of(c, 8)
    assert sorted(np.bincount(lab[0][lab[0] >= 0])[np.unique(lab[0][lab[0] >= 0])].tolist()) == [4, 9, 16]
    assert sorted(np.bincount(lab[1][lab[1] >= 0])[np.unique(lab[1][lab[1] >= 0])].tolist()) == [4, 6, 25]
    count = {m: LC.reference(c, 8, m)[1].tolist() for m in (1, 4, 5, 6, 7, 9, 10, 16, 17)}
    assert count[1] == count[4] == [3, 3] and count[5] == [2, 2]                  # the 4 -> 4 link: both sides at once
    assert count[6] == [2, 2] and count[7] == [1, 1]                              # 16 -> 6 goes with its TARGET at 7
    assert count[9] == [1, 1] and count[10] == [0, 1]                             # 9 -> 25 goes with its SOURCE at 10
    assert count[16] == [0, 1] and count[17] == [0, 1]
    # pair isolation: the shift is found whole, the last pair is unlike both and has no transition of its own
    c = BY("pair-isolation-64x16")
    lab = LC.labels_of(c, 4)
    (first, second), n = LC.reference(c, 4)
    assert (first[:, 1] == first[:, 0] + 64 + 3).all() and len(first) == len(set(first[:, 0])) == len(set(first[:, 1]))
    assert not np.array_equal(c.keys[2], c.keys[0]) and not np.array_equal(c.keys[2], c.keys[1]) and len(n) == 2
    other = c.flow.copy()
    other[2] = 0                                                                  # the last pair's field takes no part
    assert all(np.array_equal(a, b) for a, b in zip(LC.links_of(lab, LC.moves_of(other))[0], (first, second)))
    # single pair: no transition
    c = BY("single-pair-64x16")
    assert len(c.keys) == 1 and LC.reference(c, 8)[0] == [] and LC.reference(c, 8)[1].shape == (0,)
    # 1xN and Nx1: most moves leave the frame sideways, some stay
    for name in ("1xN", "Nx1"):
        assert 20 < sum(LC.reference(BY(name), 8)[1]) < 150


def test_the_max_links_case_has_exactly_that_many_links_and_one_fewer_delivers_none():
    c = BY("many-links-129x40")
    every, n = LC.reference(c, 4, 1, 10 ** 6)
    m = int(n[0])
    assert m == len(every[0]) == n[1] and 2048 < m <= LC.MAXL
    links, n = LC.reference(c, 4, 1, m)
    assert n.tolist() == [m, m] and len(links[0]) == m
    links, n = LC.reference(c, 4, 1, m - 1)
    assert n.tolist() == [-1, -1] and links[0].shape == (0, LC.LINK_NF)
    rows, k = LC.deliver(every[0][:5], 5)
    assert k == 5 and len(rows) == 5 and LC.deliver(every[0][:5], 4)[1] == -1


# ---- from the device's slots to the table: the host function, stand-alone, under sanitizers ----
@pytest.fixture(scope="module")
def order_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("order") / "blob_links_order")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(BC.ROOT, "tests", "blob_links_order_main.cpp"), "-o", exe])
    return exe


def run_order(exe, max_links, counter, keys, votes):
    text = f"{max_links} {counter}\n" + "".join(f"{int(k)} {int(v)}\n" for k, v in zip(keys, votes))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.split("\n")
    state, n = lines[0].split()
    rows = np.array([[int(v) for v in line.split()] for line in lines[1:1 + max_links]], np.int64).reshape(max_links, 3)
    return state, int(n), rows


def test_the_host_order_sorts_zeroes_and_applies_the_minus_one_rule(order_program):
    EMPTY, FULL = 2 ** 64 - 1, 1 << 30
    r = np.random.default_rng(4)
    max_links, cap = 6, 16
    want = np.array([[0, 0, 3], [0, 5, 1], [2, 1, 7], [2 ** 31 - 2, 0, 2], [2 ** 31 - 2, 2 ** 31 - 2, 2 ** 31 - 1]], np.int64)
    keys, votes = np.full(cap, EMPTY, np.uint64), np.zeros(cap, np.int64)
    where = r.permutation(cap)[:len(want)]                                       # the device's order is unspecified
    keys[where] = (want[:, 0].astype(np.uint64) << np.uint64(32)) | want[:, 1].astype(np.uint64)
    votes[where] = want[:, 2]
    state, n, rows = run_order(order_program, max_links, len(want), keys, votes)
    assert (state, n) == ("ok", len(want)) and np.array_equal(rows[:n], want) and not rows[n:].any()
    keys6, votes6 = keys.copy(), votes.copy()
    free = np.flatnonzero(keys == EMPTY)[:2]
    keys6[free[0]], votes6[free[0]] = (1 << 32) | 9, 4
    state, n, rows = run_order(order_program, max_links, 6, keys6, votes6)       # exactly max_links: delivered
    assert (state, n) == ("ok", 6) and np.array_equal(rows, np.insert(want, 2, [1, 9, 4], 0))
    keys6[free[1]], votes6[free[1]] = (7 << 32) | 7, 4
    state, n, rows = run_order(order_program, max_links, 7, keys6, votes6)       # one more was claimed: none, -1
    assert (state, n) == ("ok", -1) and not rows.any()
    state, n, rows = run_order(order_program, max_links, 9 | FULL, keys6, votes6)        # a full table past max_links is overflow
    assert (state, n) == ("ok", -1) and not rows.any()
    state, n, rows = run_order(order_program, max_links, 5 | FULL, keys, votes)  # full with room left: the cap was hit wrongly
    assert state == "unsound" and not rows.any()
    state, n, rows = run_order(order_program, max_links, 4, keys, votes)         # the counter and the slots disagree
    assert state == "unsound" and not rows.any()
    state, n, rows = run_order(order_program, 1, 0, [EMPTY, EMPTY], [0, 0])      # the smallest table, empty
    assert (state, n) == ("ok", 0) and not rows.any()


# ---- tracks ----
def blobs_with(roots_per_pair, links, nlinks=None, found=None):
    B = _B()
    recs = []
    for roots in roots_per_pair:
        r = np.zeros((len(roots), BC.NF), np.int64)
        r[:, 0], r[:, 2] = roots, 5
        recs.append(r)
    b = B.Blobs(100, 50, None, recs, np.array([len(r) for r in recs] if found is None else found, np.int32))
    b.links = [np.array(l, np.int64).reshape(-1, 3) for l in links]
    b.nlinks = np.array([len(l) for l in b.links] if nlinks is None else nlinks, np.int32)
    return b


def ids(t):
    return [i.tolist() for i in t.ids]


def test_tracks_on_hand_written_link_tables():
    B = _B()
    # a chain, and a blob that appears late
    t = B.tracks(blobs_with([[3, 9], [4, 10], [5, 11, 40]], [[[3, 4, 8], [9, 10, 6]], [[4, 5, 8], [10, 11, 2]]]))
    assert ids(t) == [[0, 1], [0, 1], [0, 1, 2]] and t.n_tracks == 3 and t.broken == [] and t.lengths().tolist() == [3, 3, 1]
    assert all(i.dtype == np.int64 for i in t.ids)
    # ties: succ takes the smaller root_b, pred the smaller root_a
    t = B.tracks(blobs_with([[1], [2, 6]], [[[1, 2, 5], [1, 6, 5]]]))
    assert ids(t) == [[0], [0, 1]]
    t = B.tracks(blobs_with([[1, 7], [3]], [[[1, 3, 5], [7, 3, 5]]]))
    assert ids(t) == [[0, 1], [0]]
    # a split: the larger share keeps the id, the other part starts a new one
    t = B.tracks(blobs_with([[1], [2, 6]], [[[1, 2, 4], [1, 6, 9]]]))
    assert ids(t) == [[0], [1, 0]] and t.n_tracks == 2
    # a merge: the larger share keeps the id, the other track ends
    t = B.tracks(blobs_with([[1, 7], [3], [3]], [[[1, 3, 4], [7, 3, 9]], [[3, 3, 13]]]))
    assert ids(t) == [[0, 1], [1], [1]] and t.lengths().tolist() == [1, 3]
    # succ and pred must agree: 5 prefers 6, 6 prefers 5, so 9 (whose only link is from 5) starts anew
    t = B.tracks(blobs_with([[1, 5], [2, 6, 9]], [[[1, 2, 5], [1, 6, 5], [5, 6, 7], [5, 9, 1]]]))
    assert ids(t) == [[0, 1], [0, 1, 2]]
    # a link under min_votes does not count
    b = blobs_with([[1], [2]], [[[1, 2, 3]]])
    assert ids(B.tracks(b)) == [[0], [0]] and ids(B.tracks(b, min_votes=3)) == [[0], [0]]
    assert ids(B.tracks(b, min_votes=4)) == [[0], [1]]
    # ... and with min_votes the runner-up may win
    b = blobs_with([[1, 5], [2]], [[[1, 2, 2], [5, 2, 9]]])
    assert ids(B.tracks(b)) == [[0, 1], [1]]
    # links whose roots have no record (filtered by the table's min_area or max_blobs) do not count
    t = B.tracks(blobs_with([[1], [2]], [[[1, 2, 5], [1, 30, 50], [8, 2, 50]]]))
    assert ids(t) == [[0], [0]]
    # an overflowed transition breaks every track through it
    t = B.tracks(blobs_with([[1, 5], [2, 6], [3, 7]], [[], [[2, 3, 5], [6, 7, 5]]], nlinks=[-1, 2]))
    assert ids(t) == [[0, 1], [2, 3], [2, 3]] and t.broken == [0] and t.n_tracks == 4
    # a pair that overflowed its blob table has no records: both transitions next to it break
    t = B.tracks(blobs_with([[1], [], [3], [4]], [[[1, 2, 5]], [[2, 3, 5]], [[3, 4, 5]]], found=[1, 9000, 1, 1]))
    assert ids(t) == [[0], [], [1], [1]] and t.broken == [0, 1]
    # an empty pair that did not overflow breaks nothing, it just ends the tracks
    t = B.tracks(blobs_with([[1], [], [3]], [[], []]))
    assert ids(t) == [[0], [], [1]] and t.broken == []
    # one pair, no transitions; no links at all is an error
    assert ids(B.tracks(blobs_with([[4, 8]], []))) == [[0, 1]]
    plain = B.Blobs(8, 8, None, [np.zeros((0, BC.NF), np.int64)], np.array([0], np.int32))
    assert plain.links is None and plain.nlinks is None and plain.moves is None
    with pytest.raises(ValueError, match="no links"):
        B.tracks(plain)
    with pytest.raises(ValueError, match="label map"):
        B.link(plain, np.zeros((1, 8, 8, 2), np.float32))


def test_rows_with_tracks_and_the_csv_with_and_without_them(tmp_path):
    from opticalflowclustering_amd import motionGrids as G
    B = _B()
    rec0 = np.array([[205, 1, 4, 5, 2, 6, 3, 22, 10, 4, int(1.5 * 65536 * 4), int(-0.25 * 65536 * 4)]], np.int64)
    rec1 = np.array([[3, 2, 1, 3, 0, 3, 0, 3, 0, 1, 65536, -32768], [207, 1, 4, 7, 2, 8, 3, 30, 10, 4, 0, 0]], np.int64)
    b = B.Blobs(100, 50, None, [rec0, rec1], np.array([1, 2], np.int32))
    b.links, b.nlinks = [np.array([[205, 207, 4]], np.int64)], np.array([1], np.int32)
    t = B.tracks(b)
    assert ids(t) == [[0], [1, 0]]
    plain, tracked = b.rows(), b.rows(t)
    assert [r[:-1] for r in tracked] == plain and [r[-1] for r in tracked] == [0, 1, 0] and len(tracked[0]) == len(B.TRACK_CSV_HEADER)
    assert plain[0] == (0, 1, 5, 2, 4, 5, 2, 6, 3, "5.500", "2.500", "1.5000", "-0.2500")
    without, with_ = str(tmp_path / "plain.csv"), str(tmp_path / "sub" / "tracks.csv")
    G.write_blob_csv(without, b)
    G.write_blob_csv(with_, b, tracks=True)
    head = "pair,key,root_x,root_y,area,xmin,ymin,xmax,ymax,cx,cy,mean_u,mean_v"
    body = ["0,1,5,2,4,5,2,6,3,5.500,2.500,1.5000,-0.2500", "1,2,3,0,1,3,0,3,0,3.000,0.000,1.0000,-0.5000",
            "1,1,7,2,4,7,2,8,3,7.500,2.500,0.0000,0.0000"]
    assert open(without).read() == "\n".join([head] + body) + "\n"               # byte for byte what it was
    assert open(with_).read() == "\n".join([head + ",track"] + [r + "," + i for r, i in zip(body, "010")]) + "\n"


def test_motion_grids_track_arguments():
    from opticalflowclustering_amd import motionGrids as G
    base = ["--path", "clip.npy", "-c", "3", "-f", "out.csv"]
    a = G.parse_arguments(base)
    assert not a.tracks and a.max_links == 0 and a.blob_spec is None
    a = G.parse_arguments(base + ["--blobs", "b.csv"])
    assert not a.tracks and a.max_links == 0 and a.blob_spec == dict(thr=0.5, connectivity=8, min_area=1, max_blobs=G.MAX_BLOBS)
    a = G.parse_arguments(base + ["--blobs", "b.csv", "--tracks", "--model", "m.npy", "--stream", "--camera", "affine"])
    assert a.tracks and a.max_links == G.MAX_LINKS == 4096 and a.stream
    assert a.blob_spec == dict(thr=0.5, connectivity=8, min_area=1, max_blobs=G.MAX_BLOBS)       # the spec keeps its four values
    for bad in (["--tracks"], ["--tracks", "--blob-thr", "2"], ["--blobs", "b.csv", "--tracks", "3"]):
        with pytest.raises(SystemExit):
            G.parse_arguments(base + bad)


# ---- the synthetic clip of the GPU test has the tracks that test asks for: proved on the CPU oracle ----
def host_tracks(moves_field, keyed_field, thr, min_area):
    """blobs of keyed_field (moving pixels, connectivity 8), linked by the moves of moves_field, all on the host"""
    B = _B()
    s = keyed_field[..., 0] * keyed_field[..., 0] + keyed_field[..., 1] * keyed_field[..., 1]
    keys = np.where(s >= np.float32(thr) * np.float32(thr), 0, 255).astype(np.uint8)
    lab = np.stack([BC.label_one(k, 8) for k in keys])
    recs = [np.array([r for r in BC.records_one(keys[i], lab[i]) if r[2] >= min_area], np.int64).reshape(-1, BC.NF)
            for i in range(len(keys))]
    b = B.Blobs(keys.shape[2], keys.shape[1], lab, recs, np.array([len(r) for r in recs], np.int32))
    b.links, b.nlinks = LC.links_of(lab, LC.moves_of(moves_field), min_area)
    return b, B.tracks(b)


@pytest.mark.parametrize("pan", [(0, 0), LC.CLIP_PAN], ids=["still-camera", "panning-camera"])
def test_the_synthetic_clip_has_two_tracks_on_the_cpu_oracle(pan):
    from oracle import oracle as O
    clip = LC.rect_clip(pan)
    assert clip.shape == (LC.CLIP_FRAMES, LC.CLIP_H, LC.CLIP_W) and clip.dtype == np.uint8
    fields = np.stack([O.farneback(clip[i], clip[i + 1]) for i in range(len(clip) - 1)])
    camera = np.median(fields.reshape(len(fields), -1, 2), 1)                     # the background dominates: a robust translation
    assert np.abs(camera + np.array(pan)).max() < 0.05                            # the image of the background moves by -pan
    residual = fields - camera[:, None, None, :].astype(np.float32)
    b, t = host_tracks(fields, residual, LC.CLIP_THR, LC.CLIP_MIN_AREA)
    n = len(fields)
    assert b.found.tolist() == [2] * n and t.n_tracks == 2 and t.lengths().tolist() == [n, n] and t.broken == []
    assert all(i.tolist() == [0, 1] for i in t.ids)
    for i in range(n):                                                            # they are the two rectangles, where they should be
        for j, (x, y, w, h, vx, vy) in enumerate(LC.CLIP_RECTS):
            want = np.array([x + vx * i - pan[0] * i + w / 2, y + vy * i - pan[1] * i + h / 2])
            assert np.abs(b.centroids(i)[j] - want).max() < 4.0
    if pan != (0, 0):
        # moves taken from the residual send the pixels to the wrong place: the link table changes
        wrong, _ = host_tracks(residual, residual, LC.CLIP_THR, LC.CLIP_MIN_AREA)
        assert any(not np.array_equal(a, c) for a, c in zip(b.links, wrong.links))
        assert sum(int(l[:, 2].sum()) for l in wrong.links) < sum(int(l[:, 2].sum()) for l in b.links)
