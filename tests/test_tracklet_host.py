"""The tracklets' definition on the CPU: the numpy model of tests/tracklet_cases.py against the loop in Python integers on
every case, that the case table reaches what it is named for, and the host-only parts of the library and of trajectories.py
(exports, every refusal of ofc_tracklets_check at both sides of its limits, the default pool, the Tracklets methods)."""
import numpy as np
import pytest

from tests import tracklet_cases as K

NAMES = ("ofc_tracklets_check", "ofc_tracklets_dev", "ofc_tracklets", "ofc_bench_tracklets")


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _T():
    from opticalflowclustering_amd import trajectories
    return trajectories


def live_cells(case, t):
    """the cells of the tracks that are live at frame t after its births, from the model's table"""
    pos, birth, length, why, frames = case.model()
    used = case.used()
    age = t - birth[:used]
    ids = np.flatnonzero((age >= 0) & (age <= length[:used]) & (age < case.L))
    at = pos[age[ids], ids].astype(np.int64)
    cols = K.grid(case.shape[2], case.shape[1], case.cell)[0]
    return (at[:, 1] >> 16) // case.cell * cols + (at[:, 0] >> 16) // case.cell


@pytest.mark.parametrize("case", K.CASES, ids=repr)
def test_model_equals_the_loop_and_keeps_the_tables_invariants(case):
    got = K.loop(case.flow, case.cell, case.L, case.M, case.state, case.keep)
    K.same(got, case.model())
    pos, birth, length, why, frames = got
    n, H, W = case.shape
    used, L, M = case.used(), case.L, case.M
    assert used <= M and (frames[:, 1] <= frames[:, 0]).all() and (frames[:, 0] + frames[:, 2] <= case.cells).all()
    assert (pos[:, used:] == -1).all() and (birth[used:] == -1).all() and (length[used:] == 0).all() and (why[used:] == 255).all()
    assert np.array_equal(birth[:used], np.repeat(np.arange(n), frames[:, 1]))           # ids in birth order
    steps = np.arange(L + 1)[:, None]
    inside = (pos >= 0).all(-1) & (pos[..., 0] <= (W - 1) << 16) & (pos[..., 1] <= (H - 1) << 16)
    assert np.array_equal(inside[:, :used], steps <= length[None, :used]) and ((pos == -1).all(-1) | inside).all()
    assert ((length[:used] == L) == (why[:used] == K.FULL)).all()
    assert ((why[:used] == K.RAN) <= (birth[:used] + length[:used] == n)).all()           # still live: it stepped every frame
    if (frames[:, 1] < frames[:, 0]).any():
        assert used == M


def reasons(case):
    return set(case.model()[3][:case.used()].tolist())


def test_the_table_reaches_what_it_is_named_for():
    B = K.BY_NAME
    c = B["shift-40x24-c8-L4"]
    fr = c.model()[4]
    assert fr[:5, 1].tolist() == [15, 3, 3, 0, 12] and reasons(c) == {K.FULL, K.LEAVES, K.RAN} and not (fr[:, 1] < fr[:, 0]).any()
    c = B["shift-37x19-c5-L3"]
    pos = c.model()[0]
    assert 37 % 5 and 19 % 5 and (c.model()[4][1:, 1] > 0).any()
    # the last column is 2 px wide: its seeds are clamped to x = 36; the last row is 4 px high and its centre, 17.5, is inside
    assert (pos[0, :c.cells, 0] == 36 << 16).sum() == 4 and (pos[0, :c.cells, 1] == (17 << 16) + 32768).sum() == 8
    c = B["shift-37x16-c5-L3"]
    pos = c.model()[0]
    assert (pos[0, :c.cells, 0] == 36 << 16).sum() == 4 and (pos[0, :c.cells, 1] == 15 << 16).sum() == 8      # clamped both ways
    assert (c.model()[4][1:, 1] > 0).any()
    c = B["sink-40x24-c8-L20"]
    fr = c.model()[4]
    assert c.L > c.shape[0] and c.used() == c.M and fr[-1].tolist() == [8, 5, 0] and (fr[:-1, 1] == fr[:-1, 0]).all()
    assert any(np.unique(live_cells(c, t), return_counts=True)[1].max() >= 2 for t in range(c.shape[0]))
    c = B["source-40x24-c8-L20"]
    fr = c.model()[4]
    short = np.flatnonzero(fr[:, 1] < fr[:, 0])
    assert 0 < fr[short[0], 1] < fr[short[0], 0] and (fr[short[1:], 1] == 0).all() and len(short) >= 2 and (fr[short[1:], 0] > 0).all()
    c = B["shift-67x35-c1-L2"]
    assert c.cells == 2345 > K.THREADS and (c.model()[4][:, 1] > 1000).sum() >= 2
    c = B["shift-9x7-c16-L3"]
    assert c.cells == 1 and c.model()[4][:, 1].tolist() == [1] * 5 and (c.model()[2][:5] == 0).all() and reasons(c) == {K.LEAVES}
    c = B["state-40x24-c8-L4"]
    assert (c.model()[4][:, 2] > 0).all() and K.UNTRUSTED in reasons(c) and len(set(c.model()[4][:, 2].tolist())) > 1
    assert K.INVALID in reasons(B["specials-40x24-c4-L5"])
    assert B["one-pair-40x24-c8"].shape[0] == 1 and B["one-step-40x24-c8-L1"].L == 1
    assert reasons(B["one-step-40x24-c8-L1"]) == {K.FULL, K.LEAVES}
    c = B["exact-pool-40x24-c8-L4"]
    fr = c.model()[4]
    assert c.used() == c.M and np.array_equal(fr, B["shift-40x24-c8-L4"].model()[4]) and not (fr[:, 1] < fr[:, 0]).any()
    for c in K.CASES:                                                              # every case but the one-pair one reseeds
        assert c.shape[0] == 1 or (c.model()[4][1:, 1] > 0).any(), c
    counts = {c.cells for c in K.CASES}
    assert counts >= {1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 256 * 256, 256 * 257}
    firsts = set()
    for c in K.CASES:                                                              # `used`, and the low end of the step's id window
        firsts |= set(np.cumsum(c.model()[4][:, 1]).tolist())
    assert firsts >= {255, 256, 257, 511, 513}


def test_the_exports_are_declared():
    L = _L()
    assert set(NAMES) <= set(L.EXPORTS)
    assert (L.TRAJ_FULL, L.TRACKLET_THREADS, L.TRACKLET_MAX_LEN, L.TRACKLET_MAX_TRACKS) == (4, K.THREADS, 4096, 1 << 28)
    assert _T().FULL == K.FULL


def test_every_refusal_of_the_check_at_both_sides_of_its_limit():
    L = _L()
    chk = L.load().ofc_tracklets_check
    base = dict(W=40, H=24, npair=9, cell=8, max_len=15, max_tracks=100, keep=1)
    call = lambda **kw: chk(*(dict(base, **kw)[k] for k in ("W", "H", "npair", "cell", "max_len", "max_tracks", "keep")))   # noqa: E731
    assert call() == L.OFC_OK
    for name, inside, outside in (("W", 1, 0), ("H", 1, 0), ("npair", 1, 0), ("npair", 65535, 65536), ("cell", 1, 0),
                                  ("cell", 16384, 16385), ("max_len", 1, 0), ("max_len", 4096, 4097), ("max_tracks", 1, 0),
                                  ("max_tracks", 1 << 28, (1 << 28) + 1), ("keep", 0, -1), ("keep", 65535, 65536)):
        kw = dict(max_len=1) if name == "max_tracks" else {}                       # 2 * 2^28 positions are still below 2^31
        assert call(**dict(kw, **{name: inside})) == L.OFC_OK, (name, inside)
        assert call(**dict(kw, **{name: outside})) == L.OFC_EINVAL, (name, outside)
        assert L.load().ofc_last_error()
    assert call(W=16384, H=16384, cell=4) == L.OFC_OK and call(W=16384, H=16384, cell=3) == L.OFC_EINVAL     # 2^24 cells
    assert call(W=4096, H=4096, cell=1) == L.OFC_OK and call(W=4097, H=4096, cell=1) == L.OFC_EINVAL
    assert call(W=16384, cell=16384) == L.OFC_OK and call(W=16385, cell=16384) == L.OFC_EUNSUPPORTED
    assert call(H=16384) == L.OFC_OK and call(H=16385) == L.OFC_EUNSUPPORTED
    assert call(max_len=7, max_tracks=(1 << 28) - 1) == L.OFC_OK and call(max_len=7, max_tracks=1 << 28) == L.OFC_EUNSUPPORTED
    assert call(max_len=4096, max_tracks=524160) == L.OFC_OK and call(max_len=4096, max_tracks=524161) == L.OFC_EUNSUPPORTED
    assert 4097 * 524160 < 2 ** 31 <= 4097 * 524161
    assert call(W=0, H=16385) == L.OFC_EINVAL                                      # a bad argument goes before an unsupported one
    T = _T()
    with pytest.raises(ValueError):
        T.check_dense_args(40, 24, 9, 0, 15, 100)
    with pytest.raises(L.OfcError):
        T.check_dense_args(40, 24, 9, 8, 7, 1 << 28)
    T.check_dense_args(40, 24, 9, 8, 15, 100, 65535)


def test_the_default_pool():
    T = _T()
    assert T.default_max_tracks(1920, 1080, 16, 8, 15) == 240 * 135 * 4
    assert T.default_max_tracks(40, 24, 9, 8, 4) == 15 * 6 and T.default_max_tracks(40, 24, 9, 8, 20) == 15 * 2
    assert T.default_max_tracks(40, 24, 1, 8, 15) == 15 and T.default_max_tracks(40, 24, 2, 8, 1) == 30      # capped at cells * n
    assert T.default_max_tracks(37, 19, 9, 5, 3) == 32 * 7
    for W, H, n, cell, length in ((40, 24, 9, 8, 4), (37, 19, 9, 5, 3), (67, 35, 4, 1, 2), (9, 7, 5, 16, 3), (64, 48, 8, 8, 15)):
        assert T.default_max_tracks(W, H, n, cell, length) == K.default_max_tracks(W, H, n, cell, length)
    assert T.grid_cells(37, 19, 5) == (8, 4)
    with pytest.raises(ValueError):
        T.grid_cells(37, 19, 0)


@pytest.mark.parametrize("name", ("shift-40x24-c8-L4", "source-40x24-c8-L20", "state-40x24-c8-L4", "shift-9x7-c16-L3"))
def test_the_tracklets_object_on_the_models_output(name):
    T = _T()
    case = K.BY_NAME[name]
    pos, birth, length, why, frames = case.model()
    n, used, L = case.shape[0], case.used(), case.L
    tk = T.Tracklets(pos.copy(), birth.copy(), length.copy(), why.copy(), frames.copy(), case.M)
    assert len(tk) == used and tk.pos.shape == (L + 1, used, 2) and tk.n_pairs == n and tk.max_len == L and tk.max_tracks == case.M
    assert np.array_equal(tk.pos, pos[:, :used]) and np.array_equal(tk.birth, birth[:used]) and np.array_equal(tk.why, why[:used])
    assert np.array_equal(tk.empty, frames[:, 0]) and np.array_equal(tk.born, frames[:, 1]) and np.array_equal(tk.blocked, frames[:, 2])
    assert tk.overflowed == bool((frames[:, 1] < frames[:, 0]).any()) == name.startswith("source")
    xy = tk.xy()
    assert np.array_equal(np.isnan(xy), tk.pos < 0) and np.array_equal(xy[0], tk.pos[0] / 65536.0)
    alive = tk.alive()
    assert alive.shape == (n,) and alive[0] == frames[0, 1]
    for t in range(n):
        ids, at = tk.at(t)
        assert len(ids) == alive[t]
        want = [i for i in range(used) if birth[i] <= t <= birth[i] + length[i] and t - birth[i] < L]
        assert ids.tolist() == want and np.array_equal(at, np.array([pos[t - birth[i], i] for i in want], np.int32).reshape(-1, 2))
    with pytest.raises(ValueError):
        tk.at(n)
    with pytest.raises(ValueError):
        tk.shapes(L + 1)
    rows, idx = tk.shapes()
    assert np.array_equal(idx, np.flatnonzero(length[:used] >= L)) and rows.shape == (len(idx), 2 * L)
    for k in sorted({1, L}):
        rows, idx = tk.shapes(k)
        assert np.array_equal(idx, np.flatnonzero(length[:used] >= k))
        fixed = T.Trajectories(np.ascontiguousarray(tk.pos[:k + 1]), np.where(tk.length >= k, k, 0).astype(np.int32), tk.why)
        want_rows, want_idx = fixed.shapes(k)                                      # the same descriptor as Trajectories.shapes
        assert np.array_equal(idx, want_idx) and np.array_equal(rows, want_rows)
        norm = np.sqrt((rows.reshape(len(idx), k, 2) ** 2).sum(2)).sum(1)          # 1, or 0 for a track that never moved
        moved = (tk.pos[1:k + 1, idx] != tk.pos[:k, idx]).any((0, 2))
        assert np.allclose(norm, moved.astype(np.float64))
        far, far_idx = tk.shapes(k, min_length=1e9)
        assert far.shape == (0, 2 * k) and len(far_idx) == 0
        near, near_idx = tk.shapes(k, min_length=0.0)
        assert np.array_equal(near, rows) and np.array_equal(near_idx, idx)
