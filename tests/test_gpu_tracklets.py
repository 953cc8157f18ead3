"""Tracklets on the device (tracklets.hip): pos, birth, len, why and the per-frame counts on every case of
tests/tracklet_cases.py, on device and host buffers, against the existing trajectory kernel, and the way up through
trajectories.py and ClipPipeline.

Every output is an integer, so everything is compared with array_equal against the numpy model of the case table -- there is
no tolerance anywhere; test_tracklet_host.py proves that model against a loop in Python integers and that the table reaches
what it is named for."""
import ctypes as C

import numpy as np
import pytest

from tests import tracklet_cases as K

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _T():
    from opticalflowclustering_amd import trajectories
    return trajectories


def tables(tk, M):
    """a Tracklets object back as the five padded tables of the model"""
    T, L, n = len(tk), tk.max_len, tk.n_pairs
    pos, birth = np.full((L + 1, M, 2), -1, np.int32), np.full(M, -1, np.int32)
    length, why = np.zeros(M, np.int32), np.full(M, 255, np.uint8)
    pos[:, :T], birth[:T], length[:T], why[:T] = tk.pos, tk.birth, tk.length, tk.why
    return pos, birth, length, why, np.stack([tk.empty, tk.born, tk.blocked], 1).astype(np.int32).reshape(n, 3)


class Dev:
    """a case's inputs on the device, poisoned outputs, and ofc_tracklets_dev on them"""

    def __init__(self, case):
        L = _L()
        self.case = case
        self.n, self.H, self.W = case.shape
        M, ln = case.M, case.L
        self.fd = L.DeviceBuffer(case.flow.nbytes).upload(case.flow)
        self.td = L.DeviceBuffer(case.state.nbytes).upload(case.state) if case.state is not None else None
        self.out = [L.DeviceBuffer(b) for b in ((ln + 1) * M * 8, M * 4, M * 4, M, self.n * 12)]
        self.shapes = (((ln + 1, M, 2), np.int32), ((M,), np.int32), ((M,), np.int32), ((M,), np.uint8), ((self.n, 3), np.int32))
        self.bufs = [b for b in [self.fd, self.td] + self.out if b is not None]

    def poison(self):
        L = _L()
        for b in self.out:
            L.check(L.load().ofc_memset(0, C.c_void_p(b.ptr), 0x55, b.nbytes))

    def call(self, **kw):
        c = self.case
        a = dict(flow=self.fd.ptr, state=self.td.ptr if self.td else None, W=self.W, H=self.H, n=self.n, cell=c.cell, L=c.L, M=c.M,
                 keep=c.keep, pos=self.out[0].ptr, birth=self.out[1].ptr, len=self.out[2].ptr, why=self.out[3].ptr,
                 frames=self.out[4].ptr)
        a.update(kw)
        v = lambda p: C.c_void_p(p) if p else None                                # noqa: E731
        return _L().load().ofc_tracklets_dev(0, v(a["flow"]), v(a["state"]), a["W"], a["H"], a["n"], a["cell"], a["L"], a["M"], a["keep"],
                                             v(a["pos"]), v(a["birth"]), v(a["len"]), v(a["why"]), v(a["frames"]))

    def run(self):
        self.poison()
        _L().check(self.call())
        return self.outputs()

    def outputs(self):
        return tuple(b.download(shape, dt) for b, (shape, dt) in zip(self.out, self.shapes))

    def inputs_unchanged(self):
        c = self.case
        assert np.array_equal(self.fd.download(c.flow.shape, np.uint32), c.flow.view(np.uint32))
        if self.td:
            assert np.array_equal(self.td.download(c.state.shape, np.uint8), c.state)

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("case", K.CASES, ids=repr)
def test_device_buffers_equal_the_model_twice_in_a_row(case):
    d = Dev(case)
    try:
        first = d.run()
        K.same(first, case.model())
        _L().check(d.call())                                                      # on the same buffers, not poisoned again
        K.same(d.outputs(), first)
        d.inputs_unchanged()
    finally:
        d.free()


HOST = ("shift-40x24-c8-L4", "shift-37x19-c5-L3", "sink-40x24-c8-L20", "source-40x24-c8-L20", "state-40x24-c8-L4",
        "specials-40x24-c4-L5", "one-pair-40x24-c8", "seam-257-cells")


@pytest.mark.parametrize("case", [K.BY_NAME[n] for n in HOST], ids=repr)
def test_host_buffers_and_follow_dense(case):
    L, T = _L(), _T()
    n, H, W = case.shape
    M, ln = case.M, case.L
    out = [np.full(s, 0x55, dt) for s, dt in (((ln + 1, M, 2), np.int32), ((M,), np.int32), ((M,), np.int32), ((M,), np.uint8),
                                              ((n, 3), np.int32))]
    flow = case.flow.copy()
    state = None if case.state is None else case.state.copy()
    L.check(L.load().ofc_tracklets(0, L.ptr(flow), L.ptr(state), W, H, n, case.cell, ln, M, case.keep, *(L.ptr(a) for a in out)))
    K.same(out, case.model())
    assert np.array_equal(flow.view(np.uint32), case.flow.view(np.uint32)) and (state is None or np.array_equal(state, case.state))
    tk = T.follow_dense(case.flow, case.cell, ln, M, state=case.state, keep=case.keep)
    K.same(tables(tk, M), case.model())
    assert len(tk) == case.used() and tk.overflowed == bool((case.model()[4][:, 1] < case.model()[4][:, 0]).any())
    assert tk.alive()[0] == case.model()[4][0, 1]


def test_follow_dense_defaults_and_takes_one_field():
    T = _T()
    case = K.BY_NAME["shift-40x24-c8-L4"]
    n, H, W = case.shape
    tk = T.follow_dense(case.flow)                                                # cell 8, length 15, the default pool
    M = K.default_max_tracks(W, H, n, 8, 15)
    assert tk.max_tracks == M == 45 and tk.max_len == 15
    want = K.model(case.flow, 8, 15, M)
    K.same(tables(tk, M), want)
    assert tk.overflowed == bool((want[4][:, 1] < want[4][:, 0]).any())
    one = T.follow_dense(case.flow[0], 8, 4)
    K.same(tables(one, 15), K.model(case.flow[:1], 8, 4, 15))
    with pytest.raises(ValueError, match="state"):
        T.follow_dense(case.flow, state=np.zeros((n, H, W - 1), np.uint8))
    with pytest.raises(ValueError):
        T.follow_dense(case.flow, cell=0)


CROSS = ("shift-40x24-c8-L4", "shift-37x19-c5-L3", "shift-37x16-c5-L3", "shift-67x35-c1-L2", "state-40x24-c8-L4",
         "specials-40x24-c4-L5", "one-step-40x24-c8-L1", "one-pair-40x24-c8", "seam-65-cells", "seam-257-cells")


@pytest.mark.parametrize("case", [K.BY_NAME[n] for n in CROSS], ids=repr)
def test_the_tracks_of_frame_0_equal_the_trajectory_kernel(case):
    """independent of the model: with max_tracks >= cells the ids 0 .. cells-1 hold the seeds of frame 0, and what they do is
    what ofc_traj_dev does with those seeds, cut at L steps"""
    T = _T()
    n, H, W = case.shape
    cells, ln = case.cells, case.L
    assert case.M >= cells
    d = Dev(case)
    try:
        pos, birth, length, why, frames = d.run()
        assert frames[0].tolist()[:2] == [cells - frames[0, 2], cells - frames[0, 2]]
        m = int(frames[0, 1])
        assert (birth[:m] == 0).all() and (m == case.used() or birth[m] > 0)
        seeds = np.ascontiguousarray(pos[0, :m])
        want = T.follow_dev(d.fd.ptr, W, H, n, seeds, state_ptr=d.td.ptr if d.td else None, keep=case.keep)
    finally:
        d.free()
    if case.state is None:                                                         # every cell was seeded, row by row, at its centre
        cols, rows, _ = K.grid(W, H, case.cell)
        ys, xs = np.mgrid[0:rows, 0:cols]
        centres = np.stack([np.minimum(xs * case.cell * 65536 + case.cell * 32768, (W - 1) << 16),
                            np.minimum(ys * case.cell * 65536 + case.cell * 32768, (H - 1) << 16)], -1).reshape(-1, 2)
        assert m == cells and np.array_equal(seeds, centres)
    full = want.length >= ln
    assert np.array_equal(length[:m], np.minimum(want.length, ln))
    assert np.array_equal(why[:m][full], np.full(full.sum(), K.FULL, np.uint8)) and np.array_equal(why[:m][~full], want.why[~full])
    top = min(n, ln)
    rows_kept = np.arange(top + 1)[:, None] <= length[None, :m]
    assert np.array_equal(pos[:top + 1, :m][rows_kept], want.pos[:top + 1][rows_kept])
    assert (pos[:, :m][np.arange(ln + 1)[:, None] > length[None, :m]] == -1).all()


def test_every_refusal_leaves_the_outputs_alone():
    L = _L()
    lib = L.load()
    case = K.BY_NAME["state-40x24-c8-L4"]
    n, H, W = case.shape
    d = Dev(case)
    try:
        assert d.call() == L.OFC_OK
        d.poison()
        o = d.out
        for kw in (dict(flow=None), dict(pos=None), dict(birth=None), dict(len=None), dict(why=None), dict(frames=None),
                   dict(flow=d.fd.ptr + 4), dict(pos=o[0].ptr + 4), dict(birth=o[1].ptr + 2), dict(len=o[2].ptr + 2),
                   dict(frames=o[4].ptr + 2), dict(W=0), dict(H=0), dict(n=0), dict(n=65536), dict(cell=0), dict(cell=16385),
                   dict(L=0), dict(L=4097), dict(M=0), dict(M=(1 << 28) + 1), dict(keep=-1), dict(keep=65536),
                   dict(W=4097, H=4096, cell=1)):
            assert d.call(**kw) == L.OFC_EINVAL, kw
        for kw in (dict(W=16385), dict(H=16385), dict(L=7, M=1 << 28), dict(L=4096, M=524161)):
            assert d.call(**kw) == L.OFC_EUNSUPPORTED, kw
        for got in d.outputs():
            assert (got.view(np.uint8) == 0x55).all()
        host = np.full(64, 0x55, np.uint8)
        hp = L.ptr(host)
        assert lib.ofc_tracklets(0, None, None, W, H, n, 8, 4, 4, 1, hp, hp, hp, hp, hp) == L.OFC_EINVAL
        assert lib.ofc_tracklets(0, L.ptr(case.flow), None, W, H, n, 0, 4, 4, 1, hp, hp, hp, hp, hp) == L.OFC_EINVAL
        assert lib.ofc_tracklets(0, L.ptr(case.flow), None, W, H, n, 8, 4, 4, 65536, hp, hp, hp, hp, hp) == L.OFC_EINVAL
        assert (host == 0x55).all()
        ms = C.c_float(-1.0)
        bench = lambda **kw: lib.ofc_bench_tracklets(0, C.c_void_p(kw.get("flow", d.fd.ptr)), W, H, kw.get("n", n), kw.get("cell", 8),  # noqa: E731
                                                     kw.get("L", 4), kw.get("M", 400), kw.get("iters", 2), C.byref(ms))
        assert bench(n=0) == L.OFC_EINVAL and bench(cell=0) == L.OFC_EINVAL and bench(L=0) == L.OFC_EINVAL and bench(M=0) == L.OFC_EINVAL
        assert bench(iters=0) == L.OFC_EINVAL and bench(flow=None) == L.OFC_EINVAL and ms.value == -1.0
        L.check(bench())
        assert ms.value > 0
        d.inputs_unchanged()
    finally:
        d.free()


# ---- ClipPipeline: 64x48 frames, the engine's default parameters ----
PW, PH, ST = 64, 48, 9
STRICT = dict(tau=2.0, kappa=0.25)


def test_pipeline_tracklets_equal_follow_dense_on_its_field():
    from opticalflowclustering_amd.pipeline import ClipPipeline
    from tests import motion_grid_cases as MC
    T = _T()
    frames = np.ascontiguousarray(MC.moving_blobs_clip(ST, PW, PH)[..., 0])
    pipe = ClipPipeline(PW, PH, ST, batch_pairs=3)
    try:
        pipe.upload_frames(frames)
        pipe.run_flow()
        field = pipe.flows_host()
        n = ST - 1
        args = dict(cell=8, length=3)
        for kw, sl in ((dict(), slice(0, n)), (dict(start=2), slice(2, n)), (dict(start=1, pairs=4), slice(1, 5)),
                       (dict(start=n - 1), slice(n - 1, n)), (dict(pairs=1), slice(0, 1))):
            got = pipe.tracklets(**args, **kw)
            want = T.follow_dense(field[sl], **args)
            M = K.default_max_tracks(PW, PH, sl.stop - sl.start, 8, 3)
            assert got.max_tracks == want.max_tracks == M
            K.same(tables(got, M), tables(want, M))
            K.same(tables(got, M), K.model(field[sl], 8, 3, M))
        small = pipe.tracklets(cell=5, length=2, max_tracks=200)                   # a pool that runs out, a cell that divides nothing
        K.same(tables(small, 200), K.model(field, 5, 2, 200))
        assert small.overflowed
        assert np.array_equal(pipe.flows_host().view(np.uint32), field.view(np.uint32))
        for bad in (dict(start=-1), dict(start=n), dict(pairs=0), dict(start=3, pairs=n - 2)):
            with pytest.raises(ValueError, match="range"):
                pipe.tracklets(**bad)
        with pytest.raises(ValueError, match="consistency"):                       # no state map yet
            pipe.tracklets(consistent=True)
        ph = pipe.photometric(**STRICT)
        assert len(set(ph.state.ravel().tolist())) >= 2
        for keep, kw in (((0,), dict()), ((0, 2), dict(start=3, pairs=4))):
            sl = slice(kw.get("start", 0), kw.get("start", 0) + kw.get("pairs", n))
            got = pipe.tracklets(cell=4, length=3, consistent=True, keep=keep, **kw)
            want = T.follow_dense(field[sl], 4, 3, state=ph.state[sl], keep=keep)
            M = K.default_max_tracks(PW, PH, sl.stop - sl.start, 4, 3)
            K.same(tables(got, M), tables(want, M))
            K.same(tables(got, M), K.model(field[sl], 4, 3, M, ph.state[sl], K.keep_mask(keep)))
            assert got.blocked.sum() > 0 or (got.why == T.UNTRUSTED).any()            # the state map was read
        assert np.array_equal(pipe.state.download((n, PH, PW), np.uint8), ph.state)
        pipe.compensate_camera("translation")
        with pytest.raises(ValueError, match="compensate_camera"):
            pipe.tracklets()
    finally:
        pipe.close()
