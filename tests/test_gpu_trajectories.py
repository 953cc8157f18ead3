"""Trajectories on the device (trajectories.hip): pos, len and why on every case of tests/trajectory_cases.py at every way of
cutting the pairs into launches, on device and host buffers, and the way up through trajectories.py, ClipPipeline, FlowStream
and the motionGrids command line.

Every output is an integer, so everything is compared with array_equal against the numpy reference of the case table -- there
is no tolerance anywhere; test_trajectory_host.py proves that reference against a per-point loop and that the table reaches
what it is meant to."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import trajectory_cases as TC

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _T():
    from opticalflowclustering_amd import trajectories
    return trajectories


def same(got, want):
    for g, w, dt in zip(got, want, (np.int32, np.int32, np.uint8)):
        assert g.dtype == dt and g.shape == w.shape and np.array_equal(g, w), np.argwhere(g != w)[:5]


class Dev:
    """a case's inputs on the device, poisoned outputs, and ofc_traj_dev on them"""

    def __init__(self, flow, seeds, state, alias=False):
        L = _L()
        self.n, self.H, self.W = flow.shape[:3]
        self.P, self.alias = len(seeds), alias
        self.flow, self.seeds, self.state = flow, seeds, state
        self.fd = L.DeviceBuffer(flow.nbytes).upload(flow)
        self.sd = L.DeviceBuffer(seeds.nbytes).upload(seeds)
        self.td = L.DeviceBuffer(state.nbytes).upload(state) if state is not None else None
        self.pd = L.DeviceBuffer((self.n + 1) * self.P * 8)
        self.ld, self.wd = L.DeviceBuffer(self.P * 4), L.DeviceBuffer(self.P)
        self.bufs = [b for b in (self.fd, self.sd, self.td, self.pd, self.ld, self.wd) if b is not None]

    def poison(self):
        L = _L()
        for b in (self.pd, self.ld, self.wd):
            L.check(L.load().ofc_memset(0, C.c_void_p(b.ptr), 0x55, b.nbytes))
        if self.alias:
            self.pd.upload(self.seeds)

    def call(self, keep, ppl, **kw):
        a = dict(flow=self.fd.ptr, state=self.td.ptr if self.td else None, W=self.W, H=self.H, n=self.n,
                 seeds=self.pd.ptr if self.alias else self.sd.ptr, P=self.P, keep=keep, ppl=ppl, pos=self.pd.ptr, len=self.ld.ptr,
                 why=self.wd.ptr)
        a.update(kw)
        v = lambda p: C.c_void_p(p) if p else None                                # noqa: E731
        return _L().load().ofc_traj_dev(0, v(a["flow"]), v(a["state"]), a["W"], a["H"], a["n"], v(a["seeds"]), a["P"], a["keep"], a["ppl"],
                                        v(a["pos"]), v(a["len"]), v(a["why"]))

    def run(self, keep, ppl):
        self.poison()
        _L().check(self.call(keep, ppl))
        return self.outputs()

    def outputs(self):
        return (self.pd.download((self.n + 1, self.P, 2), np.int32), self.ld.download((self.P,), np.int32),
                self.wd.download((self.P,), np.uint8))

    def inputs_unchanged(self):
        assert np.array_equal(self.fd.download(self.flow.shape, np.uint32), self.flow.view(np.uint32))
        assert np.array_equal(self.sd.download(self.seeds.shape, np.int32), self.seeds)
        if self.td:
            assert np.array_equal(self.td.download(self.state.shape, np.uint8), self.state)

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("case", TC.CASES, ids=repr)
def test_device_buffers_equal_the_reference_at_every_chunk(case):
    d = Dev(case.flow, case.seeds, case.state)
    try:
        for ppl in TC.chunks(case.shape[0]):
            same(d.run(case.keep, ppl), case.reference())
        d.inputs_unchanged()
    finally:
        d.free()


@pytest.mark.parametrize("P", TC.POINT_COUNTS)
def test_point_counts_around_the_wave_and_the_work_group(P):
    case = TC.BY_NAME["smooth-17x13-n7-keep-0"]
    seeds = np.ascontiguousarray(np.resize(case.seeds[::3], (P, 2)))
    want = TC.reference(case.flow, seeds, case.state, case.keep)
    for state in (case.state, None):
        d = Dev(case.flow, seeds, state)
        try:
            for ppl in (0, 1, 3):
                same(d.run(case.keep, ppl), want if state is not None else TC.reference(case.flow, seeds))
        finally:
            d.free()


def test_more_points_than_the_device_holds_lanes():
    case = TC.MANY()
    want = case.reference()
    d = Dev(case.flow, case.seeds, case.state)
    try:
        for ppl in (0, 1, 3):
            same(d.run(case.keep, ppl), want)
        d.inputs_unchanged()
    finally:
        d.free()
    assert _T().launch_geometry(64, 48, 3, len(case.seeds))[0] == min(3, TC.DENSE_PAIRS)


@pytest.mark.parametrize("name", ("smooth-17x13-n7-keep-01", "edges-12x10-n3", "degenerate-1x1-n1"))
def test_seeds_may_be_row_0_of_the_table(name):
    case = TC.BY_NAME[name]
    d = Dev(case.flow, case.seeds, case.state, alias=True)
    try:
        for ppl in (0, 1, 2):
            same(d.run(case.keep, ppl), case.reference())
    finally:
        d.free()


@pytest.mark.parametrize("case", [TC.BY_NAME[n] for n in ("smooth-64x48-n5", "smooth-17x13-n7-keep-012", "edges-12x10-n3",
                                                          "validity-40x7-n1", "degenerate-9x1-n9-state")], ids=repr)
def test_host_buffers_and_follow(case):
    L, T = _L(), _T()
    n, H, W = case.shape
    P = len(case.seeds)
    pos, length, why = np.full((n + 1, P, 2), 0x55555555, np.int32), np.full(P, -1, np.int32), np.full(P, 0x55, np.uint8)
    flow, seeds = case.flow.copy(), case.seeds.copy()
    L.check(L.load().ofc_traj(0, L.ptr(flow), L.ptr(case.state), W, H, n, L.ptr(seeds), P, case.keep, 2, L.ptr(pos), L.ptr(length),
                              L.ptr(why)))
    same((pos, length, why), case.reference())
    assert np.array_equal(flow.view(np.uint32), case.flow.view(np.uint32)) and np.array_equal(seeds, case.seeds)
    for ppl in (0, 1):
        tr = T.follow(case.flow, case.seeds, state=case.state, keep=case.keep, pairs_per_launch=ppl)
        same((tr.pos, tr.length, tr.why), case.reference())
    if case.state is not None and case.name.startswith("smooth"):
        tr = T.follow(case.flow, case.seeds, state=case.state, keep=(0, 1, 2))
        same((tr.pos, tr.length, tr.why), case.reference())
    assert tr.alive()[0] == P and tr.alive()[-1] == int((tr.why == T.RAN).sum())


def test_follow_defaults_to_the_grid_and_takes_one_field():
    T = _T()
    case = TC.BY_NAME["smooth-64x48-n5"]
    tr = T.follow(case.flow, step=4)
    seeds = T.grid_seeds(64, 48, 4)
    assert len(seeds) == 16 * 12
    same((tr.pos, tr.length, tr.why), TC.reference(case.flow, seeds))
    one = T.follow(case.flow[0], seeds)
    same((one.pos, one.length, one.why), TC.reference(case.flow[:1], seeds))
    with pytest.raises(ValueError, match="state"):
        T.follow(case.flow, seeds, state=np.zeros((5, 48, 63), np.uint8))
    with pytest.raises(ValueError, match="seeds"):
        T.follow(case.flow, np.zeros((0, 2), np.int32))


def test_every_refusal_leaves_the_outputs_alone():
    L = _L()
    lib = L.load()
    case = TC.BY_NAME["smooth-17x13-n7-keep-0"]
    n, H, W = case.shape
    d = Dev(case.flow, case.seeds, case.state)
    try:
        assert d.call(1, 0) == L.OFC_OK
        d.poison()
        bad = lambda **kw: d.call(kw.pop("keep", 1), kw.pop("ppl", 0), **kw)            # noqa: E731
        for kw in (dict(flow=None), dict(seeds=None), dict(pos=None), dict(len=None), dict(why=None), dict(flow=d.fd.ptr + 4),
                   dict(seeds=d.sd.ptr + 4), dict(pos=d.pd.ptr + 4), dict(len=d.ld.ptr + 2), dict(W=0), dict(H=0), dict(n=0),
                   dict(n=65536), dict(P=0), dict(P=(1 << 28) + 1), dict(keep=-1), dict(keep=65536), dict(ppl=-1),
                   dict(seeds=d.pd.ptr + 8)):                                       # inside the table but not its row 0
            assert bad(**kw) == L.OFC_EINVAL, kw
        assert d.call(1, 0, W=16385) == L.OFC_EUNSUPPORTED and d.call(1, 0, H=16385) == L.OFC_EUNSUPPORTED
        for got in d.outputs():
            assert (got.view(np.uint8) == 0x55).all()
        host = np.full(64, 0x55, np.uint8)
        assert lib.ofc_traj(0, None, None, W, H, n, L.ptr(host), 1, 1, 0, L.ptr(host), L.ptr(host), L.ptr(host)) == L.OFC_EINVAL
        assert lib.ofc_traj(0, L.ptr(case.flow), None, W, H, n, L.ptr(case.seeds), 4, 65536, 0, L.ptr(host), L.ptr(host),
                            L.ptr(host)) == L.OFC_EINVAL
        assert (host == 0x55).all()
        ms = C.c_float(-1.0)
        bench = lambda **kw: lib.ofc_bench_traj(0, C.c_void_p(d.fd.ptr), W, H, kw.get("n", n), C.c_void_p(kw.get("seeds", d.sd.ptr)),  # noqa: E731
                                                kw.get("P", d.P), kw.get("ppl", 0), kw.get("iters", 2), C.byref(ms))
        assert bench(n=0) == L.OFC_EINVAL and bench(P=0) == L.OFC_EINVAL and bench(ppl=-1) == L.OFC_EINVAL
        assert bench(iters=0) == L.OFC_EINVAL and bench(seeds=None) == L.OFC_EINVAL and ms.value == -1.0
        for ppl in (0, 1):
            L.check(bench(ppl=ppl))
            assert ms.value > 0
        d.inputs_unchanged()
    finally:
        d.free()


# ---- ClipPipeline and FlowStream: 64x48 frames, the engine's default parameters ----
PW, PH, ST = 64, 48, 9
STRICT = dict(tau=2.0, kappa=0.25)
REPAIR = dict(radius=1, rounds=3, min_count=2)


def gray_clip(n):
    from tests import motion_grid_cases as MC
    return np.ascontiguousarray(MC.moving_blobs_clip(n, PW, PH)[..., 0])


@pytest.fixture(scope="module")
def clip():
    """nine frames and the seeds every test below follows: once, read-only"""
    frames = gray_clip(ST)
    seeds = np.concatenate([_T().grid_seeds(PW, PH, 4), TC.spread_seeds(PW, PH, 8, extra=32)[::7]])
    for a in (frames, seeds):
        a.setflags(write=False)
    return SimpleNamespace(frames=frames, seeds=seeds)


def test_pipeline_trajectories_equal_follow_on_its_field(clip):
    from opticalflowclustering_amd.pipeline import ClipPipeline
    T = _T()
    pipe = ClipPipeline(PW, PH, ST, batch_pairs=3)
    try:
        pipe.upload_frames(clip.frames)
        pipe.run_flow()
        field = pipe.flows_host()
        n = ST - 1
        for kw, sl in ((dict(), slice(0, n)), (dict(start=2), slice(2, n)), (dict(start=1, length=4), slice(1, 5)),
                       (dict(start=n - 1), slice(n - 1, n)), (dict(length=1), slice(0, 1))):
            got = pipe.trajectories(clip.seeds, **kw)
            want = T.follow(field[sl], clip.seeds)
            same((got.pos, got.length, got.why), (want.pos, want.length, want.why))
            same((got.pos, got.length, got.why), TC.reference(field[sl], clip.seeds))
        grid = pipe.trajectories(step=8)
        same((grid.pos, grid.length, grid.why), TC.reference(field, T.grid_seeds(PW, PH, 8)))
        assert np.array_equal(pipe.flows_host().view(np.uint32), field.view(np.uint32))
        for bad in (dict(start=-1), dict(start=n), dict(length=0), dict(start=3, length=n - 2)):
            with pytest.raises(ValueError, match="range"):
                pipe.trajectories(clip.seeds, **bad)
        with pytest.raises(ValueError, match="consistency"):                       # no state map yet
            pipe.trajectories(clip.seeds, consistent=True)
        ph = pipe.photometric(**STRICT)
        assert len(set(ph.state.ravel().tolist())) >= 2
        for keep, kw in (((0,), dict()), ((0, 2), dict(start=3, length=4))):
            sl = slice(kw.get("start", 0), kw.get("start", 0) + kw.get("length", n))
            got = pipe.trajectories(clip.seeds, consistent=True, keep=keep, **kw)
            want = T.follow(field[sl], clip.seeds, state=ph.state[sl], keep=keep)
            same((got.pos, got.length, got.why), (want.pos, want.length, want.why))
            same((got.pos, got.length, got.why), TC.reference(field[sl], clip.seeds, ph.state[sl], TC.keep_mask(keep)))
            assert (got.why == T.UNTRUSTED).any()
        assert np.array_equal(pipe.state.download((n, PH, PW), np.uint8), ph.state)
        pipe.compensate_camera("translation")
        with pytest.raises(ValueError, match="compensate_camera"):
            pipe.trajectories(clip.seeds)
    finally:
        pipe.close()


def _stream(batch_pairs, **kw):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(PW, PH, batch_pairs=batch_pairs, rows=2, cols=3, **kw)


def _run(st, frames):
    for f in frames:
        st.push(f)
    return st.finish()


def staged(frames, seeds, use_state, repair):
    """the staged route: the engine's pairwise fields, the photometric check, the repair, then follow on host arrays"""
    from opticalflowclustering_amd import photometric, repair as R
    from opticalflowclustering_amd.flow import FlowEngine
    eng = FlowEngine(PW, PH, max_batch=1)
    try:
        fields = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    finally:
        eng.close()
    state = photometric.check(frames, fields, **STRICT).state
    if repair:
        fixed = R.fill(fields, state, **REPAIR)
        fields, state = fixed.flow, fixed.state
    return _T().follow(fields, seeds, state=state if use_state else None)


@pytest.mark.parametrize("use_state,repair", ((False, False), (True, False), (True, True)))
def test_stream_trajectories_equal_the_staged_route_whatever_the_batches(clip, use_state, repair):
    want = staged(clip.frames, clip.seeds, use_state, repair)
    assert set(want.length.tolist()) >= {0, ST - 1} and (not use_state or (want.why == 1).any())
    kw = dict(photometric=STRICT, repair=REPAIR if repair else None, trajectories=dict(seeds=clip.seeds, use_state=use_state))
    for batch in (3, 8):                                                         # 3 + 3 and a flush of 2; one full batch
        st = _stream(batch, **kw)
        try:
            cells = _run(st, clip.frames)
            got = st.trajectories()
            same((got.pos, got.length, got.why), (want.pos, want.length, want.why))
            assert np.array_equal(st.trajectories().pos, got.pos)                # still there until frames arrive
            if batch == 3:
                plain = _stream(batch, **dict(kw, trajectories=None))            # nothing else depends on the stage
                assert np.array_equal(_run(plain, clip.frames).view(np.uint32), cells.view(np.uint32))
                plain.close()
                st.set_camera("translation")                                     # the points land by the whole flow
                _run(st, clip.frames)
                again = st.trajectories()
                same((again.pos, again.length, again.why), (want.pos, want.length, want.why))
                st.set_camera(None)
                _run(st, clip.frames[:5])                                        # a second, shorter clip reseeds
                short = st.trajectories()
                assert short.n_pairs == 4 and np.array_equal(short.pos, want.pos[:5])
                assert np.array_equal(short.length, np.minimum(want.length, 4))
                assert np.array_equal(short.why, np.where(want.length >= 4, 0, want.why))
        finally:
            st.close()


def test_stream_set_traj_and_read_traj_refusals(clip):
    L = _L()
    lib = L.load()
    P = len(clip.seeds)
    st = _stream(3)
    try:
        pos, ln, why = np.full((ST, P, 2), 0x55555555, np.int32), np.full(P, 0x55555555, np.int32), np.full(P, 0x55, np.uint8)
        read = lambda max_pairs: lib.ofc_stream_read_traj(st._h, L.ptr(pos), L.ptr(ln), L.ptr(why), max_pairs)     # noqa: E731
        assert read(ST) == L.OFC_EINVAL and "no trajectories" in lib.ofc_last_error().decode()
        seeds = np.ascontiguousarray(clip.seeds)
        assert lib.ofc_stream_set_traj(st._h, P, None, 0) == L.OFC_EINVAL
        assert lib.ofc_stream_set_traj(st._h, -1, L.ptr(seeds), 0) == L.OFC_EINVAL
        assert lib.ofc_stream_set_traj(st._h, (1 << 28) + 1, L.ptr(seeds), 0) == L.OFC_EINVAL
        assert lib.ofc_stream_set_traj(st._h, P, L.ptr(seeds), 1) == L.OFC_EINVAL       # use_state without a check
        assert "check" in lib.ofc_last_error().decode()
        assert lib.ofc_stream_set_traj(None, P, L.ptr(seeds), 0) == L.OFC_EINVAL and lib.ofc_stream_read_traj(None, None, None, None, 0) == L.OFC_EINVAL
        assert read(ST) == L.OFC_EINVAL                                              # the refusals set nothing
        with pytest.raises(ValueError, match="check"):
            st.set_trajectories(seeds=clip.seeds, use_state=True)
        st.set_trajectories(seeds=clip.seeds)
        assert st.traj_points == P
        st.push(clip.frames[0])
        for call in (lambda: st.set_trajectories(step=4), lambda: st.set_trajectories(on=False), st.trajectories):
            with pytest.raises(ValueError, match="holds frames"):                 # in mid-clip: refused, nothing changes
                call()
        for f in clip.frames[1:6]:
            st.push(f)
        st.finish()
        assert read(4) == L.OFC_EINVAL                                               # five pairs were delivered: too small
        assert (pos == 0x55555555).all() and (ln == 0x55555555).all() and (why == 0x55).all()
        assert read(5) == L.OFC_OK and np.array_equal(pos[0], clip.seeds) and (pos[6:] == 0x55555555).all()
        st.set_trajectories(on=False)
        assert st.traj_points == 0
        with pytest.raises(ValueError, match="no trajectories"):
            st.trajectories()
        grid = _stream(3, trajectories=True)
        assert grid.traj_points == len(_T().grid_seeds(PW, PH, 8))
        grid.close()
    finally:
        st.close()


def test_motion_grids_trajectories_on_the_three_routes(clip, tmp_path):
    from opticalflowclustering_amd import motionGrids as G
    names = ("clip.npy", "model.npy", "res.csv", "stream.csv", "fit.csv", "res.npz", "stream.npz", "fit.npz")
    clip_path, model, res_csv, stream_csv, fit_csv, res, stream, fit = (str(tmp_path / n) for n in names)
    np.save(clip_path, clip.frames)
    np.save(model, np.array([[0.0, 0.0], [3.0, 0.0], [0.0, -2.0]]))
    base = ["--path", clip_path, "-c", "3", "--rows", "2", "--cols", "3", "--traj-step", "4"]
    G.main(base + ["-f", res_csv, "--init", model, "--trajectories", res])
    G.main(base + ["-f", stream_csv, "--model", model, "--stream", "--batch-pairs", "3", "--trajectories", stream])
    G.main(base + ["-f", fit_csv, "--fit-stream", "--hist-bins", "256", "--hist-range", "8", "--trajectories", fit])
    want = staged(clip.frames, _T().grid_seeds(PW, PH, 4), False, False)
    for path in (res, stream, fit):
        got = np.load(path)
        same((got["pos"], got["length"], got["why"]), (want.pos, want.length, want.why))
    with pytest.raises(SystemExit):
        G.main(base[:-2] + ["-f", res_csv, "--init", model, "--traj-step", "4"])
