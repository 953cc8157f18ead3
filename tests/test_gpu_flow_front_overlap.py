"""The flow engine's front end beside the level-0 expansion: with the overlap on, the level images and
expansions of the coarse pyramid levels run on a side stream while the engine's own stream runs the level-0 front end, and
every level's iterations wait for that level's event.  The same kernels run with the same arguments in either order, so
EVERY comparison here is np.array_equal: overlap on against overlap off (OFC_FLOW_FRONT_OVERLAP=0 in the environment when
the engine is created), and both against the table of single pairs from a serial max_batch = 1 engine.

What the orders can get wrong is ordering, not arithmetic: a coarse level's R overwritten by the next call while the previous
call's iterations still read it, frames read before their copy has landed, an iteration started before its level's expansion,
a result handed out before the side stream is joined.  Hence calls in a row without a synchronisation between them, two
engines, and the host entry points (whose copies share the engine's stream) mixed with the device one.

The clips.  All cases the overlap was specified with run on the 160 x 96 clip of flow_sequence_cases.py.  At the default
parameters that clip has ONE coarse level (80 x 48: cv2's rule drops a level below 32 pixels a side, and 96 / 4 = 24), built by
the exact 2:1 decimation and expanded after it; test_pyramids_of_the_clips pins that down.  One coarse level means one event
and no chain on the side stream, so a second clip is added: 256 x 256, the smallest frame whose pyramid has three coarse levels
(128, 64, 32 a side), each an exact 2:1 / 4:1 / 8:1 decimation of a frame with dword-addressable rows, which is what
level_image_plan asks of the three decimation kernels.  162 x 98 takes the general level-image kernel for its coarse level
(rows not dword-addressable); its level 0 still reads the u8 frames, so the engine that builds a level-0 image first
(OFC_FLOW_STAGED=1, which also runs the staged iteration kernels) is tested beside it."""
import contextlib
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import flow_sequence_cases as S
from opticalflowclustering_amd import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF           # buffers are prefilled with 0xFF bytes (as float32: a NaN no kernel produces)
ENGINE_ENV = ("OFC_FLOW_FRONT_OVERLAP", "OFC_FLOW_GRAPH", "OFC_FLOW_STAGED")    # all read by ofc_flow_create
DEEP_W = DEEP_H = 256
DEEP_FRAMES, DEEP_MAX_BATCH = 5, 3
DEEP_WINDOWS = ((0, 3, False), (2, 1, True), (1, 3, True), (3, 1, False), (0, 2, False))
ODD_W, ODD_H = 162, 98


def _lib():
    from opticalflowclustering_amd import _lib
    return _lib


@contextlib.contextmanager
def _env(**kw):
    """the engine switches as given (None / absent: unset) while an engine is created, the caller's values after it"""
    old = {k: os.environ.get(k) for k in ENGINE_ENV}
    try:
        for k in ENGINE_ENV:
            if kw.get(k) is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = kw[k]
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(W, H, overlap, params=None, max_batch=1, expect=None, **env):
    """an engine created with the overlap allowed (OFC_FLOW_FRONT_OVERLAP=1, which says what unset says) or forced off (=0);
    `expect`: what the query must report when that is not simply `overlap` (an engine that may overlap and declines)"""
    from opticalflowclustering_amd.flow import FlowEngine
    with _env(OFC_FLOW_FRONT_OVERLAP="1" if overlap else "0", **env):
        eng = FlowEngine(W, H, params, max_batch=max_batch)
    assert eng.front_overlap() is (overlap if expect is None else expect)
    return eng


def _table(frames, params=None, **env):
    """every consecutive pair on its own, on a fresh serial engine that holds one pair"""
    eng = _engine(frames.shape[2], frames.shape[1], False, params, **env)
    out = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    eng.close()
    out.setflags(write=False)
    return out


def _clip(W, H, n):
    """flow_sequence_cases.clip's recipe at another size"""
    p = synth.texture_params(S.TEXTURE_SEED)
    x = y = 0.0
    out = []
    for t in range(n):
        out.append(synth.frame(W, H, x, y, p))
        dx, dy = S.step(t)
        x, y = x + dx, y + dy
    out = np.stack(out)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def ref():
    """the clips and their serial single-pair tables: computed once, shared, read-only"""
    frames = S.clip()
    frames.setflags(write=False)
    r = SimpleNamespace(frames=frames, table=_table(frames), deep=_clip(DEEP_W, DEEP_H, DEEP_FRAMES),
                        odd=_clip(ODD_W, ODD_H, S.SEQ_FRAMES))
    r.deep_table = _table(r.deep)
    assert not np.array_equal(r.table[0], r.table[1])
    return r


def _run(engines, windows, frames, sync, slack):
    """windows (first frame, pairs, _stats?) in order, call i on engines[i % len], synchronised after each call or only at
    the end; the flows land one after the other in a buffer prefilled with 0xFF bytes that has `slack` pairs of room behind
    them, the sums in 16 bytes per window.  -> (flows as uint32, sums as uint64), the slack included"""
    L = _lib()
    Hh, Ww = frames.shape[1:]
    P = Ww * Hh
    n_out = sum(n for _, n, _ in windows) + slack
    fd = L.DeviceBuffer(frames.nbytes).upload(frames)
    out, sums = L.DeviceBuffer(n_out * P * 8), L.DeviceBuffer(len(windows) * 16)
    for b in (out, sums):
        L.check(L.load().ofc_memset(0, C.c_void_p(b.ptr), 0xFF, b.nbytes))
    off = 0
    for i, (f0, n, stats) in enumerate(windows):
        engines[i % len(engines)].calc_frames_dev(fd.ptr + f0 * P, n + 1, out.ptr + off * P * 8, sync=sync,
                                                  uv_sum_ptr=sums.ptr + 16 * i if stats else None)
        off += n
    if len(engines) > 1:
        L.check(L.load().ofc_device_sync(0))            # the one synchronisation of the two-engine case
    else:
        engines[0].sync()
    got = out.download((n_out, Hh, Ww, 2), np.uint32), sums.download((len(windows), 2), np.uint64)
    for b in (fd, out, sums):
        b.free()
    return got


def _model(windows, table, slack):
    """what _run's flow buffer holds when every call wrote its own pairs and nothing else"""
    rows = [table[f0:f0 + n].view(np.uint32) for f0, n, _ in windows]
    return np.concatenate(rows + [np.full((slack,) + table.shape[1:], SENTINEL, np.uint32)])


def _assert_on_equals_off(on, off, windows, table, slack):
    flows_on, sums_on = on
    flows_off, sums_off = off
    assert np.array_equal(flows_on, flows_off)
    assert np.array_equal(sums_on, sums_off)
    assert np.array_equal(flows_on, _model(windows, table, slack))          # the slack behind the flows included
    for i, (_, _, stats) in enumerate(windows):
        assert stats != (sums_on[i] == 0xFFFFFFFFFFFFFFFF).all(), i         # written where asked for, untouched elsewhere


def _both_orders(W, H, windows, frames, table, sync, max_batch, params=None, expect=None, **env):
    got = []
    for overlap in (True, False):
        eng = _engine(W, H, overlap, params, max_batch, expect=expect if overlap else None, **env)
        got.append(_run([eng], windows, frames, sync, max_batch))
        eng.close()
    _assert_on_equals_off(got[0], got[1], windows, table, max_batch)


def _level_size(gray, k, params=None):
    """(rc, w, h) of pyramid level k through ofc_level_image, which refuses a level the pyramid does not have"""
    L = _lib()
    Hh, Ww = gray.shape
    out = np.empty((Hh, Ww), np.float32)
    w, h = C.c_int(-1), C.c_int(-1)
    p = params or L.FbParams()
    rc = L.load().ofc_level_image(0, L.ptr(np.ascontiguousarray(gray)), Ww, Hh, C.byref(p), k, L.ptr(out), C.byref(w), C.byref(h))
    return rc, w.value, h.value


def test_pyramids_of_the_clips(ref):
    """160 x 96 at the defaults: 80 x 48 and no further level (not the four levels a 0.5 pyramid of 3 would have without
    cv2's 32-pixel rule); 256 x 256: 128, 64, 32; 162 x 98: 81 x 49; 160 x 96 at pyr_scale 0.8 with 4 levels: all four"""
    L = _lib()
    assert _level_size(ref.frames[0], 1) == (L.OFC_OK, 80, 48)
    assert _level_size(ref.frames[0], 2)[0] == L.OFC_EINVAL
    assert [_level_size(ref.deep[0], k) for k in (1, 2, 3)] == [(L.OFC_OK, 128, 128), (L.OFC_OK, 64, 64), (L.OFC_OK, 32, 32)]
    assert _level_size(ref.odd[0], 1) == (L.OFC_OK, 81, 49)
    assert _level_size(ref.odd[0], 2)[0] == L.OFC_EINVAL
    p = L.FbParams(pyr_scale=0.8, levels=4)
    assert [_level_size(ref.frames[0], k, p)[1:] for k in (1, 2, 3, 4)] == [(128, 77), (102, 61), (82, 49), (66, 39)]


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
def test_calls_in_a_row(ref, sync):
    """5, 1, 3, 5, 2, 1 pairs on one max_batch = 5 engine, plain and _stats calls alternating: unsynchronised, the side
    stream of call i + 1 must not touch the coarse level's R before the iterations of call i have read it"""
    frames = ref.frames[:S.SEQ_FRAMES]
    _both_orders(S.W, S.H, S.SEQ_WINDOWS, frames, ref.table, sync, S.SEQ_MAX_BATCH)


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
def test_calls_in_a_row_on_three_coarse_levels(ref, sync):
    """256 x 256: the side stream holds a chain of three level images and expansions, and the main stream waits three
    times; calls of 3, 1, 3, 1, 2 pairs on a max_batch = 3 engine"""
    _both_orders(DEEP_W, DEEP_H, DEEP_WINDOWS, ref.deep, ref.deep_table, sync, DEEP_MAX_BATCH)


def test_two_engines_alternate(ref):
    """call i on engine i % 2 over overlapping frame windows, four streams in all, one device synchronisation at the end"""
    frames = ref.frames[:S.SEQ_FRAMES]
    got = []
    for overlap in (True, False):
        engines = [_engine(S.W, S.H, overlap, max_batch=S.SEQ_MAX_BATCH) for _ in range(2)]
        got.append(_run(engines, S.SEQ_WINDOWS, frames, False, S.SEQ_MAX_BATCH))
        for e in engines:
            e.close()
    _assert_on_equals_off(got[0], got[1], S.SEQ_WINDOWS, ref.table, S.SEQ_MAX_BATCH)


MIXED_WINDOWS = ((0, 5, False), (3, 5, True), (6, 1, False))       # the device calls of _mixed


def _mixed(ref, overlap):
    """calc, grey pushes and the device calls of MIXED_WINDOWS, unsynchronised, on one engine; every host result is held to
    the table on the spot -> (the device calls' flows as uint32, the one _stats call's sums as uint64)"""
    L = _lib()
    g, t = ref.frames, ref.table
    P = S.W * S.H
    eng = _engine(S.W, S.H, overlap, max_batch=S.SEQ_MAX_BATCH)
    fd = L.DeviceBuffer(g.nbytes).upload(g)
    out, sums = L.DeviceBuffer((11 + S.SEQ_MAX_BATCH) * P * 8), L.DeviceBuffer(16)
    for b in (out, sums):
        L.check(L.load().ofc_memset(0, C.c_void_p(b.ptr), 0xFF, b.nbytes))
    assert eng.push(g[0]) is None
    eng.calc_frames_dev(fd.ptr, 6, out.ptr, sync=False)
    assert np.array_equal(eng.calc(g[15], g[16]), t[15])
    assert np.array_equal(eng.push(g[1]), t[0])
    eng.calc_frames_dev(fd.ptr + 3 * P, 6, out.ptr + 5 * P * 8, sync=False, uv_sum_ptr=sums.ptr)
    assert np.array_equal(eng.push(g[2]), t[1])
    eng.calc_frames_dev(fd.ptr + 6 * P, 2, out.ptr + 10 * P * 8, sync=False)
    assert np.array_equal(eng.calc(g[7], g[8]), t[7])
    assert np.array_equal(eng.push(g[3]), t[2])
    eng.sync()
    got = out.download((11 + S.SEQ_MAX_BATCH, S.H, S.W, 2), np.uint32), sums.download((1, 2), np.uint64)
    eng.close()
    for b in (fd, out, sums):
        b.free()
    return got


def test_mixed_entry_points(ref):
    """the host entry points copy their frames on the engine's stream, which the side stream has to be ordered behind, and
    read the result back on it, while device calls before and after them are still in flight"""
    on, off = _mixed(ref, True), _mixed(ref, False)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert np.array_equal(on[0], _model(MIXED_WINDOWS, ref.table, S.SEQ_MAX_BATCH))
    assert not (on[1] == 0xFFFFFFFFFFFFFFFF).any()


@pytest.mark.parametrize("staged", [False, True], ids=["fused", "staged"])
def test_size_off_the_fast_paths(ref, staged):
    """162 x 98: the general level-image kernel on the side stream.  staged: OFC_FLOW_STAGED=1, the engine that builds a
    level-0 image before the expansion (two launches on the main stream beside the side chain, and a level-0 slice of I)
    and runs the staged iteration kernels behind the same events"""
    env = dict(OFC_FLOW_STAGED="1") if staged else {}
    table = _table(ref.odd, **env)
    _both_orders(ODD_W, ODD_H, S.SEQ_WINDOWS, ref.odd, table, False, S.SEQ_MAX_BATCH, **env)


def test_memory_rule_keeps_a_deep_pyramid_serial(ref):
    """pyr_scale 0.8 with 4 levels: slices per level would take 2.3 x the shared buffers (R alone 2.5 x), so an engine that
    may overlap reports the serial order and computes the table; at the default parameters (1.08 x) it reports the
    overlap, with the switch set to 1 and with no switch at all"""
    L = _lib()
    frames = ref.frames[:S.SEQ_FRAMES]
    p = L.FbParams(pyr_scale=0.8, levels=4)
    table = _table(frames, p)
    assert not np.array_equal(table, ref.table[:S.SEQ_FRAMES - 1])
    _both_orders(S.W, S.H, S.SEQ_WINDOWS, frames, table, False, S.SEQ_MAX_BATCH, params=p, expect=False)
    _engine(S.W, S.H, True, max_batch=S.SEQ_MAX_BATCH).close()              # asserts that the query says on
    _engine(DEEP_W, DEEP_H, True, max_batch=DEEP_MAX_BATCH).close()         # three coarse levels at 0.5: 1.16 x
    from opticalflowclustering_amd.flow import FlowEngine
    with _env():                                                            # no switch set: the default engine
        eng = FlowEngine(S.W, S.H, max_batch=S.SEQ_MAX_BATCH)
    assert eng.front_overlap() is True
    eng.close()


def test_graph_path_stays_serial(ref):
    """OFC_FLOW_GRAPH=1: a capture must not acquire parallel branches, so the engine reports the serial order; four
    identical calls (direct, direct, capture, replay) give the table"""
    L = _lib()
    P = S.W * S.H
    frames = ref.frames[:S.SEQ_MAX_BATCH + 1]
    eng = _engine(S.W, S.H, True, max_batch=S.SEQ_MAX_BATCH, expect=False, OFC_FLOW_GRAPH="1")
    fd = L.DeviceBuffer(frames.nbytes).upload(frames)
    out = L.DeviceBuffer(S.SEQ_MAX_BATCH * P * 8)
    for call in range(4):
        L.check(L.load().ofc_memset(0, C.c_void_p(out.ptr), 0xFF, out.nbytes))
        eng.calc_frames_dev(fd.ptr, S.SEQ_MAX_BATCH + 1, out.ptr)
        assert np.array_equal(out.download((S.SEQ_MAX_BATCH, S.H, S.W, 2), np.float32), ref.table[:S.SEQ_MAX_BATCH]), call
    eng.close()
    for b in (fd, out):
        b.free()
