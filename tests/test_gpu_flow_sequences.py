"""The flow engine (ofc_flow_*) and the streaming ingest (ofc_stream_*) across SEQUENCES of calls on one handle: the kept
previous frame, the two pinned slots and their one-frame overlap, pairs_done, reuse after finish, the growing result
buffer, scratch sized by one call and reused by the next, two handles side by side.  What a single call computes is held to
the oracle elsewhere (test_gpu_flow*.py); here every result is compared with what the same pair gives on its own.

References and bars (tests/flow_sequence_cases.py; the clips' fitness is asserted on the CPU, test_oracle_flow_sequences.py):
  1. anchor: three pairs of the 160 x 96 clip (first, middle, last) on a fresh max_batch = 1 engine against the CPU oracle,
     at test_gpu_flow.py's bars rel <= 1e-4 and max|d| <= 1e-3 px, with a margin of at least 2 x.  Size used: 160 x 96.
     Measured there on an MI355X: rel 2.3e-7 / 6.8e-8 / 5.8e-8, max|d| 2.1e-6 / 9.5e-7 / 1.2e-6 px, a margin of 430 x and
     more, so no larger size was needed.
  2. every batched, pushed or streamed flow is BIT-EQUAL to FlowEngine.calc(frame[t], frame[t + 1]) of that fresh engine (the
     table, computed once per module): batch independence is the project's established property
     (test_batched_device_path_equals_pairwise).
  3. a stream's cell mean: |got - want| <= spacing(float32(|want|)) + 2^-40 * mean|x|, want = the float64 block mean of the
     table's flow: the kernel sums in float64 and rounds once (test_grid_cell_mean_flow_grids).
  4. _stats sums: <= 1e-9 * max(1, |want|) against the float64 sum of the stored field.
Nothing runs under HIP-graph capture (OFC_FLOW_GRAPH stays unset)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import flow_sequence_cases as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF           # a buffer prefilled with 0xFF bytes, read as uint32 (as float32: a NaN no kernel produces)


def _lib():
    from opticalflowclustering_amd import _lib
    return _lib


def _pairwise(frames, params=None):
    """the reference of bar 2: every consecutive pair on its own, on a fresh engine that holds one pair"""
    from opticalflowclustering_amd.flow import FlowEngine
    Hh, Ww = frames.shape[1:]
    eng = FlowEngine(Ww, Hh, params, max_batch=1)
    out = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    eng.close()
    out.setflags(write=False)
    return out


def _cells(table, grid):
    c = SimpleNamespace(mean=np.stack([S.cell_means(f, *grid) for f in table]),
                        bar=np.stack([S.cell_mean_bar(f, *grid) for f in table]))
    c.mean.setflags(write=False)
    c.bar.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def ref():
    """the clip, its pairwise table and the table's cell means and bars: computed once, shared, read-only"""
    frames = S.clip()
    frames.setflags(write=False)
    table = _pairwise(frames)
    r = SimpleNamespace(frames=frames, table=table, cells={g: _cells(table, g) for g in (S.GRID, S.FINE_GRID)}, other={})
    for g in (S.GRID, S.FINE_GRID):                     # on the reference table itself, so that bar 3 stays meaningful
        assert min(S.cancellation(f, *g) for f in table) >= S.CANCEL_FLOOR
        assert S.min_pair_distance(r.cells[g].mean) > S.DISTINCT_PX
    return r


def _table_for(ref, name, frames, **kw):
    """pairwise table of `frames` at other parameters, computed once per module"""
    if name not in ref.other:
        ref.other[name] = _pairwise(frames, _lib().FbParams(**kw))
    return ref.other[name]


def _assert_rows(cells, want, where=""):
    """cells (n, rows*cols, 2) float32 from a stream against the table's cell means `want` (.mean, .bar of the same rows)"""
    assert cells.dtype == np.float32 and cells.shape == want.mean.shape, (where, cells.shape, want.mean.shape)
    err = np.abs(cells.astype(np.float64) - want.mean)
    bad = np.argwhere(err > want.bar)
    assert len(bad) == 0, (where, "first bad (row, cell, uv)", bad[0].tolist(), float(err[tuple(bad[0])]),
                           float(want.bar[tuple(bad[0])]), "rows", sorted({int(b[0]) for b in bad}))


def _rows(c, lo, hi):
    return SimpleNamespace(mean=c.mean[lo:hi], bar=c.bar[lo:hi])


def _push_all(st, frames, B):
    """push every frame; B: pairs_done never decreases, is never negative and never exceeds the pairs whose batch has been
    submitted, B * floor((pushes - 1) / B).  How far it lags is timing and is not asserted."""
    last = 0
    for i, f in enumerate(frames):
        done = st.push(f)
        assert 0 <= last <= done <= B * (i // B), (i, last, done)
        last = done
    return last


def _stream(B, grid=S.GRID, params=None, W=S.W, H=S.H):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(W, H, batch_pairs=B, rows=grid[0], cols=grid[1], params=params)


def _raw_finish(st, buf, max_pairs):
    """ofc_stream_finish itself -> (rc, n_pairs, message); FlowStream.finish always brings a large enough buffer"""
    L = _lib()
    n = C.c_int(-7)
    rc = L.load().ofc_stream_finish(st._h, L.ptr(buf), max_pairs, C.byref(n))
    st.pushed = 0
    return rc, n.value, L.load().ofc_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------
# 1. anchor
# ---------------------------------------------------------------------------------------------------------------------
def test_table_is_anchored_to_the_oracle(ref):
    """pairs 0 / 11 / 22 at 160 x 96.  Measured on an MI355X: rel 2.3e-7 / 6.8e-8 / 5.8e-8 (margin 430 x / 1463 x / 1725 x),
    max|d| 2.1e-6 / 9.5e-7 / 1.2e-6 px (473 x / 1049 x / 839 x); the margin has to be at least 2 x"""
    for t in S.ANCHOR_PAIRS:
        want = O.farneback(ref.frames[t], ref.frames[t + 1])
        r, a = S.rel(ref.table[t], want), float(np.abs(ref.table[t] - want).max())
        print(f"anchor pair {t}: rel {r:.3e} (margin {S.ANCHOR_REL / max(r, 1e-30):.0f}x), "
              f"max abs {a:.3e} px (margin {S.ANCHOR_ABS / max(a, 1e-30):.0f}x)")
        assert r * S.ANCHOR_MARGIN <= S.ANCHOR_REL, (t, r)
        assert a * S.ANCHOR_MARGIN <= S.ANCHOR_ABS, (t, a)


# ---------------------------------------------------------------------------------------------------------------------
# A, B. stream lengths, slot cycling, pairs_done
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", S.STREAM_CASES, ids=[f"B{B}-T{T}" for B, T in S.STREAM_CASES])
def test_stream_lengths_and_slot_cycling(ref, B, T):
    st = _stream(B)
    _push_all(st, ref.frames[:T], B)
    cells = st.finish()
    st.close()
    _assert_rows(cells, _rows(ref.cells[S.GRID], 0, T - 1), f"B={B} T={T}")


def test_stream_fine_grid(ref):
    """14 x 25 cells of 6 x 6 px; 12 rows and 10 columns of remainder ignored"""
    B, T = 3, 11
    st = _stream(B, S.FINE_GRID)
    _push_all(st, ref.frames[:T], B)
    cells = st.finish()
    st.close()
    _assert_rows(cells, _rows(ref.cells[S.FINE_GRID], 0, T - 1))


def test_stream_staged_window(ref):
    """winsize 31: the staged kernels behind the same slots"""
    B, T = 3, 8
    tab = _table_for(ref, "ws31", ref.frames[:T], winsize=31)
    want = _cells(tab, S.GRID)
    assert min(S.cancellation(f, *S.GRID) for f in tab) >= S.CANCEL_FLOOR
    assert not np.array_equal(tab, ref.table[:T - 1])
    st = _stream(B, params=_lib().FbParams(winsize=31))
    _push_all(st, ref.frames[:T], B)
    cells = st.finish()
    st.close()
    _assert_rows(cells, want)


@pytest.mark.parametrize("B,T", [(1, 4), (3, 1), (3, 7), (3, 9), (7, 3)])
def test_stream_pairs_done_and_n_pairs(ref, B, T):
    """B through the C ABI: the bounds of _push_all on every push, a NULL pairs_done accepted, n_pairs = T - 1 after finish
    (pairs_done itself may lag: no assertion on how far)"""
    L = _lib()
    st = _stream(B)
    final = _push_all(st, ref.frames[:T - 1], B) if T > 1 else 0
    assert L.load().ofc_stream_push_gray(st._h, L.ptr(np.ascontiguousarray(ref.frames[T - 1])), None) == L.OFC_OK
    assert final <= B * ((T - 1) // B)
    buf = np.zeros((max(T - 1, 1), 12, 2), np.float32)
    rc, n, _ = _raw_finish(st, buf, len(buf))
    st.close()
    assert rc == L.OFC_OK and n == T - 1
    _assert_rows(buf[:n], _rows(ref.cells[S.GRID], 0, T - 1))


# ---------------------------------------------------------------------------------------------------------------------
# C. reuse after finish
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T1", [(3, 3), (3, 4), (3, 6), (3, 7), (3, 9), (3, 10), (2, 5), (1, 2), (1, 3), (7, 8)])
def test_stream_reuse_after_finish(ref, B, T1):
    """the first pass ends with its partial batch in slot 0 (T1 <= B, or after an even number of full batches) or in slot 1,
    and with T1 = m * B + 1 exactly the overlap frame is pending; the second pass then holds its own T2 - 1 pairs only: no
    carried frame, no pair across the boundary"""
    s2, T2 = 11, 2 * B + 3
    st = _stream(B)
    _push_all(st, ref.frames[:T1], B)
    first = st.finish()
    _push_all(st, ref.frames[s2:s2 + T2], B)
    second = st.finish()
    third = st.finish()
    st.close()
    _assert_rows(first, _rows(ref.cells[S.GRID], 0, T1 - 1), "first pass")
    _assert_rows(second, _rows(ref.cells[S.GRID], s2, s2 + T2 - 1), "second pass")
    assert third.shape == (0, 12, 2)


# ---------------------------------------------------------------------------------------------------------------------
# D. short output buffer, count-only finish
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(3, 6), (3, 7), (2, 2)])
def test_stream_finish_into_a_short_buffer_can_be_retried(ref, B, T):
    """max_pairs = n - 1: OFC_EINVAL with a message, *n_pairs = n (what to bring), nothing written; the results stay with
    the stream, and the same call with room returns all n pairs (ofc.h)"""
    L = _lib()
    n = T - 1
    st = _stream(B)
    _push_all(st, ref.frames[:T], B)
    buf = np.full((n, 12, 2), np.float32(-77.0))
    rc, got_n, msg = _raw_finish(st, buf, n - 1)
    assert rc == L.OFC_EINVAL and got_n == n and "pairs" in msg
    assert (buf == np.float32(-77.0)).all()
    rc, got_n, _ = _raw_finish(st, buf, n)
    assert rc == L.OFC_OK and got_n == n
    _assert_rows(buf, _rows(ref.cells[S.GRID], 0, n), "retry")
    rc, got_n, _ = _raw_finish(st, buf, n)              # handed over: the stream is empty again
    assert rc == L.OFC_OK and got_n == 0
    _push_all(st, ref.frames[5:5 + B + 2], B)
    cells = st.finish()
    st.close()
    _assert_rows(cells, _rows(ref.cells[S.GRID], 5, 5 + B + 1), "after the retry")


@pytest.mark.parametrize("B,T", [(3, 6), (3, 7)])
def test_stream_count_only_finish_then_a_new_clip(ref, B, T):
    """cell_uv = NULL: the count comes back, the results are dropped, and the next pushes start a new clip"""
    L = _lib()
    st = _stream(B)
    _push_all(st, ref.frames[:T], B)
    rc, n, _ = _raw_finish(st, None, 0)
    assert rc == L.OFC_OK and n == T - 1
    _push_all(st, ref.frames[9:9 + 6], B)
    cells = st.finish()
    st.close()
    _assert_rows(cells, _rows(ref.cells[S.GRID], 9, 14))


# ---------------------------------------------------------------------------------------------------------------------
# E. result-buffer growth
# ---------------------------------------------------------------------------------------------------------------------
def test_stream_result_buffer_growth_keeps_the_rows_before_it():
    """299 pairs, 7 per batch: the buffer of 256 rows grows (synchronise, device copy, swap) when the 37th batch is
    submitted, 252 rows in, in the middle of the slot cycle; those 252 rows are the point"""
    frames = S.grow_clip()
    tab = _pairwise(frames)
    want = _cells(tab, S.GROW_GRID)
    assert S.min_pair_distance(want.mean) > S.GROW_DISTINCT_PX
    st = _stream(7, S.GROW_GRID, W=S.GROW_W, H=S.GROW_H)
    _push_all(st, frames, 7)
    cells = st.finish()
    _assert_rows(cells, want, "first pass")
    _push_all(st, frames[100:120], 7)                   # the grown buffer serves the next clip from row 0
    again = st.finish()
    st.close()
    _assert_rows(again, _rows(want, 100, 119), "second pass")


# ---------------------------------------------------------------------------------------------------------------------
# F. one frame only, and none
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_stream_finish_after_one_frame_and_after_none(ref, B):
    st = _stream(B)
    assert st.finish().shape == (0, 12, 2)              # nothing pushed, nothing ever allocated
    assert st.push(ref.frames[0]) == 0
    assert st.finish().shape == (0, 12, 2)              # one frame: no pair, and the frame is not kept
    _push_all(st, ref.frames[4:8], B)
    cells = st.finish()
    assert st.push(ref.frames[2]) == 0
    assert st.finish().shape == (0, 12, 2)              # the same with results of an earlier clip still in the buffer
    st.close()
    _assert_rows(cells, _rows(ref.cells[S.GRID], 4, 7))


# ---------------------------------------------------------------------------------------------------------------------
# G. engine interleaving
# ---------------------------------------------------------------------------------------------------------------------
def test_engine_calc_and_refused_push_leave_the_kept_frame_alone(ref):
    from opticalflowclustering_amd.flow import FlowEngine
    L = _lib()
    g = ref.frames
    eng = FlowEngine(S.W, S.H)
    assert eng.push(g[0]) is None
    assert np.array_equal(eng.calc(g[15], g[16]), ref.table[15])            # unrelated frames through the shared staging
    assert np.array_equal(eng.push(g[1]), ref.table[0])                     # calc did not disturb the kept frame
    rc = L.load().ofc_flow_push_gray(eng._h, L.ptr(np.ascontiguousarray(g[9])), None)
    assert rc == L.OFC_EINVAL and L.load().ofc_last_error()
    assert np.array_equal(eng.push(g[2]), ref.table[1])                     # nor did the refused push replace it
    assert np.array_equal(eng.calc(g[7], g[8]), ref.table[7])
    assert np.array_equal(eng.push(g[3]), ref.table[2])
    eng.close()


def test_engine_grey_and_bgr_pushes_share_one_kept_frame(ref):
    from opticalflowclustering_amd import vis
    from opticalflowclustering_amd.flow import FlowEngine
    L = _lib()
    lib = L.load()
    g = ref.frames
    P = S.W * S.H
    f0, f2 = S.bgr_frame(0, g), S.gray_as_bgr(g[2])
    g0 = O.bgr2gray(f0)
    want01 = _pairwise(np.stack([g0, g[1]]))[0]
    want_vis, want_mag = vis.flow_to_bgr(ref.table[1])

    def last_vis(eng):
        p = C.c_void_p()
        rc = lib.ofc_flow_last_vis_dev(eng._h, C.byref(p))
        if rc != L.OFC_OK:
            return rc, None
        out = np.empty((S.H, S.W, 3), np.uint8)
        L.check(lib.ofc_memcpy_d2h(0, L.ptr(out), p, P * 3))
        return rc, out

    flows, mags = [], []
    for outputs in (False, True):
        eng = FlowEngine(S.W, S.H)
        assert last_vis(eng)[0] == L.OFC_EINVAL                             # before any BGR push
        assert lib.ofc_flow_push_bgr(eng._h, L.ptr(f0), None, None, None) == L.OFC_ENOTREADY
        assert last_vis(eng)[0] == L.OFC_EINVAL                             # a frame is kept, nothing is drawn yet
        assert np.array_equal(eng.push(g[1]), want01)                       # the grey push pairs with the kept BGR frame
        out_vis = np.zeros((S.H, S.W, 3), np.uint8)
        out_flow = np.zeros((S.H, S.W, 2), np.float32)
        mm = C.c_float(-1.0)
        if outputs:
            rc = lib.ofc_flow_push_bgr(eng._h, L.ptr(f2), L.ptr(out_vis), C.byref(mm), L.ptr(out_flow))
        else:
            rc = lib.ofc_flow_push_bgr(eng._h, L.ptr(f2), None, None, None)
        assert rc == L.OFC_OK
        rc, dev_vis = last_vis(eng)
        assert rc == L.OFC_OK and np.array_equal(dev_vis, want_vis)
        if outputs:
            assert np.array_equal(out_vis, want_vis) and np.array_equal(out_flow, ref.table[1])
            assert np.float32(mm.value).tobytes() == np.float32(want_mag).tobytes()
        assert np.array_equal(eng.push(g[3]), ref.table[2])                 # and the BGR push left its grey frame behind
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# H. batch sizes in sequence on one engine
# ---------------------------------------------------------------------------------------------------------------------
def _run_windows(engines, windows, frames, table, sync, running=False):
    """windows (first frame, pairs, _stats?) in order, call i on engines[i % len]; flows land at their pair index in one
    buffer (as ClipPipeline lays them out; synchronised calls only: the window is wiped before each call, so that a call
    which leaves a pair unwritten cannot hide behind an earlier call's identical values) or, running, one after the other
    (disjoint: what unsynchronised calls and two streams need).  The buffer, max_batch pairs of slack behind it included, is
    modelled on the host: a call writes its n pairs and nothing else."""
    assert sync or running
    L = _lib()
    Hh, Ww = frames.shape[1:]
    P = Ww * Hh
    n_out = (sum(n for _, n, _ in windows) if running else len(frames) - 1) + S.SEQ_MAX_BATCH
    fd = L.DeviceBuffer(frames.nbytes).upload(frames)
    out, sums = L.DeviceBuffer(n_out * P * 8), L.DeviceBuffer(len(windows) * 16)
    for b in (out, sums):
        L.check(L.load().ofc_memset(0, C.c_void_p(b.ptr), 0xFF, b.nbytes))
    model = np.full((n_out, Hh, Ww, 2), SENTINEL, np.uint32)
    want_sums, off = {}, 0

    def compare(where):
        got = out.download(model.shape, np.uint32)
        bad = sorted({int(i) for i in np.argwhere((got != model).reshape(n_out, -1).any(1))[:, 0]})
        assert not bad, (where, "pairs that differ from the model", bad)

    for i, (f0, n, stats) in enumerate(windows):
        o = off if running else f0
        if not running:
            L.check(L.load().ofc_memset(0, C.c_void_p(out.ptr + o * P * 8), 0xFF, n * P * 8))
            model[o:o + n] = SENTINEL
        engines[i % len(engines)].calc_frames_dev(fd.ptr + f0 * P, n + 1, out.ptr + o * P * 8, sync=sync,
                                                  uv_sum_ptr=sums.ptr + 16 * i if stats else None)
        model[o:o + n] = table[f0:f0 + n].view(np.uint32)
        if stats:
            want_sums[i] = table[f0:f0 + n].astype(np.float64).reshape(-1, 2).sum(0)
        if sync:
            compare(f"after call {i} {(f0, n, stats)}")
        off += n
    for e in engines:
        e.sync()
    compare("at the end")
    got = sums.download((len(windows), 2), np.float64)
    for i in range(len(windows)):
        if i in want_sums:
            w = want_sums[i]
            assert (np.abs(got[i] - w) <= S.SUM_BAR * np.maximum(1.0, np.abs(w))).all(), (i, got[i], w)
        else:
            assert (got[i].view(np.uint64) == 0xFFFFFFFFFFFFFFFF).all(), i
    for b in (fd, out, sums):
        b.free()


SEQ_VARIANTS = {"defaults": {}, "one_iteration": dict(iterations=1), "winsize9": dict(winsize=9), "winsize31": dict(winsize=31)}


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
@pytest.mark.parametrize("variant", list(SEQ_VARIANTS))
def test_engine_batch_sizes_in_sequence(ref, variant, sync):
    """5, 1, 3, 5, 2, 1 pairs on one max_batch = 5 engine.  defaults: the sums ride in the last iteration's epilogue and
    their scratch, sized by the 1-pair call, has to grow for the 5-pair one (the launch checks its grid against what the
    buffer holds and refuses otherwise); one_iteration / winsize9 / winsize31: the sweep form, whose scratch has one size"""
    from opticalflowclustering_amd.flow import FlowEngine
    frames = ref.frames[:S.SEQ_FRAMES]
    kw = SEQ_VARIANTS[variant]
    table = _table_for(ref, variant, frames, **kw) if kw else ref.table[:S.SEQ_FRAMES - 1]
    eng = FlowEngine(S.W, S.H, _lib().FbParams(**kw), max_batch=S.SEQ_MAX_BATCH)
    _run_windows([eng], S.SEQ_WINDOWS, frames, table, sync, running=not sync)
    eng.close()


@pytest.mark.parametrize("iterations", [2, 3])
def test_engine_batch_sizes_in_sequence_on_one_level(ref, iterations):
    """32 x 32: level 0 is the top of the pyramid, so the zero flow the first iteration starts from is filled by the call
    itself, with an even iteration count in the caller's buffer: n pairs of it, not max_batch"""
    from opticalflowclustering_amd.flow import FlowEngine
    frames = S.grow_clip()[:S.SEQ_FRAMES]
    table = _table_for(ref, f"grow-it{iterations}", frames, iterations=iterations)
    eng = FlowEngine(S.GROW_W, S.GROW_H, _lib().FbParams(iterations=iterations), max_batch=S.SEQ_MAX_BATCH)
    _run_windows([eng], S.SEQ_WINDOWS, frames, table, True)
    eng.close()


def test_two_engines_alternate_over_overlapping_windows(ref):
    """as ClipPipeline runs them: call i on engine i % 2, nothing synchronised until the end, the frame windows overlap,
    the outputs do not"""
    from opticalflowclustering_amd.flow import FlowEngine
    engines = [FlowEngine(S.W, S.H, max_batch=S.SEQ_MAX_BATCH) for _ in range(2)]
    _run_windows(engines, S.SEQ_WINDOWS, ref.frames[:S.SEQ_FRAMES], ref.table[:S.SEQ_FRAMES - 1], False, running=True)
    for e in engines:
        e.close()


@pytest.mark.parametrize("first,n_frames,batch,schedule", [(0, 8, 3, [1, 3, 3]), (3, 5, 2, [2, 2]), (6, 5, [1, 2, 1], [1, 2, 1])])
def test_clip_pipeline_schedules(ref, first, n_frames, batch, schedule):
    from opticalflowclustering_amd.pipeline import ClipPipeline
    pipe = ClipPipeline(S.W, S.H, n_frames, batch_pairs=batch)
    assert pipe.schedule == schedule and len(pipe.engines) == 2
    pipe.upload_frames(ref.frames[first:first + n_frames])
    want = ref.table[first:first + n_frames - 1]
    for stats in (True, False, True):
        pipe.run_flow(stats=stats)
        assert np.array_equal(pipe.flows_host(), want)
    sums = pipe.uv_sums.download((pipe.n_batches, 2), np.float64)
    starts = np.concatenate([[0], np.cumsum(schedule)])
    for b in range(pipe.n_batches):
        w = want[starts[b]:starts[b + 1]].astype(np.float64).reshape(-1, 2).sum(0)
        assert (np.abs(sums[b] - w) <= S.SUM_BAR * np.maximum(1.0, np.abs(w))).all(), (b, sums[b], w)
    pipe.close()


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
def test_engine_refuses_bad_frame_counts_and_stays_exact(ref, stats):
    """n_frames 1 and max_batch + 2: OFC_EINVAL, nothing written, and the next valid call is still exact"""
    from opticalflowclustering_amd.flow import FlowEngine
    L = _lib()
    frames = ref.frames[:S.SEQ_FRAMES]
    P = S.W * S.H
    eng = FlowEngine(S.W, S.H, max_batch=S.SEQ_MAX_BATCH)
    fd = L.DeviceBuffer(frames.nbytes).upload(frames)
    out, sums = L.DeviceBuffer((S.SEQ_MAX_BATCH + 2) * P * 8), L.DeviceBuffer(16)
    for b in (out, sums):
        L.check(L.load().ofc_memset(0, C.c_void_p(b.ptr), 0xFF, b.nbytes))
    eng.calc_frames_dev(fd.ptr, 4, out.ptr, uv_sum_ptr=sums.ptr if stats else None)          # sizes the scratch
    L.check(L.load().ofc_memset(0, C.c_void_p(out.ptr), 0xFF, out.nbytes))
    L.check(L.load().ofc_memset(0, C.c_void_p(sums.ptr), 0xFF, sums.nbytes))
    for n_frames in (1, S.SEQ_MAX_BATCH + 2, 0, -3):
        with pytest.raises(ValueError, match="max_batch"):
            eng.calc_frames_dev(fd.ptr, n_frames, out.ptr, uv_sum_ptr=sums.ptr if stats else None)
        eng.sync()
        assert (out.download(((S.SEQ_MAX_BATCH + 2) * P * 2,), np.uint32) == SENTINEL).all(), n_frames
        assert (sums.download((2,), np.uint64) == 0xFFFFFFFFFFFFFFFF).all(), n_frames
    eng.calc_frames_dev(fd.ptr + 2 * P, S.SEQ_MAX_BATCH + 1, out.ptr, uv_sum_ptr=sums.ptr if stats else None)
    got = out.download((S.SEQ_MAX_BATCH + 2, S.H, S.W, 2), np.float32)
    assert np.array_equal(got[:S.SEQ_MAX_BATCH], ref.table[2:2 + S.SEQ_MAX_BATCH])
    assert (got[S.SEQ_MAX_BATCH:].view(np.uint32) == SENTINEL).all()
    if stats:
        w = ref.table[2:2 + S.SEQ_MAX_BATCH].astype(np.float64).reshape(-1, 2).sum(0)
        assert (np.abs(sums.download((2,), np.float64) - w) <= S.SUM_BAR * np.maximum(1.0, np.abs(w))).all()
    eng.close()
    for b in (fd, out, sums):
        b.free()


# ---------------------------------------------------------------------------------------------------------------------
# I. two handles at once
# ---------------------------------------------------------------------------------------------------------------------
def test_stream_and_engine_side_by_side(ref):
    """a FlowStream and a FlowEngine of the same size, alternating: the handles share nothing"""
    from opticalflowclustering_amd.flow import FlowEngine
    B, T = 2, 10
    st, eng = _stream(B), FlowEngine(S.W, S.H)
    last = 0
    for t in range(T):
        done = st.push(ref.frames[t])
        assert 0 <= last <= done <= B * (t // B)
        last = done
        assert np.array_equal(eng.calc(ref.frames[20 - t], ref.frames[21 - t]), ref.table[20 - t]), t
        flow = eng.push(ref.frames[12 + t])
        assert flow is None if t == 0 else np.array_equal(flow, ref.table[11 + t]), t
    cells = st.finish()
    assert np.array_equal(eng.calc(ref.frames[0], ref.frames[1]), ref.table[0])
    st.close()
    eng.close()
    _assert_rows(cells, _rows(ref.cells[S.GRID], 0, T - 1))
