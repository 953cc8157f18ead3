"""The streaming ingest with a model (ofc_stream_set_model / ofc_stream_finish_clusters, FlowStream, motionGrids --stream):
every pair's field is labelled and counted per cell on the device, batch by batch, behind the cell means.

The reference is the hook ofc_grid_assign_counts_dev (held to the numpy model by test_gpu_grid_assign.py) on the pairwise
table: every consecutive pair computed on its own by FlowEngine.calc.  A pair's flow does not depend on the batch it is
computed in (test_gpu_flow_sequences.py pins that), and a frame's counts depend on that frame alone, so the stream's
counts are equal and its sums bit-equal, whatever the batches were.  The clip is flow_sequence_cases' 160 x 96 one: 8 frames
at batch_pairs = 3 run as batches of 3, 3 and 1 pairs over both slots."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import flow_sequence_cases as S
from tests import motion_grid_cases as MC

pytestmark = pytest.mark.gpu

T, B = 8, 3
# around the clip's steps (u 0.45 .. 1.2, v -0.4 .. -0.8 px) and the still background; not dyadic
CENTRES = np.array([[0.0213, -0.0131], [0.5127, -0.4471], [0.8391, -0.7113], [1.1873, -0.5209], [0.7031, 0.1907]])
OTHER = CENTRES[:3] + 0.05
GRIDS = (S.GRID, S.FINE_GRID)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _lib():
    from opticalflowclustering_amd import _lib
    return _lib


def _pairwise(frames):
    from opticalflowclustering_amd.flow import FlowEngine
    Hh, Ww = frames.shape[1:]
    eng = FlowEngine(Ww, Hh, max_batch=1)
    out = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    eng.close()
    return out


def _stream(grid, centers=None, sums=False, batch=B, W=S.W, H=S.H):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(W, H, batch_pairs=batch, rows=grid[0], cols=grid[1], centers=centers, sums=sums)


def _hook(table, grid, centers=CENTRES):
    from opticalflowclustering_amd.vis import grid_assign_counts
    return grid_assign_counts(table, centers, grid[0], grid[1], sums=True)


@pytest.fixture(scope="module")
def ref():
    """the clip, its pairwise table, the hook's counts and sums per grid and a model-less stream's cell means: once, read-only"""
    frames = S.clip()[:T]
    table = _pairwise(frames)
    r = SimpleNamespace(frames=frames, table=table, counts={}, sums={}, cells={})
    for g in GRIDS:
        r.counts[g], r.sums[g] = _hook(table, g)
        assert len(np.unique(np.argmax(r.counts[g], -1))) >= 2          # the model tells the cells apart
        st = _stream(g)
        for f in frames:
            st.push(f)
        r.cells[g] = st.finish()
        st.close()
        for a in (r.counts[g], r.sums[g], r.cells[g]):
            a.setflags(write=False)
    frames.setflags(write=False)
    table.setflags(write=False)
    return r


def _assert_pairs(got, ref, grid, lo=0, hi=T - 1):
    cells, counts, sums = got
    assert counts.dtype == np.int32 and sums.dtype == np.float64 and cells.dtype == np.float32
    assert np.array_equal(counts, ref.counts[grid][lo:hi])
    assert np.array_equal(bits(sums), bits(ref.sums[grid][lo:hi]))
    assert np.array_equal(cells.view(np.uint32), ref.cells[grid][lo:hi].view(np.uint32))


def _raw_finish_clusters(st, cells, counts, sums, max_pairs):
    L = _lib()
    n = C.c_int(-7)
    rc = L.load().ofc_stream_finish_clusters(st._h, L.ptr(cells), L.ptr(counts), L.ptr(sums), max_pairs, C.byref(n))
    return rc, n.value, L.load().ofc_last_error().decode()


@pytest.mark.parametrize("grid", GRIDS, ids=["3x4", "14x25"])
def test_every_pair_equals_the_hook_on_the_pairwise_table(ref, grid):
    st = _stream(grid, CENTRES, sums=True)
    for f in ref.frames:
        st.push(f)
    got = st.finish_clusters()
    st.close()
    assert len(got) == 3 and len(got[0]) == T - 1
    _assert_pairs(got, ref, grid)


def test_a_model_without_sums_counts_the_same_and_refuses_a_sums_buffer(ref):
    L, g = _lib(), S.GRID
    cells_n = g[0] * g[1]
    st = _stream(g, CENTRES)                                                 # sums=False
    for f in ref.frames:
        st.push(f)
    sums = np.full((T - 1, cells_n, 5, 2), -7.25)
    counts = np.full((T - 1, cells_n, 5), 0x5A5A5A5A, np.int32)
    cells = np.full((T - 1, cells_n, 2), np.nan, np.float32)
    rc, n, msg = _raw_finish_clusters(st, cells, counts, sums, T - 1)
    assert rc == L.OFC_EINVAL and "sums" in msg
    assert (sums == -7.25).all() and (counts == 0x5A5A5A5A).all() and np.isnan(cells).all()
    got = st.finish_clusters()                                               # nothing was lost
    st.close()
    assert len(got) == 2
    assert np.array_equal(got[1], ref.counts[g]) and np.array_equal(got[0].view(np.uint32), ref.cells[g].view(np.uint32))


def test_finish_on_a_model_stream_returns_the_means_and_drops_the_counts(ref):
    g = S.GRID
    st = _stream(g, CENTRES, sums=True)
    for f in ref.frames:
        st.push(f)
    cells = st.finish()
    assert np.array_equal(cells.view(np.uint32), ref.cells[g].view(np.uint32))
    cells, counts, sums = st.finish_clusters()                               # the counts went with the means
    assert len(cells) == 0 and len(counts) == 0 and len(sums) == 0
    for f in ref.frames[2:7]:                                                # and the stream takes another clip
        st.push(f)
    _assert_pairs(st.finish_clusters(), ref, g, 2, 6)
    st.close()


def test_the_stream_is_reused_after_finish_clusters_and_takes_another_model(ref):
    from opticalflowclustering_amd.vis import grid_assign_counts
    g = S.GRID
    st = _stream(g, CENTRES, sums=True)
    for f in ref.frames:
        st.push(f)
    _assert_pairs(st.finish_clusters(), ref, g)
    for f in ref.frames[1:6]:                                                # pairs 1 .. 4: no frame is carried over
        st.push(f)
    _assert_pairs(st.finish_clusters(), ref, g, 1, 5)
    st.set_model(OTHER, sums=False)                                          # straight after a finish: another k, no sums
    for f in ref.frames[:5]:
        st.push(f)
    cells, counts = st.finish_clusters()
    assert counts.shape == (4, g[0] * g[1], 3)
    assert np.array_equal(counts, grid_assign_counts(ref.table[:4], OTHER, *g))
    assert np.array_equal(cells.view(np.uint32), ref.cells[g][:4].view(np.uint32))
    st.set_model(None)                                                       # k = 0 removes it
    for f in ref.frames[:3]:
        st.push(f)
    with pytest.raises(ValueError, match="no model"):
        st.finish_clusters()
    assert np.array_equal(st.finish().view(np.uint32), ref.cells[g][:2].view(np.uint32))
    st.close()


@pytest.mark.parametrize("pushed", [1, 2, 4, 7])
def test_set_model_in_mid_clip_is_refused_and_the_run_continues_unharmed(ref, pushed):
    L, g = _lib(), S.GRID
    st = _stream(g, CENTRES, sums=True)
    for f in ref.frames[:pushed]:
        st.push(f)
    with pytest.raises(ValueError, match="holds frames"):
        st.set_model(OTHER)
    with pytest.raises(ValueError, match="holds frames"):
        st.set_model(None)
    assert (st.k, st.sums) == (5, True)
    for f in ref.frames[pushed:]:
        st.push(f)
    _assert_pairs(st.finish_clusters(), ref, g)                              # the model stayed as it was
    bad = CENTRES.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        st.set_model(bad)
    z = np.zeros((17, 2))
    assert L.load().ofc_stream_set_model(st._h, 17, None, L.ptr(z), 0) == L.OFC_EUNSUPPORTED
    assert L.load().ofc_stream_set_model(st._h, -1, None, L.ptr(z), 0) == L.OFC_EUNSUPPORTED
    assert L.load().ofc_stream_set_model(st._h, 3, None, None, 0) == L.OFC_EINVAL
    for f in ref.frames[:4]:
        st.push(f)
    _assert_pairs(st.finish_clusters(), ref, g, 0, 3)                        # ... through every refusal
    st.close()


def test_finish_clusters_into_short_buffers_can_be_retried(ref):
    L, g = _lib(), S.GRID
    cells_n = g[0] * g[1]
    st = _stream(g, CENTRES, sums=True)
    for f in ref.frames:
        st.push(f)
    sums = np.full((T - 1, cells_n, 5, 2), -7.25)
    counts = np.full((T - 1, cells_n, 5), 0x5A5A5A5A, np.int32)
    cells = np.full((T - 1, cells_n, 2), np.nan, np.float32)
    for outs in ((cells, counts, sums), (None, counts, None), (None, None, sums)):
        rc, n, msg = _raw_finish_clusters(st, *outs, T - 2)
        assert rc == L.OFC_EINVAL and n == T - 1 and str(T - 1) in msg
        assert (sums == -7.25).all() and (counts == 0x5A5A5A5A).all() and np.isnan(cells).all()
    rc, n, _ = _raw_finish_clusters(st, cells, counts, sums, T - 1)
    assert rc == L.OFC_OK and n == T - 1
    _assert_pairs((cells, counts, sums), ref, g)
    rc, n, _ = _raw_finish_clusters(st, cells, counts, sums, T - 1)          # delivered: the stream is empty
    assert rc == L.OFC_OK and n == 0
    for f in ref.frames[:4]:                                                 # all NULL: count and drop
        st.push(f)
    rc, n, _ = _raw_finish_clusters(st, None, None, None, 0)
    assert rc == L.OFC_OK and n == 3
    rc, n, _ = _raw_finish_clusters(st, cells, counts, sums, T - 1)
    assert rc == L.OFC_OK and n == 0
    st.pushed = 0
    st.close()


def test_finish_clusters_without_a_model_is_refused(ref):
    L, g = _lib(), S.GRID
    st = _stream(g)
    for f in ref.frames[:5]:
        st.push(f)
    with pytest.raises(ValueError, match="no model"):
        st.finish_clusters()
    n = C.c_int(-7)
    assert L.load().ofc_stream_finish_clusters(st._h, None, None, None, 0, C.byref(n)) == L.OFC_EINVAL and n.value == -7
    assert np.array_equal(st.finish().view(np.uint32), ref.cells[g][:4].view(np.uint32))      # the run is unharmed
    st.close()


def test_result_buffers_grow_past_their_first_allocation():
    """64 x 48 frames cycling through 4 distinct images, 261 pushes at batch_pairs = 8: the 33rd batch takes the buffers
    past their 256 pairs.  Pair t is (image t % 4, image (t + 1) % 4), so its row equals the hook's on pair t % 4"""
    from opticalflowclustering_amd import synth
    Wg, Hg, n_push, grid = 64, 48, 261, (2, 3)
    p = synth.texture_params(S.GROW_SEED)
    xs, ys = (0.0, 0.5, 1.3, 2.4), (0.0, -0.3, -0.9, -1.3)                   # four different steps, the last one back to the start
    images = np.stack([synth.frame(Wg, Hg, xs[t], ys[t], p) for t in range(4)]).astype(np.uint8)
    table = _pairwise(np.concatenate([images, images[:1]]))
    cen = np.array([[0.0137, 0.0211], [0.5113, -0.2891], [0.7871, -0.6109], [1.0931, -0.4117], [-2.3871, 1.3309]])
    want_c, want_s = _hook(table, grid, cen)
    assert len(np.unique(want_c, axis=0)) == 4                               # the four pairs differ: a misplaced row shows
    st = _stream(grid, cen, sums=True, batch=8, W=Wg, H=Hg)
    for t in range(n_push):
        st.push(images[t % 4])
    cells, counts, sums = st.finish_clusters()
    st.close()
    idx = np.arange(n_push - 1) % 4
    assert counts.shape == (260, 6, 5) and np.array_equal(counts, want_c[idx])
    assert np.array_equal(bits(sums), bits(want_s[idx]))
    assert np.array_equal(cells.view(np.uint32), cells[:4][idx].view(np.uint32))


def test_motion_grids_stream_cli(tmp_path):
    from opticalflowclustering_amd import motionGrids as G
    from opticalflowclustering_amd.vis import bgr2gray, grid_assign_counts
    clip, csv, model, saved, cnt = (str(tmp_path / n) for n in ("clip.npy", "out.csv", "model.npy", "saved.npy", "counts.npy"))
    frames = MC.moving_blobs_clip()
    np.save(clip, frames)
    centres = np.array([[0.0112, -0.0071], [2.9, 0.05], [-0.04, -1.93]])       # still, the blob moving right, the one moving up
    np.save(model, centres)
    got_c, got_cen = G.main(["--path", clip, "-c", "3", "--rows", "3", "--cols", "4", "-f", csv, "--model", model, "--stream",
                             "--batch-pairs", "3", "--counts", cnt, "--save-model", saved])
    table = _pairwise(np.stack([bgr2gray(f) for f in frames]))
    want = grid_assign_counts(table, centres, 3, 4)
    counts = np.load(cnt)
    assert counts.dtype == np.int32 and counts.shape == (4, 12, 3) and np.array_equal(counts, want)
    assert np.array_equal(got_c, want) and np.array_equal(np.load(saved), centres) and np.array_equal(got_cen, centres)
    assert len(np.unique(np.argmax(counts, -1))) >= 2
    lines = open(csv).read().splitlines()
    assert len(lines) == 1 + 4 and lines[0] == ",".join(f"cell_{i}" for i in range(12))
    rows = np.array([[int(v) for v in ln.split(",")] for ln in lines[1:]])
    assert np.array_equal(rows, G.hue_rows(want, centres))

    np.save(clip, frames[:1])                                                # one frame: the resident route's error
    with pytest.raises(RuntimeError, match="a flow field needs two"):
        G.main(["--path", clip, "-c", "3", "-f", csv, "--model", model, "--stream"])
