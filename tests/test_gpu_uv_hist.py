"""The (u,v) histogram on the device (uv_hist.hip: ofc_uv_hist_accum_dev, ofc_uv_hist, the streaming ingest's table) and the
fit on it (uvhist.UVHistogram.fit, ClipPipeline.uv_histogram, motionGrids --fit-stream).

The table is integers, so everything is compared with array_equal against the numpy model of tests/uv_hist_cases.py;
test_uv_hist_host.py proves the cases well-conditioned.  Sizes run either side of a wave, of a work-group's share and of a
whole grid's first round; patterns put one bin, two, 64 or a changing one into the kernel's waves."""
import ctypes as C

import numpy as np
import pytest

from tests import motion_grid_cases as MC
from tests import uv_hist_cases as UC

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def accum(flow, bins, rng, table=None, offset=0):
    """ofc_uv_hist_accum_dev on a fresh device copy of `flow`, placed `offset` vectors into its allocation; the table starts
    as `table` (zeros when None) -> the table after the call"""
    L = _L()
    f = np.ascontiguousarray(flow, np.float32).reshape(-1, 2)
    fd = L.DeviceBuffer(max((len(f) + offset) * 8, 8))
    td = L.DeviceBuffer(UC.table_len(bins) * 8)
    try:
        if len(f):
            fd.upload(f, offset * 8)
        td.upload(np.zeros(UC.table_len(bins), np.int64) if table is None else table)
        L.check(L.load().ofc_uv_hist_accum_dev(0, C.c_void_p(fd.ptr + offset * 8), len(f), bins, rng, C.c_void_p(td.ptr)))
        return td.download((UC.table_len(bins),), np.int64)
    finally:
        fd.free()
        td.free()


def host(flow, bins, rng):
    from opticalflowclustering_amd.uvhist import uv_histogram
    return uv_histogram(flow, bins, rng)


@pytest.mark.parametrize("n", UC.SMALL_SIZES + UC.SHARE_SIZES)
def test_sizes_around_a_wave_and_a_share(n):
    for bins, rng in ((256, 8.0), (16, 2.0 ** -4)):
        f = UC.mixed_field(n, bins, rng, seed=n)
        assert np.array_equal(accum(f, bins, rng), UC.model(f, bins, rng))
    f = UC.pattern("63-and-1", n, 256, 8.0)
    assert np.array_equal(accum(f, 256, 8.0), UC.model(f, 256, 8.0))


@pytest.mark.parametrize("n", UC.GRID_SIZES)
def test_sizes_around_a_whole_grid(n):
    """the last vector is the only one of its bin: lost or counted twice, it shows"""
    f = UC.mixed_field(n, 256, 8.0, seed=2)
    f[-1] = (-7.99, 7.99)
    want = UC.model(f, 256, 8.0)
    assert want[255 * 256] == 1
    assert np.array_equal(accum(f, 256, 8.0), want)


@pytest.mark.parametrize("n", (1, 65, 4099))
def test_a_field_one_vector_into_its_allocation(n):
    f = UC.mixed_field(n, 1024, 32.0, seed=9)
    assert np.array_equal(accum(f, 1024, 32.0, offset=1), UC.model(f, 1024, 32.0))


@pytest.mark.parametrize("bins,rng", UC.PARAMS)
def test_special_and_edge_values_in_u_only_and_in_v_only(bins, rng):
    vals = np.concatenate([UC.special_values(bins, rng), UC.edge_values(bins, rng)])
    for axis in (0, 1):
        for other in (0.25 * rng, -0.5 * rng):
            f = UC.in_one_axis(vals, axis, other)
            want = UC.model(f, bins, rng)
            assert want[-1] >= 9 and (want[bins * bins:-1] < 0).any()
            assert np.array_equal(accum(f, bins, rng), want)
    f = np.stack([vals, vals[::-1]], -1)                                         # both axes special at once
    assert np.array_equal(accum(f, bins, rng), UC.model(f, bins, rng))


@pytest.mark.parametrize("bins,rng", UC.PARAMS)
@pytest.mark.parametrize("name", UC.PATTERNS)
def test_patterns(name, bins, rng):
    n = 3 * UC.SHARE + 77                                                        # several work-groups, a ragged last share
    f = UC.pattern(name, n, bins, rng)
    assert np.array_equal(accum(f, bins, rng), UC.model(f, bins, rng))


def test_one_bin_over_many_shares_per_work_group():
    """the contention path at length: half the work-groups walk two shares, all of it in one bin"""
    n = 3 * UC.SHARE * UC.MAX_GRID // 2 + 5
    f = UC.pattern("one-bin", n, 1024, 32.0)
    got = accum(f, 1024, 32.0)
    assert np.array_equal(got, UC.model(f, 1024, 32.0)) and np.count_nonzero(got[:1024 * 1024]) == 1


def test_two_calls_add_up_and_two_runs_give_equal_bits():
    bins, rng = 1024, 32.0
    a, b = UC.mixed_field(5000, bins, rng, seed=3), UC.pattern("uniform", 4099, bins, rng, seed=4)
    both = UC.model(np.concatenate([a, b]), bins, rng)
    first = accum(a, bins, rng)
    assert np.array_equal(first, UC.model(a, bins, rng))
    assert np.array_equal(accum(b, bins, rng, table=first), both)
    assert np.array_equal(accum(np.concatenate([a, b]), bins, rng), both)
    assert np.array_equal(accum(np.concatenate([b, a]), bins, rng), both)       # nor does the order matter
    assert np.array_equal(accum(a, bins, rng), first)
    junk = np.full(UC.table_len(bins), -5, np.int64)                             # it adds to whatever is there
    assert np.array_equal(accum(a, bins, rng, table=junk), first - 5)
    assert np.array_equal(accum(a[:0], bins, rng, table=junk), junk)            # n = 0 is a no-op


def test_host_form_writes_the_table_and_takes_stacks():
    L = _L()
    f = UC.mixed_field(3 * 20 * 30, 256, 8.0, seed=5).reshape(3, 20, 30, 2)
    want = UC.model(f, 256, 8.0)
    h = host(f, 256, 8.0)
    assert np.array_equal(h.table, want) and h.outside == want[-1] > 0 and h.n == 1800 - want[-1]
    assert np.array_equal(host(f[0], 256, 8.0).table, UC.model(f[0], 256, 8.0))
    assert np.array_equal((host(f[0], 256, 8.0) + host(f[1:], 256, 8.0)).table, want)
    table = np.full(UC.table_len(16), 77, np.int64)                              # written, not added to
    assert L.load().ofc_uv_hist(0, None, 0, 16, 2.0, L.ptr(table)) == L.OFC_OK and not table.any()
    d = host(f, 1024, 32.0)                                                      # the defaults
    from opticalflowclustering_amd.uvhist import uv_histogram
    assert np.array_equal(uv_histogram(f).table, d.table) and (d.bins, d.range) == (1024, 32.0)


def test_refusals_launch_nothing():
    L = _L()
    lib = L.load()
    f = UC.mixed_field(100, 16, 2.0)
    fd, td = L.DeviceBuffer(800).upload(f), L.DeviceBuffer(UC.table_len(16) * 8)
    td.zero()
    host_table = np.full(UC.table_len(16), 9, np.int64)
    ms = C.c_float(-1.0)
    fp, tp = C.c_void_p(fd.ptr), C.c_void_p(td.ptr)
    bad = [(8, 2.0), (4096, 2.0), (24, 2.0), (0, 2.0), (-16, 2.0), (16, 3.0), (16, 0.03125), (16, 2048.0), (16, 0.0), (16, -2.0),
           (16, float("nan")), (16, float("inf"))]
    for bins, rng in bad:
        assert lib.ofc_uv_hist_accum_dev(0, fp, 100, bins, rng, tp) == L.OFC_EINVAL, (bins, rng)
        assert lib.ofc_uv_hist(0, L.ptr(f), 100, bins, rng, L.ptr(host_table)) == L.OFC_EINVAL
        assert lib.ofc_bench_uv_hist(0, fp, 100, bins, rng, 1, C.byref(ms)) == L.OFC_EINVAL
    assert "range" in lib.ofc_last_error().decode()
    assert lib.ofc_uv_hist_accum_dev(0, fp, -1, 16, 2.0, tp) == L.OFC_EINVAL
    assert lib.ofc_uv_hist_accum_dev(0, None, 100, 16, 2.0, tp) == L.OFC_EINVAL
    assert lib.ofc_uv_hist_accum_dev(0, fp, 100, 16, 2.0, None) == L.OFC_EINVAL
    assert lib.ofc_uv_hist_accum_dev(0, None, 0, 16, 2.0, None) == L.OFC_EINVAL
    assert lib.ofc_uv_hist_accum_dev(0, C.c_void_p(fd.ptr + 4), 99, 16, 2.0, tp) == L.OFC_EINVAL
    assert lib.ofc_uv_hist(0, None, 100, 16, 2.0, L.ptr(host_table)) == L.OFC_EINVAL
    assert lib.ofc_uv_hist(0, L.ptr(f), -1, 16, 2.0, L.ptr(host_table)) == L.OFC_EINVAL
    assert lib.ofc_uv_hist(0, L.ptr(f), 100, 16, 2.0, None) == L.OFC_EINVAL
    assert lib.ofc_bench_uv_hist(0, fp, 0, 16, 2.0, 1, C.byref(ms)) == L.OFC_EINVAL
    assert lib.ofc_bench_uv_hist(0, fp, 100, 16, 2.0, 0, C.byref(ms)) == L.OFC_EINVAL
    assert lib.ofc_bench_uv_hist(0, None, 100, 16, 2.0, 1, C.byref(ms)) == L.OFC_EINVAL
    assert lib.ofc_bench_uv_hist(0, fp, 100, 16, 2.0, 1, None) == L.OFC_EINVAL
    assert lib.ofc_uv_hist_accum_dev(99, fp, 100, 16, 2.0, tp) == L.OFC_ENODEV
    assert not td.download((UC.table_len(16),), np.int64).any() and (host_table == 9).all() and ms.value == -1.0
    assert lib.ofc_uv_hist_accum_dev(0, None, 0, 16, 2.0, tp) == L.OFC_OK        # n = 0 needs no field
    assert lib.ofc_bench_uv_hist(0, fp, 100, 16, 2.0, 2, C.byref(ms)) == L.OFC_OK and ms.value > 0
    assert not td.download((UC.table_len(16),), np.int64).any()                  # the hook's table is its own
    fd.free()
    td.free()


# ---- the stream ----
def _pairwise(frames):
    from opticalflowclustering_amd.flow import FlowEngine
    eng = FlowEngine(UC.STREAM_W, UC.STREAM_H, max_batch=1)
    out = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    eng.close()
    return out


def _stream(**kw):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(UC.STREAM_W, UC.STREAM_H, batch_pairs=UC.STREAM_BATCH, rows=UC.STREAM_GRID[0], cols=UC.STREAM_GRID[1], **kw)


@pytest.fixture(scope="module")
def clip():
    """six frames, their five pairwise fields (the engine's, one pair at a time) and what a plain stream delivers: read-only"""
    from types import SimpleNamespace
    from opticalflowclustering_amd.vis import grid_assign_counts
    frames = UC.stream_clip(6)
    table = _pairwise(frames)
    st = _stream()
    for f in frames:
        st.push(f)
    cells = st.finish()
    st.close()
    counts = grid_assign_counts(table, UC.STREAM_CENTRES, *UC.STREAM_GRID)
    bins, rng = UC.STREAM_PARAMS
    assert len(np.unique(UC.bin_of(table, bins, rng))) > 20                      # the fields spread over many bins
    for a in (frames, table, cells, counts):
        a.setflags(write=False)
    return SimpleNamespace(frames=frames, table=table, cells=cells, counts=counts)


@pytest.mark.parametrize("n_frames", (5, 6), ids=["full-batches", "partial-batch"])
@pytest.mark.parametrize("model", (False, True), ids=["plain", "model"])
def test_stream_table_equals_the_histogram_of_the_pairwise_fields(clip, n_frames, model):
    bins, rng = UC.STREAM_PARAMS
    st = _stream(histogram=(bins, rng), centers=UC.STREAM_CENTRES if model else None)
    assert st.hist == (bins, rng)
    for f in clip.frames[:n_frames]:
        st.push(f)
    if model:
        cells, counts = st.finish_clusters()
        assert np.array_equal(counts, clip.counts[:n_frames - 1])
    else:
        cells = st.finish()
    assert np.array_equal(cells.view(np.uint32), clip.cells[:n_frames - 1].view(np.uint32))
    want = host(clip.table[:n_frames - 1], bins, rng)
    assert np.array_equal(want.table, UC.model(clip.table[:n_frames - 1], bins, rng))
    keep = st.histogram(reset=False)
    assert np.array_equal(keep.table, want.table) and (keep.bins, keep.range) == (bins, rng)
    assert np.array_equal(st.histogram(reset=False).table, want.table)          # reading leaves it
    assert np.array_equal(st.histogram().table, want.table)                      # reset=True is the default ...
    assert not st.histogram(reset=False).table.any()                             # ... and zeroes it
    st.close()


def test_stream_table_spans_clips_until_reset_and_follows_set_histogram(clip):
    bins, rng = UC.STREAM_PARAMS
    st = _stream(histogram=(bins, rng))
    for f in clip.frames:
        st.push(f)
    st.finish()
    for f in clip.frames[1:5]:                                                   # a second clip: pairs 1 .. 3, no frame carried over
        st.push(f)
    st.finish()
    two = host(clip.table, bins, rng) + host(clip.table[1:4], bins, rng)
    assert np.array_equal(st.histogram(reset=False).table, two.table)
    st.set_histogram(bins, rng)                                                  # the same parameters keep the table
    assert np.array_equal(st.histogram(reset=False).table, two.table)
    st.set_model(UC.STREAM_CENTRES)                                              # a model arrives: the table goes on
    for f in clip.frames[:3]:
        st.push(f)
    cells, counts = st.finish_clusters()
    assert np.array_equal(counts, clip.counts[:2])
    assert np.array_equal(st.histogram().table, (two + host(clip.table[:2], bins, rng)).table)
    st.set_histogram(1024, 32.0)                                                 # other parameters: a new, empty table
    assert st.histogram(reset=False).table.shape == (UC.table_len(1024),) and not st.histogram(reset=False).table.any()
    for f in clip.frames[:4]:
        st.push(f)
    st.finish_clusters()
    assert np.array_equal(st.histogram().table, host(clip.table[:3], 1024, 32.0).table)
    st.set_histogram(None)                                                       # removed: what the stream delivers is unchanged
    assert st.hist is None
    for f in clip.frames:
        st.push(f)
    cells, counts = st.finish_clusters()
    assert np.array_equal(cells.view(np.uint32), clip.cells.view(np.uint32)) and np.array_equal(counts, clip.counts)
    with pytest.raises(ValueError, match="no histogram"):
        st.histogram()
    st.close()


@pytest.mark.parametrize("pushed", [1, 2, 3, 4])
def test_stream_histogram_preconditions(clip, pushed):
    L = _L()
    bins, rng = UC.STREAM_PARAMS
    st = _stream(histogram=(bins, rng))
    assert not st.histogram(reset=False).table.any()                             # a fresh stream: an empty table
    for f in clip.frames[:pushed]:
        st.push(f)
    with pytest.raises(ValueError, match="holds frames"):
        st.set_histogram(16, 2.0)
    with pytest.raises(ValueError, match="holds frames"):
        st.set_histogram(None)
    with pytest.raises(ValueError, match="holds frames"):
        st.histogram()
    assert L.load().ofc_stream_read_histogram(st._h, None, 1) == L.OFC_EINVAL
    assert st.hist == (bins, rng)
    for f in clip.frames[pushed:]:
        st.push(f)
    st.finish()
    for b, r in ((8, 2.0), (16, 3.0), (4096, 1.0), (-1, 2.0)):                   # refused after a finish too, nothing changes
        assert L.load().ofc_stream_set_histogram(st._h, b, r) == L.OFC_EINVAL
    assert L.load().ofc_stream_set_histogram(None, 16, 2.0) == L.OFC_EINVAL
    assert L.load().ofc_stream_read_histogram(None, None, 0) == L.OFC_EINVAL
    assert L.load().ofc_stream_read_histogram(st._h, None, 0) == L.OFC_OK        # NULL: nothing copied, nothing lost
    assert np.array_equal(st.histogram().table, host(clip.table, bins, rng).table)
    st.close()
    plain = _stream()
    with pytest.raises(ValueError, match="no histogram"):
        plain.histogram()
    plain.close()


# ---- the fit ----
@pytest.fixture(scope="module")
def lattice():
    X = UC.lattice_field()
    X.setflags(write=False)
    return X, host(X, UC.FIT_BINS, UC.FIT_RANGE)


def test_fit_on_the_lattice_equals_the_full_fit(lattice):
    from opticalflowclustering_amd.cluster import KMeans
    X, h = lattice
    assert np.array_equal(h.table, UC.model(X, UC.FIT_BINS, UC.FIT_RANGE))
    full = KMeans(UC.FIT_K, init=UC.FIT_INIT, tol=0).fit(X)
    cen, inertia, n_iter = h.fit(UC.FIT_K, init=UC.FIT_INIT, tol=0)
    err = np.abs(cen - full.cluster_centers_).max()
    print("lattice: |histogram fit - full fit| = %.3e px, n_iter %d / %d" % (err, n_iter, full.n_iter_))
    assert err <= 1e-9 and n_iter == full.n_iter_
    P, _ = h.points()
    bin_labels = KMeans(UC.FIT_K, init=cen).fit(P, sample_weight=h.points()[1]).labels_
    order = np.flatnonzero(h.counts.ravel())
    assert np.array_equal(bin_labels[np.searchsorted(order, UC.bin_of(X, UC.FIT_BINS, UC.FIT_RANGE))], full.labels_)
    assert abs(inertia - full.inertia_) <= 1e-9 * full.inertia_                  # one value per bin: no scatter is left out


def test_fit_off_the_lattice_stays_within_the_fixed_point_step():
    """a centre is the mean of its members, each member is off by at most 2^-17 px (half the fixed-point step), and the
    partitions agree (test_uv_hist_host.py): so is the centre.  The bound is derived, not measured"""
    from opticalflowclustering_amd.cluster import KMeans
    X = UC.off_lattice_field()
    full = KMeans(UC.FIT_K, init=UC.FIT_INIT, tol=0).fit(X)
    cen, _, n_iter = host(X, UC.FIT_BINS, UC.FIT_RANGE).fit(UC.FIT_K, init=UC.FIT_INIT, tol=0)
    err = np.abs(cen - full.cluster_centers_).max()
    print("off the lattice: |histogram fit - full fit| = %.3e px (bound %.3e)" % (err, 2.0 ** -17))
    assert err <= 2.0 ** -17 and n_iter == full.n_iter_


def test_n_init_is_the_best_of_the_single_fits_with_the_derived_seeds(lattice):
    from opticalflowclustering_amd.uvhist import restart_seeds
    _, h = lattice
    singles = [h.fit(UC.FIT_K, random_state=int(s)) for s in restart_seeds(11, 3)]
    inertias = [s[1] for s in singles]
    best = singles[int(np.argmin(inertias))]                                     # argmin: the first smallest
    got = h.fit(UC.FIT_K, random_state=11, n_init=3)
    assert np.array_equal(got[0], best[0]) and got[1] == best[1] and got[2] == best[2]
    again = h.fit(UC.FIT_K, init=UC.FIT_INIT, n_init=3)                          # an explicit init runs once
    once = h.fit(UC.FIT_K, init=UC.FIT_INIT)
    assert np.array_equal(again[0], once[0]) and again[1:] == once[1:]
    with pytest.raises(ValueError, match="n_init"):
        h.fit(UC.FIT_K, n_init=0)
    with pytest.raises(ValueError, match="init should be"):
        h.fit(UC.FIT_K, init="random")


def test_clip_pipeline_histogram_equals_the_host_form():
    from opticalflowclustering_amd.pipeline import ClipPipeline
    pipe = ClipPipeline(MC.ASSIGN_W, MC.ASSIGN_H, MC.ASSIGN_FRAMES, batch_pairs=2)
    try:
        pipe.synth()
        pipe.run_flow()
        flows = pipe.flows_host()
        for bins, rng in ((1024, 32.0), (256, 8.0)):
            h = pipe.uv_histogram(bins, rng)
            assert np.array_equal(h.table, host(flows, bins, rng).table) and h.n + h.outside == flows.size // 2
        assert np.array_equal(pipe.uv_histogram().table, host(flows, 1024, 32.0).table)
        with pytest.raises(ValueError, match="power of two"):
            pipe.uv_histogram(100, 32.0)
    finally:
        pipe.close()


def test_motion_grids_fit_stream_cli(tmp_path, capsys):
    """two passes over a clip that is never resident: the centres are the fit on the histogram of the pairwise fields, the
    CSV is the --stream route's with those centres"""
    from opticalflowclustering_amd import motionGrids as G
    from opticalflowclustering_amd.flow import FlowEngine
    from opticalflowclustering_amd.vis import bgr2gray, grid_assign_counts
    clip_path, csv, saved, init = (str(tmp_path / n) for n in ("clip.npy", "out.csv", "saved.npy", "init.npy"))
    frames = MC.moving_blobs_clip()
    np.save(clip_path, frames)
    gray = np.stack([bgr2gray(f) for f in frames])
    eng = FlowEngine(gray.shape[2], gray.shape[1], max_batch=1)
    table = np.stack([eng.calc(gray[t], gray[t + 1]) for t in range(len(gray) - 1)])
    eng.close()
    h = host(table, 256, 8.0)
    base = ["--path", clip_path, "-c", "3", "--rows", "3", "--cols", "4", "-f", csv, "--fit-stream", "--hist-bins", "256",
            "--hist-range", "8", "--batch-pairs", "3"]
    counts, centres = G.main(base + ["--seed", "5", "--n-init", "2", "--save-model", saved])
    want_c, _, _ = h.fit(3, random_state=5, n_init=2)
    assert np.array_equal(centres, want_c) and np.array_equal(np.load(saved), want_c)
    assert np.array_equal(counts, grid_assign_counts(table, want_c, 3, 4))
    out = capsys.readouterr().out
    assert "outside" in out and f"{h.n} vectors" in out and f"{h.outside} outside" in out
    lines = open(csv).read().splitlines()
    assert len(lines) == 1 + 4 and lines[0] == ",".join(f"cell_{i}" for i in range(12))
    rows = np.array([[int(v) for v in ln.split(",")] for ln in lines[1:]])
    assert np.array_equal(rows, G.hue_rows(counts, want_c))
    c0 = np.array([[0.0112, -0.0071], [2.9, 0.05], [-0.04, -1.93]])              # an --init file runs once from it
    np.save(init, c0)
    _, centres = G.main(base + ["--init", init])
    assert np.array_equal(centres, h.fit(3, init=c0)[0])
    assert len(np.unique(np.argmax(counts, -1))) >= 2                            # the fit tells the cells apart
