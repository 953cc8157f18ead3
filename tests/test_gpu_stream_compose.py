"""The frame stream with every stage on (csrc/stream_api.cpp; FlowStream) against the staged routes.

Each stage has a test file of its own that holds it to a model; this one holds the chain to its documented order.  One clip
of nine pairs goes through a stream with the photometric check, the repair, the link moves, the camera, the cell means, the
model, the histogram, the blobs and their links all on, and every output is compared bit for bit with
stream_compose_cases.compose, which applies the same stages one at a time on host arrays.  A pair's field does not depend on
its batch (test_gpu_flow_sequences.py), and every stage behind the flow is integer or fixed-order arithmetic per pair, so
equality is the bar.  test_stream_compose_host.py proves compose itself on the CPU."""
import types

import numpy as np
import pytest

from tests import stream_compose_cases as SC

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def make_stream(batch_pairs, spec):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(SC.W, SC.H, batch_pairs=batch_pairs, rows=SC.ROWS, cols=SC.COLS, **spec)


def configure(st, spec):
    """an existing, idle stream to another spec, stage by stage, through FlowStream's setters"""
    st.set_model(spec["centers"], None, spec["sums"])
    st.set_histogram(*(spec["histogram"] or (None,)))
    st.set_camera(spec["camera"])
    st.set_blobs(**(spec["blobs"] or dict(connectivity=None)))
    st.set_photometric(**(spec["photometric"] or dict(on=False)))
    st.set_repair(**(spec["repair"] or dict(on=False)))


def read(st, cells_and_counts, reset=True):
    """everything a finished stream delivers -> a record with SC.OUTPUTS, None where the stage is off"""
    r = types.SimpleNamespace(**{k: None for k in SC.OUTPUTS})
    r.cells = cells_and_counts[0]
    if st.k:
        r.counts = cells_and_counts[1]
        r.sums = cells_and_counts[2] if st.sums else None
    if st.hist:
        r.hist = st.histogram(reset=reset).table
    if st.camera:
        cm = st.camera_motion()
        r.cam_params, r.cam_status = cm.params, cm.status
    if st.photo_args:
        r.photo_stats = st.photometric_stats()
    if st.repair_args:
        r.repair_counts = st.repair_stats()
    if st.blob_args:
        b = st.blobs()
        assert b.labels is None
        r.records, r.found, r.links, r.nlinks = b.records, b.found, b.links, b.nlinks
    return r


def run(st, frames, reset=True):
    """push, finish, read -> (record, what every push returned)"""
    done = [st.push(f) for f in frames]
    out = st.finish_clusters() if st.k else (st.finish(),)
    return read(st, out, reset), done


def fresh(batch_pairs, spec, frames):
    st = make_stream(batch_pairs, spec)
    try:
        return run(st, frames)[0]
    finally:
        st.close()


@pytest.fixture(scope="module")
def clip():
    """the clip, its nine pairwise fields (the engine's, one pair at a time, as the other stream tests obtain them), the
    composed reference with every stage on and the one without the repair; the preconditions of the clip.  Read-only."""
    from opticalflowclustering_amd.flow import FlowEngine
    frames = SC.clip()
    eng = FlowEngine(SC.W, SC.H, max_batch=1)
    try:
        fields = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    finally:
        eng.close()
    fields.setflags(write=False)
    c = types.SimpleNamespace(frames=frames, fields=fields, n=len(fields), refs={})

    def reference(name, spec, a=0, b=len(fields), order=SC.DOCUMENTED):
        """compose of pairs a .. b-1 under a spec, computed once per name"""
        key = (name, a, b)
        if key not in c.refs:
            c.refs[key] = SC.compose(frames[a:b + 1], fields[a:b], spec, order)
        return c.refs[key]

    c.reference = reference
    c.ref = reference("all", SC.ALL)
    c.plain = reference("no-repair", SC.without(SC.ALL, "repair"))
    print("observed on this clip:", SC.observed(c.ref, c.plain))
    SC.check_preconditions(c.ref, c.plain)
    return c


@pytest.fixture(scope="module")
def streamed(clip):
    """the all-stages stream's record at batch_pairs = 4: 4 + 4 + 1, a one-pair flush behind a carried transition"""
    return fresh(4, SC.ALL, clip.frames)


# ---- a. all stages on, every batching ----
@pytest.mark.parametrize("batch_pairs", (1, 3, 4, 8))
def test_all_stages_equal_the_composed_reference_at_every_batching(clip, batch_pairs):
    got = fresh(batch_pairs, SC.ALL, clip.frames)
    assert len(got.cells) == clip.n and len(got.links) == clip.n - 1
    SC.same_record(got, clip.ref)


# ---- b. the order is what the clip tests ----
@pytest.mark.parametrize("name", sorted(SC.WRONG))
def test_a_wrong_order_changes_the_named_output(clip, streamed, name):
    order, outputs = SC.WRONG[name]
    wrong = SC.compose(clip.frames, clip.fields, SC.ALL, order)
    for out in outputs:
        assert SC.differs(wrong, clip.ref, out), out
        if out in SC.OUTPUTS:                                        # ... so the stream, which equals the right chain, is not this one
            assert SC.differs(wrong, streamed, out), out
    SC.same_record(streamed, clip.ref)


# ---- c. leave one out ----
@pytest.mark.parametrize("stage", SC.LEAVE_OUT)
def test_all_stages_but_one_equal_the_reference_without_it(clip, stage):
    spec = SC.without(SC.ALL, stage)
    want = clip.reference("without-" + stage, spec)
    got = fresh(3, spec, clip.frames)
    SC.same_record(got, want)
    if stage == "model":
        assert all((r[:, 1] == 0).all() for r in got.records)        # blob keys all 0


# ---- d. the resident route agrees ----
def test_the_resident_route_agrees(clip, streamed):
    from opticalflowclustering_amd.pipeline import ClipPipeline
    from opticalflowclustering_amd.vis import grid_assign_counts
    ref, blob = clip.ref, SC.BLOBS
    pipe = ClipPipeline(SC.W, SC.H, len(clip.frames), batch_pairs=4, n_engines=2)
    try:
        pipe.upload_frames(clip.frames)
        pipe.run_flow()
        assert np.array_equal(pipe.flows_host().view(np.uint32), clip.fields.view(np.uint32))
        photo = pipe.photometric(**SC.STRICT)
        counts = pipe.repair(**SC.REPAIR)
        pipe.capture_moves()
        cam = pipe.compensate_camera(SC.CAMERA)
        hist = pipe.uv_histogram(*SC.HISTOGRAM)
        b = pipe.blobs(by=SC.CENTRES, mean=None, consistent=True, links=blob["max_links"], labels=False, thr=blob["thr"],
                       connectivity=blob["connectivity"], min_area=blob["min_area"], max_blobs=blob["max_blobs"])
        cell = pipe.cell_clusters(SC.ROWS, SC.COLS, centers=SC.CENTRES)
        residual = pipe.flows_host()
    finally:
        pipe.close()
    res = types.SimpleNamespace(**{k: None for k in SC.OUTPUTS})
    res.photo_stats, res.repair_counts, res.cam_params, res.cam_status, res.hist = photo.stats, counts, cam.params, cam.status, hist.table
    res.records, res.found, res.links, res.nlinks = b.records, b.found, b.links, b.nlinks
    # cell_clusters centres by the field mean and promises no bit equality: the counts go through mean 0 on the same field
    res.counts, res.sums = grid_assign_counts(residual, SC.CENTRES, SC.ROWS, SC.COLS, mean=None, sums=True)
    names = ("photo_stats", "repair_counts", "cam_params", "cam_status", "hist", "records", "found", "links", "nlinks", "counts", "sums")
    SC.same_record(res, streamed, names)
    SC.same_record(res, ref, names)
    assert np.array_equal(residual.view(np.uint32), ref.field.view(np.uint32))
    assert cell.shape == ref.counts.shape and np.array_equal(cell.sum(-1), ref.counts.sum(-1))       # every cell's pixels, whatever the label


# ---- e. clips in sequence on one stream ----
def test_clips_in_sequence_cut_the_chain_and_add_to_the_histogram(clip):
    first, second = clip.reference("all", SC.ALL, 0, 4), clip.reference("all", SC.ALL, 4, 9)
    per_pair = [o for o in SC.OUTPUTS if o != "hist"]
    SC.same_record(first, SC.part(clip.ref, 0, 4), per_pair)         # a pair's outputs depend on that pair alone
    SC.same_record(second, SC.part(clip.ref, 4, 9), per_pair)
    st = make_stream(3, SC.ALL)
    try:
        total = np.zeros_like(clip.ref.hist)
        for frames, want in ((clip.frames, clip.ref), (clip.frames[:5], first), (clip.frames[4:], second)):
            got, _ = run(st, frames, reset=False)
            SC.same_record(got, want, per_pair)
            assert len(got.links) == len(frames) - 2                 # 8, 3 and 4: no transition into a clip's first pair
            total += want.hist
            assert np.array_equal(got.hist, total)                   # the clips add to the table
        assert np.array_equal(st.histogram(reset=True).table, total)
        assert not st.histogram().table.any()
    finally:
        st.close()


# ---- f. reconfiguration between clips ----
def test_reconfiguration_between_clips_leaves_nothing_behind(clip, streamed):
    small = clip.reference("small", SC.SMALL)
    assert SC.differs(small, clip.ref, "records") and small.sums is None and small.counts.shape[-1] == 2
    st = make_stream(4, SC.SMALL)                                    # a stream that starts small and grows into the large one
    try:
        fresh_small, _ = run(st, clip.frames)
        SC.same_record(fresh_small, small)
        configure(st, SC.ALL)                                        # the second repair snapshot and the sums appear only now
        SC.same_record(run(st, clip.frames)[0], clip.ref)
    finally:
        st.close()
    st = make_stream(4, SC.ALL)
    try:
        first, _ = run(st, clip.frames)
        SC.same_record(first, clip.ref)
        configure(st, SC.SMALL)                                      # smaller tables, another layout, one repair snapshot
        got, _ = run(st, clip.frames)
        SC.same_record(got, small)
        SC.same_record(got, fresh_small)
        configure(st, SC.ALL)
        again, _ = run(st, clip.frames)
        SC.same_record(again, clip.ref)
        SC.same_record(again, first)
        SC.same_record(again, streamed)
        configure(st, SC.NONE)                                       # every stage off: a plain stream
        got, _ = run(st, clip.frames)
        plain = fresh(4, SC.NONE, clip.frames)
        for o in SC.OUTPUTS:
            assert (getattr(got, o) is None) == (o != "cells"), o
        SC.same_record(got, plain)
        SC.same_record(got, clip.reference("none", SC.NONE))
    finally:
        st.close()


NEW_MIN_AREA = 400                   # between the areas of the clip's blobs: some of them stop voting


def test_set_blobs_alone_through_the_c_abi_keeps_the_links_and_takes_the_new_arguments(clip):
    """ofc_stream_set_blobs with a new min_area and max_blobs and no ofc_stream_set_blob_links behind it, which FlowStream
    never does: the links stay on, vote under the new min_area, and the table is read with the new max_blobs"""
    L = _L()
    blob = dict(SC.BLOBS, min_area=NEW_MIN_AREA, max_blobs=64)
    spec = dict(SC.ALL, blobs=blob)
    want = clip.reference("c-abi", spec)
    assert SC.differs(want, clip.ref, "links") and SC.differs(want, clip.ref, "records")             # the new min_area bites
    st = make_stream(4, SC.ALL)
    try:
        first, _ = run(st, clip.frames)
        SC.same_record(first, clip.ref)
        L.check(L.load().ofc_stream_set_blobs(st._h, blob["connectivity"], float(blob["thr"]), blob["min_area"], blob["max_blobs"]))
        st.blob_args = (blob["connectivity"], float(blob["thr"]), blob["min_area"], blob["max_blobs"])
        assert st.max_links == SC.BLOBS["max_links"]
        got, _ = run(st, clip.frames)
        SC.same_record(got, want)
    finally:
        st.close()


# ---- g. pairs_done with every stage on ----
@pytest.mark.parametrize("batch_pairs", (3, 4))
def test_pairs_done_never_runs_ahead_or_back_with_every_stage_on(clip, batch_pairs):
    st = make_stream(batch_pairs, SC.ALL)
    try:
        got, done = run(st, clip.frames)
    finally:
        st.close()
    assert len(done) == len(clip.frames)
    for i, d in enumerate(done):                                     # after push i, (i // batch) whole batches are submitted
        assert 0 <= d <= (i // batch_pairs) * batch_pairs, (i, d)
        assert d % batch_pairs == 0, (i, d)                          # whole batches complete
    assert all(a <= b for a, b in zip(done, done[1:])), done
    assert len(got.cells) == clip.n == 9                             # the finish delivers every pair
    SC.same_record(got, clip.ref)
