"""The frame stream with the forward-backward check and the trajectories in the full chain (csrc/stream_api.cpp; FlowStream)
against the staged routes: test_gpu_stream_compose.py's sections for the two stages that joined submit() after it was written.

One clip of nine pairs goes through a stream with the forward-backward check, the repair, the trajectories by the check's
states, the link moves, the camera, the cell means, the model, the histogram, the blobs and their links all on (SC.ALL_FB),
and once with the photometric check in the other one's place (SC.ALL_TRAJ).  Every output is compared bit for bit with
stream_compose_cases.compose over the engine's pairwise fields of both directions, one pair at a time: deliberately not the
bidirectional entry point the stream itself uses, so that a pair map or a direction that entry point got wrong would show.
Both new steps of compose are integer CPU models (consistency_cases.reference, trajectory_cases.reference), so equality is
the bar; test_stream_compose_host.py proves them in the chain on the CPU."""
import types

import numpy as np
import pytest

from tests import stream_compose_cases as SC
from tests import trajectory_cases as TC

pytestmark = pytest.mark.gpu

PER_PAIR = tuple(o for o in SC.OUTPUTS if o != "hist" and o not in SC.TRAJ)       # what a slice of a clip has of the whole clip's
NOT_TRAJ = tuple(o for o in SC.OUTPUTS if o not in SC.TRAJ)


def make_stream(batch_pairs, spec):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(SC.W, SC.H, batch_pairs=batch_pairs, rows=SC.ROWS, cols=SC.COLS, **spec)


def configure(st, spec):
    """an existing, idle stream to another spec, stage by stage, through FlowStream's setters.  The stream has one state map:
    the trajectories that go by it are taken off first, the check that leaves before the other one comes"""
    photo, cons, traj = spec.get("photometric"), spec.get("consistency"), spec.get("trajectories")
    st.set_trajectories(on=False)
    st.set_model(spec["centers"], None, spec["sums"])
    st.set_histogram(*(spec["histogram"] or (None,)))
    st.set_camera(spec["camera"])
    st.set_blobs(**(spec["blobs"] or dict(connectivity=None)))
    if not photo:
        st.set_photometric(on=False)
    if not cons:
        st.set_consistency(on=False)
    if photo:
        st.set_photometric(**photo)
    if cons:
        st.set_consistency(**cons)
    st.set_repair(**(spec["repair"] or dict(on=False)))
    if traj:
        st.set_trajectories(**traj)


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
    if st.consist_args:
        r.consist_counts = st.consistency_stats()
    if st.repair_args:
        r.repair_counts = st.repair_stats()
    if st.traj_points:
        tr = st.trajectories()
        r.traj_pos, r.traj_len, r.traj_why = tr.pos, tr.length, tr.why
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


def bidirectional(frames):
    """FlowEngine.calc_frames_dev_bidir over the whole clip in one batch -> (forward, backward) fields"""
    from opticalflowclustering_amd import _lib as L
    from opticalflowclustering_amd.flow import FlowEngine
    n, half = len(frames) - 1, (len(frames) - 1) * SC.H * SC.W * 8
    eng = FlowEngine(SC.W, SC.H, max_batch=n)
    fd, od = L.DeviceBuffer(frames.nbytes).upload(np.ascontiguousarray(frames)), L.DeviceBuffer(2 * half)
    try:
        eng.calc_frames_dev_bidir(fd.ptr, n + 1, od.ptr, od.ptr + half)
        return od.download((n, SC.H, SC.W, 2), np.float32), od.download((n, SC.H, SC.W, 2), np.float32, offset=half)
    finally:
        eng.close()
        fd.free()
        od.free()


@pytest.fixture(scope="module")
def clip():
    """the clip, its nine pairwise fields in both directions from one engine, one pair at a time; the composed reference of
    ALL_FB and the one without the repair; the preconditions of the clip.  Read-only."""
    from opticalflowclustering_amd.flow import FlowEngine
    frames = SC.clip()
    n = len(frames) - 1
    eng = FlowEngine(SC.W, SC.H, max_batch=1)
    try:
        fields = np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(n)])
        back = np.stack([eng.calc(frames[t + 1], frames[t]) for t in range(n)])
    finally:
        eng.close()
    fields.setflags(write=False)
    back.setflags(write=False)
    # the entry point the stream uses gives exactly these: a pair's field depends on neither its batch nor its direction slot
    fwd2, bwd2 = bidirectional(frames)
    assert np.array_equal(fwd2.view(np.uint32), fields.view(np.uint32)), "calc_frames_dev_bidir: forward fields"
    assert np.array_equal(bwd2.view(np.uint32), back.view(np.uint32)), "calc_frames_dev_bidir: backward fields"
    c = types.SimpleNamespace(frames=frames, fields=fields, back=back, n=n, refs={})

    def reference(name, spec, a=0, b=n):
        """compose of pairs a .. b-1 under a spec, computed once per name"""
        key = (name, a, b)
        if key not in c.refs:
            c.refs[key] = SC.compose(frames[a:b + 1], fields[a:b], spec, back=back[a:b])
        return c.refs[key]

    c.reference = reference
    c.ref = reference("all-fb", SC.ALL_FB)
    c.plain = reference("fb-no-repair", SC.without(SC.ALL_FB, "repair"))
    print("observed on this clip:", SC.observed_fb(c.ref, c.plain))
    SC.check_preconditions_fb(c.ref, c.plain)
    return c


@pytest.fixture(scope="module")
def streamed(clip):
    """the ALL_FB stream's record at batch_pairs = 4: 4 + 4 + 1, a one-pair flush behind a carried row of points"""
    return fresh(4, SC.ALL_FB, clip.frames)


# ---- a. all stages on, every batching ----
@pytest.mark.parametrize("batch_pairs", (1, 3, 4, 8))
def test_all_fb_stages_equal_the_composed_reference_at_every_batching(clip, batch_pairs):
    got = fresh(batch_pairs, SC.ALL_FB, clip.frames)
    assert len(got.cells) == clip.n and len(got.links) == clip.n - 1
    assert got.consist_counts.shape == (clip.n, 4) and got.traj_pos.shape == (clip.n + 1, len(SC.SEEDS), 2)
    SC.same_record(got, clip.ref)


@pytest.mark.parametrize("batch_pairs", (3, 4))
def test_the_photometric_chain_with_trajectories_equals_the_composed_reference(clip, batch_pairs):
    want = clip.reference("all-traj", SC.ALL_TRAJ)
    assert (want.traj_why == TC.UNTRUSTED).any() and SC.differs(want, clip.ref, "traj_pos")
    got = fresh(batch_pairs, SC.ALL_TRAJ, clip.frames)
    assert got.consist_counts is None and got.photo_stats is not None
    SC.same_record(got, want)


# ---- b. the order is what the clip tests ----
@pytest.mark.parametrize("name", sorted(SC.WRONG_FB))
def test_a_wrong_fb_chain_changes_the_named_output(clip, streamed, name):
    wrong, outputs = SC.compose_wrong_fb(name, clip.frames, clip.fields, clip.back)
    for out in outputs:
        assert out in SC.OUTPUTS
        assert SC.differs(wrong, clip.ref, out), out
        assert SC.differs(wrong, streamed, out), out                 # the stream, which equals the right chain, is not this one
    SC.same_record(streamed, clip.ref)


# ---- c. leave one out ----
@pytest.mark.parametrize("stage", SC.LEAVE_OUT_FB)
def test_all_fb_stages_but_one_equal_the_reference_without_it(clip, streamed, stage):
    spec = SC.without(SC.ALL_FB, stage)
    want = clip.reference("fb-without-" + stage, spec)
    got = fresh(3, spec, clip.frames)
    SC.same_record(got, want)
    if stage == "consistency":
        assert spec["trajectories"]["use_state"] is False and got.traj_pos is not None and got.consist_counts is None
        with pytest.raises(ValueError, match="check"):               # the points cannot go by the states of no check
            make_stream(3, dict(spec, trajectories=SC.ALL_FB["trajectories"]))
    if stage == "trajectories":                                      # nothing depends on the stage
        assert got.traj_pos is None
        SC.same_record(got, streamed, NOT_TRAJ)
        SC.same_record(got, clip.ref, NOT_TRAJ)
    if stage == "model":
        assert all((r[:, 1] == 0).all() for r in got.records)        # blob keys all 0


# ---- d. the resident route agrees ----
def test_the_resident_bidirectional_route_agrees(clip, streamed):
    from opticalflowclustering_amd.pipeline import ClipPipeline
    from opticalflowclustering_amd.vis import grid_assign_counts
    ref, blob, check = clip.ref, SC.BLOBS, SC.CHECK_FB
    pipe = ClipPipeline(SC.W, SC.H, len(clip.frames), batch_pairs=4, n_engines=2)
    try:
        pipe.upload_frames(clip.frames)
        pipe.run_flow_bidirectional()
        assert np.array_equal(pipe.flows_host().view(np.uint32), clip.fields.view(np.uint32))
        assert np.array_equal(pipe.flows_bwd_host().view(np.uint32), clip.back.view(np.uint32))
        cons = pipe.consistency(check["alpha"], check["beta"])
        counts = pipe.repair(**SC.REPAIR)
        tr = pipe.trajectories(SC.SEEDS, consistent=True, keep=check["keep"])
        pipe.capture_moves()
        cam = pipe.compensate_camera(SC.CAMERA)
        hist = pipe.uv_histogram(*SC.HISTOGRAM)
        b = pipe.blobs(by=SC.CENTRES, mean=None, consistent=True, links=blob["max_links"], labels=False, thr=blob["thr"],
                       connectivity=blob["connectivity"], min_area=blob["min_area"], max_blobs=blob["max_blobs"])
        residual = pipe.flows_host()
    finally:
        pipe.close()
    assert np.array_equal(cons.state, ref.state_pre)
    res = types.SimpleNamespace(**{k: None for k in SC.OUTPUTS})
    res.consist_counts, res.repair_counts, res.cam_params, res.cam_status, res.hist = cons.counts, counts, cam.params, cam.status, hist.table
    res.traj_pos, res.traj_len, res.traj_why = tr.pos, tr.length, tr.why
    res.records, res.found, res.links, res.nlinks = b.records, b.found, b.links, b.nlinks
    res.counts, res.sums = grid_assign_counts(residual, SC.CENTRES, SC.ROWS, SC.COLS, mean=None, sums=True)
    names = ("consist_counts", "repair_counts", "cam_params", "cam_status", "hist", "records", "found", "links", "nlinks", "counts",
             "sums") + SC.TRAJ
    SC.same_record(res, streamed, names)
    SC.same_record(res, ref, names)
    assert np.array_equal(residual.view(np.uint32), ref.field.view(np.uint32))


# ---- e. clips in sequence on one stream ----
def test_fb_clips_in_sequence_reseed_the_points_and_cut_the_chain(clip):
    first, second = clip.reference("all-fb", SC.ALL_FB, 0, 4), clip.reference("all-fb", SC.ALL_FB, 4, 9)
    SC.same_record(first, SC.part(clip.ref, 0, 4), PER_PAIR)         # a pair's outputs depend on that pair alone
    SC.same_record(second, SC.part(clip.ref, 4, 9), PER_PAIR)
    assert not np.array_equal(second.traj_pos, clip.ref.traj_pos[4:])              # ... its points on where the clip began
    st = make_stream(3, SC.ALL_FB)
    try:
        total = np.zeros_like(clip.ref.hist)
        for frames, want in ((clip.frames, clip.ref), (clip.frames[:5], first), (clip.frames[4:], second)):
            got, _ = run(st, frames, reset=False)
            SC.same_record(got, want, PER_PAIR + SC.TRAJ)            # the points placed afresh at this clip's first pair
            assert np.array_equal(got.traj_pos[0], SC.SEEDS) and len(got.traj_pos) == len(frames)
            assert len(got.links) == len(frames) - 2
            total += want.hist
            assert np.array_equal(got.hist, total)
        st.push(clip.frames[0])
        for call in (st.consistency_stats, st.trajectories):
            with pytest.raises(ValueError, match="holds frames"):    # frames held: not idle
                call()
        for f in clip.frames[1:3]:
            st.push(f)
        got = read(st, st.finish_clusters())
        SC.same_record(got, clip.reference("all-fb", SC.ALL_FB, 0, 2), PER_PAIR + SC.TRAJ)
    finally:
        st.close()


# ---- f. reconfiguration between clips ----
def test_reconfiguration_between_the_checks_leaves_nothing_behind(clip, streamed):
    """ALL_FB -> ALL (the photometric check takes over the stream's one state map, the points go) -> ALL_TRAJ (the points
    come back, by the other check's states) -> SMALL -> ALL_FB"""
    specs = dict(all=SC.ALL, traj=SC.ALL_TRAJ, small=SC.SMALL)
    refs = {k: clip.reference("reconf-" + k, v) for k, v in specs.items()}
    fresh_records = {k: fresh(4, v, clip.frames) for k, v in specs.items()}
    for k in specs:
        SC.same_record(fresh_records[k], refs[k])
    assert SC.differs(refs["traj"], clip.ref, "traj_why") and SC.differs(refs["small"], clip.ref, "records")
    st = make_stream(4, SC.ALL_FB)
    try:
        first, _ = run(st, clip.frames)
        SC.same_record(first, clip.ref)
        with pytest.raises(ValueError):                              # one state map: the other check is refused ...
            st.set_photometric(**SC.STRICT)
        assert st.photo_args is None and st.consist_args is not None
        SC.same_record(run(st, clip.frames)[0], clip.ref)            # ... and nothing has changed
        for k in ("all", "traj"):
            configure(st, specs[k])
            got, _ = run(st, clip.frames)
            SC.same_record(got, refs[k])
            SC.same_record(got, fresh_records[k])
            with pytest.raises(ValueError):
                st.set_consistency(**SC.CHECK_FB)
            assert st.consist_args is None and st.photo_args is not None
            again, _ = run(st, clip.frames)
            SC.same_record(again, refs[k])
        configure(st, SC.SMALL)
        got, _ = run(st, clip.frames)
        SC.same_record(got, refs["small"])
        SC.same_record(got, fresh_records["small"])
        configure(st, SC.ALL_FB)
        again, _ = run(st, clip.frames)
        SC.same_record(again, clip.ref)
        SC.same_record(again, first)
        SC.same_record(again, streamed)
    finally:
        st.close()


# ---- g. the table grows under the carry ----
WALK_PAIRS = 264                     # PairTable starts at 256 pairs


def test_the_points_table_grows_under_the_carried_row(clip):
    """a palindrome walk over the clip, 264 pairs at 8 a batch: traj_pos is reallocated at pair 256, between two batches, and
    the next batch starts from the carried row of the new buffer"""
    order = np.concatenate([np.arange(clip.n + 1), np.arange(clip.n - 1, 0, -1)])            # 0 .. 9, 8 .. 1
    walk = np.concatenate([order] * (WALK_PAIRS // len(order) + 1) + [order[:1]])[:WALK_PAIRS + 1]
    # pair (a -> a + 1) is the forward field of pair a, pair (a + 1 -> a) its backward field: nothing is computed again
    fields = np.stack([clip.fields[a] if b == a + 1 else clip.back[b] for a, b in zip(walk[:-1].tolist(), walk[1:].tolist())])
    assert len(fields) == WALK_PAIRS and all(abs(a - b) == 1 for a, b in zip(walk[:-1].tolist(), walk[1:].tolist()))
    seeds = np.ascontiguousarray(SC.SEEDS[:64])
    want = TC.reference(fields, seeds)
    assert (want[1] > 256).any() and (want[1] < 256).any()          # points that live past the growth, and points that do not
    st = make_stream(8, dict(trajectories=dict(seeds=seeds)))
    try:
        for t in walk.tolist():
            st.push(clip.frames[t])
        cells = st.finish()
        tr = st.trajectories()
    finally:
        st.close()
    assert len(cells) == WALK_PAIRS and tr.pos.shape == (WALK_PAIRS + 1, 64, 2)
    for got, exp, dt in zip((tr.pos, tr.length, tr.why), want, (np.int32, np.int32, np.uint8)):
        assert got.dtype == dt and got.shape == exp.shape and np.array_equal(got, exp), np.argwhere(got != exp)[:5]


# ---- h. pairs_done with every stage on ----
@pytest.mark.parametrize("batch_pairs", (1, 4))
def test_pairs_done_never_runs_ahead_or_back_with_the_fb_chain(clip, batch_pairs):
    st = make_stream(batch_pairs, SC.ALL_FB)
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
