"""stream_compose_cases.compose on the CPU: the composed reference is code that can be wrong too, so on a synthetic input it
must behave as test_gpu_stream_compose.py assumes.  No flow engine and no device: the steps without a bit-exact CPU model are
replaced by the numpy models of the stages' own case files (HostOps), the camera by camera_motion_cases.fit and predict.
The second half does the same for the forward-backward check and the trajectories in the chain, as
test_gpu_stream_compose_bidir.py assumes them: against the per-pixel and per-point loops, which share no code with the
references that compose() calls."""
import types

import numpy as np
import pytest

from tests import blob_cases as BC
from tests import blob_link_cases as LC
from tests import camera_motion_cases as CM
from tests import consistency_cases as CC
from tests import grid_assign_cases as GA
from tests import motion_grid_cases as MC
from tests import photometric_cases as PC
from tests import stream_compose_cases as SC
from tests import trajectory_cases as TC
from tests import uv_hist_cases as UH

W, H, N = 48, 32, 9
ROWS, COLS = 4, 6
THRESHOLDS = CM.DEFAULT_THRESHOLDS


class HostOps:
    """SC.DeviceOps' interface on numpy models"""

    @staticmethod
    def camera_fit(field, kind):
        fits = [CM.fit(f, CM.KIND[kind], THRESHOLDS) for f in field]
        return np.stack([x["models"][-1] for x in fits]), np.array([x["status"] for x in fits], np.int32)

    @staticmethod
    def camera_sub(field, params):
        out = np.array(field, np.float32)
        for t, p in enumerate(params):
            eu, ev = CM.predict(p, field.shape[2], field.shape[1])
            ok = np.isfinite(field[t]).all(-1)                       # a non-finite vector passes through unchanged
            sub = np.stack([field[t, ..., 0].astype(np.float64) - eu, field[t, ..., 1].astype(np.float64) - ev], -1).astype(np.float32)
            out[t] = np.where(ok[..., None], sub, field[t])
        return out

    @staticmethod
    def camera(field, kind):
        params, status = HostOps.camera_fit(field, kind)
        return HostOps.camera_sub(field, params), params, status

    @staticmethod
    def cells(field, rows, cols):
        n, h, w = field.shape[:3]
        ys, xs = h // rows, w // cols
        with np.errstate(invalid="ignore", over="ignore"):
            return np.stack([[field[t, cy * ys:(cy + 1) * ys, cx * xs:(cx + 1) * xs].reshape(-1, 2).astype(np.float64).mean(0)
                              for cy in range(rows) for cx in range(cols)] for t in range(n)]).astype(np.float32)

    @staticmethod
    def _labels(field, centres):
        with np.errstate(invalid="ignore", over="ignore"):
            return GA.model_labels(field, centres)

    @staticmethod
    def counts(field, centres, rows, cols):
        clean = np.where(np.isfinite(field), field, 0)               # fsum of the model refuses inf - inf; the labels are kept
        return MC.model_counts(HostOps._labels(field, centres), len(centres), rows, cols, clean)

    @staticmethod
    def hist(field, bins, rng):
        return UH.model(field, bins, rng)

    @staticmethod
    def keys(field, centres, thr):
        with np.errstate(invalid="ignore", over="ignore"):
            s = field[..., 0] * field[..., 0] + field[..., 1] * field[..., 1]
            moving = s >= np.float32(thr) * np.float32(thr)
        lab = np.zeros(field.shape[:3], np.uint8) if centres is None else HostOps._labels(field, centres)
        return np.where(moving, lab, 255).astype(np.uint8)

    @staticmethod
    def components(keys, field, connectivity, min_area, max_blobs):
        labels = np.stack([BC.label_one(k, connectivity) for k in keys])
        tabs = [BC.table(BC.records_one(keys[t], labels[t], field[t]), min_area, max_blobs) for t in range(len(keys))]
        return labels, [r for r, _ in tabs], np.array([f for _, f in tabs], np.int32)

    @staticmethod
    def links(labels, move_field, moves, min_area, max_links):
        return LC.links_of(labels, moves, min_area, max_links)


SPEC = dict(centers=np.array([[0.0, 0.0], [2.5, -1.5], [-1.0, 2.0]]), sums=True, histogram=(64, 2.0), camera="affine",
            blobs=dict(thr=1.0, connectivity=8, min_area=3, max_blobs=64, max_links=64),
            photometric=dict(tau=6.0, kappa=0.25), repair=dict(radius=1, rounds=2, min_count=2))


def run(inp, spec=SPEC, order=SC.DOCUMENTED, a=0, b=N):
    return SC.compose(inp.frames[a:b + 1], inp.fields[a:b], spec, order, ops=HostOps, rows=ROWS, cols=COLS)


@pytest.fixture(scope="module")
def inp():
    """nine pairs: photometric_cases' sliding texture, a smooth field of about its motion, a rectangle of other motion that
    itself moves, strips of NaN (one of them inside that rectangle) and a strip of vectors at and past 1024.  Read-only."""
    r = np.random.default_rng(5)
    frames = PC.frames_smooth(r, N, H, W)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    fields = np.empty((N, H, W, 2), np.float32)
    for t in range(N):
        u = 1.2 + 0.004 * (xx - W / 2) + 0.002 * (yy - H / 2) + r.integers(-8, 9, (H, W)) / 256.0
        v = -0.7 - 0.003 * (xx - W / 2) + 0.004 * (yy - H / 2) + r.integers(-8, 9, (H, W)) / 256.0
        f = np.stack([u, v], -1)
        f[6 + t:16 + t, 8 + 2 * t:20 + 2 * t] += (2.5, -1.5)           # moves by (2, 1) per pair
        f[24:29, 30:42] += (-1.0, 2.0)
        f[2, 30:40] = np.nan
        f[9 + t, 11 + 2 * t:15 + 2 * t] = np.nan                       # inside the rectangle: no move before the repair, a vote after
        f[20, 2:8, 0] = (1024.0, 2000.0, -1024.0, 1500.0, 3.0e38, -np.inf)
        fields[t] = f
    frames.setflags(write=False)
    fields.setflags(write=False)
    return types.SimpleNamespace(frames=frames, fields=fields)


@pytest.fixture(scope="module")
def ref(inp):
    return run(inp)


def test_the_input_gives_every_stage_work(inp, ref):
    assert (ref.photo_stats[:, 1:4].sum(1) > 0).all() and (ref.photo_stats[:, PC.INVALID] >= 16).all()
    assert (ref.repair_counts[:, 1] > 0).all() and ref.repair_counts[:, 2].sum() > 0
    assert (ref.cam_status == 0).all() and (np.abs(ref.cam_params[:, [0, 3]]) > 0.2).all()
    assert len(np.unique(ref.counts.argmax(-1))) >= 2
    assert min(len(x) for x in ref.records) >= 2 and ref.nlinks.min() >= 1 and ref.nlinks.max() >= 2
    assert ref.hist[-1] > 0 and ref.hist[:64 * 64].sum() > 0
    assert ((ref.keys_pre == 255) & (ref.keys != 255)).any()
    assert ref.cells.shape == (N, ROWS * COLS, 2) and ref.sums.shape == (N, ROWS * COLS, 3, 2)


@pytest.mark.parametrize("name", sorted(SC.WRONG))
def test_every_wrong_order_differs_in_its_named_output(inp, ref, name):
    order, outputs = SC.WRONG[name]
    wrong = run(inp, order=order)
    for out in outputs:
        assert SC.differs(wrong, ref, out), out
    SC.same_record(run(inp), ref)                                    # ... and the documented chain repeats itself


def test_differs_and_same_record_see_a_single_bit(ref):
    other = types.SimpleNamespace(**vars(ref))
    other.cam_params = ref.cam_params.copy()
    other.cam_params.view(np.int64)[3, 4] ^= 1
    assert SC.differs(other, ref, "cam_params") and not SC.differs(other, ref, "cells")
    with pytest.raises(AssertionError):
        SC.same_record(other, ref)
    other = types.SimpleNamespace(**vars(ref))
    other.links = [x.copy() for x in ref.links]
    other.links[2][0, 2] += 1
    assert SC.differs(other, ref, "links")
    with pytest.raises(AssertionError):
        SC.same_record(other, ref)
    other = types.SimpleNamespace(**vars(ref))
    other.cells = np.where(ref.cells == 0, np.float32(-0.0), ref.cells)          # a sign of zero is a bit too
    other.cells = other.cells.copy()
    other.cells.view(np.uint32)[0, 0, 0] ^= 1 << 31
    with pytest.raises(AssertionError):
        SC.same_record(other, ref)


# the outputs a stage can reach: switching it off must leave every other output as it was
REACH = {
    "photometric": ("photo_stats", "repair_counts", "cam_params", "cam_status", "cells", "counts", "sums", "hist", "records", "found",
                    "links", "nlinks"),
    "repair": ("repair_counts", "cam_params", "cam_status", "cells", "counts", "sums", "hist", "records", "found", "links", "nlinks"),
    "camera": ("cam_params", "cam_status", "cells", "counts", "sums", "hist", "records", "found", "links", "nlinks"),
    "model": ("counts", "sums", "records", "found", "links", "nlinks"),
    "histogram": ("hist",),
    "links": ("links", "nlinks"),
    "blobs": ("records", "found", "links", "nlinks"),
}


@pytest.mark.parametrize("stage", SC.LEAVE_OUT)
def test_a_stage_switched_off_leaves_the_stages_before_it_untouched(inp, ref, stage):
    got = run(inp, SC.without(SPEC, stage))
    SC.same_record(got, ref, [o for o in SC.OUTPUTS if o not in REACH[stage]])
    gone = {"photometric": ("photo_stats",), "repair": ("repair_counts",), "camera": ("cam_params", "cam_status"),
            "model": ("counts", "sums"), "histogram": ("hist",), "links": ("links", "nlinks"),
            "blobs": ("records", "found", "links", "nlinks")}[stage]
    for o in gone:
        assert getattr(got, o) is None, o
    if stage == "photometric":                                       # the repair then sees a NULL state: only unusable vectors
        assert np.array_equal(got.repair_counts[:, 1] + got.repair_counts[:, 2], ref.photo_stats[:, PC.INVALID])
    if stage == "model":
        assert all((r[:, 1] == 0).all() for r in got.records)        # blob keys all 0


def test_everything_off_is_the_cell_means_of_the_field(inp):
    got = run(inp, SC.NONE)
    for o in SC.OUTPUTS:
        assert (getattr(got, o) is None) == (o != "cells"), o
    assert np.array_equal(got.cells.view(np.uint32), HostOps.cells(inp.fields, ROWS, COLS).view(np.uint32))
    assert np.array_equal(got.field.view(np.uint32), inp.fields.view(np.uint32))


def test_compose_writes_neither_input(inp):
    frames, fields = inp.frames.copy(), inp.fields.copy()
    assert not inp.frames.flags.writeable and not inp.fields.flags.writeable
    for order in (SC.DOCUMENTED,) + tuple(o for o, _ in SC.WRONG.values()):
        run(inp, order=order)
    assert np.array_equal(inp.frames, frames) and np.array_equal(inp.fields.view(np.uint32), fields.view(np.uint32))


def test_nine_pairs_equal_four_four_and_one_with_the_transitions_across_the_cuts(inp, ref):
    """what the stream's carried pair implements: a pair's outputs depend on that pair alone, a transition on its two pairs"""
    parts = [run(inp, a=a, b=b) for a, b in ((0, 4), (4, 8), (8, 9))]
    whole = types.SimpleNamespace(**{k: None for k in SC.OUTPUTS})
    for name in SC.PER_PAIR:
        if getattr(ref, name) is not None:                           # SPEC has no forward-backward check: no consist_counts
            setattr(whole, name, np.concatenate([getattr(p, name) for p in parts]))
    whole.records = [x for p in parts for x in p.records]
    whole.hist = sum(p.hist for p in parts)
    spec = SPEC["blobs"]
    links, nlinks = [], []
    for i, p in enumerate(parts):
        if i:                                                        # the carried pair: label map and moves of the part before
            q = parts[i - 1]
            rows, m = LC.deliver(LC.links_one(q.labels[-1], q.moves[-1], p.labels[0], spec["min_area"]), spec["max_links"])
            links.append(rows)
            nlinks.append(m)
        links += list(p.links)
        nlinks += list(p.nlinks)
    whole.links, whole.nlinks = links, np.array(nlinks, np.int32)
    assert len(links) == N - 1 and len(parts[2].links) == 0
    SC.same_record(whole, ref)
    for a, b in ((0, 4), (4, 8), (8, 9), (2, 7)):
        SC.same_record(SC.part(ref, a, b), run(inp, a=a, b=b), [o for o in SC.OUTPUTS if o != "hist"])


# ---- the forward-backward check and the trajectories in the chain ----
# every other pixel, then every pairing of SC.FRACTIONS on nine pixels of which some lie in the rectangle's path
SEEDS = np.concatenate([SC.grid_seeds(W, H, 2), np.array([[((10 + 8 * i) << 16) + fx, ((8 + 6 * j) << 16) + fy]
                                                          for j, fy in enumerate(SC.FRACTIONS) for i, fx in enumerate(SC.FRACTIONS)], np.int32)])
SPEC_FB = dict(SPEC, photometric=None, consistency=dict(alpha=0.01, beta=0.5, keep=(0,)), trajectories=dict(seeds=SEEDS, use_state=True))
SPEC_TRAJ = dict(SPEC, trajectories=dict(seeds=SEEDS, use_state=True))
RECT_MOVE = (2.5, -1.5)               # the rectangle's own motion; with the drift it lands (4, -2) px on, to the pixel
DISAGREE = ((12, 4, 3, 3), (30, 12, 9, 9))        # x, y, w, h relative to the rectangle's corner / in the frame: a patch the
#                                                   repair closes in two rounds, and one it cannot


def run_fb(inp, spec=SPEC_FB, order=SC.DOCUMENTED, a=0, b=N, back=None):
    back = inp.back if back is None else back
    return SC.compose(inp.frames[a:b + 1], inp.fwd[a:b], spec, order, ops=HostOps, rows=ROWS, cols=COLS, back=back[a:b])


@pytest.fixture(scope="module")
def inp_fb(inp):
    """nine pairs in both directions, after consistency_cases.smooth_fields and RECT: a smooth drift with a rectangle of other
    motion that itself moves; the backward field is the negated forward one taken where the forward one lands (the
    rectangle (4, -2) px on), plus patches of disagreement, one of them inside the rectangle; a strip of NaN in each
    direction and vectors at and past 1024 in the forward one.  Read-only."""
    r = np.random.default_rng(6)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    fwd, back = np.empty((N, H, W, 2), np.float32), np.empty((N, H, W, 2), np.float32)
    for t in range(N):
        u = 1.2 + 0.004 * (xx - W / 2) + 0.002 * (yy - H / 2)
        v = -0.7 - 0.003 * (xx - W / 2) + 0.004 * (yy - H / 2)
        f = np.stack([u, v], -1) + r.integers(-8, 9, (H, W, 2)) / 256.0
        b = -np.stack([u, v], -1) + r.integers(-8, 9, (H, W, 2)) / 256.0
        x0, y0 = 8 + 2 * t, 8 + t                                      # moves by (2, 1) per pair
        f[y0:y0 + 10, x0:x0 + 12] += RECT_MOVE
        b[y0 - 2:y0 + 8, x0 + 4:x0 + 16] -= RECT_MOVE
        f[24:29, 2:14] += (-1.0, 2.0)                                  # a second one that rests: it lands (0, 1) px on
        b[25:30, 2:14] -= (-1.0, 2.0)
        (dx, dy, w, h), (X, Y, w2, h2) = DISAGREE
        b[y0 - 2 + dy:y0 - 2 + dy + h, x0 + dx:x0 + dx + w] += (3.0, 2.0)
        b[Y:Y + h2, X:X + w2] += (-2.0, 3.0)
        f[2, 30:40] = np.nan
        b[28, 4:12] = np.nan
        f[20, 2:8, 0] = (1024.0, 2000.0, -1024.0, 1500.0, 3.0e38, -np.inf)
        fwd[t], back[t] = f, b
    fwd.setflags(write=False)
    back.setflags(write=False)
    return types.SimpleNamespace(frames=inp.frames, fwd=fwd, back=back)


@pytest.fixture(scope="module")
def ref_fb(inp_fb):
    return run_fb(inp_fb)


def test_the_fb_input_gives_the_new_stages_work(inp_fb, ref_fb):
    plain = run_fb(inp_fb, SC.without(SPEC_FB, "repair"))
    assert (ref_fb.consist_counts[:, [CC.MISMATCH, CC.LEAVES, CC.INVALID]] > 0).all()
    assert (ref_fb.consist_counts.sum(1) == W * H).all() and ref_fb.consist_counts.dtype == np.int64
    assert (ref_fb.repair_counts[:, 1] > 0).all() and (ref_fb.repair_counts[:, 2] > 0).all()
    assert ref_fb.traj_pos.shape == (N + 1, len(SEEDS), 2) and ref_fb.traj_pos.dtype == np.int32
    assert ref_fb.traj_len.dtype == np.int32 and ref_fb.traj_why.dtype == np.uint8
    assert set(ref_fb.traj_why.tolist()) == {TC.RAN, TC.UNTRUSTED, TC.LEAVES}    # a repaired field has no unusable vector in reach
    assert TC.INVALID in set(run_fb(inp_fb, SC.without(SC.without(SPEC_FB, "repair"), "consistency")).traj_why.tolist())
    assert min(len(x) for x in ref_fb.records) >= 2 and ref_fb.nlinks.min() >= 1
    assert ((ref_fb.keys_pre == 255) & (ref_fb.keys != 255)).any()

    # check_preconditions_fb and observed_fb are written for SC.SEEDS: the same conditions on this input's seeds
    moved = (ref_fb.traj_pos[-1] != plain.traj_pos[-1]).any(-1)
    _, _, why_pre = TC.reference(ref_fb.traj_field, SEEDS, ref_fb.state_pre, 1)
    assert ((ref_fb.traj_why == TC.RAN) & (ref_fb.traj_len == N)).any() and moved.any() and (why_pre != ref_fb.traj_why).any()


def test_the_consist_step_is_the_per_pixel_loop(inp_fb, ref_fb):
    state, counts, _ = CC.loop(inp_fb.fwd, inp_fb.back, *SC.quantise_fb(0.01, 0.5))
    assert SC.quantise_fb(0.01, 0.5) == (CC.ALPHA_Q, CC.BETA_Q)
    assert np.array_equal(ref_fb.state_pre, state) and np.array_equal(ref_fb.consist_counts, counts)
    assert (ref_fb.state != ref_fb.state_pre).any()                  # ... and the repair went on from those states
    other = run_fb(inp_fb, dict(SPEC_FB, consistency=dict(alpha=0.5, beta=0.25, keep=(0,))))
    assert np.array_equal(other.consist_counts, CC.loop(inp_fb.fwd, inp_fb.back, 32768, 1 << 30)[1])
    assert SC.differs(other, ref_fb, "consist_counts")


@pytest.mark.parametrize("spec_name", ("fb", "fb-keep-01", "photo", "no-state"))
def test_the_traj_step_is_the_per_point_loop(inp, inp_fb, ref_fb, spec_name):
    """on the field and the states of the chain at that point: repaired, not yet compensated"""
    if spec_name == "photo":
        got = SC.compose(inp.frames, inp.fields, SPEC_TRAJ, ops=HostOps, rows=ROWS, cols=COLS)
        keep, use_state = 1, True
    else:
        keep, use_state = (3, True) if spec_name == "fb-keep-01" else (1, spec_name != "no-state")
        spec = dict(SPEC_FB, trajectories=dict(seeds=SEEDS, use_state=use_state))
        if keep == 3:
            spec["consistency"] = dict(SPEC_FB["consistency"], keep=(0, 1))
        got = ref_fb if spec_name == "fb" else run_fb(inp_fb, spec)
    no_traj = SC.compose(inp.frames, inp.fields, SPEC, ops=HostOps, rows=ROWS, cols=COLS) if spec_name == "photo" else \
        run_fb(inp_fb, SC.without(SPEC_FB, "trajectories"))
    if keep == 1:                                                    # the field behind the repair is what the moves are taken from
        assert np.array_equal(got.traj_field.view(np.uint32), no_traj.move_field.view(np.uint32))
        assert np.array_equal(got.state, no_traj.state)
    pos, length, why = TC.loop(got.traj_field, SEEDS, got.state if use_state else None, keep)
    assert np.array_equal(got.traj_pos, pos) and np.array_equal(got.traj_len, length) and np.array_equal(got.traj_why, why)
    assert np.array_equal(got.traj_pos[0], SEEDS)
    if spec_name != "fb":
        assert SC.differs(got, ref_fb, "traj_pos") and SC.differs(got, ref_fb, "traj_why")


@pytest.mark.parametrize("name", sorted(SC.WRONG_FB))
def test_every_wrong_fb_chain_differs_in_its_named_output(inp_fb, ref_fb, name):
    wrong, outputs = SC.compose_wrong_fb(name, inp_fb.frames, inp_fb.fwd, inp_fb.back, SPEC_FB, ops=HostOps, rows=ROWS, cols=COLS)
    assert outputs
    for out in outputs:
        assert SC.differs(wrong, ref_fb, out), out
    SC.same_record(run_fb(inp_fb), ref_fb)                           # ... and the documented chain repeats itself


def test_the_table_of_wrong_fb_chains_is_the_issues():
    assert sorted(SC.WRONG_FB) == sorted(("traj-before-the-repair", "traj-after-the-camera", "traj-by-the-pre-repair-states",
                                          "fb-check-after-the-repair", "fb-check-on-the-residual",
                                          "fb-blobs-masked-by-the-pre-repair-states", "backward-fields-in-reverse-order"))
    assert SC.DOCUMENTED == ("photo", "consist", "repair", "traj", "moves", "camera", "cells", "counts", "hist", "blobs", "links")
    for order, _ in SC.WRONG_FB.values():                            # every chain has every stage of ALL_FB
        assert {"consist", "repair", "moves", "camera", "cells", "counts", "hist", "links"} <= set(order)
        assert {"traj", "traj_prestate"} & set(order) and {"blobs", "blobs_prestate"} & set(order)


@pytest.mark.parametrize("spec", (SPEC, SC.without(SPEC, "repair"), SC.without(SPEC, "photometric"), SC.NONE), ids=("all", "no-repair", "no-check", "none"))
def test_a_spec_without_the_new_stages_is_unchanged_by_the_new_order(inp, spec):
    new, old = run(inp, spec), run(inp, spec, order=SC.DOCUMENTED_BEFORE)
    SC.same_record(new, old)
    for o in ("consist_counts",) + SC.TRAJ:
        assert getattr(new, o) is None, o
    for o in SC.INTERMEDIATE + ("field",):
        x, y = getattr(new, o), getattr(old, o)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y, equal_nan=x.dtype.kind == "f")), o
    for name, (order, _) in SC.WRONG.items():                        # the old wrong chains have no new step to be changed by
        assert not {"consist", "traj", "traj_prestate"} & set(order), name


REACH_FB = dict(REACH, consistency=("consist_counts",) + REACH["photometric"][1:] + SC.TRAJ, trajectories=SC.TRAJ,
                repair=REACH["repair"] + SC.TRAJ)


@pytest.mark.parametrize("stage", SC.LEAVE_OUT_FB)
def test_a_stage_switched_off_leaves_the_fb_chain_before_it_untouched(inp_fb, ref_fb, stage):
    spec = SC.without(SPEC_FB, stage)
    got = run_fb(inp_fb, spec)
    SC.same_record(got, ref_fb, [o for o in SC.OUTPUTS if o not in REACH_FB[stage]])
    if stage == "consistency":
        assert got.consist_counts is None and spec["trajectories"]["use_state"] is False and got.traj_pos is not None
        with pytest.raises(AssertionError):                          # use_state with no check: the stream refuses it too
            run_fb(inp_fb, dict(spec, trajectories=SPEC_FB["trajectories"]))
    if stage == "trajectories":
        assert all(getattr(got, o) is None for o in SC.TRAJ)
    if stage in ("camera", "model", "histogram", "links", "blobs"):  # behind the trajectories in the chain
        SC.same_record(got, ref_fb, SC.TRAJ + ("consist_counts", "repair_counts"))


def test_part_slices_the_counts_and_leaves_the_trajectories_out(inp_fb, ref_fb):
    for a, b in ((0, 4), (4, 9), (2, 7)):
        sub, cut = run_fb(inp_fb, a=a, b=b), SC.part(ref_fb, a, b)
        SC.same_record(cut, sub, [o for o in SC.OUTPUTS if o not in ("hist",) + SC.TRAJ])
        assert np.array_equal(cut.consist_counts, ref_fb.consist_counts[a:b])
        assert all(getattr(cut, o) is None for o in SC.TRAJ)
        if a:                                                        # reseeded at pair a: not a slice of the whole clip's table
            assert np.array_equal(sub.traj_pos[0], SEEDS) and not np.array_equal(sub.traj_pos, ref_fb.traj_pos[a:b + 1])
        else:                                                        # from the first pair on it is the whole clip's, cut short
            assert np.array_equal(sub.traj_pos, ref_fb.traj_pos[:b + 1])
            assert np.array_equal(sub.traj_len, np.minimum(ref_fb.traj_len, b))


def test_compose_writes_no_fb_input(inp_fb):
    fwd, back = inp_fb.fwd.copy(), inp_fb.back.copy()
    for name in SC.WRONG_FB:
        SC.compose_wrong_fb(name, inp_fb.frames, inp_fb.fwd, inp_fb.back, SPEC_FB, ops=HostOps, rows=ROWS, cols=COLS)
    assert np.array_equal(inp_fb.fwd.view(np.uint32), fwd.view(np.uint32)) and np.array_equal(inp_fb.back.view(np.uint32), back.view(np.uint32))
