"""The frame stream with every stage on (csrc/stream_api.cpp): the clip, the specs and the composed reference that
test_gpu_stream_compose.py holds FlowStream to, and that test_stream_compose_host.py proves on the CPU.

compose() takes a clip and its pairwise fields and applies the stages one at a time on host arrays, in the order the stream's
header comment and FlowStream's docstrings promise.  Every step is the single-stage route that the stage's own test file
already holds to a model: the CPU model where one is bit-exact (photometric check, repair, moves, key mask), the library's
single-stage hook where none is (camera solve, cell means, centred distance, components, link votes).  `order` builds the
wrong chains of WRONG: what a stream would deliver if a stage read or wrote the field at another point of the chain.

Observed on the MI355X, on the reference over the engine's pairwise fields of clip(), pairs 0 .. 8 (check_preconditions holds):
    flagged pixels (states other than OK)   2416 2372 2251 2157 3888 2107 2175 2008 2099   (pair 4 crosses the brightness step)
    filled by the repair                    2389 2334 2241 2146 2429 2100 2166 2006 2090
    left unfilled                             27   38   10   11 1459    7    9    2    9
    blobs                                      3    3    3    3    3    3    4    3    3
    links per transition                         5    4    4    4    5    6    6    4
    camera tx -1.94 .. -1.98, ty -0.99 .. -1.03 (the pan is (2, 1)); the repair changes 4802 move words and all 54 camera
    parameters of the clip; 13317 pixels are background under the check's states and foreground under the repaired ones.

With the forward-backward check (`consistency`, which needs `back`, the fields of the pairs taken backwards) in the photometric
one's place and the trajectories behind the repair, the chain is ALL_FB, its wrong chains WRONG_FB; both steps are the integer
CPU models of consistency_cases and trajectory_cases.  test_gpu_stream_compose_bidir.py holds FlowStream to it.

Observed on the MI355X, on the reference of ALL_FB over the engine's pairwise fields of both directions, observed_fb()
(check_preconditions_fb holds):
    flagged pixels (states other than OK)    750  813  799  799  704  812 1265  949  786
    filled by the repair                     717  810  757  774  704  776 1032  850  783
    left unfilled                             33    3   42   25    0   36  233   99    3
    blobs                                      3    3    3    3    3    3    4    3    3
    links per transition                         4    4    4    4    5    6    6    4
    of the 649 points of SEEDS 512 run the whole clip, 34 end UNTRUSTED, 103 LEAVE and none meets an unusable vector; without
    the repair 267 points end elsewhere; followed by the states as the check left them 288 points end for another reason."""
import types

import numpy as np

from tests import blob_link_cases as LC
from tests import consistency_cases as CC
from tests import photometric_cases as PC
from tests import repair_cases as RC
from tests import trajectory_cases as TC

W, H, N_FRAMES = LC.CLIP_W, LC.CLIP_H, 10
ROWS, COLS = 2, 3
STRICT = dict(tau=2.0, kappa=0.25)                                   # test_gpu_repair.py's thresholds
REPAIR = dict(radius=1, rounds=3, min_count=2)
# behind the camera the pan is gone: the background rests and the rectangles move by their own speed per frame
CENTRES = np.array([[0.1, 0.05], [2.9, 0.1], [0.1, -2.8]])
BLOBS = dict(thr=LC.CLIP_THR, connectivity=8, min_area=12, max_blobs=256, max_links=128)
HISTOGRAM = (256, 8.0)
CAMERA = "affine"

# FlowStream's keyword arguments: a spec is what the stream is made with
ALL = dict(centers=CENTRES, sums=True, histogram=HISTOGRAM, camera=CAMERA, blobs=BLOBS, photometric=STRICT, repair=REPAIR)
# configuration B of the reconfiguration test: every table and scratch buffer smaller or of another layout
SMALL = dict(centers=CENTRES[:2], sums=False, histogram=(64, 4.0), camera="translation",
             blobs=dict(BLOBS, max_blobs=64, max_links=16), photometric=dict(STRICT, keep=(0, 1)),
             repair=dict(radius=1, rounds=1, min_count=2, smooth=False))
NONE = dict(centers=None, sums=False, histogram=None, camera=None, blobs=None, photometric=None, repair=None)


def grid_seeds(w, h, step):
    """trajectories.grid_seeds(w, h, step) for a whole step: the centres of the step x step cells, row by row, 1/65536 px"""
    xs = np.arange(step * 32768, (w - 1) * 65536 + 1, step * 65536, dtype=np.int64)
    ys = np.arange(step * 32768, (h - 1) * 65536 + 1, step * 65536, dtype=np.int64)
    out = np.empty((len(ys), len(xs), 2), np.int32)
    out[..., 0], out[..., 1] = xs[None, :], ys[:, None]
    return out.reshape(-1, 2)


FRACTIONS = (1, 32768, 65535)                                        # one quantum past a pixel, half way, one quantum short of the next
# the centre of every 4x4 cell, then every pairing of FRACTIONS in x and y on nine pixels spread over the frame
SEEDS = np.concatenate([grid_seeds(W, H, 4),
                        np.array([[((24 + 36 * i) << 16) + fx, ((18 + 20 * j) << 16) + fy]
                                  for j, fy in enumerate(FRACTIONS) for i, fx in enumerate(FRACTIONS)], np.int32)])
SEEDS.setflags(write=False)
CHECK_FB = dict(alpha=0.01, beta=0.5, keep=(0,))                     # test_gpu_flow_bidir.py's values on this clip
# the forward-backward check in the photometric one's place, and the trajectories by its states
ALL_FB = dict(ALL, photometric=None, consistency=CHECK_FB, trajectories=dict(seeds=SEEDS, use_state=True))
# the photometric check with everything on
ALL_TRAJ = dict(ALL, trajectories=dict(seeds=SEEDS, use_state=True))


def without(spec, stage):
    """the spec with one stage off: 'photometric', 'consistency', 'trajectories', 'repair', 'camera', 'model', 'histogram',
    'links' or 'blobs'.  Without its check a spec's trajectories have no state map to go by: use_state goes off with it."""
    s = dict(spec)
    if stage == "model":
        s.update(centers=None, sums=False)
    elif stage == "links":
        s["blobs"] = dict(spec["blobs"], max_links=0)
    else:
        assert stage in ("photometric", "consistency", "trajectories", "repair", "camera", "histogram", "blobs"), stage
        s[stage] = None
        if stage in ("photometric", "consistency") and isinstance(s.get("trajectories"), dict):
            s["trajectories"] = dict(s["trajectories"], use_state=False)
    return s


LEAVE_OUT = ("photometric", "repair", "camera", "model", "histogram", "links", "blobs")
LEAVE_OUT_FB = ("consistency", "trajectories", "repair", "camera", "model", "histogram", "links", "blobs")

# ---- the order.  A step: photo, consist, repair, traj, moves, camera (= camera_fit, camera_sub), cells, counts, hist, blobs,
# links; blobs_prestate and traj_prestate are blobs masked, and points followed, by the states as the check left them, before
# the repair updated them.  A step whose stage the spec does not have does nothing. ----
DOCUMENTED = ("photo", "consist", "repair", "traj", "moves", "camera", "cells", "counts", "hist", "blobs", "links")
# the chain as it was before the forward-backward check and the trajectories joined it: a spec without them gives the same
DOCUMENTED_BEFORE = ("photo", "repair", "moves", "camera", "cells", "counts", "hist", "blobs", "links")
_TAIL = ("cells", "counts", "hist", "blobs", "links")
# name -> (order, the outputs of the record that must differ from the documented chain's)
WRONG = {
    "check-after-repair": (("photo", "repair", "photo", "moves", "camera") + _TAIL, ("photo_stats",)),
    "check-on-the-residual": (("camera", "photo", "repair", "moves") + _TAIL, ("photo_stats",)),
    "moves-before-the-repair": (("photo", "moves", "repair", "camera") + _TAIL, ("moves", "links")),
    "moves-after-the-camera": (("photo", "repair", "camera", "moves") + _TAIL, ("moves", "links")),
    "camera-fitted-on-the-unrepaired-field": (("photo", "camera_fit", "repair", "moves", "camera_sub") + _TAIL, ("cam_params",)),
    "blobs-masked-by-the-pre-repair-states": (("photo", "repair", "moves", "camera", "cells", "counts", "hist", "blobs_prestate", "links"),
                                              ("records",)),
    "blobs-keyed-on-the-unsubtracted-field": (("photo", "repair", "moves", "blobs", "camera", "cells", "counts", "hist", "links"),
                                              ("records",)),
}
# the same for a stream with the forward-backward check and the trajectories (ALL_FB); REVERSED: the documented order over the
# backward fields in the reversed clip's order, the bwd_reversed mix-up of ofc_consist_dev
WRONG_FB = {
    "traj-before-the-repair": (("consist", "traj", "repair", "moves", "camera") + _TAIL, ("traj_pos",)),
    "traj-after-the-camera": (("consist", "repair", "moves", "camera", "traj") + _TAIL, ("traj_pos",)),
    "traj-by-the-pre-repair-states": (("consist", "repair", "traj_prestate", "moves", "camera") + _TAIL, ("traj_len", "traj_why")),
    "fb-check-after-the-repair": (("consist", "repair", "consist", "traj", "moves", "camera") + _TAIL, ("consist_counts",)),
    # the camera is subtracted from the forward field alone, as a stream would do it
    "fb-check-on-the-residual": (("camera", "consist", "repair", "traj", "moves") + _TAIL, ("consist_counts",)),
    "fb-blobs-masked-by-the-pre-repair-states": (("consist", "repair", "traj", "moves", "camera", "cells", "counts", "hist",
                                                  "blobs_prestate", "links"), ("records",)),
    "backward-fields-in-reverse-order": (DOCUMENTED, ("consist_counts",)),
}
REVERSED = ("backward-fields-in-reverse-order",)


def compose_wrong_fb(name, frames, fields, back, spec=None, **kw):
    """the record of the wrong chain WRONG_FB[name] -> (record, the outputs that must differ)"""
    order, outputs = WRONG_FB[name]
    return compose(frames, fields, ALL_FB if spec is None else spec, order, back=back[::-1] if name in REVERSED else back, **kw), outputs


# ---- the clip ----
# x, y, w, h in frame 0 of the image; vx, vy per frame in the image: it crosses the first rectangle
OCCLUDER = (60, 0, 10, 30, -4, 1)
STEP_FRAME, STEP_X, STEP_LEVELS = 5, 96, 12


def clip(n_frames=N_FRAMES):
    """(n, H, W) u8, read-only: blob_link_cases' panning clip of two rectangles with what makes every stage bite: finer
    texture on the world, a third rectangle that passes in front of the first (occlusion: vectors the check flags in
    clumps that three rounds of the repair cannot all close), and a brightness step from frame STEP_FRAME on"""
    frames = LC.rect_clip(LC.CLIP_PAN, n_frames=n_frames, W=W, H=H).astype(np.float64)
    rng = np.random.default_rng(77)
    M = 32
    yy, xx = np.mgrid[0:H + 2 * M, 0:W + 2 * M].astype(np.float64)
    fine = 14 * np.sin(xx * 1.1 + yy * 0.6) * np.cos(xx * 0.5 - yy * 0.9) + rng.integers(-4, 5, xx.shape)
    x, y, w, h, vx, vy = OCCLUDER
    occ = 128 + 100 * np.sin(xx[:h, :w] * 0.6 - yy[:h, :w] * 0.9) * np.cos(xx[:h, :w] * 0.45 + yy[:h, :w] * 0.3)
    out = np.empty((n_frames, H, W), np.uint8)
    for t in range(n_frames):
        ox, oy = M + LC.CLIP_PAN[0] * t, M + LC.CLIP_PAN[1] * t
        img = frames[t] + fine[oy:oy + H, ox:ox + W]
        x0, y0 = x + vx * t, y + vy * t
        xa, xb, ya, yb = max(x0, 0), min(x0 + w, W), max(y0, 0), min(y0 + h, H)
        if xa < xb and ya < yb:
            img[ya:yb, xa:xb] = occ[ya - y0:yb - y0, xa - x0:xb - x0]
        if t >= STEP_FRAME:
            img[:, STEP_X:] += STEP_LEVELS
        out[t] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


# ---- the steps on the device: the single-stage hooks of the library ----
class DeviceOps:
    """every step of compose() that has no bit-exact CPU model, by the library's single-stage route"""

    @staticmethod
    def camera_fit(field, kind):
        from opticalflowclustering_amd import camera
        cm = camera.estimate_camera_motion(field, kind)
        return cm.params, cm.status

    @staticmethod
    def camera_sub(field, params):
        import ctypes as C
        from opticalflowclustering_amd import _lib
        n, h, w = field.shape[:3]
        buf = _lib.DeviceBuffer(field.nbytes).upload(np.ascontiguousarray(field, np.float32))
        try:
            p = np.ascontiguousarray(params, np.float64)
            _lib.check(_lib.load().ofc_motion_subtract_dev(0, C.c_void_p(buf.ptr), w, h, n, _lib.ptr(p), C.c_void_p(buf.ptr)))
            return buf.download(field.shape, np.float32)
        finally:
            buf.free()

    @staticmethod
    def camera(field, kind):
        from opticalflowclustering_amd import camera
        res, cm = camera.compensate(field, kind)
        return res, cm.params, cm.status

    @staticmethod
    def cells(field, rows, cols):
        from opticalflowclustering_amd.stream import grid_cell_mean_flow
        return np.stack([grid_cell_mean_flow(f, rows, cols) for f in field])

    @staticmethod
    def counts(field, centres, rows, cols):
        from opticalflowclustering_amd.vis import grid_assign_counts
        return grid_assign_counts(field, centres, rows, cols, mean=None, sums=True)

    @staticmethod
    def hist(field, bins, rng):
        from opticalflowclustering_amd.uvhist import uv_histogram
        return uv_histogram(field, bins, rng).table

    @staticmethod
    def keys(field, centres, thr):
        from opticalflowclustering_amd import blobs as B
        if centres is None:
            return B.moving_blobs(field, thr, labels=False).keys
        return B.cluster_blobs(field, centres, thr=thr, labels=False).keys

    @staticmethod
    def components(keys, field, connectivity, min_area, max_blobs):
        from opticalflowclustering_amd import blobs as B
        b = B.connected_components(keys, connectivity, min_area, max_blobs, flow=field)
        return b.labels, b.records, b.found

    @staticmethod
    def links(labels, move_field, moves, min_area, max_links):
        from opticalflowclustering_amd import blobs as B
        h, w = labels.shape[1:]
        b = B.link(B.Blobs(w, h, labels, None, None), move_field, min_area, max_links)
        assert np.array_equal(b.moves, moves)                       # blobs.link took the moves that moves_of gives
        return b.links, b.nlinks


def masked(keys, state, keep):
    """the key map with every pixel whose state is not in `keep` made background: ofc_consist_mask_dev's rule"""
    st = state.astype(np.int64)
    kept = (st < 4) & (((keep >> np.minimum(st, 4)) & 1) == 1)
    return np.where(kept, keys, 255).astype(np.uint8)


def keep_mask(states):
    m = 0
    for s in states:
        m |= 1 << int(s)
    return m


def quantise(tau, kappa):
    """photometric.quantise's arithmetic: 1/256 grey levels, 1/256"""
    return int(round(tau * 256)), int(round(kappa * 256))


def quantise_fb(alpha, beta):
    """consistency.quantise's arithmetic: alpha in 1/65536, beta in px^2 in units of 2^-32"""
    return int(round(float(alpha) * 65536)), int(round(float(beta) * 2.0 ** 32))


OUTPUTS = ("cells", "counts", "sums", "hist", "cam_params", "cam_status", "photo_stats", "repair_counts", "records", "found",
           "links", "nlinks", "consist_counts", "traj_pos", "traj_len", "traj_why")
INTERMEDIATE = ("state_pre", "state", "filled", "moves", "move_field", "labels", "keys", "keys_pre", "traj_field")
PER_PAIR = ("cells", "counts", "sums", "cam_params", "cam_status", "photo_stats", "repair_counts", "found", "consist_counts")
TRAJ = ("traj_pos", "traj_len", "traj_why")


def compose(frames, fields, spec, order=DOCUMENTED, ops=DeviceOps, rows=ROWS, cols=COLS, back=None):
    """frames (n+1,H,W) u8, fields (n,H,W,2) f32 (pair by pair, as FlowEngine(max_batch=1) gives them), spec = FlowStream's
    keyword arguments -> a record with OUTPUTS (None where the stage is off) and the intermediate maps a test may ask
    about: state_pre (as the check left it), state (as the repair left it), filled, moves, labels, keys, traj_field (as
    the trajectories saw it), field (as the last stage saw it).  back (n,H,W,2) f32: the field of pair (t+1 -> t) at index
    t, which a spec with the forward-backward check needs.  No input is written."""
    f = np.array(fields, np.float32)                                 # the chain's field: rewritten, never in place
    r = types.SimpleNamespace(**{k: None for k in OUTPUTS + INTERMEDIATE})
    photo, rep, blob = spec.get("photometric"), spec.get("repair"), spec.get("blobs")
    photo = {} if photo is True else photo
    rep = {} if rep is True else rep
    cam, centres, hist = spec.get("camera"), spec.get("centers"), spec.get("histogram")
    cons, traj = spec.get("consistency") or None, spec.get("trajectories") or None
    cons = {} if cons is True else cons
    traj = {} if traj is True else traj
    assert photo is None or cons is None, "one check per stream"
    check = photo if photo is not None else cons                     # the check whose states the later stages go by
    check_keep = keep_mask(check.get("keep", (0,))) if check is not None else 0
    if traj is not None:
        seeds = traj.get("seeds")
        seeds = grid_seeds(f.shape[2], f.shape[1], traj.get("step", 8)) if seeds is None else np.ascontiguousarray(seeds, np.int32)
        assert not traj.get("use_state") or check is not None, "use_state needs the state map of a check"
    for step in order:
        if step == "photo" and photo is not None:
            tau_q, kappa_q = quantise(photo.get("tau", 8.0), photo.get("kappa", 0.5))
            r.state_pre, r.photo_stats, _ = PC.reference(frames, f, tau_q, kappa_q)
            r.state = r.state_pre
        elif step == "consist" and cons is not None:
            alpha, beta = cons.get("alpha"), cons.get("beta")        # None: consistency.ALPHA and BETA
            alpha_q, beta_q = quantise_fb(0.01 if alpha is None else alpha, 0.5 if beta is None else beta)
            r.state_pre, r.consist_counts, _ = CC.reference(f, np.asarray(back, np.float32), alpha_q, beta_q)
            r.state = r.state_pre
        elif step in ("traj", "traj_prestate") and traj is not None:
            st = (r.state_pre if step == "traj_prestate" else r.state) if traj.get("use_state") else None
            assert st is not None or not traj.get("use_state"), "the trajectories go by a state map no step has made yet"
            r.traj_field = f
            r.traj_pos, r.traj_len, r.traj_why = TC.reference(f, seeds, st, check_keep)
        elif step == "repair" and rep is not None:
            f, r.filled, r.repair_counts, st = RC.model(f, r.state, keep_mask(rep.get("keep", (0,))), rep.get("radius", 1),
                                                        rep.get("rounds", 8), rep.get("min_count", 1), rep.get("smooth", False))
            r.state = st if st is not None else r.state
        elif step == "moves" and blob is not None and blob.get("max_links"):
            r.move_field, r.moves = f, LC.moves_of(f)
        elif step == "camera" and cam is not None:
            f, r.cam_params, r.cam_status = ops.camera(f, cam)
        elif step == "camera_fit" and cam is not None:
            r.cam_params, r.cam_status = ops.camera_fit(f, cam)
        elif step == "camera_sub" and cam is not None:
            f = ops.camera_sub(f, r.cam_params)
        elif step == "cells":
            r.cells = ops.cells(f, rows, cols)
        elif step == "counts" and centres is not None:
            r.counts, r.sums = ops.counts(f, centres, rows, cols)
            if not spec.get("sums"):
                r.sums = None
        elif step == "hist" and hist is not None:
            r.hist = np.asarray(ops.hist(f, *hist), np.int64)
        elif step in ("blobs", "blobs_prestate") and blob is not None:
            keys = np.array(ops.keys(f, centres, blob["thr"]), np.uint8)
            if check is not None:                                    # a pixel whose state is not kept belongs to no blob
                r.keys_pre = masked(keys, r.state_pre, check_keep)
                keys = r.keys_pre if step == "blobs_prestate" else masked(keys, r.state, check_keep)
            r.keys = keys
            r.labels, r.records, r.found = ops.components(keys, f, blob.get("connectivity", 8), blob.get("min_area", 1),
                                                          blob.get("max_blobs", 4096))
        elif step == "links" and blob is not None and blob.get("max_links"):
            r.links, r.nlinks = ops.links(r.labels, r.move_field, r.moves, blob.get("min_area", 1), blob["max_links"])
    r.field = f
    return r


def differs(a, b, name):
    """whether output `name` of two records differs in any bit"""
    x, y = getattr(a, name), getattr(b, name)
    if name in ("records", "links"):
        return len(x) != len(y) or any(p.shape != q.shape or not np.array_equal(p, q) for p, q in zip(x, y))
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape != y.shape or x.tobytes() != y.tobytes()


def same_record(got, want, names=OUTPUTS):
    """bit for bit: floats through their words, integers by array_equal, tables row by row"""
    for name in names:
        g, w = getattr(got, name), getattr(want, name)
        assert (g is None) == (w is None), name
        if w is None:
            continue
        if name in ("records", "links"):
            assert len(g) == len(w), name
            for t, (p, q) in enumerate(zip(g, w)):
                assert p.dtype == np.int64 and p.shape == q.shape and np.array_equal(p, q), (name, t)
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype.kind == "f":
            word = np.uint32 if g.dtype.itemsize == 4 else np.int64
            assert np.array_equal(g.view(word), w.view(word)), name
        else:
            assert np.array_equal(g, w), name


def part(rec, a, b):
    """pairs a .. b-1 of a record: the per-pair outputs sliced, the transitions between those pairs; no histogram (a clip's
    table is a sum, not a slice) and no trajectories (a clip's points are placed at its own first pair)"""
    out = types.SimpleNamespace(**{k: None for k in OUTPUTS})
    for name in PER_PAIR:
        v = getattr(rec, name)
        setattr(out, name, None if v is None else v[a:b])
    if rec.records is not None:
        out.records = rec.records[a:b]
    if rec.links is not None:
        out.links, out.nlinks = rec.links[a:b - 1], rec.nlinks[a:b - 1]
    return out


def observed(ref, plain):
    """the figures the module docstring records, from the documented reference and the one without the repair"""
    return dict(flagged=(ref.photo_stats[:, 1:4].sum(1)).tolist(), filled=ref.repair_counts[:, 1].tolist(),
                unfilled=ref.repair_counts[:, 2].tolist(), blobs=[len(x) for x in ref.records], links=ref.nlinks.tolist(),
                tx=np.round(ref.cam_params[:, 0], 3).tolist(), ty=np.round(ref.cam_params[:, 3], 3).tolist(),
                moves_changed=int((ref.moves != plain.moves).sum()),
                camera_bits_changed=int((ref.cam_params.view(np.int64) != plain.cam_params.view(np.int64)).sum()),
                back_in=int(((ref.keys_pre == 255) & (ref.keys != 255)).sum()))


def check_preconditions(ref, plain):
    """what the clip must do for the GPU tests to mean anything, asserted on the reference (`plain`: the same without the
    repair): every stage has work, and the repair changes what the stages behind it see"""
    n = len(ref.photo_stats)
    assert (ref.photo_stats[:, 1:4].sum(1) > 0).all(), "every pair has flagged pixels"
    assert (ref.repair_counts[:, 1] > 0).all() and ref.repair_counts[:, 2].sum() > 0, "filled in every pair, some unfilled"
    assert (np.abs(ref.cam_params[:, 0]) > 0.2).all() and (np.abs(ref.cam_params[:, 3]) > 0.2).all(), "a camera that moves"
    assert (ref.cam_status == 0).all()
    assert len(np.unique(ref.counts.argmax(-1))) >= 2, "the cells' arg-max label takes two values"
    assert min(len(x) for x in ref.records) >= 2 and (ref.found <= 256).all(), "two blobs per pair"
    assert len(ref.nlinks) == n - 1 and ref.nlinks.min() >= 2, "two links per transition"
    assert (ref.moves != plain.moves).any(), "the repair changes a move word"
    assert (ref.cam_params.view(np.int64) != plain.cam_params.view(np.int64)).any(), "the repair changes a camera parameter bit"
    assert ((ref.keys_pre == 255) & (ref.keys != 255)).any(), "a pixel is background under the pre-repair states and foreground after"


def _ends_elsewhere(a, b):
    """the points that two records leave at different positions when the clip ends: (P,) bool"""
    return (a.traj_pos[-1] != b.traj_pos[-1]).any(-1)


def prestate_trajectories(ref):
    """ALL_FB's points followed through the field the reference's own were, by the states as the check left them -> (len, why)"""
    _, length, why = TC.reference(ref.traj_field, SEEDS, ref.state_pre, keep_mask(CHECK_FB["keep"]))
    return length, why


def observed_fb(ref, plain):
    """the figures the module docstring records for ALL_FB, from the documented reference and the one without the repair"""
    n = len(ref.consist_counts)
    moved = _ends_elsewhere(ref, plain)
    _, why_pre = prestate_trajectories(ref)
    return dict(flagged=ref.consist_counts[:, 1:].sum(1).tolist(), filled=ref.repair_counts[:, 1].tolist(),
                unfilled=ref.repair_counts[:, 2].tolist(), points=len(ref.traj_len),
                why=np.bincount(ref.traj_why, minlength=4).tolist(), whole_clip=int(((ref.traj_why == TC.RAN) & (ref.traj_len == n)).sum()),
                ends_elsewhere_without_the_repair=int(moved.sum()), why_differs_by_the_pre_repair_states=int((why_pre != ref.traj_why).sum()),
                blobs=[len(x) for x in ref.records], links=ref.nlinks.tolist())


def check_preconditions_fb(ref, plain):
    """check_preconditions for ALL_FB: the forward-backward check and the repair have work in every pair, the points end
    for every reason the chain can give them, and both the repaired field and the repaired states change a trajectory"""
    n = len(ref.consist_counts)
    assert (ref.consist_counts[:, 1:].sum(1) > 0).all(), "every pair has flagged pixels"
    assert (ref.repair_counts[:, 1] > 0).all() and ref.repair_counts[:, 2].sum() > 0, "filled in every pair, some unfilled"
    assert (ref.traj_why == TC.UNTRUSTED).any() and (ref.traj_why == TC.LEAVES).any(), "a point ends UNTRUSTED, another LEAVES"
    assert ((ref.traj_why == TC.RAN) & (ref.traj_len == n)).any(), "a point runs the whole clip"
    assert _ends_elsewhere(ref, plain).any(), "the repair changes a point's final position"
    assert (prestate_trajectories(ref)[1] != ref.traj_why).any(), "a point's why differs between the states before and after the repair"
