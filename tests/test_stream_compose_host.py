"""stream_compose_cases.compose on the CPU: the composed reference is code that can be wrong too, so on a synthetic input it
must behave as test_gpu_stream_compose.py assumes.  No flow engine and no device: the steps without a bit-exact CPU model are
replaced by the numpy models of the stages' own case files (HostOps), the camera by camera_motion_cases.fit and predict."""
import types

import numpy as np
import pytest

from tests import blob_cases as BC
from tests import blob_link_cases as LC
from tests import camera_motion_cases as CM
from tests import grid_assign_cases as GA
from tests import motion_grid_cases as MC
from tests import photometric_cases as PC
from tests import stream_compose_cases as SC
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
