"""CPU side of test_gpu_field_geometry.py.  The motion shapes of tests/field_geometry_cases.py are checked against the
library's own launch geometry (ofc_motion_launch_geometry, which touches no device and reports the functions the kernels
and launchers compute groups and per by), not against a restatement of it: each shape reaches the paths it is in the table
for, and the table reaches every path, so a retuned formula fails here instead of quietly shrinking what the GPU test
covers.  And every motion case is proved well-conditioned at camera_motion_cases' unchanged MARGIN and KAPPA_MAX, which is
what lets the GPU test demand equal integers.  The rest: the sizes of the weight, key and grid-count cases against the
caps they are meant to pass, the all-frames restatement of model_counts against model_counts, and the host-side refusals
of the launchers that put frames in gridDim.y or .z without chunking."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libofc.so is loaded, as in test_camera_motion_host.py)

from tests import camera_motion_cases as CC
from tests import field_geometry_cases as F
from tests import motion_grid_cases as MC


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def geometry():
    from opticalflowclustering_amd import camera
    return camera.motion_launch_geometry


def test_the_export_exists_answers_without_a_device_and_refuses_bad_arguments(geometry):
    L = _L()
    lib = L.load()
    assert "ofc_motion_launch_geometry" in L.EXPORTS
    header = open(L.LIB_PATH.replace("opticalflowclustering_amd/libofc.so", "include/ofc.h")).read()
    assert "int ofc_motion_launch_geometry(" in header
    # a 1080p pair: 1013 shares, 256 groups of 4, the last two empty; the benchmark's 32 pairs: 64 groups of 16
    assert geometry(1920, 1080, 1) == (256, 4, 254, 1)
    assert geometry(1920, 1080, 32) == (64, 16, 64, 5)
    assert geometry(64, 48, 1) == (2, 1, 2, 1) == geometry(64, 48, 3)            # what the stream tests ran so far
    assert geometry(1, 1, 1) == (1, 1, 1, 1)
    out = (C.c_int * 4)(-7, -7, -7, -7)
    for W, H, n in ((0, 16, 1), (16, 0, 1), (16, 16, 0), (-1, 16, 1)):
        assert lib.ofc_motion_launch_geometry(W, H, n, out) == L.OFC_EINVAL, (W, H, n)
    assert lib.ofc_motion_launch_geometry(16, 16, 1, None) == L.OFC_EINVAL
    assert lib.ofc_motion_launch_geometry(8192, 8192, 1, out) == L.OFC_EUNSUPPORTED         # as ofc_motion_check
    assert lib.ofc_motion_launch_geometry(16, 16, 65536, out) == L.OFC_EUNSUPPORTED
    assert list(out) == [-7] * 4                                                             # a refusal writes nothing
    assert lib.ofc_motion_launch_geometry(16, 16, 65535, out) == L.OFC_OK and list(out) == [1, 1, 1, 1]


def test_the_geometry_covers_every_share_exactly_once(geometry):
    rng = np.random.default_rng(1)
    sizes = [(int(w), int(h), int(n)) for w, h, n in zip(rng.integers(1, 2000, 300), rng.integers(1, 2000, 300),
                                                         2 ** rng.integers(0, 12, 300) + rng.integers(0, 3, 300))]
    for W, H, n in sizes + [(1920, 1080, n) for n in range(1, 140)] + [(3840, 2160, 1), (4096, 4096, 1)]:
        groups, per, used, last = geometry(W, H, n)
        nshare = F.cdiv(W * H, F.MOTION_SHARE)
        assert 1 <= groups <= min(nshare, 256) and per == F.cdiv(nshare, groups), (W, H, n)
        assert 1 <= used <= groups and 1 <= last <= per and (used - 1) * per + last == nshare, (W, H, n)
        assert groups * n <= 2048 or groups == 16 or groups == nshare, (W, H, n)


def test_each_motion_shape_reaches_its_paths_and_the_table_reaches_them_all(geometry):
    reached = set()
    for s in F.MOTION_SHAPES:
        got = geometry(s.W, s.H, s.npair)
        assert (F.cdiv(s.W * s.H, F.MOTION_SHARE),) + got == s.geometry, (s, got)      # the table is the formula's answer
        paths = F.paths_of(s.W, s.H, s.npair, got)
        assert set(s.reaches) <= paths, (s, paths)
        reached |= paths
        assert _L().load().ofc_motion_check(s.W, s.H, 2) == _L().OFC_OK
    assert reached == set(F.PATHS), set(F.PATHS) - reached
    assert len({s.name for s in F.MOTION_SHAPES}) == len(F.MOTION_SHAPES)
    # both instantiations of the moment kernel loop over several shares, and one of them with a short last group
    multi = [(s, k) for s, k in F.MOTION_CASES if "several shares per group" in s.reaches]
    assert {k for _, k in multi} == {"affine", "translation"}
    # no existing case reaches any of them: there groups == nshare <= 23
    for c in CC.CASES:
        assert not F.paths_of(c.W, c.H, c.npair, geometry(c.W, c.H, c.npair)), c
    # the batch that is also fitted pair by pair: the two calls take different groups and per
    one = F.MOTION_BY_NAME[F.ONE_BY_ONE]
    assert geometry(one.W, one.H, one.npair)[:2] != geometry(one.W, one.H, 1)[:2]


def test_the_stream_flush_gets_another_geometry_than_the_full_batch(geometry):
    full, flush = (geometry(F.STREAM_W, F.STREAM_H, n)[:2] for n in (F.STREAM_BATCH, F.STREAM_FLUSH))
    assert F.STREAM_FLUSH == 3 and F.STREAM_PUSHES - 1 == F.STREAM_BATCH + F.STREAM_FLUSH
    assert full == F.STREAM_GEOMETRY[F.STREAM_BATCH] == (85, 2) and flush == F.STREAM_GEOMETRY[F.STREAM_FLUSH] == (101, 1)
    assert full[0] != flush[0] and full[1] != flush[1]
    # the full batch needs the most room for partials, the flush the most groups per pair: the stream sizes by the maximum
    assert full[0] * F.STREAM_BATCH > flush[0] * F.STREAM_FLUSH and flush[0] > full[0]


@pytest.mark.parametrize("case", F.MOTION_CASES, ids=F.motion_case_id)
def test_every_motion_case_is_well_conditioned(case):
    """as test_camera_motion_host.py proves for its cases: no valid pixel's residual lies within 2^-20 px of a threshold in
    any round, so the reference's plain f64 and the device's fma chains select the same pixels; and no moment comes near
    the end of int64"""
    shape, kind = case
    fields, fits, layout = F.motion_reference(shape, kind)
    assert fields.shape == ((1 if shape.npair == 1 else 6), shape.H, shape.W, 2) and fields.dtype == np.float32
    assert len(layout) == shape.npair and set(layout) == set(range(len(fields)))
    least, worst = np.inf, 0.0
    for ref in fits:
        assert ref["margin"] >= CC.MARGIN, (case, ref["margin"])
        assert all(k <= CC.KAPPA_MAX for k in ref["kappa"]), (case, ref["kappa"])
        assert all(abs(v) < 2 ** 62 for m in ref["full"] for v in m), case
        least, worst = min(least, ref["margin"]), max([worst] + ref["kappa"])
    print("%s: least margin %.3e px, largest kappa_inf %.3g" % (F.motion_case_id(case), least, worst))
    if shape.npair > 1:
        assert [ref["status"] for ref in fits] == [0, 0, 0, 0, 0, 2]
        # the four backgrounds and the specials differ in every round's moments and in their models: a misplaced pair shows
        for t in range(len(F.THRESHOLDS) + 1):
            assert len({tuple(ref["full"][t]) for ref in fits[:5]}) == 5
        assert len({ref["models"][-1].tobytes() for ref in fits[:5]}) == 5
        assert fits[4]["full"][0][12] == F.SPECIALS_OUTSIDE and not any(ref["full"][0][12] for ref in fits[:4])
        assert fits[5]["full"][0][12] == shape.W * shape.H and len(fits[5]["full"]) == 1 and not fits[5]["models"].any()
        assert (layout[5], layout[shape.npair - 2]) == (4, 5) and (layout == 4).sum() == 1 == (layout == 5).sum()
    else:
        assert fits[0]["status"] == 0
    # an affine fit ends on the background (the block is 10-15 % of the frame); a translation cannot follow an affine
    # background to within 1 px across a whole frame and ends on a band of it
    kept = fits[0]["moments"][-1][0] / (shape.W * shape.H)
    assert fits[0]["moments"][0][0] == shape.W * shape.H and (0.8 < kept < 1 if kind == "affine" else 0 < kept < 0.8), kept


def test_the_weight_and_key_sizes_pass_their_grid_caps():
    assert F.WEIGHTS_N == 4 * 256 * 4096 + 1027 and F.WEIGHTS_N % 4 == 3
    assert F.WEIGHTS_PASS < F.WEIGHTS_N - 3 < 2 * F.WEIGHTS_PASS                    # a partial second pass before the tail
    assert F.KEYS_N == 4 * 256 * 8192 + 4 * 256 * 3 + 2 == F.KEYS_W * F.KEYS_H * F.KEYS_PAIRS
    assert F.KEYS_PASS_VEC < F.KEYS_N < 2 * F.KEYS_PASS_VEC and F.KEYS_N % 4 == 2
    assert 4 * F.KEYS_PASS_ONE < F.KEYS_N < 5 * F.KEYS_PASS_ONE                     # without VEC: four passes and a bit
    f = F.big_field(5000, 3, (2000,))
    assert f.shape == (5000, 2) and f.dtype == np.float32
    s = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]
    t2 = np.float32(F.THR) * np.float32(F.THR)
    for lo in (0, 1992, 2000, 4992):                                                 # first, either side of a boundary, last
        blk, sq = f[lo:lo + 8], s[lo:lo + 8]
        assert np.isnan(blk[0, 0]) and np.isinf(blk[1, 1]) and not blk[2].any() and np.isnan(blk[7, 1])
        assert sq[4] == t2 and sq[5] < t2 < sq[6]
    assert np.isfinite(f[8:1992]).all() and 0.2 < (s[8:1992] >= t2).mean() < 0.8    # both sides of the threshold occur


def test_the_all_frames_counts_are_model_counts():
    rows, cols = F.GRID_ROWS, F.GRID_COLS
    fl = F.grid_flow()
    assert F.GRID_FRAMES == 65537 > F.GRID_CHUNK and fl.shape == (F.GRID_FRAMES, 3, 4, 2)
    some = np.r_[0:3, F.GRID_CHUNK - 3:F.GRID_FRAMES]
    for k in F.GRID_KS:
        lab = F.grid_labels(k)
        counts, sums = F.counts_all_frames(lab, k, rows, cols, fl)
        assert counts.shape == (F.GRID_FRAMES, 4, k) and counts.dtype == np.int32 and sums.shape == (F.GRID_FRAMES, 4, k, 2)
        want_c, want_s = MC.model_counts(lab[some], k, rows, cols, fl[some])
        assert np.array_equal(counts[some], want_c) and np.array_equal(sums[some].view(np.int64), want_s.view(np.int64))
        assert np.array_equal(F.counts_all_frames(lab, k, rows, cols), counts)
        assert np.array_equal(F.counts_all_frames(lab[some], k, rows, cols, fl[some], absolute=True)[1],
                              MC.model_abs_sums(lab[some], k, rows, cols, fl[some]))
        assert (counts.sum(axis=(1, 2)) == 8).all()                                  # 2 x 2 cells of 2 x 1 px; row 2 in no cell
        # the frames either side of the chunk differ from their neighbours and from frame 0, in counts and in sums
        edge = [0, F.GRID_CHUNK - 2, F.GRID_CHUNK - 1, F.GRID_CHUNK, F.GRID_CHUNK + 1]
        assert edge[1:] == [65533, 65534, 65535, 65536]
        for a in edge:
            for b in edge:
                if a != b:
                    assert not np.array_equal(counts[a], counts[b]) and not np.array_equal(sums[a], sums[b]), (k, a, b)


def test_frame_counts_past_a_grid_dimension_are_refused_on_the_host():
    """k_mag_stats / k_flow_colorize and k_synth_frames put a frame in gridDim.y / .z and do not chunk: their entry points
    refuse more than 65535 before any launch, before a device is even looked for.  k_grid_cell_means and
    k_grid_cell_mean_flow are only ever launched over one frame (ofc_grid_cell_means, ofc_grid_cell_mean_flow) or over a
    stream's batch, which the engine keeps to 4096 pairs"""
    L = _L()
    lib = L.load()
    fake = C.c_void_p(4096)                                                          # never dereferenced: every call is refused
    assert lib.ofc_flow_to_bgr_dev(0, fake, 4, 3, 65536, fake, None) == L.OFC_EUNSUPPORTED
    assert "65535" in lib.ofc_last_error().decode()
    assert lib.ofc_synth_frames_dev(0, fake, 4, 3, 65536, 0, 0) == L.OFC_EUNSUPPORTED
    assert "65535" in lib.ofc_last_error().decode()
    assert lib.ofc_synth_frames_dev(0, fake, 4, 65536, 1, 0, 0) == L.OFC_EUNSUPPORTED
    assert lib.ofc_flow_to_bgr_dev(0, fake, 4, 3, 0, fake, None) == L.OFC_EINVAL
    h = C.c_void_p()
    for batch in (4097, 65536):
        assert lib.ofc_flow_create(0, 64, 48, None, batch, C.byref(h)) == L.OFC_EINVAL and not h.value
        assert "max_batch" in lib.ofc_last_error().decode()
