"""k_pyramid_dec: the level images of the coarse pyramid levels 1..3 of a batch from one march over the
u8 frames.  It copies k_level_dec's arithmetic statement by statement, so EVERY comparison here is np.array_equal: against the
per-level kernels run by the same hook (stages.pyramid_dec(fused=False), which reaches levels below the pyramid's 32-pixel
minimum), against stages.level_image where the pyramid has the level, and, at the engine, flow fields with the one launch
against flow fields with OFC_PYRAMID_FUSED=0.

Sizes (W x H), chosen where the march can go wrong: a work-group owns a band of 256 input columns and a strip of 8-row steps
(at least four steps a strip: these small batches are cut into the shortest strips the plan allows).
  256 x 256    one band; levels 128, 64, 32; eight strips of four steps: every level's window crosses a seam
  264 x 72     a second band 8 columns wide; level 3 is 33 x 9; nine steps in strips of 4, 4, 1
  512 x 40     the height just above 2R + S = 26 of level 3: every row is reflected by some level; five steps
  1024 x 136   four bands; seventeen steps in strips of 4, 4, 4, 4, 1
  260 x 68     a height that is no multiple of the 8-row step (levels 1 and 2 only: 65 x 17 is level 2, level 3 is no exact
               decimation)
Frames: seeded random bytes, all 255, a checkerboard of period 1, single 255s in the corners and at the band seam."""
import contextlib
import os

import numpy as np
import pytest

import flow_sequence_cases as S
from opticalflowclustering_amd import stages, synth

pytestmark = pytest.mark.gpu

SIZES = ((256, 256, 3), (264, 72, 3), (512, 40, 3), (1024, 136, 3), (260, 68, 2))
ENGINE_ENV = ("OFC_FLOW_FRONT_OVERLAP", "OFC_FLOW_GRAPH", "OFC_FLOW_STAGED", "OFC_PYRAMID_FUSED")


def _patterns(W, H):
    rng = np.random.default_rng(W * 10007 + H)
    yy, xx = np.mgrid[0:H, 0:W]
    dots = np.zeros((H, W), np.uint8)
    for y in (0, H - 1):
        for x in (0, W - 1, 255, 256):
            if x < W:
                dots[y, x] = 255
    dots[H // 2, min(255, W - 1)] = 255
    if W > 256:
        dots[H // 2 + 1, 256] = 255
    f = np.stack([rng.integers(0, 256, (H, W), dtype=np.uint8), np.full((H, W), 255, np.uint8),
                  (((xx + yy) & 1) * 255).astype(np.uint8), dots])
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def cases():
    """per size: the frames and the per-level kernels' images of every level, computed once, shared, read-only"""
    out = {}
    for W, H, L in SIZES:
        frames = _patterns(W, H)
        ref, nf = stages.pyramid_dec(frames, L, fused=False)
        assert nf == 0
        for r in ref:
            r.setflags(write=False)
        out[(W, H)] = (frames, ref)
    return out


@pytest.mark.parametrize("W,H,L", SIZES)
def test_all_levels_equal_the_per_level_kernels(cases, W, H, L):
    frames, ref = cases[(W, H)]
    got, nf = stages.pyramid_dec(frames, L)
    assert nf == L
    for k in range(L):
        assert got[k].shape == (len(frames), round(H / 2 ** (k + 1)), round(W / 2 ** (k + 1)))
        assert np.array_equal(got[k], ref[k]), f"level {k + 1} of {W}x{H}"
    assert not np.array_equal(ref[0][0], ref[0][2])


@pytest.mark.parametrize("L", (1, 2))
def test_fewer_levels(cases, L):
    """the one- and two-level instantiations, and a single frame (the launch then has as many strips as the plan allows)"""
    for W, H in ((256, 256), (264, 72)):
        frames, ref = cases[(W, H)]
        got, nf = stages.pyramid_dec(frames[:1], L)
        assert nf == L
        for k in range(L):
            assert np.array_equal(got[k][0], ref[k][0]), f"level {k + 1} of {W}x{H}"


def test_against_level_image_where_the_pyramid_has_the_level(cases):
    for (W, H), levels in (((256, 256), 3), ((1024, 136), 2)):
        frames, _ = cases[(W, H)]
        got, _ = stages.pyramid_dec(frames, levels)
        for k in range(1, levels + 1):
            for i in (0, 3):
                assert np.array_equal(got[k - 1][i], stages.level_image(frames[i], k)), f"level {k}, frame {i} of {W}x{H}"


@pytest.mark.parametrize("W,H,fused", ((512, 24, 2), (260, 64, 2), (162, 98, 0), (520, 64, 3)))
def test_a_level_outside_the_preconditions_keeps_its_kernel(W, H, fused):
    """512 x 24: H0 <= 2R + S of level 3; 260 x 64: level 3 (32 x 8) is no exact 8:1 decimation; 162 x 98: rows not
    dword-addressable, nothing fused; 520 x 64 (three bands, the last 8 columns wide) takes all three"""
    frames = _patterns(W, H)[[0, 3]]
    ref, _ = stages.pyramid_dec(frames, 3, fused=False)
    got, nf = stages.pyramid_dec(frames, 3)
    assert nf == fused
    for k in range(3):
        assert np.array_equal(got[k], ref[k]), f"level {k + 1} of {W}x{H}"


# ---- the engine -------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(**kw):
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


def _engine(W, H, max_batch, **env):
    from opticalflowclustering_amd.flow import FlowEngine
    with _env(**env):
        return FlowEngine(W, H, None, max_batch=max_batch)


def _clip(W, H, n):
    p = synth.texture_params(S.TEXTURE_SEED)
    x = y = 0.0
    out = []
    for t in range(n):
        out.append(synth.frame(W, H, x, y, p))
        dx, dy = S.step(t)
        x, y = x + dx, y + dy
    return np.stack(out)


def _flows(eng, frames, windows):
    """the flow fields of the windows (first frame, pairs), one call each on one handle, no synchronisation between them"""
    from opticalflowclustering_amd import _lib as L
    Hh, Ww = frames.shape[1:]
    P = Ww * Hh
    n_out = sum(n for _, n in windows)
    fd, out = L.DeviceBuffer(frames.nbytes).upload(frames), L.DeviceBuffer(n_out * P * 8)
    off = 0
    for f0, n in windows:
        eng.calc_frames_dev(fd.ptr + f0 * P, n + 1, out.ptr + off * P * 8, sync=False)
        off += n
    eng.sync()
    got = out.download((n_out, Hh, Ww, 2), np.uint32)
    fd.free()
    out.free()
    return got


@pytest.mark.parametrize("max_batch,windows", ((1, ((0, 1), (1, 1))), (3, ((0, 3), (1, 3)))))
def test_engine_flow_fields_equal_with_and_without_the_one_launch(max_batch, windows):
    frames = _clip(256, 256, 5)
    on, off = _engine(256, 256, max_batch), _engine(256, 256, max_batch, OFC_PYRAMID_FUSED="0")
    assert on.front_overlap() and off.front_overlap()
    assert on.pyramid_fused() is True and off.pyramid_fused() is False
    a, b = _flows(on, frames, windows), _flows(off, frames, windows)
    on.close()
    off.close()
    assert np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1])


def test_engine_reports_what_it_uses():
    for W, H, env, want in ((256, 256, {}, True), (256, 256, {"OFC_PYRAMID_FUSED": "0"}, False), (162, 98, {}, False),
                            (256, 256, {"OFC_FLOW_FRONT_OVERLAP": "0"}, False), (256, 256, {"OFC_FLOW_GRAPH": "1"}, False)):
        eng = _engine(W, H, 1, **env)
        assert eng.pyramid_fused() is want, (W, H, env)
        eng.close()
