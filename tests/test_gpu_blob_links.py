"""Blob links on the device (blob_links.hip): the moves, the link tables, the overflow rule, the refusals, and the way up
through blobs.py, ClipPipeline, FlowStream and the motionGrids command line.

Every output is an integer, so everything is compared with array_equal against the numpy reference of
tests/blob_link_cases.py; test_blob_links_host.py proves that reference against a per-pixel loop, that each case has the
property it is named for, and (on the CPU oracle) that the synthetic clip used here has exactly the two tracks asked for."""
import ctypes as C

import numpy as np
import pytest

from tests import blob_link_cases as LC

pytestmark = pytest.mark.gpu


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def _B():
    from opticalflowclustering_amd import blobs
    return blobs


def _dev(a):
    L = _L()
    a = np.ascontiguousarray(a)
    return L.DeviceBuffer(max(a.nbytes, 8)).upload(a)


def _fill(buf, byte=0x55):
    L = _L()
    L.check(L.load().ofc_memset(0, C.c_void_p(buf.ptr), byte, buf.nbytes))


def same_links(got, want):
    links, nlinks = got
    wl, wn = want
    assert nlinks.dtype == np.int32 and np.array_equal(nlinks, wn), (nlinks, wn)
    assert len(links) == len(wl)
    for a, b in zip(links, wl):
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b)


# ---- moves ----
def moves_dev(flow, shift=0):
    """ofc_blob_moves_dev; shift = 1 puts the field 8 bytes and the moves 4 bytes past their buffers' starts, where the
    kernel cannot take four vectors at a time.  Checks that the field is left alone and nothing is written past the moves."""
    L = _L()
    n, H, W = flow.shape[:3]
    fd = L.DeviceBuffer(flow.nbytes + 16).upload(flow, offset=8 * shift)
    md = L.DeviceBuffer(n * H * W * 4 + 16)
    try:
        _fill(md)
        L.check(L.load().ofc_blob_moves_dev(0, C.c_void_p(fd.ptr + 8 * shift), W, H, n, C.c_void_p(md.ptr + 4 * shift)))
        assert (md.download((16,), np.uint8, offset=n * H * W * 4)[4 * shift:] == 0x55).all()
        assert (md.download((4 * shift,), np.uint8) == 0x55).all()
        assert np.array_equal(fd.download(flow.shape, np.float32, offset=8 * shift).view(np.uint32), flow.view(np.uint32))
        return md.download((n, H, W), np.int32, offset=4 * shift)
    finally:
        fd.free()
        md.free()


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_moves_equal_the_reference_on_aligned_and_odd_bases(case):
    want = LC.case_moves(case)
    for shift in (0, 1):
        got = moves_dev(case.flow, shift)
        assert got.dtype == np.int32 and np.array_equal(got, want), shift


# ---- links ----
def device_labels(case, connectivity):
    """ofc_blob_label_dev's own label maps of the case, left on the device -> (buffer, host copy)"""
    L = _L()
    n, H, W = case.keys.shape
    kd = _dev(case.keys)
    ld = L.DeviceBuffer(max(case.keys.size * 4, 8))
    try:
        L.check(L.load().ofc_blob_label_dev(0, C.c_void_p(kd.ptr), W, H, n, connectivity, C.c_void_p(ld.ptr)))
    finally:
        kd.free()
    return ld, ld.download((n, H, W), np.int32)


def links_dev_raw(ld, md, W, H, n, min_area, max_links, calls=1):
    """ofc_blob_links_dev + ofc_blob_links_read, `calls` times into buffers pre-filled with 0x55 -> [(links, nlinks)]"""
    L = _L()
    lib = L.load()
    nt = n - 1
    size = lib.ofc_blob_links_bytes(max_links, nt)
    assert size == 12 * nt * (1 << int(np.ceil(np.log2(2 * max_links))))
    td, cd = L.DeviceBuffer(max(size, 8)), L.DeviceBuffer(max(4 * nt, 8))
    out = []
    try:
        for _ in range(calls):
            _fill(td)
            _fill(cd)
            table, nlinks = np.full((nt, max_links, LC.LINK_NF), -7, np.int64), np.full(nt, -7, np.int32)
            L.check(lib.ofc_blob_links_dev(0, C.c_void_p(ld.ptr), C.c_void_p(md.ptr), W, H, n, min_area, max_links,
                                           C.c_void_p(td.ptr), C.c_void_p(cd.ptr)))
            L.check(lib.ofc_blob_links_read(0, C.c_void_p(td.ptr), C.c_void_p(cd.ptr), nt, max_links, L.ptr(table), L.ptr(nlinks)))
            for t in range(nt):
                assert not table[t, max(int(nlinks[t]), 0):].any()               # rows past n are zeroed; all of them on overflow
            out.append(([np.ascontiguousarray(table[t, :max(int(m), 0)]) for t, m in enumerate(nlinks)], nlinks))
    finally:
        td.free()
        cd.free()
    return out


def links_of_case(case, connectivity, min_area=1, max_links=LC.MAXL, calls=1):
    n, H, W = case.keys.shape
    ld, lab = device_labels(case, connectivity)
    assert np.array_equal(lab, LC.labels_of(case, connectivity))                 # the device's own label maps are the reference's
    moves = LC.case_moves(case)
    md = _dev(moves)
    try:
        out = links_dev_raw(ld, md, W, H, n, min_area, max_links, calls)
        assert np.array_equal(ld.download(lab.shape, np.int32), lab)             # both inputs are left alone
        assert np.array_equal(md.download(moves.shape, np.int32), moves)
    finally:
        ld.free()
        md.free()
    return out


@pytest.mark.parametrize("connectivity", LC.CONNECTIVITIES)
@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_links_equal_the_reference_and_repeat(case, connectivity):
    first, second = links_of_case(case, connectivity, calls=2)
    same_links(first, LC.reference(case, connectivity))
    same_links(second, first)


@pytest.mark.parametrize("min_area", [4, 5, 6, 7, 9, 10, 17])
def test_min_area_at_a_blob_s_area_and_one_above_on_either_side(min_area):
    case = LC.BY_NAME["min-area-70x33"]
    same_links(links_of_case(case, 8, min_area)[0], LC.reference(case, 8, min_area))


@pytest.mark.parametrize("name,min_area", [("blocks-200x50", 30), ("background-129x40", 3), ("specials-64x16", 26)])
def test_min_area_on_busy_cases(name, min_area):
    case = LC.BY_NAME[name]
    want = LC.reference(case, 4, min_area)
    assert 0 < sum(want[1]) < sum(LC.reference(case, 4)[1])                      # the filter bites, and leaves something
    same_links(links_of_case(case, 4, min_area)[0], want)


def test_max_links_exactly_the_count_delivers_and_one_below_delivers_none():
    case = LC.BY_NAME["many-links-129x40"]
    m = int(LC.reference(case, 4, 1, 10 ** 6)[1][0])
    exact = links_of_case(case, 4, 1, m, calls=2)
    same_links(exact[0], LC.reference(case, 4, 1, m))
    same_links(exact[1], exact[0])
    assert exact[0][1].tolist() == [m, m]
    below = links_of_case(case, 4, 1, m - 1, calls=2)
    same_links(below[0], LC.reference(case, 4, 1, m - 1))
    same_links(below[1], below[0])
    assert below[0][1].tolist() == [-1, -1] and all(len(r) == 0 for r in below[0][0])
    for max_links in (1, 2, 700):                                                # far below: tables that fill up whole
        same_links(links_of_case(case, 4, 1, max_links)[0], LC.reference(case, 4, 1, max_links))
    case = LC.BY_NAME["blocks-200x50"]                                           # one transition over, the other not
    counts = LC.reference(case, 8)[1]
    lo, hi = sorted(counts.tolist())
    assert lo < hi
    got = links_of_case(case, 8, 1, lo)[0]
    same_links(got, LC.reference(case, 8, 1, lo))
    assert sorted(got[1].tolist()) == [-1, lo]


def test_labels_outside_the_map_vote_for_nothing():
    """a caller's label map with words outside [-1, P): they are checked before they index anything"""
    case = LC.BY_NAME["background-129x40"]
    n, H, W = case.keys.shape
    lab = LC.labels_of(case, 8).copy()
    r = np.random.default_rng(6)
    bad = r.random(lab.shape) < 0.02
    lab[bad] = r.choice(np.array([H * W, H * W + 5, 2 ** 31 - 1, -2, -2 ** 31], np.int64), int(bad.sum())).astype(np.int32)
    moves = LC.case_moves(case)
    clean = np.where((lab >= 0) & (lab < H * W), lab, -1).astype(np.int32)
    ld, md = _dev(lab), _dev(moves)
    try:
        got = links_dev_raw(ld, md, W, H, n, 1, LC.MAXL)[0]
    finally:
        ld.free()
        md.free()
    same_links(got, LC.links_of(clean, moves))


# ---- refusals ----
def test_every_refusal_comes_before_any_launch():
    """dimensions beyond the limits with small buffers: a launch would fault, a refusal returns; outputs keep their fill"""
    L = _L()
    lib = L.load()
    a, b, c, d = (L.DeviceBuffer(256) for _ in range(4))
    pa, pb, pc, pd = (C.c_void_p(x.ptr) for x in (a, b, c, d))
    host, small = np.full(64, -7, np.int64), np.full(8, -7, np.int32)
    hp, sp = L.ptr(host), L.ptr(small)
    try:
        for x in (c, d):
            _fill(x)
        big = (65536, 32768)                                                     # 2^31 pixels
        for W, H, n, rc in ((*big, 2, L.OFC_EUNSUPPORTED), (4, 4, 65536, L.OFC_EUNSUPPORTED), (0, 4, 2, L.OFC_EINVAL),
                            (4, 0, 2, L.OFC_EINVAL), (4, 4, 0, L.OFC_EINVAL)):
            assert lib.ofc_blob_moves_dev(0, pa, W, H, n, pc) == rc
            assert lib.ofc_blob_links_dev(0, pa, pb, W, H, n, 1, 4, pc, pd) == rc
            assert lib.ofc_blob_links(0, hp, hp, W, H, n, 1, 4, None, hp, sp) == rc
            assert lib.ofc_bench_blob_links(0, pa, pb, W, H, n, 3, 1, C.byref(C.c_float())) == rc
        for min_area, max_links, rc in ((0, 4, L.OFC_EINVAL), (1, 0, L.OFC_EINVAL), (1, -4, L.OFC_EINVAL), (1, 65537, L.OFC_EUNSUPPORTED)):
            assert lib.ofc_blob_links_dev(0, pa, pb, 2, 2, 2, min_area, max_links, pc, pd) == rc
            assert lib.ofc_blob_links(0, hp, hp, 2, 2, 2, min_area, max_links, None, hp, sp) == rc
        assert lib.ofc_blob_links_read(0, pc, pd, 1, 65537, hp, sp) == L.OFC_EUNSUPPORTED
        assert lib.ofc_blob_links_read(0, pc, pd, 1, 0, hp, sp) == L.OFC_EINVAL
        assert lib.ofc_blob_links_read(0, pc, pd, -1, 4, hp, sp) == L.OFC_EINVAL
        assert lib.ofc_blob_links_read(0, pc, pd, 65535, 4, hp, sp) == L.OFC_EUNSUPPORTED
        assert lib.ofc_blob_links_read(0, None, pd, 1, 4, hp, sp) == L.OFC_EINVAL
        assert lib.ofc_blob_moves_dev(0, None, 2, 2, 1, pc) == L.OFC_EINVAL and lib.ofc_blob_moves_dev(0, pa, 2, 2, 1, None) == L.OFC_EINVAL
        assert lib.ofc_blob_moves_dev(0, C.c_void_p(a.ptr + 4), 2, 2, 1, pc) == L.OFC_EINVAL         # a field is 8-byte aligned
        assert lib.ofc_blob_moves_dev(0, pa, 2, 2, 1, C.c_void_p(c.ptr + 2)) == L.OFC_EINVAL
        assert lib.ofc_blob_links_dev(0, None, pb, 2, 2, 2, 1, 4, pc, pd) == L.OFC_EINVAL
        assert lib.ofc_blob_links_dev(0, pa, None, 2, 2, 2, 1, 4, pc, pd) == L.OFC_EINVAL
        assert lib.ofc_blob_links_dev(0, pa, pb, 2, 2, 2, 1, 4, None, pd) == L.OFC_EINVAL
        assert lib.ofc_blob_links_dev(0, pa, pb, 2, 2, 2, 1, 4, pc, None) == L.OFC_EINVAL
        assert lib.ofc_blob_links_dev(0, pa, pb, 2, 2, 2, 1, 4, C.c_void_p(c.ptr + 4), pd) == L.OFC_EINVAL      # the keys are 8 bytes
        assert lib.ofc_blob_links(0, None, hp, 2, 2, 2, 1, 4, None, hp, sp) == L.OFC_EINVAL
        assert lib.ofc_blob_links(0, hp, None, 2, 2, 2, 1, 4, None, hp, sp) == L.OFC_EINVAL
        assert lib.ofc_blob_links(0, hp, hp, 2, 2, 2, 1, 4, None, None, sp) == L.OFC_EINVAL
        assert lib.ofc_bench_blob_links(0, pa, pb, 2, 2, 2, 4, 1, C.byref(C.c_float())) == L.OFC_EINVAL
        assert lib.ofc_bench_blob_links(0, pa, pb, 2, 2, 2, 0, 0, C.byref(C.c_float())) == L.OFC_EINVAL
        assert lib.ofc_stream_set_blob_links(None, 4) == L.OFC_EINVAL and lib.ofc_stream_read_blob_links(None, hp, sp, 4) == L.OFC_EINVAL
        for x in (c, d):                                                         # nothing was launched: the outputs keep their fill
            assert (x.download((x.nbytes,), np.uint8) == 0x55).all()
        assert (host == -7).all() and (small == -7).all()
        # one pair: allowed, zero transitions, nothing written, and the outputs may be NULL
        a.upload(np.full(4, -1, np.int32))
        b.upload(np.zeros(4, np.int32))
        assert lib.ofc_blob_links_dev(0, pa, pb, 2, 2, 1, 1, 4, None, None) == L.OFC_OK
        assert lib.ofc_blob_links_dev(0, pa, pb, 2, 2, 1, 1, 4, pc, pd) == L.OFC_OK
        assert lib.ofc_blob_links_read(0, None, None, 0, 4, None, None) == L.OFC_OK
        assert (c.download((c.nbytes,), np.uint8) == 0x55).all() and (d.download((d.nbytes,), np.uint8) == 0x55).all()
        with pytest.raises(ValueError):
            _B().links_dev(a.ptr, b.ptr, 2, 2, 2, max_links=0)
        with pytest.raises(L.OfcError):
            _B().links_dev(a.ptr, b.ptr, 2, 2, 2, max_links=65537)
    finally:
        for x in (a, b, c, d):
            x.free()


# ---- the Python layer on host arrays ----
@pytest.mark.parametrize("name", ["blocks-200x50", "merge-and-split-200x50", "single-pair-64x16", "Nx1"])
def test_blobs_then_link_on_host_arrays(name):
    B = _B()
    case = LC.BY_NAME[name]
    for conn, min_area in ((8, 1), (4, 9)):
        b = B.connected_components(case.keys, connectivity=conn, min_area=min_area, flow=case.flow)
        assert b.links is None and b.nlinks is None and b.moves is None
        assert B.link(b, case.flow, min_area=min_area) is b
        assert np.array_equal(b.moves, LC.case_moves(case)) and b.moves.dtype == np.int32
        same_links((b.links, b.nlinks), LC.reference(case, conn, min_area))
        t = B.tracks(b)
        assert len(t.ids) == len(b) and all(len(i) == len(r) for i, r in zip(t.ids, b.records))
    raw = np.full((len(case.keys) - 1, 8, 3), -7, np.int64)                      # ofc_blob_links itself, without moves_out
    n = np.full(len(case.keys) - 1, -7, np.int32)
    L = _L()
    H, W = case.keys.shape[1:]
    lab = np.ascontiguousarray(b.labels)
    L.check(L.load().ofc_blob_links(0, L.ptr(lab), L.ptr(case.flow), W, H, len(lab), 9, 8, None, L.ptr(raw), L.ptr(n)))
    same_links(([raw[t, :max(m, 0)] for t, m in enumerate(n)], n), LC.reference(case, 4, 9, 8))
    with pytest.raises(ValueError, match="does not match"):
        B.link(b, case.flow[:, :, :-1])
    if name == "merge-and-split-200x50":                                         # two merge: the tie goes to the smaller root
        b = B.link(B.connected_components(case.keys), case.flow)
        assert [i.tolist() for i in B.tracks(b).ids] == [[0, 1], [0], [0, 2]]


# ---- compensation: tracks over a synthetic clip ----
def pairwise_fields(frames):
    from opticalflowclustering_amd.flow import FlowEngine
    eng = FlowEngine(frames.shape[2], frames.shape[1], max_batch=1)
    try:
        return np.stack([eng.calc(frames[t], frames[t + 1]) for t in range(len(frames) - 1)])
    finally:
        eng.close()


@pytest.fixture(scope="module")
def clips():
    """the still and the panning clip of blob_link_cases with their pairwise fields: read-only"""
    from types import SimpleNamespace
    out = {}
    for name, pan in (("still", (0, 0)), ("pan", LC.CLIP_PAN)):
        frames = LC.rect_clip(pan)
        fields = pairwise_fields(frames)
        for a in (frames, fields):
            a.setflags(write=False)
        out[name] = SimpleNamespace(frames=frames, fields=fields, W=frames.shape[2], H=frames.shape[1], n=len(fields))
    return out


def two_whole_tracks(b, n):
    t = _B().tracks(b)
    assert b.found.tolist() == [2] * n and t.n_tracks == 2 and t.lengths().tolist() == [n, n] and t.broken == []
    assert all(i.tolist() == [0, 1] for i in t.ids)
    return t


@pytest.mark.parametrize("which,model", [("still", "translation"), ("pan", "translation"), ("pan", "affine")])
def test_compensate_blobs_link_tracks_finds_the_two_rectangles_through_the_clip(clips, which, model):
    from opticalflowclustering_amd import camera
    B = _B()
    clip = clips[which]
    residual, _ = camera.compensate(clip.fields, model)
    b = B.moving_blobs(residual, thr=LC.CLIP_THR, min_area=LC.CLIP_MIN_AREA)
    B.link(b, clip.fields, min_area=LC.CLIP_MIN_AREA)                            # the moves of the raw flow
    two_whole_tracks(b, clip.n)
    if which == "pan":
        # the residual does not say where a pixel goes: moves taken from it change the link table
        wrong = B.link(B.moving_blobs(residual, thr=LC.CLIP_THR, min_area=LC.CLIP_MIN_AREA), residual, min_area=LC.CLIP_MIN_AREA)
        assert any(not np.array_equal(x, y) for x, y in zip(b.links, wrong.links))
        assert not np.array_equal(b.moves, wrong.moves)


# ---- ClipPipeline ----
def test_pipeline_links_equal_the_host_route_and_need_captured_moves_after_compensation(clips):
    from opticalflowclustering_amd.pipeline import ClipPipeline
    B = _B()
    clip = clips["pan"]
    spec = dict(thr=LC.CLIP_THR, min_area=LC.CLIP_MIN_AREA)
    pipe = ClipPipeline(clip.W, clip.H, len(clip.frames), batch_pairs=2)
    try:
        pipe.upload_frames(clip.frames)
        pipe.run_flow()
        raw = pipe.flows_host()
        got = pipe.blobs(by="moving", links=64, **spec)                          # moves of the resident field as it stands
        want = B.link(B.moving_blobs(raw, **spec), raw, min_area=LC.CLIP_MIN_AREA, max_links=64)
        same_links((got.links, got.nlinks), (want.links, want.nlinks))
        assert np.array_equal(got.labels, want.labels)
        plain = pipe.blobs(by="moving", **spec)                                  # without links= nothing changes
        assert plain.links is None and np.array_equal(plain.labels, want.labels)
        with pytest.raises(ValueError, match="max_links"):
            pipe.blobs(by="moving", links=0, **spec)
        pipe.compensate_camera("translation")
        with pytest.raises(ValueError, match="capture_moves"):
            pipe.blobs(by="moving", links=64, **spec)
        assert pipe.blobs(by="moving", **spec).links is None                     # blobs alone are as before
        pipe.run_flow()                                                          # a new field: the flag is gone
        raw = pipe.flows_host()
        pipe.capture_moves()
        pipe.compensate_camera("translation")
        residual = pipe.flows_host()
        got = pipe.blobs(by="moving", links=64, **spec)
        want = B.link(B.moving_blobs(residual, **spec), raw, min_area=LC.CLIP_MIN_AREA, max_links=64)
        same_links((got.links, got.nlinks), (want.links, want.nlinks))
        two_whole_tracks(got, clip.n)
        pipe.run_flow()                                                          # discards the captured moves
        assert pipe.moves is None
        pipe.compensate_camera("translation")
        with pytest.raises(ValueError, match="capture_moves"):
            pipe.blobs(by="moving", links=64, **spec)
    finally:
        pipe.close()


# ---- FlowStream ----
@pytest.fixture(scope="module")
def long_clip():
    """ten frames of the panning clip and their nine pairwise fields: read-only"""
    from types import SimpleNamespace
    frames = LC.rect_clip(LC.CLIP_PAN, n_frames=10)
    fields = pairwise_fields(frames)
    for a in (frames, fields):
        a.setflags(write=False)
    return SimpleNamespace(frames=frames, fields=fields, W=frames.shape[2], H=frames.shape[1], n=len(fields))


STREAM_SPEC = dict(thr=LC.CLIP_THR, connectivity=8, min_area=12, max_blobs=256)


def _stream(clip, batch_pairs, **kw):
    from opticalflowclustering_amd.stream import FlowStream
    return FlowStream(clip.W, clip.H, batch_pairs=batch_pairs, rows=2, cols=3, **kw)


def run_stream(clip, batch_pairs, camera=None, frames=None, max_links=128):
    st = _stream(clip, batch_pairs, blobs=dict(STREAM_SPEC, max_links=max_links), camera=camera)
    try:
        assert st.blob_args == (8, LC.CLIP_THR, 12, 256) and st.max_links == max_links       # blob_args keeps its four values
        for f in (clip.frames if frames is None else frames):
            st.push(f)
        st.finish()
        return st.blobs()
    finally:
        st.close()


@pytest.mark.parametrize("camera", [None, "affine"])
def test_stream_links_are_the_same_at_every_batch_size_and_equal_the_pairwise_fields(long_clip, camera):
    from opticalflowclustering_amd import camera as cam
    B = _B()
    keyed = long_clip.fields if camera is None else cam.compensate(long_clip.fields, camera)[0]
    want = B.moving_blobs(keyed, STREAM_SPEC["thr"], min_area=12, max_blobs=256)
    B.link(want, long_clip.fields, min_area=12, max_links=128)                   # by the raw flow, whatever the blobs are keyed on
    # under the pan everything moves and the frame is one blob; against the background the two rectangles at the least
    assert min(want.nlinks) >= (1 if camera is None else 2)
    for batch_pairs in (1, 3, 8):                                                # inside a batch, across batches, a short flush
        got = run_stream(long_clip, batch_pairs, camera)
        assert got.labels is None and len(got) == long_clip.n and len(got.links) == long_clip.n - 1
        for a, b in zip(got.records, want.records):
            assert np.array_equal(a, b)
        same_links((got.links, got.nlinks), (want.links, want.nlinks))
    if camera is not None:
        wrong = B.link(B.moving_blobs(keyed, STREAM_SPEC["thr"], min_area=12, max_blobs=256), keyed, min_area=12, max_links=128)
        assert any(not np.array_equal(a, b) for a, b in zip(want.links, wrong.links))        # the order in the stream matters


def test_stream_finish_cuts_the_chain_and_zero_removes_the_links(long_clip):
    B = _B()
    L = _L()
    st = _stream(long_clip, 3, blobs=dict(STREAM_SPEC, max_links=128))
    try:
        for f in long_clip.frames[:5]:
            st.push(f)
        st.finish()
        first = st.blobs()
        for f in long_clip.frames[4:]:                                           # a new clip: its first pair has no predecessor
            st.push(f)
        st.finish()
        second = st.blobs()
        for part, fields in ((first, long_clip.fields[:4]), (second, long_clip.fields[4:])):
            want = B.link(B.moving_blobs(fields, STREAM_SPEC["thr"], min_area=12, max_blobs=256), fields, min_area=12, max_links=128)
            assert len(part.links) == len(fields) - 1
            same_links((part.links, part.nlinks), (want.links, want.nlinks))
        same = st.blobs()                                                        # still there until frames arrive
        same_links((same.links, same.nlinks), (second.links, second.nlinks))
        lib = L.load()
        host, n = np.full((8, 128, 3), -7, np.int64), np.full(8, -7, np.int32)
        assert lib.ofc_stream_read_blob_links(st._h, L.ptr(host), L.ptr(n), 3) == L.OFC_EINVAL      # four transitions need four
        assert (host == -7).all() and (n == -7).all()
        assert lib.ofc_stream_read_blob_links(st._h, L.ptr(host), L.ptr(n), 4) == L.OFC_OK and n[:4].tolist() == second.nlinks.tolist()
        for bad, rc in ((-1, L.OFC_EINVAL), (65537, L.OFC_EUNSUPPORTED)):
            assert lib.ofc_stream_set_blob_links(st._h, bad) == rc
        same_links((st.blobs().links, st.blobs().nlinks), (second.links, second.nlinks))             # the refusals changed nothing
        st.push(long_clip.frames[0])
        assert lib.ofc_stream_set_blob_links(st._h, 64) == L.OFC_EINVAL          # refused while frames are held
        assert lib.ofc_stream_read_blob_links(st._h, L.ptr(host), L.ptr(n), 8) == L.OFC_EINVAL
        with pytest.raises(ValueError, match="holds frames"):
            st.set_blobs(**STREAM_SPEC, max_links=0)
        for f in long_clip.frames[1:4]:
            st.push(f)
        st.finish()
        assert len(st.blobs().links) == 2
        st.set_blobs(**STREAM_SPEC, max_links=0)                                 # removes the links, keeps the blobs
        assert st.max_links == 0 and st.blob_args == (8, LC.CLIP_THR, 12, 256)
        for f in long_clip.frames[:4]:
            st.push(f)
        st.finish()
        got = st.blobs()
        assert got.links is None and got.nlinks is None and len(got) == 3
        assert lib.ofc_stream_read_blob_links(st._h, L.ptr(host), L.ptr(n), 8) == L.OFC_EINVAL       # no links: nothing to read
        st.set_blobs(**STREAM_SPEC, max_links=16)
        st.set_blobs(connectivity=None)                                          # the blobs go, and the links with them
        assert st.blob_args is None and st.max_links == 0
        assert lib.ofc_stream_set_blob_links(st._h, 16) == L.OFC_EINVAL          # only on a stream that has blobs
        assert lib.ofc_stream_set_blob_links(st._h, 0) == L.OFC_EINVAL
    finally:
        st.close()


def test_stream_link_tables_grow_past_their_first_allocation(clips):
    """frames cycling through 4 images of the still clip, 261 pushes at batch_pairs = 8: the 33rd batch takes the tables past
    their 256 pairs.  Pair t is (image t % 4, image (t + 1) % 4), so transition t equals transition t % 4 of the cycle"""
    B = _B()
    clip = clips["still"]
    images = clip.frames[:4]
    cycle = np.stack([images[t % 4] for t in range(6)])                          # pairs 0 .. 4: transitions 0 .. 3
    fields = pairwise_fields(cycle)
    want = B.link(B.moving_blobs(fields, STREAM_SPEC["thr"], min_area=12, max_blobs=256), fields, min_area=12, max_links=32)
    assert np.array_equal(fields[4].view(np.uint32), fields[0].view(np.uint32)) and min(want.nlinks) >= 2
    assert len({l.tobytes() for l in want.links}) == 4                           # the four transitions differ: a misplaced one shows
    got = run_stream(clip, 8, frames=[images[t % 4] for t in range(261)], max_links=32)
    assert len(got) == 260 and len(got.links) == 259
    for t in range(259):
        assert got.nlinks[t] == want.nlinks[t % 4] and np.array_equal(got.links[t], want.links[t % 4]), t


# ---- the command line ----
def test_motion_grids_tracks_on_the_resident_route_and_on_the_stream(tmp_path, long_clip):
    from opticalflowclustering_amd import camera as cam
    from opticalflowclustering_amd import motionGrids as G
    names = ("clip.npy", "fit.csv", "model.npy", "res.csv", "stream.csv", "t_fit.csv", "t_res.csv", "t_stream.csv", "b_plain.csv")
    clip_path, fit_csv, model, res_csv, stream_csv, t_fit, t_res, t_stream, b_plain = (str(tmp_path / n) for n in names)
    frames = long_clip.frames[:6]
    np.save(clip_path, np.repeat(frames[..., None], 3, -1))
    B = _B()
    fields = long_clip.fields[:5]
    residual, _ = cam.compensate(fields, "translation", (3.0, 1.5))
    blob = ["--blob-thr", str(LC.CLIP_THR), "--blob-min-area", "12"]
    base = ["--path", clip_path, "-c", "3", "--rows", "3", "--cols", "4", "--camera", "translation", "--camera-thresholds", "3,1.5"]
    _, centres = G.main(base + blob + ["-f", fit_csv, "--seed", "5", "--save-model", model, "--blobs", t_fit, "--tracks"])
    G.main(base + blob + ["-f", res_csv, "--model", model, "--blobs", t_res, "--tracks"])
    G.main(base + blob + ["-f", stream_csv, "--model", model, "--stream", "--batch-pairs", "2", "--blobs", t_stream, "--tracks"])
    want = B.cluster_blobs(residual, centres, thr=LC.CLIP_THR, min_area=12)
    B.link(want, fields, min_area=12, max_links=G.MAX_LINKS)
    tracks = B.tracks(want)
    text = ",".join(B.TRACK_CSV_HEADER) + "\n" + "".join(",".join(str(v) for v in r) + "\n" for r in want.rows(tracks))
    assert len(want.rows()) >= 2 * len(fields) and tracks.lengths().max() >= 2 and tracks.n_tracks < len(want.rows())
    assert open(t_res).read() == text and open(t_stream).read() == text and open(t_fit).read() == text
    G.main(base + blob + ["-f", res_csv, "--model", model, "--blobs", b_plain])                    # without --tracks: as it was
    assert open(b_plain).read() == ",".join(B.CSV_HEADER) + "\n" + "".join(",".join(str(v) for v in r) + "\n" for r in want.rows())
