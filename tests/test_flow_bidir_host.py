"""CPU side of test_gpu_flow_bidir.py: the new exports are declared and bound with the arity of their declarations, the
work-group map of the bidirectional iteration (restated in tests/flow_bidir_cases.py) is a bijection that stays inside the
batch's frames, the geometry export answers without a device, and the case table reaches what it is meant to reach."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libofc.so is loaded, as in test_consistency_host.py)

import flow_bidir_cases as B
import flow_domain_cases as D
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("ofc_flow_calc_frames_dev_bidir", "ofc_flow_calc_frames_dev_bidir_stats", "ofc_flow_launch_geometry_bidir",
           "ofc_bench_flow_bidir", "ofc_stream_set_consist", "ofc_stream_read_consist")


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def geometry():
    from opticalflowclustering_amd import stages
    return stages.flow_launch_geometry_bidir


def test_every_new_export_is_declared_built_and_bound_with_its_arity():
    L = _L()
    lib = C.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "ofc.h")).read()
    for name in EXPORTS:
        assert hasattr(lib, name), name
        m = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
        assert m, name
        assert name in L.EXPORTS, name
        fn = getattr(L.load(), name)
        assert len(fn.argtypes) == len(m.group(1).split(",")), (name, m.group(1))
        assert fn.restype is C.c_int


@pytest.mark.parametrize("n_pairs", range(1, 18))
def test_the_work_group_map_is_a_bijection_inside_the_batch(n_pairs):
    """over a launch of `tiles` tiles (rounded up to groups of eight): every (tile, pair, direction) has exactly one
    work-group, the two directions of a (tile, pair) are 8 ids apart (neighbours on one XCD), the fields fill 0 .. 2n-1
    with the forward ones first, and no operand is read past frame n_pairs"""
    for tiles in (1, 3, 8, 13):
        grid = B.cdiv(tiles, B.GROUP) * B.GROUP * 2 * n_pairs
        seen = {}
        for b in range(grid):
            tile, pair, direction = B.block_map(b, n_pairs)
            assert 0 <= pair < n_pairs and direction in (0, 1)
            assert (tile, pair, direction) not in seen
            seen[(tile, pair, direction)] = b
            r0, r1 = B.operand_frames(pair, direction)
            assert {r0, r1} == {pair, pair + 1} and max(r0, r1) <= n_pairs       # n_pairs + 1 frames: 0 .. n_pairs
            assert (r0, r1) == ((pair, pair + 1) if direction == 0 else (pair + 1, pair))
        padded = B.cdiv(tiles, B.GROUP) * B.GROUP
        assert len(seen) == padded * 2 * n_pairs
        assert {t for t, _, _ in seen} == set(range(padded))
        for (tile, pair, direction), b in seen.items():
            if direction == 0:
                assert seen[(tile, pair, 1)] == b + B.GROUP and b % B.GROUP == seen[(tile, pair, 1)] % B.GROUP
        fields = sorted({B.field_index(p, d, n_pairs) for _, p, d in seen})
        assert fields == list(range(2 * n_pairs))
        assert all(B.field_index(p, 0, n_pairs) < n_pairs <= B.field_index(p, 1, n_pairs) for p in range(n_pairs))


def test_palindrome_pairs_are_the_two_directions():
    frames = np.arange(6)
    pal = B.palindrome(frames)
    assert list(pal) == [0, 1, 2, 3, 4, 5, 4, 3, 2, 1, 0]
    fwd, bwd = B.palindrome_pairs(5)
    for t in range(5):
        assert (pal[fwd[t]], pal[fwd[t] + 1]) == (t, t + 1)
        assert (pal[bwd[t]], pal[bwd[t] + 1]) == (t + 1, t)


def test_geometry_export_is_the_forward_model_at_twice_the_pairs(geometry):
    from opticalflowclustering_amd import stages
    L = _L()
    for W, H, n, ws in ((16, 16, 1, 5), (272, 80, 2, 15), (250, 190, 22, 15), (1920, 1080, 37, 15), (3840, 2160, 16, 9)):
        rows, tiles, grid = geometry(W, H, n, ws)
        assert rows == stages.flow_launch_geometry(W, H, 2 * n, ws)[0]
        assert tiles == B.cdiv(W, 257 - ws) * B.cdiv(H, rows)
        assert grid == B.cdiv(tiles, B.GROUP) * B.GROUP * 2 * n
    out = (C.c_int * 3)()
    for W, H, n, ws in ((0, 16, 1, 15), (16, 0, 1, 15), (16, 16, 0, 15), (16, 16, 1, 14), (16, 16, 1, 3), (16, 16, 1, 17)):
        assert L.load().ofc_flow_launch_geometry_bidir(W, H, n, ws, out) == L.OFC_EINVAL, (W, H, n, ws)
    assert L.load().ofc_flow_launch_geometry_bidir(16, 16, 1, 15, None) == L.OFC_EINVAL


def test_host_only_refusals_of_the_entry_points():
    L = _L()
    lib = L.load()
    assert lib.ofc_flow_calc_frames_dev_bidir(None, None, 2, None, None) == L.OFC_EINVAL
    assert lib.ofc_flow_calc_frames_dev_bidir_stats(None, None, 2, None, None, None) == L.OFC_EINVAL
    ms = C.c_float()
    assert lib.ofc_bench_flow_bidir(0, 64, 64, 1, 1, 0, C.byref(ms)) == L.OFC_EINVAL
    assert lib.ofc_bench_flow_bidir(0, 64, 64, 2, 1, 2, C.byref(ms)) == L.OFC_EINVAL
    assert lib.ofc_bench_flow_bidir(0, 64, 64, 2, 0, 0, C.byref(ms)) == L.OFC_EINVAL


def test_the_case_table_reaches_what_it_names(geometry):
    names = [c[0] for c in B.CASES]
    assert len(set(names)) == len(names)
    assert {c[3]["winsize"] for c in B.CASES} >= {5, 9, 15, 17, 21}
    assert {c[4] for c in B.CASES} >= {1, 2, 5}
    assert any(c[3]["poly_n"] == 7 for c in B.CASES) and any(c[3]["levels"] == 0 for c in B.CASES)
    ups, strips = set(), set()
    for name, W, H, kw, n in B.CASES:
        po = D.oracle_params(kw)
        lv = [tuple(O.level_geometry(W, H, k, po)[:2]) for k in range(O.pyramid_levels(W, H, po) + 1)]
        if kw["winsize"] > 15:
            continue
        ups.add(0)                                                        # every level's later iterations, and the top level
        for k in range(len(lv) - 1):
            ups.add(2 if lv[k] == (2 * lv[k + 1][0], 2 * lv[k + 1][1]) else 1)
        rows, tiles, grid = geometry(W, H, n, kw["winsize"])
        cols = B.cdiv(W, 257 - kw["winsize"])
        strips.add((cols, tiles // cols, H % rows != 0))
        if "two-column-tiles" in name:
            assert cols == 2
        if "one-column-tile" in name:
            assert cols == 1 and tiles < B.GROUP and 2 * n < B.GROUP
        if "three-strips-partial-last" in name:
            assert tiles // cols == 3 and H % rows != 0
        if "straddling" in name:
            # the two directions of the last pair take the last two groups of eight ids; with tiles < 8 both end in padding
            assert tiles % B.GROUP != 0 and n == 5
    assert ups == {0, 1, 2}
    assert any(s >= 2 and part for _, s, part in strips) and any(c == 2 for c, _, _ in strips)
    assert B.case(B.FRONT_END_CASE)[3] == B.DEFAULTS
