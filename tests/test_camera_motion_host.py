"""Camera motion without a GPU: the exports, the host-only check and solve (the function the kernel runs), the proof that
the cases of tests/camera_motion_cases.py are well-conditioned, and the Python and command-line fronts."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libofc.so is loaded, as in bench.py: this file sorts first in the suite, and a process
#               that loads libofc first and torch later holds two HIP runtimes, on which the RCCL tests then fail)

from tests import camera_motion_cases as CC

EXPORTS = ("ofc_motion_check", "ofc_motion_solve", "ofc_motion_moments_dev", "ofc_motion_fit_dev", "ofc_motion_subtract_dev",
           "ofc_motion_fit", "ofc_motion_compensate", "ofc_stream_set_camera", "ofc_stream_read_camera", "ofc_bench_motion")


def _L():
    from opticalflowclustering_amd import _lib
    return _lib


def test_the_new_exports_exist():
    L = _L()
    lib = C.CDLL(L.LIB_PATH)
    missing = [n for n in EXPORTS if not hasattr(lib, n)]
    assert not missing, missing
    assert set(EXPORTS) <= set(L.EXPORTS)
    header = open(L.LIB_PATH.replace("opticalflowclustering_amd/libofc.so", "include/ofc.h")).read()
    assert all(f"int {n}(" in header for n in EXPORTS)


def test_motion_check_decides_on_the_host():
    L = _L()
    lib = L.load()
    assert lib.ofc_motion_check(8192, 8192, 2) == L.OFC_EUNSUPPORTED and "2^37" in lib.ofc_last_error().decode()
    assert lib.ofc_motion_check(8192, 8192, 1) == L.OFC_EUNSUPPORTED
    assert lib.ofc_motion_check(1, 64, 2) == L.OFC_EINVAL and lib.ofc_motion_check(64, 1, 2) == L.OFC_EINVAL
    assert lib.ofc_motion_check(1, 64, 1) == L.OFC_OK
    assert lib.ofc_motion_check(3840, 2160, 2) == L.OFC_OK and lib.ofc_motion_check(3840, 2160, 1) == L.OFC_OK
    for kind in (0, 3, -1):
        assert lib.ofc_motion_check(64, 48, kind) == L.OFC_EINVAL
    assert lib.ofc_motion_check(0, 48, 1) == L.OFC_EINVAL and lib.ofc_motion_check(64, -2, 2) == L.OFC_EINVAL
    # the limit itself: W * H * max(W, H) < 2^37.  4096 x 4096 x 4096 = 2^36 passes, 2^37 exactly does not
    assert lib.ofc_motion_check(4096, 4096, 2) == L.OFC_OK
    assert lib.ofc_motion_check(8192, 2048, 2) == L.OFC_EUNSUPPORTED          # 2^13 * 2^11 * 2^13 = 2^37
    assert lib.ofc_motion_check(8191, 2048, 2) == L.OFC_OK


def _solve(m, kind):
    L = _L()
    mm = np.array([int(v) for v in m], np.int64)
    p, st = np.full(6, 7.0), C.c_int(-1)
    assert L.load().ofc_motion_solve(L.ptr(mm), kind, L.ptr(p), C.byref(st)) == L.OFC_OK
    return p, st.value


def test_solve_refusals_and_degenerate_moments():
    L = _L()
    lib = L.load()
    m, p, st = np.zeros(13, np.int64), np.zeros(6), C.c_int()
    assert lib.ofc_motion_solve(None, 2, L.ptr(p), C.byref(st)) == L.OFC_EINVAL
    assert lib.ofc_motion_solve(L.ptr(m), 2, None, C.byref(st)) == L.OFC_EINVAL
    assert lib.ofc_motion_solve(L.ptr(m), 2, L.ptr(p), None) == L.OFC_EINVAL
    assert lib.ofc_motion_solve(L.ptr(m), 0, L.ptr(p), C.byref(st)) == L.OFC_EINVAL
    for kind, n in ((2, 0), (2, 2), (1, 0)):                                     # too few pixels
        mm = [n, 0, 0, 4 * n, 0, 4 * n, 5, 0, 0, 5, 0, 0, 0]
        p, status = _solve(mm, kind)
        assert status == 1 and not p.any() and CC.solve_exact(mm, kind)[0] is None
    one_column = [6, 0, 0, 0, 0, 70, 6 << 16, 0, 0, 0, 0, 0, 0]                  # X = 0 throughout: the second pivot is 0
    assert _solve(one_column, 2)[1] == 1 and CC.solve_exact(one_column, 2)[0] is None
    p, status = _solve([1] + [0] * 5 + [3 << 15, 0, 0, -(1 << 14), 0, 0, 0], 1)  # one pixel is enough for a translation
    assert status == 0 and np.array_equal(p, [1.5, 0, 0, -0.25, 0, 0])


@pytest.mark.parametrize("case", CC.CASES, ids=repr)
def test_solve_against_the_exact_solution_of_every_round(case):
    _, fits = CC.reference(case)
    solved = 0
    for ref in fits:
        # all thirteen of every round under both kinds, and the rounds as a history of the case's kind reports them
        todo = [(m, k) for m in ref["full"] for k in (1, 2)] + [([int(v) for v in r], case.kind) for r in ref["moments"]]
        for m, kind in todo:
            want, kappa = CC.solve_exact(m, kind)
            got, status = _solve(m, kind)
            assert status == (want is None)
            if want is None:
                assert not got.any()
                continue
            err, bound = np.abs(got - want).max(), CC.solve_bound(kappa, want)
            assert err <= bound, (case, kind, err, bound, kappa)
            solved += 1
    assert solved or case.name.startswith("all-outside")


def test_every_case_is_well_conditioned_and_none_is_left_out():
    """what lets the GPU tests demand equal integers: no valid pixel's residual lies within 2^-20 px of a threshold in any
    round, so the reference's plain f64 and the device's fma chains (and its own model, which differs from the reference's
    by the solve bound, orders of magnitude below the margin) select the same pixels"""
    seen, least, worst = [], np.inf, 0.0
    for case in CC.CASES:
        f, fits = CC.reference(case)
        assert f.shape == (case.npair, case.H, case.W, 2) and f.dtype == np.float32
        for ref in fits:
            assert ref["margin"] >= CC.MARGIN, (case, ref["margin"])
            assert all(k < CC.KAPPA_MAX for k in ref["kappa"]), (case, ref["kappa"])
            least, worst = min(least, ref["margin"]), max([worst] + ref["kappa"])
        seen.append(case.name)
    print("least margin %.3e px, largest kappa_inf %.3e" % (least, worst))
    assert seen == [c.name for c in CC.CASES] and len(set(seen)) == len(seen) >= 19
    sizes = {(c.W, c.H) for c in CC.CASES}
    assert sizes >= {(2, 2), (3, 130), (130, 3), (64, 48), (67, 45), (257, 5), (1, 64), (1920, 24)}
    assert {c.npair for c in CC.CASES} == {1, 3}


def test_the_cases_show_what_they_are_named_for():
    def one(name, i=0):
        f, fits = CC.reference(CC.BY_NAME[name])
        return f[i], fits[i]
    f, ref = one("64x48")
    block = np.abs(f[..., 0] - CC.predict(np.array(CC.BACKGROUND), 64, 48)[0]) > 3
    assert 0.10 <= block.mean() <= 0.15
    assert ref["status"] == 0 and ref["moments"][0][0] == 64 * 48 and ref["moments"][-1][0] == 64 * 48 - block.sum()
    assert np.abs(ref["models"][-1] - CC.BACKGROUND).max() < 2e-3 < np.abs(ref["models"][0] - CC.BACKGROUND).max()
    f, ref = one("range-limit")
    assert ref["moments"][0][12] == 3 and ref["moments"][0][0] == 64 * 48 - 3 and (np.abs(f) == np.float32(1024)).sum() == 3
    assert ref["moments"][0][6] > 1023 * 65536 and ref["moments"][-1][0] < ref["moments"][0][0] - 2   # the largest float below: used, then dropped
    f, ref = one("non-finite")
    assert ref["moments"][0][12] == 6 and ref["status"] == 0
    f, ref = one("ties")
    assert (np.abs(f) == 2.0 ** -17).sum() > 1000 and ref["moments"][-1][0] == 64 * 48
    assert ref["moments"][0][6] != int(round(float(f[..., 0].astype(np.float64).sum() * 65536)))     # the ties went to even
    f, ref = one("all-outside-in-the-middle", 1)
    assert ref["status"] == 2 and not ref["models"].any() and ref["moments"][0][12] == 64 * 48 and not ref["moments"][1:].any()
    assert one("all-outside-in-the-middle", 0)[1]["status"] == 0 == one("all-outside-in-the-middle", 2)[1]["status"]
    f, ref = one("starved-in-round-2")
    assert ref["status"] == 1 and ref["moments"][1][0] == 64 * 48 and ref["moments"][2][0] < 3 and not ref["moments"][3].any()
    assert np.array_equal(ref["models"][2], ref["models"][1]) and np.array_equal(ref["models"][3], ref["models"][1])
    f, ref = one("constant")
    assert np.array_equal(ref["models"][-1], [1.25, 0, 0, -0.5, 0, 0])
    f, ref = one("67x45-x3-translation", 1)
    assert not ref["moments"][:, list(CC.COORD_MOMENTS)].any() and ref["moments"][:, 0].all()


def test_camera_motion_tuple_evaluate_and_arguments():
    from opticalflowclustering_amd import camera as cam
    cm = cam.CameraMotion(np.zeros((2, 6)), np.zeros(2, np.int32), np.ones(2, np.int64), np.zeros(2, np.int64))
    assert cm.params.shape == (2, 6) and cm._fields == ("params", "status", "inliers", "outside")
    p = np.array([1.5, 0.25, -0.5, -2.0, 0.125, 1.0])
    e = cam.evaluate(p, 5, 4)
    assert e.shape == (4, 5, 2) and e.dtype == np.float64
    for y in range(4):
        for x in range(5):
            hx, hy = x - 2.0, y - 1.5
            assert e[y, x, 0] == 1.5 + 0.25 * hx - 0.5 * hy and e[y, x, 1] == -2.0 + 0.125 * hx + hy
    eu, ev = CC.predict(p, 5, 4)
    assert np.array_equal(e[..., 0], eu) and np.array_equal(e[..., 1], ev)
    both = cam.evaluate(np.stack([p, 2 * p]), 5, 4)
    assert both.shape == (2, 4, 5, 2) and np.array_equal(both[0], e) and np.array_equal(both[1], 2 * e)
    with pytest.raises(ValueError, match="params"):
        cam.evaluate(np.zeros(5), 5, 4)
    assert cam.camera_args("affine")[0::2] == (2, 3) and cam.camera_args("translation", ())[0::2] == (1, 0)
    for bad in (("similarity", (1.0,)), ("affine", (0.0,)), ("affine", (1.0, float("nan"))), ("affine", (-1.0,)),
                ("affine", (1.0,) * 9)):
        with pytest.raises(ValueError):
            cam.camera_args(*bad)
    assert cam.parse_camera(None) is None and cam.parse_camera("affine") == ("affine", (4.0, 2.0, 1.0))
    assert cam.parse_camera(("translation", [3, 1])) == ("translation", (3.0, 1.0))
    p6, st = cam.solve([4, 0, 0, 4, 0, 4, 4 << 16, 4 << 16, 0, 0, 0, 8 << 16, 0])    # 2 x 2: u = 1 + X, v = 2 Y
    assert st == 0 and np.array_equal(p6, [1.0, 2.0, 0, 0, 0, 4.0])
    assert "guess" in cam.estimate_camera_motion.__doc__ and "guess" in cam.__doc__


def test_motion_grids_camera_arguments():
    from opticalflowclustering_amd import motionGrids as G
    base = ["--path", "x.npy", "-c", "3", "-f", "out.csv"]
    a = G.parse_arguments(base)
    assert a.camera == "none" and a.camera_spec is None and a.camera_thresholds == (4.0, 2.0, 1.0) and a.camera_out is None
    a = G.parse_arguments(base + ["--camera", "affine"])
    assert a.camera_spec == ("affine", (4.0, 2.0, 1.0))
    a = G.parse_arguments(base + ["--camera", "translation", "--camera-thresholds", "3,1.5", "--camera-out", "cam.npy"])
    assert a.camera_spec == ("translation", (3.0, 1.5)) and a.camera_out == "cam.npy"
    assert G.parse_arguments(base + ["--camera", "affine", "--camera-thresholds", ""]).camera_spec == ("affine", ())
    a = G.parse_arguments(base + ["--camera", "affine", "--fit-stream"])
    assert a.fit_stream and a.camera_spec[0] == "affine"
    a = G.parse_arguments(base + ["--camera", "affine", "--stream", "--model", "m.npy", ])
    assert a.stream and a.camera_spec[0] == "affine"
    for bad in (["--camera", "projective"], ["--camera", "affine", "--camera-thresholds", "4,0"],
                ["--camera", "affine", "--camera-thresholds", "4,x"], ["--camera", "affine", "--camera-thresholds", "1,1,1,1,1,1,1,1,1"],
                ["--camera-out", "cam.npy"]):
        with pytest.raises(SystemExit):
            G.parse_arguments(base + bad)
