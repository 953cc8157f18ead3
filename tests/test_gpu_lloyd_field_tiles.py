"""GPU parity of the Lloyd tile sweeps in their field form (csrc/lloyd_tiles.hip: 16 x 4-pixel tiles under 64 x 8-pixel
groups, taken when the fit is told the field's size, ofc_kmeans_fit_dev_field).  Every fit runs under OFC_LLOYD_PRUNE=2 and
3 and is held to the CPU oracle and to the same call under OFC_LLOYD_PRUNE=0 by the bars of test_gpu_lloyd_tiles.same_fit:
labels bit-equal, n_iter equal, centres <= 1e-9, inertia <= 1e-10 relative.  The `tested` / `pure` counts of every sweep
(OFC_LLOYD_TRACE) must equal the two-level float64 model of lloyd_field_tile_cases.py, whose fields have no borderline box.

Measured on an MI355X: this module 1.9 s (38 tests).
"""
import re

import numpy as np
import pytest

import lloyd_field_tile_cases as F
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TRACE = re.compile(r"\[ofc lloyd\] it (\d+) tiles_mode (-?\d+) tested (\d+) pure (\d+) ")
FULL, PRUNED, PROBE = 0, 1, 2


def fit_dev(X, C0, field, policy, monkeypatch, capfd=None, **kw):
    """kmeans_fit_dev on an uploaded field -> dict(cen, lab, inertia, n_iter, st: prune_stats(), rows: (mode, tested, pure)
    per sweep from the trace line when capfd is given)"""
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.cluster import kmeans_fit_dev, prune_stats
    monkeypatch.setenv("OFC_LLOYD_PRUNE", str(policy))
    if capfd is not None:
        monkeypatch.setenv("OFC_LLOYD_TRACE", "1")
        capfd.readouterr()
    buf = _lib.DeviceBuffer(X.nbytes, 0).upload(np.ascontiguousarray(X))
    lab = _lib.DeviceBuffer(len(X), 0)
    try:
        lab.upload(np.full(len(X), 0xEE, np.uint8))                    # a label that is never written shows
        cen, inertia, n_iter = kmeans_fit_dev(buf.ptr, _lib.F32, len(X), 2, C0, labels_ptr=lab.ptr, field=field, **kw)
        out = dict(cen=cen, inertia=inertia, n_iter=n_iter, lab=lab.download((len(X),), np.uint8).astype(np.int32),
                   st=prune_stats())
    finally:
        buf.free()
        lab.free()
    if capfd is not None:
        out["rows"] = [tuple(int(v) for v in m.groups())[1:] for m in TRACE.finditer(capfd.readouterr().err)]
    return out


def same_fit(r, cen, lab, inertia, n_iter):
    assert r["n_iter"] == n_iter
    assert np.array_equal(r["lab"], lab)
    assert np.abs(r["cen"] - cen).max() <= 1e-9
    assert abs(r["inertia"] - inertia) <= 1e-10 * max(inertia, 1e-300)


@pytest.fixture(scope="module")
def unpruned():
    """the same call under OFC_LLOYD_PRUNE=0, once per case"""
    cache = {}

    def get(name, monkeypatch):
        if name not in cache:
            c = F.case(name)
            cache[name] = fit_dev(c["X"], c["C0"], (c["W"], c["H"]), 0, monkeypatch)
            assert cache[name]["st"]["tile_sweeps"] == 0
        return cache[name]
    return get


@pytest.mark.parametrize("policy", [2, 3])
@pytest.mark.parametrize("name", list(F.CASES))
def test_field_fit_equals_oracle_unpruned_and_the_models_counts(name, policy, unpruned, monkeypatch, capfd):
    c = F.case(name)
    assert c["borderline"] == 0 and c["n_iter"] >= 2
    r = fit_dev(c["X"], c["C0"], (c["W"], c["H"]), policy, monkeypatch, capfd)
    same_fit(r, c["cen"], c["lab"], c["inertia"], c["n_iter"])
    plain = unpruned(name, monkeypatch)
    same_fit(plain, c["cen"], c["lab"], c["inertia"], c["n_iter"])
    assert np.abs(r["cen"] - plain["cen"]).max() <= 1e-12
    # the labels as an image stack: a wrong row or quad of a label store would show here
    assert np.array_equal(r["lab"].reshape(c["n"], c["H"], c["W"]), c["lab"].reshape(c["n"], c["H"], c["W"]))
    # every sweep ran pruned (these fields pass the 45 % / 30 % thresholds by far) with the model's counts, in tiles
    want = [(PRUNED, s["tested"], s["pure"]) for s in c["sweeps"]]
    print("trace", r["rows"], "model", want)
    assert r["rows"] == want
    st = r["st"]
    assert st["tile_sweeps"] == st["pruned_sweeps"] == c["n_iter"] and st["final_pruned"], st
    assert st["tiles_tested"] == sum(s["tested"] for s in c["sweeps"]) and st["tiles_pure"] == sum(s["pure"] for s in c["sweeps"])


def test_contents_fail_exactly_where_they_are_built_to():
    """what the issue asks of each content, on the model at the converged centres (host arithmetic only)"""
    def failing(name):
        c = F.case(name)
        rep = c["final"]
        return c, ~rep["group_pass"], (~rep["tile_pass"]).reshape(-1, 8)
    # vertical edge at x = 40: group column 0 of every band fails, and in it the tile column x 32..47 (both tile rows)
    c, g, t = failing("vertical-128x16x3")
    assert np.array_equal(g.reshape(-1, 2), np.tile([True, False], (6, 1)))
    assert np.array_equal(t[g], np.tile([0, 0, 1, 0, 0, 0, 1, 0], (6, 1)).astype(bool)) and not t[~g].any()
    # horizontal edge at y = 5: band 0 of every field fails, and in it the lower tile row
    c, g, t = failing("horizontal-128x16x3")
    assert np.array_equal(g.reshape(3, 2, 2), np.tile([[[True, True], [False, False]]], (3, 1, 1)))
    assert np.array_equal(t[g], np.tile([0, 0, 0, 0, 1, 1, 1, 1], (6, 1)).astype(bool))
    # one pixel: one group fails, one of its 8 tiles is mixed
    c, g, t = failing("one-tile-128x16x3")
    assert g.sum() == 1 and t.sum() == 1
    # group-aligned populations: nothing fails
    c, g, t = failing("aligned-128x16x3")
    assert not g.any() and not t.any()
    # the layout field: group blocks pass, tile blocks fail as groups and pass as tiles, quad blocks fail altogether
    c, g, t = failing("layout-128x16x3")
    assert np.array_equal(g, np.repeat([False, True, True], 4)) and np.array_equal(t.all(1), np.repeat([False, False, True], 4))
    assert not t[:8].any()


@pytest.mark.parametrize("policy", [2, 3])
def test_constant_field_every_group_passes_and_the_group_path_writes_the_labels(policy, monkeypatch, capfd):
    W, H, n = 128, 16, 3
    X, C0 = F.constant_field(W, H, n)
    cen, lab, inertia, n_iter = O.kmeans_fit(X, C0)
    r = fit_dev(X, C0, (W, H), policy, monkeypatch, capfd)
    same_fit(r, cen, lab, inertia, n_iter)
    NT = len(X) // 64
    assert r["rows"] == [(PRUNED, NT, NT)] * n_iter, r["rows"]
    assert r["st"]["final_pruned"] and (r["lab"] == 0).all()       # 0xEE anywhere: a label the group path did not write


@pytest.mark.parametrize("W,H", [(80, 8), (64, 12)])
@pytest.mark.parametrize("policy", [2, 3])
def test_sizes_the_2d_tiles_do_not_fit_run_the_1d_tiles(W, H, policy, monkeypatch, capfd):
    """W % 64 != 0 or H % 8 != 0: the fit silently takes the 64 x 1 tiles -- the very records of the call without a field"""
    n = 4
    pop = np.zeros((n, H, W), int)          # a field is 10 or 12 whole 64-sample runs: one population per field, except that
    pop[1::2] = 1                           # field 0 is cut at x = 40, so a quarter of the 64 x 1 tiles is mixed
    pop[0, :, 40:] = 1
    X = F.populations(pop, seed=W)
    C0 = F.POP[:2] + 0.25
    cen, lab, inertia, n_iter = O.kmeans_fit(X, C0)
    a = fit_dev(X, C0, (W, H), policy, monkeypatch, capfd)
    b = fit_dev(X, C0, None, policy, monkeypatch, capfd)
    same_fit(a, cen, lab, inertia, n_iter)
    assert np.array_equal(a["cen"], b["cen"]) and a["inertia"] == b["inertia"] and np.array_equal(a["lab"], b["lab"])
    assert a["rows"] == b["rows"] and a["st"] == b["st"] and a["st"]["pruned_sweeps"] >= 1


@pytest.mark.parametrize("policy", [2, 3])
def test_white_noise_field_the_probe_switches_pruning_off(policy, monkeypatch, capfd):
    W, H, n = 128, 16, 3
    X, C0 = F.noise_field(W, H, n)
    cen, lab, inertia, n_iter = O.kmeans_fit(X, C0)
    mean = X.astype(np.float64).mean(0)
    share = F.field_report(X, W, H, mean, C0 - mean)["pure"] / (len(X) // 64)
    assert share < 0.2                                                # far under the 45 % and 30 % thresholds
    r = fit_dev(X, C0, (W, H), policy, monkeypatch, capfd)
    same_fit(r, cen, lab, inertia, n_iter)
    plain = fit_dev(X, C0, (W, H), 0, monkeypatch)
    same_fit(plain, cen, lab, inertia, n_iter)
    if policy == 2:       # the probe before iteration 0 turns the policy off: full sweeps, no metadata, full final E-step
        assert r["st"]["pruned_sweeps"] == 0 and r["st"]["tile_sweeps"] == n_iter and not r["st"]["final_pruned"], r["st"]
        assert all(row == (FULL, 0, 0) for row in r["rows"]), r["rows"]
    else:                 # forced: pruned sweeps that skip next to nothing, same fit
        assert r["st"]["pruned_sweeps"] == n_iter and r["st"]["skip_fraction"] < 0.2, r["st"]


def test_one_nan_sample_poisons_its_tile_and_its_group_only(monkeypatch):
    """as test_gpu_lloyd_tile_patterns.test_non_finite_sample_with_a_finite_mean asks of the 1-D tiles: sklearn refuses such
    input, so the reference is the unpruned kernels; the column sums are handed in with the bad sample zeroed, so the mean
    stays finite.  The NaN's tile and its group never pass; the other 7 tiles of that group and every other group do."""
    from opticalflowclustering_amd import _lib
    from opticalflowclustering_amd.cluster import kmeans_fit_dev, prune_stats
    W, H, n = 128, 16, 3
    X, C0, bad = F.nan_field(W, H, n)
    colsum = np.where(np.isfinite(X), X, 0).astype(np.float64).sum(0)
    mean = colsum / len(X)
    rep = F.field_report(X, W, H, mean, C0 - mean)
    NT = len(X) // 64
    assert rep["pure"] == NT - 1 and (~rep["group_pass"]).sum() == 1 and (~rep["tile_pass"]).sum() == 1
    buf = _lib.DeviceBuffer(X.nbytes, 0).upload(X)
    lab = _lib.DeviceBuffer(len(X), 0)
    out = []
    try:
        for policy in (0, 3):
            monkeypatch.setenv("OFC_LLOYD_PRUNE", str(policy))
            cen, inertia, n_iter = kmeans_fit_dev(buf.ptr, _lib.F32, len(X), 2, C0, max_iter=1, labels_ptr=lab.ptr, colsum=colsum,
                                                  field=(W, H))
            st = prune_stats()
            out.append((cen, lab.download((len(X),), np.uint8).copy(), n_iter))
            if policy == 3:
                assert st["pruned_sweeps"] == 1 and st["tiles_tested"] == NT and st["tiles_pure"] == NT - 1, st
    finally:
        buf.free()
        lab.free()
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    a, b = out[0][0], out[1][0]
    fin = np.isfinite(a)
    print("finite coordinates:", int(fin.sum()), "largest difference:", np.abs(a[fin] - b[fin]).max())
    assert fin.sum() == 3 and np.array_equal(fin, np.isfinite(b))     # one centre coordinate is poisoned, the fit is not
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True) and np.abs(a[fin] - b[fin]).max() <= 1e-12


def test_run_kmeans_takes_the_field_path_and_a_weighted_fit_stays_unpruned(monkeypatch):
    """ClipPipeline.run_kmeans hands (W, H) on: on a 64 x 48 clip the unweighted fit sweeps 2-D tiles and equals the oracle
    on the resident vectors; with sample_weight the sweeps read every sample, whatever OFC_LLOYD_PRUNE says"""
    from opticalflowclustering_amd.cluster import prune_stats
    from opticalflowclustering_amd.pipeline import ClipPipeline
    pipe = ClipPipeline(64, 48, 3, batch_pairs=2)
    try:
        pipe.synth(0, 1)
        pipe.run_flow()
        uv = pipe.flows_host().reshape(-1, 2)
        C0 = np.quantile(uv.astype(np.float64), [0.1, 0.5, 0.9], axis=0)
        cen, lab, inertia, n_iter = O.kmeans_fit(uv, C0)
        fits = {}
        for policy in (0, 3):
            monkeypatch.setenv("OFC_LLOYD_PRUNE", str(policy))
            c, i, it = pipe.run_kmeans(C0)
            st = prune_stats()
            assert it == n_iter and np.array_equal(pipe.labels_host().reshape(-1), lab)
            assert np.abs(c - cen).max() <= 1e-9 and abs(i - inertia) <= 1e-10 * inertia
            assert st["tile_sweeps"] == (n_iter if policy else 0), st
            if policy:      # 2 pairs x 6 bands x 1 column = 12 groups = 96 tiles per sweep: the 2-D cut was taken
                assert st["tiles_tested"] == st["pruned_sweeps"] * (len(uv) // 64), st
            fits[policy] = pipe.run_kmeans(C0, sample_weight="magnitude")
            assert prune_stats()["tile_sweeps"] == 0
        assert np.array_equal(fits[0][0], fits[3][0]) and fits[0][1:] == fits[3][1:]
    finally:
        pipe.close()


def test_field_entry_point_refuses_what_is_not_a_stack_of_fields():
    from opticalflowclustering_amd import _lib
    import ctypes as C
    lib = _lib.load()
    X = np.zeros((512, 2), np.float32)
    buf = _lib.DeviceBuffer(X.nbytes, 0).upload(X)
    C0, cen = np.zeros((1, 2)), np.zeros((1, 2))
    inertia, n_iter = C.c_double(), C.c_int()

    def call(N, d, dtype, W, H, n):
        return lib.ofc_kmeans_fit_dev_field(0, C.c_void_p(buf.ptr), dtype, N, d, 1, _lib.ptr(C0), 3, 1e-4, None, _lib.ptr(cen),
                                            None, C.byref(inertia), C.byref(n_iter), W, H, n)
    try:
        assert call(512, 2, _lib.F32, 64, 8, 1) == _lib.OFC_OK
        assert call(512, 2, _lib.F32, 32, 8, 2) == _lib.OFC_OK             # a size the 2-D tiles do not fit: the 1-D path
        for bad in [(512, 2, _lib.F32, 64, 8, 2), (512, 2, _lib.F32, 64, 4, 1), (512, 2, _lib.F32, 0, 8, 1),
                    (512, 2, _lib.F32, 64, 8, 0), (256, 4, _lib.F32, 64, 4, 1), (512, 2, _lib.F64, 64, 8, 1)]:
            assert call(*bad) == _lib.OFC_EINVAL, bad
    finally:
        buf.free()
