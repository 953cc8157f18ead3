"""The clip-wide fit's output on the device: ClipPipeline.assign / cell_clusters and the motionGrids CLI, against the
numpy model of tests/motion_grid_cases.py.

assign's labels are demanded one by one only on the field test_motion_grids_host.py proves unambiguous (the two nearest
centres of every lattice point are >= 1e-3 apart in squared distance); on a computed flow field they are compared with
the fit's own labels and the follow-up is skipped, with a message, should a borderline sample make them differ.
Bars for cell_clusters: counts exact; sums bit-equal where every partial sum is exactly representable (the dyadic lattice),
within n 2^-53 sum|x| of the exact sum otherwise."""
import numpy as np
import pytest

from tests import motion_grid_cases as MC

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattice_pipe():
    """the proven field resident in a pipeline, labelled by assign(ASSIGN_CENTRES)"""
    from opticalflowclustering_amd.pipeline import ClipPipeline
    pipe = ClipPipeline(MC.ASSIGN_W, MC.ASSIGN_H, MC.ASSIGN_FRAMES, batch_pairs=2)
    field = MC.assign_field()
    pipe.flows.upload(field)
    pipe._sums_valid = False            # the engine's column sums are not this field's: assign takes its own
    pipe.assign(MC.ASSIGN_CENTRES)
    yield pipe, field
    pipe.close()


def test_assign_labels_the_proven_field(lattice_pipe):
    pipe, field = lattice_pipe
    want = np.argmin(MC.direct_sqdist(field.reshape(-1, 2), MC.ASSIGN_CENTRES), axis=1).astype(np.uint8)
    got = pipe.labels_host()
    assert got.shape == field.shape[:3]
    assert np.array_equal(got.ravel(), want)            # every sample: none is ambiguous, none is left out
    assert np.array_equal(pipe.flows_host(), field)     # the field itself is untouched


def test_cell_clusters_after_assign(lattice_pipe):
    pipe, field = lattice_pipe
    labels = pipe.labels_host()
    counts, sums = MC.model_counts(labels, 5, 3, 4, field)
    got_c, got_s = pipe.cell_clusters(3, 4, sums=True)
    assert got_c.dtype == np.int32 and np.array_equal(got_c, counts)
    assert np.array_equal(bits(got_s), bits(sums))      # multiples of 1/8 below 2^53/8: every partial sum is exact
    assert np.array_equal(pipe.cell_clusters(3, 4), counts)
    occupancy = np.stack([np.bincount(f.ravel(), minlength=5) for f in labels])
    assert np.array_equal(pipe.cell_clusters(1, 1)[:, 0, :], occupancy)      # rows = cols = 1: the frame's occupancy


def test_assign_with_fewer_centres_rewrites_the_recorded_k(lattice_pipe):
    from opticalflowclustering_amd.pipeline import ClipPipeline
    pipe = ClipPipeline(MC.ASSIGN_W, MC.ASSIGN_H, 2, batch_pairs=1)
    try:
        pipe.flows.upload(lattice_pipe[1][:1])
        pipe._sums_valid = False
        pipe.assign(MC.ASSIGN_CENTRES)
        assert pipe.cell_clusters(2, 2).shape == (1, 4, 5)
        pipe.assign(MC.ASSIGN_CENTRES[:2])
        c = pipe.cell_clusters(2, 2)
        assert c.shape == (1, 4, 2) and c.sum() == MC.ASSIGN_W * MC.ASSIGN_H
        with pytest.raises(ValueError):
            pipe.assign(np.zeros((3, 3)))
    finally:
        pipe.close()


def test_fit_path_and_assign_of_the_fitted_centres():
    from opticalflowclustering_amd.pipeline import ClipPipeline
    W, H, T, k, rows, cols = 96, 64, 4, 3, 3, 4
    pipe = ClipPipeline(W, H, T, batch_pairs=2)
    try:
        pipe.synth()
        pipe.run_flow()
        with pytest.raises(ValueError, match="run_kmeans"):         # run_flow leaves no labels
            pipe.cell_clusters(rows, cols)
        C0, _ = pipe.seed_kmeans(k, random_state=5)
        centers, inertia, n_iter = pipe.run_kmeans(C0)
        labels, flows = pipe.labels_host(), pipe.flows_host()
        counts, sums = MC.model_counts(labels, k, rows, cols, flows)
        got_c, got_s = pipe.cell_clusters(rows, cols, sums=True)
        assert np.array_equal(got_c, counts)
        bound = MC.sum_bound(counts, MC.model_abs_sums(labels, k, rows, cols, flows))
        assert (np.abs(got_s - sums) <= bound).all()
        assert (counts.sum(axis=(1, 2)) == (W // cols) * cols * (H // rows) * rows).all()

        pipe.assign(centers)
        relabelled = pipe.labels_host()
        if not np.array_equal(relabelled, labels):
            pytest.skip(f"assign(fitted centres) and the fit's final E-step disagree on {(relabelled != labels).sum()} "
                        "borderline sample(s) of a field whose conditioning nobody proved: counts not compared")
        assert np.array_equal(pipe.cell_clusters(rows, cols), counts)

        pipe.run_flow()                                             # ... and forgets them again
        with pytest.raises(ValueError, match="assign"):
            pipe.cell_clusters(rows, cols)
    finally:
        pipe.close()


def test_cli(tmp_path):
    from opticalflowclustering_amd import motionGrids as G
    clip, csv, model, cnt = (str(tmp_path / n) for n in ("clip.npy", "out.csv", "model.npy", "counts.npy"))
    np.save(clip, MC.moving_blobs_clip())
    base = ["--path", clip, "-c", "3", "--rows", "3", "--cols", "4"]
    G.main(base + ["-f", csv, "--init", "k-means++", "--seed", "0", "--save-model", model, "--counts", cnt])
    counts, centers = np.load(cnt), np.load(model)
    assert counts.shape == (4, 12, 3) and counts.dtype == np.int32 and centers.shape == (3, 2)
    assert (counts.sum(axis=(1, 2)) == 96 * 63).all()               # 3 x 4 cells of 21 x 24 px
    lines = open(csv).read().splitlines()
    assert len(lines) == 1 + 4 and lines[0] == ",".join(f"cell_{i}" for i in range(12))
    table = np.array([[int(v) for v in ln.split(",")] for ln in lines[1:]])
    assert table.shape == (4, 12) and np.array_equal(table, G.hue_rows(counts, centers))

    csv2, cnt2 = str(tmp_path / "again.csv"), str(tmp_path / "again.npy")
    G.main(base + ["-f", csv2, "--model", model, "--counts", cnt2, "--value", "label"])
    assert np.array_equal(np.load(cnt2), counts)                    # the saved model reproduces the fit's counts
    lines = open(csv2).read().splitlines()
    table = np.array([[int(v) for v in ln.split(",")] for ln in lines[1:]])
    assert np.array_equal(table, G.dominant(counts))

    with pytest.raises(ValueError, match="expected \\(2, 2\\)"):       # a model of another k is refused, not reshaped
        G.main(["--path", clip, "-c", "2", "-f", csv2, "--model", model])
