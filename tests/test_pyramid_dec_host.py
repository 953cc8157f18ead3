"""The launch geometry of k_pyramid_dec (ofc_pyramid_dec_geometry; no device): bands of 256 input columns, 8-row steps, strips
of whole steps.  Checked against brute force: the bands cover the columns, the strips cover the steps, no strip is empty or
shorter than four steps except the last, and the output rows the kernel assigns to the steps of a strip (step t: level 1 rows
4t+3 .. 4t+6, level 2 rows 2t+1, 2t+2, level 3 row t; step -1 belongs to the first strip) give every row of every level to
exactly one strip."""
import pytest

from opticalflowclustering_amd import stages

SIZES = [(W, H) for W in (32, 256, 260, 512, 1024, 1920, 3840) for H in (32, 40, 68, 72, 136, 256, 1080, 2160)]


@pytest.mark.parametrize("n", (1, 2, 3, 4, 61, 300))
def test_plan_against_brute_force(n):
    for W, H in SIZES:
        bands, steps, sps, strips = stages.pyramid_dec_geometry(W, H, n)
        assert (bands - 1) * 256 < W <= bands * 256
        assert (steps - 1) * 8 < H <= steps * 8
        assert sps >= 4 and strips >= 1 and (strips - 1) * sps < steps <= strips * sps
        # as many strips as bring the batch to about 1024 work-groups, while a strip keeps four steps
        want = max(1, (1024 + n * bands // 2) // (n * bands))
        assert strips <= want
        for per_step, lead, h in ((4, 3, H // 2), (2, 1, H // 4), (1, 0, H // 8)):
            owner = [0] * h
            for s in range(strips):
                t0, t1 = s * sps, min(steps, (s + 1) * sps)
                for t in range(-1 if s == 0 else t0, t1):
                    for a in range(per_step):
                        oy = per_step * t + lead + a
                        if 0 <= oy < h:
                            owner[oy] += 1
            assert owner == [1] * h, (W, H, n, per_step)


def test_the_bench_batch():
    """61 frames of 1080p: 8 bands x 2 strips, 976 work-groups on 256 CUs"""
    assert stages.pyramid_dec_geometry(1920, 1080, 61) == (8, 135, 68, 2)
