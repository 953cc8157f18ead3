"""The case tables test_gpu_flow_geometry.py (GPU: the three strip-marching flow kernels at every strip height their cost
models pick) and test_flow_geometry_host.py (CPU: the tables reach what they claim, asked of the C cost models through
ofc_flow_launch_geometry, and the stage inputs make bit equality across heights a fair demand) share.  numpy only at
import, in the style of flow_domain_cases.py, whose inputs, oracle unrolling and bars are reused.

Why: k_flow_iter, k_box_solve and k_polyexp cut a level into horizontal strips whose height comes from a host-side cost
model of the level size AND the number of pairs in the batch.  At the suite's small frames and batches of at most 5 pairs
the fused iteration always gets 16-row strips -- exactly one super-step of its unrolled march -- so what a strip carries
from one super-step to the next (the register ring wrapping, the f64 running sums, the carried coarse rows of the x2
upsample, the flow vectors prefetched a step ahead) would only be exercised at 1080p.  Two ways in:
  stage level   ofc_flow_iterate mode 0 takes the strip height as an argument: every multiple of 16 on small frames
  engine level  one batch of many pairs of a small frame moves every level's models to the heights production runs"""
import json
import os

import numpy as np

import flow_domain_cases as D

BARS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_geometry_bars.json")

SUPER_STEP = 16         # rows of one unrolled super-step of k_flow_iter: strip heights are multiples of it


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# 1. stage level: ofc_flow_iterate mode 0 (k_flow_iter<M, 0>) at every strip height
# ---------------------------------------------------------------------------------------------------------------------
STAGE_HEIGHTS = (190,       # 11 full super-steps + 14 rows, not a multiple of 4
                 77,        # odd
                 48)        # exactly three super-steps
STAGE_ITERS = (1, 3)
# one taller frame at the default window: the only way to three or more strips higher than 128 rows (rows 144: 144 + 144 +
# 13), which the bench's first batch runs at level 0 of 1080p (272-row strips, four of them, the last one partial)
STAGE_TALL = (15, 301)


def stage_rows(H):
    """every multiple of 16 up to the single strip, one height above the frame, and one value that is no multiple of 16
    (the launcher rounds it up to 32)"""
    single = cdiv(H, SUPER_STEP) * SUPER_STEP
    return list(range(SUPER_STEP, single + 1, SUPER_STEP)) + [single + SUPER_STEP, 17]


# (winsize, W, H): one width with a column seam per window, T + 1
STAGE_CASES = [(ws, D.tile_width(ws) + 1, H) for ws in D.ITER_WINDOWS for H in STAGE_HEIGHTS] + \
              [(STAGE_TALL[0], D.tile_width(STAGE_TALL[0]) + 1, STAGE_TALL[1])]


def stage_case_id(ws, W, H, iters):
    return D.iter_case_id(ws, "T+1", W, H, iters)


def stage_inputs(ws, W, H):
    return D.iter_inputs(W, H, seed=W + ws)


def measure_stage_distances():
    """{case id: max |oracle - float64|} per stage case and iteration count: flow_domain_cases.measure_stage_distances'
    method on this table (what golden/make_flow_geometry_bars.py records)"""
    out = {}
    for ws, W, H in STAGE_CASES:
        R0, R1, flow = stage_inputs(ws, W, H)
        n = max(STAGE_ITERS)
        o32, o64 = D.oracle_iterations(R0, R1, flow, n, ws), D.f64_iterations(R0, R1, flow, n, ws)
        for it in STAGE_ITERS:
            out[stage_case_id(ws, W, H, it)] = float(np.abs(o32[it - 1] - o64[it - 1]).max())
    return out


def recorded_stage_distances():
    with open(BARS_PATH) as f:
        return json.load(f)["max_abs_oracle_minus_float64"]


def window_sums_running(M, m):
    """float64 sums of M (H, W, C float32) over rows y - m .. y + m, replicate-clamped, as the kernels form them: the first
    window added up top to bottom, then + the row that enters - the row that leaves, all the way down the frame"""
    H = M.shape[0]
    M = M.astype(np.float64)
    rows = lambda y: M[min(max(y, 0), H - 1)]
    out = np.empty_like(M)
    v = np.zeros_like(M[0])
    for j in range(-m, m + 1):
        v = v + rows(j)
    out[0] = v
    for y in range(1, H):
        v = v + (rows(y + m) - rows(y - 1 - m))
        out[y] = v
    return out


def window_sums_fresh(M, m, reverse):
    """the same sums, each window added up on its own, top to bottom (a strip's warm-up) or bottom to top"""
    H = M.shape[0]
    M = M.astype(np.float64)
    idx = np.clip(np.arange(H)[:, None] + np.arange(-m, m + 1)[None, :], 0, H - 1)      # (H, 2m + 1)
    out = np.zeros_like(M)
    for j in (range(2 * m, -1, -1) if reverse else range(2 * m + 1)):
        out = out + M[idx[:, j]]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 2. engine level: one calc_frames_dev of n pairs; the pair counts were read off ofc_flow_launch_geometry (the host test
#    asserts through it what they reach, so a retuned model fails there instead of quietly shrinking coverage)
# ---------------------------------------------------------------------------------------------------------------------
REF_BATCH = 3           # the reference runs the same clip three pairs at a time: 16-row strips (box 16, polyexp 8) at every
                        # level of every case here, the geometry the rest of the suite anchors against the oracle
SLACK_BYTES = 4096      # behind the last pair, pre-filled with 0xFF like the rest of the result buffer
ANCHOR_REL, ANCHOR_ABS = 1e-4, 1e-3     # the end-to-end bars
SUM_BAR = 1e-9          # _stats sums: <= 1e-9 * max(1, |want|) (flow_sequence_cases.SUM_BAR)


def _g(name, W, H, pairs, **kw):
    return (name, dict(D.DEFAULTS, **kw), W, H, tuple(pairs))


# level-0 strip height of the fused iteration (k_box_solve for winsize 17) per pair count in the comments; the coarser levels
# move as well (test_flow_geometry_host prints the whole table)
ENGINE_CASES = [
    # every level an exact half (250x150, 125x75; 62x38 is not): the x2 upsample form with its carried coarse rows
    #                           16  80  112  112  304  64   160 (two strips)
    _g("defaults-500x300", 500, 300, (1, 35, 52, 103, 137, 171, 256)),
    # odd width, inexact halves: the general upsample form, per-pixel stores
    _g("defaults-499x301", 499, 301, (52, 103, 171, 256)),
    # 250x190 (the x2 form from 125x95, the general form at 125x95 from 62x48): two column tiles x one strip at 256 pairs: 2 tiles padded to 8 work-groups per group of pairs, so 6 of every 8
    # work-groups are grid padding and the pair map's early exit carries most of the grid
    _g("defaults-250x190-grid-padding", 250, 190, (256,)),
    #                                    16  32  48  64   96
    _g("ws5-250x190", 250, 190, (1, 43, 86, 129, 256), winsize=5),
    # staged k_box_solve<8>: box rows 16  32  64   128 at level 0, 64 at level 1 with 256 pairs
    _g("ws17-staged-500x300", 500, 300, (1, 52, 103, 171, 256), winsize=17),
    # k_polyexp<7>: 8-row strips up to 41 pairs (42 images), 16 from 42 pairs on
    _g("poly7-sigma1.5-250x190", 250, 190, (1, 22, 41, 42, 65, 128, 256), poly_n=7, poly_sigma=1.5),
]

ENGINE_RUNS = [(name, kw, W, H, n) for name, kw, W, H, pairs in ENGINE_CASES for n in pairs]


def engine_run_id(name, n):
    return f"{name}-{n}pairs"


def engine_levels(W, H, kw):
    """[(w, h)] of the pyramid levels the engine runs, level 0 first"""
    n = D.pyramid_levels(W, H, kw["pyr_scale"], kw["levels"])
    return [D.level_geometry(W, H, kw["pyr_scale"], k)[:2] for k in range(n + 1)]


def anchor_pairs(n):
    """first, middle, last"""
    return sorted({0, n // 2, n - 1})


# ---------------------------------------------------------------------------------------------------------------------
# 3. what a (strip height, level height) is an instance of
# ---------------------------------------------------------------------------------------------------------------------
HEIGHT_CLASSES = ("16", "32", "48", "64-128", ">128")
STRIP_CLASSES = ("1", "2", "3+partial", "3+exact")


def height_class(rows):
    assert rows >= SUPER_STEP and rows % SUPER_STEP == 0, rows
    return str(rows) if rows <= 48 else ("64-128" if rows <= 128 else ">128")


def strip_class(rows, H):
    n = cdiv(H, rows)
    return str(n) if n <= 2 else ("3+partial" if H % rows else "3+exact")


def geometry_class(rows, H):
    return height_class(rows), strip_class(rows, H)
