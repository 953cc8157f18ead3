"""The clips, case tables and bars test_gpu_flow_sequences.py (GPU: the flow engine and the streaming ingest across sequences
of calls on one handle) and test_oracle_flow_sequences.py (CPU: the clips are fit for that purpose) share.  numpy only at
import.

Two clips, both of synth.frame's analytic texture:
  the clip         N_FRAMES frames of W x H = 160 x 96 (two pyramid levels at the default parameters: 96 * 0.5 = 48 >= 32,
                   24 < 32).  The step from frame t to t + 1 differs from every other step (step()), so a pair built from
                   the wrong frame, a repeated frame or a pair across a boundary is off by far more than any bar here.
  the growth clip  GROW_FRAMES frames of 32 x 32 (one level), a rule without a period: for the one case that pushes more
                   pairs than the stream's result buffer first holds (256)."""
import numpy as np

from opticalflowclustering_amd import synth

W, H = 160, 96
N_FRAMES = 24                       # 3 * 7 + 2 = 23 frames is the longest stream; one more for a shifted second segment
GRID = (3, 4)                       # rows, cols of the stream cases: 32 x 40 px cells
FINE_GRID = (14, 25)                # used once: 6 x 6 px cells, 12 rows and 10 columns of remainder ignored
TEXTURE_SEED = 11

GROW_W = GROW_H = 32
GROW_FRAMES = 300                   # 299 pairs at 7 per batch: the buffer of 256 grows at the 37th batch, slot 0's 19th
GROW_GRID = (2, 2)
GROW_SEED = 12

ANCHOR_PAIRS = (0, (N_FRAMES - 1) // 2, N_FRAMES - 2)      # first, a middle one, last: against the CPU oracle
ANCHOR_REL, ANCHOR_ABS = 1e-4, 1e-3                        # test_gpu_flow.py's end-to-end bars
ANCHOR_MARGIN = 2.0                                        # the oracle's own float32 error leaves at least this much room

DISTINCT_PX = 0.05                  # any two pairs of the clip differ by more than this in some cell mean
CANCEL_FLOOR = 1e-3                 # |cell mean| >= this * mean|x| over the cell, for u and v, in every cell
GROW_DISTINCT_PX = 1e-4             # growth clip: any two rows differ by more than this (1000 x the cell-mean bar)
SUM_BAR = 1e-9                      # _stats sums: <= 1e-9 * max(1, |want|) (test_flow_epilogue_column_sums_feed_the_fit)

STREAM_BATCHES = (1, 2, 3, 7)


def step(t):
    """displacement of the content from frame t to frame t + 1, px: u grows with t, v cycles with period 3, so no two
    steps are closer than 0.11 px in u"""
    return 0.45 + 0.11 * t, -0.4 - 0.2 * (t % 3)


def clip():
    """(N_FRAMES, H, W) uint8"""
    p = synth.texture_params(TEXTURE_SEED)
    x = y = 0.0
    out = []
    for t in range(N_FRAMES):
        out.append(synth.frame(W, H, x, y, p))
        dx, dy = step(t)
        x, y = x + dx, y + dy
    return np.stack(out)


def grow_step(t):
    """never repeats within the clip: u rises by 0.004 px per frame, v falls by 0.003"""
    return 0.2 + 0.004 * t, -0.1 - 0.003 * t


def grow_clip():
    """(GROW_FRAMES, 32, 32) uint8"""
    p = synth.texture_params(GROW_SEED)
    x = y = 0.0
    out = []
    for t in range(GROW_FRAMES):
        out.append(synth.frame(GROW_W, GROW_H, x, y, p))
        dx, dy = grow_step(t)
        x, y = x + dx, y + dy
    return np.stack(out)


def bgr_frame(t, frames):
    """a coloured HxWx3 frame whose three channels are three different frames of the clip (so BGR2GRAY mixes them)"""
    n = len(frames)
    return np.ascontiguousarray(np.stack([frames[t % n], frames[(t + 5) % n], frames[(t + 11) % n]], -1))


def gray_as_bgr(g):
    """g in all three channels: BGR2GRAY's weights (1868 + 9617 + 4899) / 16384 sum to one, so it gives g back exactly"""
    return np.ascontiguousarray(np.stack([g, g, g], -1))


def stream_lengths(B):
    """T of case A for batch_pairs B: 1, 2, B, B+1, B+2, 2B+1, 2B+2, 3B+1, 3B+2 without duplicates"""
    return sorted({1, 2, B, B + 1, B + 2, 2 * B + 1, 2 * B + 2, 3 * B + 1, 3 * B + 2})


STREAM_CASES = [(B, T) for B in STREAM_BATCHES for T in stream_lengths(B)]


def cell_blocks(flow, rows, cols):
    """(rows, ys, cols, xs, 2) float64 view of the KmeanGrids geometry: H // rows x W // cols cells, remainder ignored"""
    h, w = flow.shape[:2]
    ys, xs = h // rows, w // cols
    return np.asarray(flow[:ys * rows, :xs * cols], np.float64).reshape(rows, ys, cols, xs, 2)


def cell_means(flow, rows, cols):
    """(rows * cols, 2) float64 block means"""
    return cell_blocks(flow, rows, cols).mean((1, 3)).reshape(rows * cols, 2)


def cell_mean_bar(flow, rows, cols):
    """(rows * cols, 2) bar on |got - want| for a float32 cell mean formed as ONE rounding of a float64 sum:
    spacing(float32(|want|)) for the rounding (twice the half ulp it can cost, which also covers the float64 division) plus
    2^-40 * mean|x| over the cell, which bounds the float64 sum of up to 2^12 terms in any order (n * 2^-53 * sum|x| / n),
    the reference's own float64 mean included"""
    b = cell_blocks(flow, rows, cols)
    assert b.shape[1] * b.shape[3] <= 1 << 12
    want = b.mean((1, 3)).reshape(rows * cols, 2)
    mean_abs = np.abs(b).mean((1, 3)).reshape(rows * cols, 2)
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2.0 ** -40 * mean_abs


def cancellation(flow, rows, cols):
    """min over cells and components of |cell mean| / mean|x|"""
    b = cell_blocks(flow, rows, cols)
    return float((np.abs(b.mean((1, 3))) / np.abs(b).mean((1, 3))).min())


def min_pair_distance(means):
    """min over distinct rows a != b of max|means[a] - means[b]|; means (n, cells, 2)"""
    m = means.reshape(len(means), -1)
    d = np.abs(m[:, None, :] - m[None, :, :]).max(-1)
    d[np.diag_indices(len(m))] = np.inf
    return float(d.min())


def rel(a, b):
    return np.linalg.norm((a - b).ravel().astype(np.float64)) / max(np.linalg.norm(b.ravel().astype(np.float64)), 1e-30)


# H: windows (first frame, pairs, _stats call?) run in this order on one max_batch = 5 engine over the first 9 frames: 5, 1, 3,
# 5, 2 pairs, plain and _stats calls alternating.  The first _stats call is the 1-pair window, so the scratch of the sums has
# to grow for the 5-pair one; the last window is a short _stats call into scratch sized by a longer one
SEQ_FRAMES = 9
SEQ_MAX_BATCH = 5
SEQ_WINDOWS = ((0, 5, False), (6, 1, True), (2, 3, False), (3, 5, True), (1, 2, False), (7, 1, True))
