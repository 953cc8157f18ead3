"""What test_gpu_flow_bidir.py (GPU) and test_flow_bidir_host.py (CPU) share: the work-group map of the bidirectional
iteration restated in numpy, the palindrome clip the bidirectional call is held against, and the case table.  numpy only at
import.

The demand is bit equality, and it is a fair one: a forward-only engine on the palindrome f0 .. fn fn-1 .. f0 (2n pairs)
sizes its strips for 2n pairs, as the bidirectional call on f0 .. fn does for its 2n logical pairs; level images and
expansions are per frame; so every work-group does the same arithmetic on the same operands.  fwd[t] is pair t of the
palindrome run and bwd[t] pair 2n - 1 - t."""
import numpy as np

from opticalflowclustering_amd import synth

DEFAULTS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)
GROUP = 8                   # work-groups that share an XCD's L2 are 8 ids apart; a group of 8 ids takes 8 tiles of one pair


def cdiv(a, b):
    return -(-a // b)


# ---- the work-group map (k_flow_iter<.., BIDIR>), restated ----
def block_map(block, n_pairs):
    """work-group id -> (tile, frame pair, direction) of a bidirectional launch over n_pairs frame pairs"""
    logical = 2 * n_pairs
    group, rem = divmod(block, GROUP * logical)
    q = rem // GROUP
    return group * GROUP + rem % GROUP, q >> 1, q & 1


def field_index(pair, direction, n_pairs):
    """where the field of (pair, direction) lives in a buffer of 2 n_pairs fields: forward fields first"""
    return direction * n_pairs + pair


def operand_frames(pair, direction):
    """(frame of R0, frame of R1): the backward work-group swaps the two"""
    return pair + direction, pair + 1 - direction


# ---- frames ----
def clip(W, H, n_frames, seed=3, step=(0.8, -0.4)):
    p = synth.texture_params(seed)
    return np.stack([synth.frame(W, H, step[0] * t, step[1] * t, p) for t in range(n_frames)])


def palindrome(frames):
    """f0 .. fn fn-1 .. f0: 2n + 1 frames, 2n pairs"""
    return np.concatenate([frames, frames[-2::-1]])


def palindrome_pairs(n_pairs):
    """-> (pairs of the palindrome run that are fwd[0..n), pairs that are bwd[0..n))"""
    return list(range(n_pairs)), [2 * n_pairs - 1 - t for t in range(n_pairs)]


# ---- cases: (name, W, H, parameters, frame pairs) ----
def _c(name, W, H, n, **kw):
    return (name, W, H, dict(DEFAULTS, **kw), n)


CASES = [
    _c("ws15-two-column-tiles-272x80-2pairs", 272, 80, 2),
    _c("ws15-one-column-tile-160x64-1pair", 160, 64, 1),                    # 2 logical pairs: less than a group of eight
    _c("ws15-three-strips-partial-last-200x40-2pairs", 200, 40, 2),
    _c("ws15-5pairs-straddling-the-padded-tail-272x80", 272, 80, 5),
    _c("ws15-odd-size-UPS1-251x67-2pairs", 251, 67, 2),
    _c("ws15-levels0-UPS0-only-160x64-2pairs", 160, 64, 2, levels=0),
    _c("ws15-one-iteration-UPS-only-launch-272x80-2pairs", 272, 80, 2, iterations=1),
    _c("ws15-two-iterations-272x80-1pair", 272, 80, 1, iterations=2),
    _c("ws5-258x80-2pairs", 258, 80, 2, winsize=5),                  # tile 252: two column tiles
    _c("ws9-251x67-2pairs", 251, 67, 2, winsize=9),                  # tile 248: two column tiles, UPS 1
    _c("ws17-staged-box8-272x80-2pairs", 272, 80, 2, winsize=17),
    _c("ws17-staged-levels0-160x64-1pair", 160, 64, 1, winsize=17, levels=0),
    _c("ws21-staged-wide-251x67-2pairs", 251, 67, 2, winsize=21),
    _c("poly7-272x80-2pairs", 272, 80, 2, poly_n=7, poly_sigma=1.5),
    _c("scale0.7-levels4-ws11-UPS1-200x120-2pairs", 200, 120, 2, pyr_scale=0.7, levels=4, winsize=11),
]
FRONT_END_ENV = [("OFC_FLOW_FRONT_OVERLAP", "0"), ("OFC_PYRAMID_FUSED", "0"), ("OFC_FLOW_STAGED", "1")]
FRONT_END_CASE = "ws15-two-column-tiles-272x80-2pairs"


def case(name):
    return next(c for c in CASES if c[0] == name)

