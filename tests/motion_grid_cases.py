"""What test_motion_grids_host.py and the two GPU files share: a numpy restatement of ofc_grid_label_counts_dev, the
cases it is run on, and the field on which ClipPipeline.assign is checked label for label."""
import math

import numpy as np


def model_counts(labels, k, rows, cols, flow=None):
    """labels (n, H, W) u8, flow (n, H, W, 2) or None -> counts (n, rows*cols, k) int32 [, sums (n, rows*cols, k, 2) f64].
    The grid of KmeanGrids.py:56-59: cells of (H // rows) x (W // cols) pixels from the top left, the remainder in no
    cell; np.bincount per cell over the labels below k; sums by math.fsum (the correctly rounded exact sum)"""
    labels = np.asarray(labels, np.uint8)
    n, H, W = labels.shape
    ys, xs = H // rows, W // cols
    counts = np.zeros((n, rows * cols, k), np.int32)
    sums = np.zeros((n, rows * cols, k, 2), np.float64) if flow is not None else None
    for f in range(n):
        for cy in range(rows):
            for cx in range(cols):
                sl = (f, slice(cy * ys, (cy + 1) * ys), slice(cx * xs, (cx + 1) * xs))
                lab = labels[sl].ravel()
                keep = lab < k
                counts[f, cy * cols + cx] = np.bincount(lab[keep], minlength=k)
                if flow is None:
                    continue
                uv = np.asarray(flow)[sl].reshape(-1, 2).astype(np.float64)
                for j in np.unique(lab[keep]):
                    for c in range(2):
                        sums[f, cy * cols + cx, j, c] = math.fsum(uv[lab == j, c])
    return counts if flow is None else (counts, sums)


def model_abs_sums(labels, k, rows, cols, flow):
    """model_counts' sums over |u|, |v|: the sum of magnitudes the f64 summation bound is stated in"""
    return model_counts(labels, k, rows, cols, np.abs(np.asarray(flow)))[1]


def sum_bound(counts, abs_sums):
    """|any-order f64 sum - exact sum| <= n 2^-53 sum|x| per entry, n = its count (valid while n^2 2^-53 <= 1)"""
    n = counts.astype(np.float64)[..., None]
    assert (n * n * 2.0 ** -53 <= 1).all()
    return n * 2.0 ** -53 * abs_sums


# (rows, cols, W, H, n frames): see each line of the issue's geometry list
GEOMETRIES = {
    "remainders-odd-frame": (3, 4, 83, 61, 3),         # remainders 3 and 1; W*H odd: frames 1, 2 start at odd addresses
    "whole-frame": (1, 1, 64, 48, 2),
    "one-px-wide": (2, 40, 40, 9, 2),                   # cols = W
    "one-px-high": (9, 3, 40, 9, 2),                    # rows = H
    "wider-than-group": (2, 2, 600, 10, 2),             # cells 300 px wide: wider than a wave and than a work-group
    "smaller-than-wave": (7, 9, 67, 59, 2),             # cells 7 x 8 px
    "reference-1080p": (14, 25, 1920, 1080, 1),
    "one-px-cells": (16, 16, 16, 16, 2),
}
KS = (1, 2, 5, 6, 8, 9, 16)                             # either side of the 5 / 8 / 16 instantiations


def random_labels(seed, n, H, W, k, kind="uniform"):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, k, (n, H, W)).astype(np.uint8)
    if kind == "absent":                                # cluster 1 occurs nowhere (k >= 2)
        lab = rng.integers(0, k - 1, (n, H, W))
        return np.where(lab >= 1, lab + 1, lab).astype(np.uint8)
    if kind == "unassigned":                            # about 10 % 0xFF
        lab = rng.integers(0, k, (n, H, W)).astype(np.uint8)
        lab[rng.random((n, H, W)) < 0.1] = 0xFF
        return lab
    if kind == "out-of-range":                          # labels in [k, 255] only
        return rng.integers(k, 256, (n, H, W)).astype(np.uint8)
    raise ValueError(kind)


def integer_flow(seed, n, H, W):
    return np.random.default_rng(seed).integers(-8, 9, (n, H, W, 2)).astype(np.float32)


def real_flow(seed, n, H, W):
    return (np.random.default_rng(seed).standard_normal((n, H, W, 2)) * 3).astype(np.float32)


# ---- the field ClipPipeline.assign is checked on, label for label ----
ASSIGN_CENTRES = np.array([[0.0131, -0.0217], [2.7183, 0.3679], [-1.9319, 2.2913], [0.6180, -3.1416], [-3.3166, -1.0986]])
ASSIGN_W, ASSIGN_H, ASSIGN_FRAMES = 64, 48, 4


def lattice():
    """every point of the lattice the assign field draws from: multiples of 1/8 in [-4, 4]^2, (65*65, 2) f64"""
    g = np.arange(-32, 33) / 8.0
    return np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def direct_sqdist(X, centres):
    """float64 direct-form squared distances (dx*dx + dy*dy), (N, k)"""
    X = np.asarray(X, np.float64)
    d = X[:, None, :] - np.asarray(centres, np.float64)[None]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]


def assign_field(seed=7):
    """(pairs, H, W, 2) f32 on the lattice, for ClipPipeline(ASSIGN_W, ASSIGN_H, ASSIGN_FRAMES)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-32, 33, (ASSIGN_FRAMES - 1, ASSIGN_H, ASSIGN_W, 2)) / 8.0).astype(np.float32)


def moving_blobs_clip(n_frames=5, W=96, H=64):
    """(n, H, W, 3) u8: two textured blobs moving in different directions over a static textured background"""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    back = (110 + 40 * np.sin(xx * 0.21) * np.cos(yy * 0.17) + rng.integers(-6, 7, (H, W))).astype(np.float64)
    tex = 128 + 100 * np.sin(xx * 0.9 + yy * 0.6) * np.cos(xx * 0.4 - yy * 0.8)
    clip = np.empty((n_frames, H, W), np.uint8)
    for t in range(n_frames):
        img = back.copy()
        for (cx, cy, vx, vy, r) in ((24 + 3 * t, 20, 3, 0, 11), (70, 44 - 2 * t, 0, -2, 10)):
            m = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
            img[m] = np.roll(np.roll(tex, vy * t, 0), vx * t, 1)[m]
        clip[t] = np.clip(img, 0, 255).astype(np.uint8)
    return np.repeat(clip[..., None], 3, -1)
