"""The oracle's box mean + solve at windows wider than 17 px -- the semantics k_box_solve_wide is held to -- against an
independent float64 box mean (scipy.ndimage.uniform_filter, mode="nearest": the edge row / column repeated as far as the
window reaches) and 2x2 solve, windows wider than the frame included.  CPU only."""
import numpy as np
import pytest
from scipy import ndimage

from oracle import oracle as O


def _solve_f64(M, winsize):
    M = M.astype(np.float64)
    b = [ndimage.uniform_filter(M[..., c], winsize, mode="nearest") for c in range(5)]
    idet = 1.0 / (b[0] * b[2] - b[1] * b[1] + 1e-3)
    return np.stack([(b[0] * b[4] - b[1] * b[3]) * idet, (b[2] * b[3] - b[1] * b[4]) * idet], -1)


@pytest.mark.parametrize("ws", [31, 61, 255])
@pytest.mark.parametrize("W,H", [(130, 60), (333, 97), (40, 24), (17, 200), (16, 16)])
def test_update_flow_blur_wide_window(W, H, ws):
    rng = np.random.default_rng(W * H + ws)
    M = rng.random((H, W, 5)).astype(np.float32) + np.float32([1, 0, 1, 0, 0])
    z5 = np.zeros((H, W, 5), np.float32)
    got, M_out = O.update_flow_blur(z5, z5, np.zeros((H, W, 2), np.float32), M, ws, False)
    want = _solve_f64(M, ws)
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (W, H, ws)
    assert np.array_equal(M_out, M)                       # update_mats off: the matrices are left alone


def test_window_wider_than_the_frame_repeats_the_edges():
    """a window twice the frame: every output averages the same replicated extension, so a field constant along one axis
    gives the mean of the edge-weighted profile"""
    H, W, ws = 24, 40, 101
    m = ws // 2
    rng = np.random.default_rng(1)
    prof = rng.random(W).astype(np.float32)
    M = np.zeros((H, W, 5), np.float32)
    M[..., 0] = 1
    M[..., 2] = 1
    M[..., 3] = prof[None, :]
    z5 = np.zeros_like(M)
    got, _ = O.update_flow_blur(z5, z5, np.zeros((H, W, 2), np.float32), M, ws, False)
    for xx in (0, W // 2, W - 1):
        idx = np.clip(np.arange(xx - m, xx + m + 1), 0, W - 1)
        h1 = prof[idx].astype(np.float64).mean()
        # g11 = g22 = 1, g12 = 0, h2 = 0: flow = (0, h1 / (1 + 1e-3))
        assert abs(got[5, xx, 1] - h1 / (1 + 1e-3)) <= 1e-6 and abs(got[5, xx, 0]) <= 1e-7
