"""numpy-level access to the individual Farneback stages of libofc (parity-test and bench hooks).
Layouts are OpenCV's internal interleaved ones so results compare 1:1 with the oracle."""
import ctypes as C

import numpy as np

from ._lib import FbParams, check, load, ptr


def level_image(gray, k, params=None, device=0):
    gray = np.ascontiguousarray(gray, np.uint8)
    H, W = gray.shape
    p = params or FbParams()
    out = np.empty((H, W), np.float32)
    w, h = C.c_int(), C.c_int()
    check(load().ofc_level_image(device, ptr(gray), W, H, C.byref(p), k, ptr(out), C.byref(w), C.byref(h)))
    return out.reshape(-1)[: w.value * h.value].reshape(h.value, w.value).copy()


def pyramid_dec(frames, levels, fused=True, device=0):
    """(images, fused_levels): the f32 images of pyramid levels 1..levels (pyr_scale 0.5) of u8 frames [n][H][W], each
    [n][h][w]; fused: one k_pyramid_dec launch for the leading exact decimations (fused_levels of them) and the per-level
    kernels for the rest, otherwise the per-level kernels throughout"""
    frames = np.ascontiguousarray(frames, np.uint8)
    n, H, W = frames.shape
    outs = [np.empty((n, int(np.rint(H * 0.5 ** k)), int(np.rint(W * 0.5 ** k))), np.float32) for k in range(1, levels + 1)]
    ptrs = [ptr(o) for o in outs] + [None] * (3 - levels)
    nf = C.c_int(-1)
    check(load().ofc_pyramid_dec(device, ptr(frames), n, W, H, levels, int(bool(fused)), *ptrs, C.byref(nf)))
    return outs, nf.value


def pyramid_dec_geometry(W, H, n):
    """(bands, steps, steps per strip, strips) of a k_pyramid_dec launch over n frames; needs no device"""
    out = (C.c_int * 4)()
    check(load().ofc_pyramid_dec_geometry(W, H, n, out))
    return tuple(out)


def polyexp(img, n=5, sigma=1.2, device=0):
    img = np.ascontiguousarray(img, np.float32)
    H, W = img.shape
    out = np.empty((H, W, 5), np.float32)
    check(load().ofc_polyexp(device, ptr(img), W, H, n, sigma, ptr(out)))
    return out


def polyexp_u8(gray, n=5, sigma=1.2, device=0):
    """polyexp of pyramid level 0 straight from the u8 frame (the fused form the flow engine runs)"""
    gray = np.ascontiguousarray(gray, np.uint8)
    H, W = gray.shape
    out = np.empty((H, W, 5), np.float32)
    check(load().ofc_polyexp_u8(device, ptr(gray), W, H, n, sigma, ptr(out)))
    return out


def update_matrices(R0, R1, flow, device=0):
    R0, R1, flow = (np.ascontiguousarray(a, np.float32) for a in (R0, R1, flow))
    H, W = flow.shape[:2]
    M = np.empty((H, W, 5), np.float32)
    check(load().ofc_update_matrices(device, ptr(R0), ptr(R1), ptr(flow), W, H, ptr(M)))
    return M


def box_solve(M, winsize=15, device=0):
    M = np.ascontiguousarray(M, np.float32)
    H, W = M.shape[:2]
    flow = np.empty((H, W, 2), np.float32)
    check(load().ofc_box_solve(device, ptr(M), W, H, winsize, ptr(flow)))
    return flow


def flow_resize(flow, dw, dh, mul=1.0, device=0):
    flow = np.ascontiguousarray(flow, np.float32)
    sh, sw = flow.shape[:2]
    out = np.empty((dh, dw, 2), np.float32)
    check(load().ofc_flow_resize(device, ptr(flow), sw, sh, dw, dh, mul, ptr(out)))
    return out


def flow_iterate(R0, R1, flow_in, iters, winsize=15, mode=0, rows_per_block=0, device=0):
    """`iters` Farneback iterations from flow_in with the engine's fused kernels (mode 1: two iterations per launch);
    rows_per_block: strip height of every mode, 0 = the cost model's (mode 0 rounds up to a multiple of 16)"""
    R0, R1, flow_in = (np.ascontiguousarray(a, np.float32) for a in (R0, R1, flow_in))
    H, W = flow_in.shape[:2]
    out = np.empty((H, W, 2), np.float32)
    check(load().ofc_flow_iterate(device, ptr(R0), ptr(R1), ptr(flow_in), W, H, winsize, iters, mode, rows_per_block,
                                  ptr(out)))
    return out


def flow_launch_geometry(W, H, n_pairs, winsize=15):
    """(rows of k_flow_iter, rows of k_box_solve, rows of k_polyexp over n_pairs + 1 images) the cost models pick for a
    W x H level (ofc_flow_launch_geometry); needs no device"""
    out = (C.c_int * 3)()
    check(load().ofc_flow_launch_geometry(W, H, n_pairs, winsize, out))
    return tuple(out)


def flow_launch_geometry_bidir(W, H, n_pairs, winsize=15):
    """(rows of k_flow_iter, tiles of one logical pair, work-groups of the launch) of the bidirectional iteration over
    n_pairs frame pairs (ofc_flow_launch_geometry_bidir); needs no device"""
    out = (C.c_int * 3)()
    check(load().ofc_flow_launch_geometry_bidir(W, H, n_pairs, winsize, out))
    return tuple(out)


def bench_flow_bidir(W, H, n_frames, reps, what, device=0):
    """ms per batch for both directions of n_frames - 1 pairs (what 0: one bidirectional call; 1: two forward-only calls,
    the second on the reversed frames)"""
    ms = C.c_float()
    check(load().ofc_bench_flow_bidir(device, W, H, n_frames, reps, what, C.byref(ms)))
    return ms.value


def bench_flow_iters(W, H, n_pairs, reps, mode, device=0):
    """ms per batch for the last two iterations of a level (mode 0: two launches, mode 1: the two-iteration kernel)"""
    ms = C.c_float()
    check(load().ofc_bench_flow_iters(device, W, H, n_pairs, reps, mode, C.byref(ms)))
    return ms.value


def bench_pyramid_dec(W, H, n_images, levels=3, fused=True, iters=20, device=0):
    """ms per batch of the level images 1..levels of n_images resident frames: one k_pyramid_dec launch or the per-level ones"""
    ms = C.c_float()
    check(load().ofc_bench_pyramid_dec(device, W, H, n_images, levels, int(bool(fused)), iters, C.byref(ms)))
    return ms.value


def bench_polyexp(W, H, n_images, iters, rows_per_block=0, device=0):
    ms = C.c_float()
    check(load().ofc_bench_polyexp(device, W, H, n_images, iters, rows_per_block, C.byref(ms)))
    return ms.value


def bench_lloyd_sweep(X_ptr, N, centers, mean, what, iters=10, device=0):
    """ms per launch of one Lloyd sweep over a resident (u,v) stream (ofc_bench_lloyd_sweep): what 0 full label-less sweep,
    1 pruned tile sweep, 2 metadata-building sweep, 3 final E-step"""
    cen = np.ascontiguousarray(centers, np.float64)
    mean = np.ascontiguousarray(mean, np.float64)
    ms = C.c_float()
    check(load().ofc_bench_lloyd_sweep(device, C.c_void_p(X_ptr), N, len(cen), ptr(cen), ptr(mean), what, iters, C.byref(ms)))
    return ms.value


def bench_lloyd_sweep_w(X_ptr, w_ptr, w_dtype, N, centers, mean, iters=10, device=0):
    """ms per launch of the label-less weighted Lloyd sweep over a resident (u,v) stream and its weights
    (ofc_bench_lloyd_sweep_w): bench_lloyd_sweep(what=0) plus the weight stream"""
    cen = np.ascontiguousarray(centers, np.float64)
    mean = np.ascontiguousarray(mean, np.float64)
    ms = C.c_float()
    check(load().ofc_bench_lloyd_sweep_w(device, C.c_void_p(X_ptr), C.c_void_p(w_ptr), w_dtype, N, len(cen), ptr(cen), ptr(mean),
                                         iters, C.byref(ms)))
    return ms.value


def bench_uv_hist(flow_ptr, n, bins=1024, range=32.0, iters=10, device=0):
    """ms per launch of the (u,v) histogram kernel over a resident field of n vectors (ofc_bench_uv_hist)"""
    ms = C.c_float()
    check(load().ofc_bench_uv_hist(device, C.c_void_p(flow_ptr), n, bins, range, iters, C.byref(ms)))
    return ms.value


def flow_weights_dev(flow_ptr, n, kind, thr, w_ptr, device=0):
    """sample weights from a resident (u,v) field (ofc_flow_weights_dev): kind 'magnitude' -> |(u,v)|, 'moving' -> 1 where
    |(u,v)| >= thr, else 0; n f32 weights written to w_ptr"""
    kinds = {"magnitude": 0, "moving": 1}
    if kind not in kinds:
        raise ValueError(f"weight kind should be 'magnitude' or 'moving', got {kind!r}")
    check(load().ofc_flow_weights_dev(device, C.c_void_p(flow_ptr), n, kinds[kind], float(thr), C.c_void_p(w_ptr)))
