"""numpy-level access to the visualisation / grid / batched k-means entry points of libofc."""
import ctypes as C

import numpy as np

from ._lib import DeviceBuffer, check, load, ptr


def bgr2gray(bgr, device=0):
    bgr = np.ascontiguousarray(bgr, np.uint8)
    H, W = bgr.shape[:2]
    out = np.empty((H, W), np.uint8)
    check(load().ofc_bgr2gray(device, ptr(bgr), W, H, ptr(out)))
    return out


def flow_to_bgr(flow, device=0):
    """computeOpticalFlowModule.py:25-33 -> (BGR uint8 HxWx3, np.mean(magnitude))"""
    flow = np.ascontiguousarray(flow, np.float32)
    H, W = flow.shape[:2]
    out = np.empty((H, W, 3), np.uint8)
    mm = C.c_float()
    check(load().ofc_flow_to_bgr(device, ptr(flow), W, H, ptr(out), C.byref(mm)))
    return out, mm.value


def flow_to_bgr_frames(flows, want_mean=True, device=0):
    """flow_to_bgr on n device-resident frames in one call (each frame normalised by its own min/max):
    (n, H, W, 2) f32 -> ((n, H, W, 3) u8, np.mean(magnitude) per frame (n,) f32, or None if not asked for)"""
    flows = np.ascontiguousarray(flows, np.float32)
    n, H, W = flows.shape[:3]
    src, dst = DeviceBuffer(flows.nbytes, device).upload(flows), DeviceBuffer(n * H * W * 3, device)
    mean = DeviceBuffer(4 * n, device) if want_mean else None
    try:
        check(load().ofc_flow_to_bgr_dev(device, src.ptr, W, H, n, dst.ptr, mean.ptr if mean else None))
        return dst.download((n, H, W, 3), np.uint8), mean.download(n, np.float32) if mean else None
    finally:
        for b in (src, dst, mean):
            if b:
                b.free()


def bgr2hsv(bgr, device=0):
    """cv2.cvtColor(BGR2HSV) on (..., 3) u8, H in [0, 180)"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    out = np.empty_like(bgr)
    check(load().ofc_bgr2hsv(device, ptr(bgr), bgr.size // 3, ptr(out)))
    return out


def preprocess_rgba(img3, thresh=30, device=0):
    """preprocess_image (KmeanGrids.py:269-286) on (..., 3) u8 -> (..., 4) u8"""
    img3 = np.ascontiguousarray(img3, np.uint8)
    out = np.empty(img3.shape[:-1] + (4,), np.uint8)
    check(load().ofc_preprocess_rgba(device, ptr(img3), img3.size // 3, thresh, ptr(out)))
    return out


def grid_cell_means(bgr, rows=14, cols=25, device=0):
    bgr = np.ascontiguousarray(bgr, np.uint8)
    H, W = bgr.shape[:2]
    mean = np.empty((rows * cols, 3), np.uint8)
    hsv = np.empty((rows * cols, 3), np.uint8)
    check(load().ofc_grid_cell_means(device, ptr(bgr), W, H, rows, cols, ptr(mean), ptr(hsv)))
    return mean, hsv


def grid_label_counts(labels, k, rows=14, cols=25, flow=None, device=0):
    """per frame, grid cell and cluster: how many of the cell's pixels carry the label, and with `flow` the sums of their
    (u, v) (ofc_grid_label_counts_dev; the grid is overlayGridAndComputeAvgColor's, remainder pixels belong to no cell;
    labels >= k are counted nowhere).  labels (n, H, W) or (H, W) u8, flow (n, H, W, 2) or (H, W, 2) f32
    -> counts (n, rows*cols, k) int32, or (counts, sums (n, rows*cols, k, 2) f64) when a flow is given"""
    labels = np.ascontiguousarray(labels, np.uint8)
    if labels.ndim == 2:
        labels = labels[None]
    if labels.ndim != 3:
        raise ValueError(f"labels must be (n, H, W) or (H, W), got shape {labels.shape}")
    n, H, W = labels.shape
    if flow is not None:
        flow = np.ascontiguousarray(flow, np.float32)
        if flow.ndim == 3:
            flow = flow[None]
        if flow.shape != (n, H, W, 2):
            raise ValueError(f"flow must be {(n, H, W, 2)} to go with the labels, got {flow.shape}")
    k, rows, cols = int(k), int(rows), int(cols)
    nout = max(n * rows * cols * k, 1)                # the library refuses a bad k / rows / cols; nothing is read back then
    bufs = [DeviceBuffer(max(labels.nbytes, 1), device).upload(labels), DeviceBuffer(nout * 4, device)]
    try:
        if flow is not None:
            bufs += [DeviceBuffer(max(flow.nbytes, 1), device).upload(flow), DeviceBuffer(nout * 16, device)]
        check(load().ofc_grid_label_counts_dev(device, bufs[0].ptr, bufs[2].ptr if flow is not None else None, W, H, n,
                                               rows, cols, k, bufs[1].ptr, bufs[3].ptr if flow is not None else None))
        counts = bufs[1].download((n, rows * cols, k), np.int32)
        return counts if flow is None else (counts, bufs[3].download((n, rows * cols, k, 2), np.float64))
    finally:
        for b in bufs:
            b.free()


def _model_args(centers, mean):
    """(k, mean (2,) f64, centred centres (k,2) f64) as ofc_lloyd_step_dev and the fused grid kernel take a model"""
    cen = np.ascontiguousarray(centers, np.float64)
    if cen.ndim != 2 or cen.shape[1] != 2 or len(cen) < 1:
        raise ValueError(f"centers should be a (k,2) array, got shape {cen.shape}")
    mean = np.zeros(2) if mean is None else np.ascontiguousarray(mean, np.float64)
    if mean.shape != (2,):
        raise ValueError(f"mean should be 2 values, got shape {mean.shape}")
    return len(cen), mean, np.ascontiguousarray(cen - mean)


def grid_assign_counts(flow, centers, rows=14, cols=25, mean=None, sums=False, device=0):
    """grid_label_counts of the labels a model gives the field, in one sweep and without the labels
    (ofc_grid_assign_counts_dev): every (u, v) gets the label ofc_lloyd_step_dev's E-step gives it against `centers`
    ((k,2), un-centred) with the arithmetic centred by `mean` (None = (0, 0): KMeans.predict's un-centred E-step;
    ClipPipeline.assign centres by the field's own mean, and the two agree except where a pixel's two nearest centres
    tie to the rounding of the expanded form |c|^2 - 2 x.c), and is counted in its grid cell.
    flow (n, H, W, 2) or (H, W, 2) f32 -> counts (n, rows*cols, k) int32, or with sums=True (counts, sums
    (n, rows*cols, k, 2) f64 of the (u, v) counted)"""
    flow = np.ascontiguousarray(flow, np.float32)
    if flow.ndim == 3:
        flow = flow[None]
    if flow.ndim != 4 or flow.shape[3] != 2:
        raise ValueError(f"flow must be (n, H, W, 2) or (H, W, 2), got shape {flow.shape}")
    n, H, W = flow.shape[:3]
    k, mean, cen_c = _model_args(centers, mean)
    rows, cols = int(rows), int(cols)
    nout = max(n * rows * cols * k, 1)                # the library refuses a bad k / rows / cols; nothing is read back then
    bufs = [DeviceBuffer(max(flow.nbytes, 1), device).upload(flow), DeviceBuffer(nout * 4, device)]
    try:
        if sums:
            bufs.append(DeviceBuffer(nout * 16, device))
        check(load().ofc_grid_assign_counts_dev(device, bufs[0].ptr, W, H, n, rows, cols, k, ptr(mean), ptr(cen_c),
                                                bufs[1].ptr, bufs[2].ptr if sums else None))
        counts = bufs[1].download((n, rows * cols, k), np.int32)
        return (counts, bufs[2].download((n, rows * cols, k, 2), np.float64)) if sums else counts
    finally:
        for b in bufs:
            b.free()


def kmeans_fit_batched(X, offsets, k, init=None, max_iter=300, tol=1e-4, device=0):
    """many independent u8 RGBA problems in one launch.
    -> centers (P,k,4) f64, counts (P,k) = bincount(predict), labels (total,), n_iter (P,)"""
    X = np.ascontiguousarray(X, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.int64)
    P = len(offsets) - 1
    if X.ndim != 2 or X.shape[1] != 4:
        raise ValueError("X must be (total, 4) uint8")
    if init is not None:
        init = np.ascontiguousarray(init, np.float64)
        if init.shape != (P, k, 4):
            raise ValueError(f"init must be ({P}, {k}, 4)")
    centers = np.empty((P, k, 4), np.float64)
    counts = np.empty((P, k), np.int32)
    labels = np.empty(len(X), np.int32)
    n_iter = np.empty(P, np.int32)
    check(load().ofc_kmeans_fit_batched(device, ptr(X), ptr(offsets), P, 4, k, ptr(init), max_iter, tol,
                                        ptr(centers), ptr(counts), ptr(labels), ptr(n_iter)))
    return centers, counts, labels, n_iter


def grid_kmeans(bgr, k=1, rows=14, cols=25, init=None, max_iter=300, tol=1e-4, channel_order=0, device=0):
    """KmeanGrids.py:376-392 for one frame: -> (rint'ed dominant centre (cells,4) f64, hsv (cells,3) u8)"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    H, W = bgr.shape[:2]
    nc = rows * cols
    if init is not None:
        init = np.ascontiguousarray(init, np.float64)
        if init.shape != (nc, k, 4):
            raise ValueError(f"init must be ({nc}, {k}, 4)")
    centers = np.empty((nc, 4), np.float64)
    hsv = np.empty((nc, 3), np.uint8)
    check(load().ofc_grid_kmeans(device, ptr(bgr), W, H, rows, cols, k, ptr(init), max_iter, tol, channel_order,
                                 ptr(centers), ptr(hsv)))
    return centers, hsv


def grid_kmeans_frames(frames, k=1, rows=14, cols=25, init=None, max_iter=300, tol=1e-4, channel_order=0, device=0):
    """grid_kmeans on n device-resident frames in one launch: (n, H, W, 3) u8 -> ((n, cells, 4) f64, (n, cells, 3) u8)"""
    frames = np.ascontiguousarray(frames, np.uint8)
    n, H, W = frames.shape[:3]
    nc = rows * cols
    if init is not None:
        init = np.ascontiguousarray(init, np.float64)
        if init.shape != (n, nc, k, 4):
            raise ValueError(f"init must be ({n}, {nc}, {k}, 4)")
    centers = np.empty((n, nc, 4), np.float64)
    hsv = np.empty((n, nc, 3), np.uint8)
    src = DeviceBuffer(frames.nbytes, device).upload(frames)
    try:
        check(load().ofc_grid_kmeans_dev(device, src.ptr, W, H, n, rows, cols, k, ptr(init), max_iter, tol,
                                         channel_order, ptr(centers), ptr(hsv)))
    finally:
        src.free()
    return centers, hsv
