"""ctypes binding of libofc.so (include/ofc.h).  Thin: numpy arrays in, numpy arrays out, error codes
turned into Python exceptions.  There is no CPU fallback -- if the shared library is missing or no
gfx950 device is present the calls raise."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libofc.so")

OFC_OK, OFC_EINVAL, OFC_ENODEV, OFC_EHIP, OFC_ENOMEM, OFC_ENOTREADY, OFC_EUNSUPPORTED, OFC_ECOMM = \
    0, -1, -2, -3, -4, -5, -6, -7
U8, F32, F64 = 0, 1, 2
UNIQUE_ID_BYTES = 128
KPP_CHUNK = 1024          # OFC_KPP_CHUNK: samples per partial sum of the seeding's two-level cumulative sum
UV_HIST_SHARE = 2048      # OFC_UV_HIST_SHARE: consecutive vectors a work-group of the histogram kernel takes at a time
UV_HIST_MAX_GRID = 2048   # OFC_UV_HIST_MAX_GRID: most work-groups of one histogram launch
BLOB_TILE_W, BLOB_TILE_H, BLOB_FIELDS = 64, 16, 12   # OFC_BLOB_TILE_W, OFC_BLOB_TILE_H, OFC_BLOB_FIELDS
BLOB_LINK_FIELDS, BLOB_NO_MOVE = 3, -0x7fff8000      # OFC_BLOB_LINK_FIELDS; OFC_BLOB_NO_MOVE (0x80008000) as an int32
CONSIST_OK, CONSIST_MISMATCH, CONSIST_LEAVES, CONSIST_INVALID, CONSIST_STATES = 0, 1, 2, 3, 4   # OFC_CONSIST_*
CONSIST_SHARE, CONSIST_MAX_DIM = 2048, 16384         # OFC_CONSIST_SHARE, OFC_CONSIST_MAX_DIM
CONSIST_ALPHA_MAX, CONSIST_BETA_MAX = 65536, 1 << 62  # OFC_CONSIST_ALPHA_MAX, OFC_CONSIST_BETA_MAX
PHOTO_SHARE, PHOTO_TAU_MAX, PHOTO_KAPPA_MAX, PHOTO_NSTAT = 2048, 65280, 1024, 5      # OFC_PHOTO_*
REPAIR_ROUNDS_MAX, REPAIR_NCOUNT, REPAIR_UNFILLED = 254, 3, 255                      # OFC_REPAIR_*
TRAJ_RAN, TRAJ_UNTRUSTED, TRAJ_LEAVES, TRAJ_INVALID = 0, 1, 2, 3                     # OFC_TRAJ_*: why a point ended
TRAJ_THREADS, TRAJ_MAX_POINTS = 256, 1 << 28                                         # OFC_TRAJ_THREADS, OFC_TRAJ_MAX_POINTS
TRAJ_ONE_LAUNCH_POINTS, TRAJ_DENSE_PAIRS = 1 << 19, 16                               # the launch model's two constants
TRAJ_FULL = 4                                                                        # OFC_TRAJ_FULL: a tracklet that took max_len steps
TRACKLET_THREADS, TRACKLET_MAX_LEN, TRACKLET_MAX_TRACKS = 256, 4096, 1 << 28         # OFC_TRACKLET_*


class OfcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libofc error {code}: {msg}")
        self.code = code


class FbParams(C.Structure):
    """ofc_fb_params; defaults = cv2.calcOpticalFlowFarneback(..., 0.5, 3, 15, 3, 5, 1.2, 0)
    as called at computeOpticalFlowModule.py:20-22"""
    _fields_ = [("pyr_scale", C.c_double), ("levels", C.c_int), ("winsize", C.c_int),
                ("iterations", C.c_int), ("poly_n", C.c_int), ("poly_sigma", C.c_double),
                ("flags", C.c_int)]

    def __init__(self, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2,
                 flags=0):
        super().__init__(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)


_lib = None

_vp, _i, _i64, _f, _d, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t
_ip = C.POINTER(C.c_int)
_PROTOS = {
    "ofc_version": ([], _i),
    "ofc_last_error": ([], C.c_char_p),
    "ofc_device_count": ([_ip], _i),
    "ofc_malloc": ([_i, _sz, C.POINTER(_vp)], _i),
    "ofc_free": ([_i, _vp], _i),
    "ofc_memcpy_h2d": ([_i, _vp, _vp, _sz], _i),
    "ofc_memcpy_d2h": ([_i, _vp, _vp, _sz], _i),
    "ofc_memset": ([_i, _vp, _i, _sz], _i),
    "ofc_device_sync": ([_i], _i),
    "ofc_fb_default_params": ([C.POINTER(FbParams)], None),
    "ofc_flow_create": ([_i, _i, _i, C.POINTER(FbParams), _i, C.POINTER(_vp)], _i),
    "ofc_flow_destroy": ([_vp], None),
    "ofc_flow_calc": ([_vp, _vp, _vp, _vp], _i),
    "ofc_flow_calc_frames_dev": ([_vp, _vp, _i, _vp], _i),
    "ofc_flow_calc_frames_dev_stats": ([_vp, _vp, _i, _vp, _vp], _i),
    "ofc_flow_calc_frames_dev_bidir": ([_vp, _vp, _i, _vp, _vp], _i),
    "ofc_flow_calc_frames_dev_bidir_stats": ([_vp, _vp, _i, _vp, _vp, _vp], _i),
    "ofc_flow_sync": ([_vp], _i),
    "ofc_flow_front_overlap": ([_vp, _ip], _i),
    "ofc_flow_pyramid_fused": ([_vp, _ip], _i),
    "ofc_flow_push_gray": ([_vp, _vp, _vp], _i),
    "ofc_flow_push_bgr": ([_vp, _vp, _vp, C.POINTER(_f), _vp], _i),
    "ofc_flow_last_vis_dev": ([_vp, C.POINTER(_vp)], _i),
    "ofc_level_image": ([_i, _vp, _i, _i, C.POINTER(FbParams), _i, _vp, _ip, _ip], _i),
    "ofc_polyexp": ([_i, _vp, _i, _i, _i, _d, _vp], _i),
    "ofc_polyexp_u8": ([_i, _vp, _i, _i, _i, _d, _vp], _i),
    "ofc_update_matrices": ([_i, _vp, _vp, _vp, _i, _i, _vp], _i),
    "ofc_box_solve": ([_i, _vp, _i, _i, _i, _vp], _i),
    "ofc_flow_resize": ([_i, _vp, _i, _i, _i, _i, _f, _vp], _i),
    "ofc_flow_iterate": ([_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "ofc_flow_launch_geometry": ([_i, _i, _i, _i, _ip], _i),
    "ofc_flow_launch_geometry_bidir": ([_i, _i, _i, _i, _ip], _i),
    "ofc_bench_flow_bidir": ([_i, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_pyramid_dec": ([_i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _ip], _i),
    "ofc_pyramid_dec_geometry": ([_i, _i, _i, _ip], _i),
    "ofc_bench_pyramid_dec": ([_i, _i, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_bench_flow_iters": ([_i, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_bench_polyexp": ([_i, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_bgr2gray": ([_i, _vp, _i, _i, _vp], _i),
    "ofc_flow_to_bgr": ([_i, _vp, _i, _i, _vp, C.POINTER(_f)], _i),
    "ofc_flow_to_bgr_dev": ([_i, _vp, _i, _i, _i, _vp, _vp], _i),
    "ofc_bgr2hsv": ([_i, _vp, _i64, _vp], _i),
    "ofc_preprocess_rgba": ([_i, _vp, _i64, _i, _vp], _i),
    "ofc_grid_cell_means": ([_i, _vp, _i, _i, _i, _i, _vp, _vp], _i),
    "ofc_kmeans_fit": ([_i, _vp, _i, _i64, _i, _i, _vp, _i, _d, _vp, _vp, C.POINTER(_d), _ip], _i),
    "ofc_kmeans_predict": ([_i, _vp, _i, _i64, _i, _i, _vp, _vp], _i),
    "ofc_kmeans_fit_dev": ([_i, _vp, _i, _i64, _i, _i, _vp, _i, _d, _vp, _vp, C.POINTER(_d), _ip], _i),
    "ofc_kmeans_fit_dev_stats": ([_i, _vp, _i, _i64, _i, _i, _vp, _i, _d, _vp, _vp, _vp, C.POINTER(_d), _ip], _i),
    "ofc_kmeans_fit_dev_field": ([_i, _vp, _i, _i64, _i, _i, _vp, _i, _d, _vp, _vp, _vp, C.POINTER(_d), _ip, _i, _i, _i64], _i),
    "ofc_lloyd_field_origin": ([_i64, _i, _i], _i64),
    "ofc_lloyd_field_origins": ([_i64, _i64, _i, _vp], _i),
    "ofc_lloyd_field_shape": ([_ip, _ip, _ip, _ip], None),
    "ofc_lloyd_prune_stats": ([_i, _vp], _i),
    "ofc_bench_lloyd_sweep": ([_i, _vp, _i64, _i, _vp, _vp, _i, _i, C.POINTER(_f)], _i),
    "ofc_lloyd_colstats_dev": ([_i, _vp, _i, _i64, _i, _vp, _i, _vp], _i),
    "ofc_lloyd_step_dev": ([_i, _vp, _i, _i64, _i, _i, _vp, _vp, _vp, _i, _vp], _i),
    "ofc_lloyd_inertia_dev": ([_i, _vp, _i, _i64, _i, _i, _vp, _vp, _vp, C.POINTER(_d)], _i),
    "ofc_lloyd_farthest_dev": ([_i, _vp, _i, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(_d), C.POINTER(_i64), _vp, _ip], _i),
    "ofc_kmeans_fit_w": ([_i, _vp, _i, _vp, _i, _i64, _i, _i, _vp, _i, _d, _vp, _vp, C.POINTER(_d), _ip], _i),
    "ofc_kmeans_fit_dev_w": ([_i, _vp, _i, _vp, _i, _i64, _i, _i, _vp, _i, _d, _vp, _vp, _vp, C.POINTER(_d), _ip], _i),
    "ofc_kmeans_score": ([_i, _vp, _i, _vp, _i, _i64, _i, _i, _vp, C.POINTER(_d)], _i),
    "ofc_lloyd_step_dev_w": ([_i, _vp, _i, _vp, _i, _i64, _i, _i, _vp, _vp, _vp, _vp], _i),
    "ofc_lloyd_inertia_dev_w": ([_i, _vp, _i, _vp, _i, _i64, _i, _i, _vp, _vp, _vp, C.POINTER(_d)], _i),
    "ofc_lloyd_farthest_dev_w": ([_i, _vp, _i, _vp, _i, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(_d), C.POINTER(_i64), _vp, _ip,
                                  C.POINTER(_d)], _i),
    "ofc_flow_weights_dev": ([_i, _vp, _i64, _i, _f, _vp], _i),
    "ofc_bench_lloyd_sweep_w": ([_i, _vp, _vp, _i, _i64, _i, _vp, _vp, _i, C.POINTER(_f)], _i),
    "ofc_kpp_candidates": ([_i, _vp, _i, _i64, _i, _vp, _vp, _i, _vp, _vp, _vp], _i),
    "ofc_kpp_seed_dev": ([_i, _vp, _i, _i64, _i, _i, _vp, _i64, _vp, _i, _vp, _vp], _i),
    "ofc_kpp_sample_dev": ([_i, _vp, _i64, _vp, _i, _vp], _i),
    "ofc_kpp_seed_dev_w": ([_i, _vp, _i, _vp, _i, _i64, _i, _i, _vp, _d, _vp, _i, _vp, _vp], _i),
    "ofc_kpp_sample_dev_w": ([_i, _vp, _i, _vp, _i64, _vp, _i, _i, _vp, _vp], _i),
    "ofc_kmeans_fit_batched": ([_i, _vp, _vp, _i, _i, _i, _vp, _i, _d, _vp, _vp, _vp, _vp], _i),
    "ofc_grid_kmeans": ([_i, _vp, _i, _i, _i, _i, _i, _vp, _i, _d, _i, _vp, _vp], _i),
    "ofc_grid_kmeans_dev": ([_i, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _d, _i, _vp, _vp], _i),
    "ofc_dist_unique_id": ([_vp], _i),
    "ofc_dist_init": ([_i, _i, _i, _vp], _i),
    "ofc_dist_allreduce_f64": ([_i, _vp, _i], _i),
    "ofc_dist_init_host": ([_i, _i, _i, _vp, _vp], _i),
    "ofc_dist_loopback": ([_i], _i),
    "ofc_dist_finalize": ([], _i),
    "ofc_stream_create": ([_i, _i, _i, C.POINTER(FbParams), _i, _i, _i, C.POINTER(_vp)], _i),
    "ofc_stream_push_gray": ([_vp, _vp, _ip], _i),
    "ofc_stream_finish": ([_vp, _vp, _i, _ip], _i),
    "ofc_stream_set_model": ([_vp, _i, _vp, _vp, _i], _i),
    "ofc_stream_finish_clusters": ([_vp, _vp, _vp, _vp, _i, _ip], _i),
    "ofc_stream_set_histogram": ([_vp, _i, _f], _i),
    "ofc_stream_read_histogram": ([_vp, _vp, _i], _i),
    "ofc_stream_destroy": ([_vp], None),
    "ofc_grid_cell_mean_flow": ([_i, _vp, _i, _i, _i, _i, _vp], _i),
    "ofc_grid_label_counts_dev": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "ofc_grid_assign_counts_dev": ([_i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "ofc_uv_hist_accum_dev": ([_i, _vp, _i64, _i, _f, _vp], _i),
    "ofc_uv_hist": ([_i, _vp, _i64, _i, _f, _vp], _i),
    "ofc_bench_uv_hist": ([_i, _vp, _i64, _i, _f, _i, C.POINTER(_f)], _i),
    "ofc_motion_check": ([_i, _i, _i], _i),
    "ofc_motion_launch_geometry": ([_i, _i, _i, _ip], _i),
    "ofc_motion_solve": ([_vp, _i, _vp, _ip], _i),
    "ofc_motion_moments_dev": ([_i, _vp, _i, _i, _i, _vp, _vp, _vp], _i),
    "ofc_motion_fit_dev": ([_i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp], _i),
    "ofc_motion_subtract_dev": ([_i, _vp, _i, _i, _i, _vp, _vp], _i),
    "ofc_motion_fit": ([_i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp], _i),
    "ofc_motion_compensate": ([_i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "ofc_stream_set_camera": ([_vp, _i, _vp, _i], _i),
    "ofc_stream_read_camera": ([_vp, _vp, _vp, _i], _i),
    "ofc_bench_motion": ([_i, _vp, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_blob_check": ([_i, _i, _i, _i, _i, _i], _i),
    "ofc_blob_keys_dev": ([_i, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp, C.c_uint32, _i, _vp], _i),
    "ofc_blob_label_dev": ([_i, _vp, _i, _i, _i, _i, _vp], _i),
    "ofc_blob_table_dev": ([_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "ofc_blob_table_read": ([_i, _vp, _vp, _i, _i, _vp, _vp, _vp], _i),
    "ofc_blobs": ([_i, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp, C.c_uint32, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "ofc_stream_set_blobs": ([_vp, _i, _f, _i, _i], _i),
    "ofc_stream_read_blobs": ([_vp, _vp, _vp, _vp, _i], _i),
    "ofc_bench_blobs": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_blob_link_check": ([_i, _i, _i, _i, _i], _i),
    "ofc_blob_links_bytes": ([_i, _i], _sz),
    "ofc_blob_moves_dev": ([_i, _vp, _i, _i, _i, _vp], _i),
    "ofc_blob_links_dev": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "ofc_blob_links_read": ([_i, _vp, _vp, _i, _i, _vp, _vp], _i),
    "ofc_blob_links": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "ofc_stream_set_blob_links": ([_vp, _i], _i),
    "ofc_stream_read_blob_links": ([_vp, _vp, _vp, _i], _i),
    "ofc_bench_blob_links": ([_i, _vp, _vp, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_consist_check": ([_i, _i, _i, _i64, _i64], _i),
    "ofc_consist_dev": ([_i, _vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _vp, _vp], _i),
    "ofc_consist": ([_i, _vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _vp, _vp], _i),
    "ofc_consist_mask_dev": ([_i, _vp, _i64, _i, _vp, _vp], _i),
    "ofc_frames_reverse_dev": ([_i, _vp, _i, _i, _i, _vp], _i),
    "ofc_bench_consist": ([_i, _vp, _vp, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_photo_check": ([_i, _i, _i, _i, _i], _i),
    "ofc_photo_dev": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "ofc_photo": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "ofc_bench_photo": ([_i, _vp, _vp, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_stream_set_photo": ([_vp, _i, _i, _i, _i], _i),
    "ofc_stream_read_photo": ([_vp, _vp, _i], _i),
    "ofc_stream_set_consist": ([_vp, _i, _i64, _i64, _i], _i),
    "ofc_stream_read_consist": ([_vp, _vp, _i], _i),
    "ofc_repair_check": ([_i, _i, _i, _i, _i, _i, _i, _i], _i),
    "ofc_repair_tile": ([_i, C.POINTER(_i * 2)], None),
    "ofc_repair_dev": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "ofc_repair": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "ofc_bench_repair": ([_i, _vp, _vp, _i, _i, _i, _i, _i, C.POINTER(_f)], _i),
    "ofc_stream_set_repair": ([_vp, _i, _i, _i, _i, _i, _i], _i),
    "ofc_stream_read_repair": ([_vp, _vp, _i], _i),
    "ofc_traj_check": ([_i, _i, _i, _i64, _i, _i], _i),
    "ofc_traj_launch_geometry": ([_i, _i, _i, _i64, C.POINTER(_i * 4)], _i),
    "ofc_traj_dev": ([_i, _vp, _vp, _i, _i, _i, _vp, _i64, _i, _i, _vp, _vp, _vp], _i),
    "ofc_traj": ([_i, _vp, _vp, _i, _i, _i, _vp, _i64, _i, _i, _vp, _vp, _vp], _i),
    "ofc_bench_traj": ([_i, _vp, _i, _i, _i, _vp, _i64, _i, _i, C.POINTER(_f)], _i),
    "ofc_stream_set_traj": ([_vp, _i64, _vp, _i], _i),
    "ofc_stream_read_traj": ([_vp, _vp, _vp, _vp, _i], _i),
    "ofc_tracklets_check": ([_i, _i, _i, _i, _i, _i64, _i], _i),
    "ofc_tracklets_dev": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "ofc_tracklets": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "ofc_bench_tracklets": ([_i, _vp, _i, _i, _i, _i, _i, _i64, _i, C.POINTER(_f)], _i),
    "ofc_sliding_cosine": ([_i, _vp, _i, _vp, _i, _vp], _i),
    "ofc_synth_frames_dev": ([_i, _vp, _i, _i, _i, _i, _i], _i),
}
EXPORTS = tuple(_PROTOS)


def load():
    """dlopen libofc.so (built in-tree by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OfcError(OFC_ENODEV, f"{LIB_PATH} not built: run `make -C {_HERE}/csrc` "
                                       "(python -c 'import __graft_entry__ as g; g.build()')")
        lib = C.CDLL(LIB_PATH)
        for name, (args, res) in _PROTOS.items():
            fn = getattr(lib, name)          # AttributeError = missing export: fail loudly
            fn.argtypes = args
            fn.restype = res
        _lib = lib
    return _lib


def check(rc):
    if rc != OFC_OK:
        msg = load().ofc_last_error().decode("utf-8", "replace")
        if rc == OFC_EINVAL:
            raise ValueError(msg)
        raise OfcError(rc, msg)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def device_count():
    n = C.c_int()
    check(load().ofc_device_count(C.byref(n)))
    return n.value


class DeviceBuffer:
    """a hipMalloc'ed buffer owned through the C ABI (inputs stay resident in HBM between calls)"""

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        check(load().ofc_malloc(device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        check(load().ofc_memcpy_h2d(self.device, self.ptr + offset, ptr(arr), arr.nbytes))
        return self

    def download(self, shape, dtype, offset=0):
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= self.nbytes
        check(load().ofc_memcpy_d2h(self.device, ptr(out), self.ptr + offset, out.nbytes))
        return out

    def zero(self):
        check(load().ofc_memset(self.device, self.ptr, 0, self.nbytes))

    def free(self):
        if self.ptr:
            load().ofc_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
