/*
 * ofc.h -- C ABI of libofc.so: the MI355X (gfx950) implementation of the dense-Farneback-flow ->
 * k-means hot path of menmitsu/opticalFlowClustering.
 *
 * The reference has no FFI of its own for this path: it reaches the arithmetic through the Python
 * call signatures of cv2 and scikit-learn.  Each entry point below names the reference call it
 * stands in for (file:line relative to k-means-color-clustering/ in the reference).  The Python
 * host side (opticalflowclustering_amd/) binds these with ctypes and re-exposes the reference's
 * own class / function / CLI names on top.
 *
 * Conventions
 *   - plain C types only; all buffers C-contiguous; images are row-major, stride == width.
 *   - "host" pointers are ordinary process memory; "_dev" entry points take device pointers
 *     obtained from ofc_malloc (or any hipMalloc'ed memory of the same device).
 *   - every call returns 0 on success or a negative OFC_E* code; ofc_last_error() gives the
 *     message for the calling host thread.  No C++ exception crosses the ABI.
 *   - handles are not thread-safe; use one per (host thread, GPU).
 *   - there is NO CPU fallback: without a usable gfx950 device every compute call fails with
 *     OFC_ENODEV.
 */
#ifndef OFC_H
#define OFC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFC_VERSION 100 /* 0.1.0 */

enum {
    OFC_OK = 0,
    OFC_EINVAL = -1,   /* bad argument (maps to Python ValueError) */
    OFC_ENODEV = -2,   /* no usable GPU / HIP runtime error at init */
    OFC_EHIP = -3,     /* HIP runtime error during the call */
    OFC_ENOMEM = -4,   /* device allocation failed */
    OFC_ENOTREADY = -5,/* streaming flow: first frame pushed, no pair yet */
    OFC_EUNSUPPORTED = -6, /* parameter combination outside what the kernels implement */
    OFC_ECOMM = -7     /* RCCL error */
};

enum { OFC_U8 = 0, OFC_F32 = 1, OFC_F64 = 2 };

int ofc_version(void);
const char *ofc_last_error(void);
int ofc_device_count(int *n);

/* ---- device memory plumbing (so a host without torch can keep inputs resident in HBM) ---- */
int ofc_malloc(int device, size_t bytes, void **dptr);
int ofc_free(int device, void *dptr);
int ofc_memcpy_h2d(int device, void *dst_dev, const void *src_host, size_t bytes);
int ofc_memcpy_d2h(int device, void *dst_host, const void *src_dev, size_t bytes);
int ofc_memset(int device, void *dst_dev, int value, size_t bytes);
int ofc_device_sync(int device);

/* ------------------------------------------------------------------------------------------
 * Dense Farneback flow.
 * Replaces cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 3, 15, 3, 5, 1.2, 0)
 * (computeOpticalFlowModule.py:20-22, computeOpticalFlow.py:99-101).
 * ------------------------------------------------------------------------------------------ */
/* The accepted domain, all of it checked by ofc_flow_create (and so by ofc_stream_create and the Python front ends) before
 * anything is allocated: frames 16 .. 16384 pixels a side; pyr_scale in (0, 1); levels 0 .. 16; iterations 1 .. 64; winsize
 * odd, 5 .. OFC_WINSIZE_MAX; poly_n 5 or 7; flags 0; max_batch 1 .. 4096 (violations OFC_EINVAL, except where noted below).
 * Two limits depend on the frame size as well, and are refused with OFC_EUNSUPPORTED and a message naming the level:
 *  - the blur of a pyramid level has at most 31 taps.  Level k is blurred with sigma = (pyr_scale^-k - 1) / 2 over
 *    cvRound(5 sigma) | 1 taps, so a level may shrink the frame by less than 13.6x: levels <= 3 at pyr_scale 0.5, <= 1 at
 *    0.25, <= 2 at 0.3, <= 7 at 0.7, <= 11 at 0.8, any (<= 16) from 0.85 up; in general levels <= log(13.6) / log(1 / pyr_scale).
 *    Only levels that are built count: cv2's rule drops a level once min(W, H) * pyr_scale^k < 32, so pyr_scale 0.5 with
 *    levels 4 is accepted below 512 pixels a side (where it runs 3 levels or fewer) and refused from 512 x 512 on.
 *  - with winsize <= 15 (the fused iteration), W * H * 5 < 2^30, i.e. up to about 14654 x 14654. */
typedef struct ofc_fb_params {
    double pyr_scale;  /* 0.5 */
    int levels;        /* 3   */
    int winsize;       /* 15  (odd, 5 .. OFC_WINSIZE_MAX; even OFC_EINVAL, wider OFC_EUNSUPPORTED) */
    int iterations;    /* 3   */
    int poly_n;        /* 5   (5 or 7: the two sizes cv2 documents; others OFC_EUNSUPPORTED) */
    double poly_sigma; /* 1.2 */
    int flags;         /* 0   */
} ofc_fb_params;
#define OFC_WINSIZE_MAX 255 /* widest Farneback window the engine implements */

void ofc_fb_default_params(ofc_fb_params *p);

typedef struct ofc_flow ofc_flow_t;

/* one engine per (device, resolution).  max_batch = the largest number of frame PAIRS processed
 * per call of ofc_flow_calc_frames_dev; all scratch (pyramid images, polynomial expansions R,
 * matrices M, per-level flows) is allocated here once. */
int ofc_flow_create(int device, int W, int H, const ofc_fb_params *p, int max_batch,
                    ofc_flow_t **out);
void ofc_flow_destroy(ofc_flow_t *f);

/* one isolated pair, host buffers: prev/next HxW u8 -> flow HxWx2 f32 (u = x-disp, v = y-disp) */
int ofc_flow_calc(ofc_flow_t *f, const uint8_t *prev_gray, const uint8_t *next_gray,
                  float *flow_out);

/* batched, device-resident: n_frames consecutive HxW u8 frames -> (n_frames-1) flows,
 * flow_dev[(t*H + y)*W + x][2] between frame t and t+1.  n_frames-1 <= max_batch.
 * Asynchronous on the engine's stream; ofc_flow_sync() (or ofc_device_sync) completes it. */
int ofc_flow_calc_frames_dev(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames,
                             float *flow_dev);
/* As above, and uv_sum_dev[0..1] (device) receive sum(u), sum(v) over the n_frames-1 flow fields in float64: the column
 * sums the clip-wide k-means needs for sklearn's centring (X.mean(axis=0), _kmeans.py:1478-1484) come out of the
 * epilogue of the iteration that writes the field instead of an extra sweep over it (pass them to
 * ofc_kmeans_fit_dev_stats).  Engines without that epilogue (one iteration per level, another winsize, the staged or
 * experimental kernels) form the same two sums with one sweep over the finished field: the call always succeeds. */
int ofc_flow_calc_frames_dev_stats(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames,
                                   float *flow_dev, double *uv_sum_dev);
/* Both directions of every pair of the batch from ONE front end (level images and polynomial expansions depend on the frame
 * alone) and one launch per iteration: fwd_dev[t] is what ofc_flow_calc_frames_dev defines; bwd_dev[t] is the flow from frame
 * t+1 to frame t on frame t+1's grid, stored at t (NOT reversed: ofc_consist_dev takes the two with bwd_reversed = 0).  Both
 * hold (n_frames-1) fields of HxWx2 f32.  Each field is, bit for bit, what a forward-only engine with max_batch >= 2(n_frames-1)
 * gives for that pair of the palindrome clip f0 .. fn fn-1 .. f0 (pairs t and 2(n_frames-1)-1-t).
 * The two buffers may lie anywhere: the last iteration of level 0 writes through two base pointers; they may not overlap.
 * The first such call of an engine doubles its per-level flow scratch (and M with winsize > 15), which waits for the device
 * once; an engine that never makes the call allocates nothing more.  With OFC_FLOW_GRAPH=1 the call makes plain launches.
 * OFC_EINVAL: a null pointer, n_frames < 2, n_frames-1 > max_batch, overlapping buffers.  Asynchronous like the call above. */
int ofc_flow_calc_frames_dev_bidir(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *fwd_dev, float *bwd_dev);
/* As above, and uv_sum_dev[0..1] receive sum(u), sum(v) over the FORWARD fields (one sweep over the finished field). */
int ofc_flow_calc_frames_dev_bidir_stats(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *fwd_dev,
                                         float *bwd_dev, double *uv_sum_dev);
int ofc_flow_sync(ofc_flow_t *f);
/* *on = 1 when the engine runs the front end of the coarse pyramid levels (level images and polynomial expansions, which
 * depend on the frames only) on a side stream beside the level-0 expansion, 0 when it runs every level in series on one
 * stream.  Either order launches the same kernels with the same arguments: the results are the same bits.  The overlap
 * gives every level its own slices of the I and R scratch, so an engine uses it only when those slices together are at most
 * 1.5 x the level-0 sized buffers of the serial order (pyr_scale 0.5: up to 1.33 x; a deep pyramid at pyr_scale 0.8 stays
 * serial), when the pyramid has a coarse level at all, and when neither OFC_FLOW_FRONT_OVERLAP=0 nor OFC_FLOW_GRAPH=1 was
 * set in the environment when the engine was created.  Everything a call issues is ordered before whatever follows it on
 * the engine's stream: callers synchronise as before. */
int ofc_flow_front_overlap(const ofc_flow_t *f, int *on);
/* *on = 1 when the engine writes the level images of all its coarse levels with one launch per batch (k_pyramid_dec: one
 * march over the u8 frames) instead of one launch per level: with the overlap above on, at most three coarse levels, every one
 * an exact decimation by 2, 4, 8 (pyr_scale 0.5 on frames whose sides divide), and OFC_PYRAMID_FUSED=0 not set in the
 * environment when the engine was created.  The images are the same bits either way. */
int ofc_flow_pyramid_fused(const ofc_flow_t *f, int *on);

/* streaming form of ComputeOpticalFLow (computeOpticalFlowModule.py:6-36): keeps the previous
 * frame; the first push returns OFC_ENOTREADY and writes nothing.
 * An engine keeps ONE previous frame (grey, on the device), shared by ofc_flow_push_gray and ofc_flow_push_bgr: the two may
 * be mixed, each push pairs with the frame the push before it left, whichever form that was.  A push that is refused
 * (NULL flow_out after the first frame: OFC_EINVAL, checked before anything is copied) leaves the kept frame as it was.
 * ofc_flow_calc and ofc_flow_calc_frames_dev[_stats] neither read nor replace it. */
int ofc_flow_push_gray(ofc_flow_t *f, const uint8_t *gray, float *flow_out);

/* ComputeOpticalFLow.compute (computeOpticalFlowModule.py:18-36) in one call: BGR frame (host) ->
 * BGR2GRAY on the device -> flow against the previous frame -> HSV-coded BGR visualisation.  The first
 * push stores the frame and returns OFC_ENOTREADY.  vis_out (HxWx3 u8), mean_mag, flow_out (HxWx2 f32)
 * may each be NULL.  The visualisation also stays resident: ofc_flow_last_vis_dev() gives its device
 * address (HxWx3 u8, valid until the next push or ofc_flow_destroy); OFC_EINVAL until a BGR push has returned OFC_OK. */
int ofc_flow_push_bgr(ofc_flow_t *f, const uint8_t *bgr, uint8_t *vis_out, float *mean_mag,
                      float *flow_out);
int ofc_flow_last_vis_dev(ofc_flow_t *f, const uint8_t **vis_dev);

/* ---- single stages, host buffers (parity-test / bench hooks; interleaved layouts as OpenCV's
 *      internals so they compare 1:1 with the oracle) ---- */
/* u8 frame -> f32 pyramid image of level k (GaussianBlur at full res + INTER_LINEAR resize) */
int ofc_level_image(int device, const uint8_t *gray, int W, int H, const ofc_fb_params *p, int k,
                    float *out, int *w_out, int *h_out);
/* u8 frames [n][H0][W0] -> the f32 images of pyramid levels 1..levels (1..3) at the default pyr_scale 0.5, [n][h][w] each.
 * fused != 0: the leading levels that are exact decimations come from one k_pyramid_dec launch (*fused_levels says how many)
 * and the others from the per-level kernels; fused == 0: every level from the per-level kernels, as ofc_level_image.  The
 * pyramid's minimum level size is not applied: the hook reaches small levels the engine would drop. */
int ofc_pyramid_dec(int device, const uint8_t *frames, int n, int W0, int H0, int levels, int fused,
                    float *out1, float *out2, float *out3, int *fused_levels);
/* out = {bands of 256 input columns, 8-row steps per frame, steps per strip, strips} of a k_pyramid_dec launch over n frames.
 * Host only. */
int ofc_pyramid_dec_geometry(int W0, int H0, int n, int out[4]);
/* bench hook: ms per batch of the level images 1..levels of n_images resident W x H frames, timed with HIP events: fused 1 =
 * one k_pyramid_dec launch (OFC_EUNSUPPORTED where the levels are not all exact decimations), 0 = the per-level launches */
int ofc_bench_pyramid_dec(int device, int W, int H, int n_images, int levels, int fused, int iters, float *ms_per_batch);
/* FarnebackPolyExp: f32 HxW -> f32 HxWx5 {y-lin, x-lin, y^2, x^2, xy}; n (poly_n) 5 or 7, else OFC_EUNSUPPORTED */
int ofc_polyexp(int device, const float *img, int W, int H, int n, double sigma, float *R5);
/* the same for pyramid level 0 straight from the u8 frame (level-0 blur fused in; what ofc_flow_* runs at level 0):
 * must equal ofc_level_image(k=0) followed by ofc_polyexp bit for bit.  n 5 or 7; OFC_EUNSUPPORTED otherwise and when
 * W < 4 or H < 2 */
int ofc_polyexp_u8(int device, const uint8_t *gray, int W, int H, int n, double sigma, float *R5);
/* FarnebackUpdateMatrices: R0,R1 HxWx5, flow HxWx2 -> M HxWx5 */
int ofc_update_matrices(int device, const float *R0, const float *R1, const float *flow, int W,
                        int H, float *M);
/* box mean (winsize) of M + 2x2 solve: M HxWx5 -> flow HxWx2.  winsize odd, 5 .. OFC_WINSIZE_MAX (19 and wider use the
 * window-independent kernel the engine runs for them); others OFC_EUNSUPPORTED */
int ofc_box_solve(int device, const float *M, int W, int H, int winsize, float *flow);
/* resize(flow, (w,h), INTER_LINEAR) * mul */
int ofc_flow_resize(int device, const float *flow, int sw, int sh, int dw, int dh, float mul,
                    float *out);

/* `iters` Farneback iterations (update matrices + box mean + solve, as ofc_update_matrices / ofc_box_solve chained:
 * oracle/farneback_ref.c, the loop of FarnebackUpdateFlow_Blur) from flow_in, with the engine's fused kernels.
 * mode 0: one launch per iteration (k_flow_iter); mode 1: two iterations per launch where possible (k_flow_iter2);
 * mode 2: one launch per iteration with the 3-waves-per-SIMD kernel (k_flow_iter_w3); rows_per_block 0 = automatic
 * strip height.  Every mode honours rows_per_block: mode 0, the kernel the engine runs, rounds it up to a multiple of 16
 * (a value above H is one strip) and refuses a negative one with OFC_EINVAL; modes 1 and 2 round up to a multiple of 2.
 * The result does not depend on the height.  Parity-test hook. */
int ofc_flow_iterate(int device, const float *R0, const float *R1, const float *flow_in, int W, int H,
                     int winsize, int iters, int mode, int rows_per_block, float *flow_out);
/* The strip heights the launches' cost models pick for a W x H pyramid level in a batch of n_pairs pairs (n_pairs + 1
 * images): out[0] rows per work-group of the fused iteration (k_flow_iter; 0 for winsize > 15, which runs staged), out[1]
 * of the staged box mean + solve (k_box_solve; the fixed height of k_box_solve_wide from winsize 19 on), out[2] of the
 * polynomial expansion over the n_pairs + 1 images.  Host only: no device is touched.  OFC_EINVAL: null pointer, W or H
 * or n_pairs < 1, winsize even or outside 5 .. OFC_WINSIZE_MAX.  Test hook: the suite's case tables are checked against
 * these models themselves. */
int ofc_flow_launch_geometry(int W, int H, int n_pairs, int winsize, int out[3]);
/* Its twin for the fused iteration of ofc_flow_calc_frames_dev_bidir over n_pairs frame pairs (2 n_pairs logical pairs):
 * out[0] rows per work-group, out[1] tiles (column tiles x strips) of one logical pair, out[2] work-groups of the launch
 * (tiles rounded up to a multiple of 8, times 2 n_pairs).  Work-group b serves tile 8 (b / (16 n_pairs)) + b % 8 of logical
 * pair q = (b % (16 n_pairs)) / 8: frame pair q >> 1, direction q & 1 (1 = backward).  Host only.  OFC_EINVAL: null pointer,
 * W, H or n_pairs < 1, winsize even or outside 5 .. 15 (wider windows run the staged kernels). */
int ofc_flow_launch_geometry_bidir(int W, int H, int n_pairs, int winsize, int out[3]);
/* bench hook: *ms = average duration, by HIP events on the engine's stream over `reps` runs after two warm-up runs, of both
 * directions of n_frames-1 synthetic pairs with the default parameters.  what 0: one ofc_flow_calc_frames_dev_bidir; what 1:
 * the two-pass route, a forward-only call, the reversal of the frames and a second forward-only call on the same engine.
 * Engine and buffers are allocated before the timed region. */
int ofc_bench_flow_bidir(int device, int W, int H, int n_frames, int reps, int what, float *ms);
/* bench hook: one 1080p-style level of `n_pairs` resident pairs, the last two of the three iterations of a level
 * timed with HIP events on their stream: mode 0 = two single-iteration launches, mode 1 = one two-iteration launch,
 * mode 2 = two launches of the 3-waves-per-SIMD kernel.
 * *ms = average duration of those two iterations per batch. */
int ofc_bench_flow_iters(int device, int W, int H, int n_pairs, int reps, int mode, float *ms);

/* bench hook: time `iters` launches of the polyexp kernel over n_images distinct resident images
 * with HIP events on the kernel's own stream; *ms_per_launch = average launch duration. */
int ofc_bench_polyexp(int device, int W, int H, int n_images, int iters, int rows_per_block,
                      float *ms_per_launch);

/* ------------------------------------------------------------------------------------------
 * Flow visualisation and grid.
 * ------------------------------------------------------------------------------------------ */
/* cvtColor(BGR2GRAY) u8 (computeOpticalFlowModule.py:16,19) */
int ofc_bgr2gray(int device, const uint8_t *bgr, int W, int H, uint8_t *gray);
/* cartToPolar + hue/normalize(MINMAX)/HSV2BGR (computeOpticalFlowModule.py:25-33) and
 * np.mean(magnitude) (computeOpticalFlow.py:114-117): flow HxWx2 f32 -> bgr HxWx3 u8 */
int ofc_flow_to_bgr(int device, const float *flow, int W, int H, uint8_t *bgr, float *mean_mag);
/* the same on n_frames resident fields; at most 65535 frames per call (OFC_EUNSUPPORTED, decided before any launch) */
int ofc_flow_to_bgr_dev(int device, const float *flow_dev, int W, int H, int n_frames,
                        uint8_t *bgr_dev, float *mean_mag_dev);
/* cvtColor(BGR2HSV) u8, H in [0,180) (KmeanGrids.py:86,336; color_kmeans.py:121) */
int ofc_bgr2hsv(int device, const uint8_t *bgr, int64_t npix, uint8_t *hsv);
/* preprocess_image (KmeanGrids.py:269-286, color_kmeans.py:35-52): per channel <thresh -> 0,
 * alpha = 255 where BGR2GRAY > 0; HxWx3 u8 -> HxWx4 u8 (channel order kept as given) */
int ofc_preprocess_rgba(int device, const uint8_t *img3, int64_t npix, int thresh, uint8_t *rgba);
/* overlayGridAndComputeAvgColor (KmeanGrids.py:52-113): per-cell mean BGR -> u8 -> BGR2HSV.
 * mean_bgr, hsv: rows*cols x 3 u8 */
int ofc_grid_cell_means(int device, const uint8_t *bgr, int W, int H, int rows, int cols,
                        uint8_t *mean_bgr, uint8_t *hsv);

/* ------------------------------------------------------------------------------------------
 * Lloyd k-means.  Replaces sklearn.cluster.KMeans(n_clusters=k, init=<k x d>, n_init=1,
 * max_iter, tol).fit(X) / .predict(X) (color_kmeans.py:66-78, KmeanGrids.py:300-304).
 * All arithmetic in f64 whatever the storage dtype (sklearn casts u8 to f64).
 * ------------------------------------------------------------------------------------------ */
/* host buffers. X: N x d of `dtype`; init: k x d f64 (required: explicit init = determinism);
 * centers k x d f64, labels N i32, inertia, n_iter as sklearn's attributes of the same name. */
int ofc_kmeans_fit(int device, const void *X, int dtype, int64_t N, int d, int k,
                   const double *init, int max_iter, double tol_rel, double *centers,
                   int32_t *labels, double *inertia, int *n_iter);
/* KMeans.predict: one E-step of the un-centred X against `centers` */
int ofc_kmeans_predict(int device, const void *X, int dtype, int64_t N, int d, int k,
                       const double *centers, int32_t *labels);
/* device-resident X (e.g. the (u,v) field ofc_flow_calc_frames_dev just wrote); labels_dev is
 * N x u8 (k <= 255) or NULL.  If a communicator was set up with ofc_dist_init the partial sums are
 * all-reduced over the ranks every iteration (X is then this rank's shard). */
int ofc_kmeans_fit_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k,
                       const double *init, int max_iter, double tol_rel, double *centers,
                       uint8_t *labels_dev, double *inertia, int *n_iter);
/* ofc_kmeans_fit_dev with the column sums of THIS RANK'S rows supplied by the caller (host pointer, d doubles; e.g. added
 * up from ofc_flow_calc_frames_dev_stats): the fit skips its own column-sum sweep.  colsum == NULL: as ofc_kmeans_fit_dev. */
int ofc_kmeans_fit_dev_stats(int device, const void *X_dev, int dtype, int64_t N, int d, int k,
                             const double *init, int max_iter, double tol_rel, const double *colsum,
                             double *centers, uint8_t *labels_dev, double *inertia, int *n_iter);
/* ofc_kmeans_fit_dev_stats for a caller that knows what X_dev is: a stack of n_fields flow fields, X_dev[n_fields][H][W][2]
 * float32 (dtype OFC_F32, d = 2, N = n_fields * W * H; anything else: OFC_EINVAL), e.g. the field of
 * computeOpticalFlow.py:99-101 for every frame pair of a clip, or this rank's whole pairs under a communicator.  The result
 * is ofc_kmeans_fit_dev_stats': the geometry only changes how the tile sweeps of ofc_lloyd_prune_stats cut the samples.
 * When W % 64 == 0 and H % 8 == 0 (and k <= 8, OFC_LLOYD_PRUNE != 0) a tile is 16 x 4 pixels instead of a 64 x 1 row
 * segment, and 8 tiles form a 64 x 8-pixel group that is tested first: a motion boundary is a curve in the image, and
 * compact tiles lose a quarter of the samples to it that row segments lose.  Other sizes run the 64 x 1 tiles. */
int ofc_kmeans_fit_dev_field(int device, const void *X_dev, int dtype, int64_t N, int d, int k,
                             const double *init, int max_iter, double tol_rel, const double *colsum,
                             double *centers, uint8_t *labels_dev, double *inertia, int *n_iter,
                             int W, int H, int64_t n_fields);
/* The tile -> sample map of ofc_kmeans_fit_dev_field (host arithmetic, no device needed): the index, into the stack's
 * n_fields * H * W samples, of the first of the 4 consecutive samples that quad `quad` (0..15) of tile `tile` covers, for
 * fields of width W (a multiple of 64; the map does not depend on H, which is a multiple of 8).  Tiles are numbered
 * group-major: tile = 8 * group + (tile row of the group) * (tiles across a group) + (tile column).  -1: bad arguments.
 * ofc_lloyd_field_origins: the same for the 16 quads of each of n_tiles tiles from tile0 on, out[n_tiles][16].
 * ofc_lloyd_field_shape: the tile's and the group's size in pixels. */
int64_t ofc_lloyd_field_origin(int64_t tile, int quad, int W);
int ofc_lloyd_field_origins(int64_t tile0, int64_t n_tiles, int W, int64_t *out);
void ofc_lloyd_field_shape(int *tile_w, int *tile_h, int *group_w, int *group_h);
/* How the last ofc_kmeans_fit_dev[_stats] on `device` swept its samples (no reference counterpart: sklearn's Lloyd,
 * _k_means_lloyd.pyx:23-218, reads every sample in every iteration).  For a float32 d=2 stream (the per-pixel (u,v) vectors
 * of computeOpticalFlow.py:99-101's field) of >= 2^20 samples and k <= 8 the label-less iterations run over 64-sample
 * tiles; a tile whose (u,v) bounding box lies inside one Voronoi cell of the current centres contributes its cached sum
 * without being read, in the iterations and in the final E-step (exact: same labels, same n_iter, centres and inertia equal
 * to rounding).  After ofc_kmeans_fit_dev_field on a field it can cut in 2-D the tiles are 16 x 4 pixels under 64 x 8-pixel
 * groups; the counts stay in tiles (a group that passes counts as 8 tiles tested and 8 skipped).  out6 = [tile sweeps, of them pruned,
 * tiles tested by the pruned sweeps, tiles they skipped, probe sweeps, 1 if the final E-step ran pruned].  Environment: OFC_LLOYD_PRUNE=0 switches
 * the tile sweeps off, 2 enables them for any N, 3 also forces every one of them to run pruned. */
int ofc_lloyd_prune_stats(int device, double *out6);
/* Measurement hook (bench.py's roofline.lloyd): average duration, by HIP events on the Lloyd stream, of `iters` launches of
 * one sweep over the resident float32 (u,v) stream X_dev[N][2] with fixed centres (k x 2, uncentred) and column mean.
 * what = 0: the full label-less sweep (k_lloyd_assign mode 3, 8 B/sample); 1: the pruned tile sweep (metadata built first,
 * untimed); 2: the streaming pass that builds the tile metadata before iteration 0; 3: the full final E-step (labels + inertia, every sample
 * read); 4: the pruned final E-step (tiles inside one cell labelled without being read); 5: the tile sweep in its full mode
 * (every tile walked by sample: what an incoherent field gets). */
int ofc_bench_lloyd_sweep(int device, const float *X_dev, int64_t N, int k, const double *centers, const double *mean,
                          int what, int iters, float *ms_per_launch);
/* ---- building blocks of a HOST-driven sharded fit (opticalflowclustering_amd/sharded.py): the same
 * kernels, one pass per call, records returned to the host so that ANY collective (RCCL, or
 * torch.distributed/gloo across nodes) can combine the shards.  X_dev is this rank's shard. ---- */
/* pass 0: out[f] = sum_i x[i][f]; pass 1: out[f] = sum_i (x[i][f]-mean[f])^2 */
int ofc_lloyd_colstats_dev(int device, const void *X_dev, int dtype, int64_t N, int d, const double *mean,
                           int pass, double *out);
/* one E-step (+ M-step accumulation when accumulate != 0) against the CENTRED centres centers_c (k x d):
 * labels_dev (N x u8, 0xFF = unassigned) is read and rewritten; record = [k*d sums of (x-mean) | k counts |
 * number of labels that changed] */
int ofc_lloyd_step_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *mean,
                       const double *centers_c, uint8_t *labels_dev, int accumulate, double *record);
/* PRECONDITION of ofc_lloyd_inertia_dev and ofc_lloyd_farthest_dev: every labels_dev[i] < k.  The kernels index
 * centers_c + label * d without a test, so a label that is still 0xFF (unassigned) reads past the k x d centres.  Run
 * ofc_lloyd_step_dev with the same k on the buffer first (it rewrites every label to a value below k); neither call
 * checks this itself: the labels live on the device and a check would cost a sweep. */
/* sum_i ||(x_i - mean) - centers_c[label_i]||^2 */
int ofc_lloyd_inertia_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *mean,
                          const double *centers_c, const uint8_t *labels_dev, double *inertia);
/* the sample farthest from its assigned (old) centre, skipping the local indices in excl[0..n_excl):
 * *dist2 (-1 if none), *index, x_c[d] = its centred coordinates, *label */
int ofc_lloyd_farthest_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *mean,
                           const double *centers_c, const uint8_t *labels_dev, const int64_t *excl, int n_excl,
                           double *dist2, int64_t *index, double *x_c, int *label);

/* ---- sample weights: KMeans(...).fit(X, sample_weight=w) (scikit-learn 1.7.2) ----
 * What the weights change, and what they do not:
 *   centring and tol   unweighted: X.mean(axis=0), mean(var(X)) * tol over the row count (_kmeans.py:1479-1484, _tolerance
 *                      :279-287)
 *   E-step             unweighted (first strict minimum of the expanded distance)
 *   M-step             sums[label] += x_c * w (product rounded, then added), weight_in_clusters[label] += w
 *                      (_k_means_lloyd.pyx)
 *   empty cluster      weight_in_clusters[j] == 0: a cluster that owns only zero-weight samples is empty
 *                      (_k_means_common.pyx:165-210); relocation picks the farthest samples by UNWEIGHTED squared distance
 *                      and moves each with its weight: sums[old] -= x*w, sums[new] = x*w, wk[new] = w, wk[old] -= w
 *   average            wk[j] > 0: sums / wk, otherwise the heaviest cluster's centre (_average_centers)
 *   stop               strict label equality, else shift <= tol (_kmeans.py:716-728)
 *   inertia            sum_i w_i |x_i - c_label|^2 (_inertia_dense, _k_means_common.pyx:128-164)
 * w_dtype is OFC_F32 or OFC_F64 (anything else: OFC_EINVAL); the arithmetic is f64 either way.  Weighted fits read every
 * sample in every iteration (the tile sweeps of ofc_lloyd_prune_stats hold unweighted sums).
 * PRECONDITION of every *_dev* form: the weights are finite and >= 0, and w_dev is 16-byte aligned.  The device forms do
 * not look (a check would cost a sweep); the host forms check on the host and return OFC_EINVAL. */
/* ofc_kmeans_fit with host weights w[N].  OFC_EINVAL also when the weights sum to 0. */
int ofc_kmeans_fit_w(int device, const void *X, int dtype, const void *w, int w_dtype, int64_t N, int d, int k,
                     const double *init, int max_iter, double tol_rel, double *centers, int32_t *labels,
                     double *inertia, int *n_iter);
/* ofc_kmeans_fit_dev_stats with device weights w_dev[N] (this rank's shard under a communicator).  w_dev == NULL is
 * ofc_kmeans_fit_dev_stats itself, tile sweeps included.  If the weights of all ranks sum to 0: OFC_EINVAL ("sum of sample
 * weights must be positive"), on every rank, after iteration 0's sweep. */
int ofc_kmeans_fit_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d,
                         int k, const double *init, int max_iter, double tol_rel, const double *colsum,
                         double *centers, uint8_t *labels_dev, double *inertia, int *n_iter);
/* KMeans.score's magnitude: one E-step of the UNCENTRED host X against `centers` and sum_i w_i |x_i - c_label|^2
 * (_labels_inertia, _kmeans.py:755-812); w may be NULL (unit weights).  score = -*inertia. */
int ofc_kmeans_score(int device, const void *X, int dtype, const void *w, int w_dtype, int64_t N, int d, int k,
                     const double *centers, double *inertia);
/* ofc_lloyd_step_dev (accumulate = 1) with weights: record = [k*d sums of (x-mean)*w | k weight sums | number of labels
 * that changed] (_k_means_lloyd.pyx's update_chunk) */
int ofc_lloyd_step_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d,
                         int k, const double *mean, const double *centers_c, uint8_t *labels_dev, double *record);
/* sum_i w_i ||(x_i - mean) - centers_c[label_i]||^2 (_k_means_common.pyx:128-164); labels as for ofc_lloyd_inertia_dev */
int ofc_lloyd_inertia_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d,
                            int k, const double *mean, const double *centers_c, const uint8_t *labels_dev,
                            double *inertia);
/* ofc_lloyd_farthest_dev, which ignores the weights (_k_means_common.pyx:186-187), plus *weight = the winner's weight
 * (:202; 0 if there is none) */
int ofc_lloyd_farthest_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d,
                             int k, const double *mean, const double *centers_c, const uint8_t *labels_dev,
                             const int64_t *excl, int n_excl, double *dist2, int64_t *index, double *x_c, int *label,
                             double *weight);
/* Weights from a resident (u,v) field (n vectors, f32) into w_dev (n f32), every operation rounded to f32 on its own:
 * kind 0 "magnitude": sqrtf(u*u + v*v); kind 1 "moving": u*u + v*v >= thr*thr ? 1 : 0 (thr finite, >= 0).  No reference
 * counterpart: it serves fits that should describe the motion and not the static background. */
int ofc_flow_weights_dev(int device, const float *flow_dev, int64_t n, int kind, float thr, float *w_dev);
/* Measurement hook: ofc_bench_lloyd_sweep(what = 0) with a weight stream (the label-less weighted sweep, 12 B/sample with
 * f32 weights, 16 B with f64); k 1..16 */
int ofc_bench_lloyd_sweep_w(int device, const float *X_dev, const void *w_dev, int w_dtype, int64_t N, int k,
                            const double *centers, const double *mean, int iters, float *ms_per_launch);

/* one step of k-means++ seeding (sklearn's default init for KMeans(n_clusters=k), the reference's construction at
 * color_kmeans.py:66, KmeanGrids.py:300; algorithm: sklearn/cluster/_kmeans.py:230-262): squared distances of all N
 * samples (centred by `mean`) to the rows X[cand[c]], c < n_cand <= 8, in the expanded form sklearn evaluates,
 * element-wise minimum with closest[] when it is not NULL; out_min [n_cand][N] f64, pots[c] = sum_i out_min[c][i].
 * The random draws, the cumulative sum and searchsorted stay on the host (cluster.kmeans_plusplus). */
int ofc_kpp_candidates(int device, const void *X, int dtype, int64_t N, int d, const double *mean,
                       const int64_t *cand, int n_cand, const double *closest, double *out_min, double *pots);
/* The whole seeding -- sklearn's _kmeans_plusplus (_kmeans.py:174-272), unit weights -- on device-resident X (this rank's
 * shard when a communicator is active; global row order is rank order).  The caller supplies the random numbers, so the
 * call is deterministic:
 *   first   GLOBAL index of the first centre
 *   u       (k-1) x n_trials uniforms in [0,1), in RandomState draw order; step c uses rand_vals = u[c-1][:] * current_pot
 *           (may be NULL when k == 1)
 *   colsum  this rank's column sums (as for ofc_kmeans_fit_dev_stats) or NULL
 * centers: k x d f64 (rows of X, un-centred); indices: k GLOBAL row indices.  Same result on every rank.
 * The running closest distances (N f64) stay in device scratch; one sweep over the samples per centre, nothing of size
 * N crosses to the host.  The distances are k_kpp_candidates' bit for bit; the cumulative sum is formed per
 * OFC_KPP_CHUNK samples, then per 1024 chunks, so it differs from np.cumsum's in rounding only.
 * OFC_EINVAL: null pointers, N < 0, global N < k, first outside the global range, n_trials outside 1..8, a u outside
 * [0,1); OFC_EUNSUPPORTED: k > 16, d > 4, more than 2^30 samples on one rank.  All checked before anything is launched. */
int ofc_kpp_seed_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *colsum,
                     int64_t first, const double *u, int n_trials, double *centers, int64_t *indices);
/* the sampling stage on its own (single rank; test and inspection hook):
 * idx[j] = min(searchsorted(cumsum(w_dev[0..N)), r[j], side='left'), N-1), j < n <= 8, 1 <= N <= 2^30; w_dev: N f64 >= 0 */
int ofc_kpp_sample_dev(int device, const double *w_dev, int64_t N, const double *r, int n, int64_t *idx);
/* ofc_kpp_seed_dev with sample weights: sklearn's _kmeans_plusplus(..., sample_weight) (_kmeans.py:174-272).  The data
 * is centred by the UNWEIGHTED column mean, as KMeans.fit does.  w_dev: this rank's N weights of w_dtype (OFC_F32 or
 * OFC_F64, 16-byte aligned; finite, >= 0, positive sum over all ranks), widened to f64.  They decide
 *   the first centre: the one number RandomState.choice(N, p=w/w.sum()) consumes is u_first in [0,1); the centre is the
 *           smallest GLOBAL row i with cumsum(w)[i] > u_first * W (W: the global weight sum, formed in the same fixed
 *           order), the last row of positive weight when rounding leaves none.  Never a row of weight zero.
 *   every later draw: rand_vals = u[c-1][:] * current_pot are looked up (side='left', clipped to N-1) in
 *           cumsum(w * closest), each product rounded on its own before it is added
 *   every candidate's potential: sum_i w[i] * min(closest[i], d(x_i, cand)).  The first minimum wins.
 * closest[] itself stays unweighted.  Everything else -- u, colsum, centers, indices, ranges, the result being the same
 * on every rank, a rank with an empty shard or only zero weights -- is ofc_kpp_seed_dev's.
 * OFC_EINVAL in addition: w_dev NULL or misaligned, a bad w_dtype, u_first outside [0,1) (all before anything is
 * launched), and a global weight sum that is not positive ("sum of sample weights must be positive"). */
int ofc_kpp_seed_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                       const double *colsum, double u_first, const double *u, int n_trials, double *centers,
                       int64_t *indices);
/* the weighted sampling stage on its own (single rank; test and inspection hook):
 * idx[j] = min(searchsorted(cumsum(w[0..N) * v[0..N)), r[j], side), N-1), j < n <= 8, 1 <= N <= 2^30, each product
 * rounded on its own.  w_dev: N f32 or f64 (w_dtype), 16-byte aligned; v_dev: N f64 >= 0, or NULL for ones;
 * side: 0 = 'left', 1 = 'right'.  total[0] = the sum of all N values as the device formed it. */
int ofc_kpp_sample_dev_w(int device, const void *w_dev, int w_dtype, const double *v_dev, int64_t N, const double *r, int n,
                         int side, int64_t *idx, double *total);
#define OFC_KPP_CHUNK 1024   /* samples per partial sum of the two-level cumulative sum */
/* many small independent problems in one launch (the per-grid-cell shape of KmeanGrids.py:376-392):
 * problem p owns rows [offsets[p], offsets[p+1]) of X (u8, d = 4); init/centers: P x k x d f64;
 * counts: P x k i32 = np.bincount(predict(X)); labels may be NULL. */
int ofc_kmeans_fit_batched(int device, const uint8_t *X, const int64_t *offsets, int n_problems,
                           int d, int k, const double *init, int max_iter, double tol_rel,
                           double *centers, int32_t *counts, int32_t *labels, int *n_iter);
/* the whole per-frame tail of KmeanGrids.py:376-392 on the device: grid cells of a BGR frame
 * (white row 0 / column 0 as cv2.rectangle leaves them) -> preprocess_image -> KMeans(k) ->
 * dominant cluster -> rint -> BGR2HSV.  init: cells x k x 4 f64.  centers: cells x 4 f64 (dominant
 * centre, rounded); hsv: cells x 3 u8.  channel_order: 0 = BGR as in memory (KmeanGrids.py:385),
 * 1 = swap to RGB first (the disk path, color_kmeansChange.py:33). */
int ofc_grid_kmeans(int device, const uint8_t *bgr, int W, int H, int rows, int cols, int k,
                    const double *init, int max_iter, double tol_rel, int channel_order,
                    double *centers, uint8_t *hsv);

/* same on device-resident frames (n_frames x HxWx3 u8): centers n_frames*cells x 4 f64 and
 * hsv n_frames*cells x 3 u8 are HOST buffers; init is NULL (device seeding) or host n_frames*cells*k*4 */
int ofc_grid_kmeans_dev(int device, const uint8_t *bgr_dev, int W, int H, int n_frames, int rows,
                        int cols, int k, const double *init, int max_iter, double tol_rel,
                        int channel_order, double *centers, uint8_t *hsv);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU; frames (hence (u,v) points) are sharded by rank; the only
 * exchange is one all-reduce (sum, f64) of [k*d sums | k counts | n_changed] per Lloyd iteration.
 * ------------------------------------------------------------------------------------------ */
#define OFC_UNIQUE_ID_BYTES 128
int ofc_dist_unique_id(uint8_t id[OFC_UNIQUE_ID_BYTES]);          /* rank 0, then broadcast */
int ofc_dist_init(int device, int rank, int world, const uint8_t id[OFC_UNIQUE_ID_BYTES]);
int ofc_dist_allreduce_f64(int device, double *buf_dev, int count); /* test hook */
/* The same exchange over a transport the CALLER provides: `fn` all-reduces `count` doubles in place across the ranks on
 * the host (op 0 sum, 1 max, 2 min; returns 0 on success) -- gloo or MPI across nodes without xGMI/RCCL connectivity, or a
 * pipe between processes that share one GPU (how the in-library N > 1 control flow -- all-reduced statistics, iterations
 * behind the halt flag, the relocation exchange with its owner election -- is tested with DIFFERENT shards per rank).
 * Every collective then costs a stream synchronisation and two small copies. */
typedef int (*ofc_host_allreduce_fn)(double *buf, int count, int op, void *user);
int ofc_dist_init_host(int device, int rank, int world, ofc_host_allreduce_fn fn, void *user);
/* TEST HOOK: emulate `world` ranks that all hold the caller's shard, without a communicator (sums become world-fold,
 * max/min unchanged, rank 0): lets one GPU exercise the N>1 control flow of ofc_kmeans_fit_dev -- the result must equal
 * a single-rank fit over `world` concatenated copies of the shard.  world = 1 switches it off. */
int ofc_dist_loopback(int world);
int ofc_dist_finalize(void);

/* ------------------------------------------------------------------------------------------
 * Streaming ingest (BASELINE.json configs[4] shape): frames arrive from the host one at a time (a decoder);
 * they are packed into pinned ring buffers, uploaded with hipMemcpyAsync on a copy stream while the previous batch
 * computes, and reduced on the device to the grid-cell averaged flow: per pair rows*cols (u,v) means.
 * No reference counterpart beyond the cv2.VideoCapture loop (KmeanGrids.py:180-187); the grid geometry is
 * overlayGridAndComputeAvgColor's (KmeanGrids.py:56-59).
 * ------------------------------------------------------------------------------------------ */
typedef struct ofc_stream ofc_stream_t;
int ofc_stream_create(int device, int W, int H, const ofc_fb_params *p, int batch_pairs, int rows, int cols,
                      ofc_stream_t **out);
/* push one HxW u8 frame; *pairs_done (may be NULL) = pairs whose cell means are complete so far: never decreasing between
 * two calls of ofc_stream_finish, never more than the pairs of the batches submitted (batch_pairs * ((pushes - 1) /
 * batch_pairs)), and it may lag them */
int ofc_stream_push_gray(ofc_stream_t *s, const uint8_t *gray, int *pairs_done);
/* flush the partial batch, wait, and copy all cell means out: cell_uv[n_pairs][rows*cols][2] f32, *n_pairs = pushes - 1 (0
 * after one push or none: not an error, nothing is written).  The stream is then empty and ready for the frames of another
 * clip: no frame is carried over, the first pair of the next clip is (its frame 0, its frame 1).
 * cell_uv too small (max_pairs < *n_pairs): OFC_EINVAL, *n_pairs is set to the number of pairs to make room for, nothing is
 * written to cell_uv, and the results STAY with the stream: the same call with enough room returns all of them (call it again
 * before pushing further frames).
 * cell_uv == NULL: count only; *n_pairs is set and the results are dropped. */
int ofc_stream_finish(ofc_stream_t *s, float *cell_uv, int max_pairs, int *n_pairs);
/* A stream that also counts: from the next batch on, every pair's field is labelled against the model and counted per
 * cell (ofc_grid_assign_counts_dev's kernel, behind the cell means of the same batch, so *pairs_done keeps its meaning).
 * mean: 2 doubles, NULL = (0, 0); centers_c: k x 2, the centres minus mean, as for ofc_lloyd_step_dev.  A stream has no
 * field mean before its clip ends, so the usual model is mean (0, 0): KMeans.predict's un-centred E-step.
 * Only on a stream that holds no frame and no undelivered result (fresh, or straight after a finish): otherwise OFC_EINVAL
 * and the model stays as it was.  k outside 0 .. 16: OFC_EUNSUPPORTED; a mean or centre that is not finite: OFC_EINVAL.
 * k = 0 removes the model: the stream then launches exactly what a stream that never had one launches. */
int ofc_stream_set_model(ofc_stream_t *s, int k, const double *mean, const double *centers_c, int with_sums);
/* ofc_stream_finish that also delivers counts[n_pairs][rows*cols][k] int32 (and sums[n_pairs][rows*cols][k][2] f64 when the
 * model was set with_sums), as ofc_grid_assign_counts_dev writes them for each pair's field.
 * cell_uv, counts, sums may each be NULL (not copied; all NULL: count and drop).  Too small: exactly ofc_stream_finish's
 * contract (OFC_EINVAL, *n_pairs set, nothing written, results stay).
 * OFC_EINVAL without a model, or with sums != NULL on a model without sums.
 * ofc_stream_finish on a stream with a model returns the cell means as ever and drops the counts. */
int ofc_stream_finish_clusters(ofc_stream_t *s, float *cell_uv, int32_t *counts, double *sums, int max_pairs, int *n_pairs);
/* A stream that also builds the (u,v) histogram of its footage (see "Histogram of flow vectors" below): from the next
 * batch on, every pair's field is added to the stream's table (ofc_uv_hist_accum_dev's kernel, on the compute stream behind
 * the cell means and the model's counts of the same batch, so *pairs_done keeps its meaning).  The table starts at zero.
 * bins, range as for ofc_uv_hist_accum_dev (anything else: OFC_EINVAL); bins = 0 removes the table: the stream then
 * launches exactly what a stream that never had one launches.
 * Same precondition as ofc_stream_set_model: no frame and no undelivered result, otherwise OFC_EINVAL and nothing changes.
 * Setting the bins and range the stream already has keeps the table and what is in it; any other pair starts a new one. */
int ofc_stream_set_histogram(ofc_stream_t *s, int bins, float range);
/* Copy the stream's table out (table_host: 3*bins*bins + 1 int64, may be NULL) and zero it when reset != 0.  Legal under
 * ofc_stream_set_histogram's precondition only, i.e. straight after a finish (or on a fresh stream: all zeros); OFC_EINVAL
 * otherwise, and without a histogram.  A finish neither delivers nor clears the table: it spans finishes until it is reset,
 * so one fit can cover several clips. */
int ofc_stream_read_histogram(ofc_stream_t *s, int64_t *table_host, int reset);
void ofc_stream_destroy(ofc_stream_t *s);
/* per-cell mean of a flow field (host buffers): flow HxWx2 f32 -> cell_uv rows*cols x 2 f32 */
int ofc_grid_cell_mean_flow(int device, const float *flow, int W, int H, int rows, int cols, float *cell_uv);

/* Per grid cell and label: how many pixels carry it, and optionally the sums of their flow vectors.
 * Grid geometry is overlayGridAndComputeAvgColor's (KmeanGrids.py:56-59), as k_grid_cell_mean_flow uses it:
 * xs = W / cols, ys = H / rows; cell cy*cols+cx owns rows [cy*ys, (cy+1)*ys) x columns [cx*xs, (cx+1)*xs).
 * Pixels right of cols*xs or below rows*ys belong to no cell.
 * labels_dev  n_frames x H x W u8 (what ofc_kmeans_fit_dev leaves in labels_dev for n_frames flow fields).
 *             A label >= k (0xFF = unassigned included) is counted nowhere and indexes nothing.
 * counts_dev  n_frames x rows*cols x k int32
 * flow_dev, sums_dev: both NULL, or flow_dev n_frames x H x W x 2 f32 and sums_dev n_frames x rows*cols x k x 2 f64
 *             = sum of u, sum of v over the pixels counted (f64 accumulation in a fixed order: two calls give the same
 *             bits, and a frame's sums do not depend on n_frames; +0.0 where the count is 0).
 * OFC_EINVAL: null pointers, only one of flow_dev / sums_dev, n_frames < 1, rows < 1 or > H, cols < 1 or > W.
 * OFC_EUNSUPPORTED: k outside 1 .. 16 (LLOYD_KMAX); W*H above 2^31 - 1.  Everything is checked before anything is
 * launched. */
int ofc_grid_label_counts_dev(int device, const uint8_t *labels_dev, const float *flow_dev, int W, int H,
                              int n_frames, int rows, int cols, int k, int32_t *counts_dev, double *sums_dev);
/* ofc_lloyd_step_dev's label (accumulate = 0) of every pixel's (u,v), counted as ofc_grid_label_counts_dev counts labels, in
 * one sweep and without a label buffer: 8 B read and nothing written per pixel.  The label is the byte ofc_lloyd_step_dev
 * writes for the same pixel, mean and centres (one shared device function); counts and sums are then those of
 * ofc_grid_label_counts_dev on these labels, bit for bit (same walk, same order of summation).
 * mean: 2 doubles (host), NULL = (0, 0); centers_c: k x 2 (host), the centres minus mean, as for ofc_lloyd_step_dev.
 * sums_dev may be NULL.
 * OFC_EINVAL: null pointers, a mean or centre that is not finite, n_frames < 1, rows < 1 or > H, cols < 1 or > W.
 * OFC_EUNSUPPORTED: k outside 1 .. 16; W*H above 2^31 - 1.  Everything is checked before anything is launched. */
int ofc_grid_assign_counts_dev(int device, const float *flow_dev, int W, int H, int n_frames, int rows, int cols, int k,
                               const double *mean, const double *centers_c, int32_t *counts_dev, double *sums_dev);

/* ------------------------------------------------------------------------------------------
 * Histogram of flow vectors: per bin of the (u,v) plane an exact count and exact fixed-point sums of its members.  A
 * weighted Lloyd fit over the bin means (ofc_kmeans_fit_w: points = sum / count / 65536, weights = counts) stands in for
 * the fit over the field, whose vectors need not be resident (opticalflowclustering_amd/uvhist.py).  No reference
 * counterpart.
 * bins = B: a power of two, 16 .. 2048.  range = R: a power of two, 2^-4 .. 2^10.  The table covers [-R, R) on both axes.
 * table: 3*B*B + 1 int64 = count[B*B], sum_u[B*B], sum_v[B*B], outside; the bin of (iu, iv) is iv*B + iu.
 * The bin of a vector (this arithmetic is the definition): tu = (u + R) * (B / 2R), the sum rounded to f32, the product
 * exact (the scale is a power of two); tv likewise from v.  In range iff 0 <= tu < B and 0 <= tv < B: NaN, +-inf, u = R and
 * a u whose u + R rounds up to 2R are outside.  iu = (int)floorf(tu), iv = (int)floorf(tv).
 * In range: count += 1, sum_u += llrint((double)u * 65536), sum_v += llrint((double)v * 65536).  Otherwise outside += 1 and
 * nothing else.  Integer adds only: two runs give equal bits whatever the order of the adds, and tables of batches, clips
 * or ranks merge by plain addition.
 * ------------------------------------------------------------------------------------------ */
#define OFC_UV_HIST_SHARE 2048      /* consecutive vectors a work-group of the kernel takes at a time */
#define OFC_UV_HIST_MAX_GRID 2048   /* most work-groups of a launch: above SHARE * MAX_GRID vectors they take several shares */
/* flow_dev: n vectors [n][2] f32 on the device (8-byte aligned); table_dev: the table on the device.  The caller zeroes it;
 * the call adds to what is there, and returns when the adds are done.  n = 0 is a no-op.
 * OFC_EINVAL: bins or range outside the above, n < 0, a null pointer (flow_dev may be NULL when n = 0).  Everything is
 * checked before anything is launched. */
int ofc_uv_hist_accum_dev(int device, const float *flow_dev, int64_t n, int bins, float range, int64_t *table_dev);
/* the same with host buffers; it WRITES table_host: zero, accumulate, copy out */
int ofc_uv_hist(int device, const float *flow_host, int64_t n, int bins, float range, int64_t *table_host);
/* Measurement hook: average duration, by HIP events on the kernel's stream, of `iters` launches of the histogram kernel
 * over flow_dev (n >= 1), two warm-up launches before them.  The table is the hook's own, zeroed once, untimed. */
int ofc_bench_uv_hist(int device, const float *flow_dev, int64_t n, int bins, float range, int iters, float *ms_per_launch);

/* ------------------------------------------------------------------------------------------
 * Camera motion: per frame pair, a translation or an affine model of the flow field, fitted by iteratively re-selected least
 * squares and subtracted, so that what follows the flow (the Lloyd fits and their weights, the histogram, the stream's model,
 * the cell summaries) sees the scene's motion and not the camera's.  No reference counterpart.
 * Definition (this arithmetic is the definition).  Field (u, v)[y][x], W x H.  X = 2x - (W-1), Y = 2y - (H-1): twice the
 * offset from the frame centre, always integers.  Model p = (p0..p5), f64, in pixels and pixels per pixel about the centre:
 *   u^ = p0 + p1 X/2 + p2 Y/2,  v^ = p3 + p4 X/2 + p5 Y/2,  each evaluated as one chain fma(p2, 0.5*Y, fma(p1, 0.5*X, p0)) in f64.
 * kind 1 "translation" fixes p1 = p2 = p4 = p5 = 0; kind 2 "affine" fits all six.
 * Valid: u and v finite and |u|, |v| < 1024.  Any other vector is outside: counted, never used.
 * Fixed point: qu = llrint((double)u * 65536), qv likewise (the histogram's rule).
 * Moments over a set S of valid pixels, thirteen int64:
 *   n, SX, SY, SXX, SXY, SYY, Squ, SXqu, SYqu, Sqv, SXqv, SYqv, outside
 * (sums of 1, X, Y, X X, X Y, Y Y, qu, X qu, Y qu, qv, X qv, Y qv over S; outside counts the pair's vectors that are not
 * valid, whatever S).  Integers only: any order of the adds gives equal bits.  They fit int64 iff W * H * max(W, H) < 2^37
 * (3840 x 2160 passes, 8192 x 8192 does not).
 * Rounds.  Round 0: S = every valid pixel; p = the least-squares solution of the moments.  Round t = 1..T with threshold c_t
 * px: S = valid pixels with (u - u^)^2 + (v - v^)^2 <= c_t^2, compared in f64 under round t-1's model; solve again.  If
 * n < 3 (translation: n < 1) or a pivot of the solve is not positive, the pair keeps the model of the round before, gets
 * status 1 and takes no further rounds; in round 0 the model is all zeros and the status 2.  Status 0: every round solved.
 * A fit with kind 1 forms only n, Squ, Sqv and outside; the other moments of its history are 0.
 * Solve: the exact least-squares solution of the integer moments, computed in f64: the 3 x 3 normal matrix over
 * (1, X sx, Y sy), sx = 2^-e with e = floor((floor(log2 SXX) - floor(log2 n)) / 2) (1 when SXX = 0) and sy likewise from SYY,
 * so its entries are O(n); factored as L D L^T (Cholesky without the square roots; the pivots are D's entries); u and v
 * share the factors.  One function (csrc/motion_model.h) runs in the kernel and on the host: equal bits.
 * Subtract: u' = (float)((double)u - u^), v' likewise; a vector with a non-finite component passes through unchanged.
 * thresholds: T doubles (c_1..c_T), T in 0..8, each finite and positive.  At most 65535 pairs per call (OFC_EUNSUPPORTED).
 * ------------------------------------------------------------------------------------------ */
/* Host only, no device is touched: OFC_OK if fields of W x H can be fitted with `kind`.  OFC_EINVAL: kind not 1 or 2, W or
 * H < 1, kind 2 with W < 2 or H < 2.  OFC_EUNSUPPORTED: W * H * max(W, H) >= 2^37.  Every call below decides by it first. */
int ofc_motion_check(int W, int H, int kind);
/* Host only, no device is touched: how the moment kernel and the subtraction split npair fields of W x H.  A field is
 * nshare = ceil(W H / 2048) shares of 2048 consecutive vectors; min(nshare, max(16, min(256, 2048 / npair))) work-groups
 * per pair take `per` consecutive shares each.  out = { groups, per = ceil(nshare / groups), the groups that get at least
 * one share, the shares of the last of those }.  The kernels and their launchers compute groups and per by the functions
 * this reports.  OFC_EINVAL: out NULL, npair < 1, W or H < 1; OFC_EUNSUPPORTED as ofc_motion_check, or npair > 65535. */
int ofc_motion_launch_geometry(int W, int H, int npair, int out[4]);
/* Host only: the solve above on given moments.  p receives the model and *status 0, or zeros and *status 1 when the moments
 * cannot be solved.  OFC_EINVAL: a null pointer, kind not 1 or 2. */
int ofc_motion_solve(const int64_t m[13], int kind, double p[6], int *status);
/* One launch of the moment reduction over flow_dev [npair][H][W][2] f32 (8-byte aligned) -> moments_host [npair][13].
 * models NULL: S = every valid pixel.  Otherwise models [npair][6] (finite) and c [npair] (finite, positive): S as in a
 * round under that model and threshold.  Always all thirteen.  The tests' handle on the kernel. */
int ofc_motion_moments_dev(int device, const float *flow_dev, int W, int H, int npair, const double *models, const double *c,
                           int64_t *moments_host);
/* The whole fit, T + 1 moment launches and T + 1 solves chained on one stream with no host round trip between rounds.
 * models_host [npair][6], status_host [npair]; history_models [(T+1)][npair][6] and history_moments [(T+1)][npair][13] may
 * each be NULL: what every round solved from and found.  A pair that takes no further rounds repeats its kept model, with
 * zero moments, in the rounds it does not take. */
int ofc_motion_fit_dev(int device, const float *flow_dev, int W, int H, int npair, int kind, const double *thresholds, int T,
                       double *models_host, int *status_host, double *history_models, int64_t *history_moments);
/* dst_dev = flow_dev minus the models (models_host [npair][6], finite); dst_dev may equal flow_dev.  Returns when done. */
int ofc_motion_subtract_dev(int device, const float *flow_dev, int W, int H, int npair, const double *models_host,
                            float *dst_dev);
/* ofc_motion_fit_dev with a host field: upload, fit, download */
int ofc_motion_fit(int device, const float *flow_host, int W, int H, int npair, int kind, const double *thresholds, int T,
                   double *models_host, int *status_host, double *history_models, int64_t *history_moments);
/* the same, and residual_host [npair][H][W][2] = the field minus the fitted models */
int ofc_motion_compensate(int device, const float *flow_host, int W, int H, int npair, int kind, const double *thresholds,
                          int T, float *residual_host, double *models_host, int *status_host, double *history_models,
                          int64_t *history_moments);
/* A stream that removes the camera: from the next batch on, every pair's field is fitted and the model subtracted in place,
 * on the compute stream between the flow and the cell means, so the cell means, the model's counts and the histogram all
 * see the residual field.  kind 0 removes the camera: the stream then launches exactly what a stream that never had one
 * launches.  Same precondition as ofc_stream_set_model (no frame and no undelivered result; otherwise OFC_EINVAL and
 * nothing changes); kind, thresholds, T and the frame size as for ofc_motion_fit_dev. */
int ofc_stream_set_camera(ofc_stream_t *s, int kind, const double *thresholds, int T);
/* models [n][6] and status [n] (each may be NULL) of the n pairs the LAST finish delivered, in their order.  A finish keeps
 * that count when it empties the stream, so this is valid straight after a finish (either form) and until the next frame
 * is pushed: with frames held, OFC_EINVAL.  max_pairs < n: OFC_EINVAL, nothing written.  A finish that was refused for lack
 * of room keeps the fits with the results.  OFC_EINVAL without a camera. */
int ofc_stream_read_camera(ofc_stream_t *s, double *models, int *status, int max_pairs);
/* Measurement hook: average duration, by HIP events, of `iters` launches over flow_dev [npair][H][W][2], two warm-up launches
 * before them, under round 0's affine model and c = 4 px.  what = 0: the moment kernel, all thirteen; 1: its translation
 * form (n, Squ, Sqv, outside); 2: the solve kernel; 3: the subtraction into a buffer of the hook's own; 4: a whole affine
 * fit with thresholds (4, 2, 1): four moment launches and four solves. */
int ofc_bench_motion(int device, const float *flow_dev, int W, int H, int npair, int what, int iters, float *ms_per_launch);

/* ------------------------------------------------------------------------------------------
 * Moving objects: connected components of a per-pixel key map, and one record per component.  Stands where the reference
 * read YOLO boxes and segmented contours from files (KmeanGrids.py:16-50); neither is generated here.
 * Definition (this text is the definition; every output is an integer, so any order of work gives equal bits).
 * Key map: u8 [npair][H][W]; 255 = background.  It is the format ofc_kmeans_fit_dev leaves in labels_dev (0xFF =
 * unassigned): a fitted clip's label buffer is a key map as it stands.
 * Adjacency, within one pair only: connectivity 4 = pixels that share an edge, 8 = an edge or a corner.  Adjacent pixels
 * p, q are connected iff key[p] == key[q] != 255.  A component is a class of the transitive closure.
 * Root of a component: its smallest y*W + x.  Label map: int32 [npair][H][W], the root for a foreground pixel, -1 for
 * background.  The root is a minimum, so the label map is unique whatever order the device works in.
 * Record of a component, OFC_BLOB_FIELDS = 12 int64:
 *   root, key, area, xmin, ymin, xmax, ymax, Sx, Sy, nvalid, Squ, Sqv
 * (pixel count, inclusive bounding box, sums of x and of y over its pixels).  With a flow field [npair][H][W][2] f32 the last
 * three cover the component's valid vectors: valid as the camera block has it (u, v finite and |u|, |v| < 1024), fixed point
 * as there (qu = llrint((double)u * 65536)).  Without a field they are 0.  Sums, minima and maxima of integers only.
 * Table of a pair: the records of its components with area >= min_area, ascending by root (raster order of first pixel).
 * found[pair] = how many such components there are.  If found > max_blobs the pair delivers NO record (n = 0) and found
 * stays exact: the overflow outcome is as deterministic as the rest.  The label map is complete whatever min_area and
 * max_blobs are.
 * Limits: W, H >= 1, W*H <= 2^31 - 1 (else OFC_EUNSUPPORTED); npair 1 .. 65535 (above: OFC_EUNSUPPORTED); connectivity 4
 * or 8; min_area >= 1; max_blobs 1 .. 65536 (above: OFC_EUNSUPPORTED); everything else OFC_EINVAL.
 * On the device: tiles of OFC_BLOB_TILE_W x OFC_BLOB_TILE_H pixels are resolved in LDS, then united across their borders
 * by a minimum-index union-find (csrc/blobs.hip).  Every loop there is capped; a cap that is hit (it cannot be by the
 * algorithm) makes the call return OFC_EHIP instead of hanging.
 * ------------------------------------------------------------------------------------------ */
#define OFC_BLOB_TILE_W 64
#define OFC_BLOB_TILE_H 16
#define OFC_BLOB_FIELDS 12
/* Host only, no device is touched: OFC_OK iff the arguments are inside the limits above.  Every call below decides by it
 * (with the values it does not take at their minimum) before anything is allocated or launched. */
int ofc_blob_check(int W, int H, int npair, int connectivity, int min_area, int max_blobs);
/* Key map from a field: flow_dev [npair][H][W][2] f32 (8-byte aligned) -> keys_dev u8 [npair][H][W].  Three stages:
 * 1. use_thr != 0 (thr finite, >= 0): background unless u*u + v*v >= thr*thr, every operation rounded to f32 on its own:
 *    the predicate of ofc_flow_weights_dev kind 1 (one shared device function); a NaN fails it.
 * 2. k > 0 (k, mean, centers_c as for ofc_grid_assign_counts_dev): L = the byte ofc_lloyd_step_dev writes for the vector (the
 *    shared device function); background unless bit L of `select` is set.
 * 3. key = L, or 0 when merge != 0 or k == 0.
 * k == 0: mean, centers_c, select are ignored.  k outside 0 .. 16: OFC_EUNSUPPORTED. */
int ofc_blob_keys_dev(int device, const float *flow_dev, int W, int H, int npair, int use_thr, float thr, int k,
                      const double *mean, const double *centers_c, uint32_t select, int merge, uint8_t *keys_dev);
/* keys_dev -> labels_dev int32 [npair][H][W] (4-byte aligned), the label map above.  Returns when done. */
int ofc_blob_label_dev(int device, const uint8_t *keys_dev, int W, int H, int npair, int connectivity, int32_t *labels_dev);
/* keys_dev, its label map labels_dev and flow_dev (or NULL) -> table_dev int64 [npair][max_blobs][12] and found_dev int32
 * [npair].  On the device a pair's first min(found, max_blobs) slots hold records in no specified order; slots past them
 * are not written.  ofc_blob_table_read delivers the table defined above. */
int ofc_blob_table_dev(int device, const uint8_t *keys_dev, const int32_t *labels_dev, const float *flow_dev, int W, int H,
                       int npair, int min_area, int max_blobs, int64_t *table_dev, int32_t *found_dev);
/* Device to host: table_host int64 [npair][max_blobs][12] receives each pair's records sorted by root in its first n_host
 * [pair] rows (rows past them are zeroed), found_host [pair] the exact count; found > max_blobs gives n = 0. */
int ofc_blob_table_read(int device, const int64_t *table_dev, const int32_t *found_dev, int npair, int max_blobs,
                        int64_t *table_host, int32_t *n_host, int32_t *found_host);
/* The whole chain on host buffers.  Exactly one of keys_host (u8 [npair][H][W]) and "flow_host plus the key parameters of
 * ofc_blob_keys_dev" decides the key map: with keys_host the key parameters are ignored and flow_host (may be NULL) only
 * feeds the records.  labels_host int32 [npair][H][W] and keys_out u8 [npair][H][W] may be NULL.  The rest as
 * ofc_blob_table_read. */
int ofc_blobs(int device, const uint8_t *keys_host, const float *flow_host, int W, int H, int npair, int use_thr, float thr,
              int k, const double *mean, const double *centers_c, uint32_t select, int merge, int connectivity, int min_area,
              int max_blobs, int32_t *labels_host, uint8_t *keys_out, int64_t *table_host, int32_t *n_host,
              int32_t *found_host);
/* A stream that finds moving objects: from the next batch on, every pair's field (the residual, when a camera is set) gets a
 * key map, a label map and a table, on the compute stream behind everything else of the batch.  Foreground: u*u + v*v >= thr*thr
 * (stage 1 of ofc_blob_keys_dev); with a model (ofc_stream_set_model, whenever it is set) the key is the model's label L of
 * the vector, every label selected, nothing merged; without one the key is 0.  The records' sums come from the same field.
 * connectivity 0 removes the blobs: the stream then launches exactly what a stream that never had them launches.  Same
 * precondition as ofc_stream_set_camera (no frame and no undelivered result; otherwise OFC_EINVAL and nothing changes);
 * connectivity, min_area, max_blobs as ofc_blob_check decides them for the stream's frame size, thr finite and >= 0. */
int ofc_stream_set_blobs(ofc_stream_t *s, int connectivity, float thr, int min_area, int max_blobs);
/* The tables of the n pairs the LAST finish delivered, as ofc_blob_table_read writes them: table_host [max_pairs][max_blobs]
 * [12], n_host and found_host [max_pairs].  Valid under ofc_stream_read_camera's conditions: straight after a finish (either
 * form) and until the next frame is pushed; max_pairs < n: OFC_EINVAL, nothing written; OFC_EINVAL without blobs. */
int ofc_stream_read_blobs(ofc_stream_t *s, int64_t *table_host, int32_t *n_host, int32_t *found_host, int max_pairs);
/* Measurement hook: average duration by HIP events of one stage over `iters` runs of the chain on keys_dev (flow_dev may be
 * NULL unless what is 0), two warm-up runs before them; min_area 1, max_blobs 65536, buffers of the hook's own.  Every run
 * executes the whole chain, so that each stage sees the state the stage before leaves; only the chosen part is timed.
 * what = 0: the key kernel (threshold 0.5, no model) into a buffer of the hook's own; 1: the local stage; 2: the seam
 * stage; 3: the flatten; 4: the label map (1 + 2 + 3); 5: the table (clear, areas, slots, records); 6: label map and table. */
int ofc_bench_blobs(int device, const uint8_t *keys_dev, const float *flow_dev, int W, int H, int npair, int connectivity,
                    int what, int iters, float *ms_per_run);

/* ---- Blob links: which blob of pair t continues as which blob of pair t+1.  The reference has no counterpart: it read
 * boxes per frame from files (KmeanGrids.py:16-50) and never related one frame's boxes to the next's.
 * Definition (normative, like the text above; every output is an integer).
 * Moves: int32 [npair][H][W], one word per pixel, from a flow field f32 [npair][H][W][2].  A vector is valid exactly as the
 * blob records and the camera block have it: u, v finite and |u|, |v| < 1024.  For a valid vector dx = u rounded to the
 * nearest integer, ties to even, in f32 (__float2int_rn on the device, np.rint of the float32 on the host), dy the same
 * from v; the word is (uint16)dy << 16 | (uint16)dx, and both fit int16 because |u| < 1024.  For an invalid vector the
 * word is OFC_BLOB_NO_MOVE = 0x80008000 (dx = dy = -32768).  Moves are an object of their own, not read from the flow by the
 * link kernel: the field the blobs are keyed on is often the residual after camera removal, while a pixel lands in the
 * next frame by the WHOLE flow; take the moves before the camera is subtracted.
 * Link votes: label maps `labels` int32 [npair][H][W] as ofc_blob_label_dev leaves them, the moves of the same pairs and
 * min_area >= 1.  The area of a root is the number of pixels that carry it in its pair's label map.  For every transition
 * t = 0 .. npair-2 and every pixel p = (x, y) of pair t with
 *   a = labels[t][p], a >= 0 and area_t(a) >= min_area;  moves[t][p] != OFC_BLOB_NO_MOVE;
 *   x' = x + dx, y' = y + dy, 0 <= x' < W and 0 <= y' < H;
 *   b = labels[t+1][y'*W + x'], b >= 0 and area_t+1(b) >= min_area
 * the pixel is one vote for (a, b).  (A label outside [-1, W*H) in a caller's map votes for nothing and is never used as
 * an index.)
 * Link table of transition t: one row root_a, root_b, votes (OFC_BLOB_LINK_FIELDS = 3 int64) per distinct (a, b) with at
 * least one vote, ascending by (root_a, root_b).  nlinks[t] = the number of rows when that is <= max_links; otherwise the
 * transition delivers NO row and nlinks[t] = -1.  Overflow happens if and only if there are more than max_links distinct
 * links, so the outcome is as deterministic as the rest.  npair = 1 is allowed and has zero transitions.
 * Limits: those of ofc_blob_check, plus max_links 1 .. 65536 (above: OFC_EUNSUPPORTED; below 1: OFC_EINVAL).
 * On the device a transition's table is open addressing on the 64-bit key (a << 32) | b; every probe loop is capped at the
 * table's capacity, and a cap that is hit with room left (it cannot be by the algorithm) makes ofc_blob_links_read return
 * OFC_EHIP. ---- */
#define OFC_BLOB_LINK_FIELDS 3
#define OFC_BLOB_NO_MOVE 0x80008000u
/* Host only, no device is touched: OFC_OK iff the arguments are inside the limits above.  Every call below decides by it
 * (with the values it does not take at their minimum) before anything is allocated or launched.  No counterpart in the
 * reference (it read boxes from files), as for every call of this block. */
int ofc_blob_link_check(int W, int H, int npair, int min_area, int max_links);
/* Host only: the bytes links_dev needs for ntrans transitions under max_links, 0 for arguments outside the limits.  Layout
 * (private to the library but stable within a build): uint64 keys [ntrans][cap], then int32 votes [ntrans][cap], with cap the
 * smallest power of two >= 2 * max_links; the counter words are nlinks_dev.  No counterpart in the reference. */
size_t ofc_blob_links_bytes(int max_links, int ntrans);
/* flow_dev [npair][H][W][2] f32 (8-byte aligned) -> moves_dev int32 [npair][H][W] (4-byte aligned; 16-byte loads and stores
 * where both bases allow).  Returns when done.  No counterpart in the reference. */
int ofc_blob_moves_dev(int device, const float *flow_dev, int W, int H, int npair, int32_t *moves_dev);
/* labels_dev, moves_dev int32 [npair][H][W] -> the npair-1 transitions' tables in links_dev (8-byte aligned,
 * ofc_blob_links_bytes(max_links, npair - 1) bytes) and their counter words in nlinks_dev int32 [npair-1], both as
 * ofc_blob_links_read interprets them.  The areas are counted again from the label maps into scratch of the library's own.
 * Neither input is written.  npair = 1: nothing is launched and neither output is touched (both may be NULL).  Returns when
 * done.  No counterpart in the reference. */
int ofc_blob_links_dev(int device, const int32_t *labels_dev, const int32_t *moves_dev, int W, int H, int npair, int min_area,
                       int max_links, void *links_dev, int32_t *nlinks_dev);
/* Device to host: links_host int64 [ntrans][max_links][3] receives each transition's rows sorted by (root_a, root_b) in its
 * first nlinks_host[t] rows, rows past them zeroed; an overflowed transition has nlinks_host[t] = -1 and all its rows
 * zeroed.  ntrans = 0 writes nothing.  No counterpart in the reference. */
int ofc_blob_links_read(int device, const void *links_dev, const int32_t *nlinks_dev, int ntrans, int max_links,
                        int64_t *links_host, int32_t *nlinks_host);
/* The whole chain on host buffers: labels_host int32 [npair][H][W] (ofc_blobs' labels_host) and flow_host f32 [npair][H][W][2],
 * the field that says where pixels go (before any camera removal) -> moves_out int32 [npair][H][W] (may be NULL), links_host
 * and nlinks_host as ofc_blob_links_read writes them for npair - 1 transitions.  No counterpart in the reference. */
int ofc_blob_links(int device, const int32_t *labels_host, const float *flow_host, int W, int H, int npair, int min_area,
                   int max_links, int32_t *moves_out, int64_t *links_host, int32_t *nlinks_host);
/* A stream with blobs (ofc_stream_set_blobs; without them OFC_EINVAL) that also links them: from the next batch on the
 * batch's moves are taken from the field BEFORE the camera (if any) is subtracted, and behind the batch's label maps every
 * transition is voted: those inside the batch, and the one from the previous batch's last pair, whose label map, moves and
 * areas the stream carries over (12 bytes per pixel).  A finish ends the clip: the first pair after it has no predecessor.
 * min_area is the stream's blobs' own.  max_links 0 removes the links: the stream then launches exactly what a stream with
 * blobs alone launches; ofc_stream_set_blobs with connectivity 0 removes them too.  Same precondition as
 * ofc_stream_set_blobs (no frame and no undelivered result; otherwise OFC_EINVAL and nothing changes); like it, it empties
 * what ofc_stream_read_blobs delivers.  max_links as ofc_blob_link_check decides it.  No counterpart in the reference. */
int ofc_stream_set_blob_links(ofc_stream_t *s, int max_links);
/* The n - 1 transitions of the n pairs the LAST finish delivered, as ofc_blob_links_read writes them: links_host
 * [max_trans][max_links][3], nlinks_host [max_trans].  Valid under ofc_stream_read_blobs' conditions; max_trans < n - 1:
 * OFC_EINVAL, nothing written; OFC_EINVAL without links.  No counterpart in the reference. */
int ofc_stream_read_blob_links(ofc_stream_t *s, int64_t *links_host, int32_t *nlinks_host, int max_trans);
/* Measurement hook: average duration by HIP events of one part over `iters` runs of the chain moves, areas, clears, votes on
 * labels_dev and flow_dev, two warm-up runs before them; min_area 1, max_links 65536, buffers of the hook's own.  Every run
 * executes the whole chain; only the chosen part is timed.  what = 0: the moves kernel; 1: the areas (clear and sweep);
 * 2: the link kernel with the clears of its tables; 3: all of it.  npair = 1 has no transition: 2 times two event records.
 * No counterpart in the reference. */
int ofc_bench_blob_links(int device, const int32_t *labels_dev, const float *flow_dev, int W, int H, int npair, int what,
                         int iters, float *ms_per_run);

/* ---- Forward-backward consistency: which vectors of a field survive the check against the field of the reversed pair.
 * The reference has no counterpart: it trusted every vector of cv2.calcOpticalFlowFarneback alike
 * (computeOpticalFlowModule.py:20-22).
 * Definition (normative, like the text above; every output is an integer).
 * Inputs: fwd f32 [npair][H][W][2], pair t being frame t -> t+1 on frame t's grid; bwd of the same shape, the field frame
 * t+1 -> t on frame t+1's grid.  With bwd_reversed = 0 pair t's backward field is bwd[t], with bwd_reversed = 1 it is
 * bwd[npair-1-t]: what the flow engine leaves when it is run over the clip with its frames in reverse order.
 * Q(u) = llrint((double)u * 65536).  A vector is valid exactly as the camera and blob blocks have it: u, v finite and
 * |u|, |v| < 1024.  For pixel (x, y) of pair t with a valid forward vector, X = x*65536 + Q(u), Y = y*65536 + Q(v).
 * Landing: the pixel lands inside iff 0 <= X <= (W-1) << 16 and 0 <= Y <= (H-1) << 16.  ix = X >> 16, fx = X & 65535, iy and
 * fy likewise.  The four taps are (ix, iy), (min(ix+1, W-1), iy), (ix, min(iy+1, H-1)), (min(ix+1, W-1), min(iy+1, H-1)) with
 * the weights (65536-fx)(65536-fy), fx(65536-fy), (65536-fx)fy, fx*fy (they sum to 2^32); all four taps must be valid
 * vectors of the backward field.
 * Interpolated backward vector, per component: S = sum of w_i * Q(b_i) in int64 (|S| <= 2^58), B = (S + 2^31) >> 32 with an
 * arithmetic shift.  Residual e = (Q(u) + Bx, Q(v) + By); d2 = ex^2 + ey^2; m2 = Q(u)^2 + Q(v)^2 + Bx^2 + By^2.
 * Verdict: consistent iff d2 <= (m2 >> 16) * alpha_q + beta_q, which is |f + b|^2 <= alpha (|f|^2 + |b|^2) + beta with
 * alpha = alpha_q / 65536 and beta = beta_q / 2^32 px^2.  alpha_q in 0 .. 65536, beta_q in 0 .. 2^62; nothing overflows
 * int64 (d2 < 2^55, the right side < 2^54 + 2^62).
 * Outputs: state u8 [npair][H][W], one of the four OFC_CONSIST_* below, decided in this order: the forward vector is
 * invalid -> INVALID; it lands outside -> LEAVES; a tap is invalid -> INVALID; else the comparison.  counts int64
 * [npair][4]: the pixels of the pair in each state.  Optionally resid int32 [npair][H][W][2]: e for the states CONSISTENT
 * and MISMATCH, zero otherwise.
 * Limits: W, H in 1 .. 16384, so that X and Y fit int32 (above: OFC_EUNSUPPORTED); npair in 1 .. 65535, alpha_q and beta_q
 * in their ranges, bwd_reversed 0 or 1 (otherwise, and for W, H < 1: OFC_EINVAL). ---- */
#define OFC_CONSIST_OK 0        /* consistent */
#define OFC_CONSIST_MISMATCH 1  /* the two fields do not cancel */
#define OFC_CONSIST_LEAVES 2    /* the pixel leaves the frame */
#define OFC_CONSIST_INVALID 3   /* the forward vector is invalid, or the pixel lands inside and a tap is invalid */
#define OFC_CONSIST_STATES 4
#define OFC_CONSIST_SHARE 2048  /* consecutive pixels of a pair a work-group of the check kernel takes */
#define OFC_CONSIST_MAX_DIM 16384
#define OFC_CONSIST_ALPHA_MAX 65536
#define OFC_CONSIST_BETA_MAX ((int64_t)1 << 62)
/* Host only, no device is touched: OFC_OK iff the arguments are inside the limits above.  Every call below decides by it
 * before anything is allocated or launched.  No counterpart in the reference, as for every call of this block. */
int ofc_consist_check(int W, int H, int npair, int64_t alpha_q, int64_t beta_q);
/* fwd_dev, bwd_dev f32 [npair][H][W][2] (8-byte aligned; the forward field is read with 16-byte loads where every pair's
 * base allows) -> state_dev u8 [npair][H][W], counts_dev int64 [npair][4] (8-byte aligned; cleared here), and resid_dev int32
 * [npair][H][W][2] (8-byte aligned) unless it is NULL.  Every tap index is clamped into the frame before it indexes
 * anything, whatever the fields hold.  Neither field is written.  Returns when done. */
int ofc_consist_dev(int device, const float *fwd_dev, const float *bwd_dev, int W, int H, int npair, int bwd_reversed,
                    int64_t alpha_q, int64_t beta_q, uint8_t *state_dev, int64_t *counts_dev, int32_t *resid_dev);
/* The whole chain on host buffers of the same shapes; resid_host may be NULL. */
int ofc_consist(int device, const float *fwd_host, const float *bwd_host, int W, int H, int npair, int bwd_reversed,
                int64_t alpha_q, int64_t beta_q, uint8_t *state_host, int64_t *counts_host, int32_t *resid_host);
/* state_dev u8 [n] and a set `keep` of states (bit s = state s, 0 .. 15): where bit state[p] of keep is clear (a byte above 3
 * is in no set), keys_dev[p] = 255 (the background of a blob key map) and w_dev[p] = 0.0f (a sample weight); everything else
 * is left as it is.  keys_dev u8 [n] and w_dev f32 [n] (4-byte aligned) may each be NULL; 16 elements per lane where all
 * bases given are 16-byte aligned, with a scalar tail.  n >= 1.  Returns when done. */
int ofc_consist_mask_dev(int device, const uint8_t *state_dev, int64_t n, int keep, uint8_t *keys_dev, float *w_dev);
/* frames_dev u8 [n_frames][H][W] -> out_dev of the same shape with the frames in reverse order (out[i] = frames[n-1-i]);
 * the two must not overlap.  W, H >= 1, n_frames in 1 .. 65536.  Returns when done. */
int ofc_frames_reverse_dev(int device, const uint8_t *frames_dev, int W, int H, int n_frames, uint8_t *out_dev);
/* Measurement hook: average duration by HIP events over `iters` runs, two warm-up runs before them, on fwd_dev and bwd_dev
 * (bwd_reversed 0, alpha_q 655, beta_q 2^31) with outputs of the hook's own.  what = 0: the check without the residual (the
 * clear of the counts included); 1: the check with it; 2: the mask on a key map and a weight array, keep = {0}, after one
 * untimed check. */
int ofc_bench_consist(int device, const float *fwd_dev, const float *bwd_dev, int W, int H, int npair, int what, int iters,
                      float *ms_per_run);

/* ---- Photometric consistency: which vectors of a field carry a pixel of frame t onto a like grey value of frame t+1
 * (brightness constancy).  It needs no backward field, only the u8 frames the field was computed from, so it also exists on
 * a stream; it says little where the image has no texture, so it complements the forward-backward check and does not
 * replace it.  The reference has no counterpart: it trusted every vector of cv2.calcOpticalFlowFarneback alike
 * (computeOpticalFlowModule.py:20-22).
 * Definition (normative, like the text above; every output is an integer).
 * Inputs: frames u8 [npair+1][H][W]; pair t is I0 = frames[t], I1 = frames[t+1].  fwd f32 [npair][H][W][2], pair t on frame
 * t's grid.
 * Quantisation and landing are exactly the forward-backward check's: Q(u) = llrint((double)u * 65536); a vector is valid
 * iff u, v are finite and |u|, |v| < 1024; X = x*65536 + Q(u), Y = y*65536 + Q(v); the pixel lands inside iff
 * 0 <= X <= (W-1) << 16 and 0 <= Y <= (H-1) << 16.  ix = X >> 16, fx = X & 65535, iy and fy likewise.  The four taps are
 * (ix, iy), (min(ix+1, W-1), iy), (ix, min(iy+1, H-1)), (min(ix+1, W-1), min(iy+1, H-1)) with the weights
 * (65536-fx)(65536-fy), fx(65536-fy), (65536-fx)fy, fx*fy (they sum to 2^32).
 * Warped intensity: S = sum of w_i * I1(tap_i) in 64-bit integers, 0 <= S <= 255 * 2^32 < 2^40; J = (S + 2^23) >> 24, in
 * 0 .. 65280: the grey value in 1/256 levels.  An implementation may form S as top*(65536-fy) + bot*fy with
 * top = I00*(65536-fx) + I10*fx < 2^24: that is the same integer.  No intermediate may be rounded.
 * Residual and contrast: e = J - 256 * I0(x, y); c = max - min of the four tap values of I1, in 0 .. 255.  A tap of weight
 * zero counts: nothing may depend on a fraction being exactly 0.
 * Verdict: consistent iff |e| <= tau_q + kappa_q * c, with tau_q in 0 .. 65280 (1/256 grey levels) and kappa_q in 0 .. 1024
 * (1/256 grey levels of residual per grey level of local contrast: it forgives the sub-pixel error of a vector that sits on
 * an edge).  Everything fits int32.
 * Outputs: state u8 [npair][H][W] with the forward-backward check's codes OFC_CONSIST_*, decided in this order: the forward
 * vector is invalid -> INVALID (3); the pixel lands outside -> LEAVES (2); else the comparison, OK (0) or MISMATCH (1).
 * stats int64 [npair][5]: the pixels of the pair in each of the four states, then the sum of |e| over the pixels of states 0
 * and 1 (below 2^44).  Optionally warped u16 [npair][H][W]: J for the states 0 and 1, and 0 otherwise.
 * Limits: W, H in 1 .. 16384 (above: OFC_EUNSUPPORTED; below 1: OFC_EINVAL); npair in 1 .. 65535, tau_q and kappa_q in their
 * ranges (otherwise OFC_EINVAL). ---- */
#define OFC_PHOTO_SHARE 2048     /* consecutive pixels of a pair a work-group of the check kernel takes */
#define OFC_PHOTO_TAU_MAX 65280
#define OFC_PHOTO_KAPPA_MAX 1024
#define OFC_PHOTO_NSTAT 5
/* Host only, no device is touched: OFC_OK iff the arguments are inside the limits above.  Every call below decides by it
 * before anything is allocated or launched.  No counterpart in the reference, as for every call of this block. */
int ofc_photo_check(int W, int H, int npair, int tau_q, int kappa_q);
/* frames_dev u8 [npair+1][H][W], fwd_dev f32 [npair][H][W][2] (8-byte aligned; read with 16-byte loads where every pair's
 * base allows) -> state_dev u8 [npair][H][W], stats_dev int64 [npair][5] (8-byte aligned; cleared here), and warped_dev u16
 * [npair][H][W] (2-byte aligned) unless it is NULL.  Every tap index is clamped into the frame before it indexes anything,
 * whatever the field holds.  Neither input is written.  Returns when done.  No counterpart in the reference. */
int ofc_photo_dev(int device, const uint8_t *frames_dev, const float *fwd_dev, int W, int H, int npair, int tau_q, int kappa_q,
                  uint8_t *state_dev, int64_t *stats_dev, uint16_t *warped_dev);
/* The whole chain on host buffers of the same shapes; warped_host may be NULL.  No counterpart in the reference. */
int ofc_photo(int device, const uint8_t *frames_host, const float *fwd_host, int W, int H, int npair, int tau_q, int kappa_q,
              uint8_t *state_host, int64_t *stats_host, uint16_t *warped_host);
/* Measurement hook: average duration by HIP events over `iters` runs, two warm-up runs before them, on frames_dev and
 * fwd_dev (tau_q 2048, kappa_q 128) with outputs of the hook's own, the clear of the stats included.  what = 0: the check
 * alone; 1: the check with `warped`.  No counterpart in the reference. */
int ofc_bench_photo(int device, const uint8_t *frames_dev, const float *fwd_dev, int W, int H, int npair, int what, int iters,
                    float *ms_per_run);
/* A stream that checks its vectors photometrically: from the next batch on, every pair of a batch is checked against the
 * slot's own frames directly behind the flow and BEFORE the camera (if any) is fitted and subtracted (a residual does not
 * say where a pixel lands: the rule the link moves follow); the stats go to a row per pair.  On a stream with blobs every
 * pixel whose state is not in `keep` (a set of states as for ofc_consist_mask_dev, 1 .. 15) becomes background of the key map
 * before the components are found; the links' moves are left alone.  on = 0 removes the check: the stream then launches
 * exactly what a stream that never had one launches.  Same precondition as ofc_stream_set_blobs (no frame and no
 * undelivered result; otherwise OFC_EINVAL and nothing changes); tau_q, kappa_q as ofc_photo_check decides them for the
 * stream's frame size.  No counterpart in the reference. */
int ofc_stream_set_photo(ofc_stream_t *s, int on, int tau_q, int kappa_q, int keep);
/* The stats [n][5] of the n pairs the LAST finish delivered.  Valid under ofc_stream_read_blobs' conditions; max_pairs < n:
 * OFC_EINVAL, nothing written; OFC_EINVAL without the check.  No counterpart in the reference. */
int ofc_stream_read_photo(ofc_stream_t *s, int64_t *stats_host, int max_pairs);
/* A stream that checks its vectors forward-backward: from the next batch on, a batch's flow comes from
 * ofc_flow_calc_frames_dev_bidir (both directions from one front end; the backward pair of a transition across two batches is
 * in the later batch, which carries the earlier frame), and every pair is checked as ofc_consist_dev does with bwd_reversed
 * = 0, directly behind the flow and BEFORE the repair, the moves and the camera; the counts go to a row per pair.  The state
 * map then plays the role the photometric check's plays: the repair takes and updates it, and on a stream with blobs every
 * pixel whose state is not in `keep` (1 .. 15) becomes background of the key map.  The stream keeps ONE state map: with the
 * photometric check on, turning this one on is refused with OFC_EINVAL, and the other way round.  on = 0 removes the check and
 * frees its buffers (a state map and a backward field of one batch).  Same precondition as ofc_stream_set_photo; alpha_q,
 * beta_q as ofc_consist_check decides them for the stream's frame size.  No counterpart in the reference. */
int ofc_stream_set_consist(ofc_stream_t *s, int on, int64_t alpha_q, int64_t beta_q, int keep);
/* The counts [n][4] of the n pairs the LAST finish delivered.  Valid under ofc_stream_read_photo's conditions; max_pairs < n:
 * OFC_EINVAL, nothing written; OFC_EINVAL without the check.  No counterpart in the reference. */
int ofc_stream_read_consist(ofc_stream_t *s, int64_t *counts_host, int max_pairs);

/* ---- Repair of a flow field: a masked median fill of the vectors that are not trusted, and a median smoothing pass.  What
 * the two checks above flag can so far only be thrown away; here a flagged vector is replaced by the component-wise median
 * of the trusted vectors around it, round after round, until the hole is closed.  A median only selects, so every result is
 * exact and does not depend on the order of the work.  The reference has no counterpart: it trusted every vector of
 * cv2.calcOpticalFlowFarneback alike (computeOpticalFlowModule.py:20-22).
 * Definition (normative, like the text above).
 * Inputs: flow f32 [npair][H][W][2]; state u8 [npair][H][W] or NULL; keep, a set of states as for ofc_consist_mask_dev (bit
 * s = state s), 1 .. 15; radius r in {1, 2}: a window of 3x3 or 5x5; rounds in 0 .. 254; min_count in 1 .. (2r+1)^2; smooth
 * in {0, 1}; rounds == 0 && smooth == 0 is refused.
 * Sources and targets: a vector is valid exactly as everywhere else: u, v finite and |u|, |v| < 1024.  Pixel p is a source
 * iff its vector is valid and either state is NULL or bit state[p] of keep is set (a state byte above 3 is in no set).
 * Every other pixel is a target.  V_0 is the set of sources, F_0 the input field.
 * Round g = 1 .. rounds (Jacobi: a round reads only the snapshot F_(g-1), V_(g-1)): for every pixel p not in V_(g-1), let N
 * be the pixels q with |qx - px| <= r and |qy - py| <= r that lie inside the frame and in V_(g-1); the window is clipped at
 * the border, nothing is reflected, and pairs never see one another.  If |N| >= min_count: F_g[p].u is the lower median of
 * {F_(g-1)[q].u : q in N}, the element of index floor((|N| - 1) / 2) in ascending order; F_g[p].v likewise over the v
 * components, chosen independently of u; p joins V_g; filled[p] = g.  Everything else is carried over unchanged.
 * Smoothing, if smooth is set, runs after the last round: for every p in V_rounds the output is the lower median, per
 * component, over the window's pixels in V_rounds (p itself always among them), read from the snapshot F_rounds; min_count
 * does not apply; pixels outside V_rounds and the filled map are not touched by it.
 * Outputs: out f32 of flow's shape.  A source when smooth is 0, and a target that was never filled always, are copied bit
 * for bit from the input.  A filled or smoothed component equals, as a number, one of the input components of its pair;
 * which sign a zero carries is not promised (compare with ==, not by bytes).  filled u8 [npair][H][W], optional: 0 for a
 * source, g for a target filled in round g, 255 for a target never filled.  counts int64 [npair][3]: sources, filled,
 * unfilled; they sum to W*H.  state_out u8 [npair][H][W], optional, may be the same buffer as state: the input state
 * carried over, filled targets become OFC_CONSIST_OK; it is written only once nothing reads state any more; with state NULL
 * it must be NULL.
 * Aliasing: out may be the same buffer as flow (in place), otherwise the two must not overlap.  The library owns the
 * scratch of the snapshots and works through the pairs in chunks, so that scratch does not grow with npair.
 * Limits: W, H in 1 .. 16384 (above: OFC_EUNSUPPORTED); npair in 1 .. 65535; anything else outside the ranges above:
 * OFC_EINVAL.
 * Safety: no index is formed from data; every neighbour index is clamped or predicated into the frame; no loop has a
 * data-dependent trip count. ---- */
#define OFC_REPAIR_TILE_W 64      /* the pixels of a frame a work-group of the sweep kernel takes: what ofc_repair_tile says */
#define OFC_REPAIR_TILE_H 16
#define OFC_REPAIR_ROUNDS_MAX 254
#define OFC_REPAIR_NCOUNT 3
#define OFC_REPAIR_UNFILLED 255   /* filled[p] of a target that no round filled */
/* Host only, no device is touched: OFC_OK iff the arguments are inside the limits above.  Every call below decides by it
 * before anything is allocated or launched.  No counterpart in the reference, as for every call of this block. */
int ofc_repair_check(int W, int H, int npair, int keep, int radius, int rounds, int min_count, int smooth);
/* Host only: out[0], out[1] = the width and height of the tile of a frame that one work-group of the sweep kernel takes at
 * this radius, so that a test can place holes on its seams. */
void ofc_repair_tile(int radius, int out[2]);
/* flow_dev f32 [npair][H][W][2] (8-byte aligned; read with 16-byte loads where W is even and the base allows), state_dev u8
 * [npair][H][W] or NULL -> out_dev of flow's shape (8-byte aligned; flow_dev itself, or disjoint from it), counts_dev int64
 * [npair][3] (8-byte aligned; cleared here), and filled_dev, state_out_dev u8 [npair][H][W] unless they are NULL
 * (state_out_dev may be state_dev).  rounds + smooth sweeps over the field, in scratch of the library's own.  Returns when
 * done. */
int ofc_repair_dev(int device, const float *flow_dev, const uint8_t *state_dev, int W, int H, int npair, int keep, int radius,
                   int rounds, int min_count, int smooth, float *out_dev, uint8_t *filled_dev, uint8_t *state_out_dev,
                   int64_t *counts_dev);
/* The whole chain on host buffers of the same shapes; state_host, filled_host and state_out_host may be NULL. */
int ofc_repair(int device, const float *flow_host, const uint8_t *state_host, int W, int H, int npair, int keep, int radius,
               int rounds, int min_count, int smooth, float *out_host, uint8_t *filled_host, uint8_t *state_out_host,
               int64_t *counts_host);
/* Measurement hook: average duration by HIP events over `iters` runs, two warm-up runs before them, on flow_dev and
 * state_dev (may be NULL; keep = {0}, min_count 1) with outputs of the hook's own, the clear of the counts included.
 * what = 0: one fill round, r = 1; 1: one smoothing pass, r = 1; 2: one smoothing pass, r = 2. */
int ofc_bench_repair(int device, const float *flow_dev, const uint8_t *state_dev, int W, int H, int npair, int what, int iters,
                     float *ms_per_run);
/* A stream that repairs its vectors: from the next batch on, every batch's field is repaired in place directly behind the
 * photometric check, whose state map it takes and updates (filled pixels become OFC_CONSIST_OK, so on a stream with blobs
 * they belong to blobs again and pixels that stayed unfilled do not); without a photometric check state is NULL and only
 * invalid vectors are targets.  It runs before the link moves are taken and before the camera is fitted (a repaired vector
 * says where a pixel lands), so everything downstream sees the repaired field.  The counts go to a row per pair.  on = 0
 * removes it: the stream then launches exactly what a stream that never had one launches.  Preconditions exactly as
 * ofc_stream_set_photo; the arguments as ofc_repair_check decides them for the stream's frame size. */
int ofc_stream_set_repair(ofc_stream_t *s, int on, int keep, int radius, int rounds, int min_count, int smooth);
/* The counts [n][3] of the n pairs the LAST finish delivered.  Valid under ofc_stream_read_photo's conditions; max_pairs < n:
 * OFC_EINVAL, nothing written; OFC_EINVAL without the repair. */
int ofc_stream_read_repair(ofc_stream_t *s, int64_t *counts_host, int max_pairs);

/* ---- Trajectories: points followed through a clip's flow fields (dense trajectories, particle advection).  Every other
 * temporal object of the library is a vote on whole-pixel moves between two label maps (the blob links); here a point
 * placed anywhere is carried from pair to pair by the bilinearly interpolated flow at its sub-pixel position, until it
 * leaves the frame or the vector under it cannot be trusted.  The reference has no counterpart: its motion signature over
 * time was a per-cell mean (drawGridsAndOutputCSV.py), it never followed a point.
 * Definition (normative, like the text above; every output is an integer and does not depend on the order of the work).
 * Inputs: flow f32 [npair][H][W][2]; seeds int32 [P][2] holding (X, Y) in 1/65536 px, any int32 allowed; optionally state
 * u8 [npair][H][W] with a set `keep` (bit s = state s) as ofc_consist_mask_dev reads it.  Q(u) and "valid vector" are
 * exactly the consistency block's: u, v finite, |u|, |v| < 1024, Q(u) = llrint((double)u * 65536).
 * Step t = 0 .. npair-1 of a live point at (X, Y), decided in this order:
 * 1. The point is inside iff 0 <= X <= (W-1) << 16 and 0 <= Y <= (H-1) << 16.  If it is not, it ends with OFC_TRAJ_LEAVES
 *    (only a seed at t = 0 can: rule 4 keeps every later position inside).
 * 2. With a state map: rx = (X + 32768) >> 16, ry = (Y + 32768) >> 16, the nearest pixel, inside by rule 1;
 *    s = state[t][ry][rx]; if s > 3 or bit s of keep is clear, the point ends with OFC_TRAJ_UNTRUSTED.
 * 3. ix = X >> 16, fx = X & 65535, iy and fy likewise.  The four taps of flow[t] are (ix, iy), (min(ix+1, W-1), iy),
 *    (ix, min(iy+1, H-1)), (min(ix+1, W-1), min(iy+1, H-1)) with the weights (65536-fx)(65536-fy), fx(65536-fy),
 *    (65536-fx)fy, fx*fy (they sum to 2^32).  If any of the four is not a valid vector (whatever its weight), the point ends
 *    with OFC_TRAJ_INVALID.
 * 4. Per component S = sum of w_i * Q(f_i) in int64 (|S| <= 2^58), D = (S + 2^31) >> 32 with an arithmetic shift;
 *    X' = X + Dx, Y' = Y + Dy (int32: X < 2^30, |D| < 2^26).  If (X', Y') is not inside, the point ends with
 *    OFC_TRAJ_LEAVES and does not move; otherwise it moves there and the step counts.
 * Outputs: pos int32 [npair+1][P][2], time-major: pos[0] is the seeds, pos[t+1][p] the position after step t if that step
 * was taken and pos[t][p] otherwise (an ended point stays where it ended).  len int32 [P]: the steps taken, 0 .. npair.  why u8
 * [P]: one of the OFC_TRAJ_* below; they are the consistency states' own numbers wherever they mean the same thing.
 * Limits: W, H in 1 .. 16384 (above: OFC_EUNSUPPORTED); npair in 1 .. 65535; P in 1 .. 2^28; keep in 0 .. 65535;
 * pairs_per_launch >= 0; everything else OFC_EINVAL.
 * Safety: every index, the state byte's and the taps of ended points included, is clamped into the frame before it indexes
 * anything, whatever seeds and fields hold; no loop has a data-dependent trip count. ---- */
#define OFC_TRAJ_RAN 0        /* the point took all npair steps */
#define OFC_TRAJ_UNTRUSTED 1  /* the state under it is not in keep */
#define OFC_TRAJ_LEAVES 2     /* it is, or would land, outside the frame */
#define OFC_TRAJ_INVALID 3    /* one of the four taps is not a valid vector */
#define OFC_TRAJ_THREADS 256  /* points a work-group of the kernel takes */
#define OFC_TRAJ_MAX_POINTS (1 << 28)
#define OFC_TRAJ_ONE_LAUNCH_POINTS (1 << 19)  /* the cost model: up to this many points all pairs go into one launch ... */
#define OFC_TRAJ_DENSE_PAIRS 16               /* ... and above it this many pairs per launch (see ofc_traj_launch_geometry) */
/* Host only, no device is touched: OFC_OK iff the arguments are inside the limits above.  Every call below decides by it
 * before anything is allocated or launched.  No counterpart in the reference, as for every call of this block. */
int ofc_traj_check(int W, int H, int npair, int64_t P, int keep, int pairs_per_launch);
/* Host only: how ofc_traj_dev cuts the pairs into launches when pairs_per_launch is 0.  out[0] = the pairs per launch (the
 * last launch takes what is left), out[1] = the work-groups per launch (ceil(P / OFC_TRAJ_THREADS)), out[2] = the launches
 * (ceil(npair / out[0])), out[3] = the lanes per work-group.  The model: a launch keeps a point's position in registers
 * over its pairs, so with few points (P <= OFC_TRAJ_ONE_LAUNCH_POINTS, the lanes the device holds at once) one launch over
 * all pairs saves npair - 1 launches of a latency-bound loop; with more points than that the work-groups come in rounds and
 * out[0] = min(npair, OFC_TRAJ_DENSE_PAIRS).  Measured on the MI355X at 1920x1080 x 16 pairs, longer chunks were
 * faster up to 16 pairs in both regimes; no longer chunk was timed with dense seeds, so that is where the constant stands.  The result of ofc_traj_dev is the same bits for every choice.  Refusals as
 * ofc_traj_check (keep 0, pairs_per_launch 0), and OFC_EINVAL for out NULL.  No counterpart in the reference. */
int ofc_traj_launch_geometry(int W, int H, int npair, int64_t P, int out[4]);
/* flow_dev f32 [npair][H][W][2] (8-byte aligned), state_dev u8 [npair][H][W] or NULL, seeds_dev int32 [P][2] -> pos_dev int32
 * [npair+1][P][2] (8-byte aligned), len_dev int32 [P] (4-byte aligned), why_dev u8 [P].  pairs_per_launch 0: as
 * ofc_traj_launch_geometry says; a positive value forces the chunk, one above npair means npair.  Between launches the
 * table is the carry: a point is live at step t iff len[p] == t.  seeds_dev may be row 0 of pos_dev (then nothing is
 * copied); otherwise it must not overlap pos_dev.  Neither input is written.  Returns when done.  No counterpart in the
 * reference. */
int ofc_traj_dev(int device, const float *flow_dev, const uint8_t *state_dev, int W, int H, int npair, const int32_t *seeds_dev,
                 int64_t P, int keep, int pairs_per_launch, int32_t *pos_dev, int32_t *len_dev, uint8_t *why_dev);
/* The whole chain on host buffers of the same shapes; state_host may be NULL.  No counterpart in the reference. */
int ofc_traj(int device, const float *flow_host, const uint8_t *state_host, int W, int H, int npair, const int32_t *seeds_host,
             int64_t P, int keep, int pairs_per_launch, int32_t *pos_host, int32_t *len_host, uint8_t *why_host);
/* Measurement hook: average duration by HIP events over `iters` runs of the whole chain (the clears of len and why, the copy
 * of the seeds, every launch), two warm-up runs before them, on flow_dev and seeds_dev without a state map, with outputs of
 * the hook's own that are allocated before the timed region.  No counterpart in the reference. */
int ofc_bench_traj(int device, const float *flow_dev, int W, int H, int npair, const int32_t *seeds_dev, int64_t P,
                   int pairs_per_launch, int iters, float *ms_per_run);
/* A stream that follows points: the P seeds (int32 [P][2], copied here) are placed at the first pair after this call or
 * after a finish, and every batch's advection runs directly behind the repair and BEFORE the moves and the camera (a point
 * lands by the WHOLE flow: the rule of the moves), one launch per batch; the last row written is the carry into the next
 * batch.  use_state != 0: a point ends where the state map of the stream's check (photometric or forward-backward, as the
 * repair left it) is not in that check's keep; without a check on the stream OFC_EINVAL.  P = 0 removes the stage: the
 * stream then launches exactly what a stream that never had one launches.  Same precondition as ofc_stream_set_photo; P as
 * ofc_traj_check decides it for the stream's frame size.  A check that is removed while use_state is set makes the next
 * batch fail with OFC_EINVAL.  No counterpart in the reference. */
int ofc_stream_set_traj(ofc_stream_t *s, int64_t P, const int32_t *seeds_host, int use_state);
/* pos [n+1][P][2], len [P], why [P] of the n pairs the LAST finish delivered (a finish ends the clip: the next clip starts
 * from the seeds again).  Valid under ofc_stream_read_photo's conditions; max_pairs < n: OFC_EINVAL, nothing written;
 * OFC_EINVAL without the stage.  A why of OFC_TRAJ_RAN says the point was still live when the clip ended.  No counterpart in
 * the reference. */
int ofc_stream_read_traj(ofc_stream_t *s, int32_t *pos_host, int32_t *len_host, uint8_t *why_host, int max_pairs);

/* ---- Tracklets: dense trajectories with reseeding.  The block above carries a fixed set of points from the first pair to
 * the last, so the set thins out and describes only what was visible at frame 0.  Here a pool of tracks is kept on the device:
 * every frame each grid cell without a live point in it gets a new one, and a track is cut after L steps, so that drift does
 * not accumulate and all descriptors have one length (the two remaining parts of the dense-trajectories method).  The
 * reference has no counterpart.
 * Definition (normative; every output is an integer and does not depend on the order of the work).
 * Inputs: flow f32 [npair][H][W][2]; optionally state u8 [npair][H][W] with a set `keep`, both as in the block above; `cell`,
 * the side of a square grid cell in whole px; max_len = L; max_tracks = M.
 * Grid: cols = ceil(W / cell), rows = ceil(H / cell); cell (cx, cy) has the index cy * cols + cx; the cell of a position is
 * ((X >> 16) / cell, (Y >> 16) / cell).  The seed of a cell is its centre clamped into the frame:
 * X0 = min(((cx * cell) << 16) + (cell << 15), (W-1) << 16), Y0 likewise with cy and H.
 * A track is live while it has not ended and has taken fewer than L steps.  `used` starts at 0.
 * For frame t = 0 .. npair-1, in this order:
 * 1. Occupancy.  A cell is occupied iff at least one track that is live before this frame's births has its current position
 *    in it.
 * 2. Births.  Take the unoccupied cells in increasing cell index.  With a state map, drop those whose seed's nearest pixel
 *    (rx, ry of rule 2 above, at (X0, Y0)) has a state s = state[t][ry][rx] with s > 3 or bit s of keep clear: blocked[t]
 *    counts them.  The cells left are empty[t]; born[t] = min(empty[t], M - used); the first born[t] of them, in cell-index
 *    order, get the track ids used, used+1, ..: birth = t, pos[0] = the seed, len = 0, why = OFC_TRAJ_RAN.  Then
 *    used += born[t].
 * 3. Step.  Every live track, the newborn included, takes exactly the step of the block above (rules 1-4, the same
 *    quantisation, the same order of reasons) with flow[t] and state[t].  A step that is taken stores the new position in
 *    pos[len+1] and increments len; a track whose len reaches L then ends with OFC_TRAJ_FULL.  A step that is not taken
 *    ends the track with that block's reason.
 * Outputs: pos int32 [L+1][M][2], step-major: pos[k][id] is track id's position after k steps; rows above a track's len, and
 * all rows of ids >= used, hold (-1, -1) (no inside position is negative).  birth int32 [M]: the frame of the birth, -1 for
 * unused ids.  len int32 [M]: the steps taken, 0 .. L; 0 for unused ids.  why u8 [M]: OFC_TRAJ_* (OFC_TRAJ_RAN: still live
 * when the clip ended), 255 for unused ids.  frames int32 [npair][3]: empty, born, blocked of every frame.  used is the sum
 * of born; born[t] < empty[t] is how a caller sees that the pool ran out, and nothing else changes then.
 * Limits: W, H as ofc_traj_check; npair 1 .. 65535; cell 1 .. 16384; rows * cols <= 2^24; max_len 1 .. 4096; max_tracks
 * 1 .. 2^28; keep 0 .. 65535; everything else OFC_EINVAL; then (max_len + 1) * max_tracks >= 2^31 is OFC_EUNSUPPORTED.
 * Safety: every index is formed from a clamped position, a clamped cell index or a clamped id, whatever the fields hold; no
 * loop has a data-dependent trip count; no work-group waits for another.
 * Launches: the clears, then three kernels per frame (count and scan of the empty cells; assignment of the newborn; the
 * step); the host reads nothing back and does not synchronise between frames. ---- */
#define OFC_TRAJ_FULL 4                     /* the track took max_len steps */
#define OFC_TRACKLET_THREADS 256            /* cells, or track ids, a work-group of the three kernels takes */
#define OFC_TRACKLET_MAX_LEN 4096
#define OFC_TRACKLET_MAX_TRACKS (1 << 28)
/* Host only, no device is touched: OFC_OK iff the arguments are inside the limits above.  Every call below decides by it
 * before anything is allocated or launched.  No counterpart in the reference, as for every call of this block. */
int ofc_tracklets_check(int W, int H, int npair, int cell, int max_len, int64_t max_tracks, int keep);
/* flow_dev f32 [npair][H][W][2] (8-byte aligned), state_dev u8 [npair][H][W] or NULL -> pos_dev int32 [max_len+1][max_tracks][2]
 * (8-byte aligned), birth_dev and len_dev int32 [max_tracks], why_dev u8 [max_tracks], frames_dev int32 [npair][3] (4-byte
 * aligned).  The outputs must not overlap the inputs or each other.  The call allocates its scratch (the occupancy bitmap,
 * the counts of the scan, the table of `used` per frame) and frees it on every way out.  Neither input is written.  Returns
 * when done. */
int ofc_tracklets_dev(int device, const float *flow_dev, const uint8_t *state_dev, int W, int H, int npair, int cell, int max_len,
                      int64_t max_tracks, int keep, int32_t *pos_dev, int32_t *birth_dev, int32_t *len_dev, uint8_t *why_dev,
                      int32_t *frames_dev);
/* The whole chain on host buffers of the same shapes; state_host may be NULL. */
int ofc_tracklets(int device, const float *flow_host, const uint8_t *state_host, int W, int H, int npair, int cell, int max_len,
                  int64_t max_tracks, int keep, int32_t *pos_host, int32_t *birth_host, int32_t *len_host, uint8_t *why_host,
                  int32_t *frames_host);
/* Measurement hook: average duration by HIP events over `iters` runs of the whole chain (the clears and every launch), two
 * warm-up runs before them, on flow_dev without a state map, with outputs and scratch of the hook's own that are allocated
 * before the timed region and freed when it returns. */
int ofc_bench_tracklets(int device, const float *flow_dev, int W, int H, int npair, int cell, int max_len, int64_t max_tracks, int iters,
                        float *ms_per_run);

/* ------------------------------------------------------------------------------------------
 * Downstream consumer of the hue CSVs (findCosineDifferentVectors.py:5-61): cosine similarity between
 * `small` (n_small values) and every window large[i : i+n_small], i = 0 .. n_large-n_small.
 * sims has n_large-n_small+1 entries; 0 where either norm is 0.  Integer-valued input (the hue columns) is summed exactly
 * in 64-bit integers as long as n_small * max(|small|, |large|)^2 < 2^63; larger integers and non-integer input are
 * summed in f64, each of the three sums to n_small * 2^-53 relative.
 * ------------------------------------------------------------------------------------------ */
int ofc_sliding_cosine(int device, const double *small_v, int n_small, const double *large_v, int n_large,
                       double *sims);

/* ---- synthetic input generator used by bench.py (not part of the reference path) ----
 * At most 65535 frames per call and 65535 rows per frame (OFC_EUNSUPPORTED, decided before any launch). */
int ofc_synth_frames_dev(int device, uint8_t *frames_dev, int W, int H, int n_frames,
                         int t0, int seed);

#ifdef __cplusplus
}
#endif
#endif /* OFC_H */
