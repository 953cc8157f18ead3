// flow_host.h -- host-side interface of the Farneback flow kernels: the level geometry and expansion constants
// (ofc_api.cpp), the launchers of flow_pyramid.hip, flow_polyexp.hip, flow_solve.hip, flow_iter.hip and
// flow_experiments.hip, and the checks the engine asks before it allocates.
#pragma once
#include "ofc_common.h"

namespace ofc {

// ---- Farneback level geometry (host) -- SURVEY.md App. A.1 ----
struct LevelGeom {
    int w, h, ksize;
    double sigma;
};
int pyramid_levels(int W, int H, const ofc_fb_params &p);
LevelGeom level_geometry(int W, int H, const ofc_fb_params &p, int k);
void gaussian_kernel(int n, double sigma, float *k);           // getGaussianKernel, CV_32F
struct PolyConsts {
    int n;                                  // poly_n: the launchers dispatch on it (5 and 7 are built)
    float g[8], xg[8], xxg[8];
    double ig11, ig03, ig33, ig55;
};
void polyexp_setup(int n, double sigma, PolyConsts &c);        // FarnebackPrepareGaussian
// the frame size and the Farneback parameters every flow entry point accepts: OFC_OK, or OFC_EINVAL / OFC_EUNSUPPORTED with the
// message set (an odd winsize above OFC_WINSIZE_MAX is refused here, an even one where a window is used)
int check_frame_and_fb_params(const ofc_fb_params &p, int W, int H);
int polyexp_n_check(int n);        // OFC_OK for the built poly_n (5, 7), else OFC_EUNSUPPORTED with the message set
constexpr int WINSIZE_WIDE_MIN = 19;   // launch_box_solve: this winsize and wider run k_box_solve_wide (up to OFC_WINSIZE_MAX)

// ---- kernel launchers : device pointers, asynchronous on `s` ----
// flow_pyramid.hip.  src: [nimg][H0][W0] u8 -> dst: [nimg][h][w] f32
int launch_level_image(const uint8_t *src, float *dst, int nimg, int W0, int H0,
                       const LevelGeom &g, hipStream_t s);
// what launch_level_image would refuse for this level (a blur wider than 31 taps, a tile beyond the LDS), with no launch
int level_image_check(int W0, int H0, const LevelGeom &g, bool src_aligned);
// levels 1..L of a batch in one launch (k_pyramid_dec): L = pyramid_dec_levels(...) says how many leading coarse levels
// (geom[1..levels], three at the most) are exact decimations by 2, 4, 8; dst[k-1] takes level k as launch_level_image writes it
int pyramid_dec_levels(int W0, int H0, const LevelGeom *geom, int levels, bool src_aligned);
void pyramid_dec_plan(int W0, int H0, int nimg, int &bands, int &steps, int &sps, int &strips);
int launch_pyramid_dec(const uint8_t *src, float *const *dst, int nimg, int W0, int H0, const LevelGeom *geom, int L,
                       hipStream_t s);
// flow_polyexp.hip.  level 0 fused into the polynomial expansion (frames u8 -> R), when the level is the plain 3x3 blur of the frame
bool polyexp_u8_ok(int W, int H, const LevelGeom &g);
int launch_polyexp_u8(const uint8_t *frames, float *R, int nimg, int W, int H, const PolyConsts &c, hipStream_t s);
// I: [nimg][H][W] f32 -> R: [nimg][H][W][5] f32 (pixel-interleaved)
int launch_polyexp(const float *I, float *R, int nimg, int W, int H, const PolyConsts &c,
                   int rows_per_block, hipStream_t s, bool bench_tag = false);
int polyexp_default_rows(int W, int H, int nimg);
// flow_solve.hip.  R0 = R + pair*strideR, R1 = R0 + strideR (consecutive frames, interleaved); flow [npair][H][W][2]; M [npair][5][H][W] planar
int launch_update_matrices(const float *R0, const float *R1, size_t pair_stride_R,
                           const float *flow, float *M, int npair, int W, int H, hipStream_t s);
int launch_box_solve(const float *M, float *flow, int npair, int W, int H, int winsize,
                     int rows_per_block, hipStream_t s);
int box_default_rows(int W, int H, int npair);
int box_wide_rows(int winsize);   // strip height of k_box_solve_wide
// src [npair][sh][sw][2] -> dst [npair][dh][dw][2], * mul
int launch_flow_resize(const float *src, float *dst, int npair, int sw, int sh, int dw, int dh,
                       float mul, hipStream_t s);
// flow_iter.hip.  launch geometry of the fused iteration over `fields` flow fields of a W x H level: strips `rows` high (a multiple of 16),
// tiles_x column tiles of 256 - (winsize - 1) columns, `grid` work-groups (the tiles of a field rounded up to groups of eight).
// rows 0: the height the kernel's cost model picks for this size and batch; a caller's height is rounded up to a multiple of 16
struct FlowIterGrid {
    int rows, tiles_x, strips, grid;
};
FlowIterGrid flow_iter_grid(int W, int H, int fields, int winsize, int rows = 0);
// the limits of the fused iteration that depend on the level's size and the window alone: OFC_OK or OFC_EUNSUPPORTED
int flow_iter_check(int W, int H, int winsize);
// the coarser level a level's first iteration starts from: the initial flow is resize(src [npair][sh][sw][2], (W,H)) * mul,
// sampled on the fly.  src null: flow_in is at this level's size
struct FlowCoarse {
    const float *src = nullptr;
    int sw = 0, sh = 0;
    float mul = 1.f;
};
// the column sums of the field an iteration writes: sum(u), sum(v) -> out[2], through `scratch` of `doubles` doubles (two per
// work-group; too few is OFC_EINVAL).  out null: none
struct FlowSums {
    double *out = nullptr, *scratch = nullptr;
    size_t doubles = 0;
};
// fused iteration (update matrices + box mean + solve): R [npair+1][5][H][W]; flow_in != flow_out
// rows_per_block: strip height as flow_iter_grid takes it (0 is what the engine passes); < 0 OFC_EINVAL
int launch_flow_iter(const float *R, size_t frame_stride_R, const float *flow_in, float *flow_out, int npair, int W, int H,
                     int winsize, hipStream_t s, const FlowCoarse &coarse = {}, const FlowSums &sums = {}, int rows_per_block = 0);
// one iteration of both directions of npair frame pairs in one launch; every buffer comes as its forward and its backward
// half ([npair] fields each, anywhere; coarse_bwd goes with coarse.src); strips are flow_iter_grid(W, H, 2 npair, winsize) high
int launch_flow_iter_bidir(const float *R, size_t frame_stride_R, const float *in_fwd, const float *in_bwd, float *out_fwd,
                           float *out_bwd, int npair, int W, int H, int winsize, hipStream_t s, const FlowCoarse &coarse = {},
                           const float *coarse_bwd = nullptr);
// the most work-groups launch_flow_iter starts for a level of this size at the model's height: sizes FlowSums::scratch
int flow_iter_max_grid(int W, int H, int npair, int winsize);
int launch_flow_iter_stamped(const float *R, size_t frame_stride_R, const float *flow_in, float *flow_out, int npair, int W,
                             int H, hipStream_t s, unsigned long long *dbg, int *grid_out);
// flow_experiments.hip.  two fused iterations flow_in -> flow_out (winsize 15; flow_in at this level's size, != flow_out); rows_per_block 0 = auto
int launch_flow_iter2(const float *R, size_t frame_stride_R, const float *flow_in, float *flow_out, int npair, int W,
                      int H, int winsize, hipStream_t s, int rows_per_block = 0);
// one iteration, 3-waves-per-SIMD form (winsize 15, flow_in at this level's size)
int launch_flow_iter_w3(const float *R, size_t frame_stride_R, const float *flow_in, float *flow_out, int npair, int W,
                        int H, int winsize, hipStream_t s, int rows_per_block = 0);
// round-3 experiment: k_flow_iter with the next step's gathers issued across the exchange (winsize 15)
int launch_flow_iter_pipe(const float *R, size_t frame_stride_R, const float *flow_in, float *flow_out, int npair, int W,
                          int H, const FlowIterGrid &g, hipStream_t s, const FlowSums &sums);

}  // namespace ofc
