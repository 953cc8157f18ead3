// grid_labels.hip -- what a clip-wide fit says about each grid cell: per (frame, cell, cluster) the number of pixels that
// carry the label, and optionally the sums of their flow vectors (ofc_grid_label_counts_dev).
//
// Grid geometry is overlayGridAndComputeAvgColor's (KmeanGrids.py:56-59), as k_grid_cell_mean_flow uses it: xs = W / cols,
// ys = H / rows, cell cy*cols+cx owns rows [cy*ys, (cy+1)*ys) x columns [cx*xs, (cx+1)*xs); the remainder pixels on the
// right and at the bottom belong to no cell and are never read.
//
// One work-group of four waves per (cell, frame).  The cell's xs*ys pixels are numbered row by row and dealt to the 256
// threads round robin, so a wave reads 64 consecutive pixels of a cell row (or the end of one row and the start of the
// next): 64 label bytes and 512 B of flow per instruction, four of each in flight per lane.  Labels are read byte by byte
// and flows as 8-byte pairs: a frame of labels starts at any byte address when W*H is odd, and a cell row at any pixel,
// so nothing wider is assumed.  The (row, column) of a thread's next pixel is advanced by 256 = dq*xs + dr with one
// compare, no division in the loop.
//
// A label never indexes anything: every pixel is compared against the KMAX cluster numbers of the instantiation
// (5 / 8 / 16, as the Lloyd kernels) and added, or +0.0 / 0 added, to KMAX register accumulators (a lane-indexed
// accumulator array would live in scratch, see lloyd_tiles.hip's TileCtx).  Labels >= k, 0xFF included, match no j < k.
//
// Deterministic: per-lane accumulators in pixel order, then the 16 lanes of a DPP row folded by rotations (row_sum of
// lloyd_tiles.hip), then the 16 row partials of the work-group added in row order by one thread per output value.  No
// atomics.  A frame's result depends on that frame alone, whatever n_frames is.
//
// k_grid_assign_counts is the same sweep without the label buffer (ofc_grid_assign_counts_dev, and the streaming
// ingest's per-batch pass): it reads only the flow, gives every pixel the label the Lloyd E-step gives it
// (lloyd_device.h's assign_point on (double)u - mean[0], (double)v - mean[1], the centres and |c|^2 of a LloydState),
// and counts it at once: 8 B read and nothing written per pixel, where labelling and then counting moves 10 (18 with
// sums).  Same geometry, same walk, same accumulators and the same reduction, so for equal labels equal bits.
#include "color_common.h"
#include "lloyd_device.h"

namespace ofc {

namespace {

constexpr int GL_THREADS = 256, GL_ROWS = GL_THREADS / 16, GL_UNROLL = 4;

template <int N> __device__ __forceinline__ int gl_ror(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, 0x120 + N, 0xf, 0xf, false);
}
template <int N> __device__ __forceinline__ double gl_ror(double v)
{
    return __hiloint2double(gl_ror<N>(__double2hiint(v)), gl_ror<N>(__double2loint(v)));
}
// sum over the 16 lanes of a DPP row, every lane ends with the same bits (each step combines a pair symmetrically)
template <class T> __device__ __forceinline__ T gl_row_sum(T v)
{
    v += gl_ror<8>(v); v += gl_ror<4>(v); v += gl_ror<2>(v); return v + gl_ror<1>(v);
}

template <int KMAX, bool SUMS> struct GlAcc {
    int n[KMAX];
    double u[SUMS ? KMAX : 1], v[SUMS ? KMAX : 1];

    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < KMAX; j++) {
            n[j] = 0;
            if (SUMS) { u[j] = 0.0; v[j] = 0.0; }
        }
    }
    __device__ __forceinline__ void add(unsigned label, float2 f)
    {
#pragma unroll
        for (int j = 0; j < KMAX; j++) {
            const bool hit = label == (unsigned)j;
            n[j] += hit ? 1 : 0;
            if (SUMS) {
                u[j] += hit ? (double)f.x : 0.0;
                v[j] += hit ? (double)f.y : 0.0;
            }
        }
    }
};

// the cell of this work-group (blockIdx.x) in its frame (blockIdx.y)
struct GlCell {
    int xs, ys, npx;          // npx <= W*H, which the host keeps below 2^31
    size_t origin;            // of the cell's first pixel, in pixels from the start of the buffer
    __device__ __forceinline__ GlCell(int W, int H, int rows, int cols)
    {
        const int cell = blockIdx.x, cy = cell / cols, cx = cell - cy * cols;
        xs = W / cols; ys = H / rows; npx = xs * ys;
        origin = (size_t)blockIdx.y * W * H + (size_t)cy * ys * W + (size_t)cx * xs;
    }
};

// a thread's pixels in order: threadIdx.x, + 256, + 512, ... of the cell's row-by-row numbering
struct GlWalk {
    int W, xs, dq, dr, ly, lx;
    __device__ __forceinline__ GlWalk(const GlCell &g, int W_) : W(W_), xs(g.xs)
    {
        dq = GL_THREADS / xs; dr = GL_THREADS - dq * xs;      // the next pixel of a thread: dq rows, dr columns on
        ly = (int)threadIdx.x / xs; lx = (int)threadIdx.x - ly * xs;
    }
    __device__ __forceinline__ size_t offset_and_step()
    {
        const size_t o = (size_t)ly * W + lx;
        lx += dr; ly += dq;
        if (lx >= xs) { lx -= xs; ly++; }
        return o;
    }
};

// the work-group's accumulators -> counts[frame][cell][k] and sums[frame][cell][k][2]
template <int KMAX, bool SUMS>
__device__ __forceinline__ void gl_reduce_store(const GlAcc<KMAX, SUMS> &acc, int cells, int k, int32_t *__restrict__ counts,
                                                double *__restrict__ sums)
{
    __shared__ int s_n[GL_ROWS][KMAX];
    __shared__ double s_uv[SUMS ? GL_ROWS : 1][2 * KMAX];
    const int row = threadIdx.x >> 4;
#pragma unroll
    for (int j = 0; j < KMAX; j++) {
        const int n = gl_row_sum(acc.n[j]);
        if ((threadIdx.x & 15) == 0) s_n[row][j] = n;
        if (SUMS) {
            const double u = gl_row_sum(acc.u[j]), v = gl_row_sum(acc.v[j]);
            if ((threadIdx.x & 15) == 0) { s_uv[row][2 * j] = u; s_uv[row][2 * j + 1] = v; }
        }
    }
    __syncthreads();
    const size_t out = ((size_t)blockIdx.y * cells + blockIdx.x) * k;
    const int t = threadIdx.x;
    if (t < k) {
        int n = 0;
        for (int r = 0; r < GL_ROWS; r++) n += s_n[r][t];
        counts[out + t] = n;
    }
    if (SUMS && t >= 64 && t < 64 + 2 * k) {          // the second wave: the first one is busy with the counts
        const int c = t - 64;
        double s = 0.0;
        for (int r = 0; r < GL_ROWS; r++) s += s_uv[r][c];
        sums[out * 2 + c] = s;
    }
}

template <int KMAX, bool SUMS>
__global__ __launch_bounds__(GL_THREADS) void k_grid_label_counts(const uint8_t *__restrict__ labels,
                                                                  const float2 *__restrict__ flow, int W, int H, int rows,
                                                                  int cols, int k, int32_t *__restrict__ counts,
                                                                  double *__restrict__ sums)
{
    const GlCell g(W, H, rows, cols);
    const uint8_t *lab = labels + g.origin;
    const float2 *fl = SUMS ? flow + g.origin : nullptr;

    GlAcc<KMAX, SUMS> acc;
    acc.clear();
    GlWalk w(g, W);
    int i = threadIdx.x;
    for (; i + (GL_UNROLL - 1) * GL_THREADS < g.npx; i += GL_UNROLL * GL_THREADS) {
        unsigned l[GL_UNROLL];
        float2 f[GL_UNROLL];
#pragma unroll
        for (int q = 0; q < GL_UNROLL; q++) {
            const size_t o = w.offset_and_step();
            l[q] = lab[o];
            f[q] = SUMS ? fl[o] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < GL_UNROLL; q++) acc.add(l[q], f[q]);
    }
    for (; i < g.npx; i += GL_THREADS) {
        const size_t o = w.offset_and_step();
        acc.add(lab[o], SUMS ? fl[o] : make_float2(0.f, 0.f));
    }
    gl_reduce_store<KMAX, SUMS>(acc, rows * cols, k, counts, sums);
}

// label and count in one sweep.  The model is wave-uniform: the centres, their |c|^2 and the mean are read through
// uniform addresses of the constant LloydState and stay in scalar registers (as vector registers the (16, sums) instance
// would need 96 more than its 80 of accumulators).  Every lane keeps GL_UNROLL loads of the next round in flight while it
// labels the current one; a pixel past the cell's end is not read and carries label KMAX, which no cluster matches.
template <int KMAX, bool SUMS>
__global__ __launch_bounds__(GL_THREADS) void k_grid_assign_counts(const float2 *__restrict__ flow,
                                                                   const LloydState *__restrict__ st, int W, int H, int rows,
                                                                   int cols, int k, int32_t *__restrict__ counts,
                                                                   double *__restrict__ sums)
{
    const GlCell g(W, H, rows, cols);
    const float2 *fl = flow + g.origin;
    double c[2 * KMAX], cn[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; j++) {
        cn[j] = (j < k) ? st->cn[j] : 0.0;
        c[2 * j] = (j < k) ? st->centers[2 * j] : 0.0;
        c[2 * j + 1] = (j < k) ? st->centers[2 * j + 1] : 0.0;
    }
    const double m0 = st->mean[0], m1 = st->mean[1];

    GlAcc<KMAX, SUMS> acc;
    acc.clear();
    GlWalk w(g, W);
    constexpr int ROUND = GL_UNROLL * GL_THREADS;
    float2 next[GL_UNROLL];
    auto request = [&](int left) {                    // the round whose first pixel is `left` pixels before the cell's end
#pragma unroll
        for (int q = 0; q < GL_UNROLL; q++) {
            const size_t o = w.offset_and_step();
            next[q] = q * GL_THREADS < left ? fl[o] : make_float2(0.f, 0.f);
        }
    };
    // counted down, so that nothing is ever added to a pixel number that may be close to 2^31
    int left = g.npx - (int)threadIdx.x;
    request(left);
    while (left > 0) {
        float2 f[GL_UNROLL];
#pragma unroll
        for (int q = 0; q < GL_UNROLL; q++) f[q] = next[q];
        if (left > ROUND) request(left - ROUND);
#pragma unroll
        for (int q = 0; q < GL_UNROLL; q++) {
            const double x[2] = {(double)f[q].x - m0, (double)f[q].y - m1};
            const int l = assign_point<2, KMAX>(x, c, cn, k);
            acc.add(q * GL_THREADS < left ? (unsigned)l : (unsigned)KMAX, f[q]);
        }
        left -= ROUND;
    }
    gl_reduce_store<KMAX, SUMS>(acc, rows * cols, k, counts, sums);
}

template <int KMAX, bool SUMS>
void gl_launch(const uint8_t *labels, const float *flow, int W, int H, int nf, int rows, int cols, int k, int32_t *counts,
               double *sums, hipStream_t s)
{
    hipLaunchKernelGGL((k_grid_label_counts<KMAX, SUMS>), dim3(rows * cols, nf), dim3(GL_THREADS), 0, s, labels,
                       reinterpret_cast<const float2 *>(flow), W, H, rows, cols, k, counts, sums);
}

template <int KMAX, bool SUMS>
void ga_launch(const float *flow, const LloydState *st, int W, int H, int nf, int rows, int cols, int k, int32_t *counts,
               double *sums, hipStream_t s)
{
    hipLaunchKernelGGL((k_grid_assign_counts<KMAX, SUMS>), dim3(rows * cols, nf), dim3(GL_THREADS), 0, s,
                       reinterpret_cast<const float2 *>(flow), st, W, H, rows, cols, k, counts, sums);
}

}  // namespace

// labels [n_frames][H][W] u8, flow [n_frames][H][W][2] f32 or nullptr -> counts [n_frames][rows*cols][k],
// sums [n_frames][rows*cols][k][2] (with flow).  The caller has checked every argument (ofc_grid_label_counts_dev).
int launch_grid_label_counts(const uint8_t *labels, const float *flow, int W, int H, int n_frames, int rows, int cols, int k,
                             int32_t *counts, double *sums, hipStream_t s)
{
    const int kmax = k <= 5 ? 5 : (k <= 8 ? 8 : 16);
    const size_t P = (size_t)W * H, nc = (size_t)rows * cols;
    for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {               // gridDim.y
        const int nf = n_frames - f0 < 65535 ? (int)(n_frames - f0) : 65535;
        const uint8_t *l = labels + f0 * P;
        const float *fl = flow ? flow + f0 * P * 2 : nullptr;
        int32_t *c = counts + f0 * nc * k;
        double *sm = sums ? sums + f0 * nc * k * 2 : nullptr;
#define GL_CASE(KM)                                                                                  \
    if (flow) gl_launch<KM, true>(l, fl, W, H, nf, rows, cols, k, c, sm, s);                           \
    else gl_launch<KM, false>(l, fl, W, H, nf, rows, cols, k, c, sm, s)
        if (kmax == 5) { GL_CASE(5); }
        else if (kmax == 8) { GL_CASE(8); }
        else { GL_CASE(16); }
#undef GL_CASE
        OFC_HIP(hipGetLastError());
    }
    return OFC_OK;
}

// flow [n_frames][H][W][2] f32, st: mean, centred centres and cn set (launch_lloyd_set_centers) -> counts and, with
// sums != nullptr, sums as launch_grid_label_counts writes them for the E-step's labels.  The caller has checked every
// argument (ofc_grid_assign_counts_dev, ofc_stream_set_model).
int launch_grid_assign_counts(const float *flow, const LloydState *st, int W, int H, int n_frames, int rows, int cols, int k,
                              int32_t *counts, double *sums, hipStream_t s)
{
    const int kmax = k <= 5 ? 5 : (k <= 8 ? 8 : 16);
    const size_t P = (size_t)W * H, nc = (size_t)rows * cols;
    for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {               // gridDim.y
        const int nf = n_frames - f0 < 65535 ? (int)(n_frames - f0) : 65535;
        const float *fl = flow + f0 * P * 2;
        int32_t *c = counts + f0 * nc * k;
        double *sm = sums ? sums + f0 * nc * k * 2 : nullptr;
#define GA_CASE(KM)                                                                              \
    if (sums) ga_launch<KM, true>(fl, st, W, H, nf, rows, cols, k, c, sm, s);                      \
    else ga_launch<KM, false>(fl, st, W, H, nf, rows, cols, k, c, sm, s)
        if (kmax == 5) { GA_CASE(5); }
        else if (kmax == 8) { GA_CASE(8); }
        else { GA_CASE(16); }
#undef GA_CASE
        OFC_HIP(hipGetLastError());
    }
    return OFC_OK;
}

}  // namespace ofc
