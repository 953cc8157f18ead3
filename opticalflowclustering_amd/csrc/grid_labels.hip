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
#include "color_common.h"

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

template <int KMAX, bool SUMS>
__global__ __launch_bounds__(GL_THREADS) void k_grid_label_counts(const uint8_t *__restrict__ labels,
                                                                  const float2 *__restrict__ flow, int W, int H, int rows,
                                                                  int cols, int k, int32_t *__restrict__ counts,
                                                                  double *__restrict__ sums)
{
    __shared__ int s_n[GL_ROWS][KMAX];
    __shared__ double s_uv[SUMS ? GL_ROWS : 1][2 * KMAX];

    const int cell = blockIdx.x, cy = cell / cols, cx = cell - cy * cols;
    const int xs = W / cols, ys = H / rows, npx = xs * ys;          // npx <= W*H, which the host keeps below 2^31
    const size_t origin = (size_t)blockIdx.y * W * H + (size_t)cy * ys * W + (size_t)cx * xs;
    const uint8_t *lab = labels + origin;
    const float2 *fl = SUMS ? flow + origin : nullptr;
    const int dq = GL_THREADS / xs, dr = GL_THREADS - dq * xs;      // the next pixel of a thread: dq rows, dr columns on

    GlAcc<KMAX, SUMS> acc;
    acc.clear();
    int i = threadIdx.x, ly = i / xs, lx = i - ly * xs;
    auto offset_and_step = [&]() {
        const size_t o = (size_t)ly * W + lx;
        lx += dr; ly += dq;
        if (lx >= xs) { lx -= xs; ly++; }
        return o;
    };
    for (; i + (GL_UNROLL - 1) * GL_THREADS < npx; i += GL_UNROLL * GL_THREADS) {
        unsigned l[GL_UNROLL];
        float2 f[GL_UNROLL];
#pragma unroll
        for (int q = 0; q < GL_UNROLL; q++) {
            const size_t o = offset_and_step();
            l[q] = lab[o];
            f[q] = SUMS ? fl[o] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < GL_UNROLL; q++) acc.add(l[q], f[q]);
    }
    for (; i < npx; i += GL_THREADS) {
        const size_t o = offset_and_step();
        acc.add(lab[o], SUMS ? fl[o] : make_float2(0.f, 0.f));
    }

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
    const size_t out = ((size_t)blockIdx.y * rows * cols + cell) * k;
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
void gl_launch(const uint8_t *labels, const float *flow, int W, int H, int nf, int rows, int cols, int k, int32_t *counts,
               double *sums, hipStream_t s)
{
    hipLaunchKernelGGL((k_grid_label_counts<KMAX, SUMS>), dim3(rows * cols, nf), dim3(GL_THREADS), 0, s, labels,
                       reinterpret_cast<const float2 *>(flow), W, H, rows, cols, k, counts, sums);
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

}  // namespace ofc
