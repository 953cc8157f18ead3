// flow_solve.hip -- the staged kernels of an iteration: K4 update matrices, K5 box mean + 2x2 solve (windows up to 17, and
// the wide form from 19 on), K6 flow upsample.  The engine runs them where the fused iteration (flow_iter.hip) does not apply.
// Layouts and the contraction policy: flow_device.h.
#include "flow_device.h"
#include "flow_host.h"

namespace ofc {

// (the per-pixel update-matrices arithmetic -- um_load / um_math -- lives in flow_device.h)

__global__ __launch_bounds__(256) void k_update_matrices(const float *__restrict__ R0b,
                                                         const float *__restrict__ R1b,
                                                         size_t pair_stride_R,
                                                         const float *__restrict__ flowb,
                                                         float *__restrict__ Mb, int W, int H)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t plane = (size_t)W * H;
    const float *R0 = R0b + blockIdx.z * pair_stride_R;
    const float *R1 = R1b + blockIdx.z * pair_stride_R;
    const float2 fl = reinterpret_cast<const float2 *>(flowb)[(size_t)blockIdx.z * plane + (size_t)y * W + x];
    float *M = Mb + (size_t)blockIdx.z * 5 * plane;
    float m[5];
    update_matrices_px(R0, R1, plane, W, H, x, y, fl, m);
    const size_t idx = (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 5; c++) M[c * plane + idx] = m[c];
}

int launch_update_matrices(const float *R0, const float *R1, size_t pair_stride_R,
                           const float *flow, float *M, int npair, int W, int H, hipStream_t s)
{
    if ((int64_t)W * H * 5 >= (1ll << 30)) { set_error("frame too large for 32-bit R offsets (%dx%d)", W, H); return OFC_EUNSUPPORTED; }
    dim3 grid(cdiv(W, 256), H, npair);
    hipLaunchKernelGGL(k_update_matrices, grid, dim3(256), 0, s, R0, R1, pair_stride_R, flow, M, W, H);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

// ------------------------------------------------------------------------------------------------
// K5  box mean (winsize x winsize, replicate border) of the 5 M planes + regularised 2x2 solve.
// 28 B/px algorithmic (20 read + 8 written).
//
// "Column march": work-group = 256 threads <-> 256 columns (256 - 2m outputs + halo), marching down a
// strip of rows.  Every thread keeps the vertical (2m+1)-row sums of its column for the 5 channels as
// f64 running sums in registers (+ new row - old row: 2 loads per channel per row, L2-resident), and
// every 4 rows the work-group exchanges them through LDS (41 KB -> 3 work-groups per CU) so
// that wave <-> row, lane <-> 4 consecutive x can form the horizontal sums by sliding (2m+1 + 3*2 adds
// for 4 outputs) from 9 ds_read_b128 per channel, solve, and store 4 float2.  The sums are exact f64
// sums of f32 values (the reference's running sums round the f32 differences: ~1e-7 relative).
// ------------------------------------------------------------------------------------------------

template <int M>
__global__ __launch_bounds__(256) void k_box_solve(const float *__restrict__ Mb,
                                                   float *__restrict__ flowb, int W, int H,
                                                   int rows_per_block)
{
    constexpr int TXO = 256 - 2 * M;          // outputs per work-group row
    constexpr int NV = 2 * M + 4;             // vsum values a lane needs for its 4 outputs
    constexpr int NV2 = (NV + 1) / 2;         // as double2 reads
    constexpr int PITCH = 256 + 2;            // doubles; keeps rows 16-B aligned
    __shared__ __align__(16) double vs[5][BS_ROWS][PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * TXO;
    const int y_begin = blockIdx.y * rows_per_block;
    const int y_end = min(y_begin + rows_per_block, H);
    const size_t plane = (size_t)W * H;
    const float *Mp = Mb + (size_t)blockIdx.z * 5 * plane;
    float2 *flow = reinterpret_cast<float2 *>(flowb) + (size_t)blockIdx.z * plane;
    const int xc = min(max(x0 - M + tid, 0), W - 1);
    const double scale = 1.0 / ((2 * M + 1) * (2 * M + 1));

    // vertical sums of rows [y_begin-M, y_begin+M] (replicate)
    double v[5] = {0, 0, 0, 0, 0};
    for (int j = -M; j <= M; j++) {
        const size_t o = (size_t)min(max(y_begin + j, 0), H - 1) * W + xc;
#pragma unroll
        for (int c = 0; c < 5; c++) v[c] += (double)Mp[c * plane + o];
    }
    for (int yc = y_begin; yc < y_end; yc += BS_ROWS) {
#pragma unroll
        for (int r = 0; r < BS_ROWS; r++) {
#pragma unroll
            for (int c = 0; c < 5; c++) vs[c][r][tid] = v[c];
            // advance to row yc + r + 1
            const int y = yc + r;
            const size_t oa = (size_t)min(y + 1 + M, H - 1) * W + xc;
            const size_t os = (size_t)max(y - M, 0) * W + xc;
#pragma unroll
            for (int c = 0; c < 5; c++)
                v[c] += (double)Mp[c * plane + oa] - (double)Mp[c * plane + os];
        }
        __syncthreads();
        const int y = yc + wave;
        const int xo = x0 + 4 * lane;
        if (y < y_end && 4 * lane < TXO && xo < W) {
            double S[5][4];
#pragma unroll
            for (int c = 0; c < 5; c++) {
                double a[2 * NV2];
#pragma unroll
                for (int q = 0; q < NV2; q++) {
                    double2 d = *reinterpret_cast<const double2 *>(&vs[c][wave][4 * lane + 2 * q]);
                    a[2 * q] = d.x; a[2 * q + 1] = d.y;
                }
                double s = a[0];
#pragma unroll
                for (int q = 1; q <= 2 * M; q++) s += a[q];
                S[c][0] = s;
#pragma unroll
                for (int o = 1; o < 4; o++) {
                    s += a[2 * M + o] - a[o - 1];
                    S[c][o] = s;
                }
            }
#pragma unroll
            for (int o = 0; o < 4; o++) {
                if (4 * lane + o < TXO && xo + o < W) {
                    const double g11 = S[0][o] * scale, g12 = S[1][o] * scale, g22 = S[2][o] * scale,
                                 h1 = S[3][o] * scale, h2 = S[4][o] * scale;
                    const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
                    flow[(size_t)y * W + xo + o] = make_float2((float)((g11 * h2 - g12 * h1) * idet),
                                                               (float)((g22 * h1 - g12 * h2) * idet));
                }
            }
        }
        __syncthreads();   // vs is rewritten by the next step
    }
}

int box_default_rows(int W, int H, int npair)
{
    int tiles_x = cdiv(W, 256 - 14);
    int rows = 128;
    while (rows > 16 && (int64_t)tiles_x * cdiv(H, rows) * npair < 1536) rows >>= 1;
    return rows;
}

// ------------------------------------------------------------------------------------------------
// K5 for wide windows (winsize 19 .. OFC_WINSIZE_MAX): the same box mean + solve with a cost per pixel that does not
// depend on m = winsize / 2.
//
// A work-group owns a SPAN of 1024 columns (4 consecutive per lane) starting m + 1 columns left of its TX = 1024 - 2m - 1
// output columns, and marches down a strip of rows.  Each lane keeps the f64 vertical sums of its 4 columns in registers
// (+ new row - old row, 2 loads per channel per row, as in k_box_solve).  Every row the work-group forms the inclusive
// prefix P of those sums over the span (in-lane serial, wave scan, wave totals through LDS) with columns outside the
// frame counted as 0, so that the in-frame part of the window is S(x) = P(x+m) - P(x-m-1) -- two LDS reads per channel
// whatever m is -- and the replicated border adds (x+m-(W-1))+ * v[W-1] + (m-x)+ * v[0].  Every output that needs such a
// term has that edge column inside its span.  Windows wider than the frame (coarse levels) follow from the same formula.
// f64 throughout; the prefix difference is exact up to ~1e-16 of the row's running total.
// ------------------------------------------------------------------------------------------------
constexpr int BW_SPAN = 1024;      // columns of vertical sums a work-group scans per row (4 per lane)

__global__ __launch_bounds__(256, 3) void k_box_solve_wide(const float *__restrict__ Mb, float *__restrict__ flowb,
                                                        int W, int H, int m, int rows_per_block)
{
    __shared__ __align__(16) double P[5][BW_SPAN];      // 40 KB: this row's prefix over the span
    __shared__ double wtot[5][4];                       // per-wave totals of the scan
    __shared__ double edge[2][5];                       // vertical sums of columns 0 and W-1 (when inside the span)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int TX = BW_SPAN - 2 * m - 1;
    const int x0 = blockIdx.x * TX, a0 = x0 - m - 1;   // first output column, first span column
    const int y_begin = blockIdx.y * rows_per_block;
    const int y_end = min(y_begin + rows_per_block, H);
    const size_t plane = (size_t)W * H;
    const float *Mp = Mb + (size_t)blockIdx.z * 5 * plane;
    float2 *flow = reinterpret_cast<float2 *>(flowb) + (size_t)blockIdx.z * plane;
    const double scale = 1.0 / ((2 * m + 1) * (2 * m + 1));

    // this lane's span columns a0 + 4*tid + i; out-of-frame ones load the clamped column (a valid address) and count 0
    int col[4];
    bool in[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int c = a0 + 4 * tid + i;
        in[i] = c >= 0 && c < W;
        col[i] = min(max(c, 0), W - 1);
    }

    // vertical sums of rows [y_begin-m, y_begin+m] (replicate): the rows inside the frame once each, the repeated edge
    // rows as a multiple -- at most min(2m+1, H) row loads, so a window taller than a coarse level costs no more
    double v[5][4];
#pragma unroll
    for (int c = 0; c < 5; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) v[c][i] = 0;
    const int jlo = max(y_begin - m, 0), jhi = min(y_begin + m, H - 1);
    for (int j = jlo; j <= jhi; j++) {
        const size_t ro = (size_t)j * W;
#pragma unroll
        for (int c = 0; c < 5; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) v[c][i] += (double)Mp[c * plane + ro + col[i]];
    }
    const double ntop = (double)max(m - y_begin, 0), nbot = (double)max(y_begin + m - (H - 1), 0);
    if (ntop > 0 || nbot > 0) {
#pragma unroll
        for (int c = 0; c < 5; c++)
#pragma unroll
            for (int i = 0; i < 4; i++)
                v[c][i] += ntop * (double)Mp[c * plane + col[i]] + nbot * (double)Mp[c * plane + (size_t)(H - 1) * W + col[i]];
    }

    for (int y = y_begin; y < y_end; y++) {
        // the incoming row that advances the sums to y+1, issued before this row's scan (the outgoing one, issued after
        // it, leaves the register budget of 3 waves per SIMD)
        float fa[5][4];
        const size_t oa = (size_t)min(y + 1 + m, H - 1) * W, os = (size_t)max(y - m, 0) * W;
#pragma unroll
        for (int c = 0; c < 5; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) fa[c][i] = Mp[c * plane + oa + col[i]];

        // only the lane's exclusive offset crosses the barrier; its 4 in-lane prefixes are formed again from v after it
        double ex[5];
#pragma unroll
        for (int c = 0; c < 5; c++) {
            double s = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) s += in[i] ? v[c][i] : 0.0;
            double t = s;                               // inclusive wave scan of the lane totals
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const double o = __shfl_up(t, d);
                if (lane >= d) t += o;
            }
            ex[c] = __shfl_up(t, 1);
            if (lane == 0) ex[c] = 0;
            if (lane == 63) wtot[c][wave] = t;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 5; c++) {
            double off = ex[c];
            for (int w = 0; w < wave; w++) off += wtot[c][w];
            double p[4], s = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                s += in[i] ? v[c][i] : 0.0;
                p[i] = s + off;
            }
            *reinterpret_cast<double2 *>(&P[c][4 * tid]) = make_double2(p[0], p[1]);
            *reinterpret_cast<double2 *>(&P[c][4 * tid + 2]) = make_double2(p[2], p[3]);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (in[i] && col[i] == 0)
#pragma unroll
                for (int c = 0; c < 5; c++) edge[0][c] = v[c][i];
            if (in[i] && col[i] == W - 1)
#pragma unroll
                for (int c = 0; c < 5; c++) edge[1][c] = v[c][i];
        }
        __syncthreads();
        for (int j = tid; j < TX; j += 256) {
            const int x = x0 + j;
            if (x >= W) break;
            const double nr = (double)max(x + m - (W - 1), 0), nl = (double)max(m - x, 0);
            double S[5];
#pragma unroll
            for (int c = 0; c < 5; c++) {
                S[c] = P[c][j + 2 * m + 1] - P[c][j];
                if (nr > 0) S[c] += nr * edge[1][c];
                if (nl > 0) S[c] += nl * edge[0][c];
            }
            const double g11 = S[0] * scale, g12 = S[1] * scale, g22 = S[2] * scale, h1 = S[3] * scale,
                         h2 = S[4] * scale;
            const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
            flow[(size_t)y * W + x] = make_float2((float)((g11 * h2 - g12 * h1) * idet),
                                                  (float)((g22 * h1 - g12 * h2) * idet));
        }
        __syncthreads();   // P and edge are rewritten by the next row
#pragma unroll
        for (int c = 0; c < 5; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) v[c][i] += (double)fa[c][i] - (double)Mp[c * plane + os + col[i]];
    }
}

// strips two windows tall (the prologue sums 2m+1 rows per column: <= 1/4 of a strip's loads), at least 64 rows.  A
// function of the window alone, so that a pair's flow does not depend on the batch it was computed in.
int box_wide_rows(int winsize) { return std::max(2 * winsize, 64); }

static int launch_box_solve_wide(const float *M, float *flow, int npair, int W, int H, int winsize,
                                 int rows_per_block, hipStream_t s)
{
    if (!(winsize & 1) || winsize < WINSIZE_WIDE_MIN || winsize > OFC_WINSIZE_MAX) {
        set_error("winsize %d unsupported (odd 5..%d)", winsize, OFC_WINSIZE_MAX);
        return OFC_EUNSUPPORTED;
    }
    if (rows_per_block <= 0) rows_per_block = box_wide_rows(winsize);
    const int m = winsize / 2;
    dim3 grid(cdiv(W, BW_SPAN - 2 * m - 1), cdiv(H, rows_per_block), npair);
    hipLaunchKernelGGL(k_box_solve_wide, grid, dim3(256), 0, s, M, flow, W, H, m, rows_per_block);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_box_solve(const float *M, float *flow, int npair, int W, int H, int winsize,
                     int rows_per_block, hipStream_t s)
{
    if (winsize >= WINSIZE_WIDE_MIN) return launch_box_solve_wide(M, flow, npair, W, H, winsize, rows_per_block, s);
    if (rows_per_block <= 0) rows_per_block = box_default_rows(W, H, npair);
    rows_per_block = cdiv(rows_per_block, BS_ROWS) * BS_ROWS;
    dim3 block(256);
#define OFC_BOX_CASE(MM)                                                                         \
    case 2 * MM + 1: {                                                                           \
        dim3 grid(cdiv(W, 256 - 2 * MM), cdiv(H, rows_per_block), npair);                        \
        hipLaunchKernelGGL(k_box_solve<MM>, grid, block, 0, s, M, flow, W, H, rows_per_block);   \
        break;                                                                                   \
    }
    switch (winsize) {
        OFC_BOX_CASE(2)
        OFC_BOX_CASE(3)
        OFC_BOX_CASE(4)
        OFC_BOX_CASE(5)
        OFC_BOX_CASE(6)
        OFC_BOX_CASE(7)
        OFC_BOX_CASE(8)
    default:
        set_error("winsize %d unsupported (odd 5..%d)", winsize, OFC_WINSIZE_MAX);
        return OFC_EUNSUPPORTED;
    }
#undef OFC_BOX_CASE
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

// ------------------------------------------------------------------------------------------------
// K6  flow upsample: resize(prevFlow, (w,h), INTER_LINEAR) * (1/pyr_scale).  10 B/px.  Bit-exact.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_flow_resize(const float2 *__restrict__ src,
                                                     float2 *__restrict__ dst, int sw, int sh, int dw,
                                                     int dh, double scx, double scy, float mul)
{
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    const float2 *s = src + (size_t)blockIdx.z * sw * sh;
    float2 *d = dst + (size_t)blockIdx.z * dw * dh;
    if (sw == dw && sh == dh) {
        float2 v = s[(size_t)y * sw + x];
        d[(size_t)y * dw + x] = make_float2(v.x * mul, v.y * mul);
        return;
    }
    int sx0, sy0, sy1;
    float a1, b1;
    lin_tap_x(x, scx, sw, sx0, a1);
    lin_tap_y(y, scy, sh, sy0, sy1, b1);
    const float a0 = 1.f - a1, b0 = 1.f - b1;
    const int sx1 = (a1 == 0.f) ? sx0 : sx0 + 1;
    const float2 p00 = s[(size_t)sy0 * sw + sx0], p01 = s[(size_t)sy0 * sw + sx1];
    const float2 p10 = s[(size_t)sy1 * sw + sx0], p11 = s[(size_t)sy1 * sw + sx1];
    float h0x, h0y, h1x, h1y;
    if (a1 == 0.f) {
        h0x = p00.x; h0y = p00.y; h1x = p10.x; h1y = p10.y;
    } else {
        h0x = p00.x * a0 + p01.x * a1; h0y = p00.y * a0 + p01.y * a1;
        h1x = p10.x * a0 + p11.x * a1; h1y = p10.y * a0 + p11.y * a1;
    }
    d[(size_t)y * dw + x] = make_float2((h0x * b0 + h1x * b1) * mul, (h0y * b0 + h1y * b1) * mul);
}

int launch_flow_resize(const float *src, float *dst, int npair, int sw, int sh, int dw, int dh,
                       float mul, hipStream_t s)
{
    dim3 grid(cdiv(dw, 256), dh, npair);
    hipLaunchKernelGGL(k_flow_resize, grid, dim3(256), 0, s, reinterpret_cast<const float2 *>(src),
                       reinterpret_cast<float2 *>(dst), sw, sh, dw, dh, (double)sw / dw,
                       (double)sh / dh, mul);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
