// flow_pyramid.hip -- K2, the level images of the Farneback pyramid: u8 frames -> f32 level images, one level per launch
// (k_level_image and its exact-decimation fast paths) or the coarse levels of a batch from one march (k_pyramid_dec).
// Layouts and the contraction policy: flow_device.h.
#include "flow_device.h"
#include "flow_host.h"

namespace ofc {

// ------------------------------------------------------------------------------------------------
// K2  blur + decimate:  u8 full-res frame -> f32 level image.
// The separable Gaussian (REFLECT_101) is evaluated ONLY at the <=2x2 full-res positions each output
// pixel's bilinear taps touch: 1/4 .. 1/16 of the work of blurring the whole frame per level.
// LDS: u8 input tile (+halo) and the row-filtered samples.  HBM-bound on the u8 read (1 B/px of the
// full-res frame per level) -- SURVEY.md 8d.
// ------------------------------------------------------------------------------------------------
struct LevelArgs {
    int W0, H0, w, h;
    int r;
    int txo, tyo;
    int in_w, in_h;      // LDS tile extents (upper bounds)
    int in_pitch;        // u8 pitch, multiple of 4
    double sx, sy;
    float kern[32];
};

__global__ __launch_bounds__(256) void k_level_image(const uint8_t *__restrict__ src,
                                                     float *__restrict__ dst, LevelArgs p)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * p.txo, oy0 = blockIdx.y * p.tyo;
    const int nox = min(p.txo, p.w - ox0), noy = min(p.tyo, p.h - oy0);
    const uint8_t *img = src + (size_t)blockIdx.z * p.W0 * p.H0;
    float *out = dst + (size_t)blockIdx.z * p.w * p.h;

    // LDS carve-up
    int *xs0 = reinterpret_cast<int *>(smem);                   // [txo]
    float *xa = reinterpret_cast<float *>(xs0 + p.txo);         // [txo]
    int *ys0 = reinterpret_cast<int *>(xa + p.txo);             // [tyo]
    int *ys1 = ys0 + p.tyo;                                     // [tyo]
    float *yb = reinterpret_cast<float *>(ys1 + p.tyo);         // [tyo]
    float *h1 = yb + p.tyo;                                     // [in_h][2*txo]
    unsigned char *tile = reinterpret_cast<unsigned char *>(h1 + (size_t)p.in_h * 2 * p.txo);

    if (tid < nox) {
        int s0; float a;
        lin_tap_x(ox0 + tid, p.sx, p.W0, s0, a);
        xs0[tid] = s0; xa[tid] = a;
    }
    if (tid >= 64 && tid - 64 < noy) {
        int s0, s1; float b;
        lin_tap_y(oy0 + tid - 64, p.sy, p.H0, s0, s1, b);
        ys0[tid - 64] = s0; ys1[tid - 64] = s1; yb[tid - 64] = b;
    }
    __syncthreads();
    const int x_first = xs0[0], x_last = min(xs0[nox - 1] + 1, p.W0 - 1);
    const int y_first = ys0[0], y_last = ys1[noy - 1];
    const int ix0 = x_first - p.r, iy0 = y_first - p.r;
    const int tw = x_last - x_first + 1 + 2 * p.r, th = y_last - y_first + 1 + 2 * p.r;

    for (int i = tid; i < tw * th; i += 256) {
        int ly = i / tw, lx = i - ly * tw;
        int gx = reflect101(ix0 + lx, p.W0), gy = reflect101(iy0 + ly, p.H0);
        tile[ly * p.in_pitch + lx] = img[(size_t)gy * p.W0 + gx];
    }
    __syncthreads();

    // row pass (taps summed left to right) at the two x positions of every output column
    const int ks = 2 * p.r + 1;
    for (int i = tid; i < th * nox * 2; i += 256) {
        int ly = i / (nox * 2), rem = i - ly * nox * 2;
        int j = rem >> 1, t = rem & 1;
        int x = min(xs0[j] + t, p.W0 - 1);
        const unsigned char *row = tile + ly * p.in_pitch + (x - x_first);
        float acc = p.kern[0] * (float)row[0];
        for (int q = 1; q < ks; q++) acc += p.kern[q] * (float)row[q];
        h1[(ly * p.txo + j) * 2 + t] = acc;
    }
    __syncthreads();

    // column pass (centre, then symmetric pairs) at the two y positions, then the bilinear mix
    for (int i = tid; i < noy * nox; i += 256) {
        int oy = i / nox, ox = i - oy * nox;
        float a1 = xa[ox], a0 = 1.f - a1, b1 = yb[oy], b0 = 1.f - b1;
        float hrow[2];
#pragma unroll
        for (int yt = 0; yt < 2; yt++) {
            int c = (yt ? ys1[oy] : ys0[oy]) - iy0;
            float v[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                if (t == 1 && a1 == 0.f) { v[1] = 0.f; continue; }
                const float *col = h1 + (c * p.txo + ox) * 2 + t;
                float acc = p.kern[p.r] * col[0];
                for (int m = 1; m <= p.r; m++)
                    acc += p.kern[p.r + m] * (col[-m * p.txo * 2] + col[m * p.txo * 2]);
                v[t] = acc;
            }
            hrow[yt] = (a1 == 0.f) ? v[0] : v[0] * a0 + v[1] * a1;
        }
        out[(size_t)(oy0 + oy) * p.w + ox0 + ox] = hrow[0] * b0 + hrow[1] * b1;
    }
}

// ------------------------------------------------------------------------------------------------
// K2 fast paths for the pyramid the reference actually uses (pyr_scale 0.5: exact 1, 2, 4, 8x decimation).
// Same arithmetic, same order as k_level_image (bit-exact, contraction off); only the data movement differs:
// window bytes come from aligned dword loads and are unpacked with compile-time shifts (v_cvt_f32_ubyteN),
// nothing is staged through LDS as bytes.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ubyte_of(uint32_t w, int n) { return (float)((w >> (8 * n)) & 255u); }

// level 0: 3x3 blur, no decimation.  Thread = 4 px x 8 rows; block tile 256 x 32.
__global__ __launch_bounds__(256) void k_level0(const uint8_t *__restrict__ src, float *__restrict__ dst,
                                                int W, int H, float k0, float k1, float k2)
{
#pragma clang fp contract(off)
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 256 + 4 * tx, y0 = blockIdx.y * 32 + 8 * ty;
    if (x0 >= W || y0 >= H) return;
    const uint8_t *img = src + (size_t)blockIdx.z * W * H;
    float *out = dst + (size_t)blockIdx.z * W * H;
    const bool fast = x0 >= 4 && x0 + 8 <= W;         // W % 4 == 0 is guaranteed by the launcher
    float h[10][4];
#pragma unroll
    for (int j = 0; j < 10; j++) {
        const uint8_t *row = img + (size_t)reflect101(y0 - 1 + j, H) * W;
        float b[6];
        if (fast) {
            const uint32_t *rw = reinterpret_cast<const uint32_t *>(row + x0);
            const uint32_t wa = rw[-1], wb = rw[0], wc = rw[1];
            b[0] = ubyte_of(wa, 3);
            b[1] = ubyte_of(wb, 0); b[2] = ubyte_of(wb, 1); b[3] = ubyte_of(wb, 2); b[4] = ubyte_of(wb, 3);
            b[5] = ubyte_of(wc, 0);
        } else {
#pragma unroll
            for (int q = 0; q < 6; q++) b[q] = (float)row[reflect101(x0 - 1 + q, W)];
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float acc = k0 * b[c];
            acc += k1 * b[c + 1];
            acc += k2 * b[c + 2];
            h[j][c] = acc;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (y0 + i < H) {
            float o[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                float d = k1 * h[i + 1][c];
                d += k2 * (h[i][c] + h[i + 2][c]);
                o[c] = d;
            }
            *reinterpret_cast<float4 *>(out + (size_t)(y0 + i) * W + x0) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// exact S-fold decimation with a (2R+1)-tap Gaussian.  Row pass: one item = (input row, output column):
// both bilinear x taps (xa, xa+1) from ONE 2R+2 byte window held in registers.  Column pass: both y taps from one
// 2R+2 row window of the row-filtered samples in LDS.
template <int S, int R, int TXO, int TYO>
__global__ __launch_bounds__(256) void k_level_dec(const uint8_t *__restrict__ src, float *__restrict__ dst,
                                                   int W0, int H0, int w, int h, LevelArgs p)
{
#pragma clang fp contract(off)
    constexpr int ROWS = S * TYO + 2 * R;                 // input rows feeding the tile
    constexpr int NB = 2 * R + 2;                         // bytes per window
    constexpr int XOFF = (S / 2 - 1 - R);                 // window start relative to S*ox
    constexpr int AL = ((XOFF % 4) + 4) % 4;              // its offset inside the first aligned dword
    constexpr int NW = (AL + NB + 3) / 4;                 // aligned dwords covering the window
    __shared__ float hrow[ROWS][TXO][2];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * TXO, oy0 = blockIdx.y * TYO;
    const uint8_t *img = src + (size_t)blockIdx.z * W0 * H0;
    float *out = dst + (size_t)blockIdx.z * w * h;
    const int yfirst = S * oy0 + S / 2 - 1 - R;           // global row of tile row 0 (before reflection)

    // thread <-> (output column j, row group rg): the thread's RPG input rows are requested back to back before any of
    // them is used (the first version walked "items" one after the other: five dependent memory round trips per work-group
    // on the 1/4 level, which made this trivial kernel 8 % of the flow time)
    constexpr int NG = 256 / TXO, RPG = (ROWS + NG - 1) / NG;
    const int j = tid % TXO, rg = tid / TXO;
    const int ox = ox0 + j;
    if (ox < w) {
        const int xs = S * ox + XOFF;                     // first byte of the window
        const bool fast = xs - AL >= 0 && xs - AL + 4 * NW <= W0;
        auto refl = [](int p, int len) { return p < 0 ? -p : (p >= len ? 2 * (len - 1) - p : p); };   // |overshoot| < len (launcher)
        auto rowpass = [&](int i, const float (&b)[NB]) {
            const int ly = rg + NG * i;
            float a0 = p.kern[0] * b[0], a1 = p.kern[0] * b[1];
#pragma unroll
            for (int q = 1; q <= 2 * R; q++) {
                a0 += p.kern[q] * b[q];
                a1 += p.kern[q] * b[q + 1];
            }
            if (ly < ROWS) *reinterpret_cast<float2 *>(&hrow[ly][j][0]) = make_float2(a0, a1);
        };
        if (fast) {
            uint32_t wd[RPG][NW];
#pragma unroll
            for (int i = 0; i < RPG; i++) {
                const int ly = min(rg + NG * i, ROWS - 1);
                const uint32_t *rw = reinterpret_cast<const uint32_t *>(img + (size_t)refl(yfirst + ly, H0) * W0 + (xs - AL));
#pragma unroll
                for (int q = 0; q < NW; q++) wd[i][q] = rw[q];
            }
#pragma unroll
            for (int i = 0; i < RPG; i++) {
                float b[NB];
#pragma unroll
                for (int q = 0; q < NB; q++) b[q] = ubyte_of(wd[i][(AL + q) >> 2], (AL + q) & 3);
                rowpass(i, b);
            }
        } else {
#pragma unroll
            for (int i = 0; i < RPG; i++) {
                const int ly = min(rg + NG * i, ROWS - 1);
                const uint8_t *row = img + (size_t)refl(yfirst + ly, H0) * W0;
                float b[NB];
#pragma unroll
                for (int q = 0; q < NB; q++) b[q] = (float)row[reflect101(xs + q, W0)];
                rowpass(i, b);
            }
        }
    }
    __syncthreads();
    for (int it = tid; it < TYO * TXO; it += 256) {
        const int oy = it / TXO, j = it - oy * TXO;
        if (ox0 + j >= w || oy0 + oy >= h) continue;
        const int c0 = S * oy + R;                        // tile row of the first y tap's centre
        float2 win[2 * R + 2];
#pragma unroll
        for (int q = 0; q < 2 * R + 2; q++) win[q] = *reinterpret_cast<const float2 *>(&hrow[c0 - R + q][j][0]);
        float hy[2];
#pragma unroll
        for (int yt = 0; yt < 2; yt++) {
            float v0 = p.kern[R] * win[R + yt].x, v1 = p.kern[R] * win[R + yt].y;
#pragma unroll
            for (int m = 1; m <= R; m++) {
                v0 += p.kern[R + m] * (win[R + yt - m].x + win[R + yt + m].x);
                v1 += p.kern[R + m] * (win[R + yt - m].y + win[R + yt + m].y);
            }
            hy[yt] = v0 * 0.5f + v1 * 0.5f;
        }
        out[(size_t)(oy0 + oy) * w + ox0 + j] = hy[0] * 0.5f + hy[1] * 0.5f;
    }
}

// the exact-decimation fast paths: S-fold decimation under 2R+1 taps, in k_level_dec's TXO x TYO output tiles
struct DecPath {
    int S, R, TXO, TYO;
};
constexpr DecPath DEC_PATHS[3] = {{2, 1, 64, 16}, {4, 4, 32, 8}, {8, 9, 32, 8}};

// What launch_level_image will do with a level, decided on the host with no launch: which of its four paths the level
// takes (0: the 3x3 level-0 kernel, 2 / 4 / 8: exact decimation, 1: the general LDS-staged tile) and, for the general
// path, the tile and its LDS size -- or the refusal.  launch_level_image launches exactly what this returns and
// flow_levels_check (the walk ofc_flow_create runs before it allocates) asks it about every level through
// level_image_check, so the limits of the launch and of the walk are one piece of code.
static int level_image_plan(int W0, int H0, const LevelGeom &g, bool src_aligned, LevelArgs &a, int &path, size_t &lds)
{
    memset(&a, 0, sizeof(a));
    a.W0 = W0; a.H0 = H0; a.w = g.w; a.h = g.h;
    a.r = g.ksize / 2;
    lds = 0;
    if (g.ksize > 31) { set_error("blur kernel size %d > 31 unsupported", g.ksize); return OFC_EUNSUPPORTED; }
    gaussian_kernel(g.ksize, g.sigma, a.kern);
    a.sx = (double)W0 / g.w; a.sy = (double)H0 / g.h;
    // fast paths: exact decimation by 1 / 2 / 4 / 8 with the reference's tap counts, rows dword-addressable
    const bool aligned = (W0 % 4) == 0 && src_aligned && (((size_t)W0 * H0) % 4) == 0;
    if (aligned && g.w == W0 && g.h == H0 && a.r == 1) { path = 0; return OFC_OK; }
    for (const DecPath &d : DEC_PATHS)
        if (aligned && g.w * d.S == W0 && g.h * d.S == H0 && a.r == d.R && H0 > 2 * d.R + d.S && W0 > 2 * d.R + 8) {
            path = d.S;
            return OFC_OK;
        }
    // general path (any scale / tap count): LDS-staged tile
    path = 1;
    if (a.sx <= 2.5) { a.txo = 64; a.tyo = 16; } else { a.txo = 32; a.tyo = 8; }
    a.in_w = (int)(a.txo * a.sx) + 2 * a.r + 4;
    a.in_h = (int)(a.tyo * a.sy) + 2 * a.r + 4;
    a.in_pitch = (a.in_w + 3) & ~3;
    lds = (size_t)(2 * a.txo + 3 * a.tyo) * 4 + (size_t)a.in_h * 2 * a.txo * 4 + (size_t)a.in_h * a.in_pitch;
    if (lds > 160 * 1024) { set_error("level_image tile needs %zu B LDS", lds); return OFC_EUNSUPPORTED; }
    return OFC_OK;
}

int level_image_check(int W0, int H0, const LevelGeom &g, bool src_aligned)
{
    LevelArgs a;
    int path;
    size_t lds;
    return level_image_plan(W0, H0, g, src_aligned, a, path, lds);
}

template <int I>
static void launch_level_dec(const uint8_t *src, float *dst, int nimg, int W0, int H0, const LevelGeom &g, const LevelArgs &a,
                             hipStream_t s)
{
    constexpr DecPath d = DEC_PATHS[I];
    hipLaunchKernelGGL((k_level_dec<d.S, d.R, d.TXO, d.TYO>), dim3(cdiv(g.w, d.TXO), cdiv(g.h, d.TYO), nimg), dim3(256), 0, s,
                       src, dst, W0, H0, g.w, g.h, a);
}

int launch_level_image(const uint8_t *src, float *dst, int nimg, int W0, int H0,
                       const LevelGeom &g, hipStream_t s)
{
    LevelArgs a;
    int path = 1;
    size_t lds = 0;
    OFC_TRY(level_image_plan(W0, H0, g, ((uintptr_t)src % 4) == 0, a, path, lds));
    switch (path) {
    case 0:
        hipLaunchKernelGGL(k_level0, dim3(cdiv(W0, 256), cdiv(H0, 32), nimg), dim3(256), 0, s, src, dst, W0, H0,
                           a.kern[0], a.kern[1], a.kern[2]);
        break;
    case DEC_PATHS[0].S: launch_level_dec<0>(src, dst, nimg, W0, H0, g, a, s); break;
    case DEC_PATHS[1].S: launch_level_dec<1>(src, dst, nimg, W0, H0, g, a, s); break;
    case DEC_PATHS[2].S: launch_level_dec<2>(src, dst, nimg, W0, H0, g, a, s); break;
    default:
        hipLaunchKernelGGL(k_level_image, dim3(cdiv(g.w, a.txo), cdiv(g.h, a.tyo), nimg), dim3(256), lds, s, src, dst, a);
    }
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

// ------------------------------------------------------------------------------------------------
// K2 fused: the exact-decimation levels 1..L (L <= 3: 2x / 3 taps, 4x / 9 taps, 8x / 19 taps) of a batch from ONE march
// over the u8 frames.  Every value is computed by k_level_dec's statements in k_level_dec's order, contraction off, so the
// images are the same bits; only the data movement and which values share a packed instruction differ.
//
// Work-group = 256 threads, one band of 256 input columns (128 + 64 + 32 output columns) of one strip of one frame,
// marched in steps of 8 input rows.  Step t:
//   stage     the bytes of rows 8t+7 .. 8t+14 (REFLECT_101 in y and, at the frame's sides, in x), columns x0-8 .. x0+263,
//             were requested one step ahead as 544 coalesced dwords and go to LDS: 2 176 B
//   barrier
//   request   the next step's rows
//   row pass  of the 8 new rows at all levels -> one LDS ring per level, float2 = the two x positions of an output column.
//             An item is one window in TWO rows, four apart (packed f32, one lane per row): level 3, 32 columns x 4 row
//             pairs, on waves 0-1; level 2, 64 x 4, two items a thread on waves 2-3 (as many instructions as a level 3 item);
//             then level 1, two adjacent columns x 4 row pairs, an item for every thread
//   barrier
//   column pass of the output rows whose windows end in row 8t+14: level 1 rows 4t+3 .. 4t+6 (waves 0-1, a thread owns a
//             column and reads its ten ring rows once), level 2 rows 2t+1, 2t+2 (wave 2), level 3 row t (half of wave 3)
// A ring holds whole steps: 16 rows at levels 1 and 2 (windows of 10 and 14 rows behind row 8t+14), 24 at level 3 (20 rows):
// 16 + 8 + 6 KB.  The slot of every ring access is a compile-time constant: the step body is instantiated for the six
// values of t mod 6.  No input row is row-filtered twice inside a strip; a strip warms up with the row passes of two
// steps (level 3) / one step (levels 1, 2).  Rows above the frame are the steps -2 and -1 of the first strip, which row-filters
// both at all levels and writes level 1 rows 0 .. 2 and level 2 row 0 in step -1.
// ------------------------------------------------------------------------------------------------
struct PyrDecArgs {
    int W0, H0;
    int steps, sps;              // 8-row steps per frame; steps per strip
    int w[3], h[3];
    float k1[2], k2[5], k3[10];  // taps 0..R of each level's kernel; tap q > R is tap 2R-q (gaussian_kernel computes both from the
                                 // same x*x: the same float), which halves the scalar registers the taps hold
};

constexpr int PD_BAND = 256;     // input columns per work-group
constexpr int PD_SW = 68;        // staged dwords per row: bytes x0-8 .. x0+263

typedef float pd_v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pd_v2f pd_ld2(const float2 *p) { const float2 v = *p; return pd_v2f{v.x, v.y}; }

// the two row sums of k_level_dec, a0 = sum k[q] b[q] and a1 = sum k[q] b[q+1], each left to right, for TWO input rows at once:
// b[q] = (byte q of the window in the first row, the same in the second), so that one packed operation serves both rows,
// the tap is one scalar register and no operand has to be moved into place
template <int R>
__device__ __forceinline__ void pd_row_sums(const pd_v2f *b, const float *kh, pd_v2f &a0, pd_v2f &a1)
{
#pragma clang fp contract(off)
    a0 = kh[0] * b[0];
    a1 = kh[0] * b[1];
#pragma unroll
    for (int q = 1; q <= 2 * R; q++) {
        const float k = kh[q <= R ? q : 2 * R - q];
        a0 += k * b[q];
        a1 += k * b[q + 1];
    }
}

// k_level_dec's column pass on a window of 2R+2 ring rows (centre first, then the symmetric pairs; the two mixes); the two
// x positions of a ring entry are the two lanes of the packed operations
template <int R>
__device__ __forceinline__ float pd_col(const pd_v2f *win, const float *kh)
{
#pragma clang fp contract(off)
    float hy[2];
#pragma unroll
    for (int yt = 0; yt < 2; yt++) {
        pd_v2f v = kh[R] * win[R + yt];
#pragma unroll
        for (int m = 1; m <= R; m++) v += kh[R - m] * (win[R + yt - m] + win[R + yt + m]);
        hy[yt] = v.x * 0.5f + v.y * 0.5f;
    }
    return hy[0] * 0.5f + hy[1] * 0.5f;
}

template <int L>
__global__ __launch_bounds__(256, 4) void k_pyramid_dec(const uint8_t *__restrict__ src, float *__restrict__ dst1,
                                                     float *__restrict__ dst2, float *__restrict__ dst3, PyrDecArgs p)
{
#pragma clang fp contract(off)
    __shared__ __align__(16) uint32_t stg[8][PD_SW];
    __shared__ __align__(16) float2 ring1[16][128];
    __shared__ float2 ring2[L >= 2 ? 16 : 1][64];
    __shared__ float2 ring3[L >= 3 ? 24 : 1][32];
    const int tid = threadIdx.x, W0 = p.W0, H0 = p.H0;
    const int band = blockIdx.x, x0 = band * PD_BAND;
    const int t0 = blockIdx.y * p.sps, t1 = min(p.steps, t0 + p.sps);
    const bool first = t0 == 0, last = t1 == p.steps;
    const uint8_t *img = src + (size_t)blockIdx.z * W0 * H0;
    // output rows of this strip: step t writes level 1 rows 4t+3 .. 4t+6, level 2 rows 2t+1, 2t+2, level 3 row t, and the
    // first strip also what step -1 writes
    const int lo1 = first ? 0 : 4 * t0 + 3, hi1 = last ? p.h[0] : min(p.h[0], 4 * t1 + 3);
    const int lo2 = first ? 0 : 2 * t0 + 1, hi2 = last ? p.h[1] : min(p.h[1], 2 * t1 + 1);
    const int hi3 = min(p.h[2], t1);
    float *out1 = dst1 + (size_t)blockIdx.z * p.w[0] * p.h[0];
    float *out2 = L >= 2 ? dst2 + (size_t)blockIdx.z * p.w[1] * p.h[1] : nullptr;
    float *out3 = L >= 3 ? dst3 + (size_t)blockIdx.z * p.w[2] * p.h[2] : nullptr;

    // staging: slot = tid + 256 n of the 8 x 68 dwords; its row and column stay, the frame row moves with the step
    int srow[3], scol[3], smode[3];           // mode 0: one aligned dword; 1: four reflected bytes; 2: beyond what any window reads
#pragma unroll
    for (int n = 0; n < 3; n++) {
        const int s = min(tid + 256 * n, 8 * PD_SW - 1);
        srow[n] = s / PD_SW;
        const int c = s - srow[n] * PD_SW;
        scol[n] = x0 - 8 + 4 * c;
        smode[n] = (scol[n] >= 0 && scol[n] + 4 <= W0) ? 0 : (scol[n] < W0 + 8 ? 1 : 2);
    }
    const bool third = tid < 8 * PD_SW - 512;
    uint32_t d[3];
    auto fetch = [&](int t) {
#pragma unroll
        for (int n = 0; n < 3; n++) {
            if (n == 2 && !third) break;
            const int v = 8 * t + 7 + srow[n];
            int y = v < 0 ? -v : (v >= H0 ? 2 * (H0 - 1) - v : v);
            y = min(max(y, 0), H0 - 1);       // (rows no window of this frame reads may lie further out than one reflection)
            const uint8_t *row = img + (size_t)y * W0;
            if (smode[n] == 0) {
                d[n] = *reinterpret_cast<const uint32_t *>(row + scol[n]);
            } else if (smode[n] == 1) {
                uint32_t w = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {     // |overshoot| <= 8 < W0 (level_image_plan)
                    const int x = scol[n] + e, xr = x < 0 ? -x : (x >= W0 ? 2 * (W0 - 1) - x : x);
                    w |= (uint32_t)row[min(max(xr, 0), W0 - 1)] << (8 * e);
                }
                d[n] = w;
            } else {
                d[n] = 0;
            }
        }
    };

    // row-pass items: a thread takes the same window in two of the step's rows, r and r + 4 (r + 2 and r + 6)
    auto step = [&](auto phc, int t, bool rows12, bool col12, bool col3) {
        constexpr int PH = decltype(phc)::value, P2 = PH % 2, P3 = PH % 3;
        if (tid < 128) {
            if constexpr (L >= 3) {       // level 3: 32 columns x 4 row pairs
                const int j = tid & 31, r = tid >> 5;
                uint32_t wd[2][6];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const uint2 *w2 = reinterpret_cast<const uint2 *>(&stg[r + 4 * i][2 * j]);
                    const uint2 wa = w2[0], wb = w2[1], wc = w2[2];
                    wd[i][0] = wa.x; wd[i][1] = wa.y; wd[i][2] = wb.x; wd[i][3] = wb.y; wd[i][4] = wc.x; wd[i][5] = wc.y;
                }
                pd_v2f b[20], a0, a1;
#pragma unroll
                for (int q = 0; q < 20; q++)
                    b[q] = pd_v2f{ubyte_of(wd[0][(2 + q) >> 2], (2 + q) & 3), ubyte_of(wd[1][(2 + q) >> 2], (2 + q) & 3)};
                pd_row_sums<9>(b, p.k3, a0, a1);
                ring3[P3 * 8 + r][j] = make_float2(a0.x, a1.x);
                ring3[P3 * 8 + r + 4][j] = make_float2(a0.y, a1.y);
            }
        } else if (rows12) {
            if constexpr (L >= 2) {       // level 2: 64 columns x 2 x 2 row pairs
                const int j = tid & 63, r = (tid >> 6) & 1;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    uint32_t wd[2][3];
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const uint32_t *w1 = &stg[r + 2 * h + 4 * i][j + 1];
                        wd[i][0] = w1[0]; wd[i][1] = w1[1]; wd[i][2] = w1[2];
                    }
                    pd_v2f b[10], a0, a1;
#pragma unroll
                    for (int q = 0; q < 10; q++)
                        b[q] = pd_v2f{ubyte_of(wd[0][(1 + q) >> 2], (1 + q) & 3), ubyte_of(wd[1][(1 + q) >> 2], (1 + q) & 3)};
                    pd_row_sums<4>(b, p.k2, a0, a1);
                    ring2[P2 * 8 + r + 2 * h][j] = make_float2(a0.x, a1.x);
                    ring2[P2 * 8 + r + 2 * h + 4][j] = make_float2(a0.y, a1.y);
                }
            }
        }
        if (rows12) {                     // level 1: 64 pairs of columns x 4 row pairs
            const int c = tid & 63, r = tid >> 6;
            uint32_t wd[2][3];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const uint32_t *w1 = &stg[r + 4 * i][c + 1];
                wd[i][0] = w1[0]; wd[i][1] = w1[1]; wd[i][2] = w1[2];
            }
            pd_v2f b[6], a0[2], a1[2];
#pragma unroll
            for (int q = 0; q < 6; q++)
                b[q] = pd_v2f{ubyte_of(wd[0][(3 + q) >> 2], (3 + q) & 3), ubyte_of(wd[1][(3 + q) >> 2], (3 + q) & 3)};
#pragma unroll
            for (int e = 0; e < 2; e++) pd_row_sums<1>(b + 2 * e, p.k1, a0[e], a1[e]);
            *reinterpret_cast<float4 *>(&ring1[P2 * 8 + r][2 * c]) = make_float4(a0[0].x, a1[0].x, a0[1].x, a1[1].x);
            *reinterpret_cast<float4 *>(&ring1[P2 * 8 + r + 4][2 * c]) = make_float4(a0[0].y, a1[0].y, a0[1].y, a1[1].y);
        }
        __syncthreads();
        if (tid < 128) {
            const int ox = 128 * band + tid;
            if (col12 && ox < p.w[0]) {
                pd_v2f win[10];               // rows 8t+5 .. 8t+14
#pragma unroll
                for (int q = 0; q < 10; q++) win[q] = pd_ld2(&ring1[(P2 * 8 + q - 2 + 16) % 16][tid]);
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    const int oy = 4 * t + 3 + a;
                    const float v = pd_col<1>(win + 2 * a, p.k1);
                    if (oy >= lo1 && oy < hi1) out1[(size_t)oy * p.w[0] + ox] = v;
                }
            }
        } else if (tid < 192) {
            if constexpr (L >= 2) {
                const int j = tid - 128, ox = 64 * band + j;
                if (col12 && ox < p.w[1]) {
                    pd_v2f win[14];           // rows 8t+1 .. 8t+14
#pragma unroll
                    for (int q = 0; q < 14; q++) win[q] = pd_ld2(&ring2[(P2 * 8 + q - 6 + 16) % 16][j]);
#pragma unroll
                    for (int a = 0; a < 2; a++) {
                        const int oy = 2 * t + 1 + a;
                        const float v = pd_col<4>(win + 4 * a, p.k2);
                        if (oy >= lo2 && oy < hi2) out2[(size_t)oy * p.w[1] + ox] = v;
                    }
                }
            }
        } else if (tid < 224) {
            if constexpr (L >= 3) {
                const int j = tid - 192, ox = 32 * band + j;
                if (col3 && t < hi3 && ox < p.w[2]) {
                    pd_v2f win[20];           // rows 8t-6 .. 8t+13
#pragma unroll
                    for (int q = 0; q < 20; q++) win[q] = pd_ld2(&ring3[(P3 * 8 + q - 13 + 24) % 24][j]);
                    out3[(size_t)t * p.w[2] + ox] = pd_col<9>(win, p.k3);
                }
            }
        }
    };

    // the first warm-up step: two ahead at level 3, one at levels 1 and 2; level 2's row 0 (written by step -1) reads rows
    // -3 and -2 of step -2
    const int tb = (L >= 3 || (L >= 2 && first)) ? t0 - 2 : t0 - 1;
    int ph = (tb + 6) % 6;
    fetch(tb);
    for (int t = tb; t < t1; t++) {
#pragma unroll
        for (int n = 0; n < 3; n++)
            if (n < 2 || third) stg[srow[n]][(scol[n] - x0 + 8) >> 2] = d[n];
        __syncthreads();
        if (t + 1 < t1) fetch(t + 1);
        const bool rows12 = t >= t0 - 1 || t < 0, col12 = t >= t0 || t == -1, col3 = t >= t0;
        switch (ph) {
        case 0: step(std::integral_constant<int, 0>{}, t, rows12, col12, col3); break;
        case 1: step(std::integral_constant<int, 1>{}, t, rows12, col12, col3); break;
        case 2: step(std::integral_constant<int, 2>{}, t, rows12, col12, col3); break;
        case 3: step(std::integral_constant<int, 3>{}, t, rows12, col12, col3); break;
        case 4: step(std::integral_constant<int, 4>{}, t, rows12, col12, col3); break;
        default: step(std::integral_constant<int, 5>{}, t, rows12, col12, col3); break;
        }
        ph = ph == 5 ? 0 : ph + 1;
    }
}

// The launch geometry of k_pyramid_dec: bands of 256 input columns, 8-row steps, and strips of whole steps so that a batch
// gives about four work-groups to each of the 256 CUs (61 frames of 1080p: 8 bands x 2 strips = 976); a strip is at least
// four steps, its warm-up being two.
void pyramid_dec_plan(int W0, int H0, int nimg, int &bands, int &steps, int &sps, int &strips)
{
    bands = cdiv(W0, PD_BAND);
    steps = cdiv(H0, 8);
    const int64_t nb = std::max<int64_t>(1, (int64_t)nimg * bands);
    const int want = (int)std::max<int64_t>(1, (1024 + nb / 2) / nb);
    sps = std::max(4, cdiv(steps, want));
    strips = cdiv(steps, sps);
}

// how many of the coarse levels 1..levels (geom[1..]) one k_pyramid_dec launch writes: the leading ones, three at the
// most, that take k_level_dec's paths 2, 4, 8 in that order
int pyramid_dec_levels(int W0, int H0, const LevelGeom *geom, int levels, bool src_aligned)
{
    int n = 0;
    for (int k = 1; k <= std::min(levels, 3); k++) {
        LevelArgs a;
        int path = 1;
        size_t lds = 0;
        if (level_image_plan(W0, H0, geom[k], src_aligned, a, path, lds) != OFC_OK || path != DEC_PATHS[k - 1].S) break;
        n = k;
    }
    return n;
}

// levels 1..L (L = pyramid_dec_levels(...) >= 1, the caller's check) of nimg frames into dst[0..L-1]
int launch_pyramid_dec(const uint8_t *src, float *const *dst, int nimg, int W0, int H0, const LevelGeom *geom, int L,
                       hipStream_t s)
{
    OFC_REQUIRE(L >= 1 && L <= 3 && pyramid_dec_levels(W0, H0, geom, L, ((uintptr_t)src % 4) == 0) == L,
                "k_pyramid_dec: levels 1..%d of %d x %d are not all exact decimations", L, W0, H0);
    PyrDecArgs p;
    memset(&p, 0, sizeof(p));
    p.W0 = W0; p.H0 = H0;
    int bands, strips;
    pyramid_dec_plan(W0, H0, nimg, bands, p.steps, p.sps, strips);
    for (int k = 1; k <= L; k++) {
        LevelArgs a;
        int path = 1;
        size_t lds = 0;
        OFC_TRY(level_image_plan(W0, H0, geom[k], true, a, path, lds));
        p.w[k - 1] = geom[k].w; p.h[k - 1] = geom[k].h;
        for (int q = 0; q < a.r; q++)
            OFC_REQUIRE(a.kern[q] == a.kern[2 * a.r - q], "k_pyramid_dec: level %d's kernel is not symmetric", k);
        memcpy(k == 1 ? p.k1 : k == 2 ? p.k2 : p.k3, a.kern, sizeof(float) * (a.r + 1));
    }
    const dim3 grid(bands, strips, nimg);
    float *d1 = dst[0], *d2 = L >= 2 ? dst[1] : nullptr, *d3 = L >= 3 ? dst[2] : nullptr;
    switch (L) {
    case 1: hipLaunchKernelGGL(k_pyramid_dec<1>, grid, dim3(256), 0, s, src, d1, d2, d3, p); break;
    case 2: hipLaunchKernelGGL(k_pyramid_dec<2>, grid, dim3(256), 0, s, src, d1, d2, d3, p); break;
    default: hipLaunchKernelGGL(k_pyramid_dec<3>, grid, dim3(256), 0, s, src, d1, d2, d3, p);
    }
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
