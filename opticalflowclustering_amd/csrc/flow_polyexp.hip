// flow_polyexp.hip -- K3, the polynomial expansion: level image (or, at level 0, the u8 frame) -> R.
// Layouts and the contraction policy: flow_device.h.
#include "flow_device.h"
#include "flow_host.h"

namespace ofc {

// ------------------------------------------------------------------------------------------------
// K3  polynomial expansion (the north-star kernel).  24 B/px algorithmic: 4 read + 20 written.
//
// Work-group = 256 threads = 4 waves, output strip 240 columns x rows_per_block rows, walked in chunks
// of 8 rows:
//   vertical pass   thread <-> column (240 + 2N halo columns, replicate-clamped; N = poly_n = 5 or 7).  Each thread
//                   keeps an (8 + 2N)-row register window of its column that slides down 8 rows per chunk; the 8 new rows
//                   are requested right after the barrier (lanes <-> x: coalesced), so their latency hides
//                   under the horizontal pass.  The window yields the three f32 moments t0,t1,t2 of 8 rows with
//                   the symmetric / antisymmetric tap pairing of the reference -> LDS, one float4 per pixel.
//   horizontal pass wave <-> row, lane <-> 4 consecutive x: 4 + 2N ds_read_b128 (forced whole, see lds_read4),
//                   accumulators as described in the loop, 5 float4 stores per lane (1 KiB/wave-instruction),
//                   staged through the moments row the wave has just read (no LDS beside the moments tile).
// 39 936 B LDS; at poly_n 5 the f32 form takes 112 VGPRs and the u8 form 123, so four work-groups share a CU (4 waves
// per SIMD); at poly_n 7 (132 / 143 VGPRs) three do.  DESIGN.md section 4 has the figures of every instantiation.
// Measured ceilings on MI355X for this traffic shape (tools/membench):
// 1 read : 5 write streams = 4.9 TB/s; this kernel's compute alone (stores off) = 5.9 TB/s-equivalent.
// ------------------------------------------------------------------------------------------------
// 16-byte LDS read that hipcc may not narrow: a plain float4 load whose tail elements are unused is split into
// ds_read2_b32 / ds_read2_b64, and with a 16-byte lane stride those are 8-way bank conflicts
// (SQ_LDS_BANK_CONFLICT 1.3e8 cycles per launch before this).  volatile keeps the access whole -> ds_read_b128.
__device__ __forceinline__ float4 lds_read4(const float *p)
{
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef const volatile v4f __attribute__((address_space(3))) * lds_v4f_ptr;
    const v4f v = *(lds_v4f_ptr)(p);          // explicit LDS address space: ds_read_b128, not flat_load
    return make_float4(v.x, v.y, v.z, v.w);
}

constexpr int PE_TX = 240;
constexpr int PE_CH = 8;
// float4 per (row, pixel & 3) plane of the moments tile.  Two things set it: 4 * PE_PLANE = 24 mod 32 dwords staggers
// the four planes over the banks (as 8 mod 32 does: 66, 74), and a row of four planes (4 992 B) holds a staged output
// row (240 px x 5 coefficients = 4 800 B), which 66 and 74 do not.  8 rows x 4 992 B = 39 936 B per work-group.
constexpr int PE_PLANE = 78;

// N = poly_n, the half-width of the expansion window (cv2 documents 5 and 7; both are instantiated)
template <int N>
struct PolyArgs {
    int W, H, rows_per_block;
    float g[N + 1], xg[N + 1], xxg[N + 1];
    double ig11, ig03, ig33, ig55;
};

// TAG only gives the bench hook's launches their own symbol in rocprof's kernel statistics.
// U8IN: the pyramid's level 0 (3x3 [1/4 1/2 1/4] blur of the u8 frame, REFLECT_101, no decimation) is evaluated on the
// fly from the frame instead of being read back as an f32 image: 1 B/px read instead of 4, and the level-0 image
// kernel with its 5 B/px disappears.  Every intermediate value of that blur is a multiple of 1/16 below 256, exactly
// representable in f32 whatever the evaluation order, so the result is bit-identical to k_level0 + this kernel; here the
// sums are formed as integers (16 x the sample, <= 4 080) and scaled once.
// F64H: the six horizontal sums exactly as the reference forms them (double accumulators; b1/b4 from double products, the
// other four from float products) -- a study / fallback build (OFC_POLYEXP_F64=1): see DESIGN.md section 2.
// N (last, so that the rocprof names of the poly_n=5 forms keep their prefix) is the window half-width: the strip needs
// VW = 240 + 2N columns (250 / 254 <= 256 threads), the horizontal pass 4 + 2N moments per lane, whose highest LDS index
// lane + (3 + 2N) / 4 = 63 at N = 7 stays inside the 78-float4 plane.
template <int TAG, bool U8IN, bool F64H = false, int N = 5>
__global__ __launch_bounds__(256, 3) void k_polyexp(const void *__restrict__ Iv, float *__restrict__ R,
                                                 PolyArgs<N> p)
{
    constexpr int VW = PE_TX + 2 * N;
    static_assert(VW <= 256 && (VW - 1) / 4 < PE_PLANE && PE_TX / 4 - 1 + (3 + 2 * N) / 4 < PE_PLANE,
                  "the strip and its halo must fit one work-group and one moments plane");
    // vertical moments of the chunk, one float4 (t0, t1, t2, t1) per pixel: the horizontal pass consumes them as the
    // register pairs (t0,t1) and (t2,t1), which is what lets it run on packed-f32 instructions.  Pixel p of the strip
    // lives at [p & 3][p >> 2]: lane l of the horizontal pass reads pixels 4l+j, so for a fixed j the 64 lanes touch 64
    // consecutive float4 of one plane (conflict-free ds_read_b128); planes are 78 float4 apart (312 dwords = 24 mod 32
    // banks) so that the vertical pass's writes, lane <-> pixel, spread over the banks as well.
    // Row rr is read by one wave only (rr = wave, wave + 4), whole, before that wave's first use of it; from then until
    // the next chunk's vertical pass (behind a work-group barrier) it is dead, and the wave stages its output row in it.
    static_assert(4 * PE_PLANE * 4 >= PE_TX * 5, "a moments row must hold a staged output row");
    __shared__ __align__(16) float4 t4[PE_CH][4][PE_PLANE];
    typedef float v2f __attribute__((ext_vector_type(2)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.W, H = p.H;
    const int x0 = blockIdx.x * PE_TX;
    const int y_begin = blockIdx.y * p.rows_per_block;
    const int y_end = min(y_begin + p.rows_per_block, H);
    const size_t plane = (size_t)W * H;
    const float *img = U8IN ? nullptr : reinterpret_cast<const float *>(Iv) + (size_t)blockIdx.z * plane;
    const uint8_t *img8 = U8IN ? reinterpret_cast<const uint8_t *>(Iv) + (size_t)blockIdx.z * plane : nullptr;
    float *out = R + (size_t)blockIdx.z * 5 * plane;
    const int xc = min(max(x0 - N + tid, 0), W - 1);   // this thread's (clamped) column
    const bool vec_ok = (W & 3) == 0;

    // U8IN: one (unaligned) dword per frame row holds the three horizontal taps of this column: bytes
    // reflect101(xc-1), xc, reflect101(xc+1) all lie in [base, base+3] for base = clamp(xc-1, 0, W-4)
    typedef uint32_t u32u __attribute__((aligned(1)));
    const int base = U8IN ? min(max(xc - 1, 0), W - 4) : 0;
    const int sh0 = U8IN ? 8 * (reflect101(xc - 1, W) - base) : 0, sh1 = U8IN ? 8 * (xc - base) : 0,
              sh2 = U8IN ? 8 * (reflect101(xc + 1, W) - base) : 0;
    auto hword = [&](int r) -> uint32_t { return *reinterpret_cast<const u32u *>(img8 + (size_t)r * W + base); };
    // The blur stays in integers until its last step: the row sum b(x-1) + 2 b(x) + b(x+1) <= 1 020 is one byte dot
    // product against a per-thread weight word (1, 2, 1 on the three selected bytes; weights add where reflection makes
    // two taps one byte), the column sum h(y-1) + 2 h(y) + h(y+1) <= 4 080 a shift-add and an add, and one conversion
    // and one multiply by 1/16 give the level-0 sample: the value the f32 taps give, every partial sum of which is exact.
    const uint32_t hwts = U8IN ? (1u << sh0) + (2u << sh1) + (1u << sh2) : 0u;
    auto hsum = [&](uint32_t w) -> uint32_t { return __builtin_amdgcn_udot4(w, hwts, 0u, false); };   // 4 x row-blurred sample
    auto i0_of = [&](uint32_t h0, uint32_t h1, uint32_t h2) -> float { return 0.0625f * (float)(h0 + 2u * h1 + h2); };
    auto i0_any = [&](int r) -> float {             // level-0 image at (valid) row r, any position: 3 row loads
        return i0_of(hsum(hword(reflect101(r - 1, H))), hsum(hword(r)), hsum(hword(reflect101(r + 1, H))));
    };
    // strips whose rows (incl. the +-1 blur rows) need neither clamping nor reflection share the row-blurred samples
    // between consecutive level-0 rows: 10 + 2N + 8 per chunk dword loads per thread, the count of the f32 path
    const bool interior = U8IN && y_begin >= N + 1 && y_begin + p.rows_per_block + 2 * N + 2 <= H - 1;

    // register window of this thread's column: rows yc-N .. yc+N+7; slides down 8 rows per chunk, the 8 new
    // rows are requested right after the barrier so that their HBM latency hides under the horizontal pass
    float s[8 + 2 * N], nxt[8];
    uint32_t nxtw[8];
    uint32_t hk0 = 0u, hk1 = 0u;                        // U8IN interior: row sums of window rows 8+2N, 9+2N
    if (!U8IN) {
#pragma unroll
        for (int j = 0; j < 8 + 2 * N; j++)
            s[j] = img[(size_t)min(max(y_begin - N + j, 0), H - 1) * W + xc];
    } else if (interior) {
        uint32_t hv[8 + 2 * N + 2];
#pragma unroll
        for (int j = 0; j < 8 + 2 * N + 2; j++) hv[j] = hsum(hword(y_begin - N - 1 + j));
#pragma unroll
        for (int j = 0; j < 8 + 2 * N; j++) s[j] = i0_of(hv[j], hv[j + 1], hv[j + 2]);
        hk0 = hv[8 + 2 * N];
        hk1 = hv[8 + 2 * N + 1];
    } else {
#pragma unroll
        for (int j = 0; j < 8 + 2 * N; j++) s[j] = i0_any(min(max(y_begin - N + j, 0), H - 1));
    }

    for (int yc = y_begin; yc < y_end; yc += PE_CH) {
        // ---- vertical pass ----
        // per tap pair: (a+b, b-a) in one packed add, (t0,t2) += (g,xxg)*(a+b) in one packed fma, t1 in a scalar fma:
        // 3 VALU instructions instead of 5, every lane-operation identical to the scalar form (same roundings)
        if (tid < VW) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                v2f t02 = {s[i + N] * p.g[0], 0.f};
                float t1 = 0.f;
#pragma unroll
                for (int k = 1; k <= N; k++) {
                    const float a = s[i + N - k], b = s[i + N + k];
                    const v2f pd = (v2f){b, b} + (v2f){a, -a};                     // (a + b, b - a)
                    t02 = __builtin_elementwise_fma((v2f){p.g[k], p.xxg[k]}, (v2f){pd.x, pd.x}, t02);
                    t1 = fmaf(p.xg[k], pd.y, t1);
                }
                t4[i][tid & 3][tid >> 2] = make_float4(t02.x, t1, t02.y, t1);
            }
        }
        __syncthreads();
        if (yc + PE_CH < y_end) {
            if (!U8IN) {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    nxt[j] = img[(size_t)min(yc + PE_CH + N + j, H - 1) * W + xc];
            } else if (interior) {
#pragma unroll
                for (int j = 0; j < 8; j++) nxtw[j] = hword(yc + PE_CH + N + 1 + j);   // frame rows yc+N+9 .. yc+N+16
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) nxt[j] = i0_any(min(yc + PE_CH + N + j, H - 1));
            }
        }
        // ---- horizontal pass ----
        for (int rr = wave; rr < PE_CH; rr += 4) {
            const int y = yc + rr;
            if (y >= y_end) break;
            const int xo = x0 + 4 * lane;
            float *const stage = reinterpret_cast<float *>(&t4[rr][0][0]);   // this wave's, once its moments are read
            if (lane < PE_TX / 4 && xo < W) {
                v2f A[4 + 2 * N], Q[4 + 2 * N];   // (t0, t1) and (t2, t1) of strip pixels 4*lane .. 4*lane + 3 + 2N
#pragma unroll
                for (int j = 0; j < 4 + 2 * N; j++) {
                    const float4 v = lds_read4(reinterpret_cast<const float *>(&t4[rr][j & 3][lane + (j >> 2)]));
                    A[j] = (v2f){v.x, v.y};
                    Q[j] = (v2f){v.z, v.w};
                }
                float r0[4], r1[4], r2[4], r3[4], r4[4];
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    const int c = o + N;
                    // The reference accumulates these six (2N+1)-tap sums in double.  Its inputs (the vertical moments) are
                    // f32 already, each sum has only 6 terms, and the one place where rounding is amplified -- b1*ig03
                    // cancelling against b4|b5*ig33 in the second-derivative coefficients -- is evaluated in f64 below.
                    // f32 FMA accumulation costs <= ~3 ulp per sum; measured effect on the flow vs the oracle:
                    // 4.7e-7 relative / 1.1e-4 px worst case incl. flat-bright and half-black frames (bar 1e-4 / 1e-3),
                    // the same as with f64 accumulators, for 40 % less time in this VALU-bound pass.
                    // packed over PAIRS OF SUMS (not pairs of pixels, whose operands would straddle register pairs):
                    // per tap pair 3 packed adds + 3 packed fmas instead of 5 + 6 scalar ones
                    float b1, b2, b3, b4, b5, b6;
                    double d1 = 0, d4 = 0, d5 = 0;
                    if (F64H) {
#pragma clang fp contract(off)
                        double e1 = (double)(A[c].x * p.g[0]), e2 = 0, e3 = (double)(A[c].y * p.g[0]), e4 = 0,
                               e5 = (double)(Q[c].x * p.g[0]), e6 = 0;
#pragma unroll
                        for (int k = 1; k <= N; k++) {
                            const double tg = (double)(A[c + k].x + A[c - k].x);
                            e1 += tg * (double)p.g[k];
                            e4 += tg * (double)p.xxg[k];
                            e2 += (double)((A[c + k].x - A[c - k].x) * p.xg[k]);
                            e3 += (double)((A[c + k].y + A[c - k].y) * p.g[k]);
                            e6 += (double)((A[c + k].y - A[c - k].y) * p.xg[k]);
                            e5 += (double)((Q[c + k].x + Q[c - k].x) * p.g[k]);
                        }
                        d1 = e1; d4 = e4; d5 = e5;
                        b1 = (float)e1; b4 = (float)e4; b5 = (float)e5;
                        r1[o] = (float)(e2 * p.ig11);
                        r0[o] = (float)(e3 * p.ig11);
                        r4[o] = (float)(e6 * p.ig55);
                        b2 = b3 = b6 = 0.f;
                    } else {
                    v2f b14 = {A[c].x * p.g[0], 0.f};                    // (b1, b4)
                    v2f b26 = {0.f, 0.f};                                // (b2, b6)
                    v2f b53 = Q[c] * (v2f){p.g[0], p.g[0]};              // (b5, b3)
#pragma unroll
                    for (int k = 1; k <= N; k++) {
                        const v2f sm = A[c + k] + A[c - k];              // (t0 sum, -)
                        const v2f df = A[c + k] - A[c - k];              // (t0 diff, t1 diff)
                        const v2f sq = Q[c + k] + Q[c - k];              // (t2 sum, t1 sum)
                        b14 = __builtin_elementwise_fma((v2f){sm.x, sm.x}, (v2f){p.g[k], p.xxg[k]}, b14);
                        b26 = __builtin_elementwise_fma(df, (v2f){p.xg[k], p.xg[k]}, b26);
                        b53 = __builtin_elementwise_fma(sq, (v2f){p.g[k], p.g[k]}, b53);
                    }
                    b1 = b14.x; b4 = b14.y; b2 = b26.x; b6 = b26.y; b5 = b53.x; b3 = b53.y;
                    }
                    if (F64H) {
#pragma clang fp contract(off)
                        r3[o] = (float)(d1 * p.ig03 + d4 * p.ig33);
                        r2[o] = (float)(d1 * p.ig03 + d5 * p.ig33);
                    } else {
                        r1[o] = b2 * (float)p.ig11;
                        r0[o] = b3 * (float)p.ig11;
                        r3[o] = (float)((double)b1 * p.ig03 + (double)b4 * p.ig33);
                        r2[o] = (float)((double)b1 * p.ig03 + (double)b5 * p.ig33);
                        r4[o] = b6 * (float)p.ig55;
                    }
                }
                // R is pixel-interleaved ([y][x][5], as OpenCV keeps it) so that the consumer's bilinear taps are two
                // 40-byte runs instead of 20 scattered dwords.  A lane's 4 px x 5 coefficients are 80 contiguous bytes;
                // storing them directly would make every wave-instruction write 16 B out of each 80 (measured: 5x
                // slower).  They cross the wave's own moments row instead (conflict-free at the 80-B lane stride) and
                // leave as five fully contiguous 1-KiB wave stores.  Every lane's moments are in registers by now (the
                // coefficients above depend on all of them); the wave barrier keeps the compiler from moving a staging
                // write of one lane above a moments read of another.
                if (vec_ok) {
                    __builtin_amdgcn_wave_barrier();
                    float *sg = stage + 20 * lane;
                    *reinterpret_cast<float4 *>(sg) = make_float4(r0[0], r1[0], r2[0], r3[0]);
                    *reinterpret_cast<float4 *>(sg + 4) = make_float4(r4[0], r0[1], r1[1], r2[1]);
                    *reinterpret_cast<float4 *>(sg + 8) = make_float4(r3[1], r4[1], r0[2], r1[2]);
                    *reinterpret_cast<float4 *>(sg + 12) = make_float4(r2[2], r3[2], r4[2], r0[3]);
                    *reinterpret_cast<float4 *>(sg + 16) = make_float4(r1[3], r2[3], r3[3], r4[3]);
                } else {
                    float *o0 = out + ((size_t)y * W + xo) * 5;
#pragma unroll
                    for (int o = 0; o < 4; o++)
                        if (xo + o < W) {
                            o0[o * 5] = r0[o]; o0[o * 5 + 1] = r1[o]; o0[o * 5 + 2] = r2[o];
                            o0[o * 5 + 3] = r3[o]; o0[o * 5 + 4] = r4[o];
                        }
                }
            }
            if (vec_ok) {     // wave-uniform; the staging row belongs to this wave only
                __builtin_amdgcn_wave_barrier();
                typedef float v4f __attribute__((ext_vector_type(4)));
                const int nf4 = min(PE_TX, W - x0) * 5 / 4;
                v4f *orow = reinterpret_cast<v4f *>(out + ((size_t)y * W + x0) * 5);
#pragma unroll
                for (int j = 0; j < 5; j++) {
                    const int idx = lane + 64 * j;
                    if (idx < nf4) {
                        const float4 v = lds_read4(stage + 4 * idx);
                        __builtin_nontemporal_store((v4f){v.x, v.y, v.z, v.w}, orow + idx);
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2 * N; j++) s[j] = s[j + 8];
        if (U8IN && interior) {
            uint32_t hn[10];
            hn[0] = hk0;
            hn[1] = hk1;
#pragma unroll
            for (int j = 0; j < 8; j++) hn[2 + j] = hsum(nxtw[j]);
#pragma unroll
            for (int j = 0; j < 8; j++) s[2 * N + j] = i0_of(hn[j], hn[j + 1], hn[j + 2]);
            hk0 = hn[8];
            hk1 = hn[9];
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) s[2 * N + j] = nxt[j];
        }
    }
}


// OFC_POLYEXP_F64=1: horizontal sums in double, as the reference (read at every launch: a test toggles it).  Built for
// poly_n = 5 only (it spills at 5 already): poly_n = 7 runs the f32 form whatever the switch says.
static bool polyexp_f64()
{
    const char *e = getenv("OFC_POLYEXP_F64");
    return e && e[0] == '1';
}

int polyexp_default_rows(int W, int H, int nimg)
{
    // 16-row strips: the 10-row window warm-up re-reads input rows that the strip above is reading at about the same
    // time (L2 hits), and the shorter strips keep more independent work-groups in flight -- measured 4.61 TB/s against
    // 4.38 (64 rows) .. 4.53 (32-48 rows) on 64 1080p images.  Shrink further only when the launch would not give
    // every CU a few work-groups.
    int tiles_x = cdiv(W, PE_TX);
    int rows = 16;
    while (rows > PE_CH && (int64_t)tiles_x * cdiv(H, rows) * nimg < 1024) rows >>= 1;
    return rows;
}

// the one launch of k_polyexp: the argument block, the grid (rows_per_block <= 0: the model's height) and the instantiation
// the caller chose
template <int TAG, bool U8IN, bool F64H, int N>
static int polyexp_launch(const void *in, float *R, int nimg, int W, int H, const PolyConsts &c, int rows_per_block,
                          hipStream_t s)
{
    PolyArgs<N> a;
    a.W = W; a.H = H;
    for (int i = 0; i <= N; i++) { a.g[i] = c.g[i]; a.xg[i] = c.xg[i]; a.xxg[i] = c.xxg[i]; }
    a.ig11 = c.ig11; a.ig03 = c.ig03; a.ig33 = c.ig33; a.ig55 = c.ig55;
    if (rows_per_block <= 0) rows_per_block = polyexp_default_rows(W, H, nimg);
    a.rows_per_block = cdiv(rows_per_block, PE_CH) * PE_CH;
    dim3 grid(cdiv(W, PE_TX), cdiv(H, a.rows_per_block), nimg);
    hipLaunchKernelGGL((k_polyexp<TAG, U8IN, F64H, N>), grid, dim3(256), 0, s, in, R, a);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int polyexp_n_check(int n)
{
    if (n == 5 || n == 7) return OFC_OK;
    set_error("poly_n=%d unsupported: the polyexp kernel is built for poly_n 5 and 7", n);
    return OFC_EUNSUPPORTED;
}

// polyexp of pyramid level 0 straight from the u8 frames (see U8IN); the caller checks polyexp_u8_ok()
bool polyexp_u8_ok(int W, int H, const LevelGeom &g)
{
    if (g.w != W || g.h != H || g.ksize != 3 || W < 4 || H < 2) return false;
    float k[3];
    gaussian_kernel(3, g.sigma, k);
    return k[0] == 0.25f && k[1] == 0.5f && k[2] == 0.25f;
}

int launch_polyexp_u8(const uint8_t *frames, float *R, int nimg, int W, int H, const PolyConsts &c, hipStream_t s)
{
    if (c.n == 5 && polyexp_f64()) return polyexp_launch<0, true, true, 5>(frames, R, nimg, W, H, c, 0, s);
    if (c.n == 5) return polyexp_launch<0, true, false, 5>(frames, R, nimg, W, H, c, 0, s);
    if (c.n == 7) return polyexp_launch<0, true, false, 7>(frames, R, nimg, W, H, c, 0, s);
    return polyexp_n_check(c.n);
}

int launch_polyexp(const float *I, float *R, int nimg, int W, int H, const PolyConsts &c,
                   int rows_per_block, hipStream_t s, bool bench_tag)
{
    if (c.n == 5 && polyexp_f64()) return polyexp_launch<2, false, true, 5>(I, R, nimg, W, H, c, rows_per_block, s);
    if (c.n == 5 && bench_tag) return polyexp_launch<1, false, false, 5>(I, R, nimg, W, H, c, rows_per_block, s);
    if (c.n == 5) return polyexp_launch<0, false, false, 5>(I, R, nimg, W, H, c, rows_per_block, s);
    if (c.n == 7 && bench_tag) return polyexp_launch<1, false, false, 7>(I, R, nimg, W, H, c, rows_per_block, s);
    if (c.n == 7) return polyexp_launch<0, false, false, 7>(I, R, nimg, W, H, c, rows_per_block, s);
    return polyexp_n_check(c.n);
}

}  // namespace ofc
