// fb_check.hip -- the forward-backward check of a flow field (ofc_consist*, ofc_frames_reverse_dev; the definition is in
// include/ofc.h).  The reference has no counterpart: it trusted every vector alike (computeOpticalFlowModule.py:20-22).
//
// k_fb_check: grid.y is the pair; a work-group takes FB_SHARE consecutive pixels of it in FB_PASSES passes, a lane a run of
// FB_RUN consecutive pixels per pass.  The forward vectors of a run are two 16-byte loads where every pair's base allows
// (VEC), the last short run of a pair and everything without VEC one 8-byte load per vector.  A run's sixteen backward taps
// are 8-byte gathers, issued together before any is used; neighbours move alike, so a wave's gathers fall on few lines.
// Every tap index is clamped into the frame before it indexes anything, whatever the fields hold, and no loop has a
// data-dependent trip count.  All arithmetic after the quantisation is integer, so the order of the work does not matter.
// The four counters: a lane keeps 16-bit fields (at most 8 pixels each), a wave adds them by shuffles (at most 512), the
// waves meet in LDS, and one 64-bit integer atomic per state and work-group goes to the pair's row.
// k_consist_mask: 16 states per lane as one 16-byte load where the bases allow, the rest one per lane.
#include "fb_check.h"

namespace ofc {

namespace {

constexpr int FB_THREADS = 256, FB_WAVES = FB_THREADS / 64, FB_RUN = 4, FB_PASSES = FB_SHARE / (FB_THREADS * FB_RUN);
static_assert(FB_PASSES * FB_THREADS * FB_RUN == FB_SHARE, "shares divide evenly");
static_assert(FB_PASSES * FB_RUN * 64 < 65536, "a wave's counts fit their 16-bit fields");

typedef unsigned long long u64;
typedef long long i64;

__device__ __forceinline__ unsigned fb_wave_add(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool VEC, bool RESID>
__global__ __launch_bounds__(FB_THREADS) void k_fb_check(const float2 *__restrict__ fwd, const float2 *__restrict__ bwd, int W, int H,
                                                         int npair, int bwd_reversed, i64 alpha_q, i64 beta_q,
                                                         uint8_t *__restrict__ state, u64 *__restrict__ counts, int2 *__restrict__ resid)
{
    __shared__ unsigned s_cnt[FB_WAVES][FB_NSTATE];
    const int P = W * H;                                               // <= 2^28
    const int t = blockIdx.y, tb = bwd_reversed ? npair - 1 - t : t;
    const float2 *F = fwd + (size_t)t * P, *B = bwd + (size_t)tb * P;
    uint8_t *St = state + (size_t)t * P;
    const int xmax = (W - 1) << 16, ymax = (H - 1) << 16;              // W, H <= 16384: below 2^30
    unsigned c01 = 0, c23 = 0;                                         // states 0 | 1 << 16, states 2 | 3 << 16

#pragma unroll
    for (int pass = 0; pass < FB_PASSES; pass++) {
        const int i = (int)blockIdx.x * FB_SHARE + pass * (FB_THREADS * FB_RUN) + (int)threadIdx.x * FB_RUN;   // < 2^28 + FB_SHARE
        if (i >= P) continue;
        const int nrun = min(FB_RUN, P - i);
        float2 f[FB_RUN];
        if (VEC && nrun == FB_RUN) {
            const float4 a = *reinterpret_cast<const float4 *>(F + i), b = *reinterpret_cast<const float4 *>(F + i + 2);
            f[0] = make_float2(a.x, a.y), f[1] = make_float2(a.z, a.w), f[2] = make_float2(b.x, b.y), f[3] = make_float2(b.z, b.w);
        } else {
#pragma unroll
            for (int q = 0; q < FB_RUN; q++) f[q] = q < nrun ? F[i + q] : make_float2(0.f, 0.f);
        }

        // where each pixel of the run lands: indices clamped whether or not they will be used
        FbVec v[FB_RUN];
        int st[FB_RUN], X[FB_RUN], Y[FB_RUN], i00[FB_RUN], i01[FB_RUN], i10[FB_RUN], i11[FB_RUN];
        int y = i / W, x = i - y * W;
#pragma unroll
        for (int q = 0; q < FB_RUN; q++) {
            v[q] = fb_quantise(f[q]);
            X[q] = (x << 16) + v[q].qu;                                // x <= 16383, |qu| < 2^26: fits int32
            Y[q] = (y << 16) + v[q].qv;
            const bool inside = X[q] >= 0 && X[q] <= xmax && Y[q] >= 0 && Y[q] <= ymax;
            st[q] = !v[q].valid ? OFC_CONSIST_INVALID : !inside || q >= nrun ? OFC_CONSIST_LEAVES : -1;     // -1: taps to read
            const int ix = min(max(X[q] >> 16, 0), W - 1), iy = min(max(Y[q] >> 16, 0), H - 1);
            const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
            i00[q] = iy * W + ix, i01[q] = iy * W + ix1, i10[q] = iy1 * W + ix, i11[q] = iy1 * W + ix1;      // all in [0, P)
            if (++x == W) { x = 0; y++; }
        }
        float2 b[FB_RUN][4];
#pragma unroll
        for (int q = 0; q < FB_RUN; q++) {
            b[q][0] = b[q][1] = b[q][2] = b[q][3] = make_float2(0.f, 0.f);
            if (st[q] < 0) {
                b[q][0] = B[i00[q]];
                b[q][1] = B[i01[q]];
                b[q][2] = B[i10[q]];
                b[q][3] = B[i11[q]];
            }
        }
        int ex[FB_RUN], ey[FB_RUN];
#pragma unroll
        for (int q = 0; q < FB_RUN; q++) {
            ex[q] = ey[q] = 0;
            if (st[q] < 0) {
                const FbVec t0 = fb_quantise(b[q][0]), t1 = fb_quantise(b[q][1]), t2 = fb_quantise(b[q][2]), t3 = fb_quantise(b[q][3]);
                const i64 fx = X[q] & 65535, fy = Y[q] & 65535;
                const i64 w0 = (65536 - fx) * (65536 - fy), w1 = fx * (65536 - fy), w2 = (65536 - fx) * fy, w3 = fx * fy;
                const i64 Sx = w0 * t0.qu + w1 * t1.qu + w2 * t2.qu + w3 * t3.qu;       // |S| <= 2^32 * 2^26
                const i64 Sy = w0 * t0.qv + w1 * t1.qv + w2 * t2.qv + w3 * t3.qv;
                const i64 Bx = (Sx + (1ll << 31)) >> 32, By = (Sy + (1ll << 31)) >> 32;
                const i64 rx = v[q].qu + Bx, ry = v[q].qv + By;                         // < 2^27
                const i64 d2 = rx * rx + ry * ry;
                const i64 m2 = (i64)v[q].qu * v[q].qu + (i64)v[q].qv * v[q].qv + Bx * Bx + By * By;
                if (!(t0.valid && t1.valid && t2.valid && t3.valid)) {
                    st[q] = OFC_CONSIST_INVALID;
                } else {
                    st[q] = d2 <= (m2 >> 16) * alpha_q + beta_q ? OFC_CONSIST_OK : OFC_CONSIST_MISMATCH;
                    ex[q] = (int)rx, ey[q] = (int)ry;
                }
            }
            if (q < nrun) {
                const unsigned inc = 1u << ((st[q] & 1) * 16);
                if (st[q] < 2) c01 += inc; else c23 += inc;
            }
        }

        uint8_t *sp = St + i;
        if (nrun == FB_RUN && ((uintptr_t)sp & 3) == 0) {
            *reinterpret_cast<uint32_t *>(sp) = (unsigned)st[0] | (unsigned)st[1] << 8 | (unsigned)st[2] << 16 | (unsigned)st[3] << 24;
        } else {
#pragma unroll
            for (int q = 0; q < FB_RUN; q++)
                if (q < nrun) sp[q] = (uint8_t)st[q];
        }
        if (RESID) {
            int2 *rp = resid + (size_t)t * P + i;
            if (nrun == FB_RUN && ((uintptr_t)rp & 15) == 0) {
                *reinterpret_cast<int4 *>(rp) = make_int4(ex[0], ey[0], ex[1], ey[1]);
                *reinterpret_cast<int4 *>(rp + 2) = make_int4(ex[2], ey[2], ex[3], ey[3]);
            } else {
#pragma unroll
                for (int q = 0; q < FB_RUN; q++)
                    if (q < nrun) rp[q] = make_int2(ex[q], ey[q]);
            }
        }
    }

    c01 = fb_wave_add(c01);
    c23 = fb_wave_add(c23);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_cnt[wave][0] = c01 & 0xffffu, s_cnt[wave][1] = c01 >> 16;
        s_cnt[wave][2] = c23 & 0xffffu, s_cnt[wave][3] = c23 >> 16;
    }
    __syncthreads();
    if (threadIdx.x < FB_NSTATE) {
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < FB_WAVES; w++) sum += s_cnt[w][threadIdx.x];
        if (sum) atomicAdd(counts + (size_t)t * FB_NSTATE + threadIdx.x, (u64)sum);
    }
}

__device__ __forceinline__ bool fb_kept(unsigned s, unsigned keep) { return s < (unsigned)FB_NSTATE && ((keep >> s) & 1u); }

// the four key bytes of k, each 255 where its state byte in s is not kept
__device__ __forceinline__ unsigned fb_mask_keys(unsigned s, unsigned k, unsigned keep)
{
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (!fb_kept((s >> (8 * j)) & 255u, keep)) k |= 255u << (8 * j);
    return k;
}

__device__ __forceinline__ float4 fb_mask_w(unsigned s, float4 v, unsigned keep)
{
    return make_float4(fb_kept(s & 255u, keep) ? v.x : 0.f, fb_kept((s >> 8) & 255u, keep) ? v.y : 0.f,
                       fb_kept((s >> 16) & 255u, keep) ? v.z : 0.f, fb_kept(s >> 24, keep) ? v.w : 0.f);
}

template <bool VEC>
__global__ __launch_bounds__(FB_THREADS) void k_consist_mask(const uint8_t *__restrict__ state, i64 n, unsigned keep,
                                                             uint8_t *__restrict__ keys, float *__restrict__ w)
{
    const i64 stride = (i64)gridDim.x * FB_THREADS, t0 = (i64)blockIdx.x * FB_THREADS + threadIdx.x;
    const i64 n16 = VEC ? n / 16 : 0;
    for (i64 g = t0; g < n16; g += stride) {
        const uint4 s = reinterpret_cast<const uint4 *>(state)[g];
        if (keys) {
            uint4 k = reinterpret_cast<uint4 *>(keys)[g];
            k.x = fb_mask_keys(s.x, k.x, keep), k.y = fb_mask_keys(s.y, k.y, keep);
            k.z = fb_mask_keys(s.z, k.z, keep), k.w = fb_mask_keys(s.w, k.w, keep);
            reinterpret_cast<uint4 *>(keys)[g] = k;
        }
        if (w) {
            float4 *wp = reinterpret_cast<float4 *>(w) + 4 * g;
            const float4 a = wp[0], b = wp[1], c = wp[2], d = wp[3];
            wp[0] = fb_mask_w(s.x, a, keep), wp[1] = fb_mask_w(s.y, b, keep);
            wp[2] = fb_mask_w(s.z, c, keep), wp[3] = fb_mask_w(s.w, d, keep);
        }
    }
    for (i64 i = 16 * n16 + t0; i < n; i += stride) {
        if (fb_kept(state[i], keep)) continue;
        if (keys) keys[i] = 255;
        if (w) w[i] = 0.f;
    }
}

}  // namespace

int fb_check(int W, int H, int npair, int64_t alpha_q, int64_t beta_q)
{
    OFC_REQUIRE(W >= 1 && H >= 1, "W = %d, H = %d: at least 1", W, H);
    OFC_REQUIRE(npair >= 1 && npair <= FB_MAX_PAIRS, "npair = %d: 1 .. %d", npair, FB_MAX_PAIRS);
    OFC_REQUIRE(alpha_q >= 0 && alpha_q <= OFC_CONSIST_ALPHA_MAX, "alpha_q = %lld: 0 .. 65536", (long long)alpha_q);
    OFC_REQUIRE(beta_q >= 0 && beta_q <= OFC_CONSIST_BETA_MAX, "beta_q = %lld: 0 .. 2^62", (long long)beta_q);
    if (W > FB_MAX_DIM || H > FB_MAX_DIM) {
        set_error("W = %d, H = %d: at most %d each (a landing position is an int32 in 1/65536 px)", W, H, FB_MAX_DIM);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

int launch_fb_check(const float *fwd, const float *bwd, int W, int H, int npair, bool bwd_reversed, int64_t alpha_q, int64_t beta_q,
                    uint8_t *state, int64_t *counts, int32_t *resid, hipStream_t s)
{
    const int P = W * H;
    OFC_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * FB_NSTATE * (size_t)npair, s));
    // a pair's base is fwd + pair * P * 8 bytes and a run starts at a multiple of four vectors
    const bool vec = ((uintptr_t)fwd & 15) == 0 && (P % 2 == 0 || npair == 1);
    auto kern = vec ? (resid ? &k_fb_check<true, true> : &k_fb_check<true, false>)
                    : (resid ? &k_fb_check<false, true> : &k_fb_check<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(P, FB_SHARE), npair), dim3(FB_THREADS), 0, s, reinterpret_cast<const float2 *>(fwd),
                       reinterpret_cast<const float2 *>(bwd), W, H, npair, (int)bwd_reversed, (i64)alpha_q, (i64)beta_q, state,
                       reinterpret_cast<u64 *>(counts), reinterpret_cast<int2 *>(resid));
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_consist_mask(const uint8_t *state, int64_t n, int keep, uint8_t *keys, float *w, hipStream_t s)
{
    if (!keys && !w) return OFC_OK;
    const bool vec = (((uintptr_t)state | (uintptr_t)keys | (uintptr_t)w) & 15) == 0;      // a null pointer allows it
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(vec ? cdiv64(n, 16) : n, FB_THREADS), 8192));
    auto kern = vec ? &k_consist_mask<true> : &k_consist_mask<false>;
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(FB_THREADS), 0, s, state, (i64)n, (unsigned)keep, keys, w);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_frames_reverse(const uint8_t *frames, size_t bytes, int n, uint8_t *out, hipStream_t s)
{
    for (int i = 0; i < n; i++)
        OFC_HIP(hipMemcpyAsync(out + (size_t)i * bytes, frames + (size_t)(n - 1 - i) * bytes, bytes, hipMemcpyDeviceToDevice, s));
    return OFC_OK;
}

}  // namespace ofc
