// photo_check.hip -- the photometric check of a flow field (ofc_photo*; the definition is in include/ofc.h): follow a pixel of
// frame t by its vector into frame t+1, interpolate that frame there, compare with the pixel's own grey value.  The
// reference has no counterpart: it trusted every vector alike (computeOpticalFlowModule.py:20-22).
//
// k_photo_check: shaped like k_fb_check.  grid.y is the pair; a work-group takes PHOTO_SHARE consecutive pixels of it in
// PH_PASSES passes, a lane a run of PH_RUN consecutive pixels per pass.  The forward vectors of a run are two 16-byte loads
// where every pair's base allows (VEC), the last short run of a pair and everything without VEC one 8-byte load per vector.
// The run's four grey values of frame t are one 4-byte load where that address allows, single bytes otherwise.  A run's
// sixteen taps of frame t+1 are single-byte gathers, issued together before any is used; neighbours move alike, so a wave's
// gathers fall on few lines.  Every tap index is clamped into the frame before it indexes anything, whatever the field
// holds, and no loop has a data-dependent trip count.  All arithmetic after the quantisation is integer, so the order of the
// work does not matter.  The five statistics: a lane keeps 16-bit count fields (at most 8 pixels each) and a 32-bit sum of
// |e| (at most 8 * 65280), a wave adds them by shuffles, the waves meet in LDS, and one 64-bit integer atomic per statistic
// and work-group (its sum of |e| is below 2^27) goes to the pair's row.
#include "photo_check.h"

namespace ofc {

namespace {

constexpr int PH_THREADS = 256, PH_WAVES = PH_THREADS / 64, PH_RUN = 4, PH_PASSES = PHOTO_SHARE / (PH_THREADS * PH_RUN);
static_assert(PH_PASSES * PH_THREADS * PH_RUN == PHOTO_SHARE, "shares divide evenly");
static_assert(PH_PASSES * PH_RUN * 64 < 65536, "a wave's counts fit their 16-bit fields");
static_assert((long long)PHOTO_SHARE * OFC_PHOTO_TAU_MAX < (1ll << 32), "a work-group's sum of |e| fits 32 bits");

typedef unsigned long long u64;

struct PhVec {
    int qu, qv;
    bool valid;
};

// the camera, blob and FB blocks' test and quantisation (fb_check.hip): an invalid vector quantises to 0
__device__ __forceinline__ PhVec ph_quantise(float2 f)
{
    const bool valid = fabsf(f.x) < 1024.f && fabsf(f.y) < 1024.f;     // NaN and inf fail
    PhVec q;
    q.qu = valid ? __double2int_rn((double)f.x * 65536.0) : 0;
    q.qv = valid ? __double2int_rn((double)f.y * 65536.0) : 0;
    q.valid = valid;
    return q;
}

__device__ __forceinline__ unsigned ph_wave_add(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool VEC, bool WARPED>
__global__ __launch_bounds__(PH_THREADS) void k_photo_check(const uint8_t *__restrict__ frames, const float2 *__restrict__ fwd, int W,
                                                            int H, int tau_q, int kappa_q, uint8_t *__restrict__ state,
                                                            u64 *__restrict__ stats, uint16_t *__restrict__ warped)
{
    __shared__ unsigned s_stat[PH_WAVES][PHOTO_NSTAT];
    const int P = W * H;                                               // <= 2^28
    const int t = blockIdx.y;
    const uint8_t *I0 = frames + (size_t)t * P, *I1 = I0 + P;
    const float2 *F = fwd + (size_t)t * P;
    uint8_t *St = state + (size_t)t * P;
    const int xmax = (W - 1) << 16, ymax = (H - 1) << 16;              // W, H <= 16384: below 2^30
    unsigned c01 = 0, c23 = 0, esum = 0;                               // states 0 | 1 << 16, states 2 | 3 << 16, sum of |e|

#pragma unroll
    for (int pass = 0; pass < PH_PASSES; pass++) {
        const int i = (int)blockIdx.x * PHOTO_SHARE + pass * (PH_THREADS * PH_RUN) + (int)threadIdx.x * PH_RUN;   // < 2^28 + PHOTO_SHARE
        if (i >= P) continue;
        const int nrun = min(PH_RUN, P - i);
        float2 f[PH_RUN];
        if (VEC && nrun == PH_RUN) {
            const float4 a = *reinterpret_cast<const float4 *>(F + i), b = *reinterpret_cast<const float4 *>(F + i + 2);
            f[0] = make_float2(a.x, a.y), f[1] = make_float2(a.z, a.w), f[2] = make_float2(b.x, b.y), f[3] = make_float2(b.z, b.w);
        } else {
#pragma unroll
            for (int q = 0; q < PH_RUN; q++) {
                f[q] = make_float2(0.f, 0.f);
                if (q < nrun) f[q] = F[i + q];
            }
        }
        int g0[PH_RUN];                                                // the run's own grey values, frame t
        const uint8_t *p0 = I0 + i;
        if (nrun == PH_RUN && ((uintptr_t)p0 & 3) == 0) {
            const unsigned w = *reinterpret_cast<const uint32_t *>(p0);
            g0[0] = w & 255u, g0[1] = (w >> 8) & 255u, g0[2] = (w >> 16) & 255u, g0[3] = w >> 24;
        } else {
#pragma unroll
            for (int q = 0; q < PH_RUN; q++) {
                g0[q] = 0;
                if (q < nrun) g0[q] = p0[q];
            }
        }

        // where each pixel of the run lands: indices clamped whether or not they will be used
        int st[PH_RUN], fx[PH_RUN], fy[PH_RUN], i00[PH_RUN], i01[PH_RUN], i10[PH_RUN], i11[PH_RUN];
        int y = i / W, x = i - y * W;
#pragma unroll
        for (int q = 0; q < PH_RUN; q++) {
            const PhVec v = ph_quantise(f[q]);
            const int X = (x << 16) + v.qu, Y = (y << 16) + v.qv;      // x <= 16383, |qu| < 2^26: fits int32
            const bool inside = X >= 0 && X <= xmax && Y >= 0 && Y <= ymax;
            st[q] = !v.valid ? OFC_CONSIST_INVALID : !inside || q >= nrun ? OFC_CONSIST_LEAVES : -1;         // -1: taps to read
            fx[q] = X & 65535, fy[q] = Y & 65535;
            const int ix = min(max(X >> 16, 0), W - 1), iy = min(max(Y >> 16, 0), H - 1);
            const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
            i00[q] = iy * W + ix, i01[q] = iy * W + ix1, i10[q] = iy1 * W + ix, i11[q] = iy1 * W + ix1;      // all in [0, P)
            if (++x == W) { x = 0; y++; }
        }
        int a[PH_RUN][4];
#pragma unroll
        for (int q = 0; q < PH_RUN; q++) {
            a[q][0] = a[q][1] = a[q][2] = a[q][3] = 0;
            if (st[q] < 0) {
                a[q][0] = I1[i00[q]];
                a[q][1] = I1[i01[q]];
                a[q][2] = I1[i10[q]];
                a[q][3] = I1[i11[q]];
            }
        }
        int J[PH_RUN];
#pragma unroll
        for (int q = 0; q < PH_RUN; q++) {
            J[q] = 0;
            if (st[q] < 0) {
                const unsigned top = (unsigned)a[q][0] * (unsigned)(65536 - fx[q]) + (unsigned)a[q][1] * (unsigned)fx[q];   // < 2^24
                const unsigned bot = (unsigned)a[q][2] * (unsigned)(65536 - fx[q]) + (unsigned)a[q][3] * (unsigned)fx[q];
                const u64 S = (u64)top * (unsigned)(65536 - fy[q]) + (u64)bot * (unsigned)fy[q];                             // < 2^40
                J[q] = (int)((S + (1ull << 23)) >> 24);                                                                      // 0 .. 65280
                const int e = abs(J[q] - 256 * g0[q]);
                const int c = max(max(a[q][0], a[q][1]), max(a[q][2], a[q][3])) - min(min(a[q][0], a[q][1]), min(a[q][2], a[q][3]));
                st[q] = e <= tau_q + kappa_q * c ? OFC_CONSIST_OK : OFC_CONSIST_MISMATCH;       // at most 65280 + 1024 * 255
                esum += (unsigned)e;
            }
            if (q < nrun) {
                const unsigned inc = 1u << ((st[q] & 1) * 16);
                if (st[q] < 2) c01 += inc; else c23 += inc;
            }
        }

        uint8_t *sp = St + i;
        if (nrun == PH_RUN && ((uintptr_t)sp & 3) == 0) {
            *reinterpret_cast<uint32_t *>(sp) = (unsigned)st[0] | (unsigned)st[1] << 8 | (unsigned)st[2] << 16 | (unsigned)st[3] << 24;
        } else {
#pragma unroll
            for (int q = 0; q < PH_RUN; q++)
                if (q < nrun) sp[q] = (uint8_t)st[q];
        }
        if (WARPED) {
            uint16_t *wp = warped + (size_t)t * P + i;
            if (nrun == PH_RUN && ((uintptr_t)wp & 7) == 0) {
                *reinterpret_cast<uint2 *>(wp) = make_uint2((unsigned)J[0] | (unsigned)J[1] << 16, (unsigned)J[2] | (unsigned)J[3] << 16);
            } else {
#pragma unroll
                for (int q = 0; q < PH_RUN; q++)
                    if (q < nrun) wp[q] = (uint16_t)J[q];
            }
        }
    }

    c01 = ph_wave_add(c01);
    c23 = ph_wave_add(c23);
    esum = ph_wave_add(esum);                                          // at most 512 * 65280 < 2^25
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_stat[wave][0] = c01 & 0xffffu, s_stat[wave][1] = c01 >> 16;
        s_stat[wave][2] = c23 & 0xffffu, s_stat[wave][3] = c23 >> 16;
        s_stat[wave][4] = esum;
    }
    __syncthreads();
    if (threadIdx.x < PHOTO_NSTAT) {
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < PH_WAVES; w++) sum += s_stat[w][threadIdx.x];
        if (sum) atomicAdd(stats + (size_t)t * PHOTO_NSTAT + threadIdx.x, (u64)sum);
    }
}

}  // namespace

int photo_check(int W, int H, int npair, int tau_q, int kappa_q)
{
    OFC_REQUIRE(W >= 1 && H >= 1, "W = %d, H = %d: at least 1", W, H);
    OFC_REQUIRE(npair >= 1 && npair <= PHOTO_MAX_PAIRS, "npair = %d: 1 .. %d", npair, PHOTO_MAX_PAIRS);
    OFC_REQUIRE(tau_q >= 0 && tau_q <= OFC_PHOTO_TAU_MAX, "tau_q = %d: 0 .. %d", tau_q, OFC_PHOTO_TAU_MAX);
    OFC_REQUIRE(kappa_q >= 0 && kappa_q <= OFC_PHOTO_KAPPA_MAX, "kappa_q = %d: 0 .. %d", kappa_q, OFC_PHOTO_KAPPA_MAX);
    if (W > PHOTO_MAX_DIM || H > PHOTO_MAX_DIM) {
        set_error("W = %d, H = %d: at most %d each (a landing position is an int32 in 1/65536 px)", W, H, PHOTO_MAX_DIM);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

int launch_photo_check(const uint8_t *frames, const float *fwd, int W, int H, int npair, int tau_q, int kappa_q, uint8_t *state,
                       int64_t *stats, uint16_t *warped, hipStream_t s)
{
    const int P = W * H;
    OFC_HIP(hipMemsetAsync(stats, 0, sizeof(int64_t) * PHOTO_NSTAT * (size_t)npair, s));
    // a pair's base is fwd + pair * P * 8 bytes and a run starts at a multiple of four vectors
    const bool vec = ((uintptr_t)fwd & 15) == 0 && (P % 2 == 0 || npair == 1);
    auto kern = vec ? (warped ? &k_photo_check<true, true> : &k_photo_check<true, false>)
                    : (warped ? &k_photo_check<false, true> : &k_photo_check<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(P, PHOTO_SHARE), npair), dim3(PH_THREADS), 0, s, frames,
                       reinterpret_cast<const float2 *>(fwd), W, H, tau_q, kappa_q, state, reinterpret_cast<u64 *>(stats), warped);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
