// motion_model.hip -- per-pair camera motion: fit a translation or an affine model to every pair's flow field by
// iteratively re-selected least squares, and subtract it (ofc_motion_fit_dev, ofc_motion_subtract_dev, the streaming
// ingest's camera).  Everything after the flow assumes a fixed camera; this gives it the field it assumes.
//
// Definition (include/ofc.h repeats it): X = 2x - (W-1), Y = 2y - (H-1); model p0..p5, u^ = fma(p2, Y/2, fma(p1, X/2, p0)),
// v^ likewise from p3..p5, in f64.  A vector is valid iff u, v are finite and |u|, |v| < 1024.  qu = llrint((double)u * 65536).
// Moments over a set S of valid pixels, thirteen int64: n, SX, SY, SXX, SXY, SYY, Squ, SXqu, SYqu, Sqv, SXqv, SYqv, outside.
// Round 0: S = every valid pixel.  Round t: S = valid pixels with (u-u^)^2 + (v-v^)^2 <= c_t^2 under round t-1's model.
// Integers only: whatever the order of the adds, equal bits.
//
// Shape.  k_motion_moments: grid (groups, pairs), four waves per work-group; a work-group takes ceil(shares / groups)
// consecutive shares of MOTION_SHARE vectors of its pair.  Each wave owns 512 consecutive vectors of a share and reads them
// as eight loads of 64 consecutive vectors (512 B per load, all eight in flight), as uv_hist.hip does.  A lane divides once
// per share for its first (x, y) and steps the other seven by (64 % W, 64 / W).  The pair's record (model, c^2) is uniform
// per work-group and read with scalar loads.  Twelve int64 accumulators per lane; X, Y, qu, qv stay int32 so that every
// product term is one 64-bit multiply-add (v_mad_i64_i32).  At the end: a wave fold (six exchanges per value), four waves
// through LDS, and thirteen plain vector stores of the work-group's partial record.  k_motion_solve adds the partials up.
// Partials, not atomics: both are exact, but partials need no zeroed record, so the T + 1 rounds of a fit chain without a
// clearing pass between them, and a record is written by exactly one work-group.
// k_motion_solve: one wave per pair adds the pair's partials, lane 0 runs motion_solve (motion_model.h, the function the
// host runs too), writes the record for the next round and appends to the history.
// k_motion_subtract: the same walk; eight bytes read and eight written per vector.
#include "motion_model.h"

#include <algorithm>
#include <cmath>

namespace ofc {

namespace {

constexpr int MM_THREADS = 256, MM_WAVES = MM_THREADS / 64, MM_UNROLL = MOTION_SHARE / MM_THREADS;
static_assert(MM_UNROLL == 8, "a lane holds eight vectors of a share");

__device__ __forceinline__ long long mm_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the walk both kernels share: lane's vector q of share g is i0 + 64 q; (x, y) of i0 by one division, then steps
struct MmWalk {
    int x, y, dx, dy, W;
    __device__ __forceinline__ MmWalk(int i0, int W_) : W(W_)
    {
        y = i0 / W_;
        x = i0 - y * W_;
        dy = 64 / W_;
        dx = 64 - dy * W_;
    }
    __device__ __forceinline__ void step()
    {
        x += dx;
        y += dy;
        if (x >= W) { x -= W; y++; }
    }
};

// flow [npair][H][W][2] f32, rec [npair] -> partial [npair][gridDim.x][13].  AFFINE = false: n, Squ, Sqv, outside only.
template <bool AFFINE>
__global__ __launch_bounds__(MM_THREADS) void k_motion_moments(const float2 *__restrict__ flow, int W, int H,
                                                               const MotionRec *__restrict__ rec,
                                                               long long *__restrict__ partial)
{
    __shared__ long long s_part[MM_WAVES][MOTION_NMOM];
    const int pair = blockIdx.y;
    const MotionRec r = rec[pair];                         // uniform: scalar loads
    if (r.status != 0) return;                             // the pair takes no further rounds; nobody reads its partials
    const int P = W * H;                                   // < 2^25 (motion_check)
    const float2 *f = flow + (size_t)pair * P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nshare = motion_nshare(W, H), per = motion_per(nshare, (int)gridDim.x);
    const int g1 = min(nshare, ((int)blockIdx.x + 1) * per);
    const int X0 = W - 1, Y0 = H - 1;
    const bool use = r.use != 0;

    long long a[12];
#pragma unroll
    for (int k = 0; k < 12; k++) a[k] = 0;
    int outside = 0;
    for (int g = blockIdx.x * per; g < g1; g++) {
        const int i0 = g * MOTION_SHARE + wave * (MOTION_SHARE / MM_WAVES) + lane;
        float2 v[MM_UNROLL];
#pragma unroll
        for (int q = 0; q < MM_UNROLL; q++) {
            const int i = i0 + q * 64;
            v[q] = i < P ? f[i] : make_float2(0.f, 0.f);
        }
        MmWalk w(i0, W);
#pragma unroll
        for (int q = 0; q < MM_UNROLL; q++) {
            const bool have = i0 + q * 64 < P;
            const bool valid = have && fabsf(v[q].x) < 1024.f && fabsf(v[q].y) < 1024.f;     // NaN and inf fail
            const int X = 2 * w.x - X0, Y = 2 * w.y - Y0;
            bool in = valid;
            if (use) {
                const double hx = 0.5 * (double)X, hy = 0.5 * (double)Y;
                const double du = (double)v[q].x - fma(r.p[2], hy, fma(r.p[1], hx, r.p[0]));
                const double dv = (double)v[q].y - fma(r.p[5], hy, fma(r.p[4], hx, r.p[3]));
                in = valid && du * du + dv * dv <= r.c2;
            }
            outside += have && !valid;
            // valid: |u| < 2^10, so the fixed-point value is an integer of magnitude < 2^26, exact in f64
            const int qu = in ? __double2int_rn((double)v[q].x * 65536.0) : 0;
            const int qv = in ? __double2int_rn((double)v[q].y * 65536.0) : 0;
            a[0] += in;
            a[6] += qu;
            a[9] += qv;
            if (AFFINE) {
                const int Xs = in ? X : 0, Ys = in ? Y : 0;
                a[1] += Xs;
                a[2] += Ys;
                a[3] += (long long)Xs * Xs;
                a[4] += (long long)Xs * Ys;
                a[5] += (long long)Ys * Ys;
                a[7] += (long long)Xs * qu;
                a[8] += (long long)Ys * qu;
                a[10] += (long long)Xs * qv;
                a[11] += (long long)Ys * qv;
            }
            w.step();
        }
    }
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const long long t = mm_wave_sum(a[k]);
        if (lane == 0) s_part[wave][k] = t;
    }
    const long long to = mm_wave_sum((long long)outside);
    if (lane == 0) s_part[wave][12] = to;
    __syncthreads();
    if (threadIdx.x < MOTION_NMOM) {
        long long t = 0;
#pragma unroll
        for (int wv = 0; wv < MM_WAVES; wv++) t += s_part[wv][threadIdx.x];
        partial[((size_t)pair * gridDim.x + blockIdx.x) * MOTION_NMOM + threadIdx.x] = t;
    }
}

// one wave per pair: partial [npair][groups][13] -> rec [npair], history rows of `round` (either may be nullptr)
__global__ __launch_bounds__(64) void k_motion_solve(const long long *__restrict__ partial, int groups, int npair, int kind,
                                                     int round, double c_next, MotionRec *__restrict__ rec,
                                                     double *__restrict__ hist_models, long long *__restrict__ hist_moments)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    const bool taken = rec[pair].status == 0;              // uniform
    long long m[MOTION_NMOM];
#pragma unroll
    for (int k = 0; k < MOTION_NMOM; k++) m[k] = 0;
    if (taken) {
        for (int g = lane; g < groups; g += 64) {
            const long long *p = partial + ((size_t)pair * groups + g) * MOTION_NMOM;
#pragma unroll
            for (int k = 0; k < MOTION_NMOM; k++) m[k] += p[k];
        }
#pragma unroll
        for (int k = 0; k < MOTION_NMOM; k++) m[k] = mm_wave_sum(m[k]);
    }
    if (lane != 0) return;
    MotionRec r = rec[pair];
    if (taken) {
        int64_t mi[MOTION_NMOM];
        for (int k = 0; k < MOTION_NMOM; k++) mi[k] = (int64_t)m[k];
        if (!motion_solve(mi, kind, r.p)) {                // r.p keeps the round before's model; all zeros in round 0
            r.status = round == 0 ? 2 : 1;
        }
        r.c2 = c_next * c_next;
        r.use = 1;
        rec[pair] = r;
    }
    if (hist_models)
        for (int k = 0; k < 6; k++) hist_models[((size_t)round * npair + pair) * 6 + k] = r.p[k];
    if (hist_moments)
        for (int k = 0; k < MOTION_NMOM; k++) hist_moments[((size_t)round * npair + pair) * MOTION_NMOM + k] = m[k];
}

// dst = flow - model, per pair; non-finite vectors pass through.  dst may be flow: a lane writes what it read.
__global__ __launch_bounds__(MM_THREADS) void k_motion_subtract(const float2 *flow, float2 *dst, int W, int H,
                                                                const MotionRec *__restrict__ rec)
{
    const int pair = blockIdx.y;
    const MotionRec r = rec[pair];                         // uniform: scalar loads
    const int P = W * H;
    const float2 *f = flow + (size_t)pair * P;
    float2 *o = dst + (size_t)pair * P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nshare = motion_nshare(W, H), per = motion_per(nshare, (int)gridDim.x);
    const int g1 = min(nshare, ((int)blockIdx.x + 1) * per);
    const int X0 = W - 1, Y0 = H - 1;
    for (int g = blockIdx.x * per; g < g1; g++) {
        const int i0 = g * MOTION_SHARE + wave * (MOTION_SHARE / MM_WAVES) + lane;
        float2 v[MM_UNROLL];
#pragma unroll
        for (int q = 0; q < MM_UNROLL; q++) {
            const int i = i0 + q * 64;
            v[q] = i < P ? f[i] : make_float2(0.f, 0.f);
        }
        MmWalk w(i0, W);
#pragma unroll
        for (int q = 0; q < MM_UNROLL; q++) {
            const int i = i0 + q * 64;
            const double hx = 0.5 * (double)(2 * w.x - X0), hy = 0.5 * (double)(2 * w.y - Y0);
            const double eu = fma(r.p[2], hy, fma(r.p[1], hx, r.p[0])), ev = fma(r.p[5], hy, fma(r.p[4], hx, r.p[3]));
            const bool finite = fabsf(v[q].x) < INFINITY && fabsf(v[q].y) < INFINITY;        // NaN fails the compare
            float2 out = v[q];
            if (finite) out = make_float2((float)((double)v[q].x - eu), (float)((double)v[q].y - ev));
            if (i < P) o[i] = out;
            w.step();
        }
    }
}

}  // namespace

int motion_check(int W, int H, int kind)
{
    OFC_REQUIRE(kind == 1 || kind == 2, "kind = %d is neither 1 (translation) nor 2 (affine)", kind);
    OFC_REQUIRE(W >= 1 && H >= 1, "W = %d, H = %d: a frame has at least one pixel", W, H);
    OFC_REQUIRE(kind == 1 || (W >= 2 && H >= 2), "an affine model needs W >= 2 and H >= 2, got %d x %d", W, H);
    // the moments fit int64 iff W * H * max(W, H) < 2^37
    const unsigned __int128 vol = (unsigned __int128)W * (unsigned)H * (unsigned)std::max(W, H);
    if (vol >= ((unsigned __int128)1 << 37)) {
        set_error("%d x %d: the moments fit int64 only while W * H * max(W, H) < 2^37", W, H);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

int motion_fit_check(int W, int H, int kind, const double *thresholds, int T)
{
    OFC_TRY(motion_check(W, H, kind));
    OFC_REQUIRE(T >= 0 && T <= 8, "T = %d rounds of re-selection, expected 0 .. 8", T);
    OFC_REQUIRE(T == 0 || thresholds, "null thresholds");
    for (int t = 0; t < T; t++)
        OFC_REQUIRE(std::isfinite(thresholds[t]) && thresholds[t] > 0.0, "threshold %d = %g is not finite and positive", t,
                    thresholds[t]);
    return OFC_OK;
}

int motion_groups(int W, int H, int npair)
{
    return motion_groups_of(motion_nshare(W, H), npair);
}

void motion_launch_geometry(int W, int H, int npair, int out[4])
{
    const int nshare = motion_nshare(W, H), groups = motion_groups_of(nshare, npair), per = motion_per(nshare, groups);
    const int used = (nshare + per - 1) / per;
    out[0] = groups;
    out[1] = per;
    out[2] = used;
    out[3] = nshare - (used - 1) * per;
}

int launch_motion_moments(const float *flow, int W, int H, int npair, const MotionRec *rec, int64_t *partial, bool affine,
                          hipStream_t s)
{
    const dim3 grid(motion_groups(W, H, npair), npair);
    if (affine)
        hipLaunchKernelGGL(k_motion_moments<true>, grid, dim3(MM_THREADS), 0, s, reinterpret_cast<const float2 *>(flow), W, H, rec,
                           reinterpret_cast<long long *>(partial));
    else
        hipLaunchKernelGGL(k_motion_moments<false>, grid, dim3(MM_THREADS), 0, s, reinterpret_cast<const float2 *>(flow), W, H,
                           rec, reinterpret_cast<long long *>(partial));
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_motion_solve(const int64_t *partial, int groups, int npair, int kind, int round, double c_next, MotionRec *rec,
                        double *hist_models, int64_t *hist_moments, hipStream_t s)
{
    hipLaunchKernelGGL(k_motion_solve, dim3(npair), dim3(64), 0, s, reinterpret_cast<const long long *>(partial), groups, npair,
                       kind, round, c_next, rec, hist_models, reinterpret_cast<long long *>(hist_moments));
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int motion_fit_async(const float *flow, int W, int H, int npair, int kind, const double *thresholds, int T, MotionRec *rec,
                     int64_t *partial, double *hist_models, int64_t *hist_moments, hipStream_t s)
{
    OFC_HIP(hipMemsetAsync(rec, 0, sizeof(MotionRec) * npair, s));
    const int groups = motion_groups(W, H, npair);
    for (int t = 0; t <= T; t++) {
        OFC_TRY(launch_motion_moments(flow, W, H, npair, rec, partial, kind == 2, s));
        OFC_TRY(launch_motion_solve(partial, groups, npair, kind, t, t < T ? thresholds[t] : 1.0, rec, hist_models, hist_moments,
                                    s));
    }
    return OFC_OK;
}

int launch_motion_subtract(const float *flow, float *dst, int W, int H, int npair, const MotionRec *rec, hipStream_t s)
{
    const dim3 grid(motion_groups(W, H, npair), npair);
    hipLaunchKernelGGL(k_motion_subtract, grid, dim3(MM_THREADS), 0, s, reinterpret_cast<const float2 *>(flow),
                       reinterpret_cast<float2 *>(dst), W, H, rec);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
