// uv_hist.hip -- a 2-D histogram of flow vectors: per bin of the (u,v) plane an exact count and exact fixed-point sums
// of its members (ofc_uv_hist_accum_dev, the streaming ingest's per-batch pass).  A weighted Lloyd fit over the bin means
// then stands in for the fit over the field (uvhist.py), and tables of batches, clips or ranks merge by addition.
//
// Definition (include/ofc.h repeats it): bins = B, range = R, both powers of two; tu = (u + R) * (B / 2R) with the sum
// rounded to f32 and the product exact; in range iff 0 <= tu < B and 0 <= tv < B (so NaN, +-inf, u = R and a u whose
// u + R rounds up to 2R are outside); bin = floor(tv) * B + floor(tu).  In range: count += 1,
// sum_u += llrint((double)u * 65536), sum_v likewise; otherwise outside += 1.  Table: count[B*B], sum_u[B*B], sum_v[B*B],
// outside, all int64, added to what is there.  Integers only: whatever the order of the adds, equal bits.
//
// Shape.  A work-group of four waves takes shares of UH_SHARE consecutive vectors.  The grid is ceil(n / UH_SHARE), at most
// UH_MAX_GRID; above that a work-group takes ceil(shares / grid) CONSECUTIVE shares, a band of one frame for a clip, so
// that the bins it meets are those of one place and time.  Each wave owns 512 consecutive vectors of the share and reads
// them as eight loads of 64 consecutive vectors (512 B per load, all eight in flight): a lane's eight vectors are 64 apart.
//
// Contention is taken out in three steps before the table is touched:
//   1. per lane, a run: while a lane's next vector falls into the bin of its previous one it is added to the lane's pending
//      (bin, count, sum_u, sum_v) in registers.
//   2. per wave, a leader/ballot loop over the lanes whose run has ended (all of them at the end of the share): the first
//      such lane broadcasts its bin, the lanes that hold the same bin answer in a ballot, their pending values are folded
//      across the wave and land in the leader.  One round per DISTINCT bin among those lanes.  A bin held by fewer than
//      UH_FOLD_MIN lanes is not folded: those lanes go to step 3 on their own.  At 2 that is the lane alone; at 8, where
//      up to seven adds meet on one LDS address, the loop got 0.4 ms cheaper and step 3 1 - 2 ms dearer.
//      The fold is int32 (4 DPP row rotations, then xor-16 and xor-32 exchanges): a pending sum is at most 8 * 2^16 R, so
//      for R <= 32 the wave's total stays within 2^30; above that (WIDE) the value is folded as two limbs of 14 low and
//      16 high bits.
//   3. the leaders add their bin's totals to a cache of UH_SLOTS bins in LDS (ds atomics; the leaders of one loop hold
//      distinct bins, so their adds do not pile up).  The slot of bin (iu, iv) is (iv % 32) * 32 + iu % 32: a 32 x 32
//      patch of the plane maps one to one, so a compact motion cluster never collides with itself.  The first bin to
//      arrive owns the slot (compare-and-swap on its key); a leader that finds the slot owned by another bin tries the
//      next one, and after UH_PROBES of them adds to the table directly.  The cache is written to the table once, when the
//      work-group has walked all its shares: a hot bin (the still background) costs one set of three adds per work-group,
//      not per wave and load.
// Every add to the table is a no-return 64-bit integer atomic at agent scope.
#include "color_common.h"

#include <algorithm>

namespace ofc {

namespace {

constexpr int UH_THREADS = 256, UH_WAVES = UH_THREADS / 64, UH_SLOTS = 1024, UH_PROBES = 4, UH_FOLD_MIN = 2;
constexpr int UH_UNROLL = OFC_UV_HIST_SHARE / UH_THREADS;         // loads per lane and share
static_assert(UH_UNROLL == 8 && UH_UNROLL * UH_THREADS == OFC_UV_HIST_SHARE, "the int32 folds are sized for runs of 8");

typedef unsigned long long u64;

template <int N> __device__ __forceinline__ int uh_ror(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, 0x120 + N, 0xf, 0xf, false);
}
// sum over the wave's 64 lanes of an int32 whose total fits int32.  Called by all 64 lanes; every lane ends with the total.
__device__ __forceinline__ int uh_fold(int v)
{
    v += uh_ror<8>(v); v += uh_ror<4>(v); v += uh_ror<2>(v); v += uh_ror<1>(v);
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}
// sum over the wave of a pending fixed-point sum, |v| <= 2^19 R per lane
template <bool WIDE> __device__ __forceinline__ long long uh_wave_sum(int v)
{
    if (!WIDE) return (long long)uh_fold(v);                                   // R <= 32: |total| <= 2^30
    const int lo = uh_fold(v & 0x3fff), hi = uh_fold(v >> 14);                 // 64 * 2^14 and 64 * 2^15
    return (long long)hi * 16384 + (long long)lo;
}

__device__ __forceinline__ void uh_table_add(u64 *p, u64 v)
{
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct UhCache {
    int key[UH_SLOTS];
    u64 cnt[UH_SLOTS], u[UH_SLOTS], v[UH_SLOTS];
};

// Steps 2 and 3 for the lanes with go set (their bin >= 0): called by all 64 lanes of a wave
template <bool WIDE>
__device__ __forceinline__ void uh_combine(bool go, int bin, int pcnt, int psu, int psv, int lane, int logB, UhCache &c,
                                           u64 *__restrict__ table)
{
    u64 todo = __ballot(go);
    bool lead = false;                                     // this lane carries (cnt, su, sv) of `bin` to the cache
    u64 cnt = 0, su = 0, sv = 0;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int key = __builtin_amdgcn_readlane(bin, leader);
        const bool mine = go && bin == key;
        const u64 m = __ballot(mine);
        const int members = __popcll(m);
        if (members < UH_FOLD_MIN) {                       // too few lanes to be worth a fold: each carries its own
            if (mine) { lead = true; cnt = (u64)pcnt; su = (u64)(long long)psu; sv = (u64)(long long)psv; }
        } else {
            const int tc = uh_fold(mine ? pcnt : 0);                           // <= 64 * 8
            const long long tsu = uh_wave_sum<WIDE>(mine ? psu : 0), tsv = uh_wave_sum<WIDE>(mine ? psv : 0);
            if (lane == leader) { lead = true; cnt = (u64)tc; su = (u64)tsu; sv = (u64)tsv; }
        }
        todo &= ~m;
    }
    if (lead) {
        const int B = 1 << logB;
        const size_t B2 = (size_t)B * B;
        const int iu = bin & (B - 1), iv = bin >> logB;
        int slot = ((iv & 31) << 5) | (iu & 31);
        bool cached = false;
        for (int probe = 0; probe < UH_PROBES && !cached; probe++, slot = (slot + 1) & (UH_SLOTS - 1)) {
            const int old = atomicCAS(&c.key[slot], -1, bin);
            if (old == -1 || old == bin) {
                atomicAdd(&c.cnt[slot], cnt);
                atomicAdd(&c.u[slot], su);
                atomicAdd(&c.v[slot], sv);
                cached = true;
            }
        }
        if (!cached) {                                     // UH_PROBES slots in a row belong to other bins: straight to the table
            uh_table_add(table + bin, cnt);
            uh_table_add(table + B2 + bin, su);
            uh_table_add(table + 2 * B2 + bin, sv);
        }
    }
}

// flow [n][2] f32 -> table (see the head of this file).  B = 1 << logB, scale = B / 2R.  WIDE: R > 32.
template <bool WIDE>
__global__ __launch_bounds__(UH_THREADS) void k_uv_hist(const float2 *__restrict__ flow, int64_t n, int logB, float R,
                                                        float scale, u64 *__restrict__ table)
{
    __shared__ UhCache s_c;
    __shared__ u64 s_outside;
    for (int s = threadIdx.x; s < UH_SLOTS; s += UH_THREADS) { s_c.key[s] = -1; s_c.cnt[s] = 0; s_c.u[s] = 0; s_c.v[s] = 0; }
    if (threadIdx.x == 0) s_outside = 0;
    __syncthreads();

    const int B = 1 << logB;
    const float Bf = (float)B;
    const size_t B2 = (size_t)B * B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned outside = 0;                                  // wave-uniform: this wave's vectors outside the range
    const int64_t nshare = (n + OFC_UV_HIST_SHARE - 1) / OFC_UV_HIST_SHARE, per = (nshare + gridDim.x - 1) / gridDim.x;
    const int64_t g1 = std::min<int64_t>(nshare, (blockIdx.x + 1) * per);
    for (int64_t g = blockIdx.x * per; g < g1; g++) {
        const int64_t i0 = g * OFC_UV_HIST_SHARE + wave * (OFC_UV_HIST_SHARE / UH_WAVES) + lane;
        float2 f[UH_UNROLL];
#pragma unroll
        for (int q = 0; q < UH_UNROLL; q++) {
            const int64_t i = i0 + q * 64;
            f[q] = i < n ? flow[i] : make_float2(0.f, 0.f);
        }
        int pbin = -1, pcnt = 0, psu = 0, psv = 0;         // the lane's run: <= 8 vectors, |sum| <= 8 * 2^16 R
#pragma unroll
        for (int q = 0; q < UH_UNROLL; q++) {
            const bool have = i0 + q * 64 < n;
            const float tu = __fadd_rn(f[q].x, R) * scale, tv = __fadd_rn(f[q].y, R) * scale;
            const bool in = have && tu >= 0.f && tu < Bf && tv >= 0.f && tv < Bf;       // NaN fails every compare
            const int bin = in ? (((int)floorf(tv)) << logB) + (int)floorf(tu) : -1;
            // in range |u| <= R <= 2^10: the fixed-point value is an integer of magnitude <= 2^26, exact in f64
            const int qu = in ? __double2int_rn((double)f[q].x * 65536.0) : 0;
            const int qv = in ? __double2int_rn((double)f[q].y * 65536.0) : 0;
            outside += (unsigned)__popcll(__ballot(have && !in));
            const bool ended = pbin >= 0 && in && bin != pbin;                           // a vector outside ends no run
            if (__ballot(ended)) uh_combine<WIDE>(ended, pbin, pcnt, psu, psv, lane, logB, s_c, table);
            if (ended) { pcnt = 0; psu = 0; psv = 0; }
            if (in) { pbin = bin; pcnt += 1; psu += qu; psv += qv; }
        }
        uh_combine<WIDE>(pbin >= 0, pbin, pcnt, psu, psv, lane, logB, s_c, table);
    }
    if (lane == 0 && outside) atomicAdd(&s_outside, (u64)outside);
    __syncthreads();
    for (int s = threadIdx.x; s < UH_SLOTS; s += UH_THREADS) {
        const int bin = s_c.key[s];
        if (bin >= 0) {                                    // bin < B*B: it was formed from 0 <= floor(t) < B on both axes
            uh_table_add(table + bin, s_c.cnt[s]);
            uh_table_add(table + B2 + bin, s_c.u[s]);
            uh_table_add(table + 2 * B2 + bin, s_c.v[s]);
        }
    }
    if (threadIdx.x == 0 && s_outside) uh_table_add(table + 3 * B2, s_outside);
}

}  // namespace

int uv_hist_check(int bins, float range)
{
    OFC_REQUIRE(bins >= 16 && bins <= 2048 && (bins & (bins - 1)) == 0, "bins = %d is not a power of two in 16 .. 2048", bins);
    int e = 0;
    const bool pow2 = range > 0.f && range <= 1024.f && frexpf(range, &e) == 0.5f;       // NaN fails the first compare
    OFC_REQUIRE(pow2 && range >= 0.0625f, "range = %g is not a power of two in 2^-4 .. 2^10", (double)range);
    return OFC_OK;
}

// flow [n][2] f32 (8-byte aligned), n >= 1; table 3*bins*bins + 1 int64, added to.  The caller has checked bins and range
// (uv_hist_check).  Asynchronous on s.
int launch_uv_hist(const float *flow, int64_t n, int bins, float range, int64_t *table, hipStream_t s)
{
    int logB = 0;
    while ((1 << logB) < bins) logB++;
    const int64_t nshare = (n + OFC_UV_HIST_SHARE - 1) / OFC_UV_HIST_SHARE;
    const int grid = (int)std::min<int64_t>(nshare, OFC_UV_HIST_MAX_GRID);
    const float scale = (float)bins / (2.f * range);
    if (range > 32.f)
        hipLaunchKernelGGL(k_uv_hist<true>, dim3(grid), dim3(UH_THREADS), 0, s, reinterpret_cast<const float2 *>(flow), n, logB,
                           range, scale, reinterpret_cast<u64 *>(table));
    else
        hipLaunchKernelGGL(k_uv_hist<false>, dim3(grid), dim3(UH_THREADS), 0, s, reinterpret_cast<const float2 *>(flow), n, logB,
                           range, scale, reinterpret_cast<u64 *>(table));
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
