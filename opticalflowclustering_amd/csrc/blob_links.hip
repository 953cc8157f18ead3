// blob_links.hip -- which blob of pair t continues as which blob of pair t+1 (ofc_blob_link*, ofc_blob_moves_dev; the
// definition is in include/ofc.h).  The reference has no counterpart: it read boxes per frame from files
// (KmeanGrids.py:16-50) and never related one frame's to the next's.
//
// k_blob_moves: the field's vectors, rounded to whole pixels, as one int32 per pixel.  A separate object because the blobs
// are usually keyed on the residual after camera removal while a pixel lands in the next frame by the whole flow.
// k_blob_links: a work-group takes BLOB_SHARE consecutive pixels of a source pair; grid.y is the transition.  A pixel reads
// its label and move (coalesced), the label where it lands (a gather, near-coalesced: neighbours move alike) and the two
// areas at the roots (few distinct addresses).  Every index taken from a caller's buffer is checked before it indexes
// anything.  A vote is the 64-bit key (a << 32) | b.  Votes combine before they touch memory, as in blobs.hip's k_blob_accum:
// a lane keeps a private run while its key repeats, the lanes of a wave that share a key fold by ballot and shuffles, the
// waves of a work-group meet in an LDS table keyed by the pair (a few probes, then straight to memory), flushed once.
// The transition's table in global memory is open addressing on the key: a slot is claimed by a 64-bit compare-and-swap,
// the votes are added by an integer atomic; every successful claim of an empty slot draws a ticket from the transition's
// counter, so the counter counts distinct links and "more than max_links" is exact whatever the order.  Once the counter is
// past max_links nothing more is inserted: the transition delivers no row.  Every probe loop is capped at the capacity.
#include "blob_links.h"

namespace ofc {

namespace {

constexpr int LK_THREADS = 256, LK_WAVES = LK_THREADS / 64, LK_UNROLL = BLOB_SHARE / LK_THREADS;
constexpr int LK_SLOTS = 256, LK_PROBES = 4;
static_assert(LK_UNROLL * LK_THREADS == BLOB_SHARE, "shares divide evenly");

typedef unsigned long long u64;
constexpr u64 LK_EMPTY = BLOB_LINK_EMPTY;
constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;

__device__ __forceinline__ int lk_move(float u, float v)
{
    const bool valid = fabsf(u) < 1024.f && fabsf(v) < 1024.f;         // NaN and inf fail
    const unsigned dx = (unsigned)__float2int_rn(u) & 0xffffu, dy = (unsigned)__float2int_rn(v) & 0xffffu;
    return valid ? (int)((dy << 16) | dx) : BLOB_NO_MOVE;
}

// VEC (flow and moves 16-byte aligned): a lane takes four consecutive vectors as two 16-byte loads and stores their moves
// as one; the last n % 4 vectors, and everything without VEC, go one vector per lane.
template <bool VEC>
__global__ __launch_bounds__(LK_THREADS) void k_blob_moves(const float2 *__restrict__ flow, long long n, int32_t *__restrict__ moves)
{
    const long long stride = (long long)gridDim.x * LK_THREADS, t0 = (long long)blockIdx.x * LK_THREADS + threadIdx.x;
    const long long n4 = VEC ? n / 4 : 0;
    for (long long q = t0; q < n4; q += stride) {
        const float4 a = *reinterpret_cast<const float4 *>(flow + 4 * q), b = *reinterpret_cast<const float4 *>(flow + 4 * q + 2);
        *reinterpret_cast<int4 *>(moves + 4 * q) = make_int4(lk_move(a.x, a.y), lk_move(a.z, a.w), lk_move(b.x, b.y), lk_move(b.z, b.w));
    }
    for (long long i = 4 * n4 + t0; i < n; i += stride) {
        const float2 f = flow[i];
        moves[i] = lk_move(f.x, f.y);
    }
}

__device__ __forceinline__ unsigned lk_hash(u64 key) { return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32); }

// the slot of `key` in the work-group's LDS table, or -1 after LK_PROBES slots owned by others
__device__ __forceinline__ int lk_slot(u64 *s_key, u64 key)
{
    int slot = (int)(lk_hash(key) >> 8) & (LK_SLOTS - 1);
    for (int probe = 0; probe < LK_PROBES; probe++, slot = (slot + 1) & (LK_SLOTS - 1)) {
        const u64 old = atomicCAS(&s_key[slot], LK_EMPTY, key);
        if (old == LK_EMPTY || old == key) return slot;
    }
    return -1;
}

// `votes` for `key` into the transition's table.  cap is a power of two; the loop ends after cap slots at the latest.
__device__ __forceinline__ void lk_insert(u64 *keys, int32_t *votes, unsigned cap, int max_links, int32_t *counter, u64 key, int n)
{
    // overflowed already: the transition delivers no row, and a table that may be full is not searched
    if ((__hip_atomic_load(counter, __ATOMIC_RELAXED, AG) & BLOB_LINK_COUNT) > max_links) return;
    unsigned slot = lk_hash(key) & (cap - 1);
    for (unsigned probe = 0; probe < cap; probe++, slot = (slot + 1) & (cap - 1)) {
        u64 old = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, AG);
        if (old == LK_EMPTY) {
            old = atomicCAS(keys + slot, LK_EMPTY, key);
            if (old == LK_EMPTY) {
                atomicAdd(counter, 1);                         // the ticket: past max_links it marks the overflow by itself
                old = key;
            }
        }
        if (old == key) {
            atomicAdd(votes + slot, n);
            return;
        }
    }
    atomicOr(counter, BLOB_LINK_FULL);                         // every slot holds another key
}

template <class T> __device__ __forceinline__ T lk_wave_add(T v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(LK_THREADS) void k_blob_links(const int32_t *__restrict__ labels_a, const int32_t *__restrict__ moves,
                                                           const int32_t *__restrict__ areas_a, const int32_t *__restrict__ labels_b,
                                                           const int32_t *__restrict__ areas_b, int W, int H, int min_area,
                                                           int max_links, unsigned cap, u64 *keys, int32_t *votes, int32_t *counters)
{
    __shared__ u64 s_key[LK_SLOTS];
    __shared__ int s_cnt[LK_SLOTS];
    for (int s = threadIdx.x; s < LK_SLOTS; s += LK_THREADS) { s_key[s] = LK_EMPTY; s_cnt[s] = 0; }
    __syncthreads();
    const int P = W * H;
    const size_t base = (size_t)blockIdx.y * (size_t)P;
    const int32_t *La = labels_a + base, *Mv = moves + base, *Aa = areas_a + base, *Lb = labels_b + base, *Ab = areas_b + base;
    u64 *K = keys + (size_t)blockIdx.y * cap;
    int32_t *V = votes + (size_t)blockIdx.y * cap, *counter = counters + blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * BLOB_SHARE + wave * (BLOB_SHARE / LK_WAVES) + lane;

    u64 key[LK_UNROLL];
#pragma unroll
    for (int q = 0; q < LK_UNROLL; q++) {
        const long long i = i0 + q * 64;
        key[q] = LK_EMPTY;
        if (i >= P) continue;
        const int a = La[i], mv = Mv[i];
        if (a < 0 || a >= P || mv == BLOB_NO_MOVE) continue;   // labels are the caller's: checked before they index
        if (Aa[a] < min_area) continue;
        const int dx = (int)(short)(mv & 0xffff), dy = (int)(short)((unsigned)mv >> 16);
        const int y = (int)i / W, x = (int)i - y * W;          // i < P <= 2^31 - 1
        const int xt = x + dx, yt = y + dy;                    // |dx|, |dy| <= 2^15: no overflow
        if (xt < 0 || xt >= W || yt < 0 || yt >= H) continue;
        const int b = Lb[(size_t)yt * W + xt];
        if (b < 0 || b >= P) continue;
        if (Ab[b] < min_area) continue;
        key[q] = ((u64)(unsigned)a << 32) | (unsigned)b;
    }

    auto combine = [&](bool go, u64 k, int cnt) {              // called by all 64 lanes
        u64 todo = __ballot(go);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned hi = __builtin_amdgcn_readlane((unsigned)(k >> 32), leader);
            const unsigned lo = __builtin_amdgcn_readlane((unsigned)k, leader);
            const u64 kl = ((u64)hi << 32) | lo;
            const bool mine = go && k == kl;
            const int total = lk_wave_add(mine ? cnt : 0);
            if (lane == leader) {
                const int slot = lk_slot(s_key, kl);
                if (slot >= 0) atomicAdd(&s_cnt[slot], total);
                else lk_insert(K, V, cap, max_links, counter, kl, total);
            }
            todo &= ~__ballot(mine);
        }
    };
    u64 pk = LK_EMPTY;                                         // the lane's run
    int pc = 0;
#pragma unroll
    for (int q = 0; q < LK_UNROLL; q++) {
        const bool ended = pk != LK_EMPTY && key[q] != LK_EMPTY && key[q] != pk;       // a pixel without a vote ends no run
        if (__ballot(ended)) combine(ended, pk, pc);
        if (ended) pc = 0;
        if (key[q] != LK_EMPTY) { pk = key[q]; pc++; }
    }
    combine(pk != LK_EMPTY, pk, pc);
    __syncthreads();
    for (int s = threadIdx.x; s < LK_SLOTS; s += LK_THREADS)
        if (s_key[s] != LK_EMPTY) lk_insert(K, V, cap, max_links, counter, s_key[s], s_cnt[s]);
}

}  // namespace

int blob_link_check(int W, int H, int npair, int min_area, int max_links)
{
    OFC_TRY(blob_check(W, H, npair, 8, min_area, 1));
    OFC_REQUIRE(max_links >= 1, "max_links = %d: at least 1", max_links);
    if (max_links > BLOB_MAX_LINKS) {
        set_error("max_links = %d: at most %d", max_links, BLOB_MAX_LINKS);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

int launch_blob_moves(const float *flow, int W, int H, int npair, int32_t *moves, hipStream_t s)
{
    const long long n = (long long)W * H * npair;
    const bool vec = ((uintptr_t)flow & 15) == 0 && ((uintptr_t)moves & 15) == 0;
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(vec ? cdiv64(n, 4) : n, LK_THREADS), 8192));
    auto kern = vec ? &k_blob_moves<true> : &k_blob_moves<false>;
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(LK_THREADS), 0, s, reinterpret_cast<const float2 *>(flow), n, moves);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_blob_links_clear(int max_links, int ntrans, uint64_t *keys, int32_t *votes, int32_t *counters, hipStream_t s)
{
    if (ntrans == 0) return OFC_OK;
    const size_t slots = blob_link_capacity(max_links) * (size_t)ntrans;
    OFC_HIP(hipMemsetAsync(keys, 0xff, slots * sizeof(uint64_t), s));
    OFC_HIP(hipMemsetAsync(votes, 0, slots * sizeof(int32_t), s));
    OFC_HIP(hipMemsetAsync(counters, 0, sizeof(int32_t) * ntrans, s));
    return OFC_OK;
}

int launch_blob_links(const int32_t *labels_a, const int32_t *moves, const int32_t *areas_a, const int32_t *labels_b,
                      const int32_t *areas_b, int W, int H, int ntrans, int min_area, int max_links, uint64_t *keys,
                      int32_t *votes, int32_t *counters, hipStream_t s)
{
    if (ntrans == 0) return OFC_OK;
    const int P = W * H;
    hipLaunchKernelGGL(k_blob_links, dim3((unsigned)cdiv64(P, BLOB_SHARE), ntrans), dim3(LK_THREADS), 0, s, labels_a, moves, areas_a,
                       labels_b, areas_b, W, H, min_area, max_links, (unsigned)blob_link_capacity(max_links),
                       reinterpret_cast<u64 *>(keys), votes, counters);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
