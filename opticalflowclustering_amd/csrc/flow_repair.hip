// flow_repair.hip -- the masked median fill and the median smoothing of a flow field (ofc_repair*; the definition is in
// include/ofc.h).  The reference has no counterpart: it trusted every vector alike (computeOpticalFlowModule.py:20-22).
//
// k_repair_sweep<R, VEC>: one Jacobi round, or the smoothing pass.  grid.y is the pair, a work-group takes a REPAIR_TX x
// REPAIR_TY tile of it.  The tile with a halo of R rows above and below and 2 columns left and right (2 for both radii, so
// that a halo row starts on an even x) is staged once in LDS, two pixels per lane and step: one 16-byte load where W is even
// and the base allows (VEC), two 8-byte loads otherwise.  There is no validity plane: staging turns every component into a
// key (repair_key: an int32 that orders like the float) and gives a pixel without a value -- outside the frame, an invalid
// vector, a state outside `keep` -- the key REPAIR_KEY_LOW for u, which no float has.  A sweep that is not the last writes
// that same mark (+inf) into the u of the snapshot it leaves, so only the first sweep reads `state`, and a later one reads
// 8 bytes per pixel.  A wave takes one row of the tile at a time, four rows in all; where none of its 64 pixels needs a
// median (ballot) it skips the network.  The (2R+1)^2 window is read from LDS with constant offsets into registers; the k-th
// absent slot, by prefix count, becomes REPAIR_KEY_LOW for even k and REPAIR_KEY_HIGH for odd k, so that the lower median of
// the c present keys is the middle element of the sorted slots whatever c is, and the network (flow_repair.h) is fully
// unrolled: no register is indexed by a runtime value.  No address is formed from data, every load and store is predicated
// into the frame, and every loop has a trip count fixed at compile time.  Counts: per lane, up a wave by shuffles, the
// waves meet in LDS, one 64-bit integer atomic per counter and work-group (unfilled goes down by what a round fills: the
// sum wraps to the right value).
// k_repair_state: state_out = OK where filled is a round number, the input state elsewhere; it runs behind the sweeps, when
// nothing reads `state` any more, so state_out may be state.
#include "flow_repair.h"

#include <algorithm>

namespace ofc {

namespace {

constexpr int RP_THREADS = 256, RP_WAVES = RP_THREADS / 64, RP_ROWS = REPAIR_TY / RP_WAVES;
constexpr int RP_HX = 2, RP_LW = REPAIR_TX + 2 * RP_HX, RP_LP = RP_LW / 2;        // halo columns; LDS row in pixels, in pairs
static_assert(REPAIR_TX == 64 && RP_ROWS * RP_WAVES == REPAIR_TY, "a wave takes whole rows of the tile");
constexpr unsigned RP_INF = 0x7f800000u;                                          // the mark in a snapshot's u

typedef unsigned long long u64;

enum : int { RP_FIRST = 1, RP_SMOOTH = 2, RP_LAST = 4 };

__device__ __forceinline__ unsigned rp_wave_add(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// a staged pixel: its two keys, u's being REPAIR_KEY_LOW where the pixel has no value
__device__ __forceinline__ int2 rp_stage(uint2 f, bool inside, int st, int keep)
{
    const float u = __uint_as_float(f.x), v = __uint_as_float(f.y);
    const bool kept = st < OFC_CONSIST_STATES && ((keep >> (st & 3)) & 1);          // a state byte above 3 is in no set
    const bool has = inside && kept && fabsf(u) < 1024.f && fabsf(v) < 1024.f;      // NaN and inf fail
    return make_int2(has ? repair_key((int)f.x) : REPAIR_KEY_LOW, repair_key((int)f.y));
}

template <int R, bool VEC>
__global__ __launch_bounds__(RP_THREADS) void k_repair_sweep(const uint2 *__restrict__ src, const uint8_t *__restrict__ state,
                                                             const uint2 *orig, int W, int H, int tiles_x, int keep, int min_count,
                                                             int round, int flags, uint2 *dst, uint8_t *__restrict__ filled,
                                                             u64 *__restrict__ counts)
{
    constexpr int LR = REPAIR_TY + 2 * R, NPAIRS = LR * RP_LP, STEPS = (NPAIRS + RP_THREADS - 1) / RP_THREADS, N = (2 * R + 1) * (2 * R + 1);
    __shared__ __attribute__((aligned(16))) int2 s_tile[LR][RP_LW];
    __shared__ unsigned s_cnt[RP_WAVES][REPAIR_NCOUNT];
    const int P = W * H;                                               // <= 2^28
    const int t = blockIdx.y;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int x0 = tx * REPAIR_TX, y0 = ty * REPAIR_TY;
    const uint2 *F = src + (size_t)t * P;
    const uint8_t *St = state ? state + (size_t)t * P : nullptr;
    const bool first = flags & RP_FIRST, smooth = flags & RP_SMOOTH, last = flags & RP_LAST;

#pragma unroll
    for (int step = 0; step < STEPS; step++) {
        const int i = step * RP_THREADS + (int)threadIdx.x;
        if (i < NPAIRS) {
            const int row = i / RP_LP, j = i - row * RP_LP;
            const int gy = y0 - R + row, gx = x0 - RP_HX + 2 * j;      // gx is even; it may be -2 and up to W + 65
            const bool iny = gy >= 0 && gy < H, in0 = iny && gx >= 0 && gx < W, in1 = iny && gx + 1 >= 0 && gx + 1 < W;
            const int at = gy * W + gx;                                // used only where in0 or in1 holds: then in [0, P)
            uint2 f0 = make_uint2(0u, 0u), f1 = make_uint2(0u, 0u);
            if (VEC) {                                                 // W is even: in0 == in1
                if (in0) {
                    const uint4 q = *reinterpret_cast<const uint4 *>(F + at);
                    f0 = make_uint2(q.x, q.y), f1 = make_uint2(q.z, q.w);
                }
            } else {
                if (in0) f0 = F[at];
                if (in1) f1 = F[at + 1];
            }
            int st0 = 0, st1 = 0;                                      // without a state map every state is in the set
            int kp = 1;
            if (St) {
                kp = keep;
                if (in0) st0 = St[at];
                if (in1) st1 = St[at + 1];
            }
            const int2 a = rp_stage(f0, in0, st0, kp), b = rp_stage(f1, in1, st1, kp);
            *reinterpret_cast<int4 *>(&s_tile[row][2 * j]) = make_int4(a.x, a.y, b.x, b.y);
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned nsrc = 0, nfill = 0, ntgt = 0;
#pragma unroll
    for (int k = 0; k < RP_ROWS; k++) {
        const int ly = wave + k * RP_WAVES, gy = y0 + ly, gx = x0 + lane;
        const bool inframe = gx < W && gy < H;
        const int2 c = s_tile[ly + R][lane + RP_HX];
        const bool has = c.x != REPAIR_KEY_LOW;                        // a pixel outside the frame has none
        const bool need = inframe && (smooth ? has : !has);
        int mu = 0, mv = 0, cnt = 0;
        if (__ballot(need) != 0ull) {                                  // wave-uniform: the network runs for all 64 lanes or for none
            int ku[N], kv[N];
            int absent = 0;
#pragma unroll
            for (int dy = -R; dy <= R; dy++) {
#pragma unroll
                for (int dx = -R; dx <= R; dx++) {
                    const int n = (dy + R) * (2 * R + 1) + dx + R;
                    const int2 q = s_tile[ly + R + dy][lane + RP_HX + dx];
                    const bool there = q.x != REPAIR_KEY_LOW;
                    const int pad = (absent & 1) ? REPAIR_KEY_HIGH : REPAIR_KEY_LOW;
                    ku[n] = there ? q.x : pad;
                    kv[n] = there ? q.y : pad;
                    absent += there ? 0 : 1;
                }
            }
            cnt = N - absent;
            repair_sort_network<N>(ku);
            repair_sort_network<N>(kv);
            mu = ku[(N - 1) / 2], mv = kv[(N - 1) / 2];
        }
        const bool got = need && (smooth || cnt >= min_count);
        if (inframe) {
            const int p = gy * W + gx;
            uint2 o;
            if (got) o = make_uint2((unsigned)repair_key(mu), (unsigned)repair_key(mv));
            else if (has) o = make_uint2((unsigned)repair_key(c.x), (unsigned)repair_key(c.y));
            else if (last) o = orig[(size_t)t * P + p];                // never filled: the input's own bits
            else o = make_uint2(RP_INF, (unsigned)repair_key(c.y));
            dst[(size_t)t * P + p] = o;
            if (filled) {
                if (got && !smooth) filled[(size_t)t * P + p] = (uint8_t)round;
                else if (first) filled[(size_t)t * P + p] = has ? 0 : OFC_REPAIR_UNFILLED;
            }
            nsrc += has ? 1u : 0u;
            ntgt += has ? 0u : 1u;
            nfill += got && !smooth ? 1u : 0u;
        }
    }

    nsrc = rp_wave_add(nsrc), nfill = rp_wave_add(nfill), ntgt = rp_wave_add(ntgt);
    if (lane == 0) s_cnt[wave][0] = nsrc, s_cnt[wave][1] = nfill, s_cnt[wave][2] = ntgt;
    __syncthreads();
    if (threadIdx.x < REPAIR_NCOUNT) {
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < RP_WAVES; w++) sum += s_cnt[w][threadIdx.x];
        const unsigned fill = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
        // sources and targets are counted by the first sweep only; what a round fills leaves the unfilled
        u64 add = threadIdx.x == 1 ? (u64)sum : first ? (u64)sum : 0ull;
        if (threadIdx.x == 2) add -= (u64)fill;
        if (add) atomicAdd(counts + (size_t)t * REPAIR_NCOUNT + threadIdx.x, add);
    }
}
static_assert(RP_WAVES == 4, "the counts' meeting adds four waves");

// state_out = OK where a round filled the pixel, the input state elsewhere: four pixels per lane where both maps and the
// output are 4-byte aligned, single bytes otherwise and for the tail
__global__ __launch_bounds__(RP_THREADS) void k_repair_state(const uint8_t *state, const uint8_t *__restrict__ filled, int64_t n,
                                                             bool vec, uint8_t *state_out)
{
    const int64_t i = ((int64_t)blockIdx.x * RP_THREADS + threadIdx.x) * 4;
    if (i >= n) return;
    if (vec && i + 4 <= n) {
        const unsigned s = *reinterpret_cast<const uint32_t *>(state + i), f = *reinterpret_cast<const uint32_t *>(filled + i);
        unsigned o = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned fb = (f >> (8 * q)) & 255u, sb = (s >> (8 * q)) & 255u;
            o |= (fb >= 1u && fb < (unsigned)OFC_REPAIR_UNFILLED ? (unsigned)OFC_CONSIST_OK : sb) << (8 * q);
        }
        *reinterpret_cast<uint32_t *>(state_out + i) = o;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (i + q < n) {
                const unsigned fb = filled[i + q], sb = state[i + q];
                state_out[i + q] = (uint8_t)(fb >= 1u && fb < (unsigned)OFC_REPAIR_UNFILLED ? (unsigned)OFC_CONSIST_OK : sb);
            }
        }
    }
}

}  // namespace

int repair_check(int W, int H, int npair, int keep, int radius, int rounds, int min_count, int smooth)
{
    OFC_REQUIRE(W >= 1 && H >= 1, "W = %d, H = %d: at least 1", W, H);
    OFC_REQUIRE(npair >= 1 && npair <= REPAIR_MAX_PAIRS, "npair = %d: 1 .. %d", npair, REPAIR_MAX_PAIRS);
    OFC_REQUIRE(keep >= 1 && keep < (1 << OFC_CONSIST_STATES), "keep = %d: a set of the four states, 1 .. 15", keep);
    OFC_REQUIRE(radius == 1 || radius == 2, "radius = %d: 1 (3x3) or 2 (5x5)", radius);
    OFC_REQUIRE(rounds >= 0 && rounds <= REPAIR_MAX_ROUNDS, "rounds = %d: 0 .. %d", rounds, REPAIR_MAX_ROUNDS);
    OFC_REQUIRE(min_count >= 1 && min_count <= (2 * radius + 1) * (2 * radius + 1), "min_count = %d: 1 .. %d at radius %d", min_count,
                (2 * radius + 1) * (2 * radius + 1), radius);
    OFC_REQUIRE(smooth == 0 || smooth == 1, "smooth = %d: 0 or 1", smooth);
    OFC_REQUIRE(rounds > 0 || smooth == 1, "rounds = 0 without smooth: nothing to do");
    if (W > REPAIR_MAX_DIM || H > REPAIR_MAX_DIM) {
        set_error("W = %d, H = %d: at most %d each", W, H, REPAIR_MAX_DIM);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

int repair_chunk_pairs(int W, int H, int npair)
{
    const size_t P = (size_t)W * H;
    return (int)std::min<size_t>((size_t)npair, std::max<size_t>(1, REPAIR_CHUNK_PIXELS / P));
}

int launch_repair(const float *flow, const uint8_t *state, int W, int H, int npair, int keep, int radius, int rounds, int min_count,
                  bool smooth, float *out, uint8_t *filled, uint8_t *state_out, int64_t *counts, const RepairScratch &sc,
                  hipStream_t s)
{
    const size_t P = (size_t)W * H;
    const int tiles_x = cdiv(W, REPAIR_TX), tiles = tiles_x * cdiv(H, REPAIR_TY);     // at most 256 * 1024
    const int sweeps = rounds + (smooth ? 1 : 0);
    OFC_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * REPAIR_NCOUNT * (size_t)npair, s));
    for (int t0 = 0; t0 < npair; t0 += sc.chunk) {
        const int n = std::min(sc.chunk, npair - t0);
        const uint2 *in = reinterpret_cast<const uint2 *>(flow) + t0 * P;
        uint2 *res = reinterpret_cast<uint2 *>(out) + t0 * P;
        // the map the state kernel reads: the caller's, or the scratch's when the caller wants none
        uint8_t *fil = filled ? filled + t0 * P : state_out ? sc.filled : nullptr;
        const uint2 *from = in;
        for (int g = 1; g <= sweeps; g++) {
            const bool last = g == sweeps, sm = smooth && last;
            // a single sweep in place would read neighbours that other work-groups are overwriting: it goes through a
            uint2 *to = !last ? reinterpret_cast<uint2 *>(g & 1 ? sc.a : sc.b) : sweeps == 1 && res == in ? reinterpret_cast<uint2 *>(sc.a) : res;
            const int flags = (g == 1 ? RP_FIRST : 0) | (sm ? RP_SMOOTH : 0) | (last ? RP_LAST : 0);
            // 16-byte loads: every row of every pair of the sweep's source starts on a multiple of 16 bytes
            const bool vec = ((uintptr_t)from & 15) == 0 && W % 2 == 0;
            auto kern = radius == 1 ? (vec ? &k_repair_sweep<1, true> : &k_repair_sweep<1, false>)
                                    : (vec ? &k_repair_sweep<2, true> : &k_repair_sweep<2, false>);
            hipLaunchKernelGGL(kern, dim3((unsigned)tiles, n), dim3(RP_THREADS), 0, s, from, g == 1 && state ? state + t0 * P : nullptr, in,
                               W, H, tiles_x, keep, min_count, g, flags, to, fil, reinterpret_cast<u64 *>(counts) + (size_t)t0 * REPAIR_NCOUNT);
            OFC_HIP(hipGetLastError());
            if (last && to != res) OFC_HIP(hipMemcpyAsync(res, to, sizeof(uint2) * P * n, hipMemcpyDeviceToDevice, s));
            from = to;
        }
        if (state_out) {
            const int64_t cnt = (int64_t)(P * n);
            const uint8_t *si = state + t0 * P;
            uint8_t *so = state_out + t0 * P;
            const bool vec = (((uintptr_t)si | (uintptr_t)so | (uintptr_t)fil) & 3) == 0;
            hipLaunchKernelGGL(k_repair_state, dim3((unsigned)cdiv64(cnt, 4 * RP_THREADS)), dim3(RP_THREADS), 0, s, si, fil, cnt, vec, so);
            OFC_HIP(hipGetLastError());
        }
    }
    return OFC_OK;
}

}  // namespace ofc
