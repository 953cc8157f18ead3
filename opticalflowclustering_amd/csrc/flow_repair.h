// flow_repair.h -- the masked median fill and median smoothing of a flow field (flow_repair.hip, flow_repair_api.cpp,
// stream_api.cpp): limits, the selection network, scratch and launcher.  include/ofc.h has the definition.
#pragma once
#include "ofc_common.h"

namespace ofc {

constexpr int REPAIR_TX = OFC_REPAIR_TILE_W, REPAIR_TY = OFC_REPAIR_TILE_H;   // the tile of a work-group, for both radii
constexpr int REPAIR_MAX_DIM = OFC_CONSIST_MAX_DIM, REPAIR_MAX_PAIRS = 65535, REPAIR_MAX_ROUNDS = OFC_REPAIR_ROUNDS_MAX;
constexpr int REPAIR_NCOUNT = OFC_REPAIR_NCOUNT;
constexpr size_t REPAIR_CHUNK_PIXELS = (size_t)1 << 23;    // a chunk of pairs holds at most this many pixels, or one pair

// A float as an int32 that orders like the number (-0 directly below +0); its own inverse.  Selecting on these keys is exact
// for every bit pattern, denormals included, and never meets a NaN rule.
__host__ __device__ __forceinline__ int repair_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }
constexpr int REPAIR_KEY_LOW = INT32_MIN, REPAIR_KEY_HIGH = INT32_MAX;   // below and above every float's key: absent slots

// Batcher's odd-even merge sort over p[0 .. N-1] as a fixed network (an exchange that would touch an index >= N is left out:
// that index stands for +infinity).  Fully unrolled, so p stays in registers and no index is a runtime value.  A caller that
// reads only p[(N - 1) / 2] pays only for the exchanges that element depends on: the compiler drops the rest.
template <int N> __host__ __device__ __forceinline__ void repair_sort_network(int (&p)[N])
{
    constexpr int T = N <= 16 ? 16 : 32;
    static_assert(N <= T, "at most 32 slots");
#pragma unroll
    for (int s = 1; s < T; s <<= 1) {
#pragma unroll
        for (int k = s; k >= 1; k >>= 1) {
#pragma unroll
            for (int j = k % s; j + k < T; j += 2 * k) {
#pragma unroll
                for (int i = 0; i < k; i++) {
                    const int a = i + j, b = i + j + k;
                    if (b < N && a / (2 * s) == b / (2 * s)) {
                        const int lo = p[a] < p[b] ? p[a] : p[b], hi = p[a] < p[b] ? p[b] : p[a];
                        p[a] = lo, p[b] = hi;
                    }
                }
            }
        }
    }
}

// What a launch works in: two fields of a chunk of pairs for the rounds' snapshots and a `filled` map of the chunk.
struct RepairScratch {
    float *a = nullptr, *b = nullptr;      // f32 [chunk][H][W][2] each
    uint8_t *filled = nullptr;             // u8 [chunk][H][W]
    int chunk = 0;                         // pairs
};
// the pairs a chunk holds for this frame size and npair
int repair_chunk_pairs(int W, int H, int npair);
// bytes of a (or b) and of filled for a chunk of that many pairs
static inline size_t repair_field_bytes(int W, int H, int chunk) { return sizeof(float) * 2 * (size_t)W * H * chunk; }
static inline size_t repair_filled_bytes(int W, int H, int chunk) { return (size_t)W * H * chunk; }

// OFC_OK, OFC_EINVAL or OFC_EUNSUPPORTED (message set): what ofc_repair_check documents.  Host only.
int repair_check(int W, int H, int npair, int keep, int radius, int rounds, int min_count, int smooth);
// clears counts [npair][3], then chunk by chunk: rounds + smooth sweeps, and with state_out the state kernel.  flow
// [npair][H][W][2], state u8 [npair][H][W] or nullptr -> out (may be flow), filled and state_out (each may be nullptr;
// state_out may be state), counts.  Everything is asynchronous on s; sc is free again once s has run it.
int launch_repair(const float *flow, const uint8_t *state, int W, int H, int npair, int keep, int radius, int rounds, int min_count,
                  bool smooth, float *out, uint8_t *filled, uint8_t *state_out, int64_t *counts, const RepairScratch &sc,
                  hipStream_t s);

}  // namespace ofc
