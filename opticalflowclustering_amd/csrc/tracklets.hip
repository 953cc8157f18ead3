// tracklets.hip -- dense trajectories with reseeding (ofc_tracklets*; the definition is in include/ofc.h).  The reference has
// no counterpart: it followed no point.
//
// A frame costs three launches, and the host reads nothing back between them:
//   k_trk_count   one lane per grid cell: is the cell free (its bit of the occupancy bitmap clear) and, with a state map, may its
//                 seed stand there?  A ballot per wave gives the empty cells of 64 (kept for the next kernel) and their
//                 popcount; a work-group leaves its two counts (empty, blocked) in one 8-byte word and draws a ticket.  The
//                 work-group that draws the last ticket -- nobody waits for it, or for anyone -- turns the counts into the
//                 exclusive prefix sum over the work-groups, and decides the frame: born = min(empty, M - used), first[t] =
//                 used, used += born, the row of `frames`.
//   k_trk_assign  one lane per grid cell again: the rank of an empty cell is its work-group's prefix, the popcounts of the waves
//                 before it and the bits below it in its wave's ballot; the cells of rank < born seed the ids first[t] + rank.
//                 It also clears the bitmap, which nobody reads in this launch.
//   k_trk_step    one lane per id of the window first[max(0, t-L+1)] .. used, both read on the device; the grid is sized by
//                 the host's bound min(M, cells * min(L, t+1)) and surplus lanes leave at once.  A live track takes the step of
//                 traj_step.h from pos[len][id] to pos[len+1][id] (ids born together are neighbours: the stores coalesce) and,
//                 if it is still live afterwards, sets its cell's bit for the next frame's count with an atomic OR.
// The count and the scan cannot share a launch with the assignment without a work-group waiting for another, and the step
// needs the ids of the newborn, so three it is.  Bit OR and integer sums do not depend on the order of the work; ranks are
// exact, so every output is the same bits however the device schedules it.
// The hand-off inside k_trk_count: the 8-byte count is an agent-scope atomic store, drained before the same lane's ticket
// add; the last work-group reads the counts with agent-scope atomic loads only, and resets the ticket for the next frame.
// Safety: a cell index is clamped to cells-1 and an id to M-1 before they index anything, a step count to L-1; positions are
// clamped by traj_step; every loop's trip count comes from the launch arguments.
#include "tracklets.h"
#include "traj_step.h"

namespace ofc {

namespace {

typedef unsigned long long u64;
constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
constexpr int WAVES = TRK_THREADS / 64;

// the seed of cell cc: its centre, clamped into the frame (cc < cells: cx * cell < W <= 16384, so everything stays below 2^31)
__device__ __forceinline__ int2 trk_seed(int cc, int cols, int cell, int W, int H)
{
    const int cx = cc % cols, cy = cc / cols;
    return make_int2(min(((cx * cell) << 16) + (cell << 15), (W - 1) << 16), min(((cy * cell) << 16) + (cell << 15), (H - 1) << 16));
}

template <bool STATE>
__global__ __launch_bounds__(TRK_THREADS) void k_trk_count(const unsigned *__restrict__ bitmap, const uint8_t *__restrict__ state, int W,
                                                           int H, int cell, int cols, int cells, unsigned keep, int t, int M, int groups,
                                                           u64 *__restrict__ mask, u64 *partial, unsigned *__restrict__ offs,
                                                           unsigned *ctl, int *__restrict__ first, int *__restrict__ frames)
{
    __shared__ unsigned sh_e[WAVES], sh_b[WAVES], sh_last;
    __shared__ u64 sh_scan[TRK_THREADS];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = (int)blockIdx.x * TRK_THREADS + tid;                 // below 2^24 + 256
    const int cc = min(c, cells - 1);
    const bool is_free = c < cells && !((bitmap[cc >> 5] >> (cc & 31)) & 1u);
    bool ok = true;
    if (STATE) {
        const int2 sd = trk_seed(cc, cols, cell, W, H);
        const int rx = min((sd.x + 32768) >> 16, W - 1), ry = min((sd.y + 32768) >> 16, H - 1);
        const unsigned sb = state[(size_t)ry * W + rx];
        ok = sb < 4u && ((keep >> sb) & 1u);
    }
    const u64 e = __ballot(is_free && ok), b = __ballot(is_free && !ok);
    if (lane == 0) {
        mask[(size_t)blockIdx.x * WAVES + wave] = e;
        sh_e[wave] = (unsigned)__popcll(e);
        sh_b[wave] = (unsigned)__popcll(b);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned E = 0, B = 0;
        for (int w = 0; w < WAVES; w++) E += sh_e[w], B += sh_b[w];
        __hip_atomic_store(partial + blockIdx.x, ((u64)B << 32) | E, __ATOMIC_RELAXED, AG);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the count has left before the ticket is drawn
        sh_last = __hip_atomic_fetch_add(ctl, 1u, __ATOMIC_RELAXED, AG) == (unsigned)(groups - 1);
    }
    __syncthreads();
    if (!sh_last) return;

    // the last work-group to arrive: every count is out.  Lane i takes the work-groups i * chunk .. of the scan.
    const int chunk = (groups + TRK_THREADS - 1) / TRK_THREADS;
    const int i0 = min(tid * chunk, groups), i1 = min(i0 + chunk, groups);
    u64 mine = 0;                                                      // blocked << 32 | empty: each at most 2^24, no carry
    for (int i = i0; i < i1; i++) mine += __hip_atomic_load(partial + i, __ATOMIC_RELAXED, AG);
    sh_scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < TRK_THREADS; d <<= 1) {
        const u64 a = tid >= d ? sh_scan[tid - d] : 0;
        __syncthreads();
        sh_scan[tid] += a;
        __syncthreads();
    }
    unsigned run = (unsigned)(sh_scan[tid] - mine);                    // the empty cells before work-group i0
    for (int i = i0; i < i1; i++) {
        offs[i] = run;
        run += (unsigned)__hip_atomic_load(partial + i, __ATOMIC_RELAXED, AG);
    }
    if (tid == TRK_THREADS - 1) {
        const u64 total = sh_scan[tid];
        const int E = (int)(unsigned)total, B = (int)(total >> 32);
        const int used = min((int)ctl[1], M);                          // written by the frame before: another launch
        const int born = min(E, M - used);
        first[t] = used;
        ctl[1] = (unsigned)(used + born);
        frames[3 * t] = E, frames[3 * t + 1] = born, frames[3 * t + 2] = B;
        __hip_atomic_store(ctl, 0u, __ATOMIC_RELAXED, AG);             // the ticket of the next frame starts from 0
    }
}

__global__ __launch_bounds__(TRK_THREADS) void k_trk_assign(const u64 *__restrict__ mask, const unsigned *__restrict__ offs,
                                                            unsigned *__restrict__ bitmap, const int *__restrict__ first,
                                                            const int *__restrict__ frames, int t, int W, int H, int cell, int cols,
                                                            int cells, int M, int2 *__restrict__ pos, int *__restrict__ birth,
                                                            int *__restrict__ len, uint8_t *__restrict__ why)
{
    __shared__ unsigned sh_e[WAVES];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = (int)blockIdx.x * TRK_THREADS + tid;
    const u64 e = mask[(size_t)blockIdx.x * WAVES + wave];             // no bit at or above `cells` is set
    if (lane == 0) sh_e[wave] = (unsigned)__popcll(e);
    if ((tid & 31) == 0) bitmap[c >> 5] = 0u;                          // the bitmap is padded to whole work-groups
    __syncthreads();
    unsigned rank = offs[blockIdx.x] + (unsigned)__popcll(e & ((1ull << lane) - 1ull));
    for (int w = 0; w < WAVES; w++) rank += w < wave ? sh_e[w] : 0u;
    const int born = frames[3 * t + 1], base = first[t];
    if (((e >> lane) & 1ull) && rank < (unsigned)born) {
        const int id = min(max(base + (int)rank, 0), M - 1);
        pos[id] = trk_seed(min(c, cells - 1), cols, cell, W, H);       // row 0
        birth[id] = t;
        len[id] = 0;
        why[id] = OFC_TRAJ_RAN;
    }
}

template <bool STATE>
__global__ __launch_bounds__(TRK_THREADS) void k_trk_step(const float2 *__restrict__ flow, const uint8_t *__restrict__ state, int W, int H,
                                                          int cell, int cols, int cells, int L, int M, unsigned keep,
                                                          const int *__restrict__ first_lo, const unsigned *__restrict__ ctl,
                                                          int2 *__restrict__ pos, int *__restrict__ len, uint8_t *__restrict__ why,
                                                          unsigned *__restrict__ bitmap)
{
    const int lo = *first_lo, hi = min((int)ctl[1], M);                // the ids that can be live: born in the last L frames
    const long long at = (long long)lo + ((long long)blockIdx.x * TRK_THREADS + threadIdx.x);
    if (at >= hi) return;
    const int id = (int)min(max(at, 0ll), (long long)M - 1);
    if (why[id] != OFC_TRAJ_RAN) return;                               // ended, or full
    const int n = min(max(len[id], 0), L - 1);
    const int2 p = pos[(size_t)n * M + id];
    int X = p.x, Y = p.y;
    const int r = traj_step<STATE>(flow, state, W, H, keep, true, X, Y);
    if (r != OFC_TRAJ_RAN) {
        why[id] = (uint8_t)r;
        return;
    }
    pos[(size_t)(n + 1) * M + id] = make_int2(X, Y);
    len[id] = n + 1;
    if (n + 1 >= L) {
        why[id] = OFC_TRAJ_FULL;
        return;
    }
    const int at_cell = min(((Y >> 16) / cell) * cols + (X >> 16) / cell, cells - 1);       // a step that is taken lands inside
    (void)__hip_atomic_fetch_or(bitmap + (at_cell >> 5), 1u << (at_cell & 31), __ATOMIC_RELAXED, AG);
}

}  // namespace

int trk_check(int W, int H, int npair, int cell, int max_len, int64_t max_tracks, int keep)
{
    OFC_REQUIRE(W >= 1 && H >= 1, "W = %d, H = %d: at least 1", W, H);
    OFC_REQUIRE(npair >= 1 && npair <= TRAJ_MAX_PAIRS, "npair = %d: 1 .. %d", npair, TRAJ_MAX_PAIRS);
    OFC_REQUIRE(cell >= 1 && cell <= TRK_MAX_CELL, "cell = %d: 1 .. %d px", cell, TRK_MAX_CELL);
    const int64_t cells = cdiv64(W, cell) * cdiv64(H, cell);
    OFC_REQUIRE(cells <= TRK_MAX_CELLS, "%lld grid cells: at most 2^24", (long long)cells);
    OFC_REQUIRE(max_len >= 1 && max_len <= TRK_MAX_LEN, "max_len = %d: 1 .. %d steps", max_len, TRK_MAX_LEN);
    OFC_REQUIRE(max_tracks >= 1 && max_tracks <= TRK_MAX_TRACKS, "max_tracks = %lld: 1 .. 2^28", (long long)max_tracks);
    OFC_REQUIRE(keep >= 0 && keep <= 65535, "keep = %d: a set of states, 0 .. 65535", keep);
    if (W > FB_MAX_DIM || H > FB_MAX_DIM) {
        set_error("W = %d, H = %d: at most %d each (a position is an int32 in 1/65536 px)", W, H, FB_MAX_DIM);
        return OFC_EUNSUPPORTED;
    }
    if (((int64_t)max_len + 1) * max_tracks >= (1ll << 31)) {
        set_error("(max_len + 1) * max_tracks = %lld: below 2^31 positions", (long long)(((int64_t)max_len + 1) * max_tracks));
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

namespace {
size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
}  // namespace

size_t trk_scratch_bytes(const TrkGrid &g, int npair)
{
    const size_t G = (size_t)g.groups;
    return 16 + up16(G * 8 * 4) + up16(G * WAVES * 8) + up16(G * 8) + up16(G * 4) + up16((size_t)npair * 4);
}

void trk_scratch_carve(void *base, const TrkGrid &g, int npair, TrkScratch &sc)
{
    const size_t G = (size_t)g.groups;
    char *p = static_cast<char *>(base);
    sc.ctl = reinterpret_cast<unsigned *>(p), p += 16;
    sc.bitmap = reinterpret_cast<unsigned *>(p), p += up16(G * 8 * 4);
    sc.zero_bytes = (size_t)(p - static_cast<char *>(base));
    sc.mask = reinterpret_cast<u64 *>(p), p += up16(G * WAVES * 8);
    sc.partial = reinterpret_cast<u64 *>(p), p += up16(G * 8);
    sc.offs = reinterpret_cast<unsigned *>(p), p += up16(G * 4);
    sc.first = reinterpret_cast<int *>(p);
    (void)npair;
}

int launch_tracklets(const float *flow, const uint8_t *state, int W, int H, int npair, int cell, int max_len, int64_t max_tracks,
                     int keep, int32_t *pos, int32_t *birth, int32_t *len, uint8_t *why, int32_t *frames, const TrkScratch &sc,
                     hipStream_t s)
{
    const TrkGrid g = trk_grid(W, H, cell);
    const size_t WH = (size_t)W * H, Mz = (size_t)max_tracks;
    const int M = (int)max_tracks, L = max_len;
    OFC_HIP(hipMemsetAsync(pos, 0xFF, sizeof(int32_t) * 2 * Mz * ((size_t)L + 1), s));
    OFC_HIP(hipMemsetAsync(birth, 0xFF, sizeof(int32_t) * Mz, s));
    OFC_HIP(hipMemsetAsync(len, 0, sizeof(int32_t) * Mz, s));
    OFC_HIP(hipMemsetAsync(why, 0xFF, Mz, s));
    OFC_HIP(hipMemsetAsync(sc.ctl, 0, sc.zero_bytes, s));
    auto count = state ? &k_trk_count<true> : &k_trk_count<false>;
    auto step = state ? &k_trk_step<true> : &k_trk_step<false>;
    for (int t = 0; t < npair; t++) {
        const float2 *F = reinterpret_cast<const float2 *>(flow) + WH * t;
        const uint8_t *S = state ? state + WH * t : nullptr;
        hipLaunchKernelGGL(count, dim3((unsigned)g.groups), dim3(TRK_THREADS), 0, s, sc.bitmap, S, W, H, cell, g.cols, g.cells,
                           (unsigned)keep, t, M, g.groups, sc.mask, sc.partial, sc.offs, sc.ctl, sc.first, frames);
        hipLaunchKernelGGL(k_trk_assign, dim3((unsigned)g.groups), dim3(TRK_THREADS), 0, s, sc.mask, sc.offs, sc.bitmap, sc.first, frames,
                           t, W, H, cell, g.cols, g.cells, M, reinterpret_cast<int2 *>(pos), birth, len, why);
        // the ids that can be live at frame t were born in the last min(L, t+1) frames, at most `cells` per frame
        const int64_t window = std::min<int64_t>(max_tracks, (int64_t)g.cells * std::min(L, t + 1));
        hipLaunchKernelGGL(step, dim3((unsigned)cdiv64(window, TRK_THREADS)), dim3(TRK_THREADS), 0, s, F, S, W, H, cell, g.cols, g.cells, L,
                           M, (unsigned)keep, sc.first + std::max(0, t - L + 1), sc.ctl, reinterpret_cast<int2 *>(pos), len, why,
                           sc.bitmap);
    }
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
