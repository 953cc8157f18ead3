// flow_iter.hip -- K4+K5(+K6) fused: one Farneback iteration in one kernel, its cost model, grid rule and launchers.
// Layouts and the contraction policy: flow_device.h.
#include "flow_device.h"
#include "flow_host.h"

namespace ofc {

// one vector of resize(prevFlow, (w,h), INTER_LINEAR) * mul at (x, y): the arithmetic of k_flow_resize (bit-exact)
struct UpsArgs {
    const float *src;     // coarse flow [pair][sh][sw][2]; nullptr = flow_in is already at this level's size
    int sw, sh;
    double scx, scy;
    float mul;
};

__device__ __forceinline__ float2 upsampled_flow(const float2 *__restrict__ s, int sw, int sh, double scx, double scy,
                                                 float mul, int x, int y)
{
#pragma clang fp contract(off)
    int sx0, sy0, sy1;
    float a1, b1;
    if (scx == 0.5 && scy == 0.5) {
        // exact x2 (the reference's pyr_scale 0.5 on even sizes): (d+0.5)*0.5-0.5 = 0.5d-0.25 is exact in f32 too,
        // so the taps come from integer arithmetic instead of two f64 evaluations per pixel -- same values
        const int sx = (x + 1) / 2 - 1, sy = (y + 1) / 2 - 1;          // floor(0.5d - 0.25)
        a1 = (x & 1) ? 0.25f : 0.75f;
        b1 = (y & 1) ? 0.25f : 0.75f;
        sx0 = sx;
        if (sx < 0) { a1 = 0.f; sx0 = 0; }
        if (sx >= sw - 1) { a1 = 0.f; sx0 = sw - 1; }
        sy0 = min(max(sy, 0), sh - 1);
        sy1 = min(max(sy + 1, 0), sh - 1);
    } else {
        lin_tap_x(x, scx, sw, sx0, a1);
        lin_tap_y(y, scy, sh, sy0, sy1, b1);
    }
    const float a0 = 1.f - a1, b0 = 1.f - b1;
    const int sx1 = (a1 == 0.f) ? sx0 : sx0 + 1;
    const float2 p00 = s[(size_t)sy0 * sw + sx0], p01 = s[(size_t)sy0 * sw + sx1];
    const float2 p10 = s[(size_t)sy1 * sw + sx0], p11 = s[(size_t)sy1 * sw + sx1];
    float h0x, h0y, h1x, h1y;
    if (a1 == 0.f) {
        h0x = p00.x; h0y = p00.y; h1x = p10.x; h1y = p10.y;
    } else {
        h0x = p00.x * a0 + p01.x * a1; h0y = p00.y * a0 + p01.y * a1;
        h1x = p10.x * a0 + p11.x * a1; h1y = p10.y * a0 + p11.y * a1;
    }
    return make_float2((h0x * b0 + h1x * b1) * mul, (h0y * b0 + h1y * b1) * mul);
}

// ------------------------------------------------------------------------------------------------
// K4+K5 fused: one Farneback iteration  flow_in -> flow_out  without M ever existing in memory.
// Same column march as k_box_solve, but the incoming row of M is COMPUTED (um_load/um_math: R0, flow_in,
// bilinear gather of R1) instead of loaded, and the outgoing row comes back from a 16-row ring that lives
// in REGISTERS (80 VGPRs per lane): the march is unrolled over super-steps of 16 rows so that every ring
// slot has a compile-time index.  (A first version kept the ring in a work-group-private global buffer:
// rocprof showed 2.2 GB of WRITE_SIZE and a 50 % L2 miss rate per level-0 launch -- the ring traffic alone
// was as large as the algorithmic traffic.)
// HBM traffic per pixel: 20 (R0) + 20 (R1, gathered) + 8 (flow in) + 8 (flow out) = 56 B, versus
// 68 + 28 (+20 for the second read of M) for the separate kernels.
// ------------------------------------------------------------------------------------------------
// UPS: the first iteration of a level reads its initial flow straight from the coarser level (bilinear x2, times
// 1/pyr_scale) instead of from a materialised upsampled copy -- K6 fused in, 16 B/px less traffic and one launch less.
// UPS = 0: flow_in is at this level's size; 1: bilinear upsample of the coarser level with general taps; 2: the exact x2
// pyramid (pyr_scale 0.5 on even sizes), whose taps follow a fixed parity pattern (see below)
// STAMP: diagnostic build (tools/fi_stamps.py): s_memtime stamps around the phases of a step, summed per wave into `dbg`
// [block][wave][8] -- where a step's cycles go; never used by the engine
// SUMS: also emit, per work-group, the f64 sums of the flow vectors it stores (`sums`: [grid][2]) -- the column sums Lloyd's
// centring needs, taken from the last level-0 iteration's epilogue instead of from an extra 5 GB sweep over the clip
// BIDIR: forward and backward flow of every pair from one launch (ofc_flow_calc_frames_dev_bidir).  `npair` is then the
// LOGICAL count, twice the number of frame pairs: logical pair q is (pair q >> 1, direction q & 1), so the two work-groups
// that read the same two R frames hold neighbouring same-XCD ids and march in step; the backward one swaps R0 and R1.
// Every flow buffer holds the forward fields of all pairs, then the backward fields.  The two halves need not be adjacent
// (level 0 ends in the caller's two buffers), and the argument block is the forward form's: the two pointers that only
// STAMP and SUMS read carry the bases of the backward halves -- `dbg` that of flow_out, `sums` that of flow_in (the
// coarse source with UPS).  The launch always sets both.
template <int M, int UPS, bool STAMP = false, bool SUMS = false, bool BIDIR = false>
__global__ __launch_bounds__(256, 2) void k_flow_iter(const float *__restrict__ Rb, size_t frame_stride_R,
                                                      const float *__restrict__ flow_inb,
                                                      float *__restrict__ flow_outb, int W, int H,
                                                      int rows_per_block /* multiple of 16 */, UpsArgs ups,
                                                      int tiles_x, int n_strips, int npair,
                                                      unsigned long long *__restrict__ dbg = nullptr,
                                                      double *__restrict__ sums = nullptr)
{
    constexpr int TXO = 256 - 2 * M;
    constexpr int NV = 2 * M + 4;
    constexpr int NV2 = (NV + 1) / 2;
    // Vertical sums of one row cross LDS as PAIRS of doubles, even pairs in one plane and odd pairs in another: the
    // horizontal pass's lane l reads pairs 2l .. 2l+8, so for a fixed q the 64 lanes read 64 consecutive 16-byte pairs
    // of one plane (conflict-free ds_read_b128; with the plain [column] layout the 32-byte lane stride was a 4-way bank
    // conflict: SQ_LDS_BANK_CONFLICT 1.3e8 of 2.2e8 LDS-active cycles per level-0 launch).  Plane pitch 136 doubles
    // = 64 B mod 128: the writers' two interleaved 16-byte streams then cover every bank exactly twice.
    constexpr int PLD = 136, PITCH = 2 * PLD;
    __shared__ __align__(16) double vs[5][BS_ROWS][PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware work-group -> (tile, pair) map.  Work-groups are dealt round-robin over the 8 XCDs, so ids L and
    // L+8 share an L2.  Consecutive same-XCD ids take the SAME tile of CONSECUTIVE pairs: frame t's R is R1 of pair
    // t-1 and R0 of pair t, and the two work-groups march down their strips in step, so the second read hits L2
    // instead of HBM.  (speed only: any placement gives the same result)
    const int tiles = tiles_x * n_strips;
    const int group = blockIdx.x / (8 * npair), rem = blockIdx.x - group * (8 * npair);
    static_assert(!BIDIR || (!STAMP && !SUMS), "the bidirectional mode borrows the STAMP and SUMS pointers");
    const int lpair = rem >> 3, tile = group * 8 + (rem & 7);
    const int pair = BIDIR ? lpair >> 1 : lpair, dir = BIDIR ? lpair & 1 : 0;
    if (tile >= tiles) {
        if (SUMS && threadIdx.x < 2) sums[(size_t)blockIdx.x * 2 + threadIdx.x] = 0.0;     // padding work-group of the grid
        return;
    }
    double su = 0, sv = 0;                          // SUMS: this thread's share of sum(u), sum(v)
    const int tile_x = tile % tiles_x, tile_y = tile / tiles_x;
    const int x0 = tile_x * TXO;
    const int y_begin = tile_y * rows_per_block;
    const int y_end = min(y_begin + rows_per_block, H);
    const size_t plane = (size_t)W * H;
    const float *R0 = Rb + (size_t)(pair + dir) * frame_stride_R;
    const float *R1 = BIDIR ? Rb + (size_t)(pair + 1 - dir) * frame_stride_R : R0 + frame_stride_R;
    // the direction's half of the two flow buffers (uniform: dir comes from the block id)
    const float *inb = UPS ? ups.src : flow_inb;
    float *outb = flow_outb;
    if (BIDIR && dir) {
        inb = reinterpret_cast<const float *>(sums);
        outb = reinterpret_cast<float *>(dbg);
    }
    const float2 *flow_in = UPS ? reinterpret_cast<const float2 *>(inb) + (size_t)pair * ups.sw * ups.sh
                                : reinterpret_cast<const float2 *>(inb) + (size_t)pair * plane;
    float2 *flow_out = reinterpret_cast<float2 *>(outb) + (size_t)pair * plane;
    const int xc = min(max(x0 - M + tid, 0), W - 1);
    const int vs_w = ((tid >> 1) & 1) * PLD + 2 * (tid >> 2) + (tid & 1);     // this column's slot in a row of vs
    const double scale = 1.0 / ((2 * M + 1) * (2 * M + 1));
    auto flow_at = [&](int row) -> float2 {
        if (UPS) return upsampled_flow(flow_in, ups.sw, ups.sh, ups.scx, ups.scy, ups.mul, xc, row);
        return flow_in[(size_t)row * W + xc];
    };
    // UPS with the exact x2 pyramid: this thread's horizontal taps never change, and the 4 fine rows of a step touch only
    // 3 or 4 distinct coarse rows -- interpolate each coarse row once per step (the arithmetic of upsampled_flow, shared)
    constexpr bool ups2 = UPS == 2;
    // the taps of the next step's two new coarse rows leave with this step's gathers (as fln does).  That keeps 8 more
    // registers live across um_math, which M = 4 and 5 do not have (2 and 6 VGPRs would spill): there they leave after it
    constexpr bool TAPS_EARLY = M != 4 && M != 5;
    int usx0 = 0, usx1 = 0;
    float ua1 = 0.f;
    if (ups2) {
        const int sx = (xc + 1) / 2 - 1;
        ua1 = (xc & 1) ? 0.25f : 0.75f;
        usx0 = sx;
        if (sx < 0) { ua1 = 0.f; usx0 = 0; }
        if (sx >= ups.sw - 1) { ua1 = 0.f; usx0 = ups.sw - 1; }
        usx1 = (ua1 == 0.f) ? usx0 : usx0 + 1;
    }
    auto coarse_taps = [&](int sy, float2 &p0, float2 &p1) {       // this thread's two taps of (clamped) coarse row sy
        const float2 *rowp = flow_in + (size_t)min(max(sy, 0), ups.sh - 1) * ups.sw;
        p0 = rowp[usx0];
        p1 = rowp[usx1];
    };
    auto coarse_lerp = [&](float2 p0, float2 p1) -> float2 {        // horizontal interpolation of upsampled_flow
#pragma clang fp contract(off)
        if (ua1 == 0.f) return p0;
        const float a0 = 1.f - ua1;
        return make_float2(p0.x * a0 + p1.x * ua1, p0.y * a0 + p1.y * ua1);
    };
    auto coarse_vert = [&](float2 h0, float2 h1, float b1) -> float2 {  // vertical interpolation of upsampled_flow, times mul
#pragma clang fp contract(off)
        const float b0 = 1.f - b1;
        return make_float2((h0.x * b0 + h1.x * b1) * ups.mul, (h0.y * b0 + h1.y * b1) * ups.mul);
    };
    // consecutive steps advance by two coarse rows: rows s0+2, s0+3 of a step are rows s0, s0+1 of the next (carried,
    // interpolated), and the taps of the next step's two new rows are requested one step ahead, like the flow vectors of the
    // non-UPS form, and interpolated (hnx) BEFORE the step's stores are issued (see "retire" below)
    float2 hcar[2], hnx[2], pn[2][2];
    bool have_next = false;
    float2 fl_last = ups2 ? flow_at(H - 1) : make_float2(0.f, 0.f);   // flow of the last image row this thread has seen

    float ring[16][5];          // ring[row & 15] = M(clamp(row)); statically indexed everywhere below
    double v[5] = {0, 0, 0, 0, 0};

    // ---- warm-up: rows y_begin-M .. y_begin+M (replicate-clamped), four at a time (all flow vectors of a batch first,
    //      then all gathers: two memory round trips per four rows; on the short strips of the coarse levels the warm-up
    //      is a third of a work-group's life) ----
#pragma unroll
    for (int j4 = -M; j4 <= M; j4 += BS_ROWS) {
        float2 fl[BS_ROWS];
        UmIn u[BS_ROWS];
        __builtin_amdgcn_s_setprio(3);
        if (ups2) {
            // the 16 taps of the group's four rows leave together, outside any branch (flow_at compiles to loads inside
            // divergent branches: one round trip per row); the arithmetic is upsampled_flow's exact-x2 case
            float2 tp[BS_ROWS][4];
#pragma unroll
            for (int q = 0; q < BS_ROWS; q++) {
                const int sy = (min(max(y_begin + j4 + q, 0), H - 1) + 1) / 2 - 1;
                coarse_taps(sy, tp[q][0], tp[q][1]);
                coarse_taps(sy + 1, tp[q][2], tp[q][3]);
            }
#pragma unroll
            for (int q = 0; q < BS_ROWS; q++) {
                const int row = min(max(y_begin + j4 + q, 0), H - 1);
                fl[q] = coarse_vert(coarse_lerp(tp[q][0], tp[q][1]), coarse_lerp(tp[q][2], tp[q][3]), (row & 1) ? 0.25f : 0.75f);
            }
        } else {
#pragma unroll
            for (int q = 0; q < BS_ROWS; q++) fl[q] = flow_at(min(max(y_begin + j4 + q, 0), H - 1));
        }
#pragma unroll
        for (int q = 0; q < BS_ROWS; q++)
            um_load(R0, R1, plane, W, H, xc, min(max(y_begin + j4 + q, 0), H - 1), fl[q], u[q]);
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int q = 0; q < BS_ROWS; q++) {
            if (j4 + q <= M) {
                const int row = min(max(y_begin + j4 + q, 0), H - 1);
                float m[5];
                um_math(u[q], W, H, xc, row, fl[q], m);
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    ring[(j4 + q + 16) & 15][c] = m[c];
                    v[c] += (double)m[c];
                }
            }
        }
    }

    // the flow vectors steer the gather addresses: fetched one step ahead (behind the current step's gathers) so that a
    // step does not start with a second, dependent memory round trip.  (UPS 1 computes them from 4 coarse taps: not
    // worth 16 more loads in flight; UPS 2 carries interpolated coarse rows instead, see hcar / hnx.)
    float2 fln[BS_ROWS];
    if (!UPS) {
#pragma unroll
        for (int r = 0; r < BS_ROWS; r++) fln[r] = flow_in[(size_t)min(y_begin + r + 1 + M, H - 1) * W + xc];
    }
    unsigned long long acc_t[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
    auto stamp = [&](int slot) {
        if (STAMP) {
            __builtin_amdgcn_sched_barrier(0);
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_sched_barrier(0);
            if (slot >= 0) acc_t[slot] += t - tprev;
            tprev = t;
        }
    };
    auto request_next = [&](int yc) {       // taps of coarse rows s0'+2, s0'+3 of the step after the one at yc
        const int s0n = (yc + BS_ROWS + 1 + M + 1) / 2 - 1;
        coarse_taps(s0n + 2, pn[0][0], pn[0][1]);
        coarse_taps(s0n + 3, pn[1][0], pn[1][1]);
    };
    auto retire_next = [&]() {
        hnx[0] = coarse_lerp(pn[0][0], pn[0][1]);
        hnx[1] = coarse_lerp(pn[1][0], pn[1][1]);
        asm volatile("" : "+v"(hnx[0].x), "+v"(hnx[0].y), "+v"(hnx[1].x), "+v"(hnx[1].y));
    };
    stamp(-1);
    for (int y16 = y_begin; y16 < y_end; y16 += 16) {
#pragma unroll
        for (int q4 = 0; q4 < 4; q4++) {
            const int yc = y16 + 4 * q4;
            if (yc < y_end) {                                   // uniform
                // ---- advance the window over the 4 rows of this step; loads batched two rows at a time ----
                float2 fl[BS_ROWS];
                float mi[BS_ROWS][5];
                if (ups2) {
#pragma clang fp contract(off)
                    const int e0 = yc + 1 + M, s0 = (e0 + 1) / 2 - 1;      // floor(0.5 e - 0.25) of the first fine row
                    float2 hc[BS_ROWS];
                    if (have_next) {                            // uniform
                        hc[0] = hcar[0];
                        hc[1] = hcar[1];
                        hc[2] = hnx[0];
                        hc[3] = hnx[1];
                    } else {
#pragma unroll
                        for (int j = 0; j < BS_ROWS; j++) {
                            float2 p0, p1;
                            coarse_taps(s0 + j, p0, p1);
                            hc[j] = coarse_lerp(p0, p1);
                        }
                    }
                    hcar[0] = hc[2];
                    hcar[1] = hc[3];
                    have_next = true;
#pragma unroll
                    for (int r = 0; r < BS_ROWS; r++) {
                        // yc = 0 (mod 4), so the parity of e0 is that of 1 + M: fine rows e0+r sit between coarse rows
                        // s0 + off, s0 + off + 1 with off = 0,1,1,2 (e0 even) or 0,0,1,1 (e0 odd)
                        constexpr bool E0_EVEN = ((1 + M) & 1) == 0;
                        const int off = E0_EVEN ? (r + 1) / 2 : r / 2;
                        const float b1 = (E0_EVEN == ((r & 1) == 0)) ? 0.75f : 0.25f, b0 = 1.f - b1;
                        const float2 h0 = hc[off], h1 = hc[off + 1];
                        fl[r] = make_float2((h0.x * b0 + h1.x * b1) * ups.mul, (h0.y * b0 + h1.y * b1) * ups.mul);
                        // rows below the image replicate row H-1 (the gathers are clamped to it): so does their flow
                        if (e0 + r > H - 1) fl[r] = fl_last; else fl_last = fl[r];      // uniform
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < BS_ROWS; r++)
                        fl[r] = UPS ? flow_at(min(yc + r + 1 + M, H - 1)) : fln[r];
                }
                {
                    UmIn u[BS_ROWS];
                    // a wave that is ready to issue its gathers goes first: while its SIMD neighbour grinds through a
                    // horizontal pass, the requests of this step (32 gathers + 4 flow vectors or coarse taps) leave back to
                    // back instead of trickling out between the neighbour's VALU instructions (level-0 launch 783 -> 655 us).
                    // No s_waitcnt vmcnt sits among them: everything they depend on was retired before the previous step's
                    // stores ("retire" below; tools/waitcnt_listing.py shows the sequence).  UPS 1 keeps its dependent fetch
                    // here, and the first of the four unrolled steps keeps the wait of the way in from the front of the loop
                    // 
                    stamp(0);                                   // 0: loop head, flow vectors / coarse taps of this step
                    __builtin_amdgcn_s_setprio(3);
#pragma unroll
                    for (int q = 0; q < BS_ROWS; q++)            // the gathers of all four rows in flight together
                        um_load(R0, R1, plane, W, H, xc, min(yc + q + 1 + M, H - 1), fl[q], u[q]);
                    if (!UPS) {
#pragma unroll
                        for (int r = 0; r < BS_ROWS; r++)
                            fln[r] = flow_in[(size_t)min(yc + BS_ROWS + r + 1 + M, H - 1) * W + xc];
                    }
                    if (ups2 && TAPS_EARLY) request_next(yc);
                    stamp(1);                                   // 1: issuing the gathers
                    if (STAMP) {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        stamp(2);                               // 2: waiting for the operands
                    }
                    __builtin_amdgcn_s_setprio(2);
#pragma unroll
                    // rows below the image replicate row H-1: the loads above were clamped to it, and the same inputs give
                    // the same matrix entries again (no carried copy, no select)
                    for (int r = 0; r < BS_ROWS; r++)
                        um_math(u[r], W, H, xc, min(yc + r + 1 + M, H - 1), fl[r], mi[r]);
                }
                if (ups2 && !TAPS_EARLY) request_next(yc);     // (the gathered operands are dead now)
                stamp(7);                                       // 7: matrix arithmetic
                // the barrier that protects `vs` from the previous step's readers sits HERE, after this step's loads and
                // matrix arithmetic: a wave that finished its horizontal pass early starts its gathers without waiting
                __syncthreads();
                stamp(3);                                       // 3: first barrier
#pragma unroll
                for (int r = 0; r < BS_ROWS; r++) {
                    const int s_in = (4 * q4 + r + 1 + M) & 15, s_out = (4 * q4 + r + 16 - M) & 15;
#pragma unroll
                    for (int c = 0; c < 5; c++) {
                        vs[c][r][vs_w] = v[c];
                        v[c] += (double)mi[r][c] - (double)ring[s_out][c];
                    }
#pragma unroll
                    for (int c = 0; c < 5; c++) ring[s_in][c] = mi[r][c];
                }
                stamp(4);                                       // 4: ring / vertical sums / exchange writes
                __syncthreads();
                stamp(5);                                       // 5: second barrier
                __builtin_amdgcn_s_setprio(0);
                // retire: what was prefetched for the next step becomes register values HERE, before this step's stores are
                // issued.  A store is counted in vmcnt like a load and the counter retires in order: left to the next loop
                // head, the wait for these operands would also wait for the stores issued after them
                if (!UPS) {
#pragma unroll
                    for (int r = 0; r < BS_ROWS; r++) asm volatile("" : "+v"(fln[r].x), "+v"(fln[r].y));
                }
                if (ups2) retire_next();
                const int y = yc + wave;
                const int xo = x0 + 4 * lane;
                if (y < y_end && 4 * lane < TXO && xo < W) {
                    double S[5][4];
#pragma unroll
                    for (int c = 0; c < 5; c++) {
                        double a[2 * NV2];
#pragma unroll
                        for (int q = 0; q < NV2; q++) {
                            double2 d = *reinterpret_cast<const double2 *>(&vs[c][wave][(q & 1) * PLD + 2 * (lane + (q >> 1))]);
                            a[2 * q] = d.x; a[2 * q + 1] = d.y;
                        }
                        double s = a[0];
#pragma unroll
                        for (int q = 1; q <= 2 * M; q++) s += a[q];
                        S[c][0] = s;
#pragma unroll
                        for (int o = 1; o < 4; o++) {
                            s += a[2 * M + o] - a[o - 1];
                            S[c][o] = s;
                        }
                    }
                    float2 fo[4];
#pragma unroll
                    for (int o = 0; o < 4; o++) {
                        const double g11 = S[0][o] * scale, g12 = S[1][o] * scale, g22 = S[2][o] * scale,
                                     h1 = S[3][o] * scale, h2 = S[4][o] * scale;
                        const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
                        fo[o] = make_float2((float)((g11 * h2 - g12 * h1) * idet), (float)((g22 * h1 - g12 * h2) * idet));
                    }
                    float2 *dst = flow_out + (size_t)y * W + xo;
                    if (4 * lane + 3 < TXO && xo + 3 < W && (W & 1) == 0) {      // 32 contiguous, 16-B aligned bytes
                        // both 16-byte vectors are formed before either is stored: two stores (left alone, the compiler
                        // shares the store of the fourth vector with the per-pixel path and issues 16 + 8 + 8 bytes)
                        typedef float f4v __attribute__((ext_vector_type(4)));
                        f4v o0 = {fo[0].x, fo[0].y, fo[1].x, fo[1].y}, o1 = {fo[2].x, fo[2].y, fo[3].x, fo[3].y};
                        asm volatile("" : "+v"(o0), "+v"(o1));
                        reinterpret_cast<f4v *>(dst)[0] = o0;
                        reinterpret_cast<f4v *>(dst)[1] = o1;
                        // behind the stores and inside the branch: in front of it the sums cost the registers of the two
                        // tuples (the form spilled).  All four vectors are inside the tile and the image here; same order
                        // of additions as below
                        if (SUMS) {
                            su += (double)o0.x; sv += (double)o0.y;
                            su += (double)o0.z; sv += (double)o0.w;
                            su += (double)o1.x; sv += (double)o1.y;
                            su += (double)o1.z; sv += (double)o1.w;
                        }
                    } else {
#pragma unroll
                        for (int o = 0; o < 4; o++)
                            if (4 * lane + o < TXO && xo + o < W) {
                                dst[o] = fo[o];
                                if (SUMS) { su += (double)fo[o].x; sv += (double)fo[o].y; }
                            }
                    }
                }
                stamp(6);                                       // 6: horizontal sums + solve + stores
            }
        }
    }
    if (STAMP && dbg && lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; i++) dbg[((size_t)blockIdx.x * 4 + wave) * 8 + i] = acc_t[i];
    }
    if (SUMS) {                 // fixed order: shuffle tree inside the wave, then waves 0..3
        for (int off = 32; off >= 1; off >>= 1) {
            su += __shfl_down(su, off, 64);
            sv += __shfl_down(sv, off, 64);
        }
        __syncthreads();        // the last step's readers are done with vs
        if (lane == 0) { vs[0][0][2 * wave] = su; vs[0][0][2 * wave + 1] = sv; }
        __syncthreads();
        if (tid < 2) sums[(size_t)blockIdx.x * 2 + tid] = ((vs[0][0][tid] + vs[0][0][2 + tid]) + vs[0][0][4 + tid]) + vs[0][0][6 + tid];
    }
}

static int flow_iter_rows(int W, int H, int npair, int winsize)
{
    // cost model: a launch runs in ceil(blocks / resident) rounds (224 VGPRs -> 2 work-groups per CU), each as
    // long as one strip incl. its 2m-row window warm-up.  Pick the strip count that minimises rounds x strip.
    // (Speed only: every height gives the same bits.  tests/test_flow_geometry_host.py asks this model, through
    // ofc_flow_launch_geometry, which heights the suite's tables reach -- retune it and that test says what went missing.)
    const int tiles_x = cdiv(W, 256 - (winsize - 1));
    const int resident = 2 * 256;
    int best_rows = cdiv(H, 16) * 16;
    int64_t best_cost = LLONG_MAX;
    for (int n = 1; n <= 32; n++) {
        const int rows = cdiv(cdiv(H, n), 16) * 16;
        if (rows < 16 && n > 1) break;
        const int64_t blocks = (int64_t)tiles_x * cdiv(H, rows) * npair;
        const int64_t cost = cdiv64(blocks, resident) * (rows + winsize - 1);
        if (cost < best_cost) { best_cost = cost; best_rows = rows; }
    }
    return best_rows;
}

// The one rule for the fused iteration's grid: every launch of k_flow_iter (and of its pipelined copy), the scratch its
// column sums are written into and the geometry exports ask it.  A tile is 256 columns less the window's halo; the tiles of a
// field are rounded up to groups of eight (one per XCD; the padding work-groups return at once).
FlowIterGrid flow_iter_grid(int W, int H, int fields, int winsize, int rows)
{
    FlowIterGrid g;
    // a height of the caller's (the parity tests walk every strip height on small frames) is rounded up to whole
    // super-steps, as the kernel needs; one above the frame is one strip
    g.rows = rows == 0 ? flow_iter_rows(W, H, fields, winsize) : cdiv(std::min(rows, 1 << 30), 16) * 16;
    g.tiles_x = cdiv(W, 256 - (winsize - 1));
    g.strips = cdiv(H, g.rows);
    g.grid = cdiv(g.tiles_x * g.strips, 8) * 8 * fields;
    return g;
}

int flow_iter_max_grid(int W, int H, int npair, int winsize) { return flow_iter_grid(W, H, npair, winsize).grid; }

// the limits of launch_flow_iter that depend on the level's size and the window alone (also asked by flow_levels_check)
int flow_iter_check(int W, int H, int winsize)
{
    if (winsize > 15) { set_error("fused iteration supports winsize <= 15 (ring of 16 rows)"); return OFC_EUNSUPPORTED; }
    if ((int64_t)W * H * 5 >= (1ll << 30)) { set_error("frame too large for 32-bit R offsets (%dx%d)", W, H); return OFC_EUNSUPPORTED; }
    return OFC_OK;
}

static UpsArgs ups_args(const FlowCoarse &c, int W, int H)
{
    UpsArgs u;
    u.src = c.src; u.sw = c.sw; u.sh = c.sh; u.mul = c.mul;
    u.scx = c.src ? (double)c.sw / W : 1.0; u.scy = c.src ? (double)c.sh / H : 1.0;
    return u;
}

// what every build of k_flow_iter takes besides its grid; p12 and p13 are the kernel's last two pointers: `dbg` of the
// STAMP build and `sums` of the SUMS build, the bases of the backward halves in the bidirectional one, null otherwise
struct FlowIterArgs {
    const float *R;
    size_t frame_stride_R;
    const float *flow_in;
    float *flow_out;
    int W, H, fields;
    UpsArgs u;
    unsigned long long *p12;
    double *p13;
};

// the one launch of k_flow_iter
template <int MM, int UPS, bool BIDIR, bool STAMP = false, bool SUMS = false>
static void flow_iter_launch(const FlowIterGrid &g, const FlowIterArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL((k_flow_iter<MM, UPS, STAMP, SUMS, BIDIR>), dim3(g.grid), dim3(256), 0, s, a.R, a.frame_stride_R, a.flow_in,
                       a.flow_out, a.W, a.H, g.rows, a.u, g.tiles_x, g.strips, a.fields, a.p12, a.p13);
}

// the window picks MM; the coarse level picks UPS: 2 for the exact x2 pyramid, 1 for general taps, 0 for none
template <int MM, bool BIDIR>
static void flow_iter_launch_ups(const FlowIterGrid &g, const FlowIterArgs &a, hipStream_t s)
{
    if (a.u.src && a.u.scx == 0.5 && a.u.scy == 0.5) flow_iter_launch<MM, 2, BIDIR>(g, a, s);
    else if (a.u.src) flow_iter_launch<MM, 1, BIDIR>(g, a, s);
    else flow_iter_launch<MM, 0, BIDIR>(g, a, s);
}

template <bool BIDIR>
static int flow_iter_dispatch(int winsize, const FlowIterGrid &g, const FlowIterArgs &a, hipStream_t s)
{
    switch (winsize) {
    case 5: flow_iter_launch_ups<2, BIDIR>(g, a, s); break;
    case 7: flow_iter_launch_ups<3, BIDIR>(g, a, s); break;
    case 9: flow_iter_launch_ups<4, BIDIR>(g, a, s); break;
    case 11: flow_iter_launch_ups<5, BIDIR>(g, a, s); break;
    case 13: flow_iter_launch_ups<6, BIDIR>(g, a, s); break;
    case 15: flow_iter_launch_ups<7, BIDIR>(g, a, s); break;
    default:
        set_error("winsize %d unsupported by the fused iteration (odd 5..15)", winsize);
        return OFC_EUNSUPPORTED;
    }
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_flow_iter(const float *R, size_t frame_stride_R, const float *flow_in, float *flow_out, int npair, int W, int H,
                     int winsize, hipStream_t s, const FlowCoarse &coarse, const FlowSums &sums, int rows_per_block)
{
    OFC_TRY(flow_iter_check(W, H, winsize));
    if (rows_per_block < 0) { set_error("rows_per_block %d is negative (0 = automatic)", rows_per_block); return OFC_EINVAL; }
    const FlowIterGrid g = flow_iter_grid(W, H, npair, winsize, rows_per_block);
    // OFC_FLOW_PIPE=1: the software-pipelined experiment of flow_experiments.hip (bit-identical output, 2.6x slower: it
    // does not fit 256 VGPRs); read at every launch because its parity test toggles it
    {
        const char *e = getenv("OFC_FLOW_PIPE");
        if (e && e[0] == '1' && winsize == 15 && !coarse.src) return launch_flow_iter_pipe(R, frame_stride_R, flow_in, flow_out, npair, W, H, g, s, sums);
    }
    FlowIterArgs a = {R, frame_stride_R, flow_in, flow_out, W, H, npair, ups_args(coarse, W, H), nullptr, nullptr};
    if (sums.out) {             // the last iteration of level 0: also sum(u), sum(v) of the field it writes -> sums.out[2]
        if (coarse.src || winsize != 15) { set_error("flow sums are emitted by the plain winsize-15 iteration only"); return OFC_EUNSUPPORTED; }
        if ((size_t)g.grid * 2 > sums.doubles) { set_error("flow sums: scratch too small (%d work-groups)", g.grid); return OFC_EINVAL; }
        a.p13 = sums.scratch;
        flow_iter_launch<7, 0, false, false, true>(g, a, s);
        OFC_HIP(hipGetLastError());
        return launch_reduce_records(sums.scratch, g.grid, 2, sums.out, s, nullptr);
    }
    return flow_iter_dispatch<false>(winsize, g, a, s);
}

// One iteration of both directions of `npair` frame pairs (k_flow_iter<.., BIDIR>): 2 npair logical pairs in one grid, strips
// sized for that work.  in/out/coarse: the forward and the backward half of each buffer, [npair] fields each; coarse.src null
// = in_* is at this level's size.
int launch_flow_iter_bidir(const float *R, size_t frame_stride_R, const float *in_fwd, const float *in_bwd, float *out_fwd,
                           float *out_bwd, int npair, int W, int H, int winsize, hipStream_t s, const FlowCoarse &coarse,
                           const float *coarse_bwd)
{
    OFC_TRY(flow_iter_check(W, H, winsize));
    if (npair < 1 || npair > (1 << 20)) { set_error("bidirectional iteration: %d pairs", npair); return OFC_EINVAL; }
    const int lp = 2 * npair;
    // the backward bases ride in the two pointer arguments the forward form leaves unused (see k_flow_iter)
    unsigned long long *out_b = reinterpret_cast<unsigned long long *>(out_bwd);
    double *in_b = reinterpret_cast<double *>(const_cast<float *>(coarse.src ? coarse_bwd : in_bwd));
    const FlowIterArgs a = {R, frame_stride_R, in_fwd, out_fwd, W, H, lp, ups_args(coarse, W, H), out_b, in_b};
    return flow_iter_dispatch<true>(winsize, flow_iter_grid(W, H, lp, winsize), a, s);
}

// diagnostic launch of the stamped build (non-UPS, winsize 15); dbg: [grid][4][8] u64, zeroed by the caller
int launch_flow_iter_stamped(const float *R, size_t frame_stride_R, const float *flow_in, float *flow_out, int npair, int W,
                             int H, hipStream_t s, unsigned long long *dbg, int *grid_out)
{
    const FlowIterGrid g = flow_iter_grid(W, H, npair, 15);
    if (grid_out) *grid_out = g.grid;
    const FlowIterArgs a = {R, frame_stride_R, flow_in, flow_out, W, H, npair, ups_args(FlowCoarse(), W, H), dbg, nullptr};
    if (dbg) flow_iter_launch<7, 0, false, true>(g, a, s);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
