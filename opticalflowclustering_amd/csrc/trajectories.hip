// trajectories.hip -- points followed through a clip's flow fields (ofc_traj*; the definition is in include/ofc.h).  The
// reference has no counterpart: its signature over time was a per-cell mean (drawGridsAndOutputCSV.py), it followed no point.
//
// k_traj_steps: one lane per point; a launch covers a chunk of consecutive pairs and the live position stays in registers
// across it.  The four 8-byte tap gathers and the state byte of a step are issued together before any is used, so a step
// costs one memory latency on the dependent chain.  Every index -- the state byte's and the taps of ended points included --
// is formed from the position clamped into the frame, whatever seeds and fields hold, and the trip count is the chunk
// length.  A step's row of the table is one coalesced 8-byte store per lane (the table is time-major for that), written by
// ended points too: an ended point stays where it ended.  All arithmetic after the quantisation (fb_check.h) is integer, so
// the order of the work does not matter.  Between launches the table is the carry: a point is live at step t iff len == t.
#include "trajectories.h"

namespace ofc {

namespace {

typedef long long i64;

template <bool STATE>
__global__ __launch_bounds__(TRAJ_THREADS) void k_traj_steps(const float2 *__restrict__ flow, const uint8_t *__restrict__ state, int W,
                                                             int H, int t0, int nstep, int P, unsigned keep,
                                                             const int2 *__restrict__ from, int2 *__restrict__ to,
                                                             int *__restrict__ len, uint8_t *__restrict__ why)
{
    const int p = (int)blockIdx.x * TRAJ_THREADS + (int)threadIdx.x;   // P <= 2^28: the grid's lanes stay below 2^28 + 256
    if (p >= P) return;
    const size_t WH = (size_t)W * H;
    const int xmax = (W - 1) << 16, ymax = (H - 1) << 16;              // W, H <= 16384: below 2^30
    const int2 at = from[p];                                           // the row of step t0
    int X = at.x, Y = at.y, n = len[p], reason = OFC_TRAJ_RAN;
    const bool was_live = n == t0;
    bool live = was_live;

    for (int j = 0; j < nstep; j++) {
        const float2 *F = flow + (size_t)j * WH;
        // everything that indexes comes from the clamped position; a live point past step 0 is inside, so nothing changes for it
        const int Xc = min(max(X, 0), xmax), Yc = min(max(Y, 0), ymax);
        const bool inside = Xc == X && Yc == Y;
        const int ix = Xc >> 16, iy = Yc >> 16;                        // in [0, W-1], [0, H-1]
        const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
        const int rx = min((Xc + 32768) >> 16, W - 1), ry = min((Yc + 32768) >> 16, H - 1);
        float2 f0 = make_float2(0.f, 0.f), f1 = f0, f2 = f0, f3 = f0;
        unsigned sb = 0;
        if (live) {                                                    // the five loads of the step, none used before all are issued
            f0 = F[iy * W + ix];
            f1 = F[iy * W + ix1];
            f2 = F[iy1 * W + ix];
            f3 = F[iy1 * W + ix1];
            if (STATE) sb = state[(size_t)j * WH + (size_t)(ry * W + rx)];
        }
        const FbVec q0 = fb_quantise(f0), q1 = fb_quantise(f1), q2 = fb_quantise(f2), q3 = fb_quantise(f3);
        const i64 fx = Xc & 65535, fy = Yc & 65535;
        const i64 w0 = (65536 - fx) * (65536 - fy), w1 = fx * (65536 - fy), w2 = (65536 - fx) * fy, w3 = fx * fy;
        const i64 Sx = w0 * q0.qu + w1 * q1.qu + w2 * q2.qu + w3 * q3.qu;      // |S| <= 2^32 * 2^26
        const i64 Sy = w0 * q0.qv + w1 * q1.qv + w2 * q2.qv + w3 * q3.qv;
        const int Xn = Xc + (int)((Sx + (1ll << 31)) >> 32), Yn = Yc + (int)((Sy + (1ll << 31)) >> 32);   // < 2^30 + 2^26
        if (live) {
            const bool trusted = !STATE || (sb < 4u && ((keep >> sb) & 1u));
            const bool valid = q0.valid && q1.valid && q2.valid && q3.valid;
            const bool lands = Xn >= 0 && Xn <= xmax && Yn >= 0 && Yn <= ymax;
            if (!inside) reason = OFC_TRAJ_LEAVES;
            else if (!trusted) reason = OFC_TRAJ_UNTRUSTED;
            else if (!valid) reason = OFC_TRAJ_INVALID;
            else if (!lands) reason = OFC_TRAJ_LEAVES;
            if (reason == OFC_TRAJ_RAN) {
                X = Xn, Y = Yn;
                n++;
            } else {
                live = false;
            }
        }
        to[(size_t)j * (size_t)P + p] = make_int2(X, Y);
    }
    if (was_live) {
        len[p] = n;
        if (!live) why[p] = (uint8_t)reason;
    }
}

}  // namespace

int traj_check(int W, int H, int npair, int64_t P, int keep, int pairs_per_launch)
{
    OFC_REQUIRE(W >= 1 && H >= 1, "W = %d, H = %d: at least 1", W, H);
    OFC_REQUIRE(npair >= 1 && npair <= TRAJ_MAX_PAIRS, "npair = %d: 1 .. %d", npair, TRAJ_MAX_PAIRS);
    OFC_REQUIRE(P >= 1 && P <= TRAJ_MAX_POINTS, "P = %lld: 1 .. 2^28 points", (long long)P);
    OFC_REQUIRE(keep >= 0 && keep <= 65535, "keep = %d: a set of states, 0 .. 65535", keep);
    OFC_REQUIRE(pairs_per_launch >= 0, "pairs_per_launch = %d: 0 (automatic) or the pairs of a launch", pairs_per_launch);
    if (W > FB_MAX_DIM || H > FB_MAX_DIM) {
        set_error("W = %d, H = %d: at most %d each (a position is an int32 in 1/65536 px)", W, H, FB_MAX_DIM);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

int traj_chunk_pairs(int npair, int64_t P, int pairs_per_launch)
{
    if (pairs_per_launch > 0) return std::min(pairs_per_launch, npair);
    return P <= OFC_TRAJ_ONE_LAUNCH_POINTS ? npair : std::min(npair, OFC_TRAJ_DENSE_PAIRS);
}

int launch_traj_begin(const int32_t *seeds, int64_t P, int32_t *pos, int32_t *len, uint8_t *why, hipStream_t s)
{
    OFC_HIP(hipMemsetAsync(len, 0, sizeof(int32_t) * (size_t)P, s));
    OFC_HIP(hipMemsetAsync(why, OFC_TRAJ_RAN, (size_t)P, s));
    if (seeds != pos) OFC_HIP(hipMemcpyAsync(pos, seeds, sizeof(int32_t) * 2 * (size_t)P, hipMemcpyDeviceToDevice, s));
    return OFC_OK;
}

int launch_traj_steps(const float *flow, const uint8_t *state, int W, int H, int t0, int nstep, int64_t P, int keep, const int32_t *from,
                      int32_t *to, int32_t *len, uint8_t *why, hipStream_t s)
{
    auto kern = state ? &k_traj_steps<true> : &k_traj_steps<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)cdiv64(P, TRAJ_THREADS)), dim3(TRAJ_THREADS), 0, s, reinterpret_cast<const float2 *>(flow),
                       state, W, H, t0, nstep, (int)P, (unsigned)keep, reinterpret_cast<const int2 *>(from),
                       reinterpret_cast<int2 *>(to), len, why);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_traj(const float *flow, const uint8_t *state, int W, int H, int npair, const int32_t *seeds, int64_t P, int keep,
                int pairs_per_launch, int32_t *pos, int32_t *len, uint8_t *why, hipStream_t s)
{
    const size_t WH = (size_t)W * H;
    const int chunk = traj_chunk_pairs(npair, P, pairs_per_launch);
    OFC_TRY(launch_traj_begin(seeds, P, pos, len, why, s));
    for (int t0 = 0; t0 < npair; t0 += chunk)
        OFC_TRY(launch_traj_steps(flow + 2 * WH * t0, state ? state + WH * t0 : nullptr, W, H, t0, std::min(chunk, npair - t0), P, keep,
                                  pos + 2 * (size_t)P * t0, pos + 2 * (size_t)P * (t0 + 1), len, why, s));
    return OFC_OK;
}

}  // namespace ofc
