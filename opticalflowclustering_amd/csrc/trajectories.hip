// trajectories.hip -- points followed through a clip's flow fields (ofc_traj*; the definition is in include/ofc.h).  The
// reference has no counterpart: its signature over time was a per-cell mean (drawGridsAndOutputCSV.py), it followed no point.
//
// k_traj_steps: one lane per point; a launch covers a chunk of consecutive pairs and the live position stays in registers
// across it.  The step itself is traj_step.h's, shared with the tracklets (tracklets.hip): the four 8-byte tap gathers and the
// state byte of a step are issued together before any is used, so a step costs one memory latency on the dependent chain.  Every index -- the state byte's and the taps of ended points included --
// is formed from the position clamped into the frame, whatever seeds and fields hold, and the trip count is the chunk
// length.  A step's row of the table is one coalesced 8-byte store per lane (the table is time-major for that), written by
// ended points too: an ended point stays where it ended.  All arithmetic after the quantisation (fb_check.h) is integer, so
// the order of the work does not matter.  Between launches the table is the carry: a point is live at step t iff len == t.
#include "trajectories.h"
#include "traj_step.h"

namespace ofc {

namespace {

template <bool STATE>
__global__ __launch_bounds__(TRAJ_THREADS) void k_traj_steps(const float2 *__restrict__ flow, const uint8_t *__restrict__ state, int W,
                                                             int H, int t0, int nstep, int P, unsigned keep,
                                                             const int2 *__restrict__ from, int2 *__restrict__ to,
                                                             int *__restrict__ len, uint8_t *__restrict__ why)
{
    const int p = (int)blockIdx.x * TRAJ_THREADS + (int)threadIdx.x;   // P <= 2^28: the grid's lanes stay below 2^28 + 256
    if (p >= P) return;
    const size_t WH = (size_t)W * H;
    const int2 at = from[p];                                           // the row of step t0
    int X = at.x, Y = at.y, n = len[p], reason = OFC_TRAJ_RAN;
    const bool was_live = n == t0;
    bool live = was_live;

    for (int j = 0; j < nstep; j++) {
        const int r = traj_step<STATE>(flow + (size_t)j * WH, STATE ? state + (size_t)j * WH : nullptr, W, H, keep, live, X, Y);
        if (live) {
            if (r == OFC_TRAJ_RAN) {
                n++;
            } else {
                reason = r;
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
