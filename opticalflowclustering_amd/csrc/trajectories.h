// trajectories.h -- points followed through a clip's flow fields (trajectories.hip, trajectories_api.cpp, stream_api.cpp):
// limits, the launch model and the launchers.  include/ofc.h has the definition.
#pragma once
#include "fb_check.h"

namespace ofc {

constexpr int TRAJ_THREADS = OFC_TRAJ_THREADS, TRAJ_MAX_PAIRS = 65535;
constexpr int64_t TRAJ_MAX_POINTS = OFC_TRAJ_MAX_POINTS;

// OFC_OK, OFC_EINVAL or OFC_EUNSUPPORTED (message set): what ofc_traj_check documents.  Host only.
int traj_check(int W, int H, int npair, int64_t P, int keep, int pairs_per_launch);
// the pairs a launch takes: pairs_per_launch > 0 forces it (above npair: npair), 0 asks the cost model.  Host only.
int traj_chunk_pairs(int npair, int64_t P, int pairs_per_launch);
// len = 0, why = OFC_TRAJ_RAN for all P points, and the seeds into row 0 of pos unless they are that row already
int launch_traj_begin(const int32_t *seeds, int64_t P, int32_t *pos, int32_t *len, uint8_t *why, hipStream_t s);
// steps t0 .. t0+nstep-1 in one launch: flow and state (may be nullptr) point at pair t0, `from` [P][2] holds the positions
// before step t0 and `to` [nstep][P][2] takes those after every step (in one table: rows t0 and t0+1 ..); a point is live iff
// len[p] == t0
int launch_traj_steps(const float *flow, const uint8_t *state, int W, int H, int t0, int nstep, int64_t P, int keep, const int32_t *from,
                      int32_t *to, int32_t *len, uint8_t *why, hipStream_t s);
// the whole chain: begin, then the launches of traj_chunk_pairs pairs each
int launch_traj(const float *flow, const uint8_t *state, int W, int H, int npair, const int32_t *seeds, int64_t P, int keep,
                int pairs_per_launch, int32_t *pos, int32_t *len, uint8_t *why, hipStream_t s);

}  // namespace ofc
