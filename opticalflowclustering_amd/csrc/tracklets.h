// tracklets.h -- dense trajectories with reseeding (tracklets.hip, tracklets_api.cpp): limits, the scratch of a call and the
// launcher.  include/ofc.h has the definition.
#pragma once
#include "trajectories.h"

namespace ofc {

constexpr int TRK_THREADS = OFC_TRACKLET_THREADS;            // lanes of every work-group: cells of the two birth kernels, ids of the step
constexpr int TRK_MAX_CELL = 16384, TRK_MAX_CELLS = 1 << 24, TRK_MAX_LEN = OFC_TRACKLET_MAX_LEN;
constexpr int64_t TRK_MAX_TRACKS = OFC_TRACKLET_MAX_TRACKS;

struct TrkGrid {
    int cols, rows, cells, groups;                           // groups: the work-groups of TRK_THREADS cells
};
inline TrkGrid trk_grid(int W, int H, int cell)
{
    TrkGrid g;
    g.cols = cdiv(W, cell), g.rows = cdiv(H, cell);
    g.cells = g.cols * g.rows, g.groups = cdiv(g.cells, TRK_THREADS);
    return g;
}

// OFC_OK, OFC_EINVAL or OFC_EUNSUPPORTED (message set): what ofc_tracklets_check documents.  Host only.
int trk_check(int W, int H, int npair, int cell, int max_len, int64_t max_tracks, int keep);

// The scratch of one call, in one allocation.  `ctl` leads it: ctl[0] the ticket of the count kernel, ctl[1] `used`; a
// 16-byte block that launch_tracklets zeroes together with the bitmap behind it.
struct TrkScratch {
    unsigned *ctl = nullptr;                                 // [4]
    unsigned *bitmap = nullptr;                              // [groups * 8]: a bit per cell, padded to whole work-groups of cells
    unsigned long long *mask = nullptr;                      // [groups * 4]: the empty cells of every wave of the count kernel
    unsigned long long *partial = nullptr;                   // [groups]: blocked << 32 | empty of every work-group
    unsigned *offs = nullptr;                                // [groups]: the empty cells before every work-group
    int *first = nullptr;                                    // [npair]: `used` before frame t's births
    size_t zero_bytes = 0;                                   // ctl and bitmap
};
size_t trk_scratch_bytes(const TrkGrid &g, int npair);
void trk_scratch_carve(void *base, const TrkGrid &g, int npair, TrkScratch &sc);

// the whole chain on stream s: the clears, then per frame the two birth kernels and the step; nothing is read back
int launch_tracklets(const float *flow, const uint8_t *state, int W, int H, int npair, int cell, int max_len, int64_t max_tracks,
                     int keep, int32_t *pos, int32_t *birth, int32_t *len, uint8_t *why, int32_t *frames, const TrkScratch &sc,
                     hipStream_t s);

}  // namespace ofc
