// blob_links.h -- links between the blobs of consecutive pairs (blob_links.hip, blob_links_api.cpp): limits and launchers.
// include/ofc.h has the definition, blob_links_host.h the device layout and the host's way to the table.
#pragma once
#include "blob_links_host.h"
#include "blobs.h"

namespace ofc {

static_assert(BLOB_LINK_NF == OFC_BLOB_LINK_FIELDS, "the header's row width");
constexpr int32_t BLOB_NO_MOVE = (int32_t)OFC_BLOB_NO_MOVE;

// OFC_OK, OFC_EINVAL or OFC_EUNSUPPORTED (message set): what ofc_blob_link_check documents.  Host only.
int blob_link_check(int W, int H, int npair, int min_area, int max_links);
// flow [npair][H][W][2] -> moves int32 [npair][H][W]
int launch_blob_moves(const float *flow, int W, int H, int npair, int32_t *moves, hipStream_t s);
// A transition's table on the device: uint64 keys [cap] and int32 votes [cap] (cap = blob_link_capacity(max_links)) and one
// counter word.  The launchers take ntrans consecutive transitions: keys [ntrans][cap], votes [ntrans][cap], counters [ntrans].
// clears them
int launch_blob_links_clear(int max_links, int ntrans, uint64_t *keys, int32_t *votes, int32_t *counters, hipStream_t s);
// Votes ntrans transitions: transition t goes from pair t of labels_a / moves / areas_a (each [.][H][W]) to pair t of
// labels_b / areas_b; for one array of npair pairs, labels_b = labels_a + P and ntrans = npair - 1.  areas: the pixel count
// at every root (launch_blob_area).  Nothing is cleared here.
int launch_blob_links(const int32_t *labels_a, const int32_t *moves, const int32_t *areas_a, const int32_t *labels_b,
                      const int32_t *areas_b, int W, int H, int ntrans, int min_area, int max_links, uint64_t *keys,
                      int32_t *votes, int32_t *counters, hipStream_t s);
// device to host as ofc_blob_links_read documents it; synchronous copies
int blob_links_read(const uint64_t *keys_dev, const int32_t *votes_dev, const int32_t *counters_dev, int ntrans, int max_links,
                    int64_t *links_host, int32_t *nlinks_host);

}  // namespace ofc
