// blobs.h -- connected components of a key map (blobs.hip, blobs_api.cpp): limits and launchers.  include/ofc.h has the
// definition.
#pragma once
#include "lloyd_common.h"

#include <algorithm>
#include <numeric>

namespace ofc {

constexpr int BLOB_TW = OFC_BLOB_TILE_W, BLOB_TH = OFC_BLOB_TILE_H, BLOB_NF = OFC_BLOB_FIELDS;
constexpr int BLOB_MAX_PAIRS = 65535, BLOB_MAX_BLOBS = 65536;
constexpr int BLOB_SHARE = 2048;       // consecutive pixels of a pair a work-group of the table kernels takes

// what a kernel's capped loop leaves in the error word when it runs out (it cannot, by the algorithm)
enum { BLOB_ERR_LOCAL = 1, BLOB_ERR_SEAM = 2, BLOB_ERR_FLATTEN = 4 };

// OFC_OK, OFC_EINVAL or OFC_EUNSUPPORTED (message set): what ofc_blob_check documents.  Host only.
int blob_check(int W, int H, int npair, int connectivity, int min_area, int max_blobs);
// flow [npair][H][W][2] -> keys [npair][H][W].  st (mean, centred centres, cn set) is read only when k > 0.
int launch_blob_keys(const float *flow, int W, int H, int npair, bool use_thr, float thr, const LloydState *st, int k,
                     uint32_t select, bool merge, uint8_t *keys, hipStream_t s);
// the three stages of the label map, each its own launch; err: one int32 on the device, OR-ed with BLOB_ERR_*
int launch_blob_local(const uint8_t *keys, int W, int H, int npair, int connectivity, int32_t *labels, int *err, hipStream_t s);
int launch_blob_seam(const uint8_t *keys, int W, int H, int npair, int connectivity, int32_t *labels, int *err, hipStream_t s);
int launch_blob_flatten(int W, int H, int npair, int32_t *labels, int *err, hipStream_t s);
// the table: words int32 [npair][H][W] of scratch (areas, then slots), table [npair][max_blobs][12], found [npair];
// clears words and found, counts, hands out slots, accumulates.  flow may be nullptr.
int launch_blob_table(const uint8_t *keys, const int32_t *labels, const float *flow, int W, int H, int npair, int min_area,
                      int max_blobs, int32_t *words, int64_t *table, int32_t *found, hipStream_t s);
// labels [npair][H][W] -> words int32 [npair][H][W]: cleared, then the pixel count of every component at its root (the
// first step of launch_blob_table, on its own for the blob links)
int launch_blob_area(const int32_t *labels, int W, int H, int npair, int32_t *words, hipStream_t s);

// slots in the device's order -> the table of the definition: sorted by root, none on overflow
inline void blob_order_records(const int64_t *slots, int found, int max_blobs, int64_t *out, int32_t *n)
{
    const int have = found >= 0 && found <= max_blobs ? found : 0;
    std::vector<int> idx(have);
    std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&](int a, int b) { return slots[(size_t)a * BLOB_NF] < slots[(size_t)b * BLOB_NF]; });
    for (int i = 0; i < have; i++) memcpy(out + (size_t)i * BLOB_NF, slots + (size_t)idx[i] * BLOB_NF, sizeof(int64_t) * BLOB_NF);
    memset(out + (size_t)have * BLOB_NF, 0, sizeof(int64_t) * BLOB_NF * (size_t)(max_blobs - have));
    *n = have;
}

// blobs_api.cpp: device to host as ofc_blob_table_read documents it (sorted by root, none on overflow); synchronous copies
int blob_table_read(const int64_t *table_dev, const int32_t *found_dev, int npair, int max_blobs, int64_t *table_host,
                    int32_t *n_host, int32_t *found_host);

}  // namespace ofc
