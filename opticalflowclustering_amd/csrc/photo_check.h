// photo_check.h -- the photometric (brightness-constancy) check of a flow field against the frames it was computed from
// (photo_check.hip, photo_check_api.cpp, stream_api.cpp): limits and launcher.  include/ofc.h has the definition.
#pragma once
#include "ofc_common.h"

namespace ofc {

constexpr int PHOTO_SHARE = OFC_PHOTO_SHARE, PHOTO_NSTAT = OFC_PHOTO_NSTAT;
constexpr int PHOTO_MAX_DIM = OFC_CONSIST_MAX_DIM, PHOTO_MAX_PAIRS = 65535;

// OFC_OK, OFC_EINVAL or OFC_EUNSUPPORTED (message set): what ofc_photo_check documents.  Host only.
int photo_check(int W, int H, int npair, int tau_q, int kappa_q);
// clears stats [npair][5], then one launch: frames u8 [npair+1][H][W], fwd [npair][H][W][2] -> state [npair][H][W], stats,
// warped u16 [npair][H][W] (may be nullptr)
int launch_photo_check(const uint8_t *frames, const float *fwd, int W, int H, int npair, int tau_q, int kappa_q, uint8_t *state,
                       int64_t *stats, uint16_t *warped, hipStream_t s);

}  // namespace ofc
