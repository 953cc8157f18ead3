// fb_check.h -- forward-backward consistency of a flow field (fb_check.hip, fb_check_api.cpp): limits and launchers.
// include/ofc.h has the definition.
#pragma once
#include "ofc_common.h"

#include <algorithm>

namespace ofc {

constexpr int FB_SHARE = OFC_CONSIST_SHARE, FB_NSTATE = OFC_CONSIST_STATES;
constexpr int FB_MAX_DIM = OFC_CONSIST_MAX_DIM, FB_MAX_PAIRS = 65535, FB_MAX_FRAMES = 65536;

struct FbVec {
    int qu, qv;
    bool valid;
};

// shared by the check and the trajectory kernel (trajectories.hip).  The camera and blob blocks' test and quantisation (motion_model.hip, blobs.hip): an invalid vector quantises to 0
__device__ __forceinline__ FbVec fb_quantise(float2 f)
{
    const bool valid = fabsf(f.x) < 1024.f && fabsf(f.y) < 1024.f;     // NaN and inf fail
    FbVec q;
    q.qu = valid ? __double2int_rn((double)f.x * 65536.0) : 0;
    q.qv = valid ? __double2int_rn((double)f.y * 65536.0) : 0;
    q.valid = valid;
    return q;
}

// OFC_OK, OFC_EINVAL or OFC_EUNSUPPORTED (message set): what ofc_consist_check documents.  Host only.
int fb_check(int W, int H, int npair, int64_t alpha_q, int64_t beta_q);
// clears counts [npair][4], then one launch: fwd, bwd [npair][H][W][2] -> state [npair][H][W], counts, resid (may be nullptr)
int launch_fb_check(const float *fwd, const float *bwd, int W, int H, int npair, bool bwd_reversed, int64_t alpha_q, int64_t beta_q,
                    uint8_t *state, int64_t *counts, int32_t *resid, hipStream_t s);
// keys[p] = 255 and w[p] = 0 where bit state[p] of keep is clear; keys and w may each be nullptr
int launch_consist_mask(const uint8_t *state, int64_t n, int keep, uint8_t *keys, float *w, hipStream_t s);
// out[i] = frames[n-1-i], frames of `bytes` bytes each: n device-to-device copies on s
int launch_frames_reverse(const uint8_t *frames, size_t bytes, int n, uint8_t *out, hipStream_t s);

}  // namespace ofc
