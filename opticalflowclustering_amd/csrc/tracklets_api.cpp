// tracklets_api.cpp -- C ABI of libofc.so, part 13: dense trajectories with reseeding (tracklets.hip) on device and host
// buffers, the host form of its check, and its measurement hook.  Everything a call allocates is its own and is freed on
// every way out of it (DevBuf releases in its destructor).
#include "tracklets.h"
#include "host_util.h"

using namespace ofc;

namespace {

int alloc_scratch(int W, int H, int npair, int cell, DevBuf &buf, TrkScratch &sc)
{
    const TrkGrid g = trk_grid(W, H, cell);
    OFC_TRY(buf.alloc(trk_scratch_bytes(g, npair)));
    trk_scratch_carve(buf.p, g, npair, sc);
    return OFC_OK;
}

}  // namespace

extern "C" {

int ofc_tracklets_check(int W, int H, int npair, int cell, int max_len, int64_t max_tracks, int keep)
{
    return trk_check(W, H, npair, cell, max_len, max_tracks, keep);
}

int ofc_tracklets_dev(int device, const float *flow_dev, const uint8_t *state_dev, int W, int H, int npair, int cell, int max_len,
                      int64_t max_tracks, int keep, int32_t *pos_dev, int32_t *birth_dev, int32_t *len_dev, uint8_t *why_dev,
                      int32_t *frames_dev)
{
    OFC_REQUIRE(flow_dev && pos_dev && birth_dev && len_dev && why_dev && frames_dev, "null pointer");
    OFC_REQUIRE((((uintptr_t)flow_dev | (uintptr_t)pos_dev) & 7) == 0, "flow_dev and pos_dev must be 8-byte aligned");
    OFC_REQUIRE((((uintptr_t)birth_dev | (uintptr_t)len_dev | (uintptr_t)frames_dev) & 3) == 0,
                "birth_dev, len_dev and frames_dev must be 4-byte aligned");
    OFC_TRY(trk_check(W, H, npair, cell, max_len, max_tracks, keep));
    OFC_TRY(ensure_device(device));
    DevBuf buf;
    TrkScratch sc;
    OFC_TRY(alloc_scratch(W, H, npair, cell, buf, sc));
    OFC_TRY(launch_tracklets(flow_dev, state_dev, W, H, npair, cell, max_len, max_tracks, keep, pos_dev, birth_dev, len_dev, why_dev,
                             frames_dev, sc, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_tracklets(int device, const float *flow_host, const uint8_t *state_host, int W, int H, int npair, int cell, int max_len,
                  int64_t max_tracks, int keep, int32_t *pos_host, int32_t *birth_host, int32_t *len_host, uint8_t *why_host,
                  int32_t *frames_host)
{
    OFC_REQUIRE(flow_host && pos_host && birth_host && len_host && why_host && frames_host, "null pointer");
    OFC_TRY(trk_check(W, H, npair, cell, max_len, max_tracks, keep));
    OFC_TRY(ensure_device(device));
    const size_t n = (size_t)W * H * npair, M = (size_t)max_tracks, rows = sizeof(int32_t) * 2 * M * ((size_t)max_len + 1);
    DevBuf flow, state, pos, birth, len, why, frames, buf;
    TrkScratch sc;
    OFC_TRY(flow.alloc(sizeof(float) * 2 * n));
    if (state_host) OFC_TRY(state.alloc(n));
    OFC_TRY(pos.alloc(rows));
    OFC_TRY(birth.alloc(sizeof(int32_t) * M));
    OFC_TRY(len.alloc(sizeof(int32_t) * M));
    OFC_TRY(why.alloc(M));
    OFC_TRY(frames.alloc(sizeof(int32_t) * 3 * (size_t)npair));
    OFC_TRY(alloc_scratch(W, H, npair, cell, buf, sc));
    OFC_HIP(hipMemcpy(flow.p, flow_host, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    if (state_host) OFC_HIP(hipMemcpy(state.p, state_host, n, hipMemcpyHostToDevice));
    OFC_TRY(launch_tracklets(flow.as<float>(), state_host ? state.as<uint8_t>() : nullptr, W, H, npair, cell, max_len, max_tracks, keep,
                             pos.as<int32_t>(), birth.as<int32_t>(), len.as<int32_t>(), why.as<uint8_t>(), frames.as<int32_t>(), sc,
                             nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    OFC_HIP(hipMemcpy(pos_host, pos.p, rows, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(birth_host, birth.p, sizeof(int32_t) * M, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(len_host, len.p, sizeof(int32_t) * M, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(why_host, why.p, M, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(frames_host, frames.p, sizeof(int32_t) * 3 * (size_t)npair, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_bench_tracklets(int device, const float *flow_dev, int W, int H, int npair, int cell, int max_len, int64_t max_tracks, int iters,
                        float *ms_per_run)
{
    OFC_REQUIRE(flow_dev && ms_per_run && iters >= 1, "bad arguments");
    OFC_REQUIRE(((uintptr_t)flow_dev & 7) == 0, "flow_dev must be 8-byte aligned");
    OFC_TRY(trk_check(W, H, npair, cell, max_len, max_tracks, 0));
    OFC_TRY(ensure_device(device));
    const size_t M = (size_t)max_tracks;
    DevBuf pos, birth, len, why, frames, buf;
    TrkScratch sc;
    OFC_TRY(pos.alloc(sizeof(int32_t) * 2 * M * ((size_t)max_len + 1)));
    OFC_TRY(birth.alloc(sizeof(int32_t) * M));
    OFC_TRY(len.alloc(sizeof(int32_t) * M));
    OFC_TRY(why.alloc(M));
    OFC_TRY(frames.alloc(sizeof(int32_t) * 3 * (size_t)npair));
    OFC_TRY(alloc_scratch(W, H, npair, cell, buf, sc));
    hipStream_t s = nullptr;
    auto run = [&]() -> int {
        return launch_tracklets(flow_dev, nullptr, W, H, npair, cell, max_len, max_tracks, 0, pos.as<int32_t>(), birth.as<int32_t>(),
                                len.as<int32_t>(), why.as<uint8_t>(), frames.as<int32_t>(), sc, s);
    };
    const int rc = time_launches(s, iters, run, ms_per_run);
    (void)hipStreamSynchronize(s);                                     // nothing is freed under a running kernel
    return rc;
}

}  // extern "C"
