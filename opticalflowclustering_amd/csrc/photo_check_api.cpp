// photo_check_api.cpp -- C ABI of libofc.so, part 10: the photometric check of a flow field against its frames
// (photo_check.hip) on device and host buffers, the host form of its check and its measurement hook.  The stream's side of it
// is in stream_api.cpp.
#include "host_util.h"
#include "photo_check.h"

#include <mutex>

using namespace ofc;

namespace {

// The library's scratch, one per device: the buffers the host-buffer call and the hook work in.
struct PhotoScratch {
    DevBuf frames, fwd, state, stats, warped;
    std::mutex mu;
};

PhotoScratch &scratch_for(int device) { return device_scratch<PhotoScratch>(device); }

}  // namespace

extern "C" {

int ofc_photo_check(int W, int H, int npair, int tau_q, int kappa_q) { return photo_check(W, H, npair, tau_q, kappa_q); }

int ofc_photo_dev(int device, const uint8_t *frames_dev, const float *fwd_dev, int W, int H, int npair, int tau_q, int kappa_q,
                  uint8_t *state_dev, int64_t *stats_dev, uint16_t *warped_dev)
{
    OFC_REQUIRE(frames_dev && fwd_dev && state_dev && stats_dev, "null pointer");
    OFC_REQUIRE((((uintptr_t)fwd_dev | (uintptr_t)stats_dev) & 7) == 0, "fwd_dev and stats_dev must be 8-byte aligned");
    OFC_REQUIRE(((uintptr_t)warped_dev & 1) == 0, "warped_dev must be 2-byte aligned");
    OFC_TRY(photo_check(W, H, npair, tau_q, kappa_q));
    OFC_TRY(ensure_device(device));
    OFC_TRY(launch_photo_check(frames_dev, fwd_dev, W, H, npair, tau_q, kappa_q, state_dev, stats_dev, warped_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_photo(int device, const uint8_t *frames_host, const float *fwd_host, int W, int H, int npair, int tau_q, int kappa_q,
              uint8_t *state_host, int64_t *stats_host, uint16_t *warped_host)
{
    OFC_REQUIRE(frames_host && fwd_host && state_host && stats_host, "null pointer");
    OFC_TRY(photo_check(W, H, npair, tau_q, kappa_q));
    OFC_TRY(ensure_device(device));
    PhotoScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t P = (size_t)W * H, n = P * npair;
    OFC_TRY(reserve(sc.frames, P * (npair + 1)));
    OFC_TRY(reserve(sc.fwd, sizeof(float) * 2 * n));
    OFC_TRY(reserve(sc.state, n));
    OFC_TRY(reserve(sc.stats, sizeof(int64_t) * PHOTO_NSTAT * npair));
    if (warped_host) OFC_TRY(reserve(sc.warped, sizeof(uint16_t) * n));
    OFC_HIP(hipMemcpy(sc.frames.p, frames_host, P * (npair + 1), hipMemcpyHostToDevice));
    OFC_HIP(hipMemcpy(sc.fwd.p, fwd_host, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    OFC_TRY(launch_photo_check(sc.frames.as<uint8_t>(), sc.fwd.as<float>(), W, H, npair, tau_q, kappa_q, sc.state.as<uint8_t>(),
                               sc.stats.as<int64_t>(), warped_host ? sc.warped.as<uint16_t>() : nullptr, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    OFC_HIP(hipMemcpy(state_host, sc.state.p, n, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(stats_host, sc.stats.p, sizeof(int64_t) * PHOTO_NSTAT * npair, hipMemcpyDeviceToHost));
    if (warped_host) OFC_HIP(hipMemcpy(warped_host, sc.warped.p, sizeof(uint16_t) * n, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_bench_photo(int device, const uint8_t *frames_dev, const float *fwd_dev, int W, int H, int npair, int what, int iters,
                    float *ms_per_run)
{
    OFC_REQUIRE(frames_dev && fwd_dev && ms_per_run && iters >= 1 && what >= 0 && what <= 1, "bad arguments");
    OFC_REQUIRE(((uintptr_t)fwd_dev & 7) == 0, "fwd_dev must be 8-byte aligned");
    constexpr int TAU = 2048, KAPPA = 128;
    OFC_TRY(photo_check(W, H, npair, TAU, KAPPA));
    OFC_TRY(ensure_device(device));
    PhotoScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t n = (size_t)W * H * npair;
    OFC_TRY(reserve(sc.state, n));
    OFC_TRY(reserve(sc.stats, sizeof(int64_t) * PHOTO_NSTAT * npair));
    if (what == 1) OFC_TRY(reserve(sc.warped, sizeof(uint16_t) * n));
    hipStream_t s = nullptr;
    EventPair ev;
    OFC_TRY(ev.create());
    double total = 0;
    auto run = [&](bool timed) -> int {
        if (timed) OFC_HIP(hipEventRecord(ev.e0, s));
        OFC_TRY(launch_photo_check(frames_dev, fwd_dev, W, H, npair, TAU, KAPPA, sc.state.as<uint8_t>(), sc.stats.as<int64_t>(),
                                   what == 1 ? sc.warped.as<uint16_t>() : nullptr, s));
        if (timed) {
            OFC_HIP(hipEventRecord(ev.e1, s));
            OFC_TRY(ev.add_elapsed(total));
        }
        return OFC_OK;
    };
    for (int w = 0; w < 2; w++) OFC_TRY(run(false));
    for (int i = 0; i < iters; i++) OFC_TRY(run(true));
    OFC_HIP(hipStreamSynchronize(s));
    *ms_per_run = (float)(total / iters);
    return OFC_OK;
}

}  // extern "C"
