// fb_check_api.cpp -- C ABI of libofc.so, part 9: the forward-backward check of a flow field (fb_check.hip) on device and host
// buffers, its mask on key maps and weights, the reversed copy of a clip, the host form of its check and its measurement hook.
#include "fb_check.h"
#include "host_util.h"

#include <mutex>

using namespace ofc;

namespace {

// The library's scratch, one per device: the buffers the host-buffer call and the hook work in.
struct FbScratch {
    DevBuf fwd, bwd, state, counts, resid, keys, w;
    std::mutex mu;
};

FbScratch &scratch_for(int device) { return device_scratch<FbScratch>(device); }

}  // namespace

extern "C" {

int ofc_consist_check(int W, int H, int npair, int64_t alpha_q, int64_t beta_q) { return fb_check(W, H, npair, alpha_q, beta_q); }

int ofc_consist_dev(int device, const float *fwd_dev, const float *bwd_dev, int W, int H, int npair, int bwd_reversed,
                    int64_t alpha_q, int64_t beta_q, uint8_t *state_dev, int64_t *counts_dev, int32_t *resid_dev)
{
    OFC_REQUIRE(fwd_dev && bwd_dev && state_dev && counts_dev, "null pointer");
    OFC_REQUIRE((((uintptr_t)fwd_dev | (uintptr_t)bwd_dev | (uintptr_t)counts_dev | (uintptr_t)resid_dev) & 7) == 0,
                "fwd_dev, bwd_dev, counts_dev and resid_dev must be 8-byte aligned");
    OFC_REQUIRE(bwd_reversed == 0 || bwd_reversed == 1, "bwd_reversed = %d: 0 or 1", bwd_reversed);
    OFC_TRY(fb_check(W, H, npair, alpha_q, beta_q));
    OFC_TRY(ensure_device(device));
    OFC_TRY(launch_fb_check(fwd_dev, bwd_dev, W, H, npair, bwd_reversed != 0, alpha_q, beta_q, state_dev, counts_dev, resid_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_consist(int device, const float *fwd_host, const float *bwd_host, int W, int H, int npair, int bwd_reversed,
                int64_t alpha_q, int64_t beta_q, uint8_t *state_host, int64_t *counts_host, int32_t *resid_host)
{
    OFC_REQUIRE(fwd_host && bwd_host && state_host && counts_host, "null pointer");
    OFC_REQUIRE(bwd_reversed == 0 || bwd_reversed == 1, "bwd_reversed = %d: 0 or 1", bwd_reversed);
    OFC_TRY(fb_check(W, H, npair, alpha_q, beta_q));
    OFC_TRY(ensure_device(device));
    FbScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t n = (size_t)W * H * npair;
    OFC_TRY(reserve(sc.fwd, sizeof(float) * 2 * n));
    OFC_TRY(reserve(sc.bwd, sizeof(float) * 2 * n));
    OFC_TRY(reserve(sc.state, n));
    OFC_TRY(reserve(sc.counts, sizeof(int64_t) * FB_NSTATE * npair));
    if (resid_host) OFC_TRY(reserve(sc.resid, sizeof(int32_t) * 2 * n));
    OFC_HIP(hipMemcpy(sc.fwd.p, fwd_host, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    OFC_HIP(hipMemcpy(sc.bwd.p, bwd_host, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    OFC_TRY(launch_fb_check(sc.fwd.as<float>(), sc.bwd.as<float>(), W, H, npair, bwd_reversed != 0, alpha_q, beta_q,
                            sc.state.as<uint8_t>(), sc.counts.as<int64_t>(), resid_host ? sc.resid.as<int32_t>() : nullptr, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    OFC_HIP(hipMemcpy(state_host, sc.state.p, n, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(counts_host, sc.counts.p, sizeof(int64_t) * FB_NSTATE * npair, hipMemcpyDeviceToHost));
    if (resid_host) OFC_HIP(hipMemcpy(resid_host, sc.resid.p, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_consist_mask_dev(int device, const uint8_t *state_dev, int64_t n, int keep, uint8_t *keys_dev, float *w_dev)
{
    OFC_REQUIRE(state_dev, "null pointer");
    OFC_REQUIRE(n >= 1, "n = %lld: at least 1", (long long)n);
    OFC_REQUIRE(keep >= 0 && keep < (1 << FB_NSTATE), "keep = %d: a set of the four states, 0 .. 15", keep);
    OFC_REQUIRE(((uintptr_t)w_dev & 3) == 0, "w_dev must be 4-byte aligned");
    OFC_TRY(ensure_device(device));
    OFC_TRY(launch_consist_mask(state_dev, n, keep, keys_dev, w_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_frames_reverse_dev(int device, const uint8_t *frames_dev, int W, int H, int n_frames, uint8_t *out_dev)
{
    OFC_REQUIRE(frames_dev && out_dev, "null pointer");
    OFC_REQUIRE(W >= 1 && H >= 1, "W = %d, H = %d: at least 1", W, H);
    OFC_REQUIRE(n_frames >= 1 && n_frames <= FB_MAX_FRAMES, "n_frames = %d: 1 .. %d", n_frames, FB_MAX_FRAMES);
    const size_t bytes = (size_t)W * H, all = bytes * (size_t)n_frames;
    OFC_REQUIRE(frames_dev + all <= out_dev || out_dev + all <= frames_dev, "frames_dev and out_dev overlap");
    OFC_TRY(ensure_device(device));
    OFC_TRY(launch_frames_reverse(frames_dev, bytes, n_frames, out_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_bench_consist(int device, const float *fwd_dev, const float *bwd_dev, int W, int H, int npair, int what, int iters,
                      float *ms_per_run)
{
    OFC_REQUIRE(fwd_dev && bwd_dev && ms_per_run && iters >= 1 && what >= 0 && what <= 2, "bad arguments");
    OFC_REQUIRE((((uintptr_t)fwd_dev | (uintptr_t)bwd_dev) & 7) == 0, "fwd_dev and bwd_dev must be 8-byte aligned");
    constexpr int64_t ALPHA = 655, BETA = (int64_t)1 << 31;
    OFC_TRY(fb_check(W, H, npair, ALPHA, BETA));
    OFC_TRY(ensure_device(device));
    FbScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t n = (size_t)W * H * npair;
    OFC_TRY(reserve(sc.state, n));
    OFC_TRY(reserve(sc.counts, sizeof(int64_t) * FB_NSTATE * npair));
    if (what == 1) OFC_TRY(reserve(sc.resid, sizeof(int32_t) * 2 * n));
    if (what == 2) {
        OFC_TRY(reserve(sc.keys, n));
        OFC_TRY(reserve(sc.w, sizeof(float) * n));
    }
    hipStream_t s = nullptr;
    uint8_t *state = sc.state.as<uint8_t>();
    int64_t *counts = sc.counts.as<int64_t>();
    if (what == 2) {
        OFC_HIP(hipMemsetAsync(sc.keys.p, 0, n, s));
        OFC_HIP(hipMemsetAsync(sc.w.p, 0, sizeof(float) * n, s));
        OFC_TRY(launch_fb_check(fwd_dev, bwd_dev, W, H, npair, false, ALPHA, BETA, state, counts, nullptr, s));
    }
    EventPair ev;
    OFC_TRY(ev.create());
    double total = 0;
    auto run = [&](bool timed) -> int {
        if (timed) OFC_HIP(hipEventRecord(ev.e0, s));
        if (what == 2)
            OFC_TRY(launch_consist_mask(state, (int64_t)n, 1 << OFC_CONSIST_OK, sc.keys.as<uint8_t>(), sc.w.as<float>(), s));
        else
            OFC_TRY(launch_fb_check(fwd_dev, bwd_dev, W, H, npair, false, ALPHA, BETA, state, counts,
                                    what == 1 ? sc.resid.as<int32_t>() : nullptr, s));
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
