// trajectories_api.cpp -- C ABI of libofc.so, part 12: points followed through a clip's flow fields (trajectories.hip) on
// device and host buffers, the host form of its check and of its launch model, and its measurement hook.
#include "trajectories.h"
#include "host_util.h"

#include <mutex>

using namespace ofc;

namespace {

// The library's scratch, one per device: the buffers the host-buffer call and the hook work in.
struct TrajScratch {
    DevBuf flow, state, seeds, pos, len, why;
    std::mutex mu;
};

TrajScratch &scratch_for(int device) { return device_scratch<TrajScratch>(device); }

int check_buffers(const int32_t *seeds, int64_t P, int npair, const int32_t *pos)
{
    const int32_t *end = pos + 2 * (size_t)P * ((size_t)npair + 1);
    OFC_REQUIRE(seeds == pos || seeds + 2 * (size_t)P <= pos || end <= seeds, "seeds overlap pos without being its row 0");
    return OFC_OK;
}

}  // namespace

extern "C" {

int ofc_traj_check(int W, int H, int npair, int64_t P, int keep, int pairs_per_launch)
{
    return traj_check(W, H, npair, P, keep, pairs_per_launch);
}

int ofc_traj_launch_geometry(int W, int H, int npair, int64_t P, int out[4])
{
    OFC_REQUIRE(out, "null pointer");
    OFC_TRY(traj_check(W, H, npair, P, 0, 0));
    out[0] = traj_chunk_pairs(npair, P, 0);
    out[1] = (int)cdiv64(P, TRAJ_THREADS);
    out[2] = cdiv(npair, out[0]);
    out[3] = TRAJ_THREADS;
    return OFC_OK;
}

int ofc_traj_dev(int device, const float *flow_dev, const uint8_t *state_dev, int W, int H, int npair, const int32_t *seeds_dev,
                 int64_t P, int keep, int pairs_per_launch, int32_t *pos_dev, int32_t *len_dev, uint8_t *why_dev)
{
    OFC_REQUIRE(flow_dev && seeds_dev && pos_dev && len_dev && why_dev, "null pointer");
    OFC_REQUIRE((((uintptr_t)flow_dev | (uintptr_t)seeds_dev | (uintptr_t)pos_dev) & 7) == 0,
                "flow_dev, seeds_dev and pos_dev must be 8-byte aligned");
    OFC_REQUIRE(((uintptr_t)len_dev & 3) == 0, "len_dev must be 4-byte aligned");
    OFC_TRY(traj_check(W, H, npair, P, keep, pairs_per_launch));
    OFC_TRY(check_buffers(seeds_dev, P, npair, pos_dev));
    OFC_TRY(ensure_device(device));
    OFC_TRY(launch_traj(flow_dev, state_dev, W, H, npair, seeds_dev, P, keep, pairs_per_launch, pos_dev, len_dev, why_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_traj(int device, const float *flow_host, const uint8_t *state_host, int W, int H, int npair, const int32_t *seeds_host,
             int64_t P, int keep, int pairs_per_launch, int32_t *pos_host, int32_t *len_host, uint8_t *why_host)
{
    OFC_REQUIRE(flow_host && seeds_host && pos_host && len_host && why_host, "null pointer");
    OFC_TRY(traj_check(W, H, npair, P, keep, pairs_per_launch));
    OFC_TRY(ensure_device(device));
    TrajScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t n = (size_t)W * H * npair, np = (size_t)P, rows = sizeof(int32_t) * 2 * np * ((size_t)npair + 1);
    OFC_TRY(reserve(sc.flow, sizeof(float) * 2 * n));
    if (state_host) OFC_TRY(reserve(sc.state, n));
    OFC_TRY(reserve(sc.pos, rows));
    OFC_TRY(reserve(sc.len, sizeof(int32_t) * np));
    OFC_TRY(reserve(sc.why, np));
    OFC_HIP(hipMemcpy(sc.flow.p, flow_host, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    if (state_host) OFC_HIP(hipMemcpy(sc.state.p, state_host, n, hipMemcpyHostToDevice));
    OFC_HIP(hipMemcpy(sc.pos.p, seeds_host, sizeof(int32_t) * 2 * np, hipMemcpyHostToDevice));      // the seeds are row 0
    OFC_TRY(launch_traj(sc.flow.as<float>(), state_host ? sc.state.as<uint8_t>() : nullptr, W, H, npair, sc.pos.as<int32_t>(), P, keep,
                        pairs_per_launch, sc.pos.as<int32_t>(), sc.len.as<int32_t>(), sc.why.as<uint8_t>(), nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    OFC_HIP(hipMemcpy(pos_host, sc.pos.p, rows, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(len_host, sc.len.p, sizeof(int32_t) * np, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(why_host, sc.why.p, np, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_bench_traj(int device, const float *flow_dev, int W, int H, int npair, const int32_t *seeds_dev, int64_t P,
                   int pairs_per_launch, int iters, float *ms_per_run)
{
    OFC_REQUIRE(flow_dev && seeds_dev && ms_per_run && iters >= 1, "bad arguments");
    OFC_REQUIRE((((uintptr_t)flow_dev | (uintptr_t)seeds_dev) & 7) == 0, "flow_dev and seeds_dev must be 8-byte aligned");
    OFC_TRY(traj_check(W, H, npair, P, 0, pairs_per_launch));
    OFC_TRY(ensure_device(device));
    TrajScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t np = (size_t)P;
    OFC_TRY(reserve(sc.pos, sizeof(int32_t) * 2 * np * ((size_t)npair + 1)));
    OFC_TRY(reserve(sc.len, sizeof(int32_t) * np));
    OFC_TRY(reserve(sc.why, np));
    hipStream_t s = nullptr;
    auto run = [&]() -> int {
        return launch_traj(flow_dev, nullptr, W, H, npair, seeds_dev, P, 0, pairs_per_launch, sc.pos.as<int32_t>(), sc.len.as<int32_t>(),
                           sc.why.as<uint8_t>(), s);
    };
    OFC_TRY(time_launches(s, iters, run, ms_per_run));
    OFC_HIP(hipStreamSynchronize(s));
    return OFC_OK;
}

}  // extern "C"
