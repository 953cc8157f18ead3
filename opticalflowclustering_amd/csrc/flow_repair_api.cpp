// flow_repair_api.cpp -- C ABI of libofc.so, part 11: the masked median fill and median smoothing of a flow field
// (flow_repair.hip) on device and host buffers, the host form of its check, its tile shape and its measurement hook.  The
// stream's side of it is in stream_api.cpp.
#include "flow_repair.h"
#include "host_util.h"

#include <mutex>

using namespace ofc;

namespace {

// The library's scratch, one per device: the snapshots of a chunk, and the buffers the host-buffer call and the hook work in.
struct RepairBuffers {
    DevBuf a, b, filled;               // the snapshots and the filled map of a chunk (RepairScratch)
    DevBuf flow, state, counts, work;  // the host-buffer call's uploads and its filled map; the hook's output field
    std::mutex mu;
};

RepairBuffers &scratch_for(int device) { return device_scratch<RepairBuffers>(device); }

// the snapshots a launch of this shape needs: b only with more than two sweeps, filled only where the caller keeps none
int ensure_scratch(RepairBuffers &sc, int W, int H, int npair, int sweeps, bool own_filled, RepairScratch &out)
{
    out.chunk = repair_chunk_pairs(W, H, npair);
    OFC_TRY(reserve(sc.a, repair_field_bytes(W, H, out.chunk)));
    if (sweeps > 2) OFC_TRY(reserve(sc.b, repair_field_bytes(W, H, out.chunk)));
    if (own_filled) OFC_TRY(reserve(sc.filled, repair_filled_bytes(W, H, out.chunk)));
    out.a = sc.a.as<float>(), out.b = sc.b.as<float>(), out.filled = sc.filled.as<uint8_t>();
    return OFC_OK;
}

}  // namespace

extern "C" {

int ofc_repair_check(int W, int H, int npair, int keep, int radius, int rounds, int min_count, int smooth)
{
    return repair_check(W, H, npair, keep, radius, rounds, min_count, smooth);
}

void ofc_repair_tile(int radius, int out[2])
{
    (void)radius;                                          // one tile shape serves both radii
    out[0] = REPAIR_TX, out[1] = REPAIR_TY;
}

int ofc_repair_dev(int device, const float *flow_dev, const uint8_t *state_dev, int W, int H, int npair, int keep, int radius,
                   int rounds, int min_count, int smooth, float *out_dev, uint8_t *filled_dev, uint8_t *state_out_dev,
                   int64_t *counts_dev)
{
    OFC_REQUIRE(flow_dev && out_dev && counts_dev, "null pointer");
    OFC_REQUIRE((((uintptr_t)flow_dev | (uintptr_t)out_dev | (uintptr_t)counts_dev) & 7) == 0,
                "flow_dev, out_dev and counts_dev must be 8-byte aligned");
    OFC_REQUIRE(state_dev || !state_out_dev, "state_out_dev without state_dev");
    OFC_TRY(repair_check(W, H, npair, keep, radius, rounds, min_count, smooth));
    const uintptr_t fa = (uintptr_t)flow_dev, oa = (uintptr_t)out_dev, bytes = repair_field_bytes(W, H, npair);
    OFC_REQUIRE(fa == oa || fa + bytes <= oa || oa + bytes <= fa, "out_dev overlaps flow_dev: the same buffer or a disjoint one");
    OFC_TRY(ensure_device(device));
    RepairBuffers &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    RepairScratch rs;
    OFC_TRY(ensure_scratch(sc, W, H, npair, rounds + smooth, state_out_dev && !filled_dev, rs));
    OFC_TRY(launch_repair(flow_dev, state_dev, W, H, npair, keep, radius, rounds, min_count, smooth != 0, out_dev, filled_dev,
                          state_out_dev, counts_dev, rs, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_repair(int device, const float *flow_host, const uint8_t *state_host, int W, int H, int npair, int keep, int radius,
               int rounds, int min_count, int smooth, float *out_host, uint8_t *filled_host, uint8_t *state_out_host,
               int64_t *counts_host)
{
    OFC_REQUIRE(flow_host && out_host && counts_host, "null pointer");
    OFC_REQUIRE(state_host || !state_out_host, "state_out_host without state_host");
    OFC_TRY(repair_check(W, H, npair, keep, radius, rounds, min_count, smooth));
    OFC_TRY(ensure_device(device));
    RepairBuffers &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t n = (size_t)W * H * npair, fbytes = repair_field_bytes(W, H, npair);
    RepairScratch rs;
    OFC_TRY(ensure_scratch(sc, W, H, npair, rounds + smooth, false, rs));
    OFC_TRY(reserve(sc.flow, fbytes));
    OFC_TRY(reserve(sc.work, n));                            // the whole clip's filled map
    OFC_TRY(reserve(sc.counts, sizeof(int64_t) * REPAIR_NCOUNT * npair));
    if (state_host) OFC_TRY(reserve(sc.state, n));
    OFC_HIP(hipMemcpy(sc.flow.p, flow_host, fbytes, hipMemcpyHostToDevice));
    if (state_host) OFC_HIP(hipMemcpy(sc.state.p, state_host, n, hipMemcpyHostToDevice));
    // in place on the uploaded field and, where asked for, on the uploaded state map
    OFC_TRY(launch_repair(sc.flow.as<float>(), state_host ? sc.state.as<uint8_t>() : nullptr, W, H, npair, keep, radius, rounds,
                          min_count, smooth != 0, sc.flow.as<float>(), sc.work.as<uint8_t>(),
                          state_out_host ? sc.state.as<uint8_t>() : nullptr, sc.counts.as<int64_t>(), rs, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    OFC_HIP(hipMemcpy(out_host, sc.flow.p, fbytes, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(counts_host, sc.counts.p, sizeof(int64_t) * REPAIR_NCOUNT * npair, hipMemcpyDeviceToHost));
    if (filled_host) OFC_HIP(hipMemcpy(filled_host, sc.work.p, n, hipMemcpyDeviceToHost));
    if (state_out_host) OFC_HIP(hipMemcpy(state_out_host, sc.state.p, n, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_bench_repair(int device, const float *flow_dev, const uint8_t *state_dev, int W, int H, int npair, int what, int iters,
                     float *ms_per_run)
{
    OFC_REQUIRE(flow_dev && ms_per_run && iters >= 1 && what >= 0 && what <= 2, "bad arguments");
    OFC_REQUIRE(((uintptr_t)flow_dev & 7) == 0, "flow_dev must be 8-byte aligned");
    const int radius = what == 2 ? 2 : 1, rounds = what == 0 ? 1 : 0, smooth = what == 0 ? 0 : 1;
    constexpr int KEEP = 1 << OFC_CONSIST_OK, MIN_COUNT = 1;
    OFC_TRY(repair_check(W, H, npair, KEEP, radius, rounds, MIN_COUNT, smooth));
    OFC_TRY(ensure_device(device));
    RepairBuffers &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    RepairScratch rs;
    OFC_TRY(ensure_scratch(sc, W, H, npair, 1, false, rs));
    OFC_TRY(reserve(sc.work, repair_field_bytes(W, H, npair)));
    OFC_TRY(reserve(sc.counts, sizeof(int64_t) * REPAIR_NCOUNT * npair));
    hipStream_t s = nullptr;
    EventPair ev;
    OFC_TRY(ev.create());
    double total = 0;
    auto run = [&](bool timed) -> int {
        if (timed) OFC_HIP(hipEventRecord(ev.e0, s));
        OFC_TRY(launch_repair(flow_dev, state_dev, W, H, npair, KEEP, radius, rounds, MIN_COUNT, smooth != 0, sc.work.as<float>(), nullptr,
                              nullptr, sc.counts.as<int64_t>(), rs, s));
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
