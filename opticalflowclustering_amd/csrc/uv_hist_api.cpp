// uv_hist_api.cpp -- C ABI of libofc.so, part 5: the histogram of flow vectors (uv_hist.hip) on device and host buffers,
// and its measurement hook.  The streaming ingest's table is stream_api.cpp's.
#include "color_common.h"
#include "host_util.h"

using namespace ofc;

namespace {

size_t table_bytes(int bins) { return sizeof(int64_t) * (3 * (size_t)bins * bins + 1); }

}  // namespace

extern "C" {

int ofc_uv_hist_accum_dev(int device, const float *flow_dev, int64_t n, int bins, float range, int64_t *table_dev)
{
    OFC_REQUIRE(n >= 0, "n = %lld is negative", (long long)n);
    OFC_REQUIRE(table_dev && (flow_dev || n == 0), "null pointer");
    OFC_REQUIRE(((uintptr_t)flow_dev & 7) == 0 && ((uintptr_t)table_dev & 7) == 0, "flow_dev and table_dev must be 8-byte aligned");
    OFC_TRY(uv_hist_check(bins, range));
    OFC_TRY(ensure_device(device));
    if (n == 0) return OFC_OK;
    OFC_TRY(launch_uv_hist(flow_dev, n, bins, range, table_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_uv_hist(int device, const float *flow_host, int64_t n, int bins, float range, int64_t *table_host)
{
    OFC_REQUIRE(n >= 0, "n = %lld is negative", (long long)n);
    OFC_REQUIRE(table_host && (flow_host || n == 0), "null pointer");
    OFC_TRY(uv_hist_check(bins, range));
    OFC_TRY(ensure_device(device));
    DevBuf f, t;
    OFC_TRY(t.alloc(table_bytes(bins)));
    OFC_HIP(hipMemset(t.p, 0, t.bytes));
    if (n) {
        OFC_TRY(f.alloc(sizeof(float) * 2 * (size_t)n));
        OFC_HIP(hipMemcpy(f.p, flow_host, f.bytes, hipMemcpyHostToDevice));
        OFC_TRY(launch_uv_hist(f.as<float>(), n, bins, range, t.as<int64_t>(), nullptr));
    }
    OFC_HIP(hipMemcpy(table_host, t.p, t.bytes, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_bench_uv_hist(int device, const float *flow_dev, int64_t n, int bins, float range, int iters, float *ms_per_launch)
{
    OFC_REQUIRE(flow_dev && ms_per_launch && iters >= 1 && n >= 1, "bad arguments");
    OFC_REQUIRE(((uintptr_t)flow_dev & 7) == 0, "flow_dev must be 8-byte aligned");
    OFC_TRY(uv_hist_check(bins, range));
    OFC_TRY(ensure_device(device));
    DevBuf t;
    OFC_TRY(t.alloc(table_bytes(bins)));
    OFC_HIP(hipMemset(t.p, 0, t.bytes));
    hipStream_t s = nullptr;
    auto launch = [&]() -> int { return launch_uv_hist(flow_dev, n, bins, range, t.as<int64_t>(), s); };
    return time_launches(s, iters, launch, ms_per_launch);
}

}  // extern "C"
