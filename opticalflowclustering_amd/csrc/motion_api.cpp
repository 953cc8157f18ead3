// motion_api.cpp -- C ABI of libofc.so, part 6: per-pair camera motion (motion_model.hip) on device and host buffers, the
// host forms of its checks and its solve, and its measurement hook.  The streaming ingest's camera is stream_api.cpp's.
#include "host_util.h"
#include "motion_model.h"

using namespace ofc;

namespace {

// rec, partials and history of a fit over npair pairs, on the device
struct FitBufs {
    DevBuf rec, partial, hm, hq;
    int alloc(int W, int H, int npair, int T, bool history)
    {
        OFC_TRY(rec.alloc(sizeof(MotionRec) * npair));
        OFC_TRY(partial.alloc(sizeof(int64_t) * MOTION_NMOM * (size_t)motion_groups(W, H, npair) * npair));
        if (history) {
            OFC_TRY(hm.alloc(sizeof(double) * 6 * (size_t)(T + 1) * npair));
            OFC_TRY(hq.alloc(sizeof(int64_t) * MOTION_NMOM * (size_t)(T + 1) * npair));
        }
        return OFC_OK;
    }
};

int check_pairs(int npair)
{
    OFC_REQUIRE(npair >= 1, "npair = %d: at least one pair", npair);
    if (npair > MOTION_MAX_PAIRS) {
        set_error("npair = %d: at most %d pairs per call", npair, MOTION_MAX_PAIRS);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

int check_field(const float *flow_dev, int npair)
{
    OFC_REQUIRE(flow_dev, "null pointer");
    OFC_REQUIRE(((uintptr_t)flow_dev & 7) == 0, "flow_dev must be 8-byte aligned");
    return check_pairs(npair);
}

int fit_dev(const float *flow_dev, int W, int H, int npair, int kind, const double *thresholds, int T, FitBufs &b,
            double *models_host, int *status_host, double *history_models, int64_t *history_moments)
{
    const bool history = history_models || history_moments;
    OFC_TRY(b.alloc(W, H, npair, T, history));
    OFC_TRY(motion_fit_async(flow_dev, W, H, npair, kind, thresholds, T, b.rec.as<MotionRec>(), b.partial.as<int64_t>(),
                             b.hm.as<double>(), b.hq.as<int64_t>(), nullptr));
    std::vector<MotionRec> rec(npair);
    OFC_HIP(hipMemcpy(rec.data(), b.rec.p, b.rec.bytes, hipMemcpyDeviceToHost));
    for (int i = 0; i < npair; i++) {
        if (models_host) memcpy(models_host + 6 * (size_t)i, rec[i].p, sizeof(double) * 6);
        if (status_host) status_host[i] = rec[i].status;
    }
    if (history_models) OFC_HIP(hipMemcpy(history_models, b.hm.p, b.hm.bytes, hipMemcpyDeviceToHost));
    if (history_moments) OFC_HIP(hipMemcpy(history_moments, b.hq.p, b.hq.bytes, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int upload_models(const double *models, const double *c, int npair, DevBuf &rec)
{
    std::vector<MotionRec> r(npair);
    memset(r.data(), 0, sizeof(MotionRec) * npair);
    for (int i = 0; i < npair; i++) {
        if (!models) continue;
        memcpy(r[i].p, models + 6 * (size_t)i, sizeof(double) * 6);
        for (int k = 0; k < 6; k++) OFC_REQUIRE(std::isfinite(r[i].p[k]), "model %d of pair %d is not finite", k, i);
        if (c) {
            OFC_REQUIRE(std::isfinite(c[i]) && c[i] > 0.0, "threshold %g of pair %d is not finite and positive", c[i], i);
            r[i].c2 = c[i] * c[i];
            r[i].use = 1;
        }
    }
    OFC_TRY(rec.alloc(sizeof(MotionRec) * npair));
    OFC_HIP(hipMemcpy(rec.p, r.data(), rec.bytes, hipMemcpyHostToDevice));
    return OFC_OK;
}

}  // namespace

extern "C" {

int ofc_motion_check(int W, int H, int kind) { return motion_check(W, H, kind); }

int ofc_motion_launch_geometry(int W, int H, int npair, int out[4])
{
    OFC_REQUIRE(out, "null pointer");
    OFC_TRY(check_pairs(npair));
    OFC_TRY(motion_check(W, H, 1));
    motion_launch_geometry(W, H, npair, out);
    return OFC_OK;
}

int ofc_motion_solve(const int64_t m[13], int kind, double p[6], int *status)
{
    OFC_REQUIRE(m && p && status, "null pointer");
    OFC_REQUIRE(kind == 1 || kind == 2, "kind = %d is neither 1 (translation) nor 2 (affine)", kind);
    for (int k = 0; k < 6; k++) p[k] = 0.0;
    *status = motion_solve(m, kind, p) ? 0 : 1;
    return OFC_OK;
}

int ofc_motion_moments_dev(int device, const float *flow_dev, int W, int H, int npair, const double *models, const double *c,
                           int64_t *moments_host)
{
    OFC_TRY(check_field(flow_dev, npair));
    OFC_REQUIRE(moments_host && (!models || c), "null pointer");
    OFC_TRY(motion_check(W, H, 1));
    OFC_TRY(ensure_device(device));
    DevBuf rec, partial;
    OFC_TRY(upload_models(models, c, npair, rec));
    const int groups = motion_groups(W, H, npair);
    OFC_TRY(partial.alloc(sizeof(int64_t) * MOTION_NMOM * (size_t)groups * npair));
    OFC_TRY(launch_motion_moments(flow_dev, W, H, npair, rec.as<MotionRec>(), partial.as<int64_t>(), true, nullptr));
    std::vector<int64_t> part((size_t)MOTION_NMOM * groups * npair);
    OFC_HIP(hipMemcpy(part.data(), partial.p, partial.bytes, hipMemcpyDeviceToHost));
    for (int i = 0; i < npair; i++)
        for (int k = 0; k < MOTION_NMOM; k++) {
            int64_t t = 0;
            for (int g = 0; g < groups; g++) t += part[((size_t)i * groups + g) * MOTION_NMOM + k];
            moments_host[(size_t)i * MOTION_NMOM + k] = t;
        }
    return OFC_OK;
}

int ofc_motion_fit_dev(int device, const float *flow_dev, int W, int H, int npair, int kind, const double *thresholds, int T,
                       double *models_host, int *status_host, double *history_models, int64_t *history_moments)
{
    OFC_TRY(check_field(flow_dev, npair));
    OFC_REQUIRE(models_host && status_host, "null pointer");
    OFC_TRY(motion_fit_check(W, H, kind, thresholds, T));
    OFC_TRY(ensure_device(device));
    FitBufs b;
    return fit_dev(flow_dev, W, H, npair, kind, thresholds, T, b, models_host, status_host, history_models, history_moments);
}

int ofc_motion_subtract_dev(int device, const float *flow_dev, int W, int H, int npair, const double *models_host,
                            float *dst_dev)
{
    OFC_TRY(check_field(flow_dev, npair));
    OFC_REQUIRE(models_host && dst_dev, "null pointer");
    OFC_REQUIRE(((uintptr_t)dst_dev & 7) == 0, "dst_dev must be 8-byte aligned");
    OFC_TRY(motion_check(W, H, 1));
    OFC_TRY(ensure_device(device));
    DevBuf rec;
    OFC_TRY(upload_models(models_host, nullptr, npair, rec));
    OFC_TRY(launch_motion_subtract(flow_dev, dst_dev, W, H, npair, rec.as<MotionRec>(), nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_motion_fit(int device, const float *flow_host, int W, int H, int npair, int kind, const double *thresholds, int T,
                   double *models_host, int *status_host, double *history_models, int64_t *history_moments)
{
    OFC_REQUIRE(flow_host && models_host && status_host, "null pointer");
    OFC_TRY(motion_fit_check(W, H, kind, thresholds, T));
    OFC_TRY(check_pairs(npair));
    OFC_TRY(ensure_device(device));
    DevBuf f;
    OFC_TRY(f.alloc(sizeof(float) * 2 * (size_t)W * H * npair));
    OFC_HIP(hipMemcpy(f.p, flow_host, f.bytes, hipMemcpyHostToDevice));
    FitBufs b;
    return fit_dev(f.as<float>(), W, H, npair, kind, thresholds, T, b, models_host, status_host, history_models,
                   history_moments);
}

int ofc_motion_compensate(int device, const float *flow_host, int W, int H, int npair, int kind, const double *thresholds,
                          int T, float *residual_host, double *models_host, int *status_host, double *history_models,
                          int64_t *history_moments)
{
    OFC_REQUIRE(flow_host && residual_host && models_host && status_host, "null pointer");
    OFC_TRY(motion_fit_check(W, H, kind, thresholds, T));
    OFC_TRY(check_pairs(npair));
    OFC_TRY(ensure_device(device));
    DevBuf f;
    OFC_TRY(f.alloc(sizeof(float) * 2 * (size_t)W * H * npair));
    OFC_HIP(hipMemcpy(f.p, flow_host, f.bytes, hipMemcpyHostToDevice));
    FitBufs b;
    OFC_TRY(fit_dev(f.as<float>(), W, H, npair, kind, thresholds, T, b, models_host, status_host, history_models,
                    history_moments));
    OFC_TRY(launch_motion_subtract(f.as<float>(), f.as<float>(), W, H, npair, b.rec.as<MotionRec>(), nullptr));
    OFC_HIP(hipMemcpy(residual_host, f.p, f.bytes, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_bench_motion(int device, const float *flow_dev, int W, int H, int npair, int what, int iters, float *ms_per_launch)
{
    OFC_REQUIRE(ms_per_launch && iters >= 1 && what >= 0 && what <= 4, "bad arguments");
    OFC_TRY(check_field(flow_dev, npair));
    OFC_TRY(motion_check(W, H, 2));
    OFC_TRY(ensure_device(device));
    static const double thr[3] = {4.0, 2.0, 1.0};
    FitBufs b;
    DevBuf dst;
    OFC_TRY(b.alloc(W, H, npair, 3, false));
    if (what == 3) OFC_TRY(dst.alloc(sizeof(float) * 2 * (size_t)W * H * npair));
    hipStream_t s = nullptr;
    // the record every timed launch runs under: round 0's affine fit, selecting within 4 px
    OFC_TRY(motion_fit_async(flow_dev, W, H, npair, 2, thr, 0, b.rec.as<MotionRec>(), b.partial.as<int64_t>(), nullptr, nullptr, s));
    const int groups = motion_groups(W, H, npair);
    auto run = [&]() -> int {
        MotionRec *rec = b.rec.as<MotionRec>();
        int64_t *part = b.partial.as<int64_t>();
        switch (what) {
        case 0: return launch_motion_moments(flow_dev, W, H, npair, rec, part, true, s);
        case 1: return launch_motion_moments(flow_dev, W, H, npair, rec, part, false, s);
        case 2: return launch_motion_solve(part, groups, npair, 2, 1, 4.0, rec, nullptr, nullptr, s);
        case 3: return launch_motion_subtract(flow_dev, dst.as<float>(), W, H, npair, rec, s);
        default: return motion_fit_async(flow_dev, W, H, npair, 2, thr, 3, rec, part, nullptr, nullptr, s);
        }
    };
    return time_launches(s, iters, run, ms_per_launch);
}

}  // extern "C"
