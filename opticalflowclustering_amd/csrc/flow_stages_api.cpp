// flow_stages_api.cpp -- C ABI of libofc.so: the single stages of the Farneback flow on host buffers (parity-test hooks), the
// launch-geometry exports and the bench hooks of single kernels.  The engine itself is in flow_engine.cpp.
#include "flow_host.h"
#include "host_util.h"

#include <algorithm>

using namespace ofc;

extern "C" {

// =================================================================================================
// single stages (host buffers; parity-test hooks).  R is pixel-interleaved on the device as well; only M (planar in
// the staged fallback kernels) is converted on the host.
// =================================================================================================
static void interleave5(const float *planar, size_t P, float *inter)
{
    for (int c = 0; c < 5; c++)
        for (size_t i = 0; i < P; i++) inter[i * 5 + c] = planar[c * P + i];
}
static void planarize5(const float *inter, size_t P, float *planar)
{
    for (int c = 0; c < 5; c++)
        for (size_t i = 0; i < P; i++) planar[c * P + i] = inter[i * 5 + c];
}

int ofc_level_image(int device, const uint8_t *gray, int W, int H, const ofc_fb_params *p, int k,
                    float *out, int *w_out, int *h_out)
{
    OFC_REQUIRE(gray && out, "null pointer");
    ofc_fb_params prm;
    if (p) prm = *p; else ofc_fb_default_params(&prm);
    OFC_TRY(check_frame_and_fb_params(prm, W, H));
    OFC_REQUIRE(k >= 0 && k <= pyramid_levels(W, H, prm), "level %d out of range", k);
    OFC_TRY(ensure_device(device));
    LevelGeom g = level_geometry(W, H, prm, k);
    DevBuf src, dst;
    OFC_TRY(src.alloc((size_t)W * H));
    OFC_TRY(dst.alloc(sizeof(float) * g.w * g.h));
    OFC_HIP(hipMemcpy(src.p, gray, (size_t)W * H, hipMemcpyHostToDevice));
    OFC_TRY(launch_level_image(src.as<uint8_t>(), dst.as<float>(), 1, W, H, g, nullptr));
    OFC_HIP(hipMemcpy(out, dst.p, sizeof(float) * g.w * g.h, hipMemcpyDeviceToHost));
    if (w_out) *w_out = g.w;
    if (h_out) *h_out = g.h;
    return OFC_OK;
}

int ofc_pyramid_dec(int device, const uint8_t *frames, int n, int W0, int H0, int levels, int fused,
                    float *out1, float *out2, float *out3, int *fused_levels)
{
    OFC_REQUIRE(frames && out1 && (levels < 2 || out2) && (levels < 3 || out3), "null pointer");
    OFC_REQUIRE(n >= 1 && levels >= 1 && levels <= 3, "n >= 1 frames and 1..3 levels");
    ofc_fb_params prm;
    ofc_fb_default_params(&prm);
    prm.levels = levels;
    OFC_TRY(check_frame_and_fb_params(prm, W0, H0));
    std::vector<LevelGeom> geom;
    for (int k = 0; k <= levels; k++) {
        geom.push_back(level_geometry(W0, H0, prm, k));
        OFC_REQUIRE(geom[k].w >= 1 && geom[k].h >= 1, "level %d of %d x %d is empty", k, W0, H0);
    }
    OFC_TRY(ensure_device(device));
    float *outs[3] = {out1, out2, out3};
    DevBuf src, dst[3];
    OFC_TRY(src.alloc((size_t)n * W0 * H0));
    for (int k = 1; k <= levels; k++) OFC_TRY(dst[k - 1].alloc(sizeof(float) * n * geom[k].w * geom[k].h));
    OFC_HIP(hipMemcpy(src.p, frames, (size_t)n * W0 * H0, hipMemcpyHostToDevice));
    const int L = fused ? pyramid_dec_levels(W0, H0, geom.data(), levels, true) : 0;
    if (L >= 1) {
        float *lv[3] = {dst[0].as<float>(), dst[1].as<float>(), dst[2].as<float>()};
        OFC_TRY(launch_pyramid_dec(src.as<uint8_t>(), lv, n, W0, H0, geom.data(), L, nullptr));
    }
    for (int k = L + 1; k <= levels; k++)     // a level that is no exact decimation, and every deeper one: the per-level launches
        OFC_TRY(launch_level_image(src.as<uint8_t>(), dst[k - 1].as<float>(), n, W0, H0, geom[k], nullptr));
    for (int k = 1; k <= levels; k++)
        OFC_HIP(hipMemcpy(outs[k - 1], dst[k - 1].p, sizeof(float) * n * geom[k].w * geom[k].h, hipMemcpyDeviceToHost));
    if (fused_levels) *fused_levels = L;
    return OFC_OK;
}

int ofc_pyramid_dec_geometry(int W0, int H0, int n, int *out4)
{
    OFC_REQUIRE(out4 && W0 >= 1 && H0 >= 1 && n >= 1, "bad arguments");
    pyramid_dec_plan(W0, H0, n, out4[0], out4[1], out4[2], out4[3]);
    return OFC_OK;
}

int ofc_polyexp(int device, const float *img, int W, int H, int n, double sigma, float *R5)
{
    OFC_REQUIRE(img && R5, "null pointer");
    OFC_REQUIRE(W >= 1 && H >= 1, "bad size");
    OFC_TRY(polyexp_n_check(n));
    OFC_TRY(ensure_device(device));
    const size_t P = (size_t)W * H;
    PolyConsts pc;
    polyexp_setup(n, sigma, pc);
    DevBuf I, R;
    OFC_TRY(I.alloc(sizeof(float) * P));
    OFC_TRY(R.alloc(sizeof(float) * 5 * P));
    OFC_HIP(hipMemcpy(I.p, img, sizeof(float) * P, hipMemcpyHostToDevice));
    OFC_TRY(launch_polyexp(I.as<float>(), R.as<float>(), 1, W, H, pc, 0, nullptr));
    OFC_HIP(hipMemcpy(R5, R.p, sizeof(float) * 5 * P, hipMemcpyDeviceToHost));   // already pixel-interleaved
    return OFC_OK;
}

int ofc_polyexp_u8(int device, const uint8_t *gray, int W, int H, int n, double sigma, float *R5)
{
    OFC_REQUIRE(gray && R5 && W >= 1 && H >= 1, "bad arguments");
    OFC_TRY(polyexp_n_check(n));
    OFC_TRY(ensure_device(device));
    ofc_fb_params prm = {0.5, 0, 15, 3, n, sigma, 0};
    const LevelGeom g = level_geometry(W, H, prm, 0);
    if (!polyexp_u8_ok(W, H, g)) { set_error("fused level-0 expansion needs W >= 4 and H >= 2"); return OFC_EUNSUPPORTED; }
    const size_t P = (size_t)W * H;
    PolyConsts pc;
    polyexp_setup(n, sigma, pc);
    DevBuf I, R;
    OFC_TRY(I.alloc(P));
    OFC_TRY(R.alloc(sizeof(float) * 5 * P));
    OFC_HIP(hipMemcpy(I.p, gray, P, hipMemcpyHostToDevice));
    OFC_TRY(launch_polyexp_u8(I.as<uint8_t>(), R.as<float>(), 1, W, H, pc, nullptr));
    OFC_HIP(hipMemcpy(R5, R.p, sizeof(float) * 5 * P, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_update_matrices(int device, const float *R0, const float *R1, const float *flow, int W, int H,
                        float *M)
{
    OFC_REQUIRE(R0 && R1 && flow && M, "null pointer");
    OFC_REQUIRE(W >= 2 && H >= 2, "bad size");
    OFC_TRY(ensure_device(device));
    const size_t P = (size_t)W * H;
    std::vector<float> tmp(5 * P);
    DevBuf dR, dF, dM;
    OFC_TRY(dR.alloc(sizeof(float) * 10 * P));
    OFC_TRY(dF.alloc(sizeof(float) * 2 * P));
    OFC_TRY(dM.alloc(sizeof(float) * 5 * P));
    OFC_HIP(hipMemcpy(dR.p, R0, sizeof(float) * 5 * P, hipMemcpyHostToDevice));                       // R is pixel-interleaved
    OFC_HIP(hipMemcpy(dR.as<float>() + 5 * P, R1, sizeof(float) * 5 * P, hipMemcpyHostToDevice));
    OFC_HIP(hipMemcpy(dF.p, flow, sizeof(float) * 2 * P, hipMemcpyHostToDevice));
    OFC_TRY(launch_update_matrices(dR.as<float>(), dR.as<float>() + 5 * P, 5 * P, dF.as<float>(),
                                   dM.as<float>(), 1, W, H, nullptr));
    OFC_HIP(hipMemcpy(tmp.data(), dM.p, sizeof(float) * 5 * P, hipMemcpyDeviceToHost));
    interleave5(tmp.data(), P, M);
    return OFC_OK;
}

int ofc_box_solve(int device, const float *M, int W, int H, int winsize, float *flow)
{
    OFC_REQUIRE(M && flow, "null pointer");
    OFC_REQUIRE(W >= 1 && H >= 1, "bad size");
    OFC_TRY(ensure_device(device));
    const size_t P = (size_t)W * H;
    std::vector<float> tmp(5 * P);
    planarize5(M, P, tmp.data());
    DevBuf dM, dF;
    OFC_TRY(dM.alloc(sizeof(float) * 5 * P));
    OFC_TRY(dF.alloc(sizeof(float) * 2 * P));
    OFC_HIP(hipMemcpy(dM.p, tmp.data(), sizeof(float) * 5 * P, hipMemcpyHostToDevice));
    OFC_TRY(launch_box_solve(dM.as<float>(), dF.as<float>(), 1, W, H, winsize, 0, nullptr));
    OFC_HIP(hipMemcpy(flow, dF.p, sizeof(float) * 2 * P, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_flow_resize(int device, const float *flow, int sw, int sh, int dw, int dh, float mul, float *out)
{
    OFC_REQUIRE(flow && out, "null pointer");
    OFC_REQUIRE(sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1, "bad size");
    OFC_TRY(ensure_device(device));
    DevBuf s, d;
    OFC_TRY(s.alloc(sizeof(float) * 2 * sw * sh));
    OFC_TRY(d.alloc(sizeof(float) * 2 * dw * dh));
    OFC_HIP(hipMemcpy(s.p, flow, sizeof(float) * 2 * sw * sh, hipMemcpyHostToDevice));
    OFC_TRY(launch_flow_resize(s.as<float>(), d.as<float>(), 1, sw, sh, dw, dh, mul, nullptr));
    OFC_HIP(hipMemcpy(out, d.p, sizeof(float) * 2 * dw * dh, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_flow_iterate(int device, const float *R0, const float *R1, const float *flow_in, int W, int H,
                     int winsize, int iters, int mode, int rows_per_block, float *flow_out)
{
    OFC_REQUIRE(R0 && R1 && flow_in && flow_out, "null pointer");
    OFC_REQUIRE(W >= 2 && H >= 2 && iters >= 1 && iters <= 64, "bad size / iteration count");
    OFC_TRY(ensure_device(device));
    const size_t P = (size_t)W * H;
    DevBuf dR, dA, dB;
    OFC_TRY(dR.alloc(sizeof(float) * 10 * P));
    OFC_TRY(dA.alloc(sizeof(float) * 2 * P));
    OFC_TRY(dB.alloc(sizeof(float) * 2 * P));
    OFC_HIP(hipMemcpy(dR.p, R0, sizeof(float) * 5 * P, hipMemcpyHostToDevice));
    OFC_HIP(hipMemcpy(dR.as<float>() + 5 * P, R1, sizeof(float) * 5 * P, hipMemcpyHostToDevice));
    OFC_HIP(hipMemcpy(dA.p, flow_in, sizeof(float) * 2 * P, hipMemcpyHostToDevice));
    float *cur = dA.as<float>(), *nxt = dB.as<float>();
    for (int i = 0; i < iters;) {
        const int n = (mode == 1 && iters - i >= 2) ? 2 : 1;
        if (n == 2) OFC_TRY(launch_flow_iter2(dR.as<float>(), 5 * P, cur, nxt, 1, W, H, winsize, nullptr, rows_per_block));
        else if (mode == 2) OFC_TRY(launch_flow_iter_w3(dR.as<float>(), 5 * P, cur, nxt, 1, W, H, winsize, nullptr, rows_per_block));
        else OFC_TRY(launch_flow_iter(dR.as<float>(), 5 * P, cur, nxt, 1, W, H, winsize, nullptr, FlowCoarse(), FlowSums(), rows_per_block));
        std::swap(cur, nxt);
        i += n;
    }
    OFC_HIP(hipMemcpy(flow_out, cur, sizeof(float) * 2 * P, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_flow_launch_geometry(int W, int H, int n_pairs, int winsize, int out[3])
{
    OFC_REQUIRE(out, "null pointer");
    OFC_REQUIRE(W >= 1 && H >= 1 && n_pairs >= 1, "bad size / pair count");
    OFC_REQUIRE(winsize >= 5 && winsize <= OFC_WINSIZE_MAX && (winsize & 1), "winsize must be odd, 5 .. OFC_WINSIZE_MAX");
    out[0] = winsize <= 15 ? flow_iter_grid(W, H, n_pairs, winsize).rows : 0;
    out[1] = winsize >= WINSIZE_WIDE_MIN ? box_wide_rows(winsize) : box_default_rows(W, H, n_pairs);
    out[2] = polyexp_default_rows(W, H, n_pairs + 1);
    return OFC_OK;
}

int ofc_flow_launch_geometry_bidir(int W, int H, int n_pairs, int winsize, int out[3])
{
    OFC_REQUIRE(out, "null pointer");
    OFC_REQUIRE(W >= 1 && H >= 1 && n_pairs >= 1 && n_pairs <= (1 << 20), "bad size / pair count");
    OFC_REQUIRE(winsize >= 5 && winsize <= 15 && (winsize & 1), "winsize must be odd, 5 .. 15 (the fused iteration)");
    const FlowIterGrid g = flow_iter_grid(W, H, 2 * n_pairs, winsize);
    out[0] = g.rows;
    out[1] = g.tiles_x * g.strips;
    out[2] = g.grid;
    return OFC_OK;
}

int ofc_bench_flow_iters(int device, int W, int H, int n_pairs, int reps, int mode, float *ms_out)
{
    OFC_REQUIRE(ms_out && n_pairs >= 1 && reps >= 1, "bad arguments");
    OFC_TRY(ensure_device(device));
    const size_t P = (size_t)W * H;
    const int nf = n_pairs + 1;
    PolyConsts pc;
    polyexp_setup(5, 1.2, pc);
    DevBuf fr, R, fa, fb;
    OFC_TRY(fr.alloc(P * nf));
    OFC_TRY(R.alloc(sizeof(float) * 5 * P * nf));
    OFC_TRY(fa.alloc(sizeof(float) * 2 * P * n_pairs));
    OFC_TRY(fb.alloc(sizeof(float) * 2 * P * n_pairs));
    ScopedStream own;
    OFC_TRY(own.create());
    hipStream_t s = own.s;
    OFC_TRY(ofc_synth_frames_dev(device, fr.as<uint8_t>(), W, H, nf, 0, 0));
    OFC_HIP(hipDeviceSynchronize());
    OFC_TRY(launch_polyexp_u8(fr.as<uint8_t>(), R.as<float>(), nf, W, H, pc, s));
    OFC_HIP(hipMemsetAsync(fb.p, 0, sizeof(float) * 2 * P * n_pairs, s));
    // a realistic flow_in: one iteration from zero flow
    OFC_TRY(launch_flow_iter(R.as<float>(), 5 * P, fb.as<float>(), fa.as<float>(), n_pairs, W, H, 15, s));
    if (mode == 3) {            // diagnostic: the stamped build of k_flow_iter, phase shares printed to stdout
        int grid = 0;
        OFC_TRY(launch_flow_iter_stamped(R.as<float>(), 5 * P, fa.as<float>(), fb.as<float>(), n_pairs, W, H, s, nullptr, &grid));
        DevBuf dbg;
        OFC_TRY(dbg.alloc(sizeof(unsigned long long) * (size_t)grid * 4 * 8));
        OFC_HIP(hipMemsetAsync(dbg.p, 0, dbg.bytes, s));
        OFC_TRY(launch_flow_iter_stamped(R.as<float>(), 5 * P, fa.as<float>(), fb.as<float>(), n_pairs, W, H, s,
                                         dbg.as<unsigned long long>(), &grid));
        OFC_HIP(hipStreamSynchronize(s));
        std::vector<unsigned long long> h((size_t)grid * 4 * 8);
        OFC_HIP(hipMemcpy(h.data(), dbg.p, dbg.bytes, hipMemcpyDeviceToHost));
        double tot[8] = {0, 0, 0, 0, 0, 0, 0, 0}, all = 0;
        for (size_t i = 0; i < h.size(); i++) { tot[i & 7] += (double)h[i]; all += (double)h[i]; }
        static const char *name[8] = {"loop head / flow vectors", "issuing the gathers", "waiting for the operands", "first barrier",
                                      "ring + vertical sums + exchange writes", "second barrier", "horizontal sums + solve + stores",
                                      "matrix arithmetic"};
        printf("k_flow_iter<7,0> stamped build, %dx%d x %d pairs: share of the waves' in-loop cycles\n", W, H, n_pairs);
        for (int i = 0; i < 8; i++) printf("  %-42s %5.1f %%\n", name[i], 100.0 * tot[i] / all);
        fflush(stdout);
        *ms_out = 0.f;
        return OFC_OK;
    }
    auto two = [&]() -> int {
        if (mode == 1) return launch_flow_iter2(R.as<float>(), 5 * P, fa.as<float>(), fb.as<float>(), n_pairs, W, H, 15, s);
        if (mode == 2) {
            OFC_TRY(launch_flow_iter_w3(R.as<float>(), 5 * P, fa.as<float>(), fb.as<float>(), n_pairs, W, H, 15, s));
            return launch_flow_iter_w3(R.as<float>(), 5 * P, fb.as<float>(), fa.as<float>(), n_pairs, W, H, 15, s);
        }
        OFC_TRY(launch_flow_iter(R.as<float>(), 5 * P, fa.as<float>(), fb.as<float>(), n_pairs, W, H, 15, s));
        // second iteration in place of the pair's scratch: fb -> fa would overwrite the input; write a third pass back to fb
        return launch_flow_iter(R.as<float>(), 5 * P, fb.as<float>(), fa.as<float>(), n_pairs, W, H, 15, s);
    };
    return time_launches(s, reps, two, ms_out, 1);          // one warm-up call of the pair
}

// bench hook: polyexp over n_images distinct resident images, HIP events on the launch stream
int ofc_bench_polyexp(int device, int W, int H, int n_images, int iters, int rows_per_block,
                      float *ms_per_launch)
{
    OFC_REQUIRE(ms_per_launch && n_images >= 1 && iters >= 1, "bad arguments");
    OFC_TRY(ensure_device(device));
    const size_t P = (size_t)W * H;
    PolyConsts pc;
    polyexp_setup(5, 1.2, pc);
    DevBuf I, R;
    OFC_TRY(I.alloc(sizeof(float) * P * n_images));
    OFC_TRY(R.alloc(sizeof(float) * 5 * P * n_images));
    {   // non-trivial, image-dependent content (random-ish texture), generated on the host once
        std::vector<float> h(P);
        uint32_t st = 12345u;
        for (int im = 0; im < n_images; im++) {
            for (size_t i = 0; i < P; i++) {
                st = st * 1664525u + 1013904223u;
                h[i] = (float)(st >> 24);
            }
            OFC_HIP(hipMemcpy(I.as<float>() + (size_t)im * P, h.data(), sizeof(float) * P, hipMemcpyHostToDevice));
        }
    }
    ScopedStream own;
    OFC_TRY(own.create());
    hipStream_t s = own.s;
    auto launch = [&]() -> int { return launch_polyexp(I.as<float>(), R.as<float>(), n_images, W, H, pc, rows_per_block, s, true); };
    return time_launches(s, iters, launch, ms_per_launch);
}

int ofc_bench_pyramid_dec(int device, int W, int H, int n_images, int levels, int fused, int iters, float *ms_per_batch)
{
    OFC_REQUIRE(ms_per_batch && n_images >= 1 && iters >= 1 && levels >= 1 && levels <= 3, "bad arguments");
    ofc_fb_params prm;
    ofc_fb_default_params(&prm);
    prm.levels = levels;
    OFC_TRY(check_frame_and_fb_params(prm, W, H));
    std::vector<LevelGeom> geom;
    for (int k = 0; k <= levels; k++) geom.push_back(level_geometry(W, H, prm, k));
    if (fused && pyramid_dec_levels(W, H, geom.data(), levels, true) != levels) {
        set_error("levels 1..%d of %d x %d are not all exact decimations", levels, W, H);
        return OFC_EUNSUPPORTED;
    }
    OFC_TRY(ensure_device(device));
    const size_t P = (size_t)W * H;
    DevBuf src, dst[3];
    OFC_TRY(src.alloc(P * n_images));
    for (int k = 1; k <= levels; k++) OFC_TRY(dst[k - 1].alloc(sizeof(float) * n_images * geom[k].w * geom[k].h));
    {
        std::vector<uint8_t> h(P);
        uint32_t st = 12345u;
        for (int im = 0; im < n_images; im++) {
            for (size_t i = 0; i < P; i++) {
                st = st * 1664525u + 1013904223u;
                h[i] = (uint8_t)(st >> 24);
            }
            OFC_HIP(hipMemcpy(src.as<uint8_t>() + (size_t)im * P, h.data(), P, hipMemcpyHostToDevice));
        }
    }
    ScopedStream own;
    OFC_TRY(own.create());
    hipStream_t s = own.s;
    float *lv[3] = {dst[0].as<float>(), dst[1].as<float>(), dst[2].as<float>()};
    auto launch = [&]() -> int {
        if (fused) return launch_pyramid_dec(src.as<uint8_t>(), lv, n_images, W, H, geom.data(), levels, s);
        for (int k = levels; k >= 1; k--) OFC_TRY(launch_level_image(src.as<uint8_t>(), lv[k - 1], n_images, W, H, geom[k], s));
        return OFC_OK;
    };
    return time_launches(s, iters, launch, ms_per_batch);
}

}  // extern "C"
