// ofc_api.cpp -- C ABI of libofc.so, part 1: runtime plumbing and the Farneback flow engine.
// Declared in include/ofc.h (which cites the reference call each entry point replaces).
#include "color_common.h"
#include "fb_check.h"
#include "host_util.h"
#include "lloyd_common.h"

#include <cfloat>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>

namespace ofc {

static thread_local std::string g_err;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

int ensure_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no usable GPU (hipGetDeviceCount: %s, count %d); libofc has no CPU fallback",
                  hipGetErrorString(e), n);
        return OFC_ENODEV;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (have %d)", device, n);
        return OFC_ENODEV;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) {
        set_error("hipSetDevice(%d): %s", device, hipGetErrorString(e));
        return OFC_ENODEV;
    }
    return OFC_OK;
}

// ---- geometry & constants (host) ----
int pyramid_levels(int W, int H, const ofc_fb_params &p)
{
    const int min_size = 32;
    int k;
    double scale = 1;
    for (k = 0; k < p.levels; k++) {
        scale *= p.pyr_scale;
        if (W * scale < min_size || H * scale < min_size) break;
    }
    return k;
}

LevelGeom level_geometry(int W, int H, const ofc_fb_params &p, int k)
{
    double scale = 1;
    for (int i = 0; i < k; i++) scale *= p.pyr_scale;
    LevelGeom g;
    g.sigma = (1. / scale - 1) * 0.5;
    int sz = (int)std::nearbyint(g.sigma * 5) | 1;   // cvRound: half to even
    g.ksize = sz < 3 ? 3 : sz;
    g.w = (int)std::nearbyint(W * scale);
    g.h = (int)std::nearbyint(H * scale);
    return g;
}

void gaussian_kernel(int n, double sigma, float *k)
{
    static const float tab[4][7] = {{1.f},
                                    {0.25f, 0.5f, 0.25f},
                                    {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                                    {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
    const float *fixed = (n % 2 == 1 && n <= 7 && sigma <= 0) ? tab[n >> 1] : nullptr;
    double sigmaX = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    double scale2X = -0.5 / (sigmaX * sigmaX), sum = 0;
    for (int i = 0; i < n; i++) {
        double x = i - (n - 1) * 0.5;
        double t = fixed ? (double)fixed[i] : std::exp(scale2X * x * x);
        k[i] = (float)t;
        sum += k[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) k[i] = (float)(k[i] * sum);
}

void polyexp_setup(int n, double sigma, PolyConsts &c)
{
    if (sigma < FLT_EPSILON) sigma = n * 0.3;
    std::vector<float> gf(2 * n + 1);
    double s = 0;
    for (int x = -n; x <= n; x++) {
        gf[x + n] = (float)std::exp(-x * x / (2 * sigma * sigma));
        s += gf[x + n];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) gf[x + n] = (float)(gf[x + n] * s);
    memset(&c, 0, sizeof(c));
    c.n = n;
    for (int x = 0; x <= n && x < 8; x++) {
        c.g[x] = gf[x + n];
        c.xg[x] = (float)(x * c.g[x]);
        c.xxg[x] = (float)(x * x * c.g[x]);
    }
    double G00 = 0, G11 = 0, G33 = 0, G55 = 0;
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            float gg = gf[y + n] * gf[x + n];
            G00 += gg;
            G11 += gg * x * x;
            G33 += gg * x * x * x * x;
            G55 += gg * x * x * y * y;
        }
    double a = G00, b = G11, cc = G33, e = G55;
    double det = a * (cc * cc - e * e) - 2 * b * b * (cc - e);
    c.ig11 = 1. / G11;
    c.ig03 = -b * (cc - e) / det;
    c.ig33 = (a * cc - b * b) / det;
    c.ig55 = 1. / G55;
}

static int check_params(const ofc_fb_params &p, int W, int H)
{
    OFC_REQUIRE(W >= 16 && H >= 16 && W <= 16384 && H <= 16384, "frame size %dx%d out of range", W, H);
    OFC_REQUIRE(p.pyr_scale > 0 && p.pyr_scale < 1, "pyr_scale must be in (0,1)");
    OFC_REQUIRE(p.levels >= 0 && p.levels <= 16, "levels out of range");
    OFC_REQUIRE(p.iterations >= 1 && p.iterations <= 64, "iterations out of range");
    if (p.flags != 0) {
        set_error("flags=%d: only the box-filter variant (flags 0) the reference uses is implemented", p.flags);
        return OFC_EUNSUPPORTED;
    }
    if ((p.winsize & 1) && p.winsize > OFC_WINSIZE_MAX) {      // (even windows: OFC_EINVAL where a window is used)
        set_error("winsize %d unsupported (odd 5..%d)", p.winsize, OFC_WINSIZE_MAX);
        return OFC_EUNSUPPORTED;
    }
    return polyexp_n_check(p.poly_n);
}

}  // namespace ofc

using namespace ofc;

// =================================================================================================
// plumbing
// =================================================================================================
extern "C" {

int ofc_version(void) { return OFC_VERSION; }
const char *ofc_last_error(void) { return g_err.c_str(); }

int ofc_device_count(int *n)
{
    OFC_REQUIRE(n, "null pointer");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = (e == hipSuccess) ? c : 0;
    return OFC_OK;
}

int ofc_malloc(int device, size_t bytes, void **dptr)
{
    OFC_REQUIRE(dptr, "null pointer");
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipMalloc(dptr, bytes));
    return OFC_OK;
}

int ofc_free(int device, void *dptr)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipFree(dptr));
    return OFC_OK;
}

int ofc_memcpy_h2d(int device, void *dst, const void *src, size_t bytes)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return OFC_OK;
}

int ofc_memcpy_d2h(int device, void *dst, const void *src, size_t bytes)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_memset(int device, void *dst, int value, size_t bytes)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipMemset(dst, value, bytes));
    return OFC_OK;
}

int ofc_device_sync(int device)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipDeviceSynchronize());
    return OFC_OK;
}

void ofc_fb_default_params(ofc_fb_params *p)
{
    if (!p) return;
    p->pyr_scale = 0.5; p->levels = 3; p->winsize = 15; p->iterations = 3;
    p->poly_n = 5; p->poly_sigma = 1.2; p->flags = 0;
}

}  // extern "C"

// =================================================================================================
// flow engine
// =================================================================================================
struct ofc_flow {
    int device = 0, W = 0, H = 0, max_batch = 0, levels = 0;
    ofc_fb_params prm{};
    PolyConsts pc{};
    std::vector<LevelGeom> geom;    // [0..levels]
    hipStream_t stream = nullptr;
    DevBuf I, R, M, flowA, flowB, flowC;   // scratch sized for level 0 and max_batch
    // Front end beside the level-0 expansion: the level images and expansions of levels 1.. depend on
    // the frames only and are latency-bound chains of many short work-groups that fit beside the level-0 expansion's, so
    // they run on `side` while `stream` runs the level-0 front end, and every level's iterations wait for that level's
    // `ready` event.  Each level then needs its own slice of I and R (offI / offR, in floats; all zero in the serial order,
    // where every level reuses the level-0 sized buffers).  OFC_FLOW_FRONT_OVERLAP=0 forces the serial order (ofc_flow_create).
    bool front_overlap = false;
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr;
    std::vector<hipEvent_t> ready;  // [0..levels], [0] unused (null)
    std::vector<size_t> offI, offR; // [0..levels]
    // With the overlap on, the level images of all coarse levels come from one k_pyramid_dec launch on the side stream when
    // every one of them is an exact decimation (at most three: 2x, 4x, 8x); OFC_PYRAMID_FUSED=0 keeps the per-level launches
    bool pyramid_fused = false;
    bool fused = true;              // update-matrices fused into the box/solve kernel (winsize <= 15); otherwise the staged
                                    // kernels: k_box_solve<8> at 17, k_box_solve_wide from 19 on
    bool fuse_level0 = true;        // polyexp of level 0 reads the u8 frames (no f32 level-0 image)
    bool fuse2 = false;             // iterations 2+3 of a level in one launch (k_flow_iter2): measured SLOWER than two launches
                                    // on MI355X, kept as an opt-in experiment: OFC_FLOW_FUSE2=1 ...
    int fuse2_min_w = 0;            // ... or OFC_FLOW_FUSE2=<N > 1>: only at pyramid levels at least N pixels wide
    bool w3 = false;                // iterations 2.. of a level with the 3-waves-per-SIMD kernel (k_flow_iter_w3): OFC_FLOW_W3
    int w3_min_w = 0;
    DevBuf frames2, flow1;          // staging for the host-pointer entry points (batch of 1)
    DevBuf prev_gray;               // streaming state
    bool have_prev = false;
    DevBuf bgr_in, vis, vis_partial, vis_stats, mean_mag;   // ofc_flow_push_bgr
    bool have_vis = false;          // `vis` holds a visualisation (allocated by the first BGR push, drawn by the first pair)
    DevBuf uv_scratch;              // per-work-group (sum u, sum v) records of the last level-0 iteration (ofc_flow_calc_frames_dev_stats)
    // A batch's launch sequence (4 pyramid levels x {level image, expansion, 3 iterations}: ~20 dependent launches, most of
    // them a few microseconds long on the coarse levels) is captured once per distinct argument set into a HIP graph and
    // replayed: a clip is processed with the same resident buffers step after step.  Opt-in (OFC_FLOW_GRAPH=1): measured on
    // MI355X it changes nothing -- 36.90 against 36.90 ms per 300-frame step, 5.33-5.41 ms per 38-pair shard either way
    // (two engines on two streams already cover each other's launch gaps; rocprof shows the GPU busy 99 % of a step).
    struct Captured {
        const uint8_t *frames = nullptr;
        int n_frames = 0;
        float *flow = nullptr;
        double *uv_sum = nullptr;
        int hits = 0;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
    };
    std::vector<Captured> graphs;
    bool use_graph = false;
};

namespace ofc {

// A flow buffer of a batch as the iterations see it: the fields of the forward pairs at `f`; in a bidirectional run the
// fields of the backward pairs at `b` (in the engine's scratch right behind the forward ones, at level 0 the caller's second
// buffer), otherwise null.
struct FlowHalves {
    float *f = nullptr, *b = nullptr;
    bool operator==(const FlowHalves &o) const { return f == o.f; }
};

static void flow_drop_graphs(ofc_flow *f)
{
    for (auto &g : f->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    f->graphs.clear();
}

// The first bidirectional call doubles the flow scratch (and M in staged mode): 2 max_batch fields per buffer.  The old
// buffers are freed, which waits for the device; captured graphs hold their addresses and are dropped.
static int flow_reserve_bidir(ofc_flow *f)
{
    const size_t P0 = (size_t)f->W * f->H, nb = 2 * (size_t)f->max_batch;
    const size_t P1 = f->levels >= 1 ? (size_t)f->geom[1].w * f->geom[1].h : 1;
    const size_t needAB = sizeof(float) * 2 * P1 * nb, needC = sizeof(float) * 2 * P0 * nb, needM = sizeof(float) * 5 * P0 * nb;
    if (f->flowA.bytes >= needAB && f->flowB.bytes >= needAB && (f->fused ? f->flowC.bytes >= needC : f->M.bytes >= needM))
        return OFC_OK;
    if (!f->graphs.empty()) OFC_HIP(hipStreamSynchronize(f->stream));     // no replay in flight when its graph goes
    flow_drop_graphs(f);
    OFC_TRY(reserve(f->flowA, needAB));
    OFC_TRY(reserve(f->flowB, needAB));
    if (f->fused) OFC_TRY(reserve(f->flowC, needC));
    else OFC_TRY(reserve(f->M, needM));
    return OFC_OK;
}

// One batch: the front end of every level over the n_frames frames, then the iterations, coarsest level first.  With
// bwd_dev the iterations run both directions of every pair (ofc_flow_calc_frames_dev_bidir): the front end is the same, every
// flow buffer holds 2 npair fields, and the launches of the level loop cover both halves.
static int flow_run(ofc_flow *f, const uint8_t *frames_dev, int n_frames, float *flow_dev, double *uv_sum_dev = nullptr,
                    float *bwd_dev = nullptr)
{
    const int npair = n_frames - 1;
    const bool bidir = bwd_dev != nullptr;
    const int nfield = bidir ? 2 * npair : npair;
    const int W = f->W, H = f->H;
    hipStream_t s = f->stream;
    const int iters = f->prm.iterations;
    FlowHalves prevFlow;
    int pw = 0, ph = 0;
    if (bidir) OFC_TRY(flow_reserve_bidir(f));
    // a level's front end: level image and polynomial expansion of the batch's frames into the level's slices of I and R
    auto front_end = [&](int k, hipStream_t st) -> int {
        float *I = f->I.as<float>() + f->offI[k], *R = f->R.as<float>() + f->offR[k];
        const LevelGeom &g = f->geom[k];
        if (k == 0 && f->fuse_level0 && polyexp_u8_ok(W, H, g)) return launch_polyexp_u8(frames_dev, R, n_frames, W, H, f->pc, st);
        OFC_TRY(launch_level_image(frames_dev, I, n_frames, W, H, g, st));
        return launch_polyexp(I, R, n_frames, g.w, g.h, f->pc, 0, st);
    };
    if (f->front_overlap) {
        // fork behind everything the main stream holds: the copies of the frames, and the previous call's iterations, which
        // still read the per-level R.  Then the coarse levels' front ends on the side stream, coarsest first (the order the
        // iterations want them in), and the level-0 front end beside them on the main stream.
        OFC_HIP(hipEventRecord(f->fork, s));
        OFC_HIP(hipStreamWaitEvent(f->side, f->fork, 0));
        const bool one_launch = f->pyramid_fused && ((uintptr_t)frames_dev % 4) == 0;
        if (one_launch) {
            float *lv[3] = {nullptr, nullptr, nullptr};
            for (int k = 1; k <= f->levels; k++) lv[k - 1] = f->I.as<float>() + f->offI[k];
            OFC_TRY(launch_pyramid_dec(frames_dev, lv, n_frames, W, H, f->geom.data(), f->levels, f->side));
        }
        for (int k = f->levels; k >= 1; k--) {
            if (one_launch) {
                const LevelGeom &g = f->geom[k];
                OFC_TRY(launch_polyexp(f->I.as<float>() + f->offI[k], f->R.as<float>() + f->offR[k], n_frames, g.w, g.h, f->pc, 0, f->side));
            } else {
                OFC_TRY(front_end(k, f->side));
            }
            OFC_HIP(hipEventRecord(f->ready[k], f->side));
        }
        OFC_TRY(front_end(0, s));
    }
    for (int k = f->levels; k >= 0; k--) {
        const LevelGeom &g = f->geom[k];
        const size_t P = (size_t)g.w * g.h;
        const size_t half = 2 * P * npair;              // floats of one direction's fields at this level
        auto scratch = [&](DevBuf &b) { FlowHalves h; h.f = b.as<float>(); h.b = bidir ? h.f + half : nullptr; return h; };
        auto adjacent = [&](const FlowHalves &h) { return h.b == h.f + half; };
        auto zero = [&](const FlowHalves &h) -> int {
            OFC_HIP(hipMemsetAsync(h.f, 0, sizeof(float) * half, s));
            if (bidir) OFC_HIP(hipMemsetAsync(h.b, 0, sizeof(float) * half, s));
            return OFC_OK;
        };
        // the level's final flow lands in `dst` (level 0: the caller's buffers); iterations ping-pong between
        // dst and tmp, so the initial flow goes to whichever makes the last iteration write dst
        FlowHalves dst, tmp;
        if (k == 0) { dst.f = flow_dev; dst.b = bwd_dev; }
        else dst = scratch(((f->levels - k) & 1) ? f->flowB : f->flowA);
        if (f->fused) tmp = scratch(f->flowC);
        const float *R = f->R.as<float>() + f->offR[k];
        if (!f->front_overlap) {
            OFC_TRY(front_end(k, s));
        } else if (k >= 1) {
            // after the wait at level 1 the side stream is joined: whatever a caller could wait for is reachable from `s`
            OFC_HIP(hipStreamWaitEvent(s, f->ready[k], 0));
        }
        const size_t strideR = 5 * P;
        const float mul = (float)(1. / f->prm.pyr_scale);
        if (f->fused) {
            // launch plan: the first iteration alone (it reads the coarser level directly -- upsample fused -- or, at the
            // top of the pyramid, a zeroed buffer), then two iterations per launch while the level is wide enough for the
            // two-iteration kernel's 228-column tiles, single launches otherwise.  Launch l of L writes dst when (L-1-l)
            // is even, tmp otherwise, so that the last one lands in dst.  (The bidirectional run has the plain kernel only.)
            const bool two = !bidir && f->fuse2 && f->prm.winsize == 15 && g.w >= f->fuse2_min_w;
            const bool w3 = !bidir && f->w3 && f->prm.winsize == 15 && g.w >= f->w3_min_w;
            int plan[64], L = 0;
            for (int i = 0; i < iters;) {
                const int n = (two && i > 0 && iters - i >= 2) ? 2 : 1;
                plan[L++] = n;
                i += n;
            }
            FlowHalves cur;
            for (int l = 0; l < L; l++) {
                const FlowHalves nxt = ((L - 1 - l) & 1) ? tmp : dst;
                if (l == 0 && !prevFlow.f) {
                    cur = (nxt == dst) ? tmp : dst;
                    OFC_TRY(zero(cur));
                }
                const bool ups = l == 0 && prevFlow.f;
                if (bidir) {
                    OFC_TRY(launch_flow_iter_bidir(R, strideR, ups ? nullptr : cur.f, ups ? nullptr : cur.b, nxt.f, nxt.b, npair, g.w,
                                                   g.h, f->prm.winsize, s, ups ? prevFlow.f : nullptr, ups ? prevFlow.b : nullptr,
                                                   ups ? pw : 0, ups ? ph : 0, ups ? mul : 1.f));
                } else if (ups) {
                    OFC_TRY(launch_flow_iter(R, strideR, nullptr, nxt.f, npair, g.w, g.h, f->prm.winsize, s, prevFlow.f, pw, ph, mul));
                } else {
                    if (uv_sum_dev && k == 0 && l == L - 1 && plan[l] == 1 && f->prm.winsize == 15 && !(f->w3 && g.w >= f->w3_min_w)) {
                        // the field's column sums ride in the epilogue of the iteration that writes it
                        const size_t need = (size_t)flow_iter_max_grid(g.w, g.h, npair, f->prm.winsize) * 2;
                        OFC_TRY(reserve(f->uv_scratch, need * sizeof(double)));
                        // the launch is told what the buffer holds, not what this call needs: its own check then guards the records
                        OFC_TRY(launch_flow_iter(R, strideR, cur.f, nxt.f, npair, g.w, g.h, f->prm.winsize, s, nullptr, 0, 0, 1.f,
                                                 uv_sum_dev, f->uv_scratch.as<double>(), f->uv_scratch.bytes / sizeof(double)));
                        uv_sum_dev = nullptr;
                    } else
                    if (plan[l] == 2) OFC_TRY(launch_flow_iter2(R, strideR, cur.f, nxt.f, npair, g.w, g.h, f->prm.winsize, s));
                    else if (w3) OFC_TRY(launch_flow_iter_w3(R, strideR, cur.f, nxt.f, npair, g.w, g.h, f->prm.winsize, s));
                    else OFC_TRY(launch_flow_iter(R, strideR, cur.f, nxt.f, npair, g.w, g.h, f->prm.winsize, s));
                }
                cur = nxt;
            }
        } else {
            // staged kernels, in place in dst.  Bidirectional: M holds 2 npair pairs, its second half filled with the frames
            // swapped; the per-field kernels take both halves in one launch where the halves are adjacent (every level but
            // 0), and in two launches of the same strip height otherwise
            const FlowHalves cur = dst;
            const bool one = !bidir || adjacent(cur);
            if (!prevFlow.f) {
                OFC_TRY(zero(cur));
            } else if (one) {
                OFC_TRY(launch_flow_resize(prevFlow.f, cur.f, nfield, pw, ph, g.w, g.h, mul, s));
            } else {
                OFC_TRY(launch_flow_resize(prevFlow.f, cur.f, npair, pw, ph, g.w, g.h, mul, s));
                OFC_TRY(launch_flow_resize(prevFlow.b, cur.b, npair, pw, ph, g.w, g.h, mul, s));
            }
            float *M = f->M.as<float>(), *Mb = M + 5 * P * npair;
            const int box_rows = (bidir && f->prm.winsize < WINSIZE_WIDE_MIN) ? box_default_rows(g.w, g.h, nfield) : 0;
            auto matrices = [&]() -> int {
                OFC_TRY(launch_update_matrices(R, R + strideR, strideR, cur.f, M, npair, g.w, g.h, s));
                if (bidir) OFC_TRY(launch_update_matrices(R + strideR, R, strideR, cur.b, Mb, npair, g.w, g.h, s));
                return OFC_OK;
            };
            OFC_TRY(matrices());
            for (int i = 0; i < iters; i++) {
                if (one) {
                    OFC_TRY(launch_box_solve(M, cur.f, nfield, g.w, g.h, f->prm.winsize, box_rows, s));
                } else {
                    OFC_TRY(launch_box_solve(M, cur.f, npair, g.w, g.h, f->prm.winsize, box_rows, s));
                    OFC_TRY(launch_box_solve(Mb, cur.b, npair, g.w, g.h, f->prm.winsize, box_rows, s));
                }
                if (i < iters - 1) OFC_TRY(matrices());
            }
        }
        prevFlow = dst;
        pw = g.w; ph = g.h;
    }
    if (uv_sum_dev) {       // no epilogue carried them (one iteration per level, staged mode, another winsize, one of the
                            // experimental engines): one sweep over the finished field gives the same two sums
        const int64_t N = (int64_t)npair * W * H;
        const int max_blocks = 1024;    // the scratch is sized for the most records a sweep writes (16 KiB), whatever this call needs
        const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(N / 4, 256), max_blocks));
        OFC_TRY(reserve(f->uv_scratch, sizeof(double) * 2 * max_blocks));
        OFC_TRY(launch_lloyd_colstats(flow_dev, OFC_F32, N, 2, nullptr, 0, f->uv_scratch.as<double>(), nblocks, s));
        OFC_TRY(launch_reduce_records(f->uv_scratch.as<double>(), nblocks, 2, uv_sum_dev, s));
    }
    return OFC_OK;
}

// flow_run through a captured graph: the first call with an argument set runs directly, the second captures and
// instantiates, later ones replay.  (Two direct runs first: one-off calls -- tests, the streaming entry points with their
// rotating buffers -- never pay for an instantiation.)
static int flow_run_cached(ofc_flow *f, const uint8_t *frames_dev, int n_frames, float *flow_dev, double *uv_sum_dev)
{
    if (!f->use_graph) return flow_run(f, frames_dev, n_frames, flow_dev, uv_sum_dev);
    ofc_flow::Captured *c = nullptr;
    for (auto &g : f->graphs)
        if (g.frames == frames_dev && g.n_frames == n_frames && g.flow == flow_dev && g.uv_sum == uv_sum_dev) { c = &g; break; }
    if (!c) {
        if (f->graphs.size() >= 64) flow_drop_graphs(f);    // a caller that never repeats itself: stop bookkeeping
        f->graphs.emplace_back();
        c = &f->graphs.back();
        c->frames = frames_dev; c->n_frames = n_frames; c->flow = flow_dev; c->uv_sum = uv_sum_dev;
    }
    c->hits++;
    if (c->exec) {
        OFC_HIP(hipGraphLaunch(c->exec, f->stream));
        return OFC_OK;
    }
    if (c->hits < 2) return flow_run(f, frames_dev, n_frames, flow_dev, uv_sum_dev);   // (also sizes uv_scratch: no allocation inside a capture)
    OFC_HIP(hipStreamBeginCapture(f->stream, hipStreamCaptureModeThreadLocal));
    const int rc = flow_run(f, frames_dev, n_frames, flow_dev, uv_sum_dev);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(f->stream, &g);
    if (rc != OFC_OK || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        f->use_graph = false;                       // whatever could not be captured: plain launches from now on
        (void)hipGetLastError();
        return flow_run(f, frames_dev, n_frames, flow_dev, uv_sum_dev);
    }
    hipGraphExec_t ex = nullptr;
    if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess || !ex) {
        (void)hipGraphDestroy(g);
        f->use_graph = false;
        (void)hipGetLastError();
        return flow_run(f, frames_dev, n_frames, flow_dev, uv_sum_dev);
    }
    c->graph = g;
    c->exec = ex;
    OFC_HIP(hipGraphLaunch(c->exec, f->stream));
    return OFC_OK;
}

}  // namespace ofc

extern "C" {

int ofc_flow_create(int device, int W, int H, const ofc_fb_params *p, int max_batch, ofc_flow_t **out)
{
    OFC_REQUIRE(out, "null out pointer");
    *out = nullptr;
    ofc_fb_params prm;
    if (p) prm = *p; else ofc_fb_default_params(&prm);
    OFC_TRY(check_params(prm, W, H));
    OFC_REQUIRE(max_batch >= 1 && max_batch <= 4096, "max_batch out of range");
    OFC_REQUIRE((prm.winsize & 1) && prm.winsize >= 5, "winsize must be odd and >= 5");
    std::unique_ptr<ofc_flow, void (*)(ofc_flow_t *)> f(new ofc_flow, ofc_flow_destroy);   // a failure below leaves no stream or event behind
    f->device = device; f->W = W; f->H = H; f->max_batch = max_batch; f->prm = prm;
    f->levels = pyramid_levels(W, H, prm);
    for (int k = 0; k <= f->levels; k++) f->geom.push_back(level_geometry(W, H, prm, k));
    {
        const char *e = getenv("OFC_FLOW_STAGED");      // debugging aid: force the separate K4 / K5 kernels
        f->fused = prm.winsize <= 15 && !(e && e[0] == '1');
        f->fuse_level0 = !(e && e[0] == '1');            // the staged mode also keeps the separate level-0 image
        const char *e3 = getenv("OFC_FLOW_W3");           // 1: everywhere; N > 1: at levels >= N wide; 0: off
        if (e3 && e3[0]) {
            const int v = atoi(e3);
            f->w3 = v != 0;
            f->w3_min_w = v > 1 ? v : 0;
        }
        const char *eg = getenv("OFC_FLOW_GRAPH");
        f->use_graph = eg && eg[0] == '1';
        const char *e2 = getenv("OFC_FLOW_FUSE2");       // 1: two iterations per launch; N > 1: at levels >= N wide
        if (e2 && e2[0]) {
            const int v = atoi(e2);
            f->fuse2 = v != 0;
            if (v > 1) f->fuse2_min_w = v;
        }
    }
    // what the launches of flow_run would refuse at the first calc (a level whose blur is wider than 31 taps, a level image
    // tile beyond the LDS, a frame beyond the fused iteration's 32-bit offsets) is refused here, before the device is
    // touched: nothing is allocated, and the streaming forms have stored no frame
    OFC_TRY(flow_levels_check(W, H, prm, f->geom.data(), f->levels, f->fused, f->fuse_level0));
    OFC_TRY(ensure_device(device));
    polyexp_setup(prm.poly_n, prm.poly_sigma, f->pc);
    OFC_HIP(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    const size_t P0 = (size_t)W * H, nb = (size_t)max_batch;
    size_t nI = P0 * (nb + 1), nR = 5 * P0 * (nb + 1);          // floats: one level-0 sized buffer each, shared by the levels
    f->offI.assign(f->levels + 1, 0);
    f->offR.assign(f->levels + 1, 0);
    {
        // a slice of R per level, and of I per level that has a level image (level 0 has none when its expansion reads the
        // u8 frames), each 256-byte aligned as an allocation of its own would be
        const bool u8_level0 = f->fuse_level0 && polyexp_u8_ok(W, H, f->geom[0]);
        std::vector<size_t> oI(f->levels + 1, 0), oR(f->levels + 1, 0);
        size_t sI = 0, sR = 0;
        for (int k = 0; k <= f->levels; k++) {
            const size_t Pk = (size_t)f->geom[k].w * f->geom[k].h;
            oR[k] = sR;
            sR += (5 * Pk * (nb + 1) + 63) & ~(size_t)63;
            oI[k] = sI;
            if (k > 0 || !u8_level0) sI += (Pk * (nb + 1) + 63) & ~(size_t)63;
        }
        // On unless OFC_FLOW_FRONT_OVERLAP=0 forces the serial order (A/B runs, the parity test), when there is a coarse
        // level to run aside, the order is not captured into a graph (a capture must stay one chain), and the slices
        // together stay within 1.5 x the shared buffers: a deep pyramid at a pyr_scale near 1 must not multiply the
        // engine's memory.
        const char *eo = getenv("OFC_FLOW_FRONT_OVERLAP");
        f->front_overlap = !(eo && eo[0] == '0') && f->levels >= 1 && !f->use_graph && 2 * (sI + sR) <= 3 * (nI + nR);
        if (f->front_overlap) {
            f->offI = oI; f->offR = oR;
            nI = sI; nR = sR;
        }
    }
    {
        const char *ep = getenv("OFC_PYRAMID_FUSED");
        f->pyramid_fused = !(ep && ep[0] == '0') && f->front_overlap && f->levels <= 3 &&
                           pyramid_dec_levels(W, H, f->geom.data(), f->levels, true) == f->levels;
    }
    if (f->front_overlap) {
        OFC_HIP(hipStreamCreateWithFlags(&f->side, hipStreamNonBlocking));
        OFC_HIP(hipEventCreateWithFlags(&f->fork, hipEventDisableTiming));
        f->ready.assign(f->levels + 1, nullptr);
        for (int k = 1; k <= f->levels; k++) OFC_HIP(hipEventCreateWithFlags(&f->ready[k], hipEventDisableTiming));
    }
    OFC_TRY(f->I.alloc(sizeof(float) * nI));
    OFC_TRY(f->R.alloc(sizeof(float) * nR));
    if (f->fused) {
        OFC_TRY(f->flowC.alloc(sizeof(float) * 2 * P0 * nb));
    } else {
        OFC_TRY(f->M.alloc(sizeof(float) * 5 * P0 * nb));
    }
    const size_t P1 = f->levels >= 1 ? (size_t)f->geom[1].w * f->geom[1].h : 1;
    OFC_TRY(f->flowA.alloc(sizeof(float) * 2 * P1 * nb));
    OFC_TRY(f->flowB.alloc(sizeof(float) * 2 * P1 * nb));
    OFC_TRY(f->frames2.alloc(2 * P0));
    OFC_TRY(f->flow1.alloc(sizeof(float) * 2 * P0));
    OFC_TRY(f->prev_gray.alloc(P0));
    *out = f.release();
    return OFC_OK;
}

void ofc_flow_destroy(ofc_flow_t *f)
{
    if (!f) return;
    if (f->stream) (void)hipSetDevice(f->device);   // (an engine refused before it touched the device has nothing there)
    // both streams drain and go before any buffer is freed: the side stream may still write the coarse levels' I and R
    for (hipStream_t s : {f->stream, f->side})
        if (s) (void)hipStreamSynchronize(s);
    for (hipStream_t s : {f->stream, f->side})
        if (s) (void)hipStreamDestroy(s);
    if (f->fork) (void)hipEventDestroy(f->fork);
    for (hipEvent_t e : f->ready)
        if (e) (void)hipEventDestroy(e);
    for (auto &g : f->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    delete f;
}

int ofc_flow_calc_frames_dev(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *flow_dev)
{
    OFC_REQUIRE(f && frames_dev && flow_dev, "null pointer");
    OFC_REQUIRE(n_frames >= 2 && n_frames - 1 <= f->max_batch, "n_frames-1 = %d pairs not in [1, max_batch=%d]",
                n_frames - 1, f->max_batch);
    OFC_TRY(ensure_device(f->device));
    return flow_run_cached(f, frames_dev, n_frames, flow_dev, nullptr);
}

int ofc_flow_calc_frames_dev_stats(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *flow_dev, double *uv_sum_dev)
{
    OFC_REQUIRE(f && frames_dev && flow_dev && uv_sum_dev, "null pointer");
    OFC_REQUIRE(n_frames >= 2 && n_frames - 1 <= f->max_batch, "n_frames-1 = %d pairs not in [1, max_batch=%d]",
                n_frames - 1, f->max_batch);
    OFC_TRY(ensure_device(f->device));
    return flow_run_cached(f, frames_dev, n_frames, flow_dev, uv_sum_dev);
}

static int flow_calc_bidir(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *fwd_dev, float *bwd_dev, double *uv_sum_dev)
{
    OFC_REQUIRE(f && frames_dev && fwd_dev && bwd_dev, "null pointer");
    OFC_REQUIRE(n_frames >= 2 && n_frames - 1 <= f->max_batch, "n_frames-1 = %d pairs not in [1, max_batch=%d]",
                n_frames - 1, f->max_batch);
    const size_t half = 2 * (size_t)f->W * f->H * (size_t)(n_frames - 1);
    OFC_REQUIRE(fwd_dev + half <= bwd_dev || bwd_dev + half <= fwd_dev, "fwd_dev and bwd_dev overlap");
    OFC_TRY(ensure_device(f->device));
    return flow_run(f, frames_dev, n_frames, fwd_dev, uv_sum_dev, bwd_dev);     // plain launches, also with graph replay on
}

int ofc_flow_calc_frames_dev_bidir(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *fwd_dev, float *bwd_dev)
{
    return flow_calc_bidir(f, frames_dev, n_frames, fwd_dev, bwd_dev, nullptr);
}

int ofc_flow_calc_frames_dev_bidir_stats(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *fwd_dev, float *bwd_dev,
                                         double *uv_sum_dev)
{
    OFC_REQUIRE(uv_sum_dev, "null pointer");
    return flow_calc_bidir(f, frames_dev, n_frames, fwd_dev, bwd_dev, uv_sum_dev);
}

hipStream_t ofc_flow_stream_internal(ofc_flow_t *f) { return f->stream; }   // for stream_api.cpp (not exported in ofc.h)

int ofc_flow_sync(ofc_flow_t *f)
{
    OFC_REQUIRE(f, "null pointer");
    OFC_TRY(ensure_device(f->device));
    OFC_HIP(hipStreamSynchronize(f->stream));
    return OFC_OK;
}

int ofc_flow_front_overlap(const ofc_flow_t *f, int *on)
{
    OFC_REQUIRE(f && on, "null pointer");
    *on = f->front_overlap ? 1 : 0;
    return OFC_OK;
}

int ofc_flow_pyramid_fused(const ofc_flow_t *f, int *on)
{
    OFC_REQUIRE(f && on, "null pointer");
    *on = f->pyramid_fused ? 1 : 0;
    return OFC_OK;
}

int ofc_flow_calc(ofc_flow_t *f, const uint8_t *prev_gray, const uint8_t *next_gray, float *flow_out)
{
    OFC_REQUIRE(f && prev_gray && next_gray && flow_out, "null pointer");
    OFC_TRY(ensure_device(f->device));
    const size_t P0 = (size_t)f->W * f->H;
    uint8_t *fr = f->frames2.as<uint8_t>();
    OFC_HIP(hipMemcpyAsync(fr, prev_gray, P0, hipMemcpyHostToDevice, f->stream));
    OFC_HIP(hipMemcpyAsync(fr + P0, next_gray, P0, hipMemcpyHostToDevice, f->stream));
    OFC_TRY(flow_run(f, fr, 2, f->flow1.as<float>()));
    OFC_HIP(hipMemcpyAsync(flow_out, f->flow1.p, sizeof(float) * 2 * P0, hipMemcpyDeviceToHost, f->stream));
    OFC_HIP(hipStreamSynchronize(f->stream));
    return OFC_OK;
}

int ofc_flow_push_gray(ofc_flow_t *f, const uint8_t *gray, float *flow_out)
{
    OFC_REQUIRE(f && gray, "null pointer");
    OFC_TRY(ensure_device(f->device));
    const size_t P0 = (size_t)f->W * f->H;
    uint8_t *fr = f->frames2.as<uint8_t>();
    if (!f->have_prev) {
        OFC_HIP(hipMemcpyAsync(f->prev_gray.p, gray, P0, hipMemcpyHostToDevice, f->stream));
        OFC_HIP(hipStreamSynchronize(f->stream));
        f->have_prev = true;
        set_error("first frame pushed: no pair yet");
        return OFC_ENOTREADY;
    }
    OFC_REQUIRE(flow_out, "null flow_out");
    OFC_HIP(hipMemcpyAsync(fr, f->prev_gray.p, P0, hipMemcpyDeviceToDevice, f->stream));
    OFC_HIP(hipMemcpyAsync(fr + P0, gray, P0, hipMemcpyHostToDevice, f->stream));
    OFC_HIP(hipMemcpyAsync(f->prev_gray.p, fr + P0, P0, hipMemcpyDeviceToDevice, f->stream));
    OFC_TRY(flow_run(f, fr, 2, f->flow1.as<float>()));
    OFC_HIP(hipMemcpyAsync(flow_out, f->flow1.p, sizeof(float) * 2 * P0, hipMemcpyDeviceToHost, f->stream));
    OFC_HIP(hipStreamSynchronize(f->stream));
    return OFC_OK;
}

int ofc_flow_push_bgr(ofc_flow_t *f, const uint8_t *bgr, uint8_t *vis_out, float *mean_mag, float *flow_out)
{
    OFC_REQUIRE(f && bgr, "null pointer");
    OFC_TRY(ensure_device(f->device));
    const size_t P0 = (size_t)f->W * f->H;
    hipStream_t s = f->stream;
    if (!f->bgr_in.p) {
        OFC_TRY(f->bgr_in.alloc(P0 * 3 + 16));
        OFC_TRY(f->vis.alloc(P0 * 3 + 16));
        OFC_TRY(f->vis_partial.alloc(sizeof(double) * 3 * VIS_BLOCKS));
        OFC_TRY(f->vis_stats.alloc(sizeof(VisFrameStats)));
        OFC_TRY(f->mean_mag.alloc(sizeof(float)));
    }
    uint8_t *fr = f->frames2.as<uint8_t>();
    OFC_HIP(hipMemcpyAsync(f->bgr_in.p, bgr, P0 * 3, hipMemcpyHostToDevice, s));
    if (!f->have_prev) {
        OFC_TRY(launch_bgr2gray(f->bgr_in.as<uint8_t>(), f->prev_gray.as<uint8_t>(), (int64_t)P0, s));
        OFC_HIP(hipStreamSynchronize(s));
        f->have_prev = true;
        set_error("first frame pushed: no pair yet");
        return OFC_ENOTREADY;
    }
    OFC_HIP(hipMemcpyAsync(fr, f->prev_gray.p, P0, hipMemcpyDeviceToDevice, s));
    OFC_TRY(launch_bgr2gray(f->bgr_in.as<uint8_t>(), fr + P0, (int64_t)P0, s));
    OFC_HIP(hipMemcpyAsync(f->prev_gray.p, fr + P0, P0, hipMemcpyDeviceToDevice, s));
    OFC_TRY(flow_run(f, fr, 2, f->flow1.as<float>()));
    OFC_TRY(launch_flow_to_bgr(f->flow1.as<float>(), f->W, f->H, 1, f->vis.as<uint8_t>(), f->mean_mag.as<float>(),
                               f->vis_partial.as<double>(), f->vis_stats.as<VisFrameStats>(), s));
    if (vis_out) OFC_HIP(hipMemcpyAsync(vis_out, f->vis.p, P0 * 3, hipMemcpyDeviceToHost, s));
    if (mean_mag) OFC_HIP(hipMemcpyAsync(mean_mag, f->mean_mag.p, sizeof(float), hipMemcpyDeviceToHost, s));
    if (flow_out) OFC_HIP(hipMemcpyAsync(flow_out, f->flow1.p, sizeof(float) * 2 * P0, hipMemcpyDeviceToHost, s));
    OFC_HIP(hipStreamSynchronize(s));
    f->have_vis = true;
    return OFC_OK;
}

int ofc_flow_last_vis_dev(ofc_flow_t *f, const uint8_t **vis_dev)
{
    OFC_REQUIRE(f && vis_dev, "null pointer");
    OFC_REQUIRE(f->have_vis, "no visualisation yet: no ofc_flow_push_bgr has returned OFC_OK");
    *vis_dev = f->vis.as<uint8_t>();
    return OFC_OK;
}

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
    OFC_TRY(check_params(prm, W, H));
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
    OFC_TRY(check_params(prm, W0, H0));
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
        else OFC_TRY(launch_flow_iter(dR.as<float>(), 5 * P, cur, nxt, 1, W, H, winsize, nullptr, nullptr, 0, 0, 1.f, nullptr, nullptr, 0,
                                      rows_per_block));
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
    out[0] = winsize <= 15 ? flow_iter_rows(W, H, n_pairs, winsize) : 0;
    out[1] = winsize >= WINSIZE_WIDE_MIN ? box_wide_rows(winsize) : box_default_rows(W, H, n_pairs);
    out[2] = polyexp_default_rows(W, H, n_pairs + 1);
    return OFC_OK;
}

int ofc_flow_launch_geometry_bidir(int W, int H, int n_pairs, int winsize, int out[3])
{
    OFC_REQUIRE(out, "null pointer");
    OFC_REQUIRE(W >= 1 && H >= 1 && n_pairs >= 1 && n_pairs <= (1 << 20), "bad size / pair count");
    OFC_REQUIRE(winsize >= 5 && winsize <= 15 && (winsize & 1), "winsize must be odd, 5 .. 15 (the fused iteration)");
    const int rows = flow_iter_rows(W, H, 2 * n_pairs, winsize);
    out[0] = rows;
    out[1] = cdiv(W, 256 - (winsize - 1)) * cdiv(H, rows);
    out[2] = cdiv(out[1], 8) * 8 * 2 * n_pairs;
    return OFC_OK;
}

int ofc_bench_flow_bidir(int device, int W, int H, int n_frames, int reps, int what, float *ms)
{
    OFC_REQUIRE(ms && n_frames >= 2 && reps >= 1 && (what == 0 || what == 1), "bad arguments");
    ofc_flow_t *raw = nullptr;
    OFC_TRY(ofc_flow_create(device, W, H, nullptr, n_frames - 1, &raw));
    std::unique_ptr<ofc_flow, void (*)(ofc_flow_t *)> f(raw, ofc_flow_destroy);
    const size_t P = (size_t)W * H, np = (size_t)(n_frames - 1);
    DevBuf fr, rev, flow;
    OFC_TRY(fr.alloc(P * n_frames));
    OFC_TRY(rev.alloc(P * n_frames));
    OFC_TRY(flow.alloc(sizeof(float) * 2 * P * np * 2));
    OFC_TRY(ofc_synth_frames_dev(device, fr.as<uint8_t>(), W, H, n_frames, 0, 0));
    OFC_HIP(hipDeviceSynchronize());
    float *fwd = flow.as<float>(), *bwd = fwd + 2 * P * np;
    auto run = [&]() -> int {
        if (what == 0) return flow_run(f.get(), fr.as<uint8_t>(), n_frames, fwd, nullptr, bwd);
        OFC_TRY(flow_run(f.get(), fr.as<uint8_t>(), n_frames, fwd));
        OFC_TRY(launch_frames_reverse(fr.as<uint8_t>(), P, n_frames, rev.as<uint8_t>(), f->stream));
        return flow_run(f.get(), rev.as<uint8_t>(), n_frames, bwd);
    };
    // (the first warm-up run also grows the bidirectional scratch: no allocation inside the timed region)
    return time_launches(f->stream, reps, run, ms);
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
    OFC_TRY(check_params(prm, W, H));
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
