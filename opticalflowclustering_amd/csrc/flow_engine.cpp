// flow_engine.cpp -- C ABI of libofc.so, the Farneback flow engine: ofc_flow_create .. ofc_flow_last_vis_dev, and the one
// bench hook that needs the engine's batch run (ofc_bench_flow_bidir).  The single-stage hooks are in flow_stages_api.cpp.
// Declared in include/ofc.h (which cites the reference call each entry point replaces).
#include "color_common.h"
#include "fb_check.h"
#include "flow_host.h"
#include "host_util.h"
#include "lloyd_common.h"

#include <algorithm>
#include <cstdlib>
#include <memory>

using namespace ofc;

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

// The engine's environment switches, read once per engine.  (OFC_FLOW_PIPE and OFC_POLYEXP_F64 are read by the launchers at
// every launch: their tests toggle them inside one process.)
struct FlowSwitches {
    bool staged, graph, w3, fuse2, front_overlap, pyramid_fused;
    int w3_min_w, fuse2_min_w;
};

static FlowSwitches flow_read_switches()
{
    FlowSwitches sw = {};
    auto first_is = [](const char *name, char c) { const char *e = getenv(name); return e && e[0] == c; };
    auto number = [](const char *name, bool &on, int &min_w) {      // 1: everywhere; N > 1: at levels >= N wide; 0: off
        const char *e = getenv(name);
        if (!e || !e[0]) return;
        const int v = atoi(e);
        on = v != 0;
        if (v > 1) min_w = v;
    };
    sw.staged = first_is("OFC_FLOW_STAGED", '1');       // debugging aid: force the separate K4 / K5 kernels
    sw.graph = first_is("OFC_FLOW_GRAPH", '1');
    number("OFC_FLOW_W3", sw.w3, sw.w3_min_w);
    number("OFC_FLOW_FUSE2", sw.fuse2, sw.fuse2_min_w);  // two iterations per launch
    sw.front_overlap = !first_is("OFC_FLOW_FRONT_OVERLAP", '0');    // both on unless forced off (A/B runs, the parity tests)
    sw.pyramid_fused = !first_is("OFC_PYRAMID_FUSED", '0');
    return sw;
}

// The overlapped front end's layout of I and R, in floats: a slice of R per level, and of I per level that has a level image
// (level 0 has none when its expansion reads the u8 frames), each 256-byte aligned as an allocation of its own would be.
struct FlowSlices {
    std::vector<size_t> offI, offR;     // [0..levels]
    size_t nI = 0, nR = 0;              // floats in all
};

static FlowSlices flow_slice_layout(const ofc_flow &f)
{
    const bool u8_level0 = f.fuse_level0 && polyexp_u8_ok(f.W, f.H, f.geom[0]);
    const size_t nb = (size_t)f.max_batch;
    FlowSlices sl;
    sl.offI.assign(f.levels + 1, 0);
    sl.offR.assign(f.levels + 1, 0);
    for (int k = 0; k <= f.levels; k++) {
        const size_t Pk = (size_t)f.geom[k].w * f.geom[k].h;
        sl.offR[k] = sl.nR;
        sl.nR += (5 * Pk * (nb + 1) + 63) & ~(size_t)63;
        sl.offI[k] = sl.nI;
        if (k > 0 || !u8_level0) sl.nI += (Pk * (nb + 1) + 63) & ~(size_t)63;
    }
    return sl;
}

// A flow buffer of a batch as the iterations see it: the fields of the forward pairs at `f`; in a bidirectional run the
// fields of the backward pairs at `b` (in the engine's scratch right behind the forward ones, at level 0 the caller's second
// buffer), otherwise null.
struct FlowHalves {
    float *f = nullptr, *b = nullptr;
    bool operator==(const FlowHalves &o) const { return f == o.f; }
};

// What a batch works on.  With `bidir` the iterations run both directions of every pair (ofc_flow_calc_frames_dev_bidir): the
// front end is the same, every flow buffer holds 2 npair fields, and the launches of a level cover both halves.
struct FlowBatch {
    const uint8_t *frames;      // [npair + 1][H][W] u8
    int npair;
    bool bidir;
    float *fwd, *bwd;           // where the level-0 fields go; bwd null unless bidir
    double *sums;               // sum(u), sum(v) of the forward fields go here; null: not asked for, or already carried by a launch
    int nfield() const { return bidir ? 2 * npair : npair; }
};

// A level of the batch as its iterations see it
struct FlowLevel {
    int k = 0;
    size_t half = 0;            // floats of one direction's fields at this level
    FlowHalves dst;             // where the level's final flow lands (level 0: the caller's buffers)
    FlowHalves prev;            // the coarser level's final flow, pw x ph; null at the top of the pyramid: start from zero
    int pw = 0, ph = 0;
};

static FlowHalves flow_halves(const DevBuf &buf, const FlowBatch &b, const FlowLevel &lv)
{
    return {buf.as<float>(), b.bidir ? buf.as<float>() + lv.half : nullptr};
}

static int flow_zero(const FlowHalves &h, const FlowBatch &b, const FlowLevel &lv, hipStream_t s)
{
    OFC_HIP(hipMemsetAsync(h.f, 0, sizeof(float) * lv.half, s));
    if (b.bidir) OFC_HIP(hipMemsetAsync(h.b, 0, sizeof(float) * lv.half, s));
    return OFC_OK;
}

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

// a level's front end: level image and polynomial expansion of the batch's frames into the level's slices of I and R
static int flow_front_end(ofc_flow *f, const FlowBatch &b, int k, hipStream_t st)
{
    float *I = f->I.as<float>() + f->offI[k], *R = f->R.as<float>() + f->offR[k];
    const LevelGeom &g = f->geom[k];
    const int n_frames = b.npair + 1;
    if (k == 0 && f->fuse_level0 && polyexp_u8_ok(f->W, f->H, g)) return launch_polyexp_u8(b.frames, R, n_frames, f->W, f->H, f->pc, st);
    OFC_TRY(launch_level_image(b.frames, I, n_frames, f->W, f->H, g, st));
    return launch_polyexp(I, R, n_frames, g.w, g.h, f->pc, 0, st);
}

// The coarse levels' front ends on the side stream, coarsest first (the order the iterations want them in), each followed by
// its level's `ready` event.  The side stream forks behind everything the main stream holds: the copies of the frames, and the
// previous call's iterations, which still read the per-level R.
static int flow_coarse_front_ends(ofc_flow *f, const FlowBatch &b)
{
    OFC_HIP(hipEventRecord(f->fork, f->stream));
    OFC_HIP(hipStreamWaitEvent(f->side, f->fork, 0));
    const int n_frames = b.npair + 1;
    const bool one_launch = f->pyramid_fused && ((uintptr_t)b.frames % 4) == 0;
    if (one_launch) {
        float *lv[3] = {nullptr, nullptr, nullptr};
        for (int k = 1; k <= f->levels; k++) lv[k - 1] = f->I.as<float>() + f->offI[k];
        OFC_TRY(launch_pyramid_dec(b.frames, lv, n_frames, f->W, f->H, f->geom.data(), f->levels, f->side));
    }
    for (int k = f->levels; k >= 1; k--) {
        if (one_launch) {
            const LevelGeom &g = f->geom[k];
            OFC_TRY(launch_polyexp(f->I.as<float>() + f->offI[k], f->R.as<float>() + f->offR[k], n_frames, g.w, g.h, f->pc, 0, f->side));
        } else {
            OFC_TRY(flow_front_end(f, b, k, f->side));
        }
        OFC_HIP(hipEventRecord(f->ready[k], f->side));
    }
    return OFC_OK;
}

// "This launch can carry the column sums": only the plain winsize-15 kernel has the epilogue for them, and only the launch
// that writes the finished forward fields of level 0 has the numbers to sum.
static bool flow_launch_carries_sums(const ofc_flow *f, const FlowBatch &b, const FlowLevel &lv, bool last, int n_iters, bool ups,
                                     bool w3)
{
    return b.sums && !b.bidir && lv.k == 0 && last && n_iters == 1 && !ups && !w3 && f->prm.winsize == 15;
}

// A level's iterations with the fused kernel.  Launch plan: the first iteration alone (it reads the coarser level directly
// -- upsample fused -- or, at the top of the pyramid, a zeroed buffer), then two iterations per launch while the level is wide
// enough for the two-iteration kernel's 228-column tiles, single launches otherwise.  Iterations ping-pong between lv.dst
// and flowC: launch l of L writes dst when (L-1-l) is even, flowC otherwise, so that the last one lands in dst, and a zeroed
// start goes to whichever the first launch does not write.  (The bidirectional run has the plain kernel only.)
static int flow_level_fused(ofc_flow *f, FlowBatch &b, const FlowLevel &lv)
{
    hipStream_t s = f->stream;
    const LevelGeom &g = f->geom[lv.k];
    const int npair = b.npair, ws = f->prm.winsize, iters = f->prm.iterations;
    const float *R = f->R.as<float>() + f->offR[lv.k];
    const size_t strideR = 5 * (size_t)g.w * g.h;
    const FlowCoarse coarse = {lv.prev.f, lv.pw, lv.ph, (float)(1. / f->prm.pyr_scale)};
    const FlowHalves tmp = flow_halves(f->flowC, b, lv);
    const bool two = !b.bidir && f->fuse2 && ws == 15 && g.w >= f->fuse2_min_w;
    const bool w3 = !b.bidir && f->w3 && ws == 15 && g.w >= f->w3_min_w;
    int plan[64], L = 0;
    for (int i = 0; i < iters;) {
        const int n = (two && i > 0 && iters - i >= 2) ? 2 : 1;
        plan[L++] = n;
        i += n;
    }
    FlowHalves cur;
    for (int l = 0; l < L; l++) {
        const FlowHalves nxt = ((L - 1 - l) & 1) ? tmp : lv.dst;
        const bool ups = l == 0 && lv.prev.f;
        if (l == 0 && !ups) {
            cur = (nxt == lv.dst) ? tmp : lv.dst;
            OFC_TRY(flow_zero(cur, b, lv, s));
        }
        if (b.bidir) {
            OFC_TRY(launch_flow_iter_bidir(R, strideR, ups ? nullptr : cur.f, ups ? nullptr : cur.b, nxt.f, nxt.b, npair, g.w, g.h, ws, s,
                                           ups ? coarse : FlowCoarse(), ups ? lv.prev.b : nullptr));
        } else if (ups) {
            OFC_TRY(launch_flow_iter(R, strideR, nullptr, nxt.f, npair, g.w, g.h, ws, s, coarse));
        } else if (flow_launch_carries_sums(f, b, lv, l == L - 1, plan[l], ups, w3)) {
            // the field's column sums ride in the epilogue of the iteration that writes it
            const size_t need = (size_t)flow_iter_max_grid(g.w, g.h, npair, ws) * 2;
            OFC_TRY(reserve(f->uv_scratch, need * sizeof(double)));
            // the launch is told what the buffer holds, not what this call needs: its own check then guards the records
            const FlowSums sums = {b.sums, f->uv_scratch.as<double>(), f->uv_scratch.bytes / sizeof(double)};
            OFC_TRY(launch_flow_iter(R, strideR, cur.f, nxt.f, npair, g.w, g.h, ws, s, FlowCoarse(), sums));
            b.sums = nullptr;
        } else if (plan[l] == 2) {
            OFC_TRY(launch_flow_iter2(R, strideR, cur.f, nxt.f, npair, g.w, g.h, ws, s));
        } else if (w3) {
            OFC_TRY(launch_flow_iter_w3(R, strideR, cur.f, nxt.f, npair, g.w, g.h, ws, s));
        } else {
            OFC_TRY(launch_flow_iter(R, strideR, cur.f, nxt.f, npair, g.w, g.h, ws, s));
        }
        cur = nxt;
    }
    return OFC_OK;
}

// the matrices of both directions from the flow in `cur`: M holds 2 npair pairs, its second half filled with the frames swapped
static int flow_staged_matrices(ofc_flow *f, const FlowBatch &b, const FlowLevel &lv, const FlowHalves &cur)
{
    const LevelGeom &g = f->geom[lv.k];
    const float *R = f->R.as<float>() + f->offR[lv.k];
    const size_t strideR = 5 * (size_t)g.w * g.h;
    float *M = f->M.as<float>();
    OFC_TRY(launch_update_matrices(R, R + strideR, strideR, cur.f, M, b.npair, g.w, g.h, f->stream));
    if (b.bidir) OFC_TRY(launch_update_matrices(R + strideR, R, strideR, cur.b, M + strideR * b.npair, b.npair, g.w, g.h, f->stream));
    return OFC_OK;
}

// A level's iterations with the staged kernels, in place in lv.dst.  Bidirectional: the per-field kernels take both halves in
// one launch where the halves are adjacent (every level but 0), and in two launches of the same strip height otherwise.
static int flow_level_staged(ofc_flow *f, const FlowBatch &b, const FlowLevel &lv)
{
    hipStream_t s = f->stream;
    const LevelGeom &g = f->geom[lv.k];
    const int npair = b.npair, nfield = b.nfield(), ws = f->prm.winsize, iters = f->prm.iterations;
    const float mul = (float)(1. / f->prm.pyr_scale);
    const FlowHalves cur = lv.dst;
    const bool one = !b.bidir || cur.b == cur.f + lv.half;
    if (!lv.prev.f) {
        OFC_TRY(flow_zero(cur, b, lv, s));
    } else if (one) {
        OFC_TRY(launch_flow_resize(lv.prev.f, cur.f, nfield, lv.pw, lv.ph, g.w, g.h, mul, s));
    } else {
        OFC_TRY(launch_flow_resize(lv.prev.f, cur.f, npair, lv.pw, lv.ph, g.w, g.h, mul, s));
        OFC_TRY(launch_flow_resize(lv.prev.b, cur.b, npair, lv.pw, lv.ph, g.w, g.h, mul, s));
    }
    float *M = f->M.as<float>(), *Mb = M + 5 * (size_t)g.w * g.h * npair;
    const int box_rows = (b.bidir && ws < WINSIZE_WIDE_MIN) ? box_default_rows(g.w, g.h, nfield) : 0;
    OFC_TRY(flow_staged_matrices(f, b, lv, cur));
    for (int i = 0; i < iters; i++) {
        if (one) {
            OFC_TRY(launch_box_solve(M, cur.f, nfield, g.w, g.h, ws, box_rows, s));
        } else {
            OFC_TRY(launch_box_solve(M, cur.f, npair, g.w, g.h, ws, box_rows, s));
            OFC_TRY(launch_box_solve(Mb, cur.b, npair, g.w, g.h, ws, box_rows, s));
        }
        if (i < iters - 1) OFC_TRY(flow_staged_matrices(f, b, lv, cur));
    }
    return OFC_OK;
}

// The fallback for the column sums when no launch carried them (one iteration per level, staged mode, another winsize, one of
// the experimental engines): one sweep over the finished forward fields gives the same two sums.
static int flow_sums_sweep(ofc_flow *f, const FlowBatch &b)
{
    const int64_t N = (int64_t)b.npair * f->W * f->H;
    const int max_blocks = 1024;    // the scratch is sized for the most records a sweep writes (16 KiB), whatever this call needs
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(N / 4, 256), max_blocks));
    OFC_TRY(reserve(f->uv_scratch, sizeof(double) * 2 * max_blocks));
    OFC_TRY(launch_lloyd_colstats(b.fwd, OFC_F32, N, 2, nullptr, 0, f->uv_scratch.as<double>(), nblocks, f->stream));
    return launch_reduce_records(f->uv_scratch.as<double>(), nblocks, 2, b.sums, f->stream);
}

// One batch: the front end of every level over the n_frames frames, then the iterations, coarsest level first.  With bwd_dev
// the batch is bidirectional (FlowBatch).
static int flow_run(ofc_flow *f, const uint8_t *frames_dev, int n_frames, float *flow_dev, double *uv_sum_dev = nullptr,
                    float *bwd_dev = nullptr)
{
    FlowBatch b = {frames_dev, n_frames - 1, bwd_dev != nullptr, flow_dev, bwd_dev, uv_sum_dev};
    hipStream_t s = f->stream;
    if (b.bidir) OFC_TRY(flow_reserve_bidir(f));
    if (f->front_overlap) {     // the coarse levels' front ends aside, and the level-0 front end beside them on the main stream
        OFC_TRY(flow_coarse_front_ends(f, b));
        OFC_TRY(flow_front_end(f, b, 0, s));
    }
    FlowLevel lv;
    for (int k = f->levels; k >= 0; k--) {
        const LevelGeom &g = f->geom[k];
        lv.k = k;
        lv.half = 2 * (size_t)g.w * g.h * b.npair;
        if (k == 0) { lv.dst.f = b.fwd; lv.dst.b = b.bwd; }
        else lv.dst = flow_halves(((f->levels - k) & 1) ? f->flowB : f->flowA, b, lv);
        if (!f->front_overlap) {
            OFC_TRY(flow_front_end(f, b, k, s));
        } else if (k >= 1) {
            // after the wait at level 1 the side stream is joined: whatever a caller could wait for is reachable from `s`
            OFC_HIP(hipStreamWaitEvent(s, f->ready[k], 0));
        }
        OFC_TRY(f->fused ? flow_level_fused(f, b, lv) : flow_level_staged(f, b, lv));
        lv.prev = lv.dst;
        lv.pw = g.w; lv.ph = g.h;
    }
    if (b.sums) OFC_TRY(flow_sums_sweep(f, b));
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

// what every ofc_flow_calc_frames_dev* form checks first; pointers_ok: none of that form's pointers is null
static int flow_batch_check(const ofc_flow *f, bool pointers_ok, int n_frames)
{
    OFC_REQUIRE(f && pointers_ok, "null pointer");
    OFC_REQUIRE(n_frames >= 2 && n_frames - 1 <= f->max_batch, "n_frames-1 = %d pairs not in [1, max_batch=%d]",
                n_frames - 1, f->max_batch);
    return OFC_OK;
}

// The walk ofc_flow_create runs over an engine's levels before it allocates anything: every limit the launches of
// flow_run apply that follows from the frame size and the parameters alone, asked of the same functions the launches
// ask (level_image_check over level_image_plan, flow_iter_check), coarsest level first as flow_run visits them.  A refusal
// names the level and the limit.  (Engine buffers are hipMalloc'ed, so the level images see dword-aligned frames; a level
// that takes a decimation path when aligned also fits the general path's limits, so the answer does not depend on that.)
static int flow_levels_check(int W, int H, const ofc_fb_params &p, const LevelGeom *geom, int levels, bool fused, bool fuse_level0)
{
    for (int k = levels; k >= 0; k--) {
        const LevelGeom &g = geom[k];
        int rc = OFC_OK;
        if (!(k == 0 && fuse_level0 && polyexp_u8_ok(W, H, g))) rc = level_image_check(W, H, g, true);
        if (rc == OFC_OK && fused) rc = flow_iter_check(g.w, g.h, p.winsize);
        if (rc == OFC_OK) continue;
        const std::string why = ofc_last_error();
        if (g.ksize > 31) {
            int ok = k;         // the deepest level whose blur fits: the `levels` this pyr_scale allows at this size
            while (ok > 0 && geom[ok].ksize > 31) ok--;
            set_error("pyramid level %d (%dx%d, sigma %.3g) of %dx%d at pyr_scale %g: %s; levels <= %d is supported with this "
                      "pyr_scale (a level may shrink the frame by less than 13.6x)", k, g.w, g.h, g.sigma, W, H, p.pyr_scale,
                      why.c_str(), ok);
        } else {
            set_error("pyramid level %d (%dx%d) of %dx%d at pyr_scale %g: %s", k, g.w, g.h, W, H, p.pyr_scale, why.c_str());
        }
        return rc;
    }
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
    OFC_TRY(check_frame_and_fb_params(prm, W, H));
    OFC_REQUIRE(max_batch >= 1 && max_batch <= 4096, "max_batch out of range");
    OFC_REQUIRE((prm.winsize & 1) && prm.winsize >= 5, "winsize must be odd and >= 5");
    std::unique_ptr<ofc_flow, void (*)(ofc_flow_t *)> f(new ofc_flow, ofc_flow_destroy);   // a failure below leaves no stream or event behind
    f->device = device; f->W = W; f->H = H; f->max_batch = max_batch; f->prm = prm;
    f->levels = pyramid_levels(W, H, prm);
    for (int k = 0; k <= f->levels; k++) f->geom.push_back(level_geometry(W, H, prm, k));
    const FlowSwitches sw = flow_read_switches();
    f->fused = prm.winsize <= 15 && !sw.staged;
    f->fuse_level0 = !sw.staged;                    // the staged mode also keeps the separate level-0 image
    f->w3 = sw.w3; f->w3_min_w = sw.w3_min_w;
    f->fuse2 = sw.fuse2; f->fuse2_min_w = sw.fuse2_min_w;
    f->use_graph = sw.graph;
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
    // The overlap is on unless its switch forces the serial order, when there is a coarse level to run aside, the order is
    // not captured into a graph (a capture must stay one chain), and the slices together stay within 1.5 x the shared
    // buffers: a deep pyramid at a pyr_scale near 1 must not multiply the engine's memory.
    const FlowSlices sl = flow_slice_layout(*f);
    f->front_overlap = sw.front_overlap && f->levels >= 1 && !f->use_graph && 2 * (sl.nI + sl.nR) <= 3 * (nI + nR);
    if (f->front_overlap) {
        f->offI = sl.offI; f->offR = sl.offR;
        nI = sl.nI; nR = sl.nR;
    }
    f->pyramid_fused = sw.pyramid_fused && f->front_overlap && f->levels <= 3 &&
                       pyramid_dec_levels(W, H, f->geom.data(), f->levels, true) == f->levels;
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
    flow_drop_graphs(f);
    delete f;
}

int ofc_flow_calc_frames_dev(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *flow_dev)
{
    OFC_TRY(flow_batch_check(f, frames_dev && flow_dev, n_frames));
    OFC_TRY(ensure_device(f->device));
    return flow_run_cached(f, frames_dev, n_frames, flow_dev, nullptr);
}

int ofc_flow_calc_frames_dev_stats(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *flow_dev, double *uv_sum_dev)
{
    OFC_TRY(flow_batch_check(f, frames_dev && flow_dev && uv_sum_dev, n_frames));
    OFC_TRY(ensure_device(f->device));
    return flow_run_cached(f, frames_dev, n_frames, flow_dev, uv_sum_dev);
}

static int flow_calc_bidir(ofc_flow_t *f, const uint8_t *frames_dev, int n_frames, float *fwd_dev, float *bwd_dev, double *uv_sum_dev)
{
    OFC_TRY(flow_batch_check(f, frames_dev && fwd_dev && bwd_dev, n_frames));
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

}  // extern "C"
