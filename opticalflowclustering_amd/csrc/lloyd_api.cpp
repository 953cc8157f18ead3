// lloyd_api.cpp -- C ABI of libofc.so, part 2: Lloyd k-means drivers (streaming shape).
// Control flow = sklearn's _kmeans_single_lloyd (_kmeans.py:624-752) around the kernels of
// lloyd_kernels.hip; see include/ofc.h for the reference call sites.
#include "host_util.h"
#include "lloyd_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>

namespace ofc {

// work-groups of a streaming sweep: enough lanes to keep the memory system full, few enough that the fixed-order record
// reduction stays short (it is a visible share of an iteration on a 1/8 shard)
static int lloyd_grid(int64_t N)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(N / 4, 256), N >= (200ll << 20) ? 2048 : 1024));
}

static size_t dtype_size(int dtype) { return dtype == OFC_U8 ? 1 : (dtype == OFC_F32 ? 4 : 8); }

// Per-device scratch, created once and reused by every fit: creating/destroying a HIP stream (1.5-6 ms) and
// pinned memory per call dominated small fits (rocprof hip-trace of a 38-frame shard).
struct LloydScratch {
    DevBuf state, partial, tot, tot_local, excl, far, labels;
    DevBuf tile_block;                   // lloyd_tiles.hip: the tile (and group) records, rebuilt by every fit (k_tile_meta)
    DevBuf tile_meta;                    // k_tile_meta's reduced record (4 doubles)
    DevBuf kpp_closest, kpp_cs, kpp_ss;  // lloyd_seed.hip: closest[N], chunk sums [8][N / OFC_KPP_CHUNK], their sums per 1024
    DevBuf kpp_io;                       // seeding: [8 indices | 8 x LLOYD_DMAX rows | 192 doubles of all-reduce staging]
    double prune_stats[6] = {0, 0, 0, 0, 0, 0};   // of the last fit, see ofc_lloyd_prune_stats
    LloydStatus *status = nullptr;       // pinned, device-visible; one slot per iteration of a window
    LloydStatus *status_dev = nullptr;
    hipStream_t stream = nullptr;
    bool ready = false;
    std::mutex mu;                       // fits on one device share this scratch: serialised
    int init()
    {
        if (ready) return OFC_OK;
        constexpr int NVMAX = LLOYD_NVMAX;
        OFC_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        OFC_TRY(state.alloc(sizeof(LloydState)));
        OFC_TRY(partial.alloc(sizeof(double) * 2048 * NVMAX));
        OFC_TRY(tot.alloc(sizeof(double) * (NVMAX + 8)));
        OFC_TRY(tot_local.alloc(sizeof(double) * (NVMAX + 8)));
        OFC_TRY(excl.alloc(sizeof(int64_t) * LLOYD_KMAX));
        OFC_TRY(far.alloc(sizeof(double) * 2 * 2048));
        OFC_TRY(tile_meta.alloc(sizeof(double) * 8));
        OFC_HIP(hipHostMalloc((void **)&status, sizeof(LloydStatus) * LLOYD_WINDOW, hipHostMallocMapped));
        OFC_HIP(hipHostGetDevicePointer((void **)&status_dev, status, 0));
        ready = true;
        return OFC_OK;
    }
    // The records of the tile sweeps over N samples: box 16 + sum 16 + scatter 8 B per 64-sample tile and, for a stack of
    // fields of width W > 0, the same per 512-sample group.  One block, grown as a whole: a failed allocation leaves it
    // empty (DevBuf::alloc releases first), so no later fit can meet one array that grew next to one that did not.
    int tile_bufs(int64_t N, int W, LloydFieldBufs &f)
    {
        const size_t nt = (size_t)(N >> 6), ng = W > 0 ? nt >> 3 : 0;
        const size_t goff = (nt * 40 + 15) & ~(size_t)15, need = goff + ng * 40 + 16;
        OFC_TRY(reserve(tile_block, need));
        char *p = tile_block.as<char>();
        f.box = p;
        f.tsum = p + nt * 16;
        f.tsq = p + nt * 32;
        f.gbox = p + goff;
        f.gsum = p + goff + ng * 16;
        f.gsq = p + goff + ng * 32;
        f.W = W;
        return OFC_OK;
    }
};

// OFC_LLOYD_PRUNE: 0 = off (every sweep is k_lloyd_assign's), 1 = auto (default: tile sweeps for f32 d=2 k<=8 streams of
// >= 2^20 samples, pruning switched on and off by the device-side policy in k_lloyd_update), 2 = as auto for any N,
// 3 = every tile sweep after the first runs pruned whatever the share of tiles that pass (tests: worst cases)
static int prune_policy_for(int dtype, int64_t N, int d, int k)
{
    if (!lloyd_tiles_supported(dtype, d, k) || N < 64) return LLOYD_PRUNE_OFF;
    const char *e = getenv("OFC_LLOYD_PRUNE");
    const int v = (e && e[0] >= '0' && e[0] <= '3' && !e[1]) ? e[0] - '0' : LLOYD_PRUNE_AUTO;
    if (v == LLOYD_PRUNE_AUTO && N < (1ll << 20)) return LLOYD_PRUNE_OFF;
    return v;
}

static LloydScratch &scratch_for(int device) { return device_scratch<LloydScratch>(device); }

// empty-cluster relocation (_k_means_common.pyx:167-211) on the all-reduced totals `tot`.
// Returns with `tot` patched on the device (or untouched when the farthest distance is 0).
// wdev != nullptr: the fit is weighted.  The farthest sample is still found by its UNWEIGHTED distance; it moves with its
// weight: sums[old] -= x*w, sums[new] = x*w, wk[new] = w, wk[old] -= w (_k_means_common.pyx:197-211), the product rounded
// on its own.  Under a communicator the owner's broadcast carries the weight in one more slot.
static int relocate_empty(LloydScratch &sc, const void *X, int dtype, int64_t N, int d, int k, int kmax,
                          int nblocks, const uint8_t *labels, const double *mean_h, const void *wdev = nullptr,
                          int w_dtype = OFC_F32)
{
    hipStream_t s = sc.stream;
    const int NV = lloyd_record_len(kmax, d);
    std::vector<double> tot(NV);
    OFC_HIP(hipMemcpyAsync(tot.data(), sc.tot.p, sizeof(double) * NV, hipMemcpyDeviceToHost, s));
    OFC_HIP(hipStreamSynchronize(s));
    double *w = tot.data() + kmax * d;
    LloydState *st = sc.state.as<LloydState>();
    const double *c_old = st->centers;          // device address of the member array
    std::vector<int64_t> excl;
    std::vector<double> blk(2 * nblocks);
    bool first = true;
    for (int j = 0; j < k; j++) {
        if (w[j] != 0.0) continue;
        if (!excl.empty())
            OFC_HIP(hipMemcpyAsync(sc.excl.p, excl.data(), sizeof(int64_t) * excl.size(), hipMemcpyHostToDevice, s));
        OFC_TRY(launch_lloyd_farthest(X, dtype, N, d, st, c_old, labels, sc.excl.as<int64_t>(), (int)excl.size(),
                                      sc.far.as<double>(), nblocks, s));
        OFC_HIP(hipMemcpyAsync(blk.data(), sc.far.p, sizeof(double) * 2 * nblocks, hipMemcpyDeviceToHost, s));
        OFC_HIP(hipStreamSynchronize(s));
        double best = -1;
        int64_t bi = -1;
        for (int b = 0; b < nblocks; b++) {
            const double v = blk[2 * b];
            const int64_t i = (int64_t)blk[2 * b + 1];
            if (i < 0) continue;
            if (v > best || (v == best && i < bi)) { best = v; bi = i; }
        }
        // global winner across ranks: max distance, ties -> lowest rank (= lowest global index)
        double rec[LLOYD_DMAX + 3];   // [x_c[d] | old label | weight (weighted fits only)]
        const int nrec = d + 1 + (wdev ? 1 : 0);
        int owner = 1;
        if (dist_active()) {
            double *dv = sc.far.as<double>();
            double g = best;
            OFC_HIP(hipMemcpyAsync(dv, &g, sizeof(double), hipMemcpyHostToDevice, s));
            OFC_TRY(dist_allreduce_f64(dv, 1, DIST_MAX, s));
            OFC_HIP(hipMemcpyAsync(&g, dv, sizeof(double), hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
            double r = (bi >= 0 && best == g) ? (double)dist_rank() : 1e300;
            OFC_HIP(hipMemcpyAsync(dv, &r, sizeof(double), hipMemcpyHostToDevice, s));
            OFC_TRY(dist_allreduce_f64(dv, 1, DIST_MIN, s));
            OFC_HIP(hipMemcpyAsync(&r, dv, sizeof(double), hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
            owner = ((int)r == dist_rank()) && bi >= 0 && best == g;
            best = g;
        }
        if (first && !(best > 0)) return OFC_OK;   // np.max(distances) == 0: relocating is pointless
        first = false;
        memset(rec, 0, sizeof(rec));
        if (owner) {
            unsigned char raw[LLOYD_DMAX * 8];
            uint8_t lab;
            OFC_HIP(hipMemcpyAsync(raw, (const char *)X + (size_t)bi * d * dtype_size(dtype), d * dtype_size(dtype),
                                   hipMemcpyDeviceToHost, s));
            OFC_HIP(hipMemcpyAsync(&lab, labels + bi, 1, hipMemcpyDeviceToHost, s));
            double wraw = 1.0;
            float wraw32 = 1.0f;
            if (wdev && w_dtype == OFC_F32)
                OFC_HIP(hipMemcpyAsync(&wraw32, (const float *)wdev + bi, sizeof(float), hipMemcpyDeviceToHost, s));
            else if (wdev)
                OFC_HIP(hipMemcpyAsync(&wraw, (const double *)wdev + bi, sizeof(double), hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
            for (int f = 0; f < d; f++) {
                double v = dtype == OFC_U8 ? (double)raw[f]
                         : dtype == OFC_F32 ? (double)((float *)raw)[f] : ((double *)raw)[f];
                rec[f] = v - mean_h[f];
            }
            rec[d] = (double)lab;
            if (wdev) rec[d + 1] = w_dtype == OFC_F32 ? (double)wraw32 : wraw;
            excl.push_back(bi);
        }
        if (dist_active()) {
            double *dv = sc.far.as<double>();
            OFC_HIP(hipMemcpyAsync(dv, rec, sizeof(double) * nrec, hipMemcpyHostToDevice, s));
            OFC_TRY(dist_allreduce_f64(dv, nrec, DIST_BCAST, s));
            OFC_HIP(hipMemcpyAsync(rec, dv, sizeof(double) * nrec, hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
        }
        const int old = (int)rec[d];
        const double wt = wdev ? rec[d + 1] : 1.0;
        for (int f = 0; f < d; f++) {
            const double xw = rec[f] * wt;      // a statement of its own: rounded before it is subtracted (x * 1 is x)
            tot[old * d + f] -= xw;
            tot[j * d + f] = xw;
        }
        w[j] = wt;
        w[old] -= wt;
    }
    OFC_HIP(hipMemcpyAsync(sc.tot.p, tot.data(), sizeof(double) * NV, hipMemcpyHostToDevice, s));
    OFC_HIP(hipStreamSynchronize(s));
    return OFC_OK;
}

static int lloyd_fit_dev(int device, const void *X, int dtype, int64_t N, int d, int k, const double *init,
                         int max_iter, double tol_rel, double *centers, uint8_t *labels_dev,
                         double *inertia, int *n_iter, const double *colsum = nullptr, const void *wdev = nullptr,
                         int w_dtype = OFC_F32, int field_w = 0, int field_h = 0, int64_t n_fields = 0)
{
    OFC_REQUIRE(X && init && centers, "null pointer");
    OFC_REQUIRE(dtype >= OFC_U8 && dtype <= OFC_F64, "bad dtype %d", dtype);
    OFC_REQUIRE(!wdev || w_dtype == OFC_F32 || w_dtype == OFC_F64, "bad weight dtype %d (OFC_F32 or OFC_F64)", w_dtype);
    OFC_REQUIRE(d >= 1 && k >= 1 && max_iter >= 1 && N >= 0, "bad shape");
    if (d > LLOYD_DMAX || k > LLOYD_KMAX) {
        set_error("k=%d, d=%d outside the kernels' range (k <= %d, d <= %d)", k, d, LLOYD_KMAX, LLOYD_DMAX);
        return OFC_EUNSUPPORTED;
    }
    OFC_TRY(ensure_device(device));
    const int kmax = lloyd_kmax(k);
    const int NV = lloyd_record_len(kmax, d);
    LloydScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    OFC_TRY(sc.init());
    hipStream_t s = sc.stream;
    const int nblocks = lloyd_grid(N);
    if (!labels_dev) {
        OFC_TRY(reserve(sc.labels, (size_t)std::max<int64_t>(N, 1)));
        labels_dev = sc.labels.as<uint8_t>();
    }
    LloydState *st = sc.state.as<LloydState>();
    OFC_HIP(hipMemsetAsync(st, 0, sizeof(LloydState), s));
    double *tot = sc.tot.as<double>();

    // ---- column mean (X.mean(axis=0), _kmeans.py:1478-1484) and tol (_tolerance, :279-287) ----
    double hbuf[LLOYD_DMAX + 1], mean_h[LLOYD_DMAX];
    if (colsum) {           // the caller already has this rank's column sums (the flow kernels' epilogue): no sweep
        OFC_HIP(hipMemcpyAsync(tot, colsum, sizeof(double) * d, hipMemcpyHostToDevice, s));
    } else {
        OFC_TRY(launch_lloyd_colstats(X, dtype, N, d, st->mean, 0, sc.partial.as<double>(), nblocks, s));
        OFC_TRY(launch_reduce_records(sc.partial.as<double>(), nblocks, d, tot, s));
    }
    double nloc = (double)N;
    OFC_HIP(hipMemcpyAsync(tot + d, &nloc, sizeof(double), hipMemcpyHostToDevice, s));
    OFC_TRY(dist_allreduce_f64(tot, d + 1, DIST_SUM, s));
    OFC_HIP(hipMemcpyAsync(hbuf, tot, sizeof(double) * (d + 1), hipMemcpyDeviceToHost, s));
    OFC_HIP(hipStreamSynchronize(s));
    const double Ng = hbuf[d];
    if (Ng < (double)k) {
        set_error("n_samples=%.0f should be >= n_clusters=%d.", Ng, k);
        return OFC_EINVAL;
    }
    for (int f = 0; f < d; f++) mean_h[f] = hbuf[f] / Ng;
    OFC_HIP(hipMemcpyAsync(st->mean, mean_h, sizeof(double) * d, hipMemcpyHostToDevice, s));

    // ---- centred init ----
    double c0[LLOYD_KMAX * LLOYD_DMAX];
    for (int j = 0; j < k * d; j++) c0[j] = init[j] - mean_h[j % d];
    OFC_HIP(hipMemcpyAsync(st->centers, c0, sizeof(double) * k * d, hipMemcpyHostToDevice, s));
    // a weighted fit runs the plain sweeps: the tile metadata (cached per-tile sums) is unweighted
    const int prune = wdev ? LLOYD_PRUNE_OFF : prune_policy_for(dtype, N, d, k);
    // X is a stack of fields that the 2-D tiles fit (lloyd_field.h): the tile sweeps take their field form.  Any other
    // shape runs the 64 x 1 tiles; the result is the same either way.
    const bool field = prune && field_w > 0 && field_geometry_ok(field_w, field_h, n_fields);
    LloydFieldBufs tb = {};
    if (prune) OFC_TRY(sc.tile_bufs(N, field ? field_w : 0, tb));
    auto tiles_launch = [&](uint8_t *lab, int what, const double *meta) -> int {
        if (field) return launch_lloyd_tiles_field((const float *)X, N, k, st, tb, lab, sc.partial.as<double>(), nblocks, what, meta, s);
        return launch_lloyd_tiles((const float *)X, N, k, st, tb.box, tb.tsum, tb.tsq, lab, sc.partial.as<double>(), nblocks, what,
                                  meta, s);
    };
    for (double &v : sc.prune_stats) v = 0;
    OFC_TRY(launch_lloyd_set_centers(st, k, d, s, prune));
    // ---- Lloyd iterations ----
    // sklearn stops on `labels == labels_old` (strict) before it looks at the centre shift (_kmeans.py:716-728).  While
    // no cluster is empty that test is redundant: equal labels give bit-equal sums (fixed reduction order), hence
    // centers_new == centers, shift_tot == 0 <= tol, and the tol test stops in the SAME iteration; the E-step sklearn
    // then repeats (mode 2 below) reproduces the labels.  So the iterations stream X only (mode 3: no label read or
    // write, 8 instead of 10 B/point for float2 data).  The labelled form (mode 1) takes over from the first
    // iteration that meets an empty cluster: relocation needs the labels, and a relocated centre breaks the
    // equal-labels => zero-shift argument.  That iteration itself cannot be a strict stop: equal labels would mean the
    // previous iteration had the same empty cluster.
    //
    // The convergence test runs on the device (k_lloyd_update) and the host enqueues LLOYD_WINDOW iterations per
    // synchronisation (windows of 4, 8, 16, 16, ...): an iteration behind the one that converged (or met an empty cluster)
    // finds st->halt set and does nothing.  One host round trip per window instead of one per iteration (18 us each -- a tenth of an
    // iteration on a 1/8 shard); every rank takes the same decisions because they derive from all-reduced totals.
    bool strict = false, labelled = false, stop = false;
    int tiles_next = LLOYD_TILES_FULL;   // how the device would run the next tile sweep: decides the form of the final E-step
    const bool trace = getenv("OFC_LLOYD_TRACE") != nullptr;
    int it = 0;
    const int *halt = &st->halt;
    double *tot_local = dist_has_comm() ? sc.tot_local.as<double>() : tot;
    int window = 4;                       // 4, 8, 16, 16, ...: an 11-iteration fit costs two host round trips, and a fit
                                          // that meets its empty cluster early (iteration 1-2, typically) wastes few
    while (it < max_iter && !stop) {
        const int nwin = std::min(window, max_iter - it);
        window = std::min(2 * window, LLOYD_WINDOW);
        for (int w = 0; w < nwin; w++) sc.status[w].valid = 0;
        for (int w = 0; w < nwin; w++) {
            // label-less sweeps of a (u,v) stream go tile by tile: iteration 0 builds the tile metadata, the later ones
            // run in the mode k_lloyd_update chose from the previous iteration's tile counts (lloyd_tiles.hip)
            const int tiles = (prune && !labelled) ? (it + w == 0 ? 1 : 2) : 0;
            if (tiles == 1) {      // is the field coherent enough? then tile metadata + column sums of squares, then iteration 0
                OFC_TRY(tiles_launch(nullptr, LLOYD_WHAT_PROBE, nullptr));
                OFC_TRY(tiles_launch(nullptr, LLOYD_WHAT_META, nullptr));
                OFC_TRY(launch_reduce_records(sc.partial.as<double>(), nblocks, 2, sc.tile_meta.as<double>(), s));
            }
            if (tiles)
                OFC_TRY(tiles_launch(nullptr, LLOYD_WHAT_SWEEP, tiles == 1 ? sc.tile_meta.as<double>() : nullptr));
            else if (wdev)
                OFC_TRY(launch_lloyd_assign_w(X, dtype, wdev, w_dtype, N, d, k, st, labels_dev, sc.partial.as<double>(),
                                              nblocks, labelled ? 1 : 3, it + w == 0, s));
            else
                OFC_TRY(launch_lloyd_assign(X, dtype, N, d, k, st, labels_dev, sc.partial.as<double>(), nblocks,
                                            labelled ? 1 : 3, it + w == 0, s));
            // with a communicator the local record goes to its own buffer and the collective writes `tot`: an iteration
            // behind the halt flag then re-reduces the same local records into the same totals (in place it would sum
            // the totals of all ranks again, and a stalled iteration's `tot` is what relocate_empty reads)
            OFC_TRY(launch_reduce_records(sc.partial.as<double>(), nblocks, NV, tot_local, s, halt));
            OFC_TRY(dist_allreduce_f64(tot_local, tot, NV, DIST_SUM, s));
            OFC_TRY(launch_lloyd_update(st, tot, k, d, 0, labelled, it + w == 0, Ng, tol_rel, sc.status_dev + w, s, tiles));
        }
        OFC_HIP(hipStreamSynchronize(s));
        int done = nwin;                      // iterations of this window that really ran
        for (int w = 0; w < nwin; w++) {
            LloydStatus &S = sc.status[w];
            if (!S.valid) { set_error("internal: Lloyd iteration %d did not run", it + w); return OFC_EHIP; }
            if (trace)
                fprintf(stderr, "[ofc lloyd] it %d tiles_mode %d tested %.0f pure %.0f shift %.3e empty %d\n", it + w,
                        S.tiles_mode, S.tiles_tested, S.tiles_pure, S.shift_tot, S.n_empty);
            if (S.tiles_mode != -1) {
                tiles_next = S.tiles_next;
                sc.prune_stats[0] += 1;                                   // sweeps that went tile by tile
                if (S.tiles_mode == LLOYD_TILES_PRUNED) {
                    sc.prune_stats[1] += 1;                               // ... of them pruned
                    sc.prune_stats[2] += S.tiles_tested;                  // tiles tested / skipped by the pruned sweeps
                    sc.prune_stats[3] += S.tiles_pure;
                } else if (S.tiles_mode == LLOYD_TILES_PROBE) {
                    sc.prune_stats[4] += 1;
                }
            }
            if (wdev && it + w == 0) {
                // sklearn refuses weights whose sum is not positive (_check_sample_weight); here every cluster would be
                // empty and relocated in each of max_iter iterations.  The counts are all-reduced: every rank returns.
                double wsum = 0;
                for (int j = 0; j < k; j++) wsum += S.counts[j];
                if (!(wsum > 0)) { set_error("sum of sample weights must be positive"); return OFC_EINVAL; }
            }
            if (S.n_empty > 0) {              // the device stalled here; iterations w+1.. of the window were no-ops
                const bool was_labelled = labelled;
                if (!labelled) {   // materialise this iteration's labels (st->centers is still the E-step's input)
                    OFC_TRY(launch_lloyd_assign(X, dtype, N, d, k, st, labels_dev, nullptr, nblocks, 0, 0, s));
                    labelled = true;
                }
                OFC_TRY(relocate_empty(sc, X, dtype, N, d, k, kmax, nblocks, labels_dev, mean_h, wdev, w_dtype));
                S.valid = 0;
                OFC_TRY(launch_lloyd_update(st, tot, k, d, 1, was_labelled, it + w == 0, Ng, tol_rel, sc.status_dev + w, s));
                OFC_HIP(hipStreamSynchronize(s));
                done = w + 1;
                if (S.converged) { strict = S.strict != 0; it += w; stop = true; }
                break;
            }
            if (S.converged) { strict = S.strict != 0; it += w; stop = true; break; }
        }
        if (!stop) it += done;
    }
    if (!stop) it = max_iter - 1;        // ran out of iterations: n_iter = max_iter
    // ---- final E-step (only when not strictly converged) and inertia: one sweep ----
    const bool final_tiles = !strict && prune && !labelled && tiles_next == LLOYD_TILES_PRUNED;
    sc.prune_stats[5] = final_tiles ? 1 : 0;
    if (final_tiles)                        // the fit's tile metadata is valid and most tiles pass: those are not read
        OFC_TRY(tiles_launch(labels_dev, LLOYD_WHAT_FINAL, nullptr));
    else if (!strict && wdev)
        OFC_TRY(launch_lloyd_assign_w(X, dtype, wdev, w_dtype, N, d, k, st, labels_dev, sc.partial.as<double>(), nblocks, 2, 0, s));
    else if (!strict)
        OFC_TRY(launch_lloyd_assign(X, dtype, N, d, k, st, labels_dev, sc.partial.as<double>(), nblocks, 2, 0, s));
    else if (wdev)
        OFC_TRY(launch_lloyd_inertia_w(X, dtype, wdev, w_dtype, N, d, st, labels_dev, sc.partial.as<double>(), nblocks, s));
    else
        OFC_TRY(launch_lloyd_inertia(X, dtype, N, d, st, labels_dev, sc.partial.as<double>(), nblocks, s));
    OFC_TRY(launch_reduce_records(sc.partial.as<double>(), nblocks, 1, tot, s));
    OFC_TRY(dist_allreduce_f64(tot, 1, DIST_SUM, s));
    double in = 0, cfin[LLOYD_KMAX * LLOYD_DMAX];
    OFC_HIP(hipMemcpyAsync(&in, tot, sizeof(double), hipMemcpyDeviceToHost, s));
    OFC_HIP(hipMemcpyAsync(cfin, st->centers, sizeof(double) * k * d, hipMemcpyDeviceToHost, s));
    OFC_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < k * d; j++) centers[j] = cfin[j] + mean_h[j % d];
    if (inertia) *inertia = in;
    if (n_iter) *n_iter = it + 1;
    return OFC_OK;
}

static int lloyd_predict_dev(int device, const void *X, int dtype, int64_t N, int d, int k,
                             const double *centers, uint8_t *labels_dev)
{
    OFC_TRY(ensure_device(device));
    if (d > LLOYD_DMAX || k > LLOYD_KMAX || d < 1 || k < 1) {
        set_error("k=%d, d=%d outside the kernels' range (k <= %d, d <= %d)", k, d, LLOYD_KMAX, LLOYD_DMAX);
        return OFC_EUNSUPPORTED;
    }
    DevBuf state;
    OFC_TRY(state.alloc(sizeof(LloydState)));
    LloydState *st = state.as<LloydState>();
    OFC_HIP(hipMemset(st, 0, sizeof(LloydState)));
    OFC_HIP(hipMemcpy(st->centers, centers, sizeof(double) * k * d, hipMemcpyHostToDevice));
    OFC_TRY(launch_lloyd_set_centers(st, k, d, nullptr));
    const int nblocks = lloyd_grid(N);
    OFC_TRY(launch_lloyd_assign(X, dtype, N, d, k, st, labels_dev, nullptr, nblocks, 0, 0, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

static void widen_labels(const uint8_t *src, int64_t N, int32_t *dst)
{
    for (int64_t i = 0; i < N; i++) dst[i] = src[i];
}

}  // namespace ofc

using namespace ofc;

extern "C" {

int ofc_kmeans_fit_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *init,
                       int max_iter, double tol_rel, double *centers, uint8_t *labels_dev, double *inertia,
                       int *n_iter)
{
    return lloyd_fit_dev(device, X_dev, dtype, N, d, k, init, max_iter, tol_rel, centers, labels_dev, inertia, n_iter);
}

/* see include/ofc.h */
int ofc_bench_lloyd_sweep(int device, const float *X_dev, int64_t N, int k, const double *centers, const double *mean,
                          int what, int iters, float *ms_per_launch)
{
    OFC_REQUIRE(X_dev && centers && mean && ms_per_launch && iters >= 1 && N >= 64, "bad arguments");
    OFC_REQUIRE(what >= 0 && what <= 5, "what = %d outside 0..5", what);
    if (!lloyd_tiles_supported(OFC_F32, 2, k)) { set_error("k=%d outside 1..8", k); return OFC_EUNSUPPORTED; }
    OFC_TRY(ensure_device(device));
    LloydScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    OFC_TRY(sc.init());
    hipStream_t s = sc.stream;
    const int nblocks = lloyd_grid(N);
    LloydFieldBufs tb = {};
    OFC_TRY(sc.tile_bufs(N, 0, tb));
    OFC_TRY(reserve(sc.labels, (size_t)N));
    LloydState *st = sc.state.as<LloydState>();
    OFC_HIP(hipMemsetAsync(st, 0, sizeof(LloydState), s));
    double c0[LLOYD_KMAX * LLOYD_DMAX];
    for (int j = 0; j < k * 2; j++) c0[j] = centers[j] - mean[j % 2];
    OFC_HIP(hipMemcpyAsync(st->mean, mean, sizeof(double) * 2, hipMemcpyHostToDevice, s));
    OFC_HIP(hipMemcpyAsync(st->centers, c0, sizeof(double) * k * 2, hipMemcpyHostToDevice, s));
    OFC_TRY(launch_lloyd_set_centers(st, k, 2, s, LLOYD_PRUNE_ALWAYS));
    double *partial = sc.partial.as<double>();
    const float *X = X_dev;
    auto launch = [&]() -> int {
        switch (what) {
        case 0: return launch_lloyd_assign(X, OFC_F32, N, 2, k, st, sc.labels.as<uint8_t>(), partial, nblocks, 3, 0, s);
        case 1: case 5: return launch_lloyd_tiles(X, N, k, st, tb.box, tb.tsum, tb.tsq, nullptr, partial, nblocks, LLOYD_WHAT_SWEEP, nullptr, s);
        case 2: return launch_lloyd_tiles(X, N, k, st, tb.box, tb.tsum, tb.tsq, nullptr, partial, nblocks, LLOYD_WHAT_META, nullptr, s);
        case 3: return launch_lloyd_assign(X, OFC_F32, N, 2, k, st, sc.labels.as<uint8_t>(), partial, nblocks, 2, 0, s);
        default: return launch_lloyd_tiles(X, N, k, st, tb.box, tb.tsum, tb.tsq, sc.labels.as<uint8_t>(), partial, nblocks, LLOYD_WHAT_FINAL, nullptr, s);
        }
    };
    if (what == 1 || what == 4 || what == 5) {      // the pruned sweeps need the tile metadata and the mode flag
        OFC_TRY(launch_lloyd_tiles(X, N, k, st, tb.box, tb.tsum, tb.tsq, nullptr, partial, nblocks, LLOYD_WHAT_META, nullptr, s));
        const int mode = what == 5 ? LLOYD_TILES_FULL : LLOYD_TILES_PRUNED;
        OFC_HIP(hipMemcpyAsync(&st->prune_mode, &mode, sizeof(int), hipMemcpyHostToDevice, s));
    }
    return time_launches(s, iters, launch, ms_per_launch);
}

/* see include/ofc.h */
int ofc_lloyd_prune_stats(int device, double *out6)
{
    OFC_REQUIRE(out6, "null pointer");
    OFC_TRY(ensure_device(device));
    LloydScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    for (int i = 0; i < 6; i++) out6[i] = sc.prune_stats[i];
    return OFC_OK;
}

int ofc_kmeans_fit_dev_stats(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *init,
                             int max_iter, double tol_rel, const double *colsum, double *centers, uint8_t *labels_dev,
                             double *inertia, int *n_iter)
{
    return lloyd_fit_dev(device, X_dev, dtype, N, d, k, init, max_iter, tol_rel, centers, labels_dev, inertia, n_iter, colsum);
}

/* see include/ofc.h */
int ofc_kmeans_fit_dev_field(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *init,
                             int max_iter, double tol_rel, const double *colsum, double *centers, uint8_t *labels_dev,
                             double *inertia, int *n_iter, int W, int H, int64_t n_fields)
{
    OFC_REQUIRE(dtype == OFC_F32 && d == 2, "a stack of (u,v) fields is float32 with d = 2 (got dtype %d, d = %d)", dtype, d);
    OFC_REQUIRE(W >= 1 && H >= 1 && n_fields >= 1 && N / W / H == n_fields && n_fields * W * H == N,
                "N=%lld is not %lld fields of %d x %d", (long long)N, (long long)n_fields, W, H);
    return lloyd_fit_dev(device, X_dev, dtype, N, d, k, init, max_iter, tol_rel, centers, labels_dev, inertia, n_iter, colsum,
                         nullptr, OFC_F32, W, H, n_fields);
}

/* see include/ofc.h */
int64_t ofc_lloyd_field_origin(int64_t tile, int quad, int W)
{
    if (tile < 0 || quad < 0 || quad > 15 || W < FIELD_GW || W % FIELD_GW) return -1;
    return field_quad_origin(tile, quad, W);
}

/* see include/ofc.h */
int ofc_lloyd_field_origins(int64_t tile0, int64_t n_tiles, int W, int64_t *out)
{
    OFC_REQUIRE(out && tile0 >= 0 && n_tiles >= 0 && W >= FIELD_GW && W % FIELD_GW == 0, "bad arguments");
    for (int64_t i = 0; i < n_tiles; i++)
        for (int q = 0; q < 16; q++) out[i * 16 + q] = field_quad_origin(tile0 + i, q, W);
    return OFC_OK;
}

/* see include/ofc.h */
void ofc_lloyd_field_shape(int *tile_w, int *tile_h, int *group_w, int *group_h)
{
    if (tile_w) *tile_w = FIELD_TW;
    if (tile_h) *tile_h = FIELD_TH;
    if (group_w) *group_w = FIELD_GW;
    if (group_h) *group_h = FIELD_GH;
}

// ---- host-driven building blocks ----
namespace {
struct StepCtx {
    DevBuf state, partial, tot, excl, far;
    int nblocks = 1;
    int init(int64_t N, int nv)
    {
        nblocks = lloyd_grid(N);
        OFC_TRY(state.alloc(sizeof(LloydState)));
        OFC_TRY(partial.alloc(sizeof(double) * (size_t)nblocks * std::max(nv, 2)));
        OFC_TRY(tot.alloc(sizeof(double) * (nv + 8)));
        OFC_HIP(hipMemset(state.p, 0, sizeof(LloydState)));
        return OFC_OK;
    }
    int set(const double *mean, const double *centers_c, int k, int d)
    {
        LloydState *st = state.as<LloydState>();
        if (mean) OFC_HIP(hipMemcpy(st->mean, mean, sizeof(double) * d, hipMemcpyHostToDevice));
        if (centers_c) {
            OFC_HIP(hipMemcpy(st->centers, centers_c, sizeof(double) * k * d, hipMemcpyHostToDevice));
            OFC_TRY(launch_lloyd_set_centers(st, k, d, nullptr));
        }
        return OFC_OK;
    }
};
int check_kd(int k, int d)
{
    if (d < 1 || k < 1 || d > LLOYD_DMAX || k > LLOYD_KMAX) {
        set_error("k=%d, d=%d outside the kernels' range (k <= %d, d <= %d)", k, d, LLOYD_KMAX, LLOYD_DMAX);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}
}  // namespace

int ofc_lloyd_colstats_dev(int device, const void *X_dev, int dtype, int64_t N, int d, const double *mean, int pass,
                           double *out)
{
    OFC_REQUIRE(X_dev && out && N >= 0 && (pass == 0 || mean), "bad arguments");
    OFC_TRY(check_kd(1, d));
    OFC_TRY(ensure_device(device));
    StepCtx c;
    OFC_TRY(c.init(N, d));
    OFC_TRY(c.set(pass ? mean : nullptr, nullptr, 1, d));
    LloydState *st = c.state.as<LloydState>();
    OFC_TRY(launch_lloyd_colstats(X_dev, dtype, N, d, st->mean, pass, c.partial.as<double>(), c.nblocks, nullptr));
    OFC_TRY(launch_reduce_records(c.partial.as<double>(), c.nblocks, d, c.tot.as<double>(), nullptr));
    OFC_HIP(hipMemcpy(out, c.tot.p, sizeof(double) * d, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_lloyd_step_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *mean,
                       const double *centers_c, uint8_t *labels_dev, int accumulate, double *record)
{
    OFC_REQUIRE(X_dev && mean && centers_c && labels_dev && (record || !accumulate) && N >= 0, "bad arguments");
    OFC_TRY(check_kd(k, d));
    OFC_TRY(ensure_device(device));
    const int kmax = lloyd_kmax(k), NV = lloyd_record_len(kmax, d);
    StepCtx c;
    OFC_TRY(c.init(N, NV));
    OFC_TRY(c.set(mean, centers_c, k, d));
    LloydState *st = c.state.as<LloydState>();
    OFC_TRY(launch_lloyd_assign(X_dev, dtype, N, d, k, st, labels_dev, c.partial.as<double>(), c.nblocks, accumulate ? 1 : 0, 0, nullptr));
    if (accumulate) {
        OFC_TRY(launch_reduce_records(c.partial.as<double>(), c.nblocks, NV, c.tot.as<double>(), nullptr));
        std::vector<double> t(NV);
        OFC_HIP(hipMemcpy(t.data(), c.tot.p, sizeof(double) * NV, hipMemcpyDeviceToHost));
        for (int j = 0; j < k; j++) {
            for (int f = 0; f < d; f++) record[j * d + f] = t[j * d + f];
            record[k * d + j] = t[kmax * d + j];
        }
        record[k * d + k] = t[kmax * d + kmax];
    } else {
        OFC_HIP(hipStreamSynchronize(nullptr));
    }
    return OFC_OK;
}

int ofc_grid_assign_counts_dev(int device, const float *flow_dev, int W, int H, int n_frames, int rows, int cols, int k,
                               const double *mean, const double *centers_c, int32_t *counts_dev, double *sums_dev)
{
    OFC_REQUIRE(flow_dev && centers_c && counts_dev, "null pointer");
    OFC_REQUIRE(n_frames >= 1 && W >= 1 && H >= 1, "bad size %dx%d x %d frames", W, H, n_frames);
    OFC_REQUIRE(rows >= 1 && cols >= 1 && W >= cols && H >= rows, "grid %dx%d does not fit %dx%d", rows, cols, W, H);
    OFC_TRY(check_uv_model(k, mean, centers_c));
    if ((int64_t)W * H > INT32_MAX) {          // a cell's pixels are numbered in 32 bits
        set_error("frames of %dx%d pixels are not supported (more than 2^31 - 1)", W, H);
        return OFC_EUNSUPPORTED;
    }
    OFC_TRY(ensure_device(device));
    const double zero[2] = {0.0, 0.0};
    StepCtx c;
    OFC_TRY(c.init(0, 2));
    OFC_TRY(c.set(mean ? mean : zero, centers_c, k, 2));
    OFC_TRY(launch_grid_assign_counts(flow_dev, c.state.as<LloydState>(), W, H, n_frames, rows, cols, k, counts_dev, sums_dev,
                                      nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_lloyd_inertia_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *mean,
                          const double *centers_c, const uint8_t *labels_dev, double *inertia)
{
    OFC_REQUIRE(X_dev && mean && centers_c && labels_dev && inertia && N >= 0, "bad arguments");
    OFC_TRY(check_kd(k, d));
    OFC_TRY(ensure_device(device));
    StepCtx c;
    OFC_TRY(c.init(N, 2));
    OFC_TRY(c.set(mean, centers_c, k, d));
    OFC_TRY(launch_lloyd_inertia(X_dev, dtype, N, d, c.state.as<LloydState>(), labels_dev, c.partial.as<double>(), c.nblocks, nullptr));
    OFC_TRY(launch_reduce_records(c.partial.as<double>(), c.nblocks, 1, c.tot.as<double>(), nullptr));
    OFC_HIP(hipMemcpy(inertia, c.tot.p, sizeof(double), hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_lloyd_farthest_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *mean,
                           const double *centers_c, const uint8_t *labels_dev, const int64_t *excl, int n_excl,
                           double *dist2, int64_t *index, double *x_c, int *label)
{
    OFC_REQUIRE(X_dev && mean && centers_c && labels_dev && dist2 && index && x_c && label && N >= 0, "bad arguments");
    OFC_REQUIRE(n_excl >= 0 && n_excl <= LLOYD_KMAX && (n_excl == 0 || excl), "bad exclusion list");
    OFC_TRY(check_kd(k, d));
    OFC_TRY(ensure_device(device));
    StepCtx c;
    OFC_TRY(c.init(N, 2));
    OFC_TRY(c.set(mean, centers_c, k, d));
    OFC_TRY(c.excl.alloc(sizeof(int64_t) * LLOYD_KMAX));
    if (n_excl) OFC_HIP(hipMemcpy(c.excl.p, excl, sizeof(int64_t) * n_excl, hipMemcpyHostToDevice));
    LloydState *st = c.state.as<LloydState>();
    OFC_TRY(launch_lloyd_farthest(X_dev, dtype, N, d, st, st->centers, labels_dev, c.excl.as<int64_t>(), n_excl,
                                  c.partial.as<double>(), c.nblocks, nullptr));
    std::vector<double> blk(2 * c.nblocks);
    OFC_HIP(hipMemcpy(blk.data(), c.partial.p, sizeof(double) * 2 * c.nblocks, hipMemcpyDeviceToHost));
    double best = -1;
    int64_t bi = -1;
    for (int b = 0; b < c.nblocks; b++) {
        const double v = blk[2 * b];
        const int64_t i = (int64_t)blk[2 * b + 1];
        if (i < 0) continue;
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    }
    *dist2 = bi >= 0 ? best : -1;
    *index = bi;
    *label = -1;
    if (bi >= 0) {
        unsigned char raw[LLOYD_DMAX * 8];
        uint8_t lab;
        OFC_HIP(hipMemcpy(raw, (const char *)X_dev + (size_t)bi * d * dtype_size(dtype), d * dtype_size(dtype), hipMemcpyDeviceToHost));
        OFC_HIP(hipMemcpy(&lab, labels_dev + bi, 1, hipMemcpyDeviceToHost));
        for (int f = 0; f < d; f++) {
            double v = dtype == OFC_U8 ? (double)raw[f] : dtype == OFC_F32 ? (double)((float *)raw)[f] : ((double *)raw)[f];
            x_c[f] = v - mean[f];
        }
        *label = lab;
    }
    return OFC_OK;
}

int ofc_kmeans_fit(int device, const void *X, int dtype, int64_t N, int d, int k, const double *init,
                   int max_iter, double tol_rel, double *centers, int32_t *labels, double *inertia, int *n_iter)
{
    OFC_REQUIRE(X && init && centers, "null pointer");
    OFC_REQUIRE(dtype >= OFC_U8 && dtype <= OFC_F64 && d >= 1 && N >= 0, "bad arguments");
    OFC_REQUIRE(N >= k, "n_samples=%lld should be >= n_clusters=%d.", (long long)N, k);
    OFC_TRY(ensure_device(device));
    DevBuf dX, dL;
    const size_t bytes = (size_t)N * d * dtype_size(dtype);
    OFC_TRY(dX.alloc(std::max<size_t>(bytes, 16)));
    OFC_TRY(dL.alloc((size_t)std::max<int64_t>(N, 1)));
    OFC_HIP(hipMemcpy(dX.p, X, bytes, hipMemcpyHostToDevice));
    OFC_TRY(lloyd_fit_dev(device, dX.p, dtype, N, d, k, init, max_iter, tol_rel, centers, dL.as<uint8_t>(), inertia, n_iter));
    if (labels) {
        std::vector<uint8_t> l8((size_t)N);
        OFC_HIP(hipMemcpy(l8.data(), dL.p, (size_t)N, hipMemcpyDeviceToHost));
        widen_labels(l8.data(), N, labels);
    }
    return OFC_OK;
}

int ofc_kmeans_predict(int device, const void *X, int dtype, int64_t N, int d, int k, const double *centers,
                       int32_t *labels)
{
    OFC_REQUIRE(X && centers && labels, "null pointer");
    OFC_REQUIRE(dtype >= OFC_U8 && dtype <= OFC_F64 && d >= 1 && N >= 0 && k >= 1, "bad arguments");
    OFC_TRY(ensure_device(device));
    DevBuf dX, dL;
    const size_t bytes = (size_t)N * d * dtype_size(dtype);
    OFC_TRY(dX.alloc(std::max<size_t>(bytes, 16)));
    OFC_TRY(dL.alloc((size_t)std::max<int64_t>(N, 1)));
    OFC_HIP(hipMemcpy(dX.p, X, bytes, hipMemcpyHostToDevice));
    OFC_TRY(lloyd_predict_dev(device, dX.p, dtype, N, d, k, centers, dL.as<uint8_t>()));
    std::vector<uint8_t> l8((size_t)N);
    OFC_HIP(hipMemcpy(l8.data(), dL.p, (size_t)N, hipMemcpyDeviceToHost));
    widen_labels(l8.data(), N, labels);
    return OFC_OK;
}

/* see include/ofc.h */
int ofc_kpp_candidates(int device, const void *X, int dtype, int64_t N, int d, const double *mean,
                       const int64_t *cand, int n_cand, const double *closest, double *out_min, double *pots)
{
    OFC_REQUIRE(X && mean && cand && out_min && pots && N >= 1, "bad arguments");
    OFC_REQUIRE(dtype >= OFC_U8 && dtype <= OFC_F64, "bad dtype %d", dtype);
    OFC_REQUIRE(n_cand >= 1 && n_cand <= 8, "n_cand %d outside 1..8", n_cand);
    OFC_TRY(check_kd(1, d));
    for (int c = 0; c < n_cand; c++) OFC_REQUIRE(cand[c] >= 0 && cand[c] < N, "candidate index out of range");
    OFC_TRY(ensure_device(device));
    const size_t es = dtype_size(dtype);
    std::vector<double> cc((size_t)n_cand * d);
    for (int c = 0; c < n_cand; c++)
        for (int f = 0; f < d; f++) {
            const char *p = (const char *)X + ((size_t)cand[c] * d + f) * es;
            const double v = dtype == OFC_U8 ? (double)*(const uint8_t *)p
                           : dtype == OFC_F32 ? (double)*(const float *)p : *(const double *)p;
            cc[(size_t)c * d + f] = v - mean[f];
        }
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(N, 256), 1024));
    DevBuf Xd, cl, out, partial, tot;
    OFC_TRY(Xd.alloc((size_t)N * d * es));
    OFC_TRY(out.alloc(sizeof(double) * (size_t)N * n_cand));
    OFC_TRY(partial.alloc(sizeof(double) * 8 * nblocks));
    OFC_TRY(tot.alloc(sizeof(double) * 8));
    OFC_HIP(hipMemcpy(Xd.p, X, (size_t)N * d * es, hipMemcpyHostToDevice));
    if (closest) {
        OFC_TRY(cl.alloc(sizeof(double) * N));
        OFC_HIP(hipMemcpy(cl.p, closest, sizeof(double) * N, hipMemcpyHostToDevice));
    }
    OFC_TRY(launch_kpp_candidates(Xd.p, dtype, N, d, mean, cc.data(), n_cand, closest ? cl.as<double>() : nullptr,
                                  out.as<double>(), partial.as<double>(), nblocks, nullptr));
    OFC_TRY(launch_reduce_records(partial.as<double>(), nblocks, 8, tot.as<double>(), nullptr));
    double t[8];
    OFC_HIP(hipMemcpy(t, tot.p, sizeof(t), hipMemcpyDeviceToHost));
    for (int c = 0; c < n_cand; c++) pots[c] = t[c];
    OFC_HIP(hipMemcpy(out_min, out.p, sizeof(double) * (size_t)N * n_cand, hipMemcpyDeviceToHost));
    return OFC_OK;
}

/* ---- k-means++ seeding on resident samples, see include/ofc.h and lloyd_seed.hip ---- */
namespace {
constexpr int KPP_IO_ROWS = 8, KPP_IO_STAGE = 8 + 8 * LLOYD_DMAX, KPP_IO_LEN = KPP_IO_STAGE + 192;

// all-reduce of a few host doubles through the seeding scratch (no-op without a communicator)
int kpp_exchange(LloydScratch &sc, double *h, int count, int op)
{
    if (!dist_active()) return OFC_OK;
    double *dv = sc.kpp_io.as<double>() + KPP_IO_STAGE;
    OFC_HIP(hipMemcpyAsync(dv, h, sizeof(double) * count, hipMemcpyHostToDevice, sc.stream));
    OFC_TRY(dist_allreduce_f64(dv, count, op, sc.stream));
    OFC_HIP(hipMemcpyAsync(h, dv, sizeof(double) * count, hipMemcpyDeviceToHost, sc.stream));
    OFC_HIP(hipStreamSynchronize(sc.stream));
    return OFC_OK;
}

// potentials of the candidates the last sweep evaluated (this rank's share)
int kpp_local_pots(LloydScratch &sc, int nblocks, double *pots8)
{
    OFC_TRY(launch_reduce_records(sc.partial.as<double>(), nblocks, 8, sc.tot.as<double>(), sc.stream));
    OFC_HIP(hipMemcpyAsync(pots8, sc.tot.p, sizeof(double) * 8, hipMemcpyDeviceToHost, sc.stream));
    OFC_HIP(hipStreamSynchronize(sc.stream));
    return OFC_OK;
}
}  // namespace

namespace {
// ofc_kpp_seed_dev (w_dev == nullptr: `first` is the first centre) and ofc_kpp_seed_dev_w (w_dev: u_first draws it)
int kpp_seed(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
             const double *colsum, int64_t first, double u_first, const double *u, int n_trials, double *centers,
             int64_t *indices)
{
    OFC_REQUIRE(X_dev && centers && indices && (u || k == 1), "null pointer");
    OFC_REQUIRE(dtype >= OFC_U8 && dtype <= OFC_F64, "bad dtype %d", dtype);
    OFC_REQUIRE(N >= 0, "N=%lld is negative", (long long)N);
    OFC_TRY(check_kd(k, d));
    OFC_REQUIRE(n_trials >= 1 && n_trials <= 8, "n_trials %d outside 1..8", n_trials);
    for (int i = 0; i < (k - 1) * n_trials; i++)
        OFC_REQUIRE(u[i] >= 0.0 && u[i] < 1.0, "u[%d]=%g outside [0,1)", i, u[i]);
    OFC_REQUIRE(first >= 0, "first=%lld is negative", (long long)first);
    OFC_REQUIRE(u_first >= 0.0 && u_first < 1.0, "u_first=%g outside [0,1)", u_first);
    if (N > KPP_NMAX) {
        set_error("N=%lld outside the seeding kernels' range (<= %lld samples per rank)", (long long)N, (long long)KPP_NMAX);
        return OFC_EUNSUPPORTED;
    }
    const int world = dist_active() ? dist_world() : 1, rank = dist_active() ? dist_rank() : 0;
    if (world > 64) { set_error("seeding over %d ranks is not supported (<= 64)", world); return OFC_EUNSUPPORTED; }
    if (world == 1) {       // with a communicator the same two tests follow the exchange of the shard sizes
        OFC_REQUIRE(N >= k, "n_samples=%lld should be >= n_clusters=%d.", (long long)N, k);
        OFC_REQUIRE(w_dev || first < N, "first=%lld outside 0..%lld", (long long)first, (long long)N - 1);
    }
    OFC_TRY(ensure_device(device));
    LloydScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    OFC_TRY(sc.init());
    hipStream_t s = sc.stream;
    if (!sc.kpp_io.p) OFC_TRY(sc.kpp_io.alloc(sizeof(double) * KPP_IO_LEN));
    int64_t *idx_dev = sc.kpp_io.as<int64_t>();
    double *rows_dev = sc.kpp_io.as<double>() + KPP_IO_ROWS;

    // ---- shard layout: global row order is rank order ----
    std::vector<double> nq(world, 0.0), pq(world, 0.0);
    nq[rank] = (double)N;
    OFC_TRY(kpp_exchange(sc, nq.data(), world, DIST_SUM));
    double Ng = 0, off_me = 0;
    for (int q = 0; q < world; q++) {
        if (q < rank) off_me += nq[q];
        Ng += nq[q];
    }
    OFC_REQUIRE(Ng >= (double)k, "n_samples=%.0f should be >= n_clusters=%d.", Ng, k);
    OFC_REQUIRE(w_dev || (double)first < Ng, "first=%lld outside 0..%.0f", (long long)first, Ng - 1);
    if (nq[rank] != (double)N) { set_error("the communicator does not lay the shards out by rank"); return OFC_EUNSUPPORTED; }

    // ---- column mean, as the fit forms it ----
    double *tot = sc.tot.as<double>();
    double hbuf[LLOYD_DMAX], mean_h[LLOYD_DMAX];
    const int nb_stats = lloyd_grid(N);
    if (colsum) {
        memcpy(hbuf, colsum, sizeof(double) * d);
    } else {
        LloydState *st = sc.state.as<LloydState>();
        OFC_TRY(launch_lloyd_colstats(X_dev, dtype, N, d, st->mean, 0, sc.partial.as<double>(), nb_stats, s));
        OFC_TRY(launch_reduce_records(sc.partial.as<double>(), nb_stats, d, tot, s));
        OFC_HIP(hipMemcpyAsync(hbuf, tot, sizeof(double) * d, hipMemcpyDeviceToHost, s));
        OFC_HIP(hipStreamSynchronize(s));
    }
    OFC_TRY(kpp_exchange(sc, hbuf, d, DIST_SUM));
    for (int f = 0; f < d; f++) mean_h[f] = hbuf[f] / Ng;

    const int64_t nchunks = kpp_chunks(N);
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(nchunks, 4), 2048));
    if (N > 0) {
        OFC_TRY(reserve(sc.kpp_closest, sizeof(double) * (size_t)N));
        OFC_TRY(reserve(sc.kpp_cs, sizeof(double) * 8 * (size_t)nchunks));
        OFC_TRY(reserve(sc.kpp_ss, sizeof(double) * (size_t)cdiv64(nchunks, 1024)));
    }
    double *closest = sc.kpp_closest.as<double>(), *cs = sc.kpp_cs.as<double>(), *ss = sc.kpp_ss.as<double>();
    const size_t es = dtype_size(dtype);
    auto as_double = [&](const unsigned char *raw, int f) {
        return dtype == OFC_U8 ? (double)raw[f] : dtype == OFC_F32 ? (double)((const float *)raw)[f] : ((const double *)raw)[f];
    };
    auto sweep = [&](const double *prev, int prev_mode, const double *cand, int n_cand) {
        if (w_dev)
            return launch_kpp_sweep_w(X_dev, dtype, w_dev, w_dtype, N, d, mean_h, prev, prev_mode, cand, n_cand, closest, cs,
                                      sc.partial.as<double>(), nblocks, s);
        return launch_kpp_sweep(X_dev, dtype, N, d, mean_h, prev, prev_mode, cand, n_cand, closest, cs,
                                sc.partial.as<double>(), nblocks, s);
    };

    // ---- with weights, the first centre is drawn as RandomState.choice(N, p=w/w.sum()) draws it (_kmeans.py:224):
    //      the smallest global row whose cumulative weight exceeds u_first * W ----
    if (w_dev) {
        pq[rank] = 0;
        if (N > 0) {
            OFC_TRY(launch_kpp_wchunks(w_dev, w_dtype, nullptr, N, cs, s));
            OFC_TRY(launch_kpp_sum1024(cs, nchunks, ss, s));
            OFC_TRY(launch_kpp_total(ss, (int)cdiv64(nchunks, 1024), sc.tot.as<double>(), s));
            OFC_HIP(hipMemcpyAsync(&pq[rank], sc.tot.p, sizeof(double), hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
        }
        OFC_TRY(kpp_exchange(sc, pq.data(), world, DIST_SUM));
        double W = 0;
        for (int q = 0; q < world; q++) W += pq[q];
        if (!(W > 0)) { set_error("sum of sample weights must be positive"); return OFC_EINVAL; }
        const double r = u_first * W;
        // the first non-empty shard whose running sum exceeds r; the last one with any weight when rounding leaves none
        int owner = -1;
        double S = 0, base_me = 0;
        for (int q = 0; q < world; q++) {
            if (q == rank) base_me = S;
            if (pq[q] > 0) {
                owner = q;
                if (S + pq[q] > r) break;
            }
            S += pq[q];
        }
        double gi = 0;
        if (owner == rank) {
            int64_t li;
            OFC_TRY(launch_kpp_sample_w(X_dev, dtype, w_dev, w_dtype, N, d, mean_h, nullptr, KPP_PREV_NONE, nullptr, cs, ss,
                                        &r, 1, base_me, KPP_SIDE_FIRST, idx_dev, rows_dev, s));
            OFC_HIP(hipMemcpyAsync(&li, idx_dev, sizeof(int64_t), hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
            gi = off_me + (double)li;
        }
        OFC_TRY(kpp_exchange(sc, &gi, 1, DIST_BCAST));
        first = (int64_t)gi;
    }

    // ---- first centre: its owner broadcasts the row ----
    double rec[8 * (LLOYD_DMAX + 1)];
    memset(rec, 0, sizeof(rec));
    if ((double)first >= off_me && (double)first < off_me + (double)N) {
        unsigned char raw[LLOYD_DMAX * 8];
        const int64_t li = first - (int64_t)off_me;
        OFC_HIP(hipMemcpyAsync(raw, (const char *)X_dev + (size_t)li * d * es, d * es, hipMemcpyDeviceToHost, s));
        OFC_HIP(hipStreamSynchronize(s));
        for (int f = 0; f < d; f++) rec[f] = as_double(raw, f);
    }
    OFC_TRY(kpp_exchange(sc, rec, d, DIST_BCAST));
    double prev[LLOYD_DMAX], pl[8], pg[8];
    for (int f = 0; f < d; f++) {
        centers[f] = rec[f];
        prev[f] = rec[f] - mean_h[f];
    }
    indices[0] = first;
    for (double &v : pl) v = 0;
    if (N > 0) {
        OFC_TRY(sweep(prev, KPP_PREV_FIRST, nullptr, 0));
        OFC_TRY(launch_kpp_sum1024(cs, nchunks, ss, s));
        OFC_TRY(kpp_local_pots(sc, nblocks, pl));
    }
    memcpy(pg, pl, sizeof(pg));
    OFC_TRY(kpp_exchange(sc, pg, 8, DIST_SUM));
    double current_pot = pg[0], pot_local = pl[0];
    int slot = 0;                 // whose chunk sums (cs[slot], summed into ss) describe closest with `prev` folded in

    for (int c = 1; c < k; c++) {
        // ---- sample n_trials rows from the cumulative sum of closest (_kmeans.py:242-247) ----
        double r[8];
        for (int j = 0; j < n_trials; j++) r[j] = u[(size_t)(c - 1) * n_trials + j] * current_pot;
        for (double &v : pq) v = 0;
        pq[rank] = pot_local;
        OFC_TRY(kpp_exchange(sc, pq.data(), world, DIST_SUM));
        double base_me = 0;
        for (int q = 0; q < rank; q++) base_me += pq[q];
        bool mine[8], any = false;
        for (int j = 0; j < n_trials; j++) {
            // the first non-empty shard whose cumulative sum reaches r[j]; the last non-empty one when none does (clip)
            int owner = -1;
            double S = 0;
            for (int q = 0; q < world; q++) {
                if (nq[q] > 0) {
                    owner = q;
                    if (S + pq[q] >= r[j]) break;
                }
                S += pq[q];
            }
            mine[j] = owner == rank;
            any = any || mine[j];
        }
        memset(rec, 0, sizeof(rec));
        if (any) {
            int64_t idx_h[8];
            double rows_h[8 * LLOYD_DMAX];
            const int prev_mode = c >= 2 ? KPP_PREV_APPLY : KPP_PREV_NONE;
            if (w_dev)
                OFC_TRY(launch_kpp_sample_w(X_dev, dtype, w_dev, w_dtype, N, d, mean_h, prev, prev_mode, closest,
                                            cs + (size_t)slot * nchunks, ss, r, n_trials, base_me, KPP_SIDE_LEFT, idx_dev,
                                            rows_dev, s));
            else
                OFC_TRY(launch_kpp_sample(X_dev, dtype, N, d, mean_h, prev, prev_mode, closest,
                                          cs + (size_t)slot * nchunks, ss, r, n_trials, base_me, idx_dev, rows_dev, s));
            OFC_HIP(hipMemcpyAsync(idx_h, idx_dev, sizeof(int64_t) * n_trials, hipMemcpyDeviceToHost, s));
            OFC_HIP(hipMemcpyAsync(rows_h, rows_dev, sizeof(double) * n_trials * LLOYD_DMAX, hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
            for (int j = 0; j < n_trials; j++) {
                if (!mine[j]) continue;
                for (int f = 0; f < d; f++) rec[j * (d + 1) + f] = rows_h[j * LLOYD_DMAX + f];
                rec[j * (d + 1) + d] = off_me + (double)idx_h[j];
            }
        }
        OFC_TRY(kpp_exchange(sc, rec, n_trials * (d + 1), DIST_BCAST));
        double cand[8 * LLOYD_DMAX];
        for (int j = 0; j < n_trials; j++)
            for (int f = 0; f < d; f++) cand[j * d + f] = rec[j * (d + 1) + f] - mean_h[f];

        // ---- one sweep: fold the previous winner into closest, evaluate the candidates (:250-256) ----
        for (double &v : pl) v = 0;
        if (N > 0) {
            OFC_TRY(sweep(prev, c >= 2 ? KPP_PREV_APPLY : KPP_PREV_NONE, cand, n_trials));
            OFC_TRY(kpp_local_pots(sc, nblocks, pl));
        }
        memcpy(pg, pl, sizeof(pg));
        OFC_TRY(kpp_exchange(sc, pg, 8, DIST_SUM));
        int best = 0;                                    // np.argmin: the first minimum (:259)
        for (int j = 1; j < n_trials; j++)
            if (pg[j] < pg[best]) best = j;
        current_pot = pg[best];
        pot_local = pl[best];
        slot = best;
        if (N > 0 && c + 1 < k) OFC_TRY(launch_kpp_sum1024(cs + (size_t)slot * nchunks, nchunks, ss, s));
        for (int f = 0; f < d; f++) {
            centers[c * d + f] = rec[best * (d + 1) + f];
            prev[f] = cand[best * d + f];
        }
        indices[c] = (int64_t)rec[best * (d + 1) + d];
    }
    OFC_HIP(hipStreamSynchronize(s));
    return OFC_OK;
}

int check_w_dtype(int w_dtype)
{
    if (w_dtype != OFC_F32 && w_dtype != OFC_F64) {
        set_error("bad weight dtype %d (OFC_F32 or OFC_F64)", w_dtype);
        return OFC_EINVAL;
    }
    return OFC_OK;
}
}  // namespace

int ofc_kpp_seed_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *colsum,
                     int64_t first, const double *u, int n_trials, double *centers, int64_t *indices)
{
    return kpp_seed(device, X_dev, dtype, nullptr, OFC_F32, N, d, k, colsum, first, 0.0, u, n_trials, centers, indices);
}

int ofc_kpp_seed_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                       const double *colsum, double u_first, const double *u, int n_trials, double *centers,
                       int64_t *indices)
{
    OFC_REQUIRE(w_dev, "null weight pointer");
    OFC_TRY(check_w_dtype(w_dtype));
    OFC_REQUIRE((uintptr_t)w_dev % 16 == 0, "the weights must be 16-byte aligned");
    return kpp_seed(device, X_dev, dtype, w_dev, w_dtype, N, d, k, colsum, 0, u_first, u, n_trials, centers, indices);
}

int ofc_kpp_sample_dev_w(int device, const void *w_dev, int w_dtype, const double *v_dev, int64_t N, const double *r, int n,
                         int side, int64_t *idx, double *total)
{
    OFC_REQUIRE(w_dev && r && idx && total, "null pointer");
    OFC_TRY(check_w_dtype(w_dtype));
    OFC_REQUIRE((uintptr_t)w_dev % 16 == 0, "the weights must be 16-byte aligned");
    OFC_REQUIRE(side == 0 || side == 1, "side %d: 0 (left) or 1 (right)", side);
    OFC_REQUIRE(n >= 1 && n <= 8, "n %d outside 1..8", n);
    OFC_REQUIRE(N >= 1, "N=%lld: nothing to sample from", (long long)N);
    if (N > KPP_NMAX) {
        set_error("N=%lld outside the seeding kernels' range (<= %lld samples)", (long long)N, (long long)KPP_NMAX);
        return OFC_EUNSUPPORTED;
    }
    OFC_TRY(ensure_device(device));
    const int64_t nchunks = kpp_chunks(N);
    const int nsuper = (int)cdiv64(nchunks, 1024);
    DevBuf cs, ss, out;
    OFC_TRY(cs.alloc(sizeof(double) * (size_t)nchunks));
    OFC_TRY(ss.alloc(sizeof(double) * (size_t)nsuper));
    OFC_TRY(out.alloc(sizeof(int64_t) * 8 + sizeof(double)));
    double *tot_dev = out.as<double>() + 8;
    OFC_TRY(launch_kpp_wchunks(w_dev, w_dtype, v_dev, N, cs.as<double>(), nullptr));
    OFC_TRY(launch_kpp_sum1024(cs.as<double>(), nchunks, ss.as<double>(), nullptr));
    OFC_TRY(launch_kpp_total(ss.as<double>(), nsuper, tot_dev, nullptr));
    OFC_TRY(launch_kpp_sample_w(nullptr, OFC_F64, w_dev, w_dtype, N, 1, nullptr, nullptr, KPP_PREV_NONE, v_dev, cs.as<double>(),
                                ss.as<double>(), r, n, 0.0, side == 0 ? KPP_SIDE_LEFT : KPP_SIDE_RIGHT, out.as<int64_t>(),
                                nullptr, nullptr));
    OFC_HIP(hipMemcpy(idx, out.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(total, tot_dev, sizeof(double), hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_kpp_sample_dev(int device, const double *w_dev, int64_t N, const double *r, int n, int64_t *idx)
{
    OFC_REQUIRE(w_dev && r && idx, "null pointer");
    OFC_REQUIRE(n >= 1 && n <= 8, "n %d outside 1..8", n);
    OFC_REQUIRE(N >= 1, "N=%lld: nothing to sample from", (long long)N);
    if (N > KPP_NMAX) {
        set_error("N=%lld outside the seeding kernels' range (<= %lld samples)", (long long)N, (long long)KPP_NMAX);
        return OFC_EUNSUPPORTED;
    }
    OFC_TRY(ensure_device(device));
    const int64_t nchunks = kpp_chunks(N);
    DevBuf cs, ss, out;
    OFC_TRY(cs.alloc(sizeof(double) * (size_t)nchunks));
    OFC_TRY(ss.alloc(sizeof(double) * (size_t)cdiv64(nchunks, 1024)));
    OFC_TRY(out.alloc(sizeof(int64_t) * 8));
    OFC_TRY(launch_kpp_sum1024(w_dev, N, cs.as<double>(), nullptr));
    OFC_TRY(launch_kpp_sum1024(cs.as<double>(), nchunks, ss.as<double>(), nullptr));
    OFC_TRY(launch_kpp_sample(nullptr, OFC_F64, N, 1, nullptr, nullptr, KPP_PREV_NONE, w_dev, cs.as<double>(), ss.as<double>(),
                              r, n, 0.0, out.as<int64_t>(), nullptr, nullptr));
    OFC_HIP(hipMemcpy(idx, out.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    return OFC_OK;
}

/* ---- sample weights, see include/ofc.h ---- */
namespace {
// host weights: finite, non-negative, positive sum (sklearn's _check_sample_weight + the zero-sum refusal)
int check_host_weights(const void *w, int w_dtype, int64_t N)
{
    double sum = 0;
    for (int64_t i = 0; i < N; i++) {
        const double v = w_dtype == OFC_F32 ? (double)((const float *)w)[i] : ((const double *)w)[i];
        if (!std::isfinite(v)) { set_error("sample_weight[%lld] is not finite", (long long)i); return OFC_EINVAL; }
        if (v < 0) { set_error("sample_weight[%lld] is negative", (long long)i); return OFC_EINVAL; }
        sum += v;
    }
    if (!(sum > 0)) { set_error("sum of sample weights must be positive"); return OFC_EINVAL; }
    return OFC_OK;
}
}  // namespace

int ofc_kmeans_fit_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                         const double *init, int max_iter, double tol_rel, const double *colsum, double *centers,
                         uint8_t *labels_dev, double *inertia, int *n_iter)
{
    if (w_dev) OFC_TRY(check_w_dtype(w_dtype));
    return lloyd_fit_dev(device, X_dev, dtype, N, d, k, init, max_iter, tol_rel, centers, labels_dev, inertia, n_iter, colsum,
                         w_dev, w_dtype);
}

int ofc_kmeans_fit_w(int device, const void *X, int dtype, const void *w, int w_dtype, int64_t N, int d, int k,
                     const double *init, int max_iter, double tol_rel, double *centers, int32_t *labels, double *inertia,
                     int *n_iter)
{
    OFC_REQUIRE(X && w && init && centers, "null pointer");
    OFC_REQUIRE(dtype >= OFC_U8 && dtype <= OFC_F64 && d >= 1 && N >= 0, "bad arguments");
    OFC_TRY(check_w_dtype(w_dtype));
    OFC_REQUIRE(N >= k, "n_samples=%lld should be >= n_clusters=%d.", (long long)N, k);
    OFC_TRY(check_host_weights(w, w_dtype, N));
    OFC_TRY(ensure_device(device));
    DevBuf dX, dW, dL;
    const size_t bytes = (size_t)N * d * dtype_size(dtype), wbytes = (size_t)N * dtype_size(w_dtype);
    OFC_TRY(dX.alloc(std::max<size_t>(bytes, 16)));
    OFC_TRY(dW.alloc(std::max<size_t>(wbytes, 16)));
    OFC_TRY(dL.alloc((size_t)std::max<int64_t>(N, 1)));
    OFC_HIP(hipMemcpy(dX.p, X, bytes, hipMemcpyHostToDevice));
    OFC_HIP(hipMemcpy(dW.p, w, wbytes, hipMemcpyHostToDevice));
    OFC_TRY(lloyd_fit_dev(device, dX.p, dtype, N, d, k, init, max_iter, tol_rel, centers, dL.as<uint8_t>(), inertia, n_iter,
                          nullptr, dW.p, w_dtype));
    if (labels) {
        std::vector<uint8_t> l8((size_t)N);
        OFC_HIP(hipMemcpy(l8.data(), dL.p, (size_t)N, hipMemcpyDeviceToHost));
        widen_labels(l8.data(), N, labels);
    }
    return OFC_OK;
}

int ofc_kmeans_score(int device, const void *X, int dtype, const void *w, int w_dtype, int64_t N, int d, int k,
                     const double *centers, double *inertia)
{
    OFC_REQUIRE(X && centers && inertia, "null pointer");
    OFC_REQUIRE(dtype >= OFC_U8 && dtype <= OFC_F64 && N >= 0, "bad arguments");
    OFC_TRY(check_kd(k, d));
    if (w) {
        OFC_TRY(check_w_dtype(w_dtype));
        OFC_TRY(check_host_weights(w, w_dtype, N));
    }
    OFC_TRY(ensure_device(device));
    DevBuf dX, dW, dL;
    const size_t bytes = (size_t)N * d * dtype_size(dtype), wbytes = w ? (size_t)N * dtype_size(w_dtype) : 0;
    OFC_TRY(dX.alloc(std::max<size_t>(bytes, 16)));
    OFC_TRY(dL.alloc((size_t)std::max<int64_t>(N, 1)));
    OFC_HIP(hipMemcpy(dX.p, X, bytes, hipMemcpyHostToDevice));
    if (w) {
        OFC_TRY(dW.alloc(std::max<size_t>(wbytes, 16)));
        OFC_HIP(hipMemcpy(dW.p, w, wbytes, hipMemcpyHostToDevice));
    }
    // the centres as given (KMeans.score does not centre X): mean 0
    StepCtx c;
    OFC_TRY(c.init(N, 2));
    double zero[LLOYD_DMAX] = {0, 0, 0, 0};
    OFC_TRY(c.set(zero, centers, k, d));
    LloydState *st = c.state.as<LloydState>();
    if (w)
        OFC_TRY(launch_lloyd_assign_w(dX.p, dtype, dW.p, w_dtype, N, d, k, st, dL.as<uint8_t>(), c.partial.as<double>(),
                                      c.nblocks, 2, 0, nullptr));
    else
        OFC_TRY(launch_lloyd_assign(dX.p, dtype, N, d, k, st, dL.as<uint8_t>(), c.partial.as<double>(), c.nblocks, 2, 0, nullptr));
    OFC_TRY(launch_reduce_records(c.partial.as<double>(), c.nblocks, 1, c.tot.as<double>(), nullptr));
    OFC_HIP(hipMemcpy(inertia, c.tot.p, sizeof(double), hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_lloyd_step_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                         const double *mean, const double *centers_c, uint8_t *labels_dev, double *record)
{
    OFC_REQUIRE(X_dev && w_dev && mean && centers_c && labels_dev && record && N >= 0, "bad arguments");
    OFC_TRY(check_w_dtype(w_dtype));
    OFC_TRY(check_kd(k, d));
    OFC_TRY(ensure_device(device));
    const int kmax = lloyd_kmax(k), NV = lloyd_record_len(kmax, d);
    StepCtx c;
    OFC_TRY(c.init(N, NV));
    OFC_TRY(c.set(mean, centers_c, k, d));
    LloydState *st = c.state.as<LloydState>();
    OFC_TRY(launch_lloyd_assign_w(X_dev, dtype, w_dev, w_dtype, N, d, k, st, labels_dev, c.partial.as<double>(), c.nblocks, 1, 0, nullptr));
    OFC_TRY(launch_reduce_records(c.partial.as<double>(), c.nblocks, NV, c.tot.as<double>(), nullptr));
    std::vector<double> t(NV);
    OFC_HIP(hipMemcpy(t.data(), c.tot.p, sizeof(double) * NV, hipMemcpyDeviceToHost));
    for (int j = 0; j < k; j++) {
        for (int f = 0; f < d; f++) record[j * d + f] = t[j * d + f];
        record[k * d + j] = t[kmax * d + j];
    }
    record[k * d + k] = t[kmax * d + kmax];
    return OFC_OK;
}

int ofc_lloyd_inertia_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                            const double *mean, const double *centers_c, const uint8_t *labels_dev, double *inertia)
{
    OFC_REQUIRE(X_dev && w_dev && mean && centers_c && labels_dev && inertia && N >= 0, "bad arguments");
    OFC_TRY(check_w_dtype(w_dtype));
    OFC_TRY(check_kd(k, d));
    OFC_TRY(ensure_device(device));
    StepCtx c;
    OFC_TRY(c.init(N, 2));
    OFC_TRY(c.set(mean, centers_c, k, d));
    OFC_TRY(launch_lloyd_inertia_w(X_dev, dtype, w_dev, w_dtype, N, d, c.state.as<LloydState>(), labels_dev,
                                   c.partial.as<double>(), c.nblocks, nullptr));
    OFC_TRY(launch_reduce_records(c.partial.as<double>(), c.nblocks, 1, c.tot.as<double>(), nullptr));
    OFC_HIP(hipMemcpy(inertia, c.tot.p, sizeof(double), hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_lloyd_farthest_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                             const double *mean, const double *centers_c, const uint8_t *labels_dev, const int64_t *excl,
                             int n_excl, double *dist2, int64_t *index, double *x_c, int *label, double *weight)
{
    OFC_REQUIRE(w_dev && weight, "bad arguments");
    OFC_TRY(check_w_dtype(w_dtype));
    OFC_TRY(ofc_lloyd_farthest_dev(device, X_dev, dtype, N, d, k, mean, centers_c, labels_dev, excl, n_excl, dist2, index,
                                   x_c, label));
    *weight = 0.0;
    if (*index >= 0) {
        if (w_dtype == OFC_F32) {
            float v;
            OFC_HIP(hipMemcpy(&v, (const float *)w_dev + *index, sizeof(float), hipMemcpyDeviceToHost));
            *weight = (double)v;
        } else {
            OFC_HIP(hipMemcpy(weight, (const double *)w_dev + *index, sizeof(double), hipMemcpyDeviceToHost));
        }
    }
    return OFC_OK;
}

int ofc_flow_weights_dev(int device, const float *flow_dev, int64_t n, int kind, float thr, float *w_dev)
{
    OFC_REQUIRE(flow_dev && w_dev && n >= 0, "bad arguments");
    OFC_REQUIRE(kind == 0 || kind == 1, "kind = %d (0 magnitude, 1 moving)", kind);
    OFC_REQUIRE(kind == 0 || (std::isfinite(thr) && thr >= 0), "thr must be finite and >= 0");
    OFC_TRY(ensure_device(device));
    OFC_TRY(launch_flow_weights(flow_dev, n, kind, thr, w_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_bench_lloyd_sweep_w(int device, const float *X_dev, const void *w_dev, int w_dtype, int64_t N, int k,
                            const double *centers, const double *mean, int iters, float *ms_per_launch)
{
    OFC_REQUIRE(X_dev && w_dev && centers && mean && ms_per_launch && iters >= 1 && N >= 64, "bad arguments");
    OFC_TRY(check_w_dtype(w_dtype));
    OFC_TRY(check_kd(k, 2));
    OFC_TRY(ensure_device(device));
    LloydScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    OFC_TRY(sc.init());
    hipStream_t s = sc.stream;
    const int nblocks = lloyd_grid(N);
    LloydState *st = sc.state.as<LloydState>();
    OFC_HIP(hipMemsetAsync(st, 0, sizeof(LloydState), s));
    double c0[LLOYD_KMAX * LLOYD_DMAX];
    for (int j = 0; j < k * 2; j++) c0[j] = centers[j] - mean[j % 2];
    OFC_HIP(hipMemcpyAsync(st->mean, mean, sizeof(double) * 2, hipMemcpyHostToDevice, s));
    OFC_HIP(hipMemcpyAsync(st->centers, c0, sizeof(double) * k * 2, hipMemcpyHostToDevice, s));
    OFC_TRY(launch_lloyd_set_centers(st, k, 2, s));
    auto launch = [&]() -> int {
        return launch_lloyd_assign_w(X_dev, OFC_F32, w_dev, w_dtype, N, 2, k, st, nullptr, sc.partial.as<double>(), nblocks, 3, 0, s);
    };
    return time_launches(s, iters, launch, ms_per_launch);
}

}  // extern "C"
