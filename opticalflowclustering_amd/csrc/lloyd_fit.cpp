// lloyd_fit.cpp -- C ABI of libofc.so, part 2: the clip-wide Lloyd k-means fit (streaming shape), predict and score.
// Control flow = sklearn's _kmeans_single_lloyd (_kmeans.py:624-752) around the kernels of
// lloyd_kernels.hip; see include/ofc.h for the reference call sites.
#include "lloyd_host.h"

namespace ofc {

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

// One fit: what it is asked for (the exports fill these, in this order), what lloyd_fit_dev derives from that, the state of
// its iteration loop, and its steps in the order lloyd_fit_dev runs them.
struct LloydFit {
    int device;
    LloydSamples x;                     // on the device
    int k;
    const double *init;
    int max_iter;
    double tol_rel;
    double *centers;
    uint8_t *labels_dev;                // nullptr: the labels stay in the scratch
    double *inertia;
    int *n_iter;
    const double *colsum = nullptr;     // this rank's column sums, when the caller has them
    int field_w = 0, field_h = 0;       // X is a stack of n_fields (u,v) fields of field_w x field_h
    int64_t n_fields = 0;

    LloydScratch *sc = nullptr;         // the device's, locked by lloyd_fit_dev, and what of it every step uses:
    hipStream_t s = nullptr;
    LloydState *st = nullptr;
    double *tot = nullptr, *partial = nullptr;
    int kmax = 0, NV = 0, nblocks = 0;
    double Ng = 0, mean_h[LLOYD_DMAX];  // global sample count and column mean
    double c0[LLOYD_KMAX * LLOYD_DMAX]; // the centred initial centres, until the first window's synchronisation
    int prune = LLOYD_PRUNE_OFF;        // the sweeps' form: the tile policy, 2-D field tiles or not, the tile records
    bool field = false;
    LloydFieldBufs tb = {};
    bool trace = false;

    bool labelled = false, strict = false, stop = false;
    int tiles_next = LLOYD_TILES_FULL;   // how the device would run the next tile sweep: decides the form of the final E-step
    int it = 0;

    int check() const;                  // 1: the argument checks
    int column_mean();                  // 2: column mean and Ng, with or without colsum
    int centred_init();                 // 3: the sweeps' form, then the centred model
    int enqueue_window(int nwin);       // 4: enqueue iterations it .. it + nwin - 1
    int read_window(int nwin);          // 5: their status slots: statistics, refusal, the empty-cluster branch, the stop
    int final_sweep();                  // 6: the final E-step (only when not strictly converged) and inertia: one sweep
    int read_back();                    // 7: inertia and centres to the caller
    int tiles_launch(uint8_t *lab, int what, const double *meta) const;
    int relocate_empty();
};

// empty-cluster relocation (_k_means_common.pyx:167-211) on the all-reduced totals `tot`.
// Returns with `tot` patched on the device (or untouched when the farthest distance is 0).
// x.w != nullptr: the fit is weighted.  The farthest sample is still found by its UNWEIGHTED distance; it moves with its
// weight: sums[old] -= x*w, sums[new] = x*w, wk[new] = w, wk[old] -= w (_k_means_common.pyx:197-211), the product rounded
// on its own.  Under a communicator the owner's broadcast carries the weight in one more slot.
int LloydFit::relocate_empty()
{
    const int d = x.d;
    std::vector<double> totals(NV);
    OFC_HIP(hipMemcpyAsync(totals.data(), sc->tot.p, sizeof(double) * NV, hipMemcpyDeviceToHost, s));
    OFC_HIP(hipStreamSynchronize(s));
    double *w = totals.data() + kmax * d;
    const double *c_old = st->centers;          // device address of the member array
    std::vector<int64_t> excl;
    std::vector<double> blk(2 * nblocks);
    bool first = true;
    for (int j = 0; j < k; j++) {
        if (w[j] != 0.0) continue;
        if (!excl.empty())
            OFC_HIP(hipMemcpyAsync(sc->excl.p, excl.data(), sizeof(int64_t) * excl.size(), hipMemcpyHostToDevice, s));
        OFC_TRY(launch_lloyd_farthest(x.X, x.dtype, x.N, d, st, c_old, labels_dev, sc->excl.as<int64_t>(), (int)excl.size(),
                                      sc->far.as<double>(), nblocks, s));
        OFC_HIP(hipMemcpyAsync(blk.data(), sc->far.p, sizeof(double) * 2 * nblocks, hipMemcpyDeviceToHost, s));
        OFC_HIP(hipStreamSynchronize(s));
        double best;
        const int64_t bi = farthest_pick(blk.data(), nblocks, best);
        // global winner across ranks: max distance, ties -> lowest rank (= lowest global index)
        double rec[LLOYD_DMAX + 3];   // [x_c[d] | old label | weight (weighted fits only)]
        const int nrec = d + 1 + (x.w ? 1 : 0);
        int owner = 1;
        if (dist_active()) {
            double g = best;
            OFC_TRY(host_allreduce(sc->far.as<double>(), &g, 1, DIST_MAX, s));
            double r = (bi >= 0 && best == g) ? (double)dist_rank() : 1e300;
            OFC_TRY(host_allreduce(sc->far.as<double>(), &r, 1, DIST_MIN, s));
            owner = ((int)r == dist_rank()) && bi >= 0 && best == g;
            best = g;
        }
        if (first && !(best > 0)) return OFC_OK;   // np.max(distances) == 0: relocating is pointless
        first = false;
        memset(rec, 0, sizeof(rec));
        if (owner) {
            unsigned char raw[LLOYD_DMAX * 8], wraw[8];
            uint8_t lab;
            OFC_HIP(hipMemcpyAsync(raw, row_ptr(x, bi), row_size(x), hipMemcpyDeviceToHost, s));
            OFC_HIP(hipMemcpyAsync(&lab, labels_dev + bi, 1, hipMemcpyDeviceToHost, s));
            const size_t ws = dtype_size(x.w_dtype);
            if (x.w) OFC_HIP(hipMemcpyAsync(wraw, (const char *)x.w + (size_t)bi * ws, ws, hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
            row_centred(raw, x.dtype, d, mean_h, rec);
            rec[d] = (double)lab;
            if (x.w) rec[d + 1] = sample_elem(wraw, x.w_dtype, 0);
            excl.push_back(bi);
        }
        OFC_TRY(host_allreduce(sc->far.as<double>(), rec, nrec, DIST_BCAST, s));
        const int old = (int)rec[d];
        const double wt = x.w ? rec[d + 1] : 1.0;
        for (int f = 0; f < d; f++) {
            const double xw = rec[f] * wt;      // a statement of its own: rounded before it is subtracted (x * 1 is x)
            totals[old * d + f] -= xw;
            totals[j * d + f] = xw;
        }
        w[j] = wt;
        w[old] -= wt;
    }
    OFC_HIP(hipMemcpyAsync(sc->tot.p, totals.data(), sizeof(double) * NV, hipMemcpyHostToDevice, s));
    OFC_HIP(hipStreamSynchronize(s));
    return OFC_OK;
}

int LloydFit::check() const
{
    OFC_REQUIRE(x.X && init && centers, "null pointer");
    OFC_REQUIRE(x.dtype >= OFC_U8 && x.dtype <= OFC_F64, "bad dtype %d", x.dtype);
    if (x.w) OFC_TRY(check_w_dtype(x.w_dtype));
    OFC_REQUIRE(x.d >= 1 && k >= 1 && max_iter >= 1 && x.N >= 0, "bad shape");
    OFC_TRY(check_kd(k, x.d));
    return ensure_device(device);
}

// column mean (X.mean(axis=0), _kmeans.py:1478-1484) and tol (_tolerance, :279-287)
int LloydFit::column_mean()
{
    const int d = x.d;
    double hbuf[LLOYD_DMAX + 1];
    if (colsum) {           // the caller already has this rank's column sums (the flow kernels' epilogue): no sweep
        OFC_HIP(hipMemcpyAsync(tot, colsum, sizeof(double) * d, hipMemcpyHostToDevice, s));
    } else {
        OFC_TRY(launch_lloyd_colstats(x.X, x.dtype, x.N, d, st->mean, 0, partial, nblocks, s));
        OFC_TRY(launch_reduce_records(partial, nblocks, d, tot, s));
    }
    double nloc = (double)x.N;
    OFC_HIP(hipMemcpyAsync(tot + d, &nloc, sizeof(double), hipMemcpyHostToDevice, s));
    OFC_TRY(dist_allreduce_f64(tot, d + 1, DIST_SUM, s));
    OFC_HIP(hipMemcpyAsync(hbuf, tot, sizeof(double) * (d + 1), hipMemcpyDeviceToHost, s));
    OFC_HIP(hipStreamSynchronize(s));
    Ng = hbuf[d];
    if (Ng < (double)k) {
        set_error("n_samples=%.0f should be >= n_clusters=%d.", Ng, k);
        return OFC_EINVAL;
    }
    for (int f = 0; f < d; f++) mean_h[f] = hbuf[f] / Ng;
    return OFC_OK;
}

int LloydFit::centred_init()
{
    // a weighted fit runs the plain sweeps: the tile metadata (cached per-tile sums) is unweighted
    prune = x.w ? LLOYD_PRUNE_OFF : prune_policy_for(x.dtype, x.N, x.d, k);
    // X is a stack of fields that the 2-D tiles fit (lloyd_field.h): the tile sweeps take their field form.  Any other
    // shape runs the 64 x 1 tiles; the result is the same either way.
    field = prune && field_w > 0 && field_geometry_ok(field_w, field_h, n_fields);
    if (prune) OFC_TRY(sc->tile_bufs(x.N, field ? field_w : 0, tb));
    for (double &v : sc->prune_stats) v = 0;
    return set_centred_model(*sc, mean_h, init, k, x.d, prune, c0);
}

int LloydFit::tiles_launch(uint8_t *lab, int what, const double *meta) const
{
    const float *X = (const float *)x.X;
    if (field) return launch_lloyd_tiles_field(X, x.N, k, st, tb, lab, partial, nblocks, what, meta, s);
    return launch_lloyd_tiles(X, x.N, k, st, tb.box, tb.tsum, tb.tsq, lab, partial, nblocks, what, meta, s);
}

int LloydFit::enqueue_window(int nwin)
{
    const int *halt = &st->halt;
    double *tot_local = dist_has_comm() ? sc->tot_local.as<double>() : tot;
    for (int w = 0; w < nwin; w++) sc->status[w].valid = 0;
    for (int w = 0; w < nwin; w++) {
        // label-less sweeps of a (u,v) stream go tile by tile: iteration 0 builds the tile metadata, the later ones
        // run in the mode k_lloyd_update chose from the previous iteration's tile counts (lloyd_tiles.hip)
        const int tiles = (prune && !labelled) ? (it + w == 0 ? 1 : 2) : 0;
        if (tiles == 1) {      // is the field coherent enough? then tile metadata + column sums of squares, then iteration 0
            OFC_TRY(tiles_launch(nullptr, LLOYD_WHAT_PROBE, nullptr));
            OFC_TRY(tiles_launch(nullptr, LLOYD_WHAT_META, nullptr));
            OFC_TRY(launch_reduce_records(partial, nblocks, 2, sc->tile_meta.as<double>(), s));
        }
        if (tiles)
            OFC_TRY(tiles_launch(nullptr, LLOYD_WHAT_SWEEP, tiles == 1 ? sc->tile_meta.as<double>() : nullptr));
        else
            OFC_TRY(lloyd_assign(x, k, st, labels_dev, partial, nblocks, labelled ? 1 : 3, it + w == 0, s));
        // with a communicator the local record goes to its own buffer and the collective writes `tot`: an iteration
        // behind the halt flag then re-reduces the same local records into the same totals (in place it would sum
        // the totals of all ranks again, and a stalled iteration's `tot` is what relocate_empty reads)
        OFC_TRY(launch_reduce_records(partial, nblocks, NV, tot_local, s, halt));
        OFC_TRY(dist_allreduce_f64(tot_local, tot, NV, DIST_SUM, s));
        OFC_TRY(launch_lloyd_update(st, tot, k, x.d, 0, labelled, it + w == 0, Ng, tol_rel, sc->status_dev + w, s, tiles));
    }
    OFC_HIP(hipStreamSynchronize(s));
    return OFC_OK;
}

// Leaves `it` at the first iteration of the next window, or at the one that stopped the fit.
int LloydFit::read_window(int nwin)
{
    int done = nwin;                      // iterations of this window that really ran
    for (int w = 0; w < nwin; w++) {
        LloydStatus &S = sc->status[w];
        if (!S.valid) { set_error("internal: Lloyd iteration %d did not run", it + w); return OFC_EHIP; }
        if (trace)
            fprintf(stderr, "[ofc lloyd] it %d tiles_mode %d tested %.0f pure %.0f shift %.3e empty %d\n", it + w,
                    S.tiles_mode, S.tiles_tested, S.tiles_pure, S.shift_tot, S.n_empty);
        if (S.tiles_mode != -1) {
            tiles_next = S.tiles_next;
            sc->prune_stats[0] += 1;                                   // sweeps that went tile by tile
            if (S.tiles_mode == LLOYD_TILES_PRUNED) {
                sc->prune_stats[1] += 1;                               // ... of them pruned
                sc->prune_stats[2] += S.tiles_tested;                  // tiles tested / skipped by the pruned sweeps
                sc->prune_stats[3] += S.tiles_pure;
            } else if (S.tiles_mode == LLOYD_TILES_PROBE) {
                sc->prune_stats[4] += 1;
            }
        }
        if (x.w && it + w == 0) {
            // sklearn refuses weights whose sum is not positive (_check_sample_weight); here every cluster would be
            // empty and relocated in each of max_iter iterations.  The counts are all-reduced: every rank returns.
            double wsum = 0;
            for (int j = 0; j < k; j++) wsum += S.counts[j];
            if (!(wsum > 0)) { set_error("sum of sample weights must be positive"); return OFC_EINVAL; }
        }
        if (S.n_empty > 0) {              // the device stalled here; iterations w+1.. of the window were no-ops
            const bool was_labelled = labelled;
            if (!labelled) {   // materialise this iteration's labels (st->centers is still the E-step's input)
                OFC_TRY(launch_lloyd_assign(x.X, x.dtype, x.N, x.d, k, st, labels_dev, nullptr, nblocks, 0, 0, s));
                labelled = true;
            }
            OFC_TRY(relocate_empty());
            S.valid = 0;
            OFC_TRY(launch_lloyd_update(st, tot, k, x.d, 1, was_labelled, it + w == 0, Ng, tol_rel, sc->status_dev + w, s));
            OFC_HIP(hipStreamSynchronize(s));
            done = w + 1;
            if (S.converged) { strict = S.strict != 0; it += w; stop = true; }
            break;
        }
        if (S.converged) { strict = S.strict != 0; it += w; stop = true; break; }
    }
    if (!stop) it += done;
    return OFC_OK;
}

int LloydFit::final_sweep()
{
    const bool final_tiles = !strict && prune && !labelled && tiles_next == LLOYD_TILES_PRUNED;
    sc->prune_stats[5] = final_tiles ? 1 : 0;
    if (final_tiles)                        // the fit's tile metadata is valid and most tiles pass: those are not read
        return tiles_launch(labels_dev, LLOYD_WHAT_FINAL, nullptr);
    if (!strict) return lloyd_assign(x, k, st, labels_dev, partial, nblocks, 2, 0, s);
    return lloyd_inertia(x, st, labels_dev, partial, nblocks, s);
}

int LloydFit::read_back()
{
    OFC_TRY(launch_reduce_records(partial, nblocks, 1, tot, s));
    OFC_TRY(dist_allreduce_f64(tot, 1, DIST_SUM, s));
    double in = 0, cfin[LLOYD_KMAX * LLOYD_DMAX];
    OFC_HIP(hipMemcpyAsync(&in, tot, sizeof(double), hipMemcpyDeviceToHost, s));
    OFC_HIP(hipMemcpyAsync(cfin, st->centers, sizeof(double) * k * x.d, hipMemcpyDeviceToHost, s));
    OFC_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < k * x.d; j++) centers[j] = cfin[j] + mean_h[j % x.d];
    if (inertia) *inertia = in;
    if (n_iter) *n_iter = it + 1;
    return OFC_OK;
}

static int lloyd_fit_dev(LloydFit f)
{
    OFC_TRY(f.check());
    LloydScratch &sc = scratch_for(f.device);
    std::lock_guard<std::mutex> lock(sc.mu);
    OFC_TRY(sc.init());
    f.sc = &sc;
    f.s = sc.stream;
    f.st = sc.state.as<LloydState>();
    f.tot = sc.tot.as<double>();
    f.partial = sc.partial.as<double>();
    f.kmax = lloyd_kmax(f.k);
    f.NV = lloyd_record_len(f.kmax, f.x.d);
    f.nblocks = lloyd_grid(f.x.N);
    f.trace = getenv("OFC_LLOYD_TRACE") != nullptr;
    if (!f.labels_dev) {
        OFC_TRY(reserve(sc.labels, (size_t)std::max<int64_t>(f.x.N, 1)));
        f.labels_dev = sc.labels.as<uint8_t>();
    }
    OFC_HIP(hipMemsetAsync(f.st, 0, sizeof(LloydState), f.s));
    OFC_TRY(f.column_mean());
    OFC_TRY(f.centred_init());
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
    int window = 4;                       // 4, 8, 16, 16, ...: an 11-iteration fit costs two host round trips, and a fit
                                          // that meets its empty cluster early (iteration 1-2, typically) wastes few
    while (f.it < f.max_iter && !f.stop) {
        const int nwin = std::min(window, f.max_iter - f.it);
        window = std::min(2 * window, LLOYD_WINDOW);
        OFC_TRY(f.enqueue_window(nwin));
        OFC_TRY(f.read_window(nwin));
    }
    if (!f.stop) f.it = f.max_iter - 1;   // ran out of iterations: n_iter = max_iter
    OFC_TRY(f.final_sweep());
    return f.read_back();
}

static int lloyd_predict_dev(int device, const void *X, int dtype, int64_t N, int d, int k,
                             const double *centers, uint8_t *labels_dev)
{
    OFC_TRY(ensure_device(device));
    OFC_TRY(check_kd(k, d));
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

// host weights: finite, non-negative, positive sum (sklearn's _check_sample_weight + the zero-sum refusal)
static int check_host_weights(const void *w, int w_dtype, int64_t N)
{
    double sum = 0;
    for (int64_t i = 0; i < N; i++) {
        const double v = sample_elem(w, w_dtype, i);
        if (!std::isfinite(v)) { set_error("sample_weight[%lld] is not finite", (long long)i); return OFC_EINVAL; }
        if (v < 0) { set_error("sample_weight[%lld] is negative", (long long)i); return OFC_EINVAL; }
        sum += v;
    }
    if (!(sum > 0)) { set_error("sum of sample weights must be positive"); return OFC_EINVAL; }
    return OFC_OK;
}

// The calls on host buffers: h.X (and h.w) go up, each into room for at least 16 bytes, `run` works on the device copies and
// a label buffer, and the labels come back widened when the caller wants them.
template <class F> static int with_device_copy(const LloydSamples &h, int32_t *labels, F &&run)
{
    DevBuf dX, dW, dL;
    const size_t bytes = (size_t)h.N * h.d * dtype_size(h.dtype), wbytes = h.w ? (size_t)h.N * dtype_size(h.w_dtype) : 0;
    OFC_TRY(dX.alloc(std::max<size_t>(bytes, 16)));
    if (h.w) OFC_TRY(dW.alloc(std::max<size_t>(wbytes, 16)));
    OFC_TRY(dL.alloc((size_t)std::max<int64_t>(h.N, 1)));
    OFC_HIP(hipMemcpy(dX.p, h.X, bytes, hipMemcpyHostToDevice));
    if (h.w) OFC_HIP(hipMemcpy(dW.p, h.w, wbytes, hipMemcpyHostToDevice));
    OFC_TRY(run(LloydSamples{dX.p, h.dtype, h.N, h.d, h.w ? dW.p : nullptr, h.w_dtype}, dL.as<uint8_t>()));
    if (labels) {
        std::vector<uint8_t> l8((size_t)h.N);
        OFC_HIP(hipMemcpy(l8.data(), dL.p, (size_t)h.N, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < h.N; i++) labels[i] = l8[i];
    }
    return OFC_OK;
}

// ofc_kmeans_fit_w, and ofc_kmeans_fit with h.w == nullptr
static int lloyd_fit_host(int device, const LloydSamples &h, int k, const double *init, int max_iter, double tol_rel,
                          double *centers, int32_t *labels, double *inertia, int *n_iter)
{
    OFC_REQUIRE(h.X && init && centers, "null pointer");
    OFC_REQUIRE(h.dtype >= OFC_U8 && h.dtype <= OFC_F64 && h.d >= 1 && h.N >= 0, "bad arguments");
    if (h.w) OFC_TRY(check_w_dtype(h.w_dtype));
    OFC_REQUIRE(h.N >= k, "n_samples=%lld should be >= n_clusters=%d.", (long long)h.N, k);
    if (h.w) OFC_TRY(check_host_weights(h.w, h.w_dtype, h.N));
    OFC_TRY(ensure_device(device));
    return with_device_copy(h, labels, [&](const LloydSamples &x, uint8_t *lab) -> int {
        return lloyd_fit_dev({device, x, k, init, max_iter, tol_rel, centers, lab, inertia, n_iter});
    });
}

}  // namespace ofc

using namespace ofc;

extern "C" {

int ofc_kmeans_fit_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *init,
                       int max_iter, double tol_rel, double *centers, uint8_t *labels_dev, double *inertia,
                       int *n_iter)
{
    return lloyd_fit_dev({device, {X_dev, dtype, N, d}, k, init, max_iter, tol_rel, centers, labels_dev, inertia, n_iter});
}

int ofc_kmeans_fit_dev_stats(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *init,
                             int max_iter, double tol_rel, const double *colsum, double *centers, uint8_t *labels_dev,
                             double *inertia, int *n_iter)
{
    return lloyd_fit_dev({device, {X_dev, dtype, N, d}, k, init, max_iter, tol_rel, centers, labels_dev, inertia, n_iter, colsum});
}

/* see include/ofc.h */
int ofc_kmeans_fit_dev_field(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *init,
                             int max_iter, double tol_rel, const double *colsum, double *centers, uint8_t *labels_dev,
                             double *inertia, int *n_iter, int W, int H, int64_t n_fields)
{
    OFC_REQUIRE(dtype == OFC_F32 && d == 2, "a stack of (u,v) fields is float32 with d = 2 (got dtype %d, d = %d)", dtype, d);
    OFC_REQUIRE(W >= 1 && H >= 1 && n_fields >= 1 && N / W / H == n_fields && n_fields * W * H == N,
                "N=%lld is not %lld fields of %d x %d", (long long)N, (long long)n_fields, W, H);
    return lloyd_fit_dev({device, {X_dev, dtype, N, d}, k, init, max_iter, tol_rel, centers, labels_dev, inertia, n_iter, colsum,
                          W, H, n_fields});
}

/* ---- sample weights, see include/ofc.h ---- */
int ofc_kmeans_fit_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                         const double *init, int max_iter, double tol_rel, const double *colsum, double *centers,
                         uint8_t *labels_dev, double *inertia, int *n_iter)
{
    if (w_dev) OFC_TRY(check_w_dtype(w_dtype));
    return lloyd_fit_dev({device, {X_dev, dtype, N, d, w_dev, w_dtype}, k, init, max_iter, tol_rel, centers, labels_dev, inertia,
                          n_iter, colsum});
}

int ofc_kmeans_fit(int device, const void *X, int dtype, int64_t N, int d, int k, const double *init,
                   int max_iter, double tol_rel, double *centers, int32_t *labels, double *inertia, int *n_iter)
{
    return lloyd_fit_host(device, {X, dtype, N, d}, k, init, max_iter, tol_rel, centers, labels, inertia, n_iter);
}

int ofc_kmeans_fit_w(int device, const void *X, int dtype, const void *w, int w_dtype, int64_t N, int d, int k,
                     const double *init, int max_iter, double tol_rel, double *centers, int32_t *labels, double *inertia,
                     int *n_iter)
{
    OFC_REQUIRE(w, "null pointer");
    return lloyd_fit_host(device, {X, dtype, N, d, w, w_dtype}, k, init, max_iter, tol_rel, centers, labels, inertia, n_iter);
}

int ofc_kmeans_predict(int device, const void *X, int dtype, int64_t N, int d, int k, const double *centers,
                       int32_t *labels)
{
    OFC_REQUIRE(X && centers && labels, "null pointer");
    OFC_REQUIRE(dtype >= OFC_U8 && dtype <= OFC_F64 && d >= 1 && N >= 0 && k >= 1, "bad arguments");
    OFC_TRY(ensure_device(device));
    return with_device_copy({X, dtype, N, d}, labels, [&](const LloydSamples &x, uint8_t *lab) -> int {
        return lloyd_predict_dev(device, x.X, dtype, N, d, k, centers, lab);
    });
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
    return with_device_copy({X, dtype, N, d, w, w_dtype}, nullptr, [&](const LloydSamples &x, uint8_t *lab) -> int {
        // the centres as given (KMeans.score does not centre X): mean 0
        StepCtx c;
        double zero[LLOYD_DMAX] = {0, 0, 0, 0};
        OFC_TRY(c.open(device, N, 2, zero, centers, k, d));
        OFC_TRY(lloyd_assign(x, k, c.state.as<LloydState>(), lab, c.partial.as<double>(), c.nblocks, 2, 0, nullptr));
        OFC_TRY(launch_reduce_records(c.partial.as<double>(), c.nblocks, 1, c.tot.as<double>(), nullptr));
        OFC_HIP(hipMemcpy(inertia, c.tot.p, sizeof(double), hipMemcpyDeviceToHost));
        return OFC_OK;
    });
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

}  // extern "C"
