// lloyd_steps_api.cpp -- C ABI of libofc.so: the host-driven building blocks of Lloyd's k-means (sharded.py drives them the
// way lloyd_fit.cpp drives the same kernels in the library), the geometry of the field tiles, and the measurement hooks of
// the sweeps.  Every block runs on the null stream with a state of its own (StepCtx); the weighted and the plain export of
// a block are the same function with and without weights.
#include "lloyd_host.h"

using namespace ofc;

namespace {

int lloyd_step(int device, const LloydSamples &x, int k, const double *mean, const double *centers_c, uint8_t *labels_dev,
               int accumulate, double *record)
{
    const int kmax = lloyd_kmax(k), NV = lloyd_record_len(kmax, x.d);
    StepCtx c;
    OFC_TRY(c.open(device, x.N, NV, mean, centers_c, k, x.d));
    OFC_TRY(lloyd_assign(x, k, c.state.as<LloydState>(), labels_dev, c.partial.as<double>(), c.nblocks, accumulate ? 1 : 0, 0,
                         nullptr));
    if (accumulate) {
        OFC_TRY(launch_reduce_records(c.partial.as<double>(), c.nblocks, NV, c.tot.as<double>(), nullptr));
        std::vector<double> t(NV);
        OFC_HIP(hipMemcpy(t.data(), c.tot.p, sizeof(double) * NV, hipMemcpyDeviceToHost));
        for (int j = 0; j < k; j++) {       // the caller's k-wide [sums | counts | inertia] out of the kmax-wide record
            for (int f = 0; f < x.d; f++) record[j * x.d + f] = t[j * x.d + f];
            record[k * x.d + j] = t[kmax * x.d + j];
        }
        record[k * x.d + k] = t[kmax * x.d + kmax];
    } else {
        OFC_HIP(hipStreamSynchronize(nullptr));
    }
    return OFC_OK;
}

int lloyd_inertia_step(int device, const LloydSamples &x, int k, const double *mean, const double *centers_c,
                       const uint8_t *labels_dev, double *inertia)
{
    StepCtx c;
    OFC_TRY(c.open(device, x.N, 2, mean, centers_c, k, x.d));
    OFC_TRY(lloyd_inertia(x, c.state.as<LloydState>(), labels_dev, c.partial.as<double>(), c.nblocks, nullptr));
    OFC_TRY(launch_reduce_records(c.partial.as<double>(), c.nblocks, 1, c.tot.as<double>(), nullptr));
    OFC_HIP(hipMemcpy(inertia, c.tot.p, sizeof(double), hipMemcpyDeviceToHost));
    return OFC_OK;
}

// the farthest sample by its UNWEIGHTED distance; weight != nullptr: and its weight (0 when there is no sample)
int lloyd_farthest_step(int device, const LloydSamples &x, int k, const double *mean, const double *centers_c,
                        const uint8_t *labels_dev, const int64_t *excl, int n_excl, double *dist2, int64_t *index, double *x_c,
                        int *label, double *weight)
{
    OFC_REQUIRE(x.X && mean && centers_c && labels_dev && dist2 && index && x_c && label && x.N >= 0, "bad arguments");
    OFC_REQUIRE(n_excl >= 0 && n_excl <= LLOYD_KMAX && (n_excl == 0 || excl), "bad exclusion list");
    StepCtx c;
    OFC_TRY(c.open(device, x.N, 2, mean, centers_c, k, x.d));
    OFC_TRY(c.excl.alloc(sizeof(int64_t) * LLOYD_KMAX));
    if (n_excl) OFC_HIP(hipMemcpy(c.excl.p, excl, sizeof(int64_t) * n_excl, hipMemcpyHostToDevice));
    LloydState *st = c.state.as<LloydState>();
    OFC_TRY(launch_lloyd_farthest(x.X, x.dtype, x.N, x.d, st, st->centers, labels_dev, c.excl.as<int64_t>(), n_excl,
                                  c.partial.as<double>(), c.nblocks, nullptr));
    std::vector<double> blk(2 * c.nblocks);
    OFC_HIP(hipMemcpy(blk.data(), c.partial.p, sizeof(double) * 2 * c.nblocks, hipMemcpyDeviceToHost));
    double best;
    const int64_t bi = farthest_pick(blk.data(), c.nblocks, best);
    *dist2 = bi >= 0 ? best : -1;
    *index = bi;
    *label = -1;
    if (weight) *weight = 0.0;
    if (bi >= 0) {
        unsigned char raw[LLOYD_DMAX * 8];
        uint8_t lab;
        OFC_HIP(hipMemcpy(raw, row_ptr(x, bi), row_size(x), hipMemcpyDeviceToHost));
        OFC_HIP(hipMemcpy(&lab, labels_dev + bi, 1, hipMemcpyDeviceToHost));
        row_centred(raw, x.dtype, x.d, mean, x_c);
        *label = lab;
        if (weight) {
            const size_t ws = dtype_size(x.w_dtype);
            OFC_HIP(hipMemcpy(raw, (const char *)x.w + (size_t)bi * ws, ws, hipMemcpyDeviceToHost));
            *weight = sample_elem(raw, x.w_dtype, 0);
        }
    }
    return OFC_OK;
}

}  // namespace

extern "C" {

int ofc_lloyd_colstats_dev(int device, const void *X_dev, int dtype, int64_t N, int d, const double *mean, int pass,
                           double *out)
{
    OFC_REQUIRE(X_dev && out && N >= 0 && (pass == 0 || mean), "bad arguments");
    StepCtx c;
    OFC_TRY(c.open(device, N, d, pass ? mean : nullptr, nullptr, 1, d));
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
    return lloyd_step(device, {X_dev, dtype, N, d}, k, mean, centers_c, labels_dev, accumulate, record);
}

int ofc_lloyd_step_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                         const double *mean, const double *centers_c, uint8_t *labels_dev, double *record)
{
    OFC_REQUIRE(X_dev && w_dev && mean && centers_c && labels_dev && record && N >= 0, "bad arguments");
    OFC_TRY(check_w_dtype(w_dtype));
    return lloyd_step(device, {X_dev, dtype, N, d, w_dev, w_dtype}, k, mean, centers_c, labels_dev, 1, record);
}

int ofc_lloyd_inertia_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *mean,
                          const double *centers_c, const uint8_t *labels_dev, double *inertia)
{
    OFC_REQUIRE(X_dev && mean && centers_c && labels_dev && inertia && N >= 0, "bad arguments");
    return lloyd_inertia_step(device, {X_dev, dtype, N, d}, k, mean, centers_c, labels_dev, inertia);
}

int ofc_lloyd_inertia_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                            const double *mean, const double *centers_c, const uint8_t *labels_dev, double *inertia)
{
    OFC_REQUIRE(X_dev && w_dev && mean && centers_c && labels_dev && inertia && N >= 0, "bad arguments");
    OFC_TRY(check_w_dtype(w_dtype));
    return lloyd_inertia_step(device, {X_dev, dtype, N, d, w_dev, w_dtype}, k, mean, centers_c, labels_dev, inertia);
}

int ofc_lloyd_farthest_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *mean,
                           const double *centers_c, const uint8_t *labels_dev, const int64_t *excl, int n_excl,
                           double *dist2, int64_t *index, double *x_c, int *label)
{
    return lloyd_farthest_step(device, {X_dev, dtype, N, d}, k, mean, centers_c, labels_dev, excl, n_excl, dist2, index, x_c,
                               label, nullptr);
}

int ofc_lloyd_farthest_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                             const double *mean, const double *centers_c, const uint8_t *labels_dev, const int64_t *excl,
                             int n_excl, double *dist2, int64_t *index, double *x_c, int *label, double *weight)
{
    OFC_REQUIRE(w_dev && weight, "bad arguments");
    OFC_TRY(check_w_dtype(w_dtype));
    return lloyd_farthest_step(device, {X_dev, dtype, N, d, w_dev, w_dtype}, k, mean, centers_c, labels_dev, excl, n_excl, dist2,
                               index, x_c, label, weight);
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
    const double zero[2] = {0.0, 0.0};
    StepCtx c;
    OFC_TRY(c.open(device, 0, 2, mean ? mean : zero, centers_c, k, 2));
    OFC_TRY(launch_grid_assign_counts(flow_dev, c.state.as<LloydState>(), W, H, n_frames, rows, cols, k, counts_dev, sums_dev,
                                      nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
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
    OFC_TRY(set_centred_model(sc, mean, centers, k, 2, LLOYD_PRUNE_ALWAYS, c0));
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
    const int nblocks = lloyd_grid(N);
    LloydState *st = sc.state.as<LloydState>();
    OFC_HIP(hipMemsetAsync(st, 0, sizeof(LloydState), sc.stream));
    double c0[LLOYD_KMAX * LLOYD_DMAX];
    OFC_TRY(set_centred_model(sc, mean, centers, k, 2, LLOYD_PRUNE_OFF, c0));
    auto launch = [&]() -> int {
        return launch_lloyd_assign_w(X_dev, OFC_F32, w_dev, w_dtype, N, 2, k, st, nullptr, sc.partial.as<double>(), nblocks, 3, 0,
                                     sc.stream);
    };
    return time_launches(sc.stream, iters, launch, ms_per_launch);
}

}  // extern "C"
