// lloyd_seed_api.cpp -- C ABI of libofc.so: k-means++ seeding (sklearn's _kmeans_plusplus, _kmeans.py:163-262) around the
// kernels of lloyd_seed.hip; see include/ofc.h.  The single step on host samples, the whole seeding on resident samples
// (with and without weights, on one rank or across the shards of a communicator) and the sampling kernels on their own.
#include "lloyd_host.h"

using namespace ofc;

namespace {
constexpr int KPP_IO_ROWS = 8, KPP_IO_STAGE = 8 + 8 * LLOYD_DMAX, KPP_IO_LEN = KPP_IO_STAGE + 192;

// potentials of the candidates the last sweep evaluated (this rank's share)
int kpp_local_pots(LloydScratch &sc, int nblocks, double *pots8)
{
    OFC_TRY(launch_reduce_records(sc.partial.as<double>(), nblocks, 8, sc.tot.as<double>(), sc.stream));
    OFC_HIP(hipMemcpyAsync(pots8, sc.tot.p, sizeof(double) * 8, hipMemcpyDeviceToHost, sc.stream));
    OFC_HIP(hipStreamSynchronize(sc.stream));
    return OFC_OK;
}

// The shard that owns a draw from a cumulative sum laid over the shards in rank order (sum[q] each): the first shard that
// holds(q) anything to draw and whose running sum hits(...) the draw; the last one that holds anything when none hits.
// What holds and what hits differ between the two draws on purpose (np.searchsorted's sides): they stand at the calls.
template <class Holds, class Hits> int kpp_owner(const std::vector<double> &sum, Holds holds, Hits hits)
{
    int owner = -1;
    double S = 0;
    for (int q = 0; q < (int)sum.size(); q++) {
        if (holds(q)) {
            owner = q;
            if (hits(S + sum[q])) break;
        }
        S += sum[q];
    }
    return owner;
}

// ofc_kpp_seed_dev (x.w == nullptr: `first` is the first centre) and ofc_kpp_seed_dev_w (x.w: u_first draws it)
int kpp_seed(int device, const LloydSamples &x, int k, const double *colsum, int64_t first, double u_first, const double *u,
             int n_trials, double *centers, int64_t *indices)
{
    const int64_t N = x.N;
    const int d = x.d;
    OFC_REQUIRE(x.X && centers && indices && (u || k == 1), "null pointer");
    OFC_REQUIRE(x.dtype >= OFC_U8 && x.dtype <= OFC_F64, "bad dtype %d", x.dtype);
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
        OFC_REQUIRE(x.w || first < N, "first=%lld outside 0..%lld", (long long)first, (long long)N - 1);
    }
    OFC_TRY(ensure_device(device));
    LloydScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    OFC_TRY(sc.init());
    hipStream_t s = sc.stream;
    if (!sc.kpp_io.p) OFC_TRY(sc.kpp_io.alloc(sizeof(double) * KPP_IO_LEN));
    int64_t *idx_dev = sc.kpp_io.as<int64_t>();
    double *rows_dev = sc.kpp_io.as<double>() + KPP_IO_ROWS;
    // all-reduce of a few host doubles through the seeding scratch (no-op without a communicator)
    auto exchange = [&](double *h, int count, int op) {
        return host_allreduce(sc.kpp_io.as<double>() + KPP_IO_STAGE, h, count, op, s);
    };

    // ---- shard layout: global row order is rank order ----
    std::vector<double> nq(world, 0.0), pq(world, 0.0);
    nq[rank] = (double)N;
    OFC_TRY(exchange(nq.data(), world, DIST_SUM));
    double Ng = 0, off_me = 0;
    for (int q = 0; q < world; q++) {
        if (q < rank) off_me += nq[q];
        Ng += nq[q];
    }
    OFC_REQUIRE(Ng >= (double)k, "n_samples=%.0f should be >= n_clusters=%d.", Ng, k);
    OFC_REQUIRE(x.w || (double)first < Ng, "first=%lld outside 0..%.0f", (long long)first, Ng - 1);
    if (nq[rank] != (double)N) { set_error("the communicator does not lay the shards out by rank"); return OFC_EUNSUPPORTED; }

    // ---- column mean, as the fit forms it ----
    double *tot = sc.tot.as<double>();
    double hbuf[LLOYD_DMAX], mean_h[LLOYD_DMAX];
    const int nb_stats = lloyd_grid(N);
    if (colsum) {
        memcpy(hbuf, colsum, sizeof(double) * d);
    } else {
        LloydState *st = sc.state.as<LloydState>();
        OFC_TRY(launch_lloyd_colstats(x.X, x.dtype, N, d, st->mean, 0, sc.partial.as<double>(), nb_stats, s));
        OFC_TRY(launch_reduce_records(sc.partial.as<double>(), nb_stats, d, tot, s));
        OFC_HIP(hipMemcpyAsync(hbuf, tot, sizeof(double) * d, hipMemcpyDeviceToHost, s));
        OFC_HIP(hipStreamSynchronize(s));
    }
    OFC_TRY(exchange(hbuf, d, DIST_SUM));
    for (int f = 0; f < d; f++) mean_h[f] = hbuf[f] / Ng;

    const int64_t nchunks = kpp_chunks(N);
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(nchunks, 4), 2048));
    if (N > 0) {
        OFC_TRY(reserve(sc.kpp_closest, sizeof(double) * (size_t)N));
        OFC_TRY(reserve(sc.kpp_cs, sizeof(double) * 8 * (size_t)nchunks));
        OFC_TRY(reserve(sc.kpp_ss, sizeof(double) * (size_t)cdiv64(nchunks, 1024)));
    }
    double *closest = sc.kpp_closest.as<double>(), *cs = sc.kpp_cs.as<double>(), *ss = sc.kpp_ss.as<double>();
    auto sweep = [&](const double *prev, int prev_mode, const double *cand, int n_cand) {
        if (x.w)
            return launch_kpp_sweep_w(x.X, x.dtype, x.w, x.w_dtype, N, d, mean_h, prev, prev_mode, cand, n_cand, closest, cs,
                                      sc.partial.as<double>(), nblocks, s);
        return launch_kpp_sweep(x.X, x.dtype, N, d, mean_h, prev, prev_mode, cand, n_cand, closest, cs,
                                sc.partial.as<double>(), nblocks, s);
    };

    // ---- with weights, the first centre is drawn as RandomState.choice(N, p=w/w.sum()) draws it (_kmeans.py:224):
    //      the smallest global row whose cumulative weight exceeds u_first * W ----
    if (x.w) {
        pq[rank] = 0;
        if (N > 0) {
            OFC_TRY(launch_kpp_wchunks(x.w, x.w_dtype, nullptr, N, cs, s));
            OFC_TRY(launch_kpp_sum1024(cs, nchunks, ss, s));
            OFC_TRY(launch_kpp_total(ss, (int)cdiv64(nchunks, 1024), sc.tot.as<double>(), s));
            OFC_HIP(hipMemcpyAsync(&pq[rank], sc.tot.p, sizeof(double), hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
        }
        OFC_TRY(exchange(pq.data(), world, DIST_SUM));
        double W = 0, base_me = 0;
        for (int q = 0; q < world; q++) W += pq[q];
        for (int q = 0; q < rank; q++) base_me += pq[q];
        if (!(W > 0)) { set_error("sum of sample weights must be positive"); return OFC_EINVAL; }
        const double r = u_first * W;
        // RandomState.choice: the first shard of positive weight whose running sum EXCEEDS r (side = right)
        const int owner = kpp_owner(pq, [&](int q) { return pq[q] > 0; }, [&](double cum) { return cum > r; });
        double gi = 0;
        if (owner == rank) {
            int64_t li;
            OFC_TRY(launch_kpp_sample_w(x.X, x.dtype, x.w, x.w_dtype, N, d, mean_h, nullptr, KPP_PREV_NONE, nullptr, cs, ss,
                                        &r, 1, base_me, KPP_SIDE_FIRST, idx_dev, rows_dev, s));
            OFC_HIP(hipMemcpyAsync(&li, idx_dev, sizeof(int64_t), hipMemcpyDeviceToHost, s));
            OFC_HIP(hipStreamSynchronize(s));
            gi = off_me + (double)li;
        }
        OFC_TRY(exchange(&gi, 1, DIST_BCAST));
        first = (int64_t)gi;
    }

    // ---- first centre: its owner broadcasts the row ----
    double rec[8 * (LLOYD_DMAX + 1)];
    memset(rec, 0, sizeof(rec));
    if ((double)first >= off_me && (double)first < off_me + (double)N) {
        unsigned char raw[LLOYD_DMAX * 8];
        OFC_HIP(hipMemcpyAsync(raw, row_ptr(x, first - (int64_t)off_me), row_size(x), hipMemcpyDeviceToHost, s));
        OFC_HIP(hipStreamSynchronize(s));
        for (int f = 0; f < d; f++) rec[f] = sample_elem(raw, x.dtype, f);
    }
    OFC_TRY(exchange(rec, d, DIST_BCAST));
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
    OFC_TRY(exchange(pg, 8, DIST_SUM));
    double current_pot = pg[0], pot_local = pl[0];
    int slot = 0;                 // whose chunk sums (cs[slot], summed into ss) describe closest with `prev` folded in

    for (int c = 1; c < k; c++) {
        // ---- sample n_trials rows from the cumulative sum of closest (_kmeans.py:242-247) ----
        const int prev_mode = c >= 2 ? KPP_PREV_APPLY : KPP_PREV_NONE;
        double r[8];
        for (int j = 0; j < n_trials; j++) r[j] = u[(size_t)(c - 1) * n_trials + j] * current_pot;
        for (double &v : pq) v = 0;
        pq[rank] = pot_local;
        OFC_TRY(exchange(pq.data(), world, DIST_SUM));
        double base_me = 0;
        for (int q = 0; q < rank; q++) base_me += pq[q];
        bool mine[8], any = false;
        for (int j = 0; j < n_trials; j++) {
            // np.searchsorted, clipped: the first non-empty shard whose cumulative sum REACHES r[j] (side = left)
            mine[j] = kpp_owner(pq, [&](int q) { return nq[q] > 0; }, [&](double cum) { return cum >= r[j]; }) == rank;
            any = any || mine[j];
        }
        memset(rec, 0, sizeof(rec));
        if (any) {
            int64_t idx_h[8];
            double rows_h[8 * LLOYD_DMAX];
            if (x.w)
                OFC_TRY(launch_kpp_sample_w(x.X, x.dtype, x.w, x.w_dtype, N, d, mean_h, prev, prev_mode, closest,
                                            cs + (size_t)slot * nchunks, ss, r, n_trials, base_me, KPP_SIDE_LEFT, idx_dev,
                                            rows_dev, s));
            else
                OFC_TRY(launch_kpp_sample(x.X, x.dtype, N, d, mean_h, prev, prev_mode, closest,
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
        OFC_TRY(exchange(rec, n_trials * (d + 1), DIST_BCAST));
        double cand[8 * LLOYD_DMAX];
        for (int j = 0; j < n_trials; j++)
            for (int f = 0; f < d; f++) cand[j * d + f] = rec[j * (d + 1) + f] - mean_h[f];

        // ---- one sweep: fold the previous winner into closest, evaluate the candidates (:250-256) ----
        for (double &v : pl) v = 0;
        if (N > 0) {
            OFC_TRY(sweep(prev, prev_mode, cand, n_trials));
            OFC_TRY(kpp_local_pots(sc, nblocks, pl));
        }
        memcpy(pg, pl, sizeof(pg));
        OFC_TRY(exchange(pg, 8, DIST_SUM));
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

}  // namespace

extern "C" {

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
    for (int c = 0; c < n_cand; c++) row_centred(row_ptr({X, dtype, N, d}, cand[c]), dtype, d, mean, &cc[(size_t)c * d]);
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
int ofc_kpp_seed_dev(int device, const void *X_dev, int dtype, int64_t N, int d, int k, const double *colsum,
                     int64_t first, const double *u, int n_trials, double *centers, int64_t *indices)
{
    return kpp_seed(device, {X_dev, dtype, N, d}, k, colsum, first, 0.0, u, n_trials, centers, indices);
}

int ofc_kpp_seed_dev_w(int device, const void *X_dev, int dtype, const void *w_dev, int w_dtype, int64_t N, int d, int k,
                       const double *colsum, double u_first, const double *u, int n_trials, double *centers,
                       int64_t *indices)
{
    OFC_REQUIRE(w_dev, "null weight pointer");
    OFC_TRY(check_w_dtype(w_dtype));
    OFC_REQUIRE((uintptr_t)w_dev % 16 == 0, "the weights must be 16-byte aligned");
    return kpp_seed(device, {X_dev, dtype, N, d, w_dev, w_dtype}, k, colsum, 0, u_first, u, n_trials, centers, indices);
}

// what both sampling exports refuse: n outside 1..8, nothing to sample from, more than the kernels scan
static int kpp_sample_check(int n, int64_t N)
{
    OFC_REQUIRE(n >= 1 && n <= 8, "n %d outside 1..8", n);
    OFC_REQUIRE(N >= 1, "N=%lld: nothing to sample from", (long long)N);
    if (N > KPP_NMAX) {
        set_error("N=%lld outside the seeding kernels' range (<= %lld samples)", (long long)N, (long long)KPP_NMAX);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

int ofc_kpp_sample_dev_w(int device, const void *w_dev, int w_dtype, const double *v_dev, int64_t N, const double *r, int n,
                         int side, int64_t *idx, double *total)
{
    OFC_REQUIRE(w_dev && r && idx && total, "null pointer");
    OFC_TRY(check_w_dtype(w_dtype));
    OFC_REQUIRE((uintptr_t)w_dev % 16 == 0, "the weights must be 16-byte aligned");
    OFC_REQUIRE(side == 0 || side == 1, "side %d: 0 (left) or 1 (right)", side);
    OFC_TRY(kpp_sample_check(n, N));
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
    OFC_TRY(kpp_sample_check(n, N));
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

}  // extern "C"
