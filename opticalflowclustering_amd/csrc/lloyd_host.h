// lloyd_host.h -- what the Lloyd host files of libofc.so share: lloyd_fit.cpp (the clip-wide fit), lloyd_steps_api.cpp (the
// host-driven building blocks and the measurement hooks) and lloyd_seed_api.cpp (k-means++ seeding).  The per-device scratch,
// the argument checks, and one helper for each thing more than one of them does.  Included by those three files only.
#pragma once
#include "host_util.h"
#include "lloyd_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>

namespace ofc {

// work-groups of a streaming sweep: enough lanes to keep the memory system full, few enough that the fixed-order record
// reduction stays short (it is a visible share of an iteration on a 1/8 shard)
inline int lloyd_grid(int64_t N)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(N / 4, 256), N >= (200ll << 20) ? 2048 : 1024));
}

inline size_t dtype_size(int dtype) { return dtype == OFC_U8 ? 1 : (dtype == OFC_F32 ? 4 : 8); }

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

inline LloydScratch &scratch_for(int device) { return device_scratch<LloydScratch>(device); }

inline int check_kd(int k, int d)
{
    if (d < 1 || k < 1 || d > LLOYD_DMAX || k > LLOYD_KMAX) {
        set_error("k=%d, d=%d outside the kernels' range (k <= %d, d <= %d)", k, d, LLOYD_KMAX, LLOYD_DMAX);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

inline int check_w_dtype(int w_dtype)
{
    OFC_REQUIRE(w_dtype == OFC_F32 || w_dtype == OFC_F64, "bad weight dtype %d (OFC_F32 or OFC_F64)", w_dtype);
    return OFC_OK;
}

// The samples of a call: X[N][d] of `dtype` and, when the call is weighted, w[N] of `w_dtype` (16-byte aligned).
struct LloydSamples {
    const void *X;
    int dtype;
    int64_t N;
    int d;
    const void *w = nullptr;
    int w_dtype = OFC_F32;
};

// The state of a call on the null stream (the host-driven building blocks and ofc_kmeans_score): made and released per call.
struct StepCtx {
    DevBuf state, partial, tot, excl, far;
    int nblocks = 1;
    // k and d in range, the device current; then room for records of nv doubles over N samples, and the model (either
    // part may be nullptr) in a zeroed state
    int open(int device, int64_t N, int nv, const double *mean, const double *centers_c, int k, int d)
    {
        OFC_TRY(check_kd(k, d));
        OFC_TRY(ensure_device(device));
        nblocks = lloyd_grid(N);
        OFC_TRY(state.alloc(sizeof(LloydState)));
        OFC_TRY(partial.alloc(sizeof(double) * (size_t)nblocks * std::max(nv, 2)));
        OFC_TRY(tot.alloc(sizeof(double) * (nv + 8)));
        OFC_HIP(hipMemset(state.p, 0, sizeof(LloydState)));
        LloydState *st = state.as<LloydState>();
        if (mean) OFC_HIP(hipMemcpy(st->mean, mean, sizeof(double) * d, hipMemcpyHostToDevice));
        if (centers_c) {
            OFC_HIP(hipMemcpy(st->centers, centers_c, sizeof(double) * k * d, hipMemcpyHostToDevice));
            OFC_TRY(launch_lloyd_set_centers(st, k, d, nullptr));
        }
        return OFC_OK;
    }
};

// ---- weighted or plain: one dispatch per launcher, by whether the samples carry weights ----
inline int lloyd_assign(const LloydSamples &x, int k, const LloydState *st, uint8_t *labels, double *partial, int nblocks,
                        int mode, int first, hipStream_t s)
{
    if (x.w) return launch_lloyd_assign_w(x.X, x.dtype, x.w, x.w_dtype, x.N, x.d, k, st, labels, partial, nblocks, mode, first, s);
    return launch_lloyd_assign(x.X, x.dtype, x.N, x.d, k, st, labels, partial, nblocks, mode, first, s);
}

inline int lloyd_inertia(const LloydSamples &x, const LloydState *st, const uint8_t *labels, double *partial, int nblocks,
                         hipStream_t s)
{
    if (x.w) return launch_lloyd_inertia_w(x.X, x.dtype, x.w, x.w_dtype, x.N, x.d, st, labels, partial, nblocks, s);
    return launch_lloyd_inertia(x.X, x.dtype, x.N, x.d, st, labels, partial, nblocks, s);
}

// element f of a raw sample of `dtype`
inline double sample_elem(const void *raw, int dtype, int64_t f)
{
    return dtype == OFC_U8 ? (double)((const uint8_t *)raw)[f]
         : dtype == OFC_F32 ? (double)((const float *)raw)[f] : ((const double *)raw)[f];
}

// bytes of one sample, and where sample i starts
inline size_t row_size(const LloydSamples &x) { return x.d * dtype_size(x.dtype); }
inline const char *row_ptr(const LloydSamples &x, int64_t i) { return (const char *)x.X + (size_t)i * row_size(x); }

// out[d] = the raw sample minus `mean`
inline void row_centred(const void *raw, int dtype, int d, const double *mean, double *out)
{
    for (int f = 0; f < d; f++) out[f] = sample_elem(raw, dtype, f) - mean[f];
}

// The farthest sample among launch_lloyd_farthest's per-block (dist, index) pairs: largest distance, ties to the lowest
// index.  Returns its index and sets `best` to its distance; -1 (best = -1) when no block found one.
inline int64_t farthest_pick(const double *blk, int nblocks, double &best)
{
    best = -1;
    int64_t bi = -1;
    for (int b = 0; b < nblocks; b++) {
        const double v = blk[2 * b];
        const int64_t i = (int64_t)blk[2 * b + 1];
        if (i < 0) continue;
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    }
    return bi;
}

// All-reduce of a few host doubles through the device staging area `stage`.  Without a communicator it does nothing: no
// copy, no synchronisation.
inline int host_allreduce(double *stage, double *h, int count, int op, hipStream_t s)
{
    if (!dist_active()) return OFC_OK;
    OFC_HIP(hipMemcpyAsync(stage, h, sizeof(double) * count, hipMemcpyHostToDevice, s));
    OFC_TRY(dist_allreduce_f64(stage, count, op, s));
    OFC_HIP(hipMemcpyAsync(h, stage, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    OFC_HIP(hipStreamSynchronize(s));
    return OFC_OK;
}

// The centred model (mean, centres - mean) into the scratch state, and what k_lloyd_set_centers derives from it.  The copies
// are only enqueued: mean and c0 (room for k * d doubles) are the caller's and live until it next synchronises the stream.
inline int set_centred_model(LloydScratch &sc, const double *mean, const double *centers, int k, int d, int prune_policy,
                             double *c0)
{
    LloydState *st = sc.state.as<LloydState>();
    for (int j = 0; j < k * d; j++) c0[j] = centers[j] - mean[j % d];
    OFC_HIP(hipMemcpyAsync(st->mean, mean, sizeof(double) * d, hipMemcpyHostToDevice, sc.stream));
    OFC_HIP(hipMemcpyAsync(st->centers, c0, sizeof(double) * k * d, hipMemcpyHostToDevice, sc.stream));
    return launch_lloyd_set_centers(st, k, d, sc.stream, prune_policy);
}

}  // namespace ofc
