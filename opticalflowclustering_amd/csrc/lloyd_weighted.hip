// lloyd_weighted.hip -- the Lloyd sweeps with sample weights (sklearn's KMeans.fit(X, sample_weight=w)), and the kernel
// that derives such weights from a resident (u,v) field.
// Arithmetic = sklearn's (_k_means_lloyd.pyx, _k_means_common.pyx:165-210): the E-step does not see the weights; the M-step
// adds x_c * w (the product rounded on its own, then added: no FMA) into the sums and w into weight_in_clusters; the
// inertia adds |x_c - c_label|^2 * w.  Everything f64 whatever the storage dtypes.
// Design = k_lloyd_assign's (lloyd_kernels.hip): four samples per lane, the (u,v) f32 stream requested one quad ahead,
// per-lane private LDS accumulators -- here [k*d sums f64][k weights f64] -- folded in a fixed order, no atomics.  The
// record layout is unchanged; the count slots hold the weight sums.
#include "lloyd_device.h"

#include <algorithm>
#include <type_traits>

namespace ofc {

// lanes per work-group: the accumulators take k*(8d+8) B per lane, 160 KiB (the whole CU) for 256 lanes at k = 16, d = 4,
// which leaves no room for the kernel's static LDS; that instantiation runs 128-lane work-groups.  The fold below is
// written for any number of waves, the order inside it is fixed per instantiation.
template <int D, int KMAX> struct LloydWLanes { static constexpr int value = (KMAX == 16 && D == 4) ? 128 : 256; };

template <int NV, int NW>
__device__ __forceinline__ void block_reduce_store_w(double (&v)[NV], double *lds /*[NW][NV]*/, double *out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        double a = v[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) lds[wave * NV + i] = a;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int i = threadIdx.x;
        double r = lds[i];
#pragma unroll
        for (int w = 1; w < NW; w++) r += lds[w * NV + i];
        out[i] = r;
    }
    __syncthreads();
}

// the label is lloyd_device.h's assign_point.  sq_euclid_grouped_w repeats lloyd_kernels.hip's sq_euclid_grouped word for
// word: that file and its instantiations stay as they are
template <int D>
__device__ __forceinline__ double sq_euclid_grouped_w(const double (&a)[D], const double *b)
{
#pragma clang fp contract(off)
    double r = 0;
    int f = 0;
#pragma unroll
    for (; f + 4 <= D; f += 4)
        r += ((a[f] - b[f]) * (a[f] - b[f]) + (a[f + 1] - b[f + 1]) * (a[f + 1] - b[f + 1]) +
              (a[f + 2] - b[f + 2]) * (a[f + 2] - b[f + 2]) + (a[f + 3] - b[f + 3]) * (a[f + 3] - b[f + 3]));
#pragma unroll
    for (; f < D; f++) r += (a[f] - b[f]) * (a[f] - b[f]);
    return r;
}

// t rounded on its own: the caller adds it (x * w, then +=, as sklearn's C does)
__device__ __forceinline__ double mul_rounded(double a, double b)
{
#pragma clang fp contract(off)
    const double t = a * b;
    return t;
}

// four consecutive weights of a lane's quad as doubles
template <class TW>
__device__ __forceinline__ void load4w(const TW *W, int64_t q, double (&w)[4])
{
    if constexpr (std::is_same<TW, float>::value) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f a = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(W) + q);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    } else {
        typedef double v2d __attribute__((ext_vector_type(2)));
        const v2d a = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(W) + 2 * q);
        const v2d b = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(W) + 2 * q + 1);
        w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y;
    }
}

// MODE 1: labels + weighted M-step record (with `first` also the UNWEIGHTED column sums of (x-mean)^2: sklearn's tol does not
// see the weights, _kmeans.py:1479-1484); 2: labels + weighted inertia; 3: record only (labels neither read nor written).
// Record per work-group as k_lloyd_assign's: [KMAX*D sums of (x-mean)*w][KMAX weight sums][n_changed (labels)][...].
template <int D, int KMAX, class T, class TW, int MODE>
__global__ __launch_bounds__((LloydWLanes<D, KMAX>::value)) void k_lloyd_assign_w(
    const T *__restrict__ X, const TW *__restrict__ W, int64_t N, int k_arg, const LloydState *__restrict__ st,
    uint8_t *__restrict__ labels, double *__restrict__ partial, int first)
{
    constexpr int LANES = LloydWLanes<D, KMAX>::value, NW = LANES / 64;
    const int k = KMAX <= 8 ? KMAX : k_arg;
    constexpr bool ACCUM = (MODE == 1 || MODE == 3), LABELS = (MODE != 3);
    if (ACCUM && st->halt) return;      // speculatively enqueued behind the iteration that converged (uniform)
    constexpr int NV = KMAX * D + KMAX + LLOYD_REC_EXTRA;
    extern __shared__ __align__(16) unsigned char smem[];
    double *sacc = reinterpret_cast<double *>(smem);       // [k*D][LANES]
    double *swt = sacc + (size_t)k * D * LANES;            // [k][LANES]
    __shared__ unsigned s_changed[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double c[KMAX * D], cn[KMAX], m[D];
#pragma unroll
    for (int j = 0; j < KMAX; j++) {
        cn[j] = (j < k) ? st->cn[j] : 0.0;
#pragma unroll
        for (int f = 0; f < D; f++) c[j * D + f] = (j < k) ? st->centers[j * D + f] : 0.0;
    }
#pragma unroll
    for (int f = 0; f < D; f++) m[f] = st->mean[f];
    if (ACCUM)
        for (int i = 0; i < k * D + k; i++) sacc[i * LANES + tid] = 0.0;
    unsigned changed = 0;
    double sq[D], inert = 0;
#pragma unroll
    for (int f = 0; f < D; f++) sq[f] = 0;
    auto accumulate = [&](int l, const double (&x)[D], double w) {
#pragma unroll
        for (int f = 0; f < D; f++) sacc[(l * D + f) * LANES + tid] += mul_rounded(x[f], w);
        swt[l * LANES + tid] += w;
    };

    const int64_t n4 = N / 4;
    auto process = [&](int64_t q, double (&x)[4][D], const double (&w)[4], unsigned lo) {
        const int old[4] = {(int)(lo & 255u), (int)((lo >> 8) & 255u), (int)((lo >> 16) & 255u), (int)(lo >> 24)};
        int nl[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
#pragma unroll
            for (int f = 0; f < D; f++) x[p][f] -= m[f];
            nl[p] = assign_point<D, KMAX>(x[p], c, cn, k);
        }
        if (ACCUM) {
#pragma unroll
            for (int p = 0; p < 4; p++) {
                accumulate(nl[p], x[p], w[p]);
                if (MODE == 1) changed += (nl[p] != old[p]);
            }
            if (first) {
#pragma unroll
                for (int p = 0; p < 4; p++)
#pragma unroll
                    for (int f = 0; f < D; f++) sq[f] += x[p][f] * x[p][f];
            }
        }
        if (MODE == 2) {
#pragma unroll
            for (int p = 0; p < 4; p++)
                inert += mul_rounded(sq_euclid_grouped_w<D>(x[p], st->centers + nl[p] * D), w[p]);
        }
        if (LABELS)
            __builtin_nontemporal_store((unsigned)(nl[0] | (nl[1] << 8) | (nl[2] << 16) | (nl[3] << 24)),
                                        reinterpret_cast<unsigned *>(labels) + q);
    };
    const int64_t q0 = (int64_t)blockIdx.x * LANES + tid, qs = (int64_t)gridDim.x * LANES;
    if constexpr (std::is_same<T, float>::value && D == 2) {
        // the (u,v) stream: the next quad's 32 bytes and its weights (16 B as f32, 32 B as f64) are requested before the
        // current quad is processed, as in k_lloyd_assign
        typedef float v4f __attribute__((ext_vector_type(4)));
        auto raw = [&](int64_t q, v4f &a, v4f &b, double (&w)[4], unsigned &lo) {
            a = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(X + q * 8));
            b = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(X + q * 8 + 4));
            load4w<TW>(W, q, w);
            lo = MODE == 1 ? __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(labels) + q) : 0u;
        };
        v4f na = {0, 0, 0, 0}, nb = {0, 0, 0, 0};
        double nw[4] = {0, 0, 0, 0};
        unsigned nlo = 0;
        if (q0 < n4) raw(q0, na, nb, nw, nlo);
        for (int64_t q = q0; q < n4; q += qs) {
            const v4f a = na, b = nb;
            const double w[4] = {nw[0], nw[1], nw[2], nw[3]};
            const unsigned lo = nlo;
            if (q + qs < n4) raw(q + qs, na, nb, nw, nlo);
            double x[4][D];
            x[0][0] = a.x; x[0][1] = a.y; x[1][0] = a.z; x[1][1] = a.w;
            x[2][0] = b.x; x[2][1] = b.y; x[3][0] = b.z; x[3][1] = b.w;
            process(q, x, w, lo);
        }
    } else {
        for (int64_t q = q0; q < n4; q += qs) {
            double x[4][D], w[4];
            load4<D>(X, q * 4, x);
            load4w<TW>(W, q, w);
            const unsigned lo = MODE == 1 ? __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(labels) + q) : 0u;
            process(q, x, w, lo);
        }
    }
    if (blockIdx.x == 0 && tid < (int)(N - n4 * 4)) {
        const int64_t i = n4 * 4 + tid;
        double x[D];
        load1<D>(X, i, x);
        const double w = (double)W[i];
#pragma unroll
        for (int f = 0; f < D; f++) x[f] -= m[f];
        const int l = assign_point<D, KMAX>(x, c, cn, k);
        if (ACCUM) {
            accumulate(l, x, w);
            if (MODE == 1) changed += (l != labels[i]);
            if (first) {
#pragma unroll
                for (int f = 0; f < D; f++) sq[f] += x[f] * x[f];
            }
        }
        if (MODE == 2) inert += mul_rounded(sq_euclid_grouped_w<D>(x, st->centers + l * D), w);
        if (LABELS) labels[i] = (uint8_t)l;
    }
    if (MODE == 2) {
        __shared__ double lds1[NW];
        double a1[1] = {inert};
        block_reduce_store_w<1, NW>(a1, lds1, partial + blockIdx.x);
    }
    if (ACCUM) {
        double *rec = partial + (size_t)blockIdx.x * NV;
        if (tid < NV) rec[tid] = 0.0;
        unsigned ch = changed;
        for (int off = 32; off >= 1; off >>= 1) ch += __shfl_down(ch, off, 64);
        if (lane == 0) s_changed[wave] = ch;
        __syncthreads();
        // fold the private columns: component i by wave i % NW; a lane adds its NW columns in a fixed order, then a fixed
        // shuffle tree
        for (int i = wave; i < k * D + k; i += NW) {
            const double *col = sacc + (size_t)i * LANES;
            double a = col[lane];
#pragma unroll
            for (int w = 1; w < NW; w++) a += col[lane + 64 * w];
            for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off, 64);
            if (lane == 0) rec[i < k * D ? i : KMAX * D + (i - k * D)] = a;
        }
        if (tid == 0) {
            unsigned t = s_changed[0];
#pragma unroll
            for (int w = 1; w < NW; w++) t += s_changed[w];
            rec[KMAX * D + KMAX] = (double)t;
        }
        if (first) {                                    // uniform
            __shared__ double lds_sq[NW * D];
            block_reduce_store_w<D, NW>(sq, lds_sq, rec + KMAX * D + KMAX + 1);
        }
    }
}

// inertia = sum w_i ||x_i - c_label||^2 (centred), _inertia_dense's grouping and its `sq_dist * sample_weight[i]`
template <int D, class T, class TW>
__global__ __launch_bounds__(256) void k_lloyd_inertia_w(const T *__restrict__ X, const TW *__restrict__ W, int64_t N,
                                                         const LloydState *__restrict__ st,
                                                         const uint8_t *__restrict__ labels,
                                                         double *__restrict__ partial)
{
    __shared__ double lds[4];
    double acc[1] = {0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        double x[D];
        load1<D>(X, i, x);
#pragma unroll
        for (int f = 0; f < D; f++) x[f] -= st->mean[f];
        acc[0] += mul_rounded(sq_euclid_grouped_w<D>(x, st->centers + (int)labels[i] * D), (double)W[i]);
    }
    block_reduce_store<1>(acc, lds, partial + blockIdx.x);
}

// weights from a resident (u,v) field, f32 in and out.  kind 0: |(u,v)| = sqrtf(u*u + v*v); 1: u*u + v*v >= thr*thr ? 1 : 0.
// Every product and sum is rounded on its own (numpy's f32 expression).
__global__ __launch_bounds__(256) void k_flow_weights(const float *__restrict__ F, int64_t n, int kind, float thr2,
                                                      float *__restrict__ W)
{
#pragma clang fp contract(off)
    typedef float v4f __attribute__((ext_vector_type(4)));
    auto one = [&](float u, float v) -> float {
        return kind == 0 ? sqrtf(flow_sq_mag(u, v)) : (flow_is_moving(u, v, thr2) ? 1.0f : 0.0f);
    };
    const int64_t n4 = n / 4;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (int64_t)gridDim.x * 256) {
        const v4f a = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(F + q * 8));
        const v4f b = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(F + q * 8 + 4));
        v4f w;
        w.x = one(a.x, a.y); w.y = one(a.z, a.w); w.z = one(b.x, b.y); w.w = one(b.z, b.w);
        __builtin_nontemporal_store(w, reinterpret_cast<v4f *>(W) + q);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) {
        const int64_t i = n4 * 4 + threadIdx.x;
        W[i] = one(F[2 * i], F[2 * i + 1]);
    }
}

// ------------------------------------------------------------------------------------------------
// host-side dispatch over (dtype, weight dtype, D, KMAX)
// ------------------------------------------------------------------------------------------------
template <int D, int KMAX, class T, class TW>
static void launch_assign_w_t(const void *X, const void *W, int64_t N, int k, const LloydState *st, uint8_t *labels,
                              double *partial, int nblocks, int mode, int first, hipStream_t s)
{
    constexpr int LANES = LloydWLanes<D, KMAX>::value;
    if (mode == 1 || mode == 3) {
        const size_t lds = (size_t)k * (8 * D + 8) * LANES;
        auto kern = mode == 1 ? &k_lloyd_assign_w<D, KMAX, T, TW, 1> : &k_lloyd_assign_w<D, KMAX, T, TW, 3>;
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds);
        hipLaunchKernelGGL(kern, dim3(nblocks), dim3(LANES), lds, s, (const T *)X, (const TW *)W, N, k, st, labels,
                           partial, first);
    } else {
        hipLaunchKernelGGL((k_lloyd_assign_w<D, KMAX, T, TW, 2>), dim3(nblocks), dim3(LANES), 0, s, (const T *)X,
                           (const TW *)W, N, k, st, labels, partial, 0);
    }
}

template <int D, int KMAX, class TW>
static int launch_assign_w_d(const void *X, int dtype, const void *W, int64_t N, int k, const LloydState *st,
                             uint8_t *labels, double *partial, int nblocks, int mode, int first, hipStream_t s)
{
    switch (dtype) {
    case OFC_U8: launch_assign_w_t<D, KMAX, uint8_t, TW>(X, W, N, k, st, labels, partial, nblocks, mode, first, s); break;
    case OFC_F32: launch_assign_w_t<D, KMAX, float, TW>(X, W, N, k, st, labels, partial, nblocks, mode, first, s); break;
    case OFC_F64: launch_assign_w_t<D, KMAX, double, TW>(X, W, N, k, st, labels, partial, nblocks, mode, first, s); break;
    default: set_error("bad dtype %d", dtype); return OFC_EINVAL;
    }
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

template <int D, int KMAX>
static int launch_assign_w_k(const void *X, int dtype, const void *W, int w_dtype, int64_t N, int k,
                             const LloydState *st, uint8_t *labels, double *partial, int nblocks, int mode, int first,
                             hipStream_t s)
{
    if (w_dtype == OFC_F32)
        return launch_assign_w_d<D, KMAX, float>(X, dtype, W, N, k, st, labels, partial, nblocks, mode, first, s);
    return launch_assign_w_d<D, KMAX, double>(X, dtype, W, N, k, st, labels, partial, nblocks, mode, first, s);
}

#define OFC_DW_SWITCH(d, ...)                                    \
    switch (d) {                                                 \
    case 1: { constexpr int DD = 1; __VA_ARGS__; } break;        \
    case 2: { constexpr int DD = 2; __VA_ARGS__; } break;        \
    case 3: { constexpr int DD = 3; __VA_ARGS__; } break;        \
    case 4: { constexpr int DD = 4; __VA_ARGS__; } break;        \
    default: set_error("d=%d unsupported (1..4)", d); return OFC_EUNSUPPORTED; \
    }

int launch_lloyd_assign_w(const void *X, int dtype, const void *W, int w_dtype, int64_t N, int d, int k,
                          const LloydState *st, uint8_t *labels, double *partial, int nblocks, int mode, int first,
                          hipStream_t s)
{
    const int kmax = lloyd_kmax(k);
    if (!kmax) { set_error("k=%d unsupported by the streaming kernel (1..16)", k); return OFC_EUNSUPPORTED; }
    if (w_dtype != OFC_F32 && w_dtype != OFC_F64) { set_error("bad weight dtype %d (f32 or f64)", w_dtype); return OFC_EINVAL; }
    if (mode < 1 || mode > 3) { set_error("weighted sweep: mode %d outside 1..3", mode); return OFC_EINVAL; }
    int rc = OFC_OK;
#define OFC_W_CASE(K) case K: rc = launch_assign_w_k<DD, K>(X, dtype, W, w_dtype, N, k, st, labels, partial, nblocks, mode, first, s); break;
    OFC_DW_SWITCH(d, {
        switch (kmax) {
        OFC_W_CASE(1) OFC_W_CASE(2) OFC_W_CASE(3) OFC_W_CASE(4) OFC_W_CASE(5) OFC_W_CASE(6) OFC_W_CASE(7) OFC_W_CASE(8)
        default: rc = launch_assign_w_k<DD, 16>(X, dtype, W, w_dtype, N, k, st, labels, partial, nblocks, mode, first, s); break;
        }
    })
#undef OFC_W_CASE
    return rc;
}

template <int D, class TW>
static int launch_inertia_w_d(const void *X, int dtype, const void *W, int64_t N, const LloydState *st,
                              const uint8_t *labels, double *partial, int nblocks, hipStream_t s)
{
    switch (dtype) {
    case OFC_U8: hipLaunchKernelGGL((k_lloyd_inertia_w<D, uint8_t, TW>), dim3(nblocks), dim3(256), 0, s, (const uint8_t *)X, (const TW *)W, N, st, labels, partial); break;
    case OFC_F32: hipLaunchKernelGGL((k_lloyd_inertia_w<D, float, TW>), dim3(nblocks), dim3(256), 0, s, (const float *)X, (const TW *)W, N, st, labels, partial); break;
    case OFC_F64: hipLaunchKernelGGL((k_lloyd_inertia_w<D, double, TW>), dim3(nblocks), dim3(256), 0, s, (const double *)X, (const TW *)W, N, st, labels, partial); break;
    default: set_error("bad dtype %d", dtype); return OFC_EINVAL;
    }
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_lloyd_inertia_w(const void *X, int dtype, const void *W, int w_dtype, int64_t N, int d, const LloydState *st,
                           const uint8_t *labels, double *partial, int nblocks, hipStream_t s)
{
    if (w_dtype != OFC_F32 && w_dtype != OFC_F64) { set_error("bad weight dtype %d (f32 or f64)", w_dtype); return OFC_EINVAL; }
    int rc = OFC_OK;
    OFC_DW_SWITCH(d, {
        rc = w_dtype == OFC_F32 ? launch_inertia_w_d<DD, float>(X, dtype, W, N, st, labels, partial, nblocks, s)
                                : launch_inertia_w_d<DD, double>(X, dtype, W, N, st, labels, partial, nblocks, s);
    })
    return rc;
}

int launch_flow_weights(const float *flow, int64_t n, int kind, float thr, float *w, hipStream_t s)
{
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n / 4, 256), 4096));
    const float thr2 = thr * thr;
    hipLaunchKernelGGL(k_flow_weights, dim3(nblocks), dim3(256), 0, s, flow, n, kind, thr2, w);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
