// lloyd_seed.hip -- k-means++ seeding (sklearn's _kmeans_plusplus, _kmeans.py:174-272) on device-resident samples.
//
// closest[N] (f64, the running squared distance to the nearest chosen centre) stays on the device.  One step is ONE
// sweep over the samples (k_kpp_sweep): it folds the previous step's winning candidate into closest[], evaluates the
// step's candidates against it and leaves, per candidate, the potential and one partial sum per OFC_KPP_CHUNK samples.
// The winner's chunk sums are the first level of the cumulative sum the NEXT step samples from (k_kpp_sample): a sum
// per 1024 chunk sums is the second level (k_kpp_sum1024), one work-group scans those, then the chunk sums of the one
// group it lands in, then the samples of the one chunk it lands in.  No [n_trials][N] array, no O(N) host traffic.
//
// Arithmetic = k_kpp_candidates': centred sample, max(0, (|c|^2 - 2 c.x) + |x|^2), contraction off, minimum with
// closest.  Every sum is formed in a fixed order (lane partials -> shuffle tree -> LDS in wave order); no atomics.
#include "lloyd_device.h"

#pragma clang fp contract(off)

namespace ofc {

static_assert(OFC_KPP_CHUNK == 1024, "k_kpp_sweep walks a chunk as 4 x (64 lanes x 4 samples)");
constexpr int KPP_MAXC = 8;

struct KppSeedArgs {
    double mean[LLOYD_DMAX];
    double prev[LLOYD_DMAX];               // centred row of the previous step's winner (prev_mode != KPP_PREV_NONE)
    double cand[KPP_MAXC][LLOYD_DMAX];     // centred candidate rows
    int n_cand;                            // 0: the only "candidate" is closest[] itself (slot 0)
    int prev_mode;
};

template <int D>
__device__ __forceinline__ double kpp_norm2(const double *c)
{
    double t = 0;
#pragma unroll
    for (int f = 0; f < D; f++) t += c[f] * c[f];
    return t;
}

// x is centred in place; -> |x|^2
template <int D>
__device__ __forceinline__ double kpp_centre(double (&x)[D], const double *mean)
{
    double xx = 0;
#pragma unroll
    for (int f = 0; f < D; f++) {
        x[f] -= mean[f];
        xx += x[f] * x[f];
    }
    return xx;
}

template <int D>
__device__ __forceinline__ double kpp_dist(const double (&x)[D], double xx, const double *c, double cc)
{
    double dot = 0;
#pragma unroll
    for (int f = 0; f < D; f++) dot += c[f] * x[f];
    const double dd = (-2.0 * dot + cc) + xx;
    return dd > 0.0 ? dd : 0.0;
}

// closest[i] as the step sees it: the stored value with the pending winner folded in
template <int D>
__device__ __forceinline__ double kpp_closest(const double (&x)[D], double xx, const KppSeedArgs &a, double pc,
                                              const double *closest, int64_t i)
{
    if (a.prev_mode == KPP_PREV_FIRST) return kpp_dist<D>(x, xx, a.prev, pc);
    const double cl = closest[i];
    if (a.prev_mode == KPP_PREV_NONE) return cl;
    const double dd = kpp_dist<D>(x, xx, a.prev, pc);
    return dd < cl ? dd : cl;
}

// One wave per chunk of OFC_KPP_CHUNK samples: cs[c][chunk] = sum over the chunk of min(closest, d(x, cand c)),
// partial[block][c] = the work-group's share of candidate c's potential (its chunk sums, in chunk order).
template <int D, class T>
__global__ __launch_bounds__(256) void k_kpp_sweep(const T *__restrict__ X, int64_t N, KppSeedArgs a,
                                                   double *__restrict__ closest, double *__restrict__ cs,
                                                   int64_t nchunks, double *__restrict__ partial)
{
    __shared__ double lds[4 * KPP_MAXC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = a.n_cand > 0 ? a.n_cand : 1;
    const double pc = kpp_norm2<D>(a.prev);
    double cc[KPP_MAXC], tot[KPP_MAXC];
#pragma unroll
    for (int c = 0; c < KPP_MAXC; c++) {
        cc[c] = kpp_norm2<D>(a.cand[c]);
        tot[c] = 0;
    }
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < nchunks; g += (int64_t)gridDim.x * 4) {
        double acc[KPP_MAXC];
#pragma unroll
        for (int c = 0; c < KPP_MAXC; c++) acc[c] = 0;
        for (int it = 0; it < OFC_KPP_CHUNK / 256; it++) {
            const int64_t i0 = g * OFC_KPP_CHUNK + it * 256 + lane * 4;
            if (i0 >= N) break;
            double x[4][D];
            const int np = i0 + 4 <= N ? 4 : (int)(N - i0);
            if (np == 4) {
                load4<D>(X, i0, x);
            } else {
                for (int p = 0; p < np; p++) load1<D>(X, i0 + p, x[p]);
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if (p < np) {
                    const double xx = kpp_centre<D>(x[p], a.mean);
                    const double cl = kpp_closest<D>(x[p], xx, a, pc, closest, i0 + p);
                    if (a.prev_mode != KPP_PREV_NONE) closest[i0 + p] = cl;
                    if (a.n_cand == 0) acc[0] += cl;
#pragma unroll
                    for (int c = 0; c < KPP_MAXC; c++) {
                        if (c < a.n_cand) {
                            const double dd = kpp_dist<D>(x[p], xx, a.cand[c], cc[c]);
                            acc[c] += dd < cl ? dd : cl;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < KPP_MAXC; c++) {
            if (c < nv) {
                double s = acc[c];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
                if (lane == 0) cs[(size_t)c * nchunks + g] = s;
                tot[c] += s;        // lane 0's is the sum of this wave's chunk sums
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < KPP_MAXC; c++) lds[wave * KPP_MAXC + c] = tot[c];
    }
    __syncthreads();
    if (threadIdx.x < KPP_MAXC) {
        const int c = threadIdx.x;
        partial[(size_t)blockIdx.x * KPP_MAXC + c] =
            ((lds[c] + lds[KPP_MAXC + c]) + lds[2 * KPP_MAXC + c]) + lds[3 * KPP_MAXC + c];
    }
}

// out[b] = sum of in[b * 1024 .. min(n, (b + 1) * 1024)): the next level of the cumulative sum
__global__ __launch_bounds__(256) void k_kpp_sum1024(const double *__restrict__ in, int64_t n, double *__restrict__ out)
{
    __shared__ double lds[4];
    const int64_t i0 = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4;
    double v[1] = {0};
    for (int p = 0; p < 4; p++)
        if (i0 + p < n) v[0] += in[i0 + p];
    block_reduce_store<1>(v, lds, out + blockIdx.x);
}

// Work-group of 1024 threads, thread t holds v (0 where !valid): the smallest t with carry + sum(v[0..t]) >= r, or -1.
// carry is advanced to the sum in front of that t (to the sum over all of them when there is none).
// STRICT: > r in place of >= r (searchsorted's side='right').
template <bool STRICT = false>
__device__ __forceinline__ int kpp_block_search(double v, bool valid, double r, double &carry, double *s_w /*[17]*/,
                                                int *s_hit /*[16]*/)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0;
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    double woff = 0, all = 0;
    for (int w = 0; w < 16; w++) {
        if (w == wave) woff = all;
        all += s_w[w];
    }
    const double cum = carry + (woff + incl);
    const bool hit = valid && (STRICT ? cum > r : cum >= r);
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_hit[wave] = m ? __ffsll((long long)m) - 1 : -1;
    __syncthreads();
    int found = -1;
    for (int w = 0; w < 16 && found < 0; w++)
        if (s_hit[w] >= 0) found = w * 64 + s_hit[w];
    if (found == (int)threadIdx.x) s_w[16] = carry + (woff + excl);
    __syncthreads();
    carry = found >= 0 ? s_w[16] : carry + all;
    __syncthreads();
    return found;
}

struct KppSampleArgs {
    double r[KPP_MAXC];
    double base;        // potential of the shards in front of this one
};

// Work-group j: idx[j] = min(smallest i with base + cumsum(closest)[i] >= r[j], N - 1), rows[j] = X[idx[j]] as doubles
// (X != nullptr).  closest as k_kpp_sweep sees it (a.prev_mode folds the pending winner in); cs = its sums per chunk,
// ss = their sums per 1024 chunks, nsuper <= 1024.
template <int D, class T>
__global__ __launch_bounds__(1024) void k_kpp_sample(const T *__restrict__ X, int64_t N, KppSeedArgs a,
                                                     const double *__restrict__ closest, const double *__restrict__ cs,
                                                     int64_t nchunks, const double *__restrict__ ss, int nsuper,
                                                     KppSampleArgs in, int64_t *__restrict__ idx, double *__restrict__ rows)
{
    __shared__ double s_w[17];
    __shared__ int s_hit[16];
    const int t = threadIdx.x, j = blockIdx.x;
    const double r = in.r[j];
    double carry = in.base;
    int64_t res = N - 1;
    const int S = kpp_block_search(t < nsuper ? ss[t] : 0.0, t < nsuper, r, carry, s_w, s_hit);
    if (S >= 0) {
        const int64_t g0 = (int64_t)S * 1024;
        const int64_t ng = nchunks - g0 < 1024 ? nchunks - g0 : 1024;
        const int G = kpp_block_search(t < ng ? cs[g0 + t] : 0.0, t < ng, r, carry, s_w, s_hit);
        res = (g0 + ng) * OFC_KPP_CHUNK - 1;      // rounding left the group without a hit: its last sample
        if (G >= 0) {
            const int64_t i0 = (g0 + G) * OFC_KPP_CHUNK;
            const int64_t ni = N - i0 < OFC_KPP_CHUNK ? N - i0 : OFC_KPP_CHUNK;
            double v = 0;
            if (t < ni) {
                if (a.prev_mode == KPP_PREV_NONE) {
                    v = closest[i0 + t];
                } else {
                    double x[D];
                    load1<D>(X, i0 + t, x);
                    const double xx = kpp_centre<D>(x, a.mean);
                    v = kpp_closest<D>(x, xx, a, kpp_norm2<D>(a.prev), closest, i0 + t);
                }
            }
            const int I = kpp_block_search(v, t < ni, r, carry, s_w, s_hit);
            res = I >= 0 ? i0 + I : i0 + ni - 1;
        }
        if (res > N - 1) res = N - 1;
    }
    if (t == 0) idx[j] = res;
    if (X && rows && t < D) rows[j * LLOYD_DMAX + t] = (double)X[res * D + t];
}

template <int D, class T>
static void launch_seed_t(const T *X, int64_t N, const KppSeedArgs &a, double *closest, double *cs, int64_t nchunks,
                          double *partial, int nblocks, hipStream_t s)
{
    hipLaunchKernelGGL((k_kpp_sweep<D, T>), dim3(nblocks), dim3(256), 0, s, X, N, a, closest, cs, nchunks, partial);
}

template <int D, class T>
static void launch_sample_t(const T *X, int64_t N, const KppSeedArgs &a, const double *closest, const double *cs,
                            int64_t nchunks, const double *ss, int nsuper, const KppSampleArgs &in, int n, int64_t *idx,
                            double *rows, hipStream_t s)
{
    hipLaunchKernelGGL((k_kpp_sample<D, T>), dim3(n), dim3(1024), 0, s, X, N, a, closest, cs, nchunks, ss, nsuper, in,
                       idx, rows);
}

#define KPP_DISPATCH(d, dtype, CALL)                                                          \
    switch ((d) * 4 + (dtype)) {                                                              \
    case 1 * 4 + OFC_U8: { constexpr int DD = 1; typedef uint8_t TT; CALL; } break;           \
    case 1 * 4 + OFC_F32: { constexpr int DD = 1; typedef float TT; CALL; } break;            \
    case 1 * 4 + OFC_F64: { constexpr int DD = 1; typedef double TT; CALL; } break;           \
    case 2 * 4 + OFC_U8: { constexpr int DD = 2; typedef uint8_t TT; CALL; } break;           \
    case 2 * 4 + OFC_F32: { constexpr int DD = 2; typedef float TT; CALL; } break;            \
    case 2 * 4 + OFC_F64: { constexpr int DD = 2; typedef double TT; CALL; } break;           \
    case 3 * 4 + OFC_U8: { constexpr int DD = 3; typedef uint8_t TT; CALL; } break;           \
    case 3 * 4 + OFC_F32: { constexpr int DD = 3; typedef float TT; CALL; } break;            \
    case 3 * 4 + OFC_F64: { constexpr int DD = 3; typedef double TT; CALL; } break;           \
    case 4 * 4 + OFC_U8: { constexpr int DD = 4; typedef uint8_t TT; CALL; } break;           \
    case 4 * 4 + OFC_F32: { constexpr int DD = 4; typedef float TT; CALL; } break;            \
    case 4 * 4 + OFC_F64: { constexpr int DD = 4; typedef double TT; CALL; } break;           \
    default: set_error("d=%d, dtype=%d unsupported (d 1..4)", d, dtype); return OFC_EUNSUPPORTED; \
    }

static void fill_args(KppSeedArgs &a, int d, const double *mean, const double *prev, int prev_mode,
                      const double *cand_centred, int n_cand)
{
    memset(&a, 0, sizeof(a));
    a.n_cand = n_cand;
    a.prev_mode = prev_mode;
    for (int f = 0; f < d; f++) {
        a.mean[f] = mean ? mean[f] : 0.0;
        a.prev[f] = prev ? prev[f] : 0.0;
    }
    for (int c = 0; c < n_cand; c++)
        for (int f = 0; f < d; f++) a.cand[c][f] = cand_centred[c * d + f];
}

int launch_kpp_sweep(const void *X, int dtype, int64_t N, int d, const double *mean, const double *prev, int prev_mode,
                     const double *cand_centred, int n_cand, double *closest, double *cs, double *partial, int nblocks,
                     hipStream_t s)
{
    if (n_cand < 0 || n_cand > KPP_MAXC) { set_error("n_cand %d outside 0..%d", n_cand, KPP_MAXC); return OFC_EUNSUPPORTED; }
    KppSeedArgs a;
    fill_args(a, d, mean, prev, prev_mode, cand_centred, n_cand);
    const int64_t nchunks = kpp_chunks(N);
    KPP_DISPATCH(d, dtype, (launch_seed_t<DD, TT>((const TT *)X, N, a, closest, cs, nchunks, partial, nblocks, s)))
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_kpp_sum1024(const double *in, int64_t n, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_kpp_sum1024, dim3((unsigned)cdiv64(n, 1024)), dim3(256), 0, s, in, n, out);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_kpp_sample(const void *X, int dtype, int64_t N, int d, const double *mean, const double *prev, int prev_mode,
                      const double *closest, const double *cs, const double *ss, const double *r, int n, double base,
                      int64_t *idx, double *rows, hipStream_t s)
{
    if (n < 1 || n > KPP_MAXC) { set_error("n %d outside 1..%d", n, KPP_MAXC); return OFC_EUNSUPPORTED; }
    KppSeedArgs a;
    fill_args(a, d, mean, prev, prev_mode, nullptr, 0);
    KppSampleArgs in;
    memset(&in, 0, sizeof(in));
    for (int j = 0; j < n; j++) in.r[j] = r[j];
    in.base = base;
    const int64_t nchunks = kpp_chunks(N);
    const int nsuper = (int)cdiv64(nchunks, 1024);
    if (!X) {       // plain weights (ofc_kpp_sample_dev)
        launch_sample_t<1, double>(nullptr, N, a, closest, cs, nchunks, ss, nsuper, in, n, idx, nullptr, s);
    } else {
        KPP_DISPATCH(d, dtype, (launch_sample_t<DD, TT>((const TT *)X, N, a, closest, cs, nchunks, ss, nsuper, in, n, idx, rows, s)))
    }
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

// ------------------------------------------------------------------------------------------------
// seeding with sample weights (sklearn's _kmeans_plusplus with sample_weight): closest[] stays unweighted; what is
// summed, per chunk and per candidate, is w[i] * min(closest[i], d(x_i, cand)), the product rounded on its own.
// ------------------------------------------------------------------------------------------------

// the four weights of a lane's samples i0 .. i0+3 (i0 a multiple of 4: one aligned 16-byte load for f32, two for f64)
template <class WT>
__device__ __forceinline__ void kpp_load4w(const WT *W, int64_t i0, double (&w)[4])
{
    if constexpr (sizeof(WT) == 4) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f a = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(W + i0));
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    } else {
        typedef double v2d __attribute__((ext_vector_type(2)));
        const v2d a = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(W + i0));
        const v2d b = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(W + i0 + 2));
        w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y;
    }
}

template <class WT>
__device__ __forceinline__ int kpp_loadw(const WT *W, int64_t i0, int64_t N, double (&w)[4])
{
    const int np = i0 + 4 <= N ? 4 : (int)(N - i0);
    if (np == 4) {
        kpp_load4w<WT>(W, i0, w);
    } else {
#pragma unroll
        for (int p = 0; p < 4; p++) w[p] = p < np ? (double)W[i0 + p] : 0.0;
    }
    return np;
}

// k_kpp_sweep with a weight stream: same chunk walk, same order of every sum; cs and partial hold weighted sums
template <int D, class T, class WT>
__global__ __launch_bounds__(256) void k_kpp_sweep_w(const T *__restrict__ X, const WT *__restrict__ W, int64_t N,
                                                     KppSeedArgs a, double *__restrict__ closest, double *__restrict__ cs,
                                                     int64_t nchunks, double *__restrict__ partial)
{
    __shared__ double lds[4 * KPP_MAXC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = a.n_cand > 0 ? a.n_cand : 1;
    const double pc = kpp_norm2<D>(a.prev);
    double cc[KPP_MAXC], tot[KPP_MAXC];
#pragma unroll
    for (int c = 0; c < KPP_MAXC; c++) {
        cc[c] = kpp_norm2<D>(a.cand[c]);
        tot[c] = 0;
    }
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < nchunks; g += (int64_t)gridDim.x * 4) {
        double acc[KPP_MAXC];
#pragma unroll
        for (int c = 0; c < KPP_MAXC; c++) acc[c] = 0;
        for (int it = 0; it < OFC_KPP_CHUNK / 256; it++) {
            const int64_t i0 = g * OFC_KPP_CHUNK + it * 256 + lane * 4;
            if (i0 >= N) break;
            double x[4][D], w[4];
            const int np = kpp_loadw<WT>(W, i0, N, w);
            if (np == 4) {
                load4<D>(X, i0, x);
            } else {
                for (int p = 0; p < np; p++) load1<D>(X, i0 + p, x[p]);
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if (p < np) {
                    const double xx = kpp_centre<D>(x[p], a.mean);
                    const double cl = kpp_closest<D>(x[p], xx, a, pc, closest, i0 + p);
                    if (a.prev_mode != KPP_PREV_NONE) closest[i0 + p] = cl;
                    if (a.n_cand == 0) acc[0] += w[p] * cl;
#pragma unroll
                    for (int c = 0; c < KPP_MAXC; c++) {
                        if (c < a.n_cand) {
                            const double dd = kpp_dist<D>(x[p], xx, a.cand[c], cc[c]);
                            acc[c] += w[p] * (dd < cl ? dd : cl);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < KPP_MAXC; c++) {
            if (c < nv) {
                double s = acc[c];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
                if (lane == 0) cs[(size_t)c * nchunks + g] = s;
                tot[c] += s;        // lane 0's is the sum of this wave's chunk sums
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < KPP_MAXC; c++) lds[wave * KPP_MAXC + c] = tot[c];
    }
    __syncthreads();
    if (threadIdx.x < KPP_MAXC) {
        const int c = threadIdx.x;
        partial[(size_t)blockIdx.x * KPP_MAXC + c] =
            ((lds[c] + lds[KPP_MAXC + c]) + lds[2 * KPP_MAXC + c]) + lds[3 * KPP_MAXC + c];
    }
}

// cs[chunk] = sum over the chunk of (double)w[i] * v[i] (v == nullptr: of (double)w[i]); one wave per chunk, the sweep's walk
template <class WT>
__global__ __launch_bounds__(256) void k_kpp_wchunks(const WT *__restrict__ W, const double *__restrict__ v, int64_t N,
                                                     double *__restrict__ cs, int64_t nchunks)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < nchunks; g += (int64_t)gridDim.x * 4) {
        double acc = 0;
        for (int it = 0; it < OFC_KPP_CHUNK / 256; it++) {
            const int64_t i0 = g * OFC_KPP_CHUNK + it * 256 + lane * 4;
            if (i0 >= N) break;
            double w[4];
            const int np = kpp_loadw<WT>(W, i0, N, w);
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (p < np) acc += v ? w[p] * v[i0 + p] : w[p];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) cs[g] = acc;
    }
}

// total[0] = the sum of ss[0..nsuper) in the order kpp_block_search forms its last cumulative value
__global__ __launch_bounds__(1024) void k_kpp_total(const double *__restrict__ ss, int nsuper, double *__restrict__ total)
{
    __shared__ double s_w[17];
    __shared__ int s_hit[16];
    const int t = threadIdx.x;
    double carry = 0;
    kpp_block_search(t < nsuper ? ss[t] : 0.0, false, 0.0, carry, s_w, s_hit);
    if (t == 0) total[0] = carry;
}

// work-group of 1024 threads: the largest t whose `valid` is set, or -1
__device__ __forceinline__ int kpp_block_last(bool valid, int *s_hit /*[16]*/)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(valid);
    if (lane == 0) s_hit[wave] = m ? 63 - __clzll((long long)m) : -1;
    __syncthreads();
    int found = -1;
    for (int w = 15; w >= 0 && found < 0; w--)
        if (s_hit[w] >= 0) found = w * 64 + s_hit[w];
    __syncthreads();
    return found;
}

// one level of k_kpp_sample_w's descent.  Once a level is left without a hit (*open is cleared) every level below
// takes its last eligible entry.
template <int SIDE>
__device__ __forceinline__ int kpp_level(double v, bool in_range, double r, double &carry, bool &open, double *s_w,
                                         int *s_hit)
{
    const bool valid = in_range && (SIDE != KPP_SIDE_FIRST || v > 0.0);
    int hit = -1;
    if (open) hit = kpp_block_search<SIDE != KPP_SIDE_LEFT>(v, valid, r, carry, s_w, s_hit);
    if (hit < 0) {
        open = false;
        hit = kpp_block_last(valid, s_hit);
    }
    return hit;
}

// k_kpp_sample over the values w[i] * closest[i] (closest as k_kpp_sweep_w sees it; ones: over w[i] alone), with
// cs / ss the chunk sums of those values.  X == nullptr: closest is a plain vector (or nullptr with ones), no rows.
template <int D, class T, class WT, int SIDE>
__global__ __launch_bounds__(1024) void k_kpp_sample_w(const T *__restrict__ X, const WT *__restrict__ W, int64_t N,
                                                       KppSeedArgs a, const double *__restrict__ closest, bool ones,
                                                       const double *__restrict__ cs, int64_t nchunks,
                                                       const double *__restrict__ ss, int nsuper, KppSampleArgs in,
                                                       int64_t *__restrict__ idx, double *__restrict__ rows)
{
    __shared__ double s_w[17];
    __shared__ int s_hit[16];
    const int t = threadIdx.x, j = blockIdx.x;
    const double r = in.r[j];
    double carry = in.base;
    bool open = true;
    int64_t res = N - 1;
    const int S = kpp_level<SIDE>(t < nsuper ? ss[t] : 0.0, t < nsuper, r, carry, open, s_w, s_hit);
    if (S >= 0) {
        const int64_t g0 = (int64_t)S * 1024;
        const int64_t ng = nchunks - g0 < 1024 ? nchunks - g0 : 1024;
        const int G = kpp_level<SIDE>(t < ng ? cs[g0 + t] : 0.0, t < ng, r, carry, open, s_w, s_hit);
        if (G >= 0) {
            const int64_t i0 = (g0 + G) * OFC_KPP_CHUNK;
            const int64_t ni = N - i0 < OFC_KPP_CHUNK ? N - i0 : OFC_KPP_CHUNK;
            double v = 0;
            if (t < ni) {
                double cl = 1.0;
                if (!ones) {
                    if (!X || a.prev_mode == KPP_PREV_NONE) {
                        cl = closest[i0 + t];
                    } else {
                        double x[D];
                        load1<D>(X, i0 + t, x);
                        const double xx = kpp_centre<D>(x, a.mean);
                        cl = kpp_closest<D>(x, xx, a, kpp_norm2<D>(a.prev), closest, i0 + t);
                    }
                }
                v = (double)W[i0 + t] * cl;
            }
            const int I = kpp_level<SIDE>(v, t < ni, r, carry, open, s_w, s_hit);
            if (I >= 0) res = i0 + I;
        }
    }
    if (t == 0) idx[j] = res;
    if (X && rows && t < D) rows[j * LLOYD_DMAX + t] = (double)X[res * D + t];
}

template <int D, class T, class WT>
static void launch_seed_w_t(const T *X, const WT *W, int64_t N, const KppSeedArgs &a, double *closest, double *cs,
                            int64_t nchunks, double *partial, int nblocks, hipStream_t s)
{
    hipLaunchKernelGGL((k_kpp_sweep_w<D, T, WT>), dim3(nblocks), dim3(256), 0, s, X, W, N, a, closest, cs, nchunks, partial);
}

template <int D, class T, class WT>
static void launch_sample_w_t(const T *X, const WT *W, int64_t N, const KppSeedArgs &a, const double *closest, bool ones,
                              const double *cs, int64_t nchunks, const double *ss, int nsuper, const KppSampleArgs &in,
                              int n, int side, int64_t *idx, double *rows, hipStream_t s)
{
#define KPP_SIDE_CASE(SIDE)                                                                                             \
    hipLaunchKernelGGL((k_kpp_sample_w<D, T, WT, SIDE>), dim3(n), dim3(1024), 0, s, X, W, N, a, closest, ones, cs, nchunks, \
                       ss, nsuper, in, idx, rows)
    if (side == KPP_SIDE_LEFT) KPP_SIDE_CASE(KPP_SIDE_LEFT);
    else if (side == KPP_SIDE_RIGHT) KPP_SIDE_CASE(KPP_SIDE_RIGHT);
    else KPP_SIDE_CASE(KPP_SIDE_FIRST);
#undef KPP_SIDE_CASE
}

int launch_kpp_sweep_w(const void *X, int dtype, const void *W, int w_dtype, int64_t N, int d, const double *mean,
                       const double *prev, int prev_mode, const double *cand_centred, int n_cand, double *closest,
                       double *cs, double *partial, int nblocks, hipStream_t s)
{
    if (n_cand < 0 || n_cand > KPP_MAXC) { set_error("n_cand %d outside 0..%d", n_cand, KPP_MAXC); return OFC_EUNSUPPORTED; }
    if (w_dtype != OFC_F32 && w_dtype != OFC_F64) { set_error("bad weight dtype %d (f32 or f64)", w_dtype); return OFC_EINVAL; }
    KppSeedArgs a;
    fill_args(a, d, mean, prev, prev_mode, cand_centred, n_cand);
    const int64_t nchunks = kpp_chunks(N);
    if (w_dtype == OFC_F32) {
        KPP_DISPATCH(d, dtype, (launch_seed_w_t<DD, TT, float>((const TT *)X, (const float *)W, N, a, closest, cs, nchunks, partial, nblocks, s)))
    } else {
        KPP_DISPATCH(d, dtype, (launch_seed_w_t<DD, TT, double>((const TT *)X, (const double *)W, N, a, closest, cs, nchunks, partial, nblocks, s)))
    }
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_kpp_wchunks(const void *W, int w_dtype, const double *v, int64_t N, double *cs, hipStream_t s)
{
    if (w_dtype != OFC_F32 && w_dtype != OFC_F64) { set_error("bad weight dtype %d (f32 or f64)", w_dtype); return OFC_EINVAL; }
    const int64_t nchunks = kpp_chunks(N);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(nchunks, 4), 2048)));
    if (w_dtype == OFC_F32)
        hipLaunchKernelGGL(k_kpp_wchunks<float>, grid, dim3(256), 0, s, (const float *)W, v, N, cs, nchunks);
    else
        hipLaunchKernelGGL(k_kpp_wchunks<double>, grid, dim3(256), 0, s, (const double *)W, v, N, cs, nchunks);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_kpp_total(const double *ss, int nsuper, double *total, hipStream_t s)
{
    hipLaunchKernelGGL(k_kpp_total, dim3(1), dim3(1024), 0, s, ss, nsuper, total);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_kpp_sample_w(const void *X, int dtype, const void *W, int w_dtype, int64_t N, int d, const double *mean,
                        const double *prev, int prev_mode, const double *closest, const double *cs, const double *ss,
                        const double *r, int n, double base, int side, int64_t *idx, double *rows, hipStream_t s)
{
    if (n < 1 || n > KPP_MAXC) { set_error("n %d outside 1..%d", n, KPP_MAXC); return OFC_EUNSUPPORTED; }
    if (w_dtype != OFC_F32 && w_dtype != OFC_F64) { set_error("bad weight dtype %d (f32 or f64)", w_dtype); return OFC_EINVAL; }
    if (side < KPP_SIDE_LEFT || side > KPP_SIDE_FIRST) { set_error("bad side %d", side); return OFC_EINVAL; }
    KppSeedArgs a;
    fill_args(a, d, mean, prev, prev_mode, nullptr, 0);
    KppSampleArgs in;
    memset(&in, 0, sizeof(in));
    for (int j = 0; j < n; j++) in.r[j] = r[j];
    in.base = base;
    const int64_t nchunks = kpp_chunks(N);
    const int nsuper = (int)cdiv64(nchunks, 1024);
    const bool ones = closest == nullptr;
    if (!X) {       // plain values (ofc_kpp_sample_dev_w)
        if (w_dtype == OFC_F32)
            launch_sample_w_t<1, double, float>(nullptr, (const float *)W, N, a, closest, ones, cs, nchunks, ss, nsuper, in, n, side, idx, nullptr, s);
        else
            launch_sample_w_t<1, double, double>(nullptr, (const double *)W, N, a, closest, ones, cs, nchunks, ss, nsuper, in, n, side, idx, nullptr, s);
    } else if (w_dtype == OFC_F32) {
        KPP_DISPATCH(d, dtype, (launch_sample_w_t<DD, TT, float>((const TT *)X, (const float *)W, N, a, closest, ones, cs, nchunks, ss, nsuper, in, n, side, idx, rows, s)))
    } else {
        KPP_DISPATCH(d, dtype, (launch_sample_w_t<DD, TT, double>((const TT *)X, (const double *)W, N, a, closest, ones, cs, nchunks, ss, nsuper, in, n, side, idx, rows, s)))
    }
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc
