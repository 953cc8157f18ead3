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
    const bool hit = valid && (carry + (woff + incl) >= r);
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

}  // namespace ofc
