// lloyd_device.h -- device helpers shared by the Lloyd and seeding kernels (lloyd_kernels.hip, lloyd_weighted.hip,
// lloyd_seed.hip) and grid_labels.hip: sample loaders, the E-step's label and the deterministic work-group sum.
#pragma once
#include "lloyd_common.h"

namespace ofc {

// ------------------------------------------------------------------------------------------------
// loaders: 4 consecutive points per lane as doubles
// ------------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void load4(const uint8_t *X, int64_t i, double (&x)[4][D])
{
    if constexpr (D == 4) {
        const uint4 v = *reinterpret_cast<const uint4 *>(X + i * 4);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int f = 0; f < 4; f++) x[p][f] = (double)((w[p] >> (8 * f)) & 0xffu);
    } else {
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int f = 0; f < D; f++) x[p][f] = (double)X[(i + p) * D + f];
    }
}
template <int D>
__device__ __forceinline__ void load4(const float *X, int64_t i, double (&x)[4][D])
{
    if constexpr (D == 2) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        // streamed once per iteration and far larger than any cache: non-temporal
        const v4f a = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(X + i * 2));
        const v4f b = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(X + i * 2 + 4));
        x[0][0] = a.x; x[0][1] = a.y; x[1][0] = a.z; x[1][1] = a.w;
        x[2][0] = b.x; x[2][1] = b.y; x[3][0] = b.z; x[3][1] = b.w;
    } else if constexpr (D == 4) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const float4 a = *reinterpret_cast<const float4 *>(X + (i + p) * 4);
            x[p][0] = a.x; x[p][1] = a.y; x[p][2] = a.z; x[p][3] = a.w;
        }
    } else {
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int f = 0; f < D; f++) x[p][f] = (double)X[(i + p) * D + f];
    }
}
template <int D>
__device__ __forceinline__ void load4(const double *X, int64_t i, double (&x)[4][D])
{
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int f = 0; f < D; f++) x[p][f] = X[(i + p) * D + f];
}
template <int D, class T>
__device__ __forceinline__ void load1(const T *X, int64_t i, double (&x)[D])
{
#pragma unroll
    for (int f = 0; f < D; f++) x[f] = (double)X[i * D + f];
}

// the E-step's label of one centred sample: the first strict minimum over j < k of D_j = |c_j|^2 - 2 x.c_j, the dot
// product as one multiply and a chain of fma.  Every kernel that labels (the Lloyd sweeps, plain and weighted, and
// grid_labels.hip's fused label-and-count) calls this one function, so they give a sample the same byte.
template <int D, int KMAX>
__device__ __forceinline__ int assign_point(const double (&x)[D], const double *c /*[KMAX*D] regs*/,
                                            const double *cn, int k)
{
    double best = 0;
    int label = 0;
#pragma unroll
    for (int j = 0; j < KMAX; j++) {
        if (j < k) {
            double acc = x[0] * c[j * D];
#pragma unroll
            for (int f = 1; f < D; f++) acc = fma(x[f], c[j * D + f], acc);
            const double dj = cn[j] - 2.0 * acc;
            if (j == 0 || dj < best) { best = dj; label = j; }
        }
    }
    return label;
}

// u*u + v*v with every product and the sum rounded to f32 on its own (numpy's f32 expression).  k_flow_weights takes its
// square root (kind 0) or compares it with thr*thr (kind 1, "moving"); blobs.hip's key kernel makes the same comparison.
__device__ __forceinline__ float flow_sq_mag(float u, float v)
{
#pragma clang fp contract(off)
    const float uu = u * u, vv = v * v;
    const float s = uu + vv;
    return s;
}
// the "moving" predicate of ofc_flow_weights_dev kind 1: a NaN fails it
__device__ __forceinline__ bool flow_is_moving(float u, float v, float thr2) { return flow_sq_mag(u, v) >= thr2; }

// deterministic work-group sum of NV doubles per thread -> out[NV] (thread 0..NV-1 write)
template <int NV>
__device__ __forceinline__ void block_reduce_store(double (&v)[NV], double *lds /*[4][NV]*/, double *out)
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
        out[i] = ((lds[i] + lds[NV + i]) + lds[2 * NV + i]) + lds[3 * NV + i];
    }
    __syncthreads();
}

}  // namespace ofc
