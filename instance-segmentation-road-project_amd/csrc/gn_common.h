// What the forward (groupnorm.hip) and the backward (groupnorm_grad.hip) of the chunk-wise GroupNormalization share:
// the 16-byte accesses, the slicing of a chunk over blocks, the fp64 (sum, sum of squares) of a slice with its fixed
// reduction order, and mean / 1/sqrt(var + eps) from those sums.  The backward's statistics must have the forward's bits
// (its ReLU mask is decided by the forward's y), so both include the SAME code rather than restating it.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

// one 16-byte access = VW<T> elements, handled as floats
template <class T> struct VW { static constexpr int value = 16 / sizeof(T); };
template <class T>
__device__ __forceinline__ void vload(const T *p, float (&v)[VW<T>::value]) {
    if constexpr (std::is_same<T, float>::value) {
        const f32x4 x = *reinterpret_cast<const f32x4 *>(p);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
    } else {
        const f16x8 x = *reinterpret_cast<const f16x8 *>(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
    }
}
template <class T>
__device__ __forceinline__ void vstore(T *p, const float (&v)[VW<T>::value]) {
    if constexpr (std::is_same<T, float>::value) {
        const f32x4 x = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4 *>(p) = x;
    } else {
        const f16x8 x = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3],
                         (_Float16)v[4], (_Float16)v[5], (_Float16)v[6], (_Float16)v[7]};
        *reinterpret_cast<f16x8 *>(p) = x;
    }
}

constexpr int GN_TPB = 256;
constexpr int GN_MAX_SPLIT = 64;
// Largest chunk the one-pass (register-resident) kernel takes.  Measured on MI355X: one block per chunk wins
// while the chunk is small (8x8 .. 32x32 maps, 14x14 RoI maps: 6.3 vs 9.8 us, 8.0 vs 10.2 us); from 64x64x128
// maps up (chunk 32 768 floats, 128 fat blocks) the sliced two-pass form has the parallelism and is faster
// (19.8 vs 23.7 us), even though it reads x twice.
constexpr int GN_ONEPASS_MAX = 4096;

struct GnPlan { int S; long long slice; };

// slices are multiples of vw*GN_TPB elements (vw = 4 floats / 8 halves per access) so every block runs whole sweeps
static GnPlan gn_plan(long long L, int NG, int vw = 4) {
    long long want = (2048 + NG - 1) / NG;            // aim at >= 2048 blocks on the chip
    if (want < 1) want = 1;
    if (want > GN_MAX_SPLIT) want = GN_MAX_SPLIT;
    const long long unit = (long long)vw * GN_TPB;
    long long slice = ((L + want - 1) / want + unit - 1) / unit * unit;
    int S = (int)((L + slice - 1) / slice);
    return {S, slice};
}

// one 16-byte vector joins a thread's running sums: folded in fp32 first (3 adds, 4 fma per 4 values), then added in
// fp64: the statistics kernel was bound by its fp64 instruction count (12 per float4), not by HBM
template <int W>
__device__ __forceinline__ void gn_stats_add(const float (&v)[W], double &sum, double &sq) {
    float s4 = (v[0] + v[1]) + (v[2] + v[3]);
    float q4 = fmaf(v[3], v[3], fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0])));
    if constexpr (W == 8) {
        s4 += (v[4] + v[5]) + (v[6] + v[7]);
        q4 += fmaf(v[7], v[7], fmaf(v[6], v[6], fmaf(v[5], v[5], v[4] * v[4])));
    }
    sum += (double)s4;
    sq += (double)q4;
}

// the block's (sum, sum of squares) of slice s of chunk ng -> ws: wave reduce (64 lanes), then the 4 waves in order
__device__ __forceinline__ void gn_stats_store(double sum, double sq, double *__restrict__ ws, int S, int ng, int s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        sq += __shfl_down(sq, off, 64);
    }
    __shared__ double red[2][GN_TPB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = sum; red[1][wave] = sq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < GN_TPB / 64; ++w) { a += red[0][w]; b += red[1][w]; }
        ws[((long long)ng * S + s) * 2 + 0] = a;
        ws[((long long)ng * S + s) * 2 + 1] = b;
    }
}

template <class T, bool VEC4 = true>
__device__ __forceinline__ void gn_stats_body(const T *__restrict__ x, double *__restrict__ ws, long long L,
                                              long long slice, int S, int ng, int s) {
    constexpr int W = VW<T>::value;
    const T *p = x + (long long)ng * L;
    const long long lo = (long long)s * slice;
    const long long hi = min(lo + slice, L);
    double sum = 0.0, sq = 0.0;
    if (VEC4) {
        for (long long i = lo + threadIdx.x * W; i < hi; i += GN_TPB * W) {
            float v[W];
            vload<T>(p + i, v);
            gn_stats_add<W>(v, sum, sq);
        }
    } else {
        for (long long i = lo + threadIdx.x; i < hi; i += GN_TPB) { const double d = (double)(float)p[i]; sum += d; sq += d * d; }
    }
    gn_stats_store(sum, sq, ws, S, ng, s);
}

// The chunk's Sp (sum, sum of squares) pairs, added in index order (uniform, L2-resident) -> mean and 1/sqrt(var + eps),
// in fp64 and rounded to float
struct GnMoments { double meand, rstdd; float mean, rstd; };
__device__ __forceinline__ GnMoments gn_moments(const double *__restrict__ ws, int ng, int Sp, long long L, float eps) {
    double sum = 0, sq = 0;
    for (int i = 0; i < Sp; ++i) {
        sum += ws[((long long)ng * Sp + i) * 2 + 0];
        sq += ws[((long long)ng * Sp + i) * 2 + 1];
    }
    const double meand = sum / (double)L;
    double vard = sq / (double)L - meand * meand;
    if (vard < 0) vard = 0;
    const double rstdd = 1.0 / sqrt(vard + (double)eps);
    return {meand, rstdd, (float)meand, (float)rstdd};
}

// y of one element, before the optional ReLU: the forward's apply step, and what the backward's ReLU mask is decided by
// (has_gamma / has_beta: the layer's scale / center; gam, bet: the element's gamma[j], beta[j])
__device__ __forceinline__ float gn_y_val(float v, float mean, float rstd, bool has_gamma, float gam, bool has_beta, float bet) {
    float t = (v - mean) * rstd;
    if (has_gamma) t *= gam;
    if (has_beta) t += bet;
    return t;
}
__device__ __forceinline__ float gn_y(float v, float mean, float rstd, const float *__restrict__ gamma,
                                      const float *__restrict__ beta, int j) {
    return gn_y_val(v, mean, rstd, gamma != nullptr, gamma ? gamma[j] : 0.f, beta != nullptr, beta ? beta[j] : 0.f);
}

template <int TPB>
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                       // `red` may still be read from the previous reduction
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) t += red[w];
    return t;
}

}  // namespace
