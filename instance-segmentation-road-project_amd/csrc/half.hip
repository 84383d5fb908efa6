// fp16-STORAGE helpers of the "fp16 MFMA path" (BASELINE config 5): the ResNeXt body keeps its activations in IEEE
// half between the convolutions; these are the byte-moving pieces around conv1x1_pipe.hip / gconv_mfma4.hip that have no
// fp32 twin (the max-pool, resize, depthwise conv and global mean on half tensors are pointwise.hip's kernels, instantiated
// for _Float16).  All HBM-bound: 16-byte accesses per lane, one pass.
#include "common.h"

namespace {

constexpr int TPB = 256;

// out[b, oy, ox, :] = in[b, 2 oy, 2 ox, :]: the sampling of a 1x1 stride-2 convolution ('same' and 'valid' agree for
// k = 1), so that the strided shortcut convs (ResNext.py:199-203) run on the stride-1 pipelined kernel
__global__ void subsample2_h_kernel(const _Float16 *__restrict__ in, _Float16 *__restrict__ out, int H, int W, int C8,
                                    int Ho, int Wo, long long total) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= total) return;
    const int c8 = (int)(idx % C8);
    long long pix = idx / C8;
    const int ox = (int)(pix % Wo); pix /= Wo;
    const int oy = (int)(pix % Ho);
    const int b = (int)(pix / Ho);
    const int C = C8 * 8;
    *reinterpret_cast<f16x8 *>(out + ((long long)(b * Ho + oy) * Wo + ox) * C + c8 * 8) =
        *reinterpret_cast<const f16x8 *>(in + ((long long)(b * H + 2 * oy) * W + 2 * ox) * C + c8 * 8);
}

__global__ void cast_h2f_kernel(const _Float16 *__restrict__ in, float *__restrict__ out, long long n8) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n8) return;
    const f16x8 x = *reinterpret_cast<const f16x8 *>(in + i * 8);
    f32x4 lo = {(float)x[0], (float)x[1], (float)x[2], (float)x[3]};
    f32x4 hi = {(float)x[4], (float)x[5], (float)x[6], (float)x[7]};
    *reinterpret_cast<f32x4 *>(out + i * 8) = lo;
    *reinterpret_cast<f32x4 *>(out + i * 8 + 4) = hi;
}

// 8 halves <-> floats (add_h: fp32 arithmetic on the converted values, ONE rounding at the store)
__device__ __forceinline__ void h8_to_f(const f16x8 x, float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
}
__device__ __forceinline__ f16x8 f_to_h8(const float (&v)[8]) {
    const f16x8 x = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3],
                     (_Float16)v[4], (_Float16)v[5], (_Float16)v[6], (_Float16)v[7]};
    return x;
}

__global__ void cast_f2h_kernel(const float *__restrict__ in, _Float16 *__restrict__ out, long long n8) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n8) return;
    const f32x4 lo = *reinterpret_cast<const f32x4 *>(in + i * 8);
    const f32x4 hi = *reinterpret_cast<const f32x4 *>(in + i * 8 + 4);
    const f16x8 x = {(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3],
                     (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2], (_Float16)hi[3]};
    *reinterpret_cast<f16x8 *>(out + i * 8) = x;
}

// x += y (the skip `Add` of MobileSeparableConv2D, engine/layers/misc.py:105): fp32 sum, one rounding.  Thread i < n8 takes
// 8 halves with 16-byte accesses; thread n8 takes the n % 8 tail one by one.
__global__ void add_h_kernel(_Float16 *__restrict__ x, const _Float16 *__restrict__ y, long long n8, int tail) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n8) {
        float a[8], b[8];
        h8_to_f(*reinterpret_cast<const f16x8 *>(x + i * 8), a);
        h8_to_f(*reinterpret_cast<const f16x8 *>(y + i * 8), b);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += b[e];
        *reinterpret_cast<f16x8 *>(x + i * 8) = f_to_h8(a);
    } else if (i == n8) {
        for (int e = 0; e < tail; ++e) x[i * 8 + e] = (_Float16)((float)x[i * 8 + e] + (float)y[i * 8 + e]);
    }
}

unsigned grid_of(long long total) { return (unsigned)((total + TPB - 1) / TPB); }

}  // namespace

extern "C" int ml_cast_f32_to_f16(const float *in, void *out, int64_t n, void *stream) {
    ML_REQUIRE(in && out && n > 0 && n % 8 == 0, "cast_f32_to_f16: n must be a positive multiple of 8");
    ML_REQUIRE(ml_aligned16(in) && ml_aligned16(out), "cast_f32_to_f16: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(cast_f2h_kernel, dim3(grid_of(n / 8)), dim3(TPB), 0, (hipStream_t)stream, in,
                       reinterpret_cast<_Float16 *>(out), (long long)(n / 8));
    ML_CHECK_LAUNCH("cast_f32_to_f16");
    return ML_OK;
}

extern "C" int ml_add_f16(void *x, const void *y, int64_t n, void *stream) {
    ML_REQUIRE(x && y && n > 0, "add_f16: bad arguments");
    ML_REQUIRE(ml_aligned16(x) && ml_aligned16(y), "add_f16: pointers must be 16-byte aligned");
    const long long n8 = n / 8;
    const int tail = (int)(n % 8);
    hipLaunchKernelGGL(add_h_kernel, dim3(grid_of(n8 + (tail ? 1 : 0))), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<_Float16 *>(x), reinterpret_cast<const _Float16 *>(y), n8, tail);
    ML_CHECK_LAUNCH("add_f16");
    return ML_OK;
}

extern "C" int ml_subsample2_f16(const void *in, void *out, int32_t B, int32_t H, int32_t W, int32_t C, void *stream) {
    ML_REQUIRE(in && out && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "subsample2_f16: bad arguments (C %% 8)");
    ML_REQUIRE(ml_aligned16(in) && ml_aligned16(out), "subsample2_f16: pointers must be 16-byte aligned");
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const long long total = (long long)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(subsample2_h_kernel, dim3(grid_of(total)), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const _Float16 *>(in), reinterpret_cast<_Float16 *>(out), H, W, C / 8, Ho, Wo, total);
    ML_CHECK_LAUNCH("subsample2_f16");
    return ML_OK;
}

extern "C" int ml_cast_f16_to_f32(const void *in, float *out, int64_t n, void *stream) {
    ML_REQUIRE(in && out && n > 0 && n % 8 == 0, "cast_f16_to_f32: n must be a positive multiple of 8");
    ML_REQUIRE(ml_aligned16(in) && ml_aligned16(out), "cast_f16_to_f32: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(cast_h2f_kernel, dim3(grid_of(n / 8)), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const _Float16 *>(in), out, (long long)(n / 8));
    ML_CHECK_LAUNCH("cast_f16_to_f32");
    return ML_OK;
}
