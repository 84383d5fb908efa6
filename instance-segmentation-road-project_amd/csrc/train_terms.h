// What the trainer's forward (train_targets.hip) and the losses' backward (train_grads.hip) share: the launch constants, the
// fixed-order block sum, the per-element terms of the focal loss and the binary cross entropy, the argument structs, and the
// passes a fused "loss + gradient" call runs unchanged -- BoxLoss's statistics, the per-RoI mask loss and the finishing
// kernels.  A `*_grad` call must return the forward call's loss bit for bit, so both take every one of these from here.
// Everything is internal to the including file (anonymous namespace); per-element terms are float32 with FP contraction off.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {
namespace tt {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAX_BLOCKS = ML_TRAIN_MAX_BLOCKS;
constexpr int MAX_CLASSES = ML_EVAL_MAX_CLASSES;
constexpr int MAX_GRID_Y = 65535;

// ----------------------------------------------------------------------------- fixed-order block sum
// Thread 0 returns the block's sum: lanes by a shuffle tree, waves in index order.  Uniform call sites only.
__device__ inline double block_sum(double v) {
    __shared__ double s[WAVES];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();                                   // the previous call's read of s[] is over
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < WAVES; ++w) t += s[w];
    return t;
}

__device__ inline int block_min(int v) {
    __shared__ int s[WAVES];
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_down(v, off, 64);
        v = o < v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = s[0];
    for (int w = 1; w < WAVES; ++w) m = s[w] < m ? s[w] : m;
    return m;                                          // every thread
}

inline int blocks_for(long long n) {
    long long nb = (n + TPB - 1) / TPB;
    return (int)(nb < 1 ? 1 : nb > MAX_BLOCKS ? MAX_BLOCKS : nb);
}

// ----------------------------------------------------------------------------- ClassLoss
struct FocalArgs { float eps, one_minus_eps, alpha, gamma; };

__device__ inline float focal_term(float t, float pred, const FocalArgs &f) {        // losses.py:204-218
    const float p = pred < f.eps ? f.eps : pred > f.one_minus_eps ? f.one_minus_eps : pred;
    const float pt = t == 1.f ? p : 1.f - p;
    return f.alpha * (-powf(1.f - pt, f.gamma) * logf(pt));
}

// partial [B, nblk, 2] = (sum, count) -> out[b] = weight * sum / (count + eps): ClassLoss and BoxLoss
__global__ void class_loss_finish_kernel(const double *partial, int B, int nblk, float eps, float weight, float *out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0, n = 0.0;
    for (int k = 0; k < nblk; ++k) {
        s += partial[((long long)b * nblk + k) * 2];
        n += partial[((long long)b * nblk + k) * 2 + 1];
    }
    out[b] = weight * (float)(s / (n + (double)eps));
}

// ----------------------------------------------------------------------------- BoxLoss: beta per coordinate
// STAT 0: sum of offsets = |loc_true - loc_pred| * pos_mask per coordinate; STAT 1: sum of (offsets - mean)^2.
// partial [gridDim.x, 4] over ALL N = B * A anchors.
template <int STAT>
__global__ __launch_bounds__(TPB) void box_stat_kernel(const float *loc_true, const float *loc_pred, const float *mask, long long N,
                                                       const float *mean, double *partial) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float mu[4] = {0.f, 0.f, 0.f, 0.f};
    if (STAT == 1)
        for (int q = 0; q < 4; ++q) mu[q] = mean[q];
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < N; i += (long long)gridDim.x * TPB) {
        const float pos = mask[i] == 0.f ? 1.f : 0.f;
        const f32x4 t = *(const f32x4 *)(loc_true + 4 * i), p = *(const f32x4 *)(loc_pred + 4 * i);
        for (int q = 0; q < 4; ++q) {
            const float off = fabsf(t[q] - p[q]) * pos;
            if (STAT == 0) {
                acc[q] += (double)off;
            } else {
                const float d = off - mu[q];
                acc[q] += (double)(d * d);
            }
        }
    }
    for (int q = 0; q < 4; ++q) {
        const double s = block_sum(acc[q]);
        if (threadIdx.x == 0) partial[(long long)blockIdx.x * 4 + q] = s;
    }
}

struct BoxArgs { float momentum, one_minus_momentum, beta, weight, eps; };

// 4 threads.  STAT 0: scratch[q] = mean.  STAT 1: var, the moving values' update, scratch[4 + q] = beta per coordinate.
template <int STAT>
__global__ void box_stat_finish_kernel(const double *partial, int nblk, long long N, BoxArgs k, float *state, float *scratch) {
    const int q = threadIdx.x;
    if (q >= 4) return;
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += partial[(long long)i * 4 + q];
    const float m = (float)(s / (double)N);
    if (STAT == 0) {
        scratch[q] = m;
    } else {
        const float next_mean = state[q] * k.momentum + scratch[q] * k.one_minus_momentum;
        const float next_var = state[4 + q] * k.momentum + m * k.one_minus_momentum;
        state[q] = next_mean;
        state[4 + q] = next_var;
        const float beta = next_mean - next_var;
        scratch[4 + q] = beta < 1e-3f ? 1e-3f : beta > k.beta ? k.beta : beta;
    }
}

__global__ void box_fixed_beta_kernel(float beta, float *scratch) {
    if (threadIdx.x < 4) scratch[4 + threadIdx.x] = beta;
}

// The 8 floats behind the partials of a BoxLoss workspace: mean[4], beta[4].
inline float *box_scratch(double *partial, int B) { return (float *)(partial + (size_t)B * MAX_BLOCKS * 4); }

// scratch[4..7] = this call's beta per coordinate; with use_adjust the two statistics passes, which move `state` ONCE.
inline void launch_box_beta(const float *loc_true, const float *loc_pred, const float *mask, int B, int A, const BoxArgs &k, int use_adjust,
                            float *state, double *partial, hipStream_t s) {
    float *scratch = box_scratch(partial, B);
    if (!use_adjust) {
        hipLaunchKernelGGL(box_fixed_beta_kernel, dim3(1), dim3(64), 0, s, k.beta, scratch);
        return;
    }
    const long long N = (long long)B * A;
    const int nb = blocks_for(N);
    hipLaunchKernelGGL(box_stat_kernel<0>, dim3(nb), dim3(TPB), 0, s, loc_true, loc_pred, mask, N, (const float *)scratch, partial);
    hipLaunchKernelGGL(box_stat_finish_kernel<0>, dim3(1), dim3(64), 0, s, (const double *)partial, nb, N, k, state, scratch);
    hipLaunchKernelGGL(box_stat_kernel<1>, dim3(nb), dim3(TPB), 0, s, loc_true, loc_pred, mask, N, (const float *)scratch, partial);
    hipLaunchKernelGGL(box_stat_finish_kernel<1>, dim3(1), dim3(64), 0, s, (const double *)partial, nb, N, k, state, scratch);
}

// ----------------------------------------------------------------------------- MaskLoss, SegLoss
struct BceArgs { float eps, keep, half_smooth; };         // y = keep * t + half_smooth  (1 - label_smoothing, label_smoothing / 2)

__device__ inline float bce_term(float t, float p, const BceArgs &k) {               // losses.py:237-248
    const float y = k.keep * t + k.half_smooth;
    return -(y * logf(p + k.eps) + (1.f - y) * logf(1.f - p + k.eps));
}

// one block per (image, RoI): roi_loss [B, R] = mean BCE of the RoI's class channel, 0 for an RoI that is not selected
__global__ __launch_bounds__(TPB) void mask_roi_loss_kernel(const int32_t *target, const float *pred, int R, int hw, int C, BceArgs k,
                                                            float *roi_loss) {
    const long long row = (long long)blockIdx.y * R + blockIdx.x;
    const int32_t *t = target + row * hw;
    int m = 0x7fffffff;
    for (int i = threadIdx.x; i < hw; i += TPB) m = t[i] < m ? t[i] : m;
    const int cls = block_min(m);
    if (cls >= C || cls < 0) {                          // (a negative class cannot come out of AssignMasks; it would index nothing)
        if (threadIdx.x == 0) roi_loss[row] = 0.f;
        return;
    }
    const float *p = pred + row * hw * C + cls;
    double sum = 0.0;
    for (int i = threadIdx.x; i < hw; i += TPB) sum += (double)bce_term(t[i] == cls ? 1.f : 0.f, p[(long long)i * C], k);
    const double s = block_sum(sum);
    if (threadIdx.x == 0) roi_loss[row] = (float)(s / (double)hw);
}

__global__ void mask_loss_finish_kernel(const float *roi_loss, int B, int R, float weight, float *out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    int nz = 0;
    for (int r = 0; r < R; ++r) {
        const float l = roi_loss[(long long)b * R + r];
        s += (double)l;
        nz += l != 0.f;
    }
    out[b] = weight * (float)(s / (double)(nz + 1));
}

// partial [B, nblk, C] of seg_loss_kernel -> out [B]
__global__ void seg_loss_finish_kernel(const double *partial, const float *exist, int B, int nblk, long long HW, int C, float weight,
                                       float *out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double tot = 0.0;
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
        for (int i = 0; i < nblk; ++i) s += partial[((long long)b * nblk + i) * C + c];
        tot += (double)(exist[b * C + c] * (float)(s / (double)HW));
    }
    out[b] = weight * (float)(tot / (double)C);
}

}  // namespace tt
}  // namespace

#define ML_HIP_OK(call, what)                                                \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) {                                              \
            ml_set_error("%s: %s", what, hipGetErrorString(e_));             \
            return ML_E_LAUNCH;                                              \
        }                                                                    \
    } while (0)
