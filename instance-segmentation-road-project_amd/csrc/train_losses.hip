// The trainer network's four loss layers (engine/losses.py), forward and backward.  Each loss has two entry points built
// from ONE kernel source: `ml_train_*_loss_f32` and `ml_train_*_loss_grad_f32`, which adds the gradient of
// sum_b upstream[b] * loss[b] with respect to the prediction, written in the pass that sums the loss.  The contract is in
// include/masklab_hip.h ("Trainer forward", "Trainer backward: the losses"); what matters here:
//
//   * the fused call returns the forward call's loss bit for bit.  It holds by construction: a loss kernel is a template
//     over GRAD, whose `if constexpr (GRAD)` parts only add the gradient's store to the loop that sums the loss, and both
//     forms run the same statistics, per-RoI and finishing kernels.
//   * no float atomics.  A sum is per-thread float64 -> wave shuffle tree -> one LDS word per wave -> one float64 partial
//     per block in the workspace, and a finishing kernel adds the partials of an image in block order: the same bits run
//     to run.
//   * per-element terms are float32 with FP contraction OFF, operation by operation as NumPy evaluates
//     tests/trainer_ref.py; logf / powf are the only operations that may differ from NumPy's by an ulp or two.
//   * what reaches a loss only through a count, a comparison or an assigned variable is a constant of the gradient: num_tot,
//     num_pos, the count_nonzero + 1 of MaskLoss, the clip's and the smooth-L1's branch, BoxLoss's beta.  The counts a gradient
//     is divided by are therefore taken first, by a pass over the [B,A] mask (ClassLoss, BoxLoss) or over the [B,R] RoI losses
//     (MaskLoss).
//   * every element of `grad` is written, the zeros included.
//   * the focal derivative takes log(1 - p) as log1pf(-p) and 1 - pt as p on the t = 0 side: the same function as
//     differentiating focal_term, without the float32 rounding of 1 - p in front of a logarithm near 1.
#include "common.h"
#include "train_terms.h"

#pragma clang fp contract(off)

namespace {
namespace tt {

// ----------------------------------------------------------------------------- fixed-order block reductions
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

// ----------------------------------------------------------------------------- ClassLoss and BoxLoss: (sum, count) partials
// how a ClassLoss / BoxLoss kernel ends: partial [B, gridDim.x, 2] <- the (sum, count) of image b's block blockIdx.x
__device__ inline void store_sum_count(int b, double sum, double cnt, double *partial) {
    const double s = block_sum(sum), n = block_sum(cnt);
    if (threadIdx.x == 0) {
        double *o = partial + ((long long)b * gridDim.x + blockIdx.x) * 2;
        o[0] = s;
        o[1] = n;
    }
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

// ----------------------------------------------------------------------------- the anchors a gradient is divided by
// cnt [B, gridDim.x]: #positive anchors (positives_only) or #positive + #negative anchors of the block's stride
__global__ __launch_bounds__(TPB) void anchor_count_kernel(const float *mask, int A, int positives_only, double *cnt) {
    const int b = blockIdx.y;
    double n = 0.0;
    for (int a = blockIdx.x * TPB + threadIdx.x; a < A; a += gridDim.x * TPB) {
        const float m = mask[(long long)b * A + a];
        n += (m == 0.f || (!positives_only && m == 1.f)) ? 1.0 : 0.0;
    }
    const double s = block_sum(n);
    if (threadIdx.x == 0) cnt[(long long)b * gridDim.x + blockIdx.x] = s;
}

// scale[b] = weight * upstream[b] * factor / (count_b + eps): what every derivative of image b is multiplied by
__global__ void anchor_scale_kernel(const double *cnt, const float *upstream, int B, int nblk, float weight, float factor, float eps,
                                    float *scale) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double n = 0.0;
    for (int k = 0; k < nblk; ++k) n += cnt[(long long)b * nblk + k];
    scale[b] = (float)((double)(weight * upstream[b]) / (n + (double)eps)) * factor;
}

// A ClassLoss / BoxLoss workspace, inside the 4 doubles per (image, block) that ml_train_workspace_bytes grants at the
// least: the (sum, count) partials [B, MAX_BLOCKS, 2], the count partials [B, MAX_BLOCKS], the scales [B] and, behind all
// four, BoxLoss's 8 floats mean[4], beta[4].
inline double *count_partials(double *partial, int B) { return partial + (size_t)B * MAX_BLOCKS * 2; }
inline float *image_scales(double *partial, int B) { return (float *)(partial + (size_t)B * MAX_BLOCKS * 3); }
inline float *box_scratch(double *partial, int B) { return (float *)(partial + (size_t)B * MAX_BLOCKS * 4); }

inline void launch_anchor_scale(const float *mask, const float *upstream, int B, int A, int positives_only, float weight, float factor,
                                float eps, double *partial, hipStream_t s) {
    const int nblk = blocks_for(A);
    hipLaunchKernelGGL(anchor_count_kernel, dim3(nblk, B), dim3(TPB), 0, s, mask, A, positives_only, count_partials(partial, B));
    hipLaunchKernelGGL(anchor_scale_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double *)count_partials(partial, B), upstream, B,
                       nblk, weight, factor, eps, image_scales(partial, B));
}

// pred * (1 - pred), the slope of the sigmoid that produced pred, rounded ONCE (x - x * x in one fused operation): the
// through_sigmoid gradient is then two roundings from the plain gradient's exact product, within 2 ulp of it
__device__ inline float sigmoid_slope(float x) { return fmaf(-x, x, x); }

// ----------------------------------------------------------------------------- ClassLoss
struct FocalArgs { float eps, one_minus_eps, alpha, gamma; };

__device__ inline float focal_term(float t, float pred, const FocalArgs &f) {        // losses.py:204-218
    const float p = pred < f.eps ? f.eps : pred > f.one_minus_eps ? f.one_minus_eps : pred;
    const float pt = t == 1.f ? p : 1.f - p;
    return f.alpha * (-powf(1.f - pt, f.gamma) * logf(pt));
}

// d focal_term / d pred.  0 outside the clip, passing at equality as tf.clip_by_value's gradient does.
__device__ inline float focal_grad(float t, float pred, const FocalArgs &f) {
    if (pred < f.eps || pred > f.one_minus_eps || pred != pred) return 0.f;
    const bool on = t == 1.f;
    const float pt = on ? pred : 1.f - pred;
    const float q = on ? 1.f - pred : pred;                                      // 1 - pt
    const float lg = on ? logf(pred) : log1pf(-pred);                            // log pt
    const float w = powf(q, f.gamma - 1.f);
    const float d = f.alpha * (f.gamma * w * lg - w * q / pt);                   // d term / d pt
    return on ? d : -d;
}

// partial [B, gridDim.x, 2] = (sum of the masked focal terms, #positive + #negative anchors); GRAD: grad [B, A, C]
template <bool GRAD>
__global__ __launch_bounds__(TPB) void class_loss_kernel(const float *cls_true, const float *cls_pred, const float *mask,
                                                         const float *exists, int A, int C, FocalArgs f, const float *scale,
                                                         int through_sigmoid, double *partial, float *grad) {
    const int b = blockIdx.y;
    float sc = 0.f;
    if constexpr (GRAD) sc = scale[b];
    double sum = 0.0, cnt = 0.0;
    for (int a = blockIdx.x * TPB + threadIdx.x; a < A; a += gridDim.x * TPB) {
        const long long row = (long long)b * A + a;
        const float m = mask[row];
        cnt += (m == 1.f || m == 0.f) ? 1.0 : 0.0;
        const float keep = m == -1.f ? 0.f : 1.f;
        for (int c = 0; c < C; ++c) {
            const float t = cls_true[row * C + c] != 0.f ? 1.f : 0.f;
            const float x = cls_pred[row * C + c];
            const float l = focal_term(t, x, f) * exists[b * C + c];
            sum += (double)(keep * l);
            if constexpr (GRAD) {
                float g = 0.f;
                if (keep != 0.f) {
                    g = focal_grad(t, x, f) * exists[b * C + c] * sc;
                    if (through_sigmoid) g = g * sigmoid_slope(x);
                }
                grad[row * C + c] = g;
            }
        }
    }
    store_sum_count(b, sum, cnt, partial);
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

// ----------------------------------------------------------------------------- BoxLoss
// partial [B, gridDim.x, 2] = (sum over positives of mean_q smooth_l1, #positives); GRAD: grad [B, A, 4], zeros off the
// positives, and scale[b] carries the 1/4 of the mean over the coordinates
template <bool GRAD>
__global__ __launch_bounds__(TPB) void box_loss_kernel(const float *loc_true, const float *loc_pred, const float *mask, int A,
                                                       const float *scratch, double *partial, const float *scale, float *grad) {
    const int b = blockIdx.y;
    float sc = 0.f;
    if constexpr (GRAD) sc = scale[b];
    float beta[4];
    for (int q = 0; q < 4; ++q) beta[q] = scratch[4 + q];
    double sum = 0.0, cnt = 0.0;
    for (int a = blockIdx.x * TPB + threadIdx.x; a < A; a += gridDim.x * TPB) {
        const long long row = (long long)b * A + a;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};                 // GRAD only
        if (mask[row] != 0.f) {
            if constexpr (GRAD) *(f32x4 *)(grad + 4 * row) = g;
            continue;
        }
        const f32x4 t = *(const f32x4 *)(loc_true + 4 * row), p = *(const f32x4 *)(loc_pred + 4 * row);
        float l[4];
        for (int q = 0; q < 4; ++q) {                   // smooth_l1 as written: l2 where l1 < beta (losses.py:221-234)
            const float d = t[q] - p[q];
            const float l1 = fabsf(d) - 0.5f * beta[q];
            const float l2 = 0.5f * (d * d) / beta[q];
            l[q] = l1 < beta[q] ? l2 : l1;
            if constexpr (GRAD) {
                const float dl = l1 < beta[q] ? -d / beta[q] : d > 0.f ? -1.f : d < 0.f ? 1.f : 0.f;
                g[q] = dl * sc;
            }
        }
        sum += (double)((((l[0] + l[1]) + l[2]) + l[3]) / 4.f);
        cnt += 1.0;
        if constexpr (GRAD) *(f32x4 *)(grad + 4 * row) = g;
    }
    store_sum_count(b, sum, cnt, partial);
}

// ----------------------------------------------------------------------------- MaskLoss, SegLoss: the cross entropy
struct BceArgs { float eps, keep, half_smooth; };         // y = keep * t + half_smooth  (1 - label_smoothing, label_smoothing / 2)

__device__ inline float bce_term(float t, float p, const BceArgs &k) {               // losses.py:237-248
    const float y = k.keep * t + k.half_smooth;
    return -(y * logf(p + k.eps) + (1.f - y) * logf(1.f - p + k.eps));
}

__device__ inline float bce_grad(float t, float p, const BceArgs &k) {                // d bce_term / d p
    const float y = k.keep * t + k.half_smooth;
    return -(y / (p + k.eps) - (1.f - y) / (1.f - p + k.eps));
}

// ----------------------------------------------------------------------------- MaskLoss
// an RoI's class, in every thread of its block: the minimum of its target t [hw]
__device__ inline int roi_class(const int32_t *t, int hw) {
    int m = 0x7fffffff;
    for (int i = threadIdx.x; i < hw; i += TPB) m = t[i] < m ? t[i] : m;
    return block_min(m);
}

// one block per (image, RoI): roi_loss [B, R] = mean BCE of the RoI's class channel, 0 for an RoI that is not selected
__global__ __launch_bounds__(TPB) void mask_roi_loss_kernel(const int32_t *target, const float *pred, int R, int hw, int C, BceArgs k,
                                                            float *roi_loss) {
    const long long row = (long long)blockIdx.y * R + blockIdx.x;
    const int32_t *t = target + row * hw;
    const int cls = roi_class(t, hw);
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

// one block per (image, RoI), after the RoI losses: the whole [hw, C] slab of the RoI, zeros but for the class channel of a
// selected RoI.  nz = the forward's count of the image's RoIs with a non-zero loss, recounted here from roi_loss.
__global__ __launch_bounds__(TPB) void mask_loss_grad_kernel(const int32_t *target, const float *pred, const float *roi_loss,
                                                             const float *upstream, int R, int hw, int C, BceArgs k, float weight,
                                                             int through_sigmoid, float *grad) {
    __shared__ float s_scale;
    const int b = blockIdx.y;
    const long long row = (long long)b * R + blockIdx.x;
    const int32_t *t = target + row * hw;
    const int cls = roi_class(t, hw);
    double cnt = 0.0;
    for (int r = threadIdx.x; r < R; r += TPB) cnt += roi_loss[(long long)b * R + r] != 0.f ? 1.0 : 0.0;
    const double nz = block_sum(cnt);
    if (threadIdx.x == 0) s_scale = (float)((double)(weight * upstream[b]) / (nz + 1.0) / (double)hw);
    __syncthreads();
    const float sc = s_scale;
    const bool selected = cls < C && cls >= 0;
    const float *p = pred + row * hw * C;
    float *g = grad + row * hw * C;
    const long long n = (long long)hw * C;
    for (long long i = threadIdx.x; i < n; i += TPB) {
        const long long px = i / C;
        float v = 0.f;
        if (selected && (int)(i - px * C) == cls) {
            const float x = p[i];
            v = bce_grad(t[px] == cls ? 1.f : 0.f, x, k) * sc;
            if (through_sigmoid) v = v * sigmoid_slope(x);
        }
        g[i] = v;
    }
}

// ----------------------------------------------------------------------------- SegLoss
// what only the gradient form of seg_loss_kernel holds: per class, exist[b, c] times the image's scale
template <bool GRAD> struct SegScales {};
template <> struct SegScales<true> { float ex[MAX_CLASSES]; };

// partial [B, gridDim.x, C]: per class the sum of the BCE terms over the block's pixels; GRAD: grad [B, HW, C]
template <bool GRAD>
__global__ __launch_bounds__(TPB) void seg_loss_kernel(const float *seg_true, const float *seg_pred, const float *exist,
                                                       const float *upstream, long long HW, int C, BceArgs k, float weight,
                                                       int through_sigmoid, double *partial, float *grad) {
    const int b = blockIdx.y;
    double acc[MAX_CLASSES];
    SegScales<GRAD> g;
    float sc = 0.f;
    if constexpr (GRAD) sc = (float)((double)(weight * upstream[b]) / ((double)C * (double)HW));
#pragma unroll
    for (int c = 0; c < MAX_CLASSES; ++c) {
        acc[c] = 0.0;
        if constexpr (GRAD) g.ex[c] = c < C ? exist[b * C + c] * sc : 0.f;
    }
    for (long long px = (long long)blockIdx.x * TPB + threadIdx.x; px < HW; px += (long long)gridDim.x * TPB) {
        const long long e = ((long long)b * HW + px) * C;
#pragma unroll
        for (int c = 0; c < MAX_CLASSES; ++c)
            if (c < C) {
                const float t = seg_true[e + c], x = seg_pred[e + c];
                acc[c] += (double)bce_term(t, x, k);
                if constexpr (GRAD) {
                    float v = bce_grad(t, x, k) * g.ex[c];
                    if (through_sigmoid) v = v * sigmoid_slope(x);
                    grad[e + c] = v;
                }
            }
    }
#pragma unroll
    for (int c = 0; c < MAX_CLASSES; ++c)
        if (c < C) {
            const double s = block_sum(acc[c]);
            if (threadIdx.x == 0) partial[((long long)b * gridDim.x + blockIdx.x) * C + c] = s;
        }
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

// ----------------------------------------------------------------------------- host: one body per loss
// GRAD false is the forward entry point, which passes upstream = null, through_sigmoid = 0, grad = null.
template <bool GRAD>
int class_loss(const char *what, const float *cls_true, const float *cls_pred, const float *assign_mask, const float *cls_exists, int32_t B,
               int32_t A, int32_t C, float weight, float alpha, float gamma, void *workspace, float *out, const float *upstream,
               int32_t through_sigmoid, float *grad, void *stream) {
    ML_REQUIRE(cls_true && cls_pred && assign_mask && cls_exists && workspace && out && (!GRAD || (upstream && grad)),
               "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && A >= 1 && C >= 1, "%s: bad dims B=%d A=%d C=%d", what, B, A, C);
    hipStream_t s = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const int nblk = blocks_for(A);
    const float eps = 1e-7f;
    const FocalArgs f = {eps, 1.f - eps, alpha, gamma};
    if (GRAD) launch_anchor_scale(assign_mask, upstream, B, A, 0, weight, 1.f, eps, partial, s);
    hipLaunchKernelGGL(class_loss_kernel<GRAD>, dim3(nblk, B), dim3(TPB), 0, s, cls_true, cls_pred, assign_mask, cls_exists, A, C, f,
                       (const float *)image_scales(partial, B), through_sigmoid, partial, grad);
    hipLaunchKernelGGL(class_loss_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double *)partial, B, nblk, eps, weight, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

template <bool GRAD>
int box_loss(const char *what, const float *loc_true, const float *loc_pred, const float *assign_mask, int32_t B, int32_t A, float weight,
             float momentum, float one_minus_momentum, float beta, int32_t use_adjust, float *state, void *workspace, float *out,
             const float *upstream, float *grad, void *stream) {
    ML_REQUIRE(loc_true && loc_pred && assign_mask && workspace && out && (!GRAD || (upstream && grad)) && (state || !use_adjust),
               "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && A >= 1, "%s: bad dims B=%d A=%d", what, B, A);
    ML_REQUIRE(ml_aligned16(loc_true) && ml_aligned16(loc_pred) && (!GRAD || ml_aligned16(grad)), "%s: loc_true%s must be 16-byte aligned",
               what, GRAD ? ", loc_pred and grad" : " and loc_pred");
    hipStream_t s = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const BoxArgs k = {momentum, one_minus_momentum, beta, weight, 1e-7f};
    launch_box_beta(loc_true, loc_pred, assign_mask, B, A, k, use_adjust, state, partial, s);      // its partials are consumed ...
    if (GRAD) launch_anchor_scale(assign_mask, upstream, B, A, 1, weight, 0.25f, k.eps, partial, s);   // ... before these are written
    const int nblk = blocks_for(A);
    hipLaunchKernelGGL(box_loss_kernel<GRAD>, dim3(nblk, B), dim3(TPB), 0, s, loc_true, loc_pred, assign_mask, A,
                       (const float *)box_scratch(partial, B), partial, (const float *)image_scales(partial, B), grad);
    hipLaunchKernelGGL(class_loss_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double *)partial, B, nblk, k.eps, weight, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

template <bool GRAD>
int mask_loss(const char *what, const int32_t *mask_true, const float *mask_pred, int32_t B, int32_t R, int32_t mh, int32_t mw, int32_t C,
              float weight, float keep, float half_smooth, float *roi_loss, float *out, const float *upstream, int32_t through_sigmoid,
              float *grad, void *stream) {
    ML_REQUIRE(mask_true && mask_pred && roi_loss && out && (!GRAD || (upstream && grad)), "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= 32 && R >= 1 && mh >= 1 && mw >= 1 && C >= 1 && (long long)mh * mw < (1ll << 24),
               "%s: bad dims B=%d R=%d crop %d x %d C=%d (B <= 32: MoldBatch)", what, B, R, mh, mw, C);
    hipStream_t s = (hipStream_t)stream;
    const BceArgs k = {1e-7f, keep, half_smooth};
    hipLaunchKernelGGL(mask_roi_loss_kernel, dim3(R, B), dim3(TPB), 0, s, mask_true, mask_pred, R, mh * mw, C, k, roi_loss);
    hipLaunchKernelGGL(mask_loss_finish_kernel, dim3(1), dim3(64), 0, s, (const float *)roi_loss, B, R, weight, out);
    if (GRAD)
        hipLaunchKernelGGL(mask_loss_grad_kernel, dim3(R, B), dim3(TPB), 0, s, mask_true, mask_pred, (const float *)roi_loss, upstream, R,
                           mh * mw, C, k, weight, through_sigmoid, grad);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

template <bool GRAD>
int seg_loss(const char *what, const float *seg_true, const float *seg_pred, const float *seg_exist, int32_t B, int64_t HW, int32_t C,
             float weight, float keep, float half_smooth, void *workspace, float *out, const float *upstream, int32_t through_sigmoid,
             float *grad, void *stream) {
    ML_REQUIRE(seg_true && seg_pred && seg_exist && workspace && out && (!GRAD || (upstream && grad)), "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && HW >= 1 && C >= 1 && C <= MAX_CLASSES, "%s: bad dims B=%d HW=%lld C=%d (C <= %d)", what, B,
               (long long)HW, C, MAX_CLASSES);
    hipStream_t s = (hipStream_t)stream;
    const int nblk = blocks_for(HW);
    const BceArgs k = {1e-7f, keep, half_smooth};
    hipLaunchKernelGGL(seg_loss_kernel<GRAD>, dim3(nblk, B), dim3(TPB), 0, s, seg_true, seg_pred, seg_exist, upstream, (long long)HW, C, k,
                       weight, through_sigmoid, (double *)workspace, grad);
    hipLaunchKernelGGL(seg_loss_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double *)workspace, seg_exist, B, nblk,
                       (long long)HW, C, weight, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

}  // namespace tt
}  // namespace

using namespace tt;

extern "C" int64_t ml_train_workspace_bytes(int32_t B, int32_t C) {
    if (B < 1 || C < 1) return 0;
    const int64_t per = C > 4 ? C : 4;
    return (int64_t)sizeof(double) * ((int64_t)B * MAX_BLOCKS * per + 16);
}

extern "C" int ml_train_class_loss_f32(const float *cls_true, const float *cls_pred, const float *assign_mask, const float *cls_exists,
                                       int32_t B, int32_t A, int32_t C, float weight, float alpha, float gamma, void *workspace,
                                       float *out, void *stream) {
    return class_loss<false>("train_class_loss", cls_true, cls_pred, assign_mask, cls_exists, B, A, C, weight, alpha, gamma, workspace, out,
                             nullptr, 0, nullptr, stream);
}

extern "C" int ml_train_class_loss_grad_f32(const float *cls_true, const float *cls_pred, const float *assign_mask, const float *cls_exists,
                                            int32_t B, int32_t A, int32_t C, float weight, float alpha, float gamma, void *workspace,
                                            float *out, const float *upstream, int32_t through_sigmoid, float *grad, void *stream) {
    return class_loss<true>("train_class_loss_grad", cls_true, cls_pred, assign_mask, cls_exists, B, A, C, weight, alpha, gamma, workspace,
                            out, upstream, through_sigmoid, grad, stream);
}

extern "C" int ml_train_box_loss_f32(const float *loc_true, const float *loc_pred, const float *assign_mask, int32_t B, int32_t A,
                                     float weight, float momentum, float one_minus_momentum, float beta, int32_t use_adjust,
                                     float *state, void *workspace, float *out, void *stream) {
    return box_loss<false>("train_box_loss", loc_true, loc_pred, assign_mask, B, A, weight, momentum, one_minus_momentum, beta, use_adjust,
                           state, workspace, out, nullptr, nullptr, stream);
}

extern "C" int ml_train_box_loss_grad_f32(const float *loc_true, const float *loc_pred, const float *assign_mask, int32_t B, int32_t A,
                                          float weight, float momentum, float one_minus_momentum, float beta, int32_t use_adjust,
                                          float *state, void *workspace, float *out, const float *upstream, float *grad, void *stream) {
    return box_loss<true>("train_box_loss_grad", loc_true, loc_pred, assign_mask, B, A, weight, momentum, one_minus_momentum, beta,
                          use_adjust, state, workspace, out, upstream, grad, stream);
}

extern "C" int ml_train_mask_loss_f32(const int32_t *mask_true, const float *mask_pred, int32_t B, int32_t R, int32_t mh, int32_t mw,
                                      int32_t C, float weight, float keep, float half_smooth, float *roi_loss, float *out, void *stream) {
    return mask_loss<false>("train_mask_loss", mask_true, mask_pred, B, R, mh, mw, C, weight, keep, half_smooth, roi_loss, out, nullptr, 0,
                            nullptr, stream);
}

extern "C" int ml_train_mask_loss_grad_f32(const int32_t *mask_true, const float *mask_pred, int32_t B, int32_t R, int32_t mh, int32_t mw,
                                           int32_t C, float weight, float keep, float half_smooth, float *roi_loss, float *out,
                                           const float *upstream, int32_t through_sigmoid, float *grad, void *stream) {
    return mask_loss<true>("train_mask_loss_grad", mask_true, mask_pred, B, R, mh, mw, C, weight, keep, half_smooth, roi_loss, out,
                           upstream, through_sigmoid, grad, stream);
}

extern "C" int ml_train_seg_loss_f32(const float *seg_true, const float *seg_pred, const float *seg_exist, int32_t B, int64_t HW, int32_t C,
                                     float weight, float keep, float half_smooth, void *workspace, float *out, void *stream) {
    return seg_loss<false>("train_seg_loss", seg_true, seg_pred, seg_exist, B, HW, C, weight, keep, half_smooth, workspace, out, nullptr, 0,
                           nullptr, stream);
}

extern "C" int ml_train_seg_loss_grad_f32(const float *seg_true, const float *seg_pred, const float *seg_exist, int32_t B, int64_t HW,
                                          int32_t C, float weight, float keep, float half_smooth, void *workspace, float *out,
                                          const float *upstream, int32_t through_sigmoid, float *grad, void *stream) {
    return seg_loss<true>("train_seg_loss_grad", seg_true, seg_pred, seg_exist, B, HW, C, weight, keep, half_smooth, workspace, out,
                          upstream, through_sigmoid, grad, stream);
}
