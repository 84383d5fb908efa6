// The backward of the four loss layers (engine/losses.py): each `*_grad` entry point is its forward call of
// train_targets.hip plus the gradient of sum_b upstream[b] * loss[b] with respect to the prediction, written in the pass
// that sums the loss.  The contract is in include/masklab_hip.h ("Trainer backward: the losses"); what matters here:
//
//   * the loss kernels keep the forward's block / thread mapping, statements and partial layout -- the same loop with one
//     more store -- and the finishing kernels ARE the forward's (train_terms.h), so the returned loss has the forward's bits.
//     Whoever changes a mapping changes it in both files.
//   * what reaches a loss only through a count, a comparison or an assigned variable is a constant: num_tot, num_pos, the
//     count_nonzero + 1 of MaskLoss, the clip's and the smooth-L1's branch, BoxLoss's beta.  The counts a gradient is divided
//     by are therefore taken first, by a pass over the [B,A] mask (ClassLoss, BoxLoss) or over the [B,R] RoI losses (MaskLoss).
//   * every element of `grad` is written, the zeros included; no float atomics; float32 terms with FP contraction off.
//   * the focal derivative takes log(1 - p) as log1pf(-p) and 1 - pt as p on the t = 0 side: the same function as
//     differentiating focal_term, without the float32 rounding of 1 - p in front of a logarithm near 1.
#include "common.h"
#include "train_terms.h"

#pragma clang fp contract(off)

namespace {
namespace tt {

// ----------------------------------------------------------------------------- the anchors a loss is divided by
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

// The count partials [B, MAX_BLOCKS] and the scales [B] of a ClassLoss / BoxLoss workspace: behind the (sum, count)
// partials [B, MAX_BLOCKS, 2], inside the 4 doubles per (image, block) that ml_train_workspace_bytes grants at the least.
inline double *count_partials(double *partial, int B) { return partial + (size_t)B * MAX_BLOCKS * 2; }
inline float *image_scales(double *partial, int B) { return (float *)(partial + (size_t)B * MAX_BLOCKS * 3); }

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

// class_loss_kernel of train_targets.hip plus the store: partial [B, gridDim.x, 2], grad [B, A, C]
__global__ __launch_bounds__(TPB) void class_loss_grad_kernel(const float *cls_true, const float *cls_pred, const float *mask,
                                                              const float *exists, int A, int C, FocalArgs f, const float *scale,
                                                              int through_sigmoid, double *partial, float *grad) {
    const int b = blockIdx.y;
    const float sc = scale[b];
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
            float g = 0.f;
            if (keep != 0.f) {
                g = focal_grad(t, x, f) * exists[b * C + c] * sc;
                if (through_sigmoid) g = g * sigmoid_slope(x);
            }
            grad[row * C + c] = g;
        }
    }
    const double s = block_sum(sum), n = block_sum(cnt);
    if (threadIdx.x == 0) {
        double *o = partial + ((long long)b * gridDim.x + blockIdx.x) * 2;
        o[0] = s;
        o[1] = n;
    }
}

// ----------------------------------------------------------------------------- BoxLoss
// box_loss_kernel of train_targets.hip plus the store; scale[b] carries the 1/4 of the mean over the coordinates
__global__ __launch_bounds__(TPB) void box_loss_grad_kernel(const float *loc_true, const float *loc_pred, const float *mask, int A,
                                                            const float *scratch, const float *scale, double *partial, float *grad) {
    const int b = blockIdx.y;
    const float sc = scale[b];
    float beta[4];
    for (int q = 0; q < 4; ++q) beta[q] = scratch[4 + q];
    double sum = 0.0, cnt = 0.0;
    for (int a = blockIdx.x * TPB + threadIdx.x; a < A; a += gridDim.x * TPB) {
        const long long row = (long long)b * A + a;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (mask[row] != 0.f) {
            *(f32x4 *)(grad + 4 * row) = g;
            continue;
        }
        const f32x4 t = *(const f32x4 *)(loc_true + 4 * row), p = *(const f32x4 *)(loc_pred + 4 * row);
        float l[4];
        for (int q = 0; q < 4; ++q) {                   // smooth_l1 as written: l2 where l1 < beta (losses.py:221-234)
            const float d = t[q] - p[q];
            const float l1 = fabsf(d) - 0.5f * beta[q];
            const float l2 = 0.5f * (d * d) / beta[q];
            l[q] = l1 < beta[q] ? l2 : l1;
            const float dl = l1 < beta[q] ? -d / beta[q] : d > 0.f ? -1.f : d < 0.f ? 1.f : 0.f;
            g[q] = dl * sc;
        }
        sum += (double)((((l[0] + l[1]) + l[2]) + l[3]) / 4.f);
        cnt += 1.0;
        *(f32x4 *)(grad + 4 * row) = g;
    }
    const double s = block_sum(sum), n = block_sum(cnt);
    if (threadIdx.x == 0) {
        double *o = partial + ((long long)b * gridDim.x + blockIdx.x) * 2;
        o[0] = s;
        o[1] = n;
    }
}

// ----------------------------------------------------------------------------- MaskLoss, SegLoss
__device__ inline float bce_grad(float t, float p, const BceArgs &k) {                // d bce_term / d p
    const float y = k.keep * t + k.half_smooth;
    return -(y / (p + k.eps) - (1.f - y) / (1.f - p + k.eps));
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
    int m = 0x7fffffff;
    for (int i = threadIdx.x; i < hw; i += TPB) m = t[i] < m ? t[i] : m;
    const int cls = block_min(m);
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

// seg_loss_kernel of train_targets.hip plus the store: partial [B, gridDim.x, C], grad [B, HW, C]
__global__ __launch_bounds__(TPB) void seg_loss_grad_kernel(const float *seg_true, const float *seg_pred, const float *exist,
                                                            const float *upstream, long long HW, int C, BceArgs k, float weight,
                                                            int through_sigmoid, double *partial, float *grad) {
    const int b = blockIdx.y;
    const float sc = (float)((double)(weight * upstream[b]) / ((double)C * (double)HW));
    double acc[MAX_CLASSES];
    float ex[MAX_CLASSES];
#pragma unroll
    for (int c = 0; c < MAX_CLASSES; ++c) {
        acc[c] = 0.0;
        ex[c] = c < C ? exist[b * C + c] * sc : 0.f;
    }
    for (long long px = (long long)blockIdx.x * TPB + threadIdx.x; px < HW; px += (long long)gridDim.x * TPB) {
        const long long e = ((long long)b * HW + px) * C;
#pragma unroll
        for (int c = 0; c < MAX_CLASSES; ++c)
            if (c < C) {
                const float t = seg_true[e + c], x = seg_pred[e + c];
                acc[c] += (double)bce_term(t, x, k);
                float v = bce_grad(t, x, k) * ex[c];
                if (through_sigmoid) v = v * sigmoid_slope(x);
                grad[e + c] = v;
            }
    }
#pragma unroll
    for (int c = 0; c < MAX_CLASSES; ++c)
        if (c < C) {
            const double s = block_sum(acc[c]);
            if (threadIdx.x == 0) partial[((long long)b * gridDim.x + blockIdx.x) * C + c] = s;
        }
}

}  // namespace tt
}  // namespace

using namespace tt;

extern "C" int ml_train_class_loss_grad_f32(const float *cls_true, const float *cls_pred, const float *assign_mask, const float *cls_exists,
                                            int32_t B, int32_t A, int32_t C, float weight, float alpha, float gamma, void *workspace,
                                            float *out, const float *upstream, int32_t through_sigmoid, float *grad, void *stream) {
    const char *what = "train_class_loss_grad";
    ML_REQUIRE(cls_true && cls_pred && assign_mask && cls_exists && workspace && out && upstream && grad, "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && A >= 1 && C >= 1, "%s: bad dims B=%d A=%d C=%d", what, B, A, C);
    hipStream_t s = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const int nblk = blocks_for(A);
    const float eps = 1e-7f;
    const FocalArgs f = {eps, 1.f - eps, alpha, gamma};
    launch_anchor_scale(assign_mask, upstream, B, A, 0, weight, 1.f, eps, partial, s);
    hipLaunchKernelGGL(class_loss_grad_kernel, dim3(nblk, B), dim3(TPB), 0, s, cls_true, cls_pred, assign_mask, cls_exists, A, C, f,
                       (const float *)image_scales(partial, B), through_sigmoid, partial, grad);
    hipLaunchKernelGGL(class_loss_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double *)partial, B, nblk, eps, weight, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_train_box_loss_grad_f32(const float *loc_true, const float *loc_pred, const float *assign_mask, int32_t B, int32_t A,
                                          float weight, float momentum, float one_minus_momentum, float beta, int32_t use_adjust,
                                          float *state, void *workspace, float *out, const float *upstream, float *grad, void *stream) {
    const char *what = "train_box_loss_grad";
    ML_REQUIRE(loc_true && loc_pred && assign_mask && workspace && out && upstream && grad && (state || !use_adjust), "%s: null pointer",
               what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && A >= 1, "%s: bad dims B=%d A=%d", what, B, A);
    ML_REQUIRE(ml_aligned16(loc_true) && ml_aligned16(loc_pred) && ml_aligned16(grad),
               "%s: loc_true, loc_pred and grad must be 16-byte aligned", what);
    hipStream_t s = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const BoxArgs k = {momentum, one_minus_momentum, beta, weight, 1e-7f};
    launch_box_beta(loc_true, loc_pred, assign_mask, B, A, k, use_adjust, state, partial, s);      // its partials are consumed ...
    launch_anchor_scale(assign_mask, upstream, B, A, 1, weight, 0.25f, k.eps, partial, s);         // ... before these are written
    const int nblk = blocks_for(A);
    hipLaunchKernelGGL(box_loss_grad_kernel, dim3(nblk, B), dim3(TPB), 0, s, loc_true, loc_pred, assign_mask, A,
                       (const float *)box_scratch(partial, B), (const float *)image_scales(partial, B), partial, grad);
    hipLaunchKernelGGL(class_loss_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double *)partial, B, nblk, k.eps, weight, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_train_mask_loss_grad_f32(const int32_t *mask_true, const float *mask_pred, int32_t B, int32_t R, int32_t mh, int32_t mw,
                                           int32_t C, float weight, float keep, float half_smooth, float *roi_loss, float *out,
                                           const float *upstream, int32_t through_sigmoid, float *grad, void *stream) {
    const char *what = "train_mask_loss_grad";
    ML_REQUIRE(mask_true && mask_pred && roi_loss && out && upstream && grad, "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= 32 && R >= 1 && mh >= 1 && mw >= 1 && C >= 1 && (long long)mh * mw < (1ll << 24),
               "%s: bad dims B=%d R=%d crop %d x %d C=%d (B <= 32: MoldBatch)", what, B, R, mh, mw, C);
    hipStream_t s = (hipStream_t)stream;
    const BceArgs k = {1e-7f, keep, half_smooth};
    hipLaunchKernelGGL(mask_roi_loss_kernel, dim3(R, B), dim3(TPB), 0, s, mask_true, mask_pred, R, mh * mw, C, k, roi_loss);
    hipLaunchKernelGGL(mask_loss_finish_kernel, dim3(1), dim3(64), 0, s, (const float *)roi_loss, B, R, weight, out);
    hipLaunchKernelGGL(mask_loss_grad_kernel, dim3(R, B), dim3(TPB), 0, s, mask_true, mask_pred, (const float *)roi_loss, upstream, R,
                       mh * mw, C, k, weight, through_sigmoid, grad);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_train_seg_loss_grad_f32(const float *seg_true, const float *seg_pred, const float *seg_exist, int32_t B, int64_t HW,
                                          int32_t C, float weight, float keep, float half_smooth, void *workspace, float *out,
                                          const float *upstream, int32_t through_sigmoid, float *grad, void *stream) {
    const char *what = "train_seg_loss_grad";
    ML_REQUIRE(seg_true && seg_pred && seg_exist && workspace && out && upstream && grad, "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && HW >= 1 && C >= 1 && C <= MAX_CLASSES, "%s: bad dims B=%d HW=%lld C=%d (C <= %d)", what, B,
               (long long)HW, C, MAX_CLASSES);
    hipStream_t s = (hipStream_t)stream;
    const int nblk = blocks_for(HW);
    const BceArgs k = {1e-7f, keep, half_smooth};
    hipLaunchKernelGGL(seg_loss_grad_kernel, dim3(nblk, B), dim3(TPB), 0, s, seg_true, seg_pred, seg_exist, upstream, (long long)HW, C, k,
                       weight, through_sigmoid, (double *)workspace, grad);
    hipLaunchKernelGGL(seg_loss_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double *)workspace, seg_exist, B, nblk,
                       (long long)HW, C, weight, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}
