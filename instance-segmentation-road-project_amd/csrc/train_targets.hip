// The trainer network's target assignment: the reference's CalculateIOU, AssignBoxes (detection.py:589-697), AssignMasks
// (instance.py:296-386) and AssignSeg (semantic.py:304-311).  The contract is in include/masklab_hip.h ("Trainer
// forward"); what matters here:
//
//   * no float atomics, and integer atomics only where the order cannot matter (the packed (IoU, index) maximum): the same
//     bits run to run.
//   * per-element terms are float32 with FP contraction OFF, operation by operation as NumPy evaluates
//     tests/trainer_ref.py.
//   * the four losses these targets feed, forward and backward, are in train_losses.hip; train_terms.h holds the launch
//     constants the two files share.
#include "common.h"
#include "box_iou.h"
#include "train_terms.h"

#pragma clang fp contract(off)

namespace {
namespace tt {

constexpr int GT_TILE = 64;               // ground-truth rows held in LDS at a time
constexpr int APT = 4;                    // anchors per thread of the best-prior kernel

// ----------------------------------------------------------------------------- CalculateIOU (the standalone layer)
__global__ __launch_bounds__(TPB) void iou_matrix_kernel(const float *aa, int sa, int n, const float *bb, int sb, int m, float *out) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long long)n * m) return;
    out[i] = box_iou(aa + (i / m) * sa, bb + (i % m) * sb);
}

// ----------------------------------------------------------------------------- best prior per ground truth
// iou[b, g, a] of AssignBoxes: CalculateIOU([gt, pr_boxes[0]]) times (gt cx != -1)
__device__ inline float masked_gt_iou(const float *g, const float *p) { return box_iou(g, p) * (g[0] != -1.f ? 1.f : 0.f); }

// keys [B, G] zeroed.  key = IoU bits << 32 | ~anchor: IoUs are >= +0, so the integer order of the keys is (IoU, then
// the LOWER anchor index) and the integer maximum is tf.argmax's first maximum whatever the order of the atomics.
__global__ __launch_bounds__(TPB) void best_prior_kernel(const float *gt, const int32_t *pr, int G, int A, unsigned long long *keys) {
    __shared__ float sg[GT_TILE * 4];
    __shared__ unsigned long long sk[GT_TILE];
    const int b = blockIdx.y;
    float p[APT][4];
    unsigned a[APT];
    for (int k = 0; k < APT; ++k) {
        a[k] = (unsigned)blockIdx.x * (TPB * APT) + k * TPB + threadIdx.x;
        for (int q = 0; q < 4; ++q) p[k][q] = a[k] < (unsigned)A ? (float)pr[4ll * a[k] + q] : 0.f;
    }
    for (int g0 = 0; g0 < G; g0 += GT_TILE) {
        const int n = G - g0 < GT_TILE ? G - g0 : GT_TILE;
        __syncthreads();
        for (int i = threadIdx.x; i < n * 4; i += TPB) sg[i] = gt[((long long)b * G + g0 + i / 4) * 6 + i % 4];
        if (threadIdx.x < n) sk[threadIdx.x] = 0;
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            unsigned long long key = 0;
            for (int k = 0; k < APT; ++k)
                if (a[k] < (unsigned)A) {
                    const unsigned long long c = ((unsigned long long)__float_as_uint(masked_gt_iou(sg + 4 * j, p[k])) << 32) | (0xffffffffu - a[k]);
                    key = c > key ? c : key;
                }
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_down(key, off, 64);
                key = o > key ? o : key;
            }
            if ((threadIdx.x & 63) == 0 && key) atomicMax(&sk[j], key);
        }
        __syncthreads();
        if (threadIdx.x < n && sk[threadIdx.x]) atomicMax(&keys[(long long)b * G + g0 + threadIdx.x], sk[threadIdx.x]);
    }
}

__global__ void best_finish_kernel(const unsigned long long *keys, int n, int A, int32_t *best) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned a = 0xffffffffu - (unsigned)(keys[i] & 0xffffffffu);
    best[i] = a < (unsigned)A ? (int32_t)a : 0;
}

// ----------------------------------------------------------------------------- AssignBoxes
// float32 log of a float32 quotient, rounded once from the float64 logarithm: at most a handful per prior, and loc_true
// SUMS these terms, so their last bits matter more than their cost
__device__ inline float log_f32(float x) { return (float)log((double)x); }

// One thread per anchor.  Match entries in the reference's order: every g with IoU >= 0.5 (ascending), then every g
// with conf > 0 whose best prior this is (ascending).  label = the last entry's class, loc_true = the SUM over entries.
__global__ __launch_bounds__(TPB) void assign_boxes_kernel(const float *gt, const int32_t *pr, const int32_t *best, int G, int A, int C,
                                                           float *cls_true, float *loc_true, float *assign_mask) {
    __shared__ float sg[GT_TILE * 6];
    __shared__ int32_t sb[GT_TILE];
    const int b = blockIdx.y;
    const int a = blockIdx.x * TPB + threadIdx.x;
    const bool active = a < A;
    float p[4] = {0.f, 0.f, 1.f, 1.f};
    if (active)
        for (int q = 0; q < 4; ++q) p[q] = (float)pr[4ll * a + q];
    float label = -1.f, loc[4] = {0.f, 0.f, 0.f, 0.f};
    bool ignore = false;
    for (int pass = 0; pass < 2; ++pass)
        for (int g0 = 0; g0 < G; g0 += GT_TILE) {
            const int n = G - g0 < GT_TILE ? G - g0 : GT_TILE;
            __syncthreads();
            for (int i = threadIdx.x; i < n * 6; i += TPB) sg[i] = gt[((long long)b * G + g0) * 6 + i];
            if (threadIdx.x < n) sb[threadIdx.x] = best[(long long)b * G + g0 + threadIdx.x];
            __syncthreads();
            if (!active) continue;
            for (int j = 0; j < n; ++j) {
                const float *g = sg + 6 * j;
                bool entry;
                if (pass == 0) {
                    const float iou = masked_gt_iou(g, p);
                    entry = iou >= 0.5f;
                    ignore = ignore || (iou < 0.5f && iou >= 0.4f);
                } else {
                    entry = g[5] > 0.f && sb[j] == a;
                }
                if (entry) {
                    label = g[4];
                    loc[0] += (g[0] - p[0]) / p[2];
                    loc[1] += (g[1] - p[1]) / p[3];
                    loc[2] += log_f32(g[2] / p[2]);
                    loc[3] += log_f32(g[3] / p[3]);
                }
            }
        }
    if (!active) return;
    const int li = label != -1.f ? (int)label : C;     // tf.one_hot: a class outside [0, C] lights nothing
    const long long row = (long long)b * A + a;
    for (int c = 0; c < C; ++c) cls_true[row * C + c] = c == li ? 1.f : 0.f;
    for (int q = 0; q < 4; ++q) loc_true[row * 4 + q] = loc[q];
    assign_mask[row] = ignore ? -1.f : li == C ? 1.f : 0.f;
}

// ----------------------------------------------------------------------------- AssignMasks
struct MaskDims { int R, G, H, W, mh, mw, C; float thr; };

// tf.image.crop_and_resize's sampling position along one axis, float32 as oracle/tfops.py::crop_and_resize
__device__ inline float crop_pos(float lo, float hi, int i, int out, int in) {
    if (out > 1) {
        const float step = (hi - lo) * (float)(in - 1) / (float)(out - 1);
        return lo * (float)(in - 1) + (float)i * step;
    }
    return 0.5f * (lo + hi) * (float)(in - 1);
}

// one block per (image, RoI); out int32 [B, R, mh, mw]
template <typename T>
__global__ __launch_bounds__(TPB) void assign_masks_kernel(const float *roi, const float *gt, const T *masks, MaskDims d, int32_t *out) {
    __shared__ unsigned long long skey;
    const int b = blockIdx.y, r = blockIdx.x;
    const float *box = roi + ((long long)b * d.R + r) * 6;
    const float *G0 = gt + (long long)b * d.G * 6;
    if (threadIdx.x == 0) skey = 0;
    __syncthreads();
    if (threadIdx.x < 64) {                             // argmax over the ground truths: first maximum
        unsigned long long key = 0;
        for (int g = threadIdx.x; g < d.G; g += 64) {
            const float *gb = G0 + 6 * g;
            const float live = (gb[5] != -1.f && box[5] != -1.f) ? 1.f : 0.f;
            const float same = gb[4] == box[4] ? 1.f : 0.f;
            const float iou = box_iou(gb, box) * live * same;
            const unsigned long long c = ((unsigned long long)__float_as_uint(iou) << 32) | (0xffffffffu - (unsigned)g);
            key = c > key ? c : key;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(key, off, 64);
            key = o > key ? o : key;
        }
        if (threadIdx.x == 0) skey = key;
    }
    __syncthreads();
    const unsigned long long key = skey;
    const float best = __uint_as_float((unsigned)(key >> 32));
    unsigned g = 0xffffffffu - (unsigned)(key & 0xffffffffu);
    const bool matched = key != 0 && g < (unsigned)d.G && best >= d.thr;
    int32_t *o = out + ((long long)b * d.R + r) * d.mh * d.mw;
    if (!matched) {                                     // num_classes everywhere: the crop is skipped
        for (int i = threadIdx.x; i < d.mh * d.mw; i += TPB) o[i] = d.C;
        return;
    }
    const int cls = (int)G0[6 * g + 4];
    // NormalizeBoxes(shape = the mask's (H, W)), detection.py:360-375
    const float cx = box[0], cy = box[1], w = box[2], h = box[3];
    const float x1 = (cx - w / 2.f) / (float)d.W, y1 = (cy - h / 2.f) / (float)d.H;
    const float x2 = (cx + w / 2.f) / (float)d.W, y2 = (cy + h / 2.f) / (float)d.H;
    const T *img = masks + ((long long)b * d.G + g) * d.H * d.W;
    for (int i = threadIdx.x; i < d.mh * d.mw; i += TPB) {
        const int oy = i / d.mw, ox = i - oy * d.mw;
        const float in_y = crop_pos(y1, y2, oy, d.mh, d.H), in_x = crop_pos(x1, x2, ox, d.mw, d.W);
        float v = 0.f;                                  // extrapolation value
        if (!(in_y < 0.f || in_y > (float)(d.H - 1) || in_x < 0.f || in_x > (float)(d.W - 1)) && in_y == in_y && in_x == in_x) {
            const int ty = (int)floorf(in_y), by = (int)ceilf(in_y), lx = (int)floorf(in_x), rx = (int)ceilf(in_x);
            const float fy = in_y - (float)ty, fx = in_x - (float)lx;
            const float tl = (float)img[(long long)ty * d.W + lx], tr = (float)img[(long long)ty * d.W + rx];
            const float bl = (float)img[(long long)by * d.W + lx], br = (float)img[(long long)by * d.W + rx];
            const float top = tl + (tr - tl) * fx, bot = bl + (br - bl) * fx;
            v = top + (bot - top) * fy;
        }
        o[i] = v > 0.5f ? cls : d.C;
    }
}

// ----------------------------------------------------------------------------- AssignSeg
struct SegDims { int H, W, C, oh, ow; float sy, sx; };

// round-half-to-even of resize_bilinear(align_corners=True), the arithmetic of oracle/tfops.py::resize_bilinear_align_corners
template <typename T>
__global__ __launch_bounds__(TPB) void assign_seg_kernel(const T *gt, SegDims d, long long n, float *out) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % d.C);
    const long long px = i / d.C;
    const int ox = (int)(px % d.ow), oy = (int)((px / d.ow) % d.oh);
    const long long b = px / ((long long)d.ow * d.oh);
    const float fy = (float)oy * d.sy, fx = (float)ox * d.sx;
    const float fly = floorf(fy), flx = floorf(fx);
    int ylo = (int)fly, xlo = (int)flx, yhi = (int)ceilf(fy), xhi = (int)ceilf(fx);
    ylo = ylo < 0 ? 0 : ylo > d.H - 1 ? d.H - 1 : ylo;
    xlo = xlo < 0 ? 0 : xlo > d.W - 1 ? d.W - 1 : xlo;
    yhi = yhi > d.H - 1 ? d.H - 1 : yhi < 0 ? 0 : yhi;
    xhi = xhi > d.W - 1 ? d.W - 1 : xhi < 0 ? 0 : xhi;
    const float ty = fy - fly, tx = fx - flx;
    const T *img = gt + b * d.H * d.W * d.C + c;
    const float tl = (float)img[((long long)ylo * d.W + xlo) * d.C], tr = (float)img[((long long)ylo * d.W + xhi) * d.C];
    const float bl = (float)img[((long long)yhi * d.W + xlo) * d.C], br = (float)img[((long long)yhi * d.W + xhi) * d.C];
    const float top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx;
    out[i] = rintf(top + (bot - top) * ty);
}

}  // namespace tt
}  // namespace

using namespace tt;

extern "C" int ml_train_calculate_iou_f32(const float *aa, int32_t aa_stride, int32_t n, const float *bb, int32_t bb_stride, int32_t m,
                                          float *out, void *stream) {
    const char *what = "train_calculate_iou";
    ML_REQUIRE(aa && bb && out, "%s: null pointer", what);
    ML_REQUIRE(n >= 1 && m >= 1 && aa_stride >= 4 && bb_stride >= 4 && (long long)n * m < (1ll << 38), "%s: bad dims n=%d m=%d", what, n, m);
    const long long nb = ((long long)n * m + TPB - 1) / TPB;
    hipLaunchKernelGGL(iou_matrix_kernel, dim3((unsigned)nb), dim3(TPB), 0, (hipStream_t)stream, aa, aa_stride, n, bb, bb_stride, m, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_train_best_prior_f32(const float *gt_boxes, const int32_t *pr_boxes, int32_t B, int32_t G, int32_t A, void *keys,
                                       int32_t *best, void *stream) {
    const char *what = "train_best_prior";
    ML_REQUIRE(gt_boxes && pr_boxes && keys && best, "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && G >= 1 && A >= 1 && (long long)B * G < (1ll << 31), "%s: bad dims B=%d G=%d A=%d", what, B, G, A);
    hipStream_t s = (hipStream_t)stream;
    ML_HIP_OK(hipMemsetAsync(keys, 0, sizeof(unsigned long long) * (size_t)B * G, s), what);
    hipLaunchKernelGGL(best_prior_kernel, dim3((A + TPB * APT - 1) / (TPB * APT), B), dim3(TPB), 0, s, gt_boxes, pr_boxes, G, A,
                       (unsigned long long *)keys);
    hipLaunchKernelGGL(best_finish_kernel, dim3((B * G + TPB - 1) / TPB), dim3(TPB), 0, s, (const unsigned long long *)keys, B * G, A, best);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_train_assign_boxes_f32(const float *gt_boxes, const int32_t *pr_boxes, const int32_t *best, int32_t B, int32_t G,
                                         int32_t A, int32_t C, float *cls_true, float *loc_true, float *assign_mask, void *stream) {
    const char *what = "train_assign_boxes";
    ML_REQUIRE(gt_boxes && pr_boxes && best && cls_true && loc_true && assign_mask, "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && G >= 1 && A >= 1 && C >= 1, "%s: bad dims B=%d G=%d A=%d C=%d", what, B, G, A, C);
    hipLaunchKernelGGL(assign_boxes_kernel, dim3((A + TPB - 1) / TPB, B), dim3(TPB), 0, (hipStream_t)stream, gt_boxes, pr_boxes, best, G, A,
                       C, cls_true, loc_true, assign_mask);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_train_assign_masks(const float *roi_boxes, const float *gt_boxes, const void *gt_masks, int32_t mask_dtype, int32_t B,
                                     int32_t R, int32_t G, int32_t H, int32_t W, int32_t mh, int32_t mw, int32_t C, float threshold,
                                     int32_t *out, void *stream) {
    const char *what = "train_assign_masks";
    ML_REQUIRE(roi_boxes && gt_boxes && gt_masks && out, "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && R >= 1 && G >= 1 && H >= 1 && W >= 1 && mh >= 1 && mw >= 1 && C >= 1 &&
                   (long long)H * W < (1ll << 31) && (long long)mh * mw < (1ll << 24),
               "%s: bad dims B=%d R=%d G=%d mask %d x %d crop %d x %d C=%d", what, B, R, G, H, W, mh, mw, C);
    ML_REQUIRE(mask_dtype == ML_TRAIN_MASK_I8 || mask_dtype == ML_TRAIN_MASK_U8, "%s: gt_masks must be int8 or uint8", what);
    const MaskDims d = {R, G, H, W, mh, mw, C, threshold};
    hipStream_t s = (hipStream_t)stream;
    if (mask_dtype == ML_TRAIN_MASK_I8)
        hipLaunchKernelGGL(assign_masks_kernel<int8_t>, dim3(R, B), dim3(TPB), 0, s, roi_boxes, gt_boxes, (const int8_t *)gt_masks, d, out);
    else
        hipLaunchKernelGGL(assign_masks_kernel<uint8_t>, dim3(R, B), dim3(TPB), 0, s, roi_boxes, gt_boxes, (const uint8_t *)gt_masks, d, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_train_assign_seg(const void *gt_seg, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, int32_t oh, int32_t ow,
                                   float *out, void *stream) {
    const char *what = "train_assign_seg";
    ML_REQUIRE(gt_seg && out, "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && oh >= 1 && ow >= 1 && (long long)H * W * C < (1ll << 31), "%s: bad dims", what);
    ML_REQUIRE(dtype == ML_EVAL_F32 || dtype == ML_EVAL_U8, "%s: gt_seg must be float32 or uint8", what);
    const long long n = (long long)B * oh * ow * C;
    ML_REQUIRE((n + TPB - 1) / TPB < (1ll << 31), "%s: too many elements for one launch", what);
    const SegDims d = {H, W, C, oh, ow, oh > 1 ? (float)((double)(H - 1) / (double)(oh - 1)) : 0.f,
                       ow > 1 ? (float)((double)(W - 1) / (double)(ow - 1)) : 0.f};
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = (unsigned)((n + TPB - 1) / TPB);
    if (dtype == ML_EVAL_F32)
        hipLaunchKernelGGL(assign_seg_kernel<float>, dim3(nb), dim3(TPB), 0, s, (const float *)gt_seg, d, n, out);
    else
        hipLaunchKernelGGL(assign_seg_kernel<uint8_t>, dim3(nb), dim3(TPB), 0, s, (const uint8_t *)gt_seg, d, n, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}
