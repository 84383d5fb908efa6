// The reference's evaluation loop (road_project/train.py:101-209) and metric layers (engine/metrics.py) as integer
// counting kernels.  The contract is in include/masklab_hip.h ("Evaluation"); what matters here:
//
//   * every kernel COUNTS: per-thread uint32 counters -> wave shuffle -> LDS -> one 64-bit integer atomic per block and
//     counter.  Integer sums do not depend on their order, so every output has the same bits run to run.  No float atomics.
//   * no [n,H,W] canvas: a pair's blocks walk only the pixels of the predicted box, recompute the pasted mask's value
//     there (cv2.resize INTER_LINEAR restated, float64) from the h x w mask held in LDS, and read the ground truth once.
//   * the float arithmetic that decides a bit (the resize taps, the box IoUs of DetectionIOUMetric, the metric formulas)
//     runs with FP contraction OFF, operation by operation as NumPy evaluates the restatement.
//   * the per-thread bodies are __host__ __device__ functions of a thread index t out of T: ml_eval_reference_host runs
//     the mask-area, mask-pair and semantic bodies in CPU loops, so the CPU tests hold this very code to NumPy.
#include "common.h"
#include "box_iou.h"
#include "cv_resize.h"

#pragma clang fp contract(off)

namespace {
namespace ev {

constexpr int TPB = 256;
constexpr int MAX_CLASSES = ML_EVAL_MAX_CLASSES;
constexpr int MAX_GRID_Y = 65535;
constexpr int HOST_THREADS = 64;          // T of the CPU loops (any T >= 16 gives the same sums)

// ----------------------------------------------------------------------------- block reduction of K counters
template <int K>
__device__ inline void block_add(const uint32_t (&v)[K], unsigned long long *dst) {
    __shared__ unsigned long long s[K];
    if (threadIdx.x < K) s[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        unsigned long long x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(&s[k], x);
    }
    __syncthreads();
    if (threadIdx.x < K && s[threadIdx.x]) atomicAdd(dst + threadIdx.x, s[threadIdx.x]);
}

// ----------------------------------------------------------------------------- ml_eval_mask_area
struct alignas(16) Bytes16 { uint32_t v[4]; };

__host__ __device__ inline uint32_t nonzero_bytes(uint32_t w) {       // how many of the 4 bytes are non-zero
    const uint32_t t = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
    return (uint32_t)__builtin_popcount(t);
}

// Thread t of T (T >= 16) over the n bytes of one mask: scalar bytes up to the first 16-byte boundary, 16-byte loads,
// scalar bytes for the last (n - head) mod 16.
__host__ __device__ inline uint32_t area_thread(const uint8_t *p, long long n, long long t, long long T) {
    long long head = (long long)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u);
    if (head > n) head = n;
    const long long nvec = (n - head) / 16, tail = head + nvec * 16;
    uint32_t c = 0;
    if (t < head) c += p[t] != 0;
    if (t < n - tail) c += p[tail + t] != 0;
    const Bytes16 *v = (const Bytes16 *)(p + head);
    for (long long i = t; i < nvec; i += T) {
        const Bytes16 q = v[i];
        c += nonzero_bytes(q.v[0]) + nonzero_bytes(q.v[1]) + nonzero_bytes(q.v[2]) + nonzero_bytes(q.v[3]);
    }
    return c;
}

__global__ __launch_bounds__(TPB) void mask_area_kernel(const uint8_t *gt, long long n, int blocks_per_mask,
                                                        unsigned long long *out) {
    const long long m = blockIdx.x / blocks_per_mask;
    const int c = blockIdx.x % blocks_per_mask;
    const uint32_t v[1] = {area_thread(gt + m * n, n, (long long)c * TPB + threadIdx.x, (long long)blocks_per_mask * TPB)};
    block_add<1>(v, out + m);
}

// ----------------------------------------------------------------------------- thresholded counts per (image, class)
// ml_eval_semantic_counts (NOUT = 2: both, either) and the counts of ClassBinaryIOU (NOUT = 3: true, pred, both).
template <typename T> struct alignas(sizeof(T) * 4) Vec4 { T v[4]; };

template <typename T> __host__ __device__ inline bool above(T v, float thr) { return (float)v > thr; }     // exact: u8, f16, f32
template <> __host__ __device__ inline bool above<int32_t>(int32_t v, float thr) { return (double)v > (double)thr; }

template <int NOUT> __host__ __device__ inline void tally(bool t, bool p, uint32_t *acc) {
    if (NOUT == 2) {
        acc[0] += t && p;
        acc[1] += t || p;
    } else {
        acc[0] += t;
        acc[1] += p;
        acc[2] += t && p;
    }
}

// Thread t of T over the image that holds elements [start, start + n) of the flat [B, HW, C] tensors (both 16-byte
// aligned at element 0).  T is a multiple of C, so the four elements of each of the thread's 4-element groups keep
// their classes cls[0..3] through the whole loop and the counters stay in registers.
template <typename TT, typename TP, int NOUT>
__host__ __device__ inline void counts_thread(const TT *tr, const TP *pr, long long start, long long n, int C, float thr,
                                              long long t, long long T, uint32_t (&acc)[4][NOUT], int (&cls)[4]) {
    const long long end = start + n, a0 = (start + 3) & ~3ll;
    const long long ng = a0 < end ? (end - a0) / 4 : 0;
    for (int k = 0; k < 4; ++k) {
        cls[k] = (int)((a0 + 4 * t + k - start) % C);
        for (int o = 0; o < NOUT; ++o) acc[k][o] = 0;
    }
    const Vec4<TT> *vt = (const Vec4<TT> *)tr;
    const Vec4<TP> *vp = (const Vec4<TP> *)pr;
    for (long long g = t; g < ng; g += T) {
        const Vec4<TT> a = vt[a0 / 4 + g];
        const Vec4<TP> b = vp[a0 / 4 + g];
        for (int k = 0; k < 4; ++k) tally<NOUT>(above(a.v[k], thr), above(b.v[k], thr), acc[k]);
    }
}

// The at most 3 + 3 elements in front of the first and behind the last whole group: edge j = 0..5.
template <typename TT, typename TP, int NOUT>
__host__ __device__ inline bool counts_edge(const TT *tr, const TP *pr, long long start, long long n, int C, float thr, int j,
                                            uint32_t (&acc)[NOUT], int &cls) {
    const long long end = start + n, a0 = (start + 3) & ~3ll;
    const long long ng = a0 < end ? (end - a0) / 4 : 0;
    long long e;
    if (j < 3) {
        e = start + j;
        if (e >= a0 || e >= end) return false;
    } else {
        e = a0 + 4 * ng + (j - 3);
        if (a0 >= end || e >= end) return false;
    }
    cls = (int)((e - start) % C);
    for (int o = 0; o < NOUT; ++o) acc[o] = 0;
    tally<NOUT>(above(tr[e], thr), above(pr[e], thr), acc);
    return true;
}

template <typename TT, typename TP, int NOUT>
__global__ __launch_bounds__(TPB) void counts_kernel(const TT *tr, const TP *pr, long long n, int C, float thr,
                                                     unsigned long long *out) {
    __shared__ uint32_t sc[MAX_CLASSES * NOUT];
    const int b = blockIdx.y;
    if (threadIdx.x < C * NOUT) sc[threadIdx.x] = 0;
    __syncthreads();
    long long T = (long long)gridDim.x * TPB;
    T -= T % C;
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    if (t < T) {
        uint32_t acc[4][NOUT];
        int cls[4];
        counts_thread<TT, TP, NOUT>(tr, pr, b * n, n, C, thr, t, T, acc, cls);
        for (int k = 0; k < 4; ++k)
            for (int o = 0; o < NOUT; ++o)
                if (acc[k][o]) atomicAdd(&sc[cls[k] * NOUT + o], acc[k][o]);
    }
    if (blockIdx.x == 0 && threadIdx.x < 6) {
        uint32_t acc[NOUT];
        int cls;
        if (counts_edge<TT, TP, NOUT>(tr, pr, b * n, n, C, thr, (int)threadIdx.x, acc, cls))
            for (int o = 0; o < NOUT; ++o)
                if (acc[o]) atomicAdd(&sc[cls * NOUT + o], acc[o]);
    }
    __syncthreads();
    if (threadIdx.x < C * NOUT && sc[threadIdx.x])
        atomicAdd(out + (long long)b * C * NOUT + threadIdx.x, (unsigned long long)sc[threadIdx.x]);
}

template <typename TT, typename TP, int NOUT>
void launch_counts(const void *tr, const void *pr, int B, long long n, int C, float thr, void *out, hipStream_t s) {
    long long blocks = (n / 4 + TPB * 8 - 1) / (TPB * 8);
    blocks = blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL((counts_kernel<TT, TP, NOUT>), dim3((unsigned)blocks, B), dim3(TPB), 0, s, (const TT *)tr,
                       (const TP *)pr, n, C, thr, (unsigned long long *)out);
}

template <typename TT, typename TP, int NOUT>
void host_counts(const TT *tr, const TP *pr, int B, long long n, int C, float thr, int64_t *out) {
    const long long T = HOST_THREADS - HOST_THREADS % C;
    for (int b = 0; b < B; ++b) {
        int64_t *o = out + (long long)b * C * NOUT;
        for (long long t = 0; t < T; ++t) {
            uint32_t acc[4][NOUT];
            int cls[4];
            counts_thread<TT, TP, NOUT>(tr, pr, b * n, n, C, thr, t, T, acc, cls);
            for (int k = 0; k < 4; ++k)
                for (int q = 0; q < NOUT; ++q) o[cls[k] * NOUT + q] += acc[k][q];
        }
        for (int j = 0; j < 6; ++j) {
            uint32_t acc[NOUT];
            int cls;
            if (counts_edge<TT, TP, NOUT>(tr, pr, b * n, n, C, thr, j, acc, cls))
                for (int q = 0; q < NOUT; ++q) o[cls * NOUT + q] += acc[q];
        }
    }
}

// ClassBinaryIOU.call's float32 tail (engine/metrics.py:96-99) on the integer counts; iou [C, B].
__global__ void class_iou_kernel(const unsigned long long *counts, int B, int C, float *iou) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i % C;
    const float area_true = (float)counts[3 * i], area_pred = (float)counts[3 * i + 1], inter = (float)counts[3 * i + 2];
    const float uni = area_true + area_pred - inter;
    iou[(long long)c * B + b] = uni > 0.f ? inter / uni : 1.f;
}

// ----------------------------------------------------------------------------- ml_eval_mask_pairs
struct Box { int sx, sy, bw, bh; };

__host__ __device__ inline double clip0(double v, double hi) { return v < 0.0 ? 0.0 : v > hi ? hi : v; }

// train.py:128-136 on a detection row (cx, cy, w, h, label, conf), int32 -> float64, corners truncated to int32
__host__ __device__ inline Box pred_box(const int32_t *d, int H, int W) {
    const double cx = d[0], cy = d[1], w = d[2], h = d[3];
    const int sx = (int)clip0(cx - w / 2, W), ex = (int)clip0(cx + w / 2, W);
    const int sy = (int)clip0(cy - h / 2, H), ey = (int)clip0(cy + h / 2, H);
    return {sx, sy, ex - sx, ey - sy};
}

// one axis of cv2.resize(INTER_LINEAR): cv_resize.h, shared with cv_resize.hip
using cvr::Tap;
using cvr::axis_scale;
using cvr::axis_tap;

// m: the h x w mask, already max(., 0).  Horizontal taps inside each of the two source rows, then the two rows.
__host__ __device__ inline bool pred_pixel(const int32_t *m, int mw, const Tap &ty, const Tap &tx) {
    const int32_t *r0 = m + ty.s0 * mw, *r1 = m + ty.s1 * mw;
    const double h0 = (double)r0[tx.s0] * (double)tx.w0 + (double)r0[tx.s1] * (double)tx.w1;
    const double h1 = (double)r1[tx.s0] * (double)tx.w0 + (double)r1[tx.s1] * (double)tx.w1;
    return h0 * (double)ty.w0 + h1 * (double)ty.w1 > 0.5;
}

// Thread t of T over the box's bh x bw pixels; g: the [H, W] ground-truth mask (set = non-zero byte).
__host__ __device__ inline void pair_thread(const int32_t *m, int mh, int mw, const Box &bx, const uint8_t *g, int W, long long t,
                                            long long T, uint32_t &inter, uint32_t &area) {
    const unsigned npix = (unsigned)bx.bw * (unsigned)bx.bh, bw = (unsigned)bx.bw;      // H * W < 2^31
    const double scale_y = axis_scale(bx.bh, mh), scale_x = axis_scale(bx.bw, mw);
    for (long long q64 = t; q64 < (long long)npix; q64 += T) {
        const unsigned q = (unsigned)q64, r = q / bw, c = q - r * bw;
        if (pred_pixel(m, mw, axis_tap((int)r, scale_y, mh), axis_tap((int)c, scale_x, mw))) {
            ++area;
            inter += g[(long long)(bx.sy + (int)r) * W + bx.sx + (int)c] != 0;
        }
    }
}

struct PairDims { int P, B, n, mh, mw, G, H, W; };

__host__ __device__ inline bool pair_valid(const int32_t *pair, const PairDims &d) {
    return pair[0] >= 0 && pair[0] < d.B && pair[1] >= 0 && pair[1] < d.n && pair[2] >= 0 && pair[2] < d.G;
}

// out [P, 2] zeroed: (intersection, predicted area) accumulate; pairs_finish_kernel turns the second into the union.
__global__ __launch_bounds__(TPB) void pairs_kernel(const int32_t *det, const int32_t *ins, const uint8_t *gt, const int32_t *pairs,
                                                    PairDims d, unsigned long long *out) {
    extern __shared__ int32_t sm[];
    const int p = blockIdx.y;
    const int32_t *pair = pairs + 3ll * p;
    if (!pair_valid(pair, d)) return;                                  // the finishing kernel writes (-1, -1)
    const long long row = (long long)pair[0] * d.n + pair[1];
    const Box bx = pred_box(det + row * 6, d.H, d.W);
    if (bx.bw <= 0 || bx.bh <= 0) return;                              // empty mask
    const long long npix = (long long)bx.bw * bx.bh;
    if ((long long)blockIdx.x * TPB >= npix) return;
    const int32_t *m = ins + row * d.mh * d.mw;
    for (int i = threadIdx.x; i < d.mh * d.mw; i += TPB) sm[i] = m[i] > 0 ? m[i] : 0;
    __syncthreads();
    uint32_t v[2] = {0, 0};
    pair_thread(sm, d.mh, d.mw, bx, gt + ((long long)pair[0] * d.G + pair[2]) * d.H * d.W, d.W,
                (long long)blockIdx.x * TPB + threadIdx.x, (long long)gridDim.x * TPB, v[0], v[1]);
    block_add<2>(v, out + 2ll * p);
}

__global__ void pairs_finish_kernel(const int32_t *pairs, const long long *gt_area, PairDims d, long long *out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= d.P) return;
    const int32_t *pair = pairs + 3ll * p;
    if (!pair_valid(pair, d)) {
        out[2 * p] = out[2 * p + 1] = -1;
        return;
    }
    out[2 * p + 1] += gt_area[(long long)pair[0] * d.G + pair[2]] - out[2 * p];
}

// ----------------------------------------------------------------------------- DetectionIOUMetric
// box_iou (CalculateIOU.call for one pair) and NumPy's minimum / maximum: box_iou.h, shared with train_targets.hip
__host__ __device__ inline float masked_iou(const float *a, const float *g) {     // metrics.py:136-147, logical_or as written
    return box_iou(a, g) * ((a[0] != -1.f || g[0] != -1.f) ? 1.f : 0.f);
}

// one block per image; out [3, B] = precision, recall, fmeasure
__global__ __launch_bounds__(TPB) void detection_metric_kernel(const float *prop, const float *gt, int B, int np_, int ng, float *out) {
    const int b = blockIdx.x;
    const float *P = prop + (long long)b * np_ * 6, *G = gt + (long long)b * ng * 6;
    uint32_t v[4] = {0, 0, 0, 0};                                      // num_pos, num_true, num_pred, num_gt
    for (int i = threadIdx.x; i < np_; i += TPB) {
        v[2] += P[i * 6] != -1.f;
        if (ng > 0) {
            float m = masked_iou(P + i * 6, G);
            for (int j = 1; j < ng; ++j) m = np_max(m, masked_iou(P + i * 6, G + j * 6));
            v[0] += m > 0.5f;
        }
    }
    for (int j = threadIdx.x; j < ng; j += TPB) {
        v[3] += G[j * 6] != -1.f;
        if (np_ > 0) {
            float m = masked_iou(P, G + j * 6);
            for (int i = 1; i < np_; ++i) m = np_max(m, masked_iou(P + i * 6, G + j * 6));
            v[1] += m > 0.5f;
        }
    }
    __shared__ unsigned long long tot[4];
    if (threadIdx.x < 4) tot[threadIdx.x] = 0;
    __syncthreads();
    block_add<4>(v, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float eps = 1e-7f;                                       // K.epsilon()
        const float pr = (float)tot[0] / ((float)tot[2] + eps), rc = (float)tot[1] / ((float)tot[3] + eps);
        out[b] = pr;
        out[B + b] = rc;
        out[2 * B + b] = 2.f * (pr * rc) / (pr + rc + eps);
    }
}

// ----------------------------------------------------------------------------- ConfusionMatrixMetric
__host__ __device__ inline int first_argmax(const float *x, int C) {   // tf.argmax: the first maximum wins
    int best = 0;
    for (int c = 1; c < C; ++c)
        if (x[c] > x[best]) best = c;
    return best;
}

// metrics.py:27-54 for one anchor -> 0 tp, 1 fp, 2 fn, 3 tn, or -1 for an ignored anchor (mask == -1)
__host__ __device__ inline int confusion_anchor(const float *t, const float *p, float mask, int C, float thr) {
    if (mask == -1.f) return -1;
    const int y_true = mask == 0.f ? first_argmax(t, C) : C;
    const int ap = first_argmax(p, C);
    const int y_pred = p[ap] > thr ? ap : C;
    const bool same = y_true == y_pred, pos = y_pred < C;
    return same ? (pos ? 0 : 3) : (pos ? 1 : 2);
}

__global__ __launch_bounds__(TPB) void confusion_kernel(const float *t, const float *p, const float *mask, long long N, int C,
                                                        float thr, unsigned long long *counts) {
    uint32_t v[4] = {0, 0, 0, 0};
    for (long long a = (long long)blockIdx.x * TPB + threadIdx.x; a < N; a += (long long)gridDim.x * TPB) {
        const int k = confusion_anchor(t + a * C, p + a * C, mask[a], C, thr);
        v[0] += k == 0;
        v[1] += k == 1;
        v[2] += k == 2;
        v[3] += k == 3;
    }
    block_add<4>(v, counts);
}

__global__ void confusion_finish_kernel(const unsigned long long *counts, float *m) {     // metrics.py:56-59, float32
    const float eps = 1e-7f;
    const float tp = (float)counts[0], fp = (float)counts[1], fn = (float)counts[2], tn = (float)counts[3];
    const float precision = tp / (tp + fp + eps), recall = tp / (tp + fn + eps);
    m[0] = precision;
    m[1] = recall;
    m[2] = (tp + tn) / (tp + tn + fp + fn + eps);
    m[3] = 2.f * (precision * recall) / (precision + recall + eps);
}

// ----------------------------------------------------------------------------- argument checks
int check_masks(const char *what, const void *gt, int B, int G, int H, int W) {
    ML_REQUIRE(gt, "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && G >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "%s: bad dims B=%d G=%d H=%d W=%d", what, B,
               G, H, W);
    return ML_OK;
}

int check_pairs(const char *what, const void *det, const void *ins, const void *gt, const void *gt_area, const void *pairs,
                const void *out, const PairDims &d) {
    ML_REQUIRE(det && ins && gt && gt_area && out && (pairs || d.P == 0), "%s: null pointer", what);
    ML_REQUIRE(d.P >= 0 && d.n >= 1 && d.mh >= 1 && d.mw >= 1 && (long long)d.mh * d.mw <= ML_EVAL_MAX_MASK,
               "%s: bad dims P=%d n=%d mask %d x %d (the mask is held in LDS: at most 16368 entries)", what, d.P, d.n, d.mh, d.mw);
    return check_masks(what, gt, d.B, d.G, d.H, d.W);
}

int check_counts(const char *what, const void *tr, const void *pr, const void *out, int B, long long HW, int C) {
    ML_REQUIRE(tr && pr && out, "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && B <= MAX_GRID_Y && HW >= 1 && C >= 1 && C <= MAX_CLASSES && HW * C < (1ll << 31),
               "%s: bad dims B=%d HW=%lld C=%d (C <= %d, HW*C < 2^31)", what, B, HW, C, MAX_CLASSES);
    ML_REQUIRE(ml_aligned16(tr) && ml_aligned16(pr), "%s: the maps must be 16-byte aligned", what);
    return ML_OK;
}

}  // namespace ev
}  // namespace

using namespace ev;

#define ML_HIP_OK(call, what)                                                \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) {                                              \
            ml_set_error("%s: %s", what, hipGetErrorString(e_));             \
            return ML_E_LAUNCH;                                              \
        }                                                                    \
    } while (0)

extern "C" int ml_eval_mask_area(const void *gt, int32_t B, int32_t G, int32_t H, int32_t W, int64_t *out, void *stream) {
    const char *what = "eval_mask_area";
    const int e = check_masks(what, gt, B, G, H, W);
    if (e != ML_OK) return e;
    ML_REQUIRE(out, "%s: null pointer", what);
    const long long n = (long long)H * W, masks = (long long)B * G;
    long long bpm = (n / 16 + TPB * 4 - 1) / (TPB * 4);
    bpm = bpm < 1 ? 1 : bpm > 64 ? 64 : bpm;
    ML_REQUIRE(masks * bpm < (1ll << 31), "%s: %lld masks are too many for one launch", what, masks);
    hipStream_t s = (hipStream_t)stream;
    ML_HIP_OK(hipMemsetAsync(out, 0, sizeof(int64_t) * masks, s), what);
    hipLaunchKernelGGL(mask_area_kernel, dim3((unsigned)(masks * bpm)), dim3(TPB), 0, s, (const uint8_t *)gt, n, (int)bpm,
                       (unsigned long long *)out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_eval_mask_pairs(const int32_t *det, const int32_t *ins, const void *gt, const int64_t *gt_area, const int32_t *pairs,
                                  int32_t P, int32_t B, int32_t n, int32_t mh, int32_t mw, int32_t G, int32_t H, int32_t W,
                                  int64_t *out, void *stream) {
    const char *what = "eval_mask_pairs";
    const PairDims d = {P, B, n, mh, mw, G, H, W};
    const int e = check_pairs(what, det, ins, gt, gt_area, pairs, out, d);
    if (e != ML_OK) return e;
    if (P == 0) return ML_OK;
    hipStream_t s = (hipStream_t)stream;
    ML_HIP_OK(hipMemsetAsync(out, 0, sizeof(int64_t) * 2 * P, s), what);
    long long nb = ((long long)H * W + TPB * 8 - 1) / (TPB * 8);
    nb = nb < 1 ? 1 : nb > 128 ? 128 : nb;
    for (int p0 = 0; p0 < P; p0 += MAX_GRID_Y) {
        const int np_ = P - p0 < MAX_GRID_Y ? P - p0 : MAX_GRID_Y;
        hipLaunchKernelGGL(pairs_kernel, dim3((unsigned)nb, np_), dim3(TPB), (size_t)mh * mw * 4, s, det, ins, (const uint8_t *)gt,
                           pairs + 3ll * p0, d, (unsigned long long *)out + 2ll * p0);
    }
    hipLaunchKernelGGL(pairs_finish_kernel, dim3((P + TPB - 1) / TPB), dim3(TPB), 0, s, pairs, (const long long *)gt_area, d,
                       (long long *)out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_eval_semantic_counts(const int32_t *pr, const uint8_t *gt, int32_t B, int32_t H, int32_t W, int32_t C, int64_t *out,
                                       void *stream) {
    const char *what = "eval_semantic_counts";
    ML_REQUIRE(H >= 1 && W >= 1, "%s: bad dims H=%d W=%d", what, H, W);
    const int e = check_counts(what, gt, pr, out, B, (long long)H * W, C);
    if (e != ML_OK) return e;
    hipStream_t s = (hipStream_t)stream;
    ML_HIP_OK(hipMemsetAsync(out, 0, sizeof(int64_t) * 2 * B * C, s), what);
    launch_counts<uint8_t, int32_t, 2>(gt, pr, B, (long long)H * W * C, C, 0.5f, out, s);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_eval_class_binary_iou(const void *seg_true, int32_t true_dtype, const void *seg_pred, int32_t pred_dtype, int32_t B,
                                        int64_t HW, int32_t C, float threshold, int64_t *counts, float *iou, void *stream) {
    const char *what = "eval_class_binary_iou";
    const int e = check_counts(what, seg_true, seg_pred, counts, B, HW, C);
    if (e != ML_OK) return e;
    ML_REQUIRE(iou, "%s: null pointer", what);
    const bool same = true_dtype == pred_dtype && true_dtype >= ML_EVAL_F32 && true_dtype <= ML_EVAL_U8;
    ML_REQUIRE(same || (true_dtype == ML_EVAL_U8 && pred_dtype == ML_EVAL_I32),
               "%s: dtypes (%d, %d): both maps of one of f32 / f16 / i32 / u8, or u8 truth with i32 predictions", what, true_dtype,
               pred_dtype);
    hipStream_t s = (hipStream_t)stream;
    ML_HIP_OK(hipMemsetAsync(counts, 0, sizeof(int64_t) * 3 * B * C, s), what);
    const long long n = HW * C;
    if (!same)
        launch_counts<uint8_t, int32_t, 3>(seg_true, seg_pred, B, n, C, threshold, counts, s);
    else if (true_dtype == ML_EVAL_F32)
        launch_counts<float, float, 3>(seg_true, seg_pred, B, n, C, threshold, counts, s);
    else if (true_dtype == ML_EVAL_F16)
        launch_counts<_Float16, _Float16, 3>(seg_true, seg_pred, B, n, C, threshold, counts, s);
    else if (true_dtype == ML_EVAL_I32)
        launch_counts<int32_t, int32_t, 3>(seg_true, seg_pred, B, n, C, threshold, counts, s);
    else
        launch_counts<uint8_t, uint8_t, 3>(seg_true, seg_pred, B, n, C, threshold, counts, s);
    hipLaunchKernelGGL(class_iou_kernel, dim3((B * C + TPB - 1) / TPB), dim3(TPB), 0, s, (const unsigned long long *)counts, B, C, iou);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_eval_detection_metric_f32(const float *proposed, const float *gt, int32_t B, int32_t n_proposed, int32_t n_gt,
                                            float *out, void *stream) {
    const char *what = "eval_detection_metric";
    ML_REQUIRE(out && (proposed || n_proposed == 0) && (gt || n_gt == 0), "%s: null pointer", what);
    ML_REQUIRE(B >= 1 && n_proposed >= 0 && n_gt >= 0 && n_proposed < (1 << 24) && n_gt < (1 << 24), "%s: bad dims B=%d n=%d, %d", what,
               B, n_proposed, n_gt);
    hipLaunchKernelGGL(detection_metric_kernel, dim3(B), dim3(TPB), 0, (hipStream_t)stream, proposed, gt, B, n_proposed, n_gt, out);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_eval_confusion_f32(const float *cls_true, const float *cls_pred, const float *mask, int64_t N, int32_t C,
                                     float threshold, int64_t *counts, float *metrics, void *stream) {
    const char *what = "eval_confusion";
    ML_REQUIRE(cls_true && cls_pred && mask && counts && metrics, "%s: null pointer", what);
    ML_REQUIRE(N >= 1 && C >= 1 && N < (1ll << 40), "%s: bad dims N=%lld C=%d", what, (long long)N, C);
    hipStream_t s = (hipStream_t)stream;
    ML_HIP_OK(hipMemsetAsync(counts, 0, sizeof(int64_t) * 4, s), what);
    long long blocks = (N + TPB - 1) / TPB;
    blocks = blocks > 2048 ? 2048 : blocks;
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)blocks), dim3(TPB), 0, s, cls_true, cls_pred, mask, (long long)N, C, threshold,
                       (unsigned long long *)counts);
    hipLaunchKernelGGL(confusion_finish_kernel, dim3(1), dim3(1), 0, s, (const unsigned long long *)counts, metrics);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

// The per-thread bodies of the three evaluation kernels in CPU loops, every pointer in host memory.  Sections whose
// inputs are null are skipped; the pair section reads the areas the area section has just written.
extern "C" int ml_eval_reference_host(const int32_t *det, const int32_t *ins, const void *gt, const int32_t *pairs, int32_t P,
                                      const int32_t *pr_sem, const uint8_t *gt_sem, int32_t B, int32_t n, int32_t mh, int32_t mw,
                                      int32_t G, int32_t H, int32_t W, int32_t C, int64_t *out_area, int64_t *out_pairs,
                                      int64_t *out_sem) {
    const char *what = "eval_reference_host";
    if (gt) {
        const int e = check_masks(what, gt, B, G, H, W);
        if (e != ML_OK) return e;
        ML_REQUIRE(out_area, "%s: null pointer", what);
        const long long hw = (long long)H * W;
        for (long long m = 0; m < (long long)B * G; ++m) {
            out_area[m] = 0;
            for (int t = 0; t < HOST_THREADS; ++t) out_area[m] += area_thread((const uint8_t *)gt + m * hw, hw, t, HOST_THREADS);
        }
    }
    if (pairs || out_pairs) {
        const PairDims d = {P, B, n, mh, mw, G, H, W};
        const int e = check_pairs(what, det, ins, gt, out_area, pairs, out_pairs, d);
        if (e != ML_OK) return e;
        int32_t *m = new int32_t[(size_t)mh * mw];
        for (int p = 0; p < P; ++p) {
            const int32_t *pair = pairs + 3ll * p;
            if (!pair_valid(pair, d)) {
                out_pairs[2 * p] = out_pairs[2 * p + 1] = -1;
                continue;
            }
            const long long row = (long long)pair[0] * n + pair[1];
            const Box bx = pred_box(det + row * 6, H, W);
            uint32_t inter = 0, area = 0;
            if (bx.bw > 0 && bx.bh > 0) {
                for (int i = 0; i < mh * mw; ++i) m[i] = ins[row * mh * mw + i] > 0 ? ins[row * mh * mw + i] : 0;
                const uint8_t *g = (const uint8_t *)gt + ((long long)pair[0] * G + pair[2]) * H * W;
                for (int t = 0; t < HOST_THREADS; ++t) pair_thread(m, mh, mw, bx, g, W, t, HOST_THREADS, inter, area);
            }
            out_pairs[2 * p] = inter;
            out_pairs[2 * p + 1] = (int64_t)area + out_area[(long long)pair[0] * G + pair[2]] - inter;
        }
        delete[] m;
    }
    if (pr_sem || gt_sem) {
        ML_REQUIRE(H >= 1 && W >= 1, "%s: bad dims H=%d W=%d", what, H, W);
        const int e = check_counts(what, gt_sem, pr_sem, out_sem, B, (long long)H * W, C);
        if (e != ML_OK) return e;
        for (long long i = 0; i < 2ll * B * C; ++i) out_sem[i] = 0;
        host_counts<uint8_t, int32_t, 2>(gt_sem, pr_sem, B, (long long)H * W * C, C, 0.5f, out_sem);
    }
    return ML_OK;
}
