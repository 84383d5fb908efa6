// Backward of the resampling layers between the head outputs and the backbone taps, fp32:
//   crop_and_resize + MoldBatch (roi_crop_resize_kernel, detect.hip)        -> the gradient at the pyramid levels
//   resize_bilinear(align_corners=True) (bilinear_ac_kernel, pointwise.hip) -> the gradient at its source
//   tf.reduce_mean over H, W (global_mean_kernel, pointwise.hip)            -> the broadcast of dpool / (H W)
// All three layers are linear, so nothing of the forward is saved: shapes and the RoI tables are enough.
//
// GATHER form: a thread owns 4 channels of one INPUT-side pixel and adds the output samples that reach it in a fixed order
// (RoI slot j, then oy, then ox, ascending).  No float atomics, no zero-fill launch: every element is written, zeros
// included, and two launches give the same bits whatever output and workspace held.  Which samples reach a pixel: the
// candidate range of an axis is bounded analytically with one sample of margin on each side, then every candidate is tested
// with the forward kernel's own coordinate expressions (copied below, beside the kernel they come from).  The bound needs
// no bit-equal coordinates between forward and backward; the test decides.  This file is compiled without FP contraction and
// with correctly rounded division (Makefile): a coordinate is the float32 value of its expression, one rounding per
// operation in the order written, whatever the compiler would have fused.
#include "common.h"
#include "ranges.h"

namespace {

constexpr int TPB = 256;

inline unsigned grid_for(long long n) { return (unsigned)((n + TPB - 1) / TPB); }

// Samples o in [0, n) of an axis have the coordinate a + o*s.  -> the candidates [lo, hi] whose coordinate can lie in
// (p - 1, p + 1), one sample wider on each side.  rinv = 1/s, or 0 when every sample has the same coordinate (n == 1, s == 0
// or too small to invert): all samples are candidates then.  The products are clamped before the conversion to int.
__device__ __forceinline__ void candidates(float p, float a, float rinv, int n, int &lo, int &hi) {
    if (rinv == 0.f) { lo = 0; hi = n - 1; return; }
    const float t0 = (p - 1.f - a) * rinv, t1 = (p + 1.f - a) * rinv;
    const float tl = fminf(fmaxf(fminf(t0, t1), -1.f), (float)n);
    const float th = fminf(fmaxf(fmaxf(t0, t1), -1.f), (float)n);
    lo = max(0, (int)ceilf(tl) - 1);
    hi = min(n - 1, (int)floorf(th) + 1);
}
__device__ __forceinline__ float safe_rinv(float s, int n) { return (n > 1 && fabsf(s) > 1e-30f) ? 1.f / s : 0.f; }

// [lo, hi] -> the sub-range whose first and last sample have a non-zero weight (coordinates are monotonic in o, so the
// samples that reach a pixel are contiguous); empty (lo > hi) if none has
template <class Wt>
__device__ __forceinline__ void shrink(int &lo, int &hi, Wt weight) {
    while (lo <= hi && weight(lo) == 0.f) ++lo;
    while (hi > lo && weight(hi) == 0.f) --hi;
}

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, const f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// ------------------------------------------------------------------ crop_and_resize + MoldBatch, backward
// roi_crop_resize_kernel's sample (detect.hip): in = a + o*s, a = y1*(Hf-1) (n > 1) or 0.5*(y1+y2)*(Hf-1) (n == 1), s = hs or 0;
// outside [0, Hf-1] the sample is the extrapolation value 0 and has no gradient; inside, top = floor, bottom = ceil,
// f = in - top, weights (1 - f) and f.  -> the weight with which pixel p of the axis enters that sample
__device__ __forceinline__ float roi_axis_weight(float a, float s, int o, int p, float last) {
    const float in = a + (float)o * s;
    if (in < 0.f || in > last) return 0.f;
    const int t = (int)floorf(in), b = (int)ceilf(in);
    const float f = in - (float)t;
    float w = 0.f;
    if (t == p) w += 1.f - f;
    if (b == p) w += f;
    return w;
}

// A thread owns up to RG_ITEMS (pixel, 4-channel) items, 256 apart: a block owns 256 * ipt consecutive items of one image.
// ipt = 4 on the fine levels, where a pixel meets few samples and the RoI table in LDS is worth sharing; ipt = 1 on maps of at
// most RG_SMALL_MAP items, where every pixel meets most RoIs of its image with a dozen samples each: their few blocks are the
// launch's longest chains, so they are cut four times shorter and, in `start`, come first.
constexpr int RG_ITEMS = 4;
constexpr long long RG_SMALL_MAP = 1 << 16;
constexpr int RG_WX = 8;             // samples of a crop row that reach one pixel, kept in registers (more: recomputed per row)
constexpr int RG_CHUNK = 64;         // RoIs staged in LDS at a time

struct RgLevel {
    const float *dy;                 // [B, n_l, ch, cw, C]
    const float *add;                // [B, Hf, Wf, C] or null
    float *dx;                       // [B, Hf, Wf, C]
    int Hf, Wf, n_l, blocks_per_image, ipt;
};
struct RgArgs {
    RgLevel lv[ML_RESAMPLE_MAX_LEVELS];
    int start[ML_RESAMPLE_MAX_LEVELS];              // first block of every level; the LAST level comes first
    int n;
    const float *rows;
    const int *slots, *counts;
    int rs, roff, CV, cap, L, ch, cw;
    float img_h, img_w;
};
struct RgRoi { float ay, sy, ry, ax, sx, rx; };

__global__ void __launch_bounds__(TPB) roi_crop_resize_grad_kernel(const RgArgs A) {
    __shared__ RgRoi roi[RG_CHUNK];
    __shared__ int box[RG_CHUNK][4];                // pixel rows / columns a RoI's samples can reach, one pixel wider
    int level = A.n - 1;
    while (level > 0 && (int)blockIdx.x >= A.start[level - 1]) --level;
    const RgLevel &P = A.lv[level];
    const int id = blockIdx.x - A.start[level];
    const int b = id / P.blocks_per_image, blk = id - b * P.blocks_per_image;
    const int Hf = P.Hf, Wf = P.Wf, CV = A.CV, C = CV * 4, ch = A.ch, cw = A.cw;
    const float lasty = (float)(Hf - 1), lastx = (float)(Wf - 1);
    // rows j >= level_counts[b, level] are MoldBatch padding and are never read; neither is a row the tensor does not have
    const int cnt = min(A.counts[b * A.L + level], P.n_l);
    const long long items = (long long)Hf * Wf * CV;
    f32x4 acc[RG_ITEMS];
#pragma unroll
    for (int it = 0; it < RG_ITEMS; ++it) acc[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int base = 0; base < cnt; base += RG_CHUNK) {
        const int m = min(RG_CHUNK, cnt - base);
        if (base > 0) __syncthreads();
        if ((int)threadIdx.x < m) {
            const int slot = A.slots[((long long)b * A.L + level) * A.cap + base + threadIdx.x];
            RgRoi q = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int bx[4] = {1, 0, 1, 0};                                   // empty: reaches no pixel
            if (slot >= 0 && slot < A.cap) {
                const float *r = A.rows + ((long long)b * A.cap + slot) * A.rs + A.roff;
                // NormalizeBoxes(shape=image H,W) and the sample spacing, as the forward writes them
                const float cx = r[0], cy = r[1], bw = r[2], bh = r[3];
                const float x1 = (cx - bw / 2.f) / A.img_w, y1 = (cy - bh / 2.f) / A.img_h;
                const float x2 = (cx + bw / 2.f) / A.img_w, y2 = (cy + bh / 2.f) / A.img_h;
                const float hs = ch > 1 ? (y2 - y1) * (float)(Hf - 1) / (float)(ch - 1) : 0.f;
                const float ws = cw > 1 ? (x2 - x1) * (float)(Wf - 1) / (float)(cw - 1) : 0.f;
                q.ay = ch > 1 ? y1 * (float)(Hf - 1) : 0.5f * (y1 + y2) * (float)(Hf - 1);
                q.ax = cw > 1 ? x1 * (float)(Wf - 1) : 0.5f * (x1 + x2) * (float)(Wf - 1);
                q.sy = hs; q.sx = ws;
                q.ry = safe_rinv(hs, ch); q.rx = safe_rinv(ws, cw);
                const float ey = q.ay + (float)(ch - 1) * hs, ex = q.ax + (float)(cw - 1) * ws;
                bx[0] = (int)floorf(fminf(fmaxf(fminf(q.ay, ey), -2.f), lasty + 2.f)) - 1;
                bx[1] = (int)ceilf(fminf(fmaxf(fmaxf(q.ay, ey), -2.f), lasty + 2.f)) + 1;
                bx[2] = (int)floorf(fminf(fmaxf(fminf(q.ax, ex), -2.f), lastx + 2.f)) - 1;
                bx[3] = (int)ceilf(fminf(fmaxf(fmaxf(q.ax, ex), -2.f), lastx + 2.f)) + 1;
            }
            roi[threadIdx.x] = q;
#pragma unroll
            for (int k = 0; k < 4; ++k) box[threadIdx.x][k] = bx[k];
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < RG_ITEMS; ++it) {
            const long long item = ((long long)blk * P.ipt + it) * TPB + threadIdx.x;
            if (it >= P.ipt || item >= items) continue;
            const int c = (int)(item % CV) * 4;
            const int pix = (int)(item / CV);
            const int y = pix / Wf, x = pix - y * Wf;
            for (int k = 0; k < m; ++k) {
                if (y < box[k][0] || y > box[k][1] || x < box[k][2] || x > box[k][3]) continue;
                const RgRoi q = roi[k];
                int ylo, yhi, xlo, xhi;
                candidates((float)y, q.ay, q.ry, ch, ylo, yhi);
                shrink(ylo, yhi, [&](int o) { return roi_axis_weight(q.ay, q.sy, o, y, lasty); });
                if (ylo > yhi) continue;
                candidates((float)x, q.ax, q.rx, cw, xlo, xhi);
                shrink(xlo, xhi, [&](int o) { return roi_axis_weight(q.ax, q.sx, o, x, lastx); });
                if (xlo > xhi) continue;
                const float *dy = P.dy + ((long long)b * P.n_l + base + k) * ch * cw * C + c;
                const int nx = xhi - xlo + 1;
                if (nx <= RG_WX) {          // the usual case: the row's weights once, in registers (the same products, the same order)
                    float wxs[RG_WX];
#pragma unroll
                    for (int i = 0; i < RG_WX; ++i) wxs[i] = i < nx ? roi_axis_weight(q.ax, q.sx, xlo + i, x, lastx) : 0.f;
                    for (int oy = ylo; oy <= yhi; ++oy) {
                        const float wy = roi_axis_weight(q.ay, q.sy, oy, y, lasty);
                        if (wy == 0.f) continue;
#pragma unroll
                        for (int i = 0; i < RG_WX; ++i) {
                            if (i >= nx || wxs[i] == 0.f) continue;
                            acc[it] += (wy * wxs[i]) * ld4(dy + ((long long)oy * cw + xlo + i) * C);
                        }
                    }
                    continue;
                }
                for (int oy = ylo; oy <= yhi; ++oy) {
                    const float wy = roi_axis_weight(q.ay, q.sy, oy, y, lasty);
                    if (wy == 0.f) continue;
                    for (int ox = xlo; ox <= xhi; ++ox) {
                        const float wx = roi_axis_weight(q.ax, q.sx, ox, x, lastx);
                        if (wx == 0.f) continue;
                        acc[it] += (wy * wx) * ld4(dy + ((long long)oy * cw + ox) * C);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int it = 0; it < RG_ITEMS; ++it) {
        const long long item = ((long long)blk * P.ipt + it) * TPB + threadIdx.x;
        if (it >= P.ipt || item >= items) continue;
        const long long off = ((long long)b * Hf * Wf) * C + item * 4;
        f32x4 v = acc[it];
        if (P.add) v = ld4(P.add + off) + v;
        st4(P.dx + off, v);
    }
}

// ------------------------------------------------------------------ resize_bilinear(align_corners=True), backward
// bilinear_ac_kernel's sample (pointwise.hip, Elt<float>): f = o*s, i0 = max(floor f, 0), i1 = min(ceil f, n_in - 1),
// t = fma(o, s, -floor f), weights (1 - t) and t; where i0 == i1 the forward's top + (bot - top)*t is the pixel itself.
__device__ __forceinline__ float resize_axis_weight(float s, int o, int p, int n_in) {
    const float f = (float)o * s;
    const float fl = floorf(f);
    const int i0 = max((int)fl, 0), i1 = min((int)ceilf(f), n_in - 1);
    if (i0 == i1) return i0 == p ? 1.f : 0.f;
    const float t = fmaf((float)o, s, -fl);
    float w = 0.f;
    if (i0 == p) w += 1.f - t;
    if (i1 == p) w += t;
    return w;
}

__global__ void __launch_bounds__(TPB)
bilinear_ac_grad_kernel(const float *__restrict__ dy, const float *add, float *dx, int H, int W, int CV, int Ho, int Wo,
                        float sy, float sx, float ry, float rx, int dy_cs, int dy_co, long long total) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % CV) * 4;
    long long pix = idx / CV;
    const int x = (int)(pix % W); pix /= W;
    const int y = (int)(pix % H);
    const int b = (int)(pix / H);
    int ylo, yhi, xlo, xhi;
    candidates((float)y, 0.f, ry, Ho, ylo, yhi);
    shrink(ylo, yhi, [&](int o) { return resize_axis_weight(sy, o, y, H); });
    candidates((float)x, 0.f, rx, Wo, xlo, xhi);
    shrink(xlo, xhi, [&](int o) { return resize_axis_weight(sx, o, x, W); });
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (xlo <= xhi) {
        const float *src = dy + (long long)b * Ho * Wo * dy_cs + dy_co + c;
        for (int oy = ylo; oy <= yhi; ++oy) {
            const float wy = resize_axis_weight(sy, oy, y, H);
            if (wy == 0.f) continue;
            for (int ox = xlo; ox <= xhi; ++ox) {
                const float wx = resize_axis_weight(sx, ox, x, W);
                if (wx == 0.f) continue;
                acc += (wy * wx) * ld4(src + ((long long)oy * Wo + ox) * dy_cs);
            }
        }
    }
    if (add) acc = ld4(add + idx * 4) + acc;
    st4(dx + idx * 4, acc);
}

// A 1x1 source (ASPP's pooled branch): every output pixel is the source pixel, dx[b, c] = sum over all of dy[b, :, :, c].
// Block = RS_Q channel lanes x 256 / RS_Q pixel groups over one slice of the pixels; fp64 sums, a thread's pixels in index
// order, then the groups in index order -> ws[(b*S + s)*C + c]; the fold adds the S slices in index order.
constexpr int RS_Q = 16, RS_G = TPB / RS_Q, RS_SLICE = 256, RS_MAX_SLICES = 64;

__global__ void __launch_bounds__(TPB)
broadcast_grad_partial_kernel(const float *__restrict__ dy, double *__restrict__ ws, int HW, int CV, int dy_cs, int dy_co,
                              int S, int slice) {
    __shared__ double red[RS_G][RS_Q][4];
    const int q = threadIdx.x & (RS_Q - 1), g = threadIdx.x / RS_Q;
    const int cv = blockIdx.x * RS_Q + q, s = blockIdx.y, b = blockIdx.z;
    double acc[4] = {0, 0, 0, 0};
    if (cv < CV) {
        const float *p = dy + (long long)b * HW * dy_cs + dy_co + cv * 4;
        const int end = min(HW, (s + 1) * slice);
        for (int i = s * slice + g; i < end; i += RS_G) {
            const f32x4 v = ld4(p + (long long)i * dy_cs);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += (double)v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[g][q][e] = acc[e];
    __syncthreads();
    if (g == 0 && cv < CV) {
        double *o = ws + ((long long)b * S + s) * CV * 4 + cv * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double t = 0;
#pragma unroll
            for (int k = 0; k < RS_G; ++k) t += red[k][q][e];
            o[e] = t;
        }
    }
}

__global__ void __launch_bounds__(TPB)
broadcast_grad_fold_kernel(const double *__restrict__ ws, const float *add, float *dx, int CV, int S, int total) {
    const int idx = blockIdx.x * TPB + threadIdx.x;          // (b, cv)
    if (idx >= total) return;
    const int b = idx / CV, cv = idx - b * CV;
    double t[4] = {0, 0, 0, 0};
    for (int s = 0; s < S; ++s) {
        const double *p = ws + ((long long)b * S + s) * CV * 4 + cv * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] += p[e];
    }
    f32x4 v = {(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
    if (add) v = ld4(add + (long long)idx * 4) + v;
    st4(dx + (long long)idx * 4, v);
}

inline int rs_slices(long long HW) {
    const long long S = (HW + RS_SLICE - 1) / RS_SLICE;
    return (int)(S < RS_MAX_SLICES ? S : RS_MAX_SLICES);
}

// ------------------------------------------------------------------ tf.reduce_mean over H, W, backward
__global__ void __launch_bounds__(TPB)
global_mean_grad_kernel(const float *__restrict__ dpool, const float *add, float *dx, int HW, int CV, float n, long long total) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= total) return;
    const int cv = (int)(idx % CV);
    const int b = (int)(idx / ((long long)CV * HW));
    f32x4 v = ld4(dpool + ((long long)b * CV + cv) * 4) / n;
    if (add) v = ld4(add + idx * 4) + v;
    st4(dx + idx * 4, v);
}

}  // namespace

extern "C" int ml_roi_crop_resize_grad_f32(const ml_roi_grad_level *levels, int32_t n_levels, const float *rows,
                                           int32_t row_stride, int32_t row_off, const int32_t *level_slots,
                                           const int32_t *level_counts, int32_t B, int32_t C, int32_t cap, int32_t L,
                                           int32_t ch, int32_t cw, float img_h, float img_w, void *stream) {
    const char *what = "roi_crop_grad";
    ML_REQUIRE(levels && rows && level_slots && level_counts, "%s: null pointer", what);
    ML_REQUIRE(n_levels >= 1 && n_levels <= ML_RESAMPLE_MAX_LEVELS && n_levels <= L, "%s: need 1..%d levels, at most L", what,
               ML_RESAMPLE_MAX_LEVELS);
    ML_REQUIRE(row_off >= 0 && row_off + 6 <= row_stride, "%s: rows must hold 6 columns from row_off", what);
    ML_REQUIRE(B > 0 && cap > 0 && ch > 0 && cw > 0 && C > 0, "%s: bad dims", what);
    ML_REQUIRE(C % 4 == 0, "%s: C (%d) must be a multiple of 4 (16-byte accesses)", what, C);
    RgArgs A;
    long long blocks = 0;
    for (int i = n_levels - 1; i >= 0; --i) {
        const ml_roi_grad_level &d = levels[i];
        ML_REQUIRE(d.dy && d.dx, "%s: level %d: null pointer", what, i);
        ML_REQUIRE(d.Hf > 0 && d.Wf > 0 && d.n_l > 0 && d.n_l <= cap, "%s: level %d: bad dims (0 < n_l <= cap)", what, i);
        ML_REQUIRE(ml_aligned16(d.dy) && ml_aligned16(d.dx) && ml_aligned16(d.add), "%s: level %d: 16-byte alignment", what, i);
        const long long px = (long long)d.Hf * d.Wf;
        ML_REQUIRE((long long)B * px < (1ll << 31), "%s: level %d: too many pixels", what, i);
        const long long dx_bytes = (long long)B * px * C * 4, dy_bytes = (long long)B * d.n_l * ch * cw * C * 4;
        ML_REQUIRE(!ml_ranges_overlap(d.dx, dx_bytes, d.dy, dy_bytes), "%s: level %d: dx may not overlap dy", what, i);
        ML_REQUIRE(ml_add_or_disjoint(d.dx, d.add, dx_bytes),
                   "%s: level %d: dx may be add itself, not a shifted view of it", what, i);
        RgLevel &P = A.lv[i];
        P.dy = d.dy; P.add = d.add; P.dx = d.dx; P.Hf = d.Hf; P.Wf = d.Wf; P.n_l = d.n_l;
        P.ipt = px * (C / 4) <= RG_SMALL_MAP ? 1 : RG_ITEMS;
        P.blocks_per_image = (int)((px * (C / 4) + TPB * P.ipt - 1) / (TPB * P.ipt));
        A.start[i] = (int)blocks;
        blocks += (long long)B * P.blocks_per_image;
        ML_REQUIRE(blocks < (1ll << 31), "%s: grid too large", what);
    }
    A.n = n_levels;
    A.rows = rows; A.slots = level_slots; A.counts = level_counts;
    A.rs = row_stride; A.roff = row_off; A.CV = C / 4; A.cap = cap; A.L = L; A.ch = ch; A.cw = cw;
    A.img_h = img_h; A.img_w = img_w;
    hipLaunchKernelGGL(roi_crop_resize_grad_kernel, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, A);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int64_t ml_resize_bilinear_ac_grad_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho,
                                                              int32_t Wo) {
    if (H != 1 || W != 1 || B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return 0;
    return (int64_t)B * rs_slices((long long)Ho * Wo) * C * (int64_t)sizeof(double);
}

extern "C" int ml_resize_bilinear_ac_grad_f32(const float *dy, const float *add, float *dx, int32_t B, int32_t H, int32_t W,
                                              int32_t C, int32_t Ho, int32_t Wo, int32_t dy_cstride, int32_t dy_coff,
                                              void *workspace, int64_t workspace_bytes, void *stream) {
    const char *what = "resize_bilinear_grad";
    ML_REQUIRE(dy && dx, "%s: null pointer", what);
    ML_REQUIRE(B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && C > 0, "%s: bad dims", what);
    ML_REQUIRE(C % 4 == 0, "%s: C (%d) must be a multiple of 4 (16-byte accesses)", what, C);
    ML_REQUIRE(dy_cstride % 4 == 0 && dy_coff % 4 == 0 && dy_coff >= 0, "%s: channel stride / offset must be multiples of 4", what);
    ML_REQUIRE(dy_coff + C <= dy_cstride, "%s: slice exceeds buffer", what);
    ML_REQUIRE(ml_aligned16(dy) && ml_aligned16(dx) && ml_aligned16(add), "%s: pointers must be 16-byte aligned", what);
    ML_REQUIRE((long long)B * H * W < (1ll << 31) && (long long)B * Ho * Wo < (1ll << 31), "%s: too many pixels", what);
    const long long dx_bytes = (long long)B * H * W * C * 4, dy_bytes = (long long)B * Ho * Wo * dy_cstride * 4;
    ML_REQUIRE(!ml_ranges_overlap(dx, dx_bytes, dy, dy_bytes), "%s: dx may not overlap dy", what);
    ML_REQUIRE(ml_add_or_disjoint(dx, add, dx_bytes), "%s: dx may be add itself, not a shifted view of it", what);
    hipStream_t s = (hipStream_t)stream;
    const int CV = C / 4;
    if (H == 1 && W == 1) {
        const int HW = Ho * Wo, S = rs_slices(HW), slice = (HW + S - 1) / S;
        ML_REQUIRE(workspace && (((uintptr_t)workspace) & 15) == 0 &&
                   workspace_bytes >= ml_resize_bilinear_ac_grad_workspace_bytes(B, H, W, C, Ho, Wo),
                   "%s: the 1x1 source needs a workspace of ml_resize_bilinear_ac_grad_workspace_bytes", what);
        ML_REQUIRE(B < 65536, "%s: B too large", what);
        double *ws = reinterpret_cast<double *>(workspace);
        hipLaunchKernelGGL(broadcast_grad_partial_kernel, dim3((CV + RS_Q - 1) / RS_Q, S, B), dim3(TPB), 0, s, dy, ws, HW, CV,
                           dy_cstride, dy_coff, S, slice);
        hipLaunchKernelGGL(broadcast_grad_fold_kernel, dim3(grid_for((long long)B * CV)), dim3(TPB), 0, s, ws, add, dx, CV, S,
                           B * CV);
        ML_CHECK_LAUNCH(what);
        return ML_OK;
    }
    // the forward launcher's scales
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
    const float sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const float ry = (Ho > 1 && sy > 0.f) ? 1.f / sy : 0.f, rx = (Wo > 1 && sx > 0.f) ? 1.f / sx : 0.f;
    const long long total = (long long)B * H * W * CV;
    ML_REQUIRE(total < (1ll << 31) * TPB, "%s: grid too large", what);
    hipLaunchKernelGGL(bilinear_ac_grad_kernel, dim3(grid_for(total)), dim3(TPB), 0, s, dy, add, dx, H, W, CV, Ho, Wo, sy, sx, ry,
                       rx, dy_cstride, dy_coff, total);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_global_mean_grad_f32(const float *dpool, const float *add, float *dx, int32_t B, int32_t HW, int32_t C,
                                       void *stream) {
    const char *what = "global_mean_grad";
    ML_REQUIRE(dpool && dx && B > 0 && HW > 0 && C > 0, "%s: bad arguments", what);
    ML_REQUIRE(C % 4 == 0, "%s: C (%d) must be a multiple of 4 (16-byte accesses)", what, C);
    ML_REQUIRE(ml_aligned16(dpool) && ml_aligned16(dx) && ml_aligned16(add), "%s: pointers must be 16-byte aligned", what);
    const long long dx_bytes = (long long)B * HW * C * 4;
    ML_REQUIRE(!ml_ranges_overlap(dx, dx_bytes, dpool, (long long)B * C * 4), "%s: dx may not overlap dpool", what);
    ML_REQUIRE(ml_add_or_disjoint(dx, add, dx_bytes), "%s: dx may be add itself, not a shifted view of it", what);
    const long long total = (long long)B * HW * (C / 4);
    ML_REQUIRE(total < (1ll << 31) * TPB, "%s: grid too large", what);
    hipLaunchKernelGGL(global_mean_grad_kernel, dim3(grid_for(total)), dim3(TPB), 0, (hipStream_t)stream, dpool, add, dx, HW, C / 4,
                       (float)HW, total);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}
