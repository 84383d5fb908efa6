// CropAndPadMask's arithmetic (reference engine/layers/misc.py:358-401), shared by the kernels that paste instance
// masks (deploy.hip) and those that recompute the pasted values without a canvas (deploy.hip's summary, visualize.hip).
// One definition, so every consumer is bit-identical to ml_crop_pad_mask_f32.
#pragma once
#include "common.h"
#pragma clang fp contract(off)

namespace {

// ---- CropAndPadMask: threshold = max(conf) > 50 ? 50 : -100 (misc.py:371-374), one block
__global__ void __launch_bounds__(256) conf_threshold_kernel(const int32_t *__restrict__ det, int rows, int32_t *thr) {
    __shared__ int red[256];
    int m = INT32_MIN;
    for (int i = threadIdx.x; i < rows; i += 256) m = max(m, det[i * 6 + 5]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *thr = red[0] > 50 ? 50 : -100;
}

// Where CropAndPadMask pastes an instance (misc.py:377-398): box = max(box, 1) elementwise, corners ceil(c -+ size/2)
// clipped to the canvas; rows below the confidence threshold and zero-sized boxes paste nothing (empty box).
struct PasteBox {
    int xmin, xmax, ymin, ymax;      // [xmin, xmax) x [ymin, ymax); empty when nothing is pasted
    float sy, sx;                    // mask rows / columns per canvas row / column (align_corners)
};
__device__ __forceinline__ PasteBox paste_box(const int32_t *d, int thr, int mh, int mw, int H, int W) {
    PasteBox p = {0, 0, 0, 0, 0.f, 0.f};
    if (d[5] < thr) return p;
    const float cx = (float)max(d[0], 1), cy = (float)max(d[1], 1), w = (float)max(d[2], 1), h = (float)max(d[3], 1);
    p.xmin = min(max((int)ceilf(cx - w / 2.f), 0), W); p.xmax = min(max((int)ceilf(cx + w / 2.f), 0), W);
    p.ymin = min(max((int)ceilf(cy - h / 2.f), 0), H); p.ymax = min(max((int)ceilf(cy + h / 2.f), 0), H);
    const int oh = p.ymax - p.ymin, ow = p.xmax - p.xmin;
    p.sy = oh > 1 ? (float)(mh - 1) / (float)(oh - 1) : 0.f;
    p.sx = ow > 1 ? (float)(mw - 1) / (float)(ow - 1) : 0.f;
    if (oh <= 0 || ow <= 0) p.xmax = p.xmin = p.ymax = p.ymin = 0;
    return p;
}
// value of canvas pixel (y, x): the mh x mw int mask resized bilinear (align_corners) to the box; 0 outside it
__device__ __forceinline__ float paste_value(const PasteBox &p, const int32_t *m, int mh, int mw, int y, int x) {
    if (!(y >= p.ymin && y < p.ymax && x >= p.xmin && x < p.xmax)) return 0.f;
    const float fy = (float)(y - p.ymin) * p.sy, fx = (float)(x - p.xmin) * p.sx;
    const float fly = floorf(fy), flx = floorf(fx);
    const int y0 = max((int)fly, 0), x0 = max((int)flx, 0);
    const int y1 = min((int)ceilf(fy), mh - 1), x1 = min((int)ceilf(fx), mw - 1);
    const float ty = fy - fly, tx = fx - flx;
    const float tl = (float)m[y0 * mw + x0], tr = (float)m[y0 * mw + x1];
    const float bl = (float)m[y1 * mw + x0], br = (float)m[y1 * mw + x1];
    const float top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx;
    return top + (bot - top) * ty;
}

}  // namespace
