// The parts of the slice-sum scheme that the weight gradients share (conv_grad.hip, dwconv_grad.hip, deconv_out_grad.hip;
// "One definition: slice sums").  Their launchers' range tests come with it from ranges.h.
//
// The scheme: the pixel axis of a problem is cut into slices that are a function of its geometry alone; a block writes the
// fp32 partial of its slice into the launch's workspace (no float atomics); a finish kernel adds an element's partials in
// ascending slice order in fp64 and rounds once.  Slice constants, problem structs, partial kernels, finish kernels and the
// per-launch checks stay in the files: only what was the same text in each of them lives here.  Plain functions, no state.
#pragma once
#include "common.h"
#include "ranges.h"

inline long long ml_align256(long long v) { return (v + 255) & ~255ll; }

// pixels per slice: clamp(round_up(ceil(P / parts), round), lo, hi); hi = 0: no upper clamp
inline long long ml_slice_pixels(long long P, long long parts, long long round, long long lo, long long hi) {
    const long long sp = ((P + parts - 1) / parts + round - 1) / round * round;
    return sp < lo ? lo : (hi && sp > hi ? hi : sp);
}

// what a *_plan entry gives back: each pointer is optional
inline void ml_plan_out(int slices, int slice_pixels, long long bytes, int32_t *o_slices, int32_t *o_slice_pixels,
                        int64_t *o_bytes) {
    if (o_slices) *o_slices = slices;
    if (o_slice_pixels) *o_slice_pixels = slice_pixels;
    if (o_bytes) *o_bytes = bytes;
}

// problem i's partials: `bytes` of the launch's workspace [base, base + size) from `used` on, which moves past them.
// -> their first byte, or nullptr with the error set
inline float *ml_carve_partials(const char *what, int i, void *base, long long size, long long &used, long long bytes) {
    if (used + bytes > size) {
        ml_set_error("%s: the workspace is too small: problem %d needs %lld bytes at offset %lld of %lld", what, i, bytes, used,
                     size);
        return nullptr;
    }
    float *p = reinterpret_cast<float *>((char *)base + used);
    used += bytes;
    return p;
}

// src[0], src[pitch], ... src[(slices - 1) pitch] added in ascending slice order in fp64; sixteen loads are in flight at a
// time (one load per addition would leave the sum waiting on each)
__device__ __forceinline__ double ml_sum_slices_f64(const float *src, long long pitch, int slices) {
    double t = 0.0;
    int s = 0;
    for (; s + 16 <= slices; s += 16) {
        float part[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) part[j] = src[(long long)(s + j) * pitch];
#pragma unroll
        for (int j = 0; j < 16; ++j) t += (double)part[j];
    }
    for (; s < slices; ++s) t += (double)src[(long long)s * pitch];
    return t;
}
