// CalculateIOU.call (engine/layers/detection.py:391-422) for one pair of (cx, cy, w, h) boxes in float32, shared by
// evaluate.hip (DetectionIOUMetric) and train_targets.hip (AssignBoxes, AssignMasks).  Every operation is rounded on
// its own, as NumPy evaluates oracle/metrics.py::calculate_iou: the including file keeps FP contraction off.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

// NumPy's minimum / maximum hand a NaN on; fminf / fmaxf would drop it.
__host__ __device__ inline float np_min(float a, float b) { return (a != a || a < b) ? a : b; }
__host__ __device__ inline float np_max(float a, float b) { return (a != a || a > b) ? a : b; }

// a: a row of the layer's first input (aa_boxes), g: a row of its second (bb_boxes)
__host__ __device__ inline float box_iou(const float *a, const float *g) {
    const float areas = g[2] * g[3] + a[2] * a[3];
    const float ay1 = a[1] - a[3] / 2.f, ax1 = a[0] - a[2] / 2.f, ay2 = a[1] + a[3] / 2.f, ax2 = a[0] + a[2] / 2.f;
    const float gy1 = g[1] - g[3] / 2.f, gx1 = g[0] - g[2] / 2.f, gy2 = g[1] + g[3] / 2.f, gx2 = g[0] + g[2] / 2.f;
    const float in_w = np_max(0.f, np_min(gx2, ax2) - np_max(gx1, ax1));
    const float in_h = np_max(0.f, np_min(gy2, ay2) - np_max(gy1, ay1));
    const float inter = in_w * in_h;
    return inter / ((areas - inter) + 1e-5f);
}
