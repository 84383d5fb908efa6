// One axis of cv2.resize(INTER_LINEAR), restated from OpenCV's plain C++ path: shared by evaluate.hip (the pasted
// prediction masks) and cv_resize.hip (the generator's resizes).  OpenCV parity is unpinned: this text, not a run of
// OpenCV, is the contract (include/masklab_hip.h, "Evaluation" and "Generator resizes").
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// (d + 0.5) * scale - 0.5 must stay a multiply and a subtract: no FMA, here and in everything that includes this header
#pragma clang fp contract(off)

namespace cvr {

struct Tap { int s0, s1; float w0, w1; };

__host__ __device__ inline double axis_scale(int dst, int src) { return 1.0 / ((double)dst / (double)src); }

// destination index d -> two source indices and their float32 weights
__host__ __device__ inline Tap axis_tap(int d, double scale, int src) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    return {s, s + 1 < src ? s + 1 : src - 1, 1.f - f, f};
}

}  // namespace cvr
