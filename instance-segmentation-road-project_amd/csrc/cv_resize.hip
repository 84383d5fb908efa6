// The reference generator's resizes (engine/utils/generator/masklab.py: cv2.resize(x, (tw, th)), default INTER_LINEAR) as
// gather kernels over uint8 planes.  The contract is in include/masklab_hip.h ("Generator resizes"); what matters here:
//
//   * OpenCV parity is unpinned: the arithmetic is cv2.resize restated from OpenCV's plain C++ path (the axis taps of
//     cv_resize.h; the fixed-point uint8 path; the float64 path; the switch to INTER_AREA at exactly 2x on both axes).
//     tests/generator_ref.py restates the same text in NumPy and the results are equal byte for byte.
//   * float arithmetic that decides a bit runs with FP contraction OFF.
//   * grid = (row chunk, output row, plane): the y taps and the skip test have one value per block (every
//     thread computes them; nothing is shared); thread t makes the 4 consecutive elements of
//     the flattened ow*C row that share one aligned 4-byte (uint8) / 16-byte (float32) destination word and stores them as
//     one word, element by element at a ragged head or tail.  Sources are gathered byte by byte straight from global memory.
//   * no workspace, no host read, no atomics; every output element is written exactly once.
//   * the per-thread body is a __host__ __device__ function of (plane, row, thread): ml_cv_resize_reference_host runs it in
//     CPU loops, so the CPU tests hold this very code to NumPy.
#include "common.h"
#include "cv_resize.h"

#pragma clang fp contract(off)

namespace {
namespace cvk {

using cvr::Tap;

constexpr int TPB = 256;
constexpr int PER_THREAD = 4;
constexpr int MAX_GRID_YZ = 65535;
enum { FIXED = 0, ROUND = 1 };            // the uint8 fixed-point path; the float64 path + np.round

struct Geo {
    int H, W, C, oh, ow;
    int area;                             // H == 2*oh && W == 2*ow: cv::resize turns INTER_LINEAR into INTER_AREA
    double sy, sx;
};

Geo make_geo(int H, int W, int C, int oh, int ow) {
    return {H, W, C, oh, ow, H == 2 * oh && W == 2 * ow, cvr::axis_scale(oh, H), cvr::axis_scale(ow, W)};
}

// (short)cvRound(w * 2048): round half to even; w is in [0, 1]
__host__ __device__ inline int coef(float w) { return (int)(short)rintf(w * 2048.f); }

struct alignas(16) F4 { float v[4]; };

template <typename OUT> struct Word;
template <> struct Word<uint8_t> {
    __host__ __device__ static void store(uint8_t *p, const int (&v)[4]) {
        *reinterpret_cast<uint32_t *>(p) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    }
};
template <> struct Word<float> {
    __host__ __device__ static void store(float *p, const int (&v)[4]) {
        *reinterpret_cast<F4 *>(p) = F4{{(float)v[0], (float)v[1], (float)v[2], (float)v[3]}};
    }
};

// The values of the source taps (r0, r1: the two source rows; i0, i1: the two byte offsets inside a row) -> 0..255.
template <int MODE>
__host__ __device__ inline int linear_value(const uint8_t *r0, const uint8_t *r1, int i0, int i1, const Tap &ty, const Tap &tx) {
    const int s00 = r0[i0], s01 = r0[i1], s10 = r1[i0], s11 = r1[i1];
    if (MODE == FIXED) {
        const int a0 = coef(tx.w0), a1 = coef(tx.w1), b0 = coef(ty.w0), b1 = coef(ty.w1);
        const int h0 = s00 * a0 + s01 * a1, h1 = s10 * a0 + s11 * a1;
        return (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
    }
    const double h0 = (double)s00 * (double)tx.w0 + (double)s01 * (double)tx.w1;
    const double h1 = (double)s10 * (double)tx.w0 + (double)s11 * (double)tx.w1;
    return (int)rint(h0 * (double)ty.w0 + h1 * (double)ty.w1);
}

template <int MODE>
__host__ __device__ inline int area_value(const uint8_t *r0, const uint8_t *r1, int i0, int i1) {
    const int sum = r0[i0] + r0[i1] + r1[i0] + r1[i1];
    return MODE == FIXED ? (sum + 2) >> 2 : (int)rint((double)sum * 0.25);
}

// Thread t of output row y of one plane.  `row` is the row's first output element; `fill` (uniform per plane) writes -1
// bytes without reading the source.  Elements [4t - a, 4t - a + 4) of the row, a = the row's offset inside its aligned word.
template <int MODE, typename OUT>
__host__ __device__ inline void row_thread(const uint8_t *plane, OUT *row, const Geo &g, int y, long long t, bool fill) {
    const long long rowlen = (long long)g.ow * g.C;
    const int a = (int)(((uintptr_t)row / sizeof(OUT)) & (PER_THREAD - 1));
    const long long e0 = t * PER_THREAD - a;
    if (e0 >= rowlen) return;
    const long long first = e0 < 0 ? 0 : e0, last = e0 + PER_THREAD < rowlen ? e0 + PER_THREAD : rowlen;
    int v[PER_THREAD] = {0xFF, 0xFF, 0xFF, 0xFF};
    if (!fill) {
        int x = (int)(first / g.C), c = (int)(first - (long long)x * g.C);
        const long long pitch = (long long)g.W * g.C;
        if (g.area) {
            const uint8_t *r0 = plane + 2ll * y * pitch, *r1 = r0 + pitch;
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                if (e0 + k < first || e0 + k >= last) continue;
                v[k] = area_value<MODE>(r0, r1, 2 * x * g.C + c, (2 * x + 1) * g.C + c);
                if (++c == g.C) { c = 0; ++x; }
            }
        } else {
            const Tap ty = cvr::axis_tap(y, g.sy, g.H);
            const uint8_t *r0 = plane + ty.s0 * pitch, *r1 = plane + ty.s1 * pitch;
            Tap tx = cvr::axis_tap(x, g.sx, g.W);
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                if (e0 + k < first || e0 + k >= last) continue;
                v[k] = linear_value<MODE>(r0, r1, tx.s0 * g.C + c, tx.s1 * g.C + c, ty, tx);
                if (++c == g.C && e0 + k + 1 < last) { c = 0; tx = cvr::axis_tap(++x, g.sx, g.W); }
            }
        }
    }
    if (e0 >= 0 && e0 + PER_THREAD <= rowlen) {
        Word<OUT>::store(row + e0, v);
    } else {
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k)
            if (e0 + k >= first && e0 + k < last) row[e0 + k] = (OUT)v[k];
    }
}

template <int MODE, typename OUT>
__global__ __launch_bounds__(TPB) void resize_kernel(const uint8_t *src, OUT *dst, Geo g, int skip_minus_one) {
    const long long p = blockIdx.z;
    const int y = blockIdx.y;
    const uint8_t *plane = src + p * ((long long)g.H * g.W * g.C);
    OUT *row = dst + (p * g.oh + y) * ((long long)g.ow * g.C);
    const bool fill = skip_minus_one && plane[0] == 0xFF;
    row_thread<MODE, OUT>(plane, row, g, y, (long long)blockIdx.x * TPB + threadIdx.x, fill);
}

// threads a row needs: its elements plus the up to 3 in front of the first one in its aligned word
inline long long row_threads(const Geo &g) { return ((long long)g.ow * g.C + 2 * (PER_THREAD - 1)) / PER_THREAD; }

template <int MODE, typename OUT>
void launch(const uint8_t *src, OUT *dst, long long planes, const Geo &g, int skip, hipStream_t s) {
    const unsigned chunks = (unsigned)((row_threads(g) + TPB - 1) / TPB);
    const long long in_plane = (long long)g.H * g.W * g.C, out_plane = (long long)g.oh * g.ow * g.C;
    for (long long p0 = 0; p0 < planes; p0 += MAX_GRID_YZ) {
        const long long np_ = planes - p0 < MAX_GRID_YZ ? planes - p0 : MAX_GRID_YZ;
        hipLaunchKernelGGL((resize_kernel<MODE, OUT>), dim3(chunks, g.oh, (unsigned)np_), dim3(TPB), 0, s, src + p0 * in_plane,
                           dst + p0 * out_plane, g, skip);
    }
}

template <int MODE, typename OUT>
void host_loop(const uint8_t *src, OUT *dst, long long planes, const Geo &g, int skip) {
    const long long in_plane = (long long)g.H * g.W * g.C, rowlen = (long long)g.ow * g.C, T = row_threads(g);
    for (long long p = 0; p < planes; ++p) {
        const uint8_t *plane = src + p * in_plane;
        const bool fill = skip && plane[0] == 0xFF;
        for (int y = 0; y < g.oh; ++y)
            for (long long t = 0; t < T; ++t) row_thread<MODE, OUT>(plane, dst + (p * g.oh + y) * rowlen, g, y, t, fill);
    }
}

int check(const char *what, const void *src, const void *dst, long long planes, int H, int W, int C, int oh, int ow) {
    ML_REQUIRE(planes >= 0 && H >= 1 && W >= 1 && C >= 1 && oh >= 1 && ow >= 1, "%s: bad dims planes=%lld H=%d W=%d C=%d -> %d x %d",
               what, planes, H, W, C, oh, ow);
    ML_REQUIRE((long long)H * W * C < (1ll << 31) && (long long)oh * ow * C < (1ll << 31) && oh <= MAX_GRID_YZ,
               "%s: a plane of %d x %d x %d -> %d x %d is too large (H*W*C and oh*ow*C < 2^31, oh <= 65535)", what, H, W, C, oh, ow);
    ML_REQUIRE(planes == 0 || (src && dst), "%s: null pointer", what);
    return ML_OK;
}

}  // namespace cvk
}  // namespace

using namespace cvk;

extern "C" int ml_cv_resize_linear_u8(const void *src, void *dst, int64_t planes, int32_t H, int32_t W, int32_t C, int32_t oh,
                                      int32_t ow, int32_t skip_minus_one, void *stream) {
    const char *what = "cv_resize_linear_u8";
    const int e = check(what, src, dst, planes, H, W, C, oh, ow);
    if (e != ML_OK || planes == 0) return e;
    launch<FIXED, uint8_t>((const uint8_t *)src, (uint8_t *)dst, planes, make_geo(H, W, C, oh, ow), skip_minus_one != 0,
                           (hipStream_t)stream);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_cv_resize_linear_round_u8(const void *src, void *dst, int32_t dst_is_f32, int64_t planes, int32_t H, int32_t W,
                                            int32_t C, int32_t oh, int32_t ow, void *stream) {
    const char *what = "cv_resize_linear_round_u8";
    const int e = check(what, src, dst, planes, H, W, C, oh, ow);
    if (e != ML_OK || planes == 0) return e;
    ML_REQUIRE(!dst_is_f32 || ((uintptr_t)dst & 3u) == 0, "%s: a float32 destination must be 4-byte aligned", what);
    const Geo g = make_geo(H, W, C, oh, ow);
    if (dst_is_f32)
        launch<ROUND, float>((const uint8_t *)src, (float *)dst, planes, g, 0, (hipStream_t)stream);
    else
        launch<ROUND, uint8_t>((const uint8_t *)src, (uint8_t *)dst, planes, g, 0, (hipStream_t)stream);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_cv_resize_reference_host(const void *src, void *dst, int32_t mode, int64_t planes, int32_t H, int32_t W, int32_t C,
                                           int32_t oh, int32_t ow, int32_t skip_minus_one) {
    const char *what = "cv_resize_reference_host";
    ML_REQUIRE(mode >= ML_CV_RESIZE_U8 && mode <= ML_CV_RESIZE_ROUND_F32, "%s: mode %d", what, mode);
    const int e = check(what, src, dst, planes, H, W, C, oh, ow);
    if (e != ML_OK || planes == 0) return e;
    ML_REQUIRE(mode != ML_CV_RESIZE_ROUND_F32 || ((uintptr_t)dst & 3u) == 0, "%s: a float32 destination must be 4-byte aligned", what);
    const Geo g = make_geo(H, W, C, oh, ow);
    if (mode == ML_CV_RESIZE_U8)
        host_loop<FIXED, uint8_t>((const uint8_t *)src, (uint8_t *)dst, planes, g, skip_minus_one != 0);
    else if (mode == ML_CV_RESIZE_ROUND_U8)
        host_loop<ROUND, uint8_t>((const uint8_t *)src, (uint8_t *)dst, planes, g, 0);
    else
        host_loop<ROUND, float>((const uint8_t *)src, (float *)dst, planes, g, 0);
    return ML_OK;
}
