// HBM-bound NHWC kernels: preprocess, depthwise 3x3, max-pool, bilinear (align_corners),
// global mean, channel scale, fill.  All are vectorised over channels, 16 bytes per lane (float4, or 8 halves for the
// fp16-storage instantiations of depthwise 3x3, max-pool, bilinear and global mean), so a wave reads 1 KiB contiguous
// per instruction; none has inter-block reuse, so no LDS staging is used (re-reads of the 3x3 halo are served by L1/L2).
#include "common.h"

namespace {

constexpr int TPB = 256;

inline unsigned grid_for(long long n) { return (unsigned)((n + TPB - 1) / TPB); }

// ------------------------------------------------------------------ preprocess
struct Affine3 { float m[3], d[3], s[3]; };

__global__ void preprocess_kernel(const void *in, int is_u8, float *out, long long npix, int out_c,
                                  int flip, Affine3 a) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= npix) return;
    float v[3];
    if (is_u8) {
        const unsigned char *p = reinterpret_cast<const unsigned char *>(in) + i * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    } else {
        const float *p = reinterpret_cast<const float *>(in) + i * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    }
    if (flip) { const float t = v[0]; v[0] = v[2]; v[2] = t; }
    // reference order: (x - mean) / divisor (+ shift); a true division keeps x/127.5 bit-close
    const float r0 = (v[0] - a.m[0]) / a.d[0] + a.s[0];
    const float r1 = (v[1] - a.m[1]) / a.d[1] + a.s[1];
    const float r2 = (v[2] - a.m[2]) / a.d[2] + a.s[2];
    if (out_c == 4) {
        f32x4 o = {r0, r1, r2, 0.f};
        *reinterpret_cast<f32x4 *>(out + i * 4) = o;
    } else {
        out[i * 3 + 0] = r0; out[i * 3 + 1] = r1; out[i * 3 + 2] = r2;
    }
}

// ---- the NHWC kernels below are written once over the storage type T (float or _Float16) and run the same arithmetic in
// fp32 on the converted values, ONE rounding at the store: a lane moves V = 16 / sizeof(T) channels (4 floats or 8 halves)
template <class T> constexpr int VEC = 16 / (int)sizeof(T);

// V channels at p <-> floats, as 16-byte accesses (N = a multiple of V: the fp32 weights of a half lane are two float4)
template <class T, int N>
__device__ __forceinline__ void load_f(const T *p, float (&v)[N]) {
    typedef T Tv __attribute__((ext_vector_type(VEC<T>)));
#pragma unroll
    for (int k = 0; k < N / VEC<T>; ++k) {
        const Tv x = *reinterpret_cast<const Tv *>(p + k * VEC<T>);
#pragma unroll
        for (int e = 0; e < VEC<T>; ++e) v[k * VEC<T> + e] = (float)x[e];
    }
}
template <class T>
__device__ __forceinline__ void store_f(T *p, const float (&v)[VEC<T>]) {
    typedef T Tv __attribute__((ext_vector_type(VEC<T>)));
    Tv x;
#pragma unroll
    for (int e = 0; e < VEC<T>; ++e) x[e] = (T)v[e];
    *reinterpret_cast<Tv *>(p) = x;
}

// what the two storage types do differently: the max-pool's start value and max (fp32: fmaxf; fp16: a compare-select on
// the halves themselves); the bilinear weight of a sample position o s (fp32: o s - floor(o s) rounded once, an fma; fp16:
// o s rounded first); global_mean's block shape (channel lanes x row groups, 256 threads)
template <class T> struct Elt;
template <> struct Elt<float> {
    static constexpr float LOWEST = -3.4e38f;
    static __device__ __forceinline__ float max(float m, float x) { return fmaxf(m, x); }
    static __device__ __forceinline__ float frac(float o, float s, float fl) { return fmaf(o, s, -fl); }
    static constexpr int MEAN_Q = 16;                   // 16 float4 lanes x 16 row groups: 256 contiguous bytes per row group
};
template <> struct Elt<_Float16> {
    static constexpr float LOWEST = -65504.f;
    static __device__ __forceinline__ _Float16 max(_Float16 m, _Float16 x) { return x > m ? x : m; }
    static __device__ __forceinline__ float frac(float o, float s, float fl) {
#pragma clang fp contract(off)
        return o * s - fl;
    }
    static constexpr int MEAN_Q = 8;                    // 8 lanes of 8 halves x 32 row groups: 128 contiguous bytes per row group
};

// ------------------------------------------------------------------ depthwise 3x3 (dilated): engine/layers/semantic.py:63-64;
// weights / bias fp32
template <class T>
__global__ void dwconv3x3_kernel(const T *__restrict__ in, const float *__restrict__ wgt,
                                 const float *__restrict__ bias, T *__restrict__ out,
                                 int H, int W, int CV, int in_cs, int in_co, int out_cs, int out_co,
                                 int Ho, int Wo, int stride, int dil, int pad_t, int pad_l, int act,
                                 long long total) {
    constexpr int V = VEC<T>;
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= total) return;
    const int cv = (int)(idx % CV);
    long long pix = idx / CV;
    const int ox = (int)(pix % Wo); pix /= Wo;
    const int oy = (int)(pix % Ho);
    const int b = (int)(pix / Ho);
    const int c = cv * V;
    const int C = CV * V;
    float acc[V];
    if (bias) {
        load_f(bias + c, acc);
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int iy = oy * stride - pad_t + kh * dil;
        if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ix = ox * stride - pad_l + kw * dil;
            if ((unsigned)ix >= (unsigned)W) continue;
            float x[V], w[V];
            load_f(in + ((long long)(b * H + iy) * W + ix) * in_cs + in_co + c, x);
            load_f(wgt + (kh * 3 + kw) * C + c, w);
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += x[e] * w[e];
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = ml_apply_act(acc[e], act);
    store_f(out + ((long long)(b * Ho + oy) * Wo + ox) * out_cs + out_co + c, acc);
}

// ------------------------------------------------------------------ max pool 3x3 s2 (zero pad, input >= 0): ZeroPadding2D(1) +
// MaxPooling2D(3, 2), engine/backbone/ResNext.py:351-352; on the stored values themselves
template <class T>
__global__ void maxpool3x3s2_kernel(const T *__restrict__ in, T *__restrict__ out,
                                    int H, int W, int CV, int Ho, int Wo, int pad_t, int pad_l,
                                    long long total) {
    constexpr int V = VEC<T>;
    typedef T Tv __attribute__((ext_vector_type(V)));
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= total) return;
    const int cv = (int)(idx % CV);
    long long pix = idx / CV;
    const int ox = (int)(pix % Wo); pix /= Wo;
    const int oy = (int)(pix % Ho);
    const int b = (int)(pix / Ho);
    const int C = CV * V;
    bool any_pad = false;
    Tv m;
#pragma unroll
    for (int e = 0; e < V; ++e) m[e] = (T)Elt<T>::LOWEST;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int iy = oy * 2 - pad_t + kh;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ix = ox * 2 - pad_l + kw;
            if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) { any_pad = true; continue; }
            const Tv x = *reinterpret_cast<const Tv *>(in + ((long long)(b * H + iy) * W + ix) * C + cv * V);
#pragma unroll
            for (int e = 0; e < V; ++e) m[e] = Elt<T>::max(m[e], x[e]);
        }
    }
    if (any_pad) {  // the explicit ZeroPadding2D contributes zeros to the window
#pragma unroll
        for (int e = 0; e < V; ++e) m[e] = Elt<T>::max((T)0.f, m[e]);
    }
    *reinterpret_cast<Tv *>(out + ((long long)(b * Ho + oy) * Wo + ox) * C + cv * V) = m;
}

// ------------------------------------------------------------------ bilinear, align_corners=True (+ FPN Add / concat-slice
// store): tf.compat.v1.image.resize_bilinear(align_corners=True), engine/layers/misc.py:306
template <class T>
__global__ void bilinear_ac_kernel(const T *__restrict__ in, const T *__restrict__ add,
                                   T *__restrict__ out, int H, int W, int CV, int in_cs, int in_co,
                                   int Ho, int Wo, float sy, float sx, int add_cs, int add_co,
                                   int out_cs, int out_co, long long total) {
    constexpr int V = VEC<T>;
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % CV) * V;
    long long pix = idx / CV;
    const int ox = (int)(pix % Wo); pix /= Wo;
    const int oy = (int)(pix % Ho);
    const int b = (int)(pix / Ho);
    const float fy = (float)oy * sy;
    const float fx = (float)ox * sx;
    const float fly = floorf(fy), flx = floorf(fx);
    const int y0 = max((int)fly, 0), x0 = max((int)flx, 0);
    const int y1 = min((int)ceilf(fy), H - 1), x1 = min((int)ceilf(fx), W - 1);
    const float ty = Elt<T>::frac((float)oy, sy, fly), tx = Elt<T>::frac((float)ox, sx, flx);
    const T *base = in + (long long)b * H * W * in_cs + in_co + c;
    float tl[V], tr[V], bl[V], br[V], v[V];
    load_f(base + ((long long)y0 * W + x0) * in_cs, tl);
    load_f(base + ((long long)y0 * W + x1) * in_cs, tr);
    load_f(base + ((long long)y1 * W + x0) * in_cs, bl);
    load_f(base + ((long long)y1 * W + x1) * in_cs, br);
    const long long opix = (long long)(b * Ho + oy) * Wo + ox;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float top = tl[e] + (tr[e] - tl[e]) * tx;
        const float bot = bl[e] + (br[e] - bl[e]) * tx;
        v[e] = top + (bot - top) * ty;
    }
    if (add) {
        float a[V];
        load_f(add + opix * add_cs + add_co + c, a);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] += a[e];
    }
    store_f(out + opix * out_cs + out_co + c, v);
}

// ------------------------------------------------------------------ global mean over HW (tf.reduce_mean, semantic.py:149)
// grid (ceil(CV / Q), B), block 256 = Q channel lanes x 256 / Q row groups (Elt<T>::MEAN_Q); fp64 accumulation, the partial
// sums of a channel added in a fixed order.  (The first fp32 layout -- 64 lanes x 4 row groups -- gave ASPP's pooling branch
// 64 blocks for 67 MB: 79 us.)
template <class T>
__global__ void global_mean_kernel(const T *__restrict__ in, T *__restrict__ out, int HW, int CV) {
    constexpr int V = VEC<T>, Q = Elt<T>::MEAN_Q, G = 256 / Q;
    __shared__ double red[G][Q][V];
    const int q = threadIdx.x & (Q - 1);
    const int g = threadIdx.x / Q;
    const int cv = blockIdx.x * Q + q;
    const int b = blockIdx.y;
    double s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0;
    if (cv < CV) {
        const T *p = in + (long long)b * HW * CV * V + cv * V;
        for (int i = g; i < HW; i += G) {
            float x[V];
            load_f(p + (long long)i * CV * V, x);
#pragma unroll
            for (int e = 0; e < V; ++e) s[e] += (double)x[e];
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) red[g][q][e] = s[e];
    __syncthreads();
    if (g == 0 && cv < CV) {
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            double t = 0;
#pragma unroll
            for (int k = 0; k < G; ++k) t += red[k][q][e];
            o[e] = (float)(t / (double)HW);
        }
        store_f(out + (long long)b * CV * V + cv * V, o);
    }
}

__global__ void scale_channels_kernel(float *__restrict__ x, const float *__restrict__ s, int HW, int C4,
                                      long long total) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const int b = (int)(idx / ((long long)C4 * HW));
    f32x4 v = *reinterpret_cast<f32x4 *>(x + idx * 4);
    const f32x4 sc = *reinterpret_cast<const f32x4 *>(s + ((long long)b * C4 + c4) * 4);
    *reinterpret_cast<f32x4 *>(x + idx * 4) = v * sc;
}

__global__ void add_kernel(float *__restrict__ x, const float *__restrict__ y, long long n4) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n4) return;
    f32x4 a = *reinterpret_cast<f32x4 *>(x + i * 4);
    a += *reinterpret_cast<const f32x4 *>(y + i * 4);
    *reinterpret_cast<f32x4 *>(x + i * 4) = a;
}

__global__ void fill_kernel(float *x, float v, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) x[i] = v;
}

// ---- launchers shared by the fp32 and fp16 entry points: `name` leads every message; channel counts, strides and offsets
// are multiples of V = VEC<T>
template <class T> constexpr const char *C_NOTE = sizeof(T) == 2 ? " (C % 8)" : "";

template <class T>
int dwconv3x3_launch(const char *name, const void *in, const float *wgt, const float *bias, void *out, int B, int H, int W,
                     int C, int in_cstride, int in_coff, int out_cstride, int out_coff, int Ho, int Wo, int stride, int dil,
                     int pad_t, int pad_l, int act, void *stream) {
    constexpr int V = VEC<T>;
    ML_REQUIRE(in && wgt && out, "%s: null pointer", name);
    ML_REQUIRE(B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && C > 0 && C % V == 0, "%s: bad dims (C %% %d)", name, V);
    ML_REQUIRE(in_cstride % V == 0 && in_coff % V == 0 && out_cstride % V == 0 && out_coff % V == 0,
               "%s: channel strides/offsets must be multiples of %d", name, V);
    ML_REQUIRE(in_coff + C <= in_cstride && out_coff + C <= out_cstride, "%s: slice exceeds buffer", name);
    ML_REQUIRE(ml_aligned16(in) && ml_aligned16(wgt) && ml_aligned16(out) && (!bias || ml_aligned16(bias)),
               "%s: pointers must be 16-byte aligned", name);
    ML_REQUIRE((long long)B * H * W < (1ll << 31) && stride > 0 && dil > 0, "%s: geometry out of range", name);
    const long long total = (long long)B * Ho * Wo * (C / V);
    hipLaunchKernelGGL(dwconv3x3_kernel<T>, dim3(grid_for(total)), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const T *>(in), wgt, bias, reinterpret_cast<T *>(out), H, W, C / V, in_cstride, in_coff,
                       out_cstride, out_coff, Ho, Wo, stride, dil, pad_t, pad_l, act, total);
    ML_CHECK_LAUNCH(name);
    return ML_OK;
}

template <class T>
int maxpool3x3s2_launch(const char *name, const void *in, void *out, int B, int H, int W, int C, int Ho, int Wo, int pad_t,
                        int pad_l, void *stream) {
    constexpr int V = VEC<T>;
    ML_REQUIRE(in && out && B > 0 && H > 0 && W > 0 && C > 0 && C % V == 0, "%s: bad arguments%s", name, C_NOTE<T>);
    ML_REQUIRE(ml_aligned16(in) && ml_aligned16(out), "%s: pointers must be 16-byte aligned", name);
    ML_REQUIRE((long long)B * H * W < (1ll << 31), "%s: too many pixels", name);
    const long long total = (long long)B * Ho * Wo * (C / V);
    ML_REQUIRE(total < (1ll << 31) * TPB, "%s: grid too large", name);
    hipLaunchKernelGGL(maxpool3x3s2_kernel<T>, dim3(grid_for(total)), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const T *>(in), reinterpret_cast<T *>(out), H, W, C / V, Ho, Wo, pad_t, pad_l, total);
    ML_CHECK_LAUNCH(name);
    return ML_OK;
}

template <class T>
int resize_bilinear_ac_launch(const char *name, const void *in, const void *add, void *out, int B, int H, int W, int C,
                              int in_cstride, int in_coff, int Ho, int Wo, int add_cstride, int add_coff, int out_cstride,
                              int out_coff, void *stream) {
    constexpr int V = VEC<T>;
    ML_REQUIRE(in && out && B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && C > 0 && C % V == 0, "%s: bad arguments%s", name,
               C_NOTE<T>);
    ML_REQUIRE(in_cstride % V == 0 && in_coff % V == 0 && out_cstride % V == 0 && out_coff % V == 0,
               "%s: channel strides/offsets must be multiples of %d", name, V);
    ML_REQUIRE(in_coff + C <= in_cstride && out_coff + C <= out_cstride, "%s: slice exceeds buffer", name);
    if (add) ML_REQUIRE(add_cstride % V == 0 && add_coff % V == 0 && add_coff + C <= add_cstride && ml_aligned16(add),
                        "%s: bad add view", name);
    ML_REQUIRE(ml_aligned16(in) && ml_aligned16(out), "%s: pointers must be 16-byte aligned", name);
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
    const float sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const long long total = (long long)B * Ho * Wo * (C / V);
    hipLaunchKernelGGL(bilinear_ac_kernel<T>, dim3(grid_for(total)), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const T *>(in), reinterpret_cast<const T *>(add), reinterpret_cast<T *>(out), H, W, C / V,
                       in_cstride, in_coff, Ho, Wo, sy, sx, add_cstride, add_coff, out_cstride, out_coff, total);
    ML_CHECK_LAUNCH(name);
    return ML_OK;
}

template <class T>
int global_mean_launch(const char *name, const void *in, void *out, int B, int HW, int C, void *stream) {
    constexpr int V = VEC<T>, Q = Elt<T>::MEAN_Q;
    ML_REQUIRE(in && out && B > 0 && HW > 0 && C > 0 && C % V == 0, "%s: bad arguments%s", name, C_NOTE<T>);
    ML_REQUIRE(ml_aligned16(in) && ml_aligned16(out), "%s: pointers must be 16-byte aligned", name);
    const int CV = C / V;
    hipLaunchKernelGGL(global_mean_kernel<T>, dim3((CV + Q - 1) / Q, B), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const T *>(in), reinterpret_cast<T *>(out), HW, CV);
    ML_CHECK_LAUNCH(name);
    return ML_OK;
}

}  // namespace

extern "C" int ml_preprocess_f32(const void *in, int32_t is_u8, float *out, int64_t npix, int32_t out_c,
                                 int32_t flip, const float *mean, const float *div, const float *shift,
                                 void *stream) {
    ML_REQUIRE(in && out && npix > 0 && mean && div && shift, "preprocess: bad arguments");
    ML_REQUIRE(out_c == 3 || out_c == 4, "preprocess: out_c must be 3 or 4");
    ML_REQUIRE(div[0] != 0.f && div[1] != 0.f && div[2] != 0.f, "preprocess: zero divisor");
    Affine3 a;
    for (int k = 0; k < 3; ++k) { a.m[k] = mean[k]; a.d[k] = div[k]; a.s[k] = shift[k]; }
    if (out_c == 4) ML_REQUIRE(ml_aligned16(out), "preprocess: out must be 16-byte aligned");
    hipLaunchKernelGGL(preprocess_kernel, dim3(grid_for(npix)), dim3(TPB), 0, (hipStream_t)stream, in, is_u8, out,
                       (long long)npix, out_c, flip, a);
    ML_CHECK_LAUNCH("preprocess");
    return ML_OK;
}

extern "C" int ml_dwconv3x3_f32(const float *in, const float *wgt, const float *bias, float *out, int32_t B,
                                int32_t H, int32_t W, int32_t C, int32_t in_cstride, int32_t in_coff,
                                int32_t out_cstride, int32_t out_coff, int32_t Ho, int32_t Wo, int32_t stride,
                                int32_t dil, int32_t pad_t, int32_t pad_l, int32_t act, void *stream) {
    return dwconv3x3_launch<float>("dwconv3x3", in, wgt, bias, out, B, H, W, C, in_cstride, in_coff, out_cstride, out_coff, Ho,
                                   Wo, stride, dil, pad_t, pad_l, act, stream);
}

extern "C" int ml_dwconv3x3_f16(const void *in, const float *wgt, const float *bias, void *out, int32_t B, int32_t H,
                                int32_t W, int32_t C, int32_t in_cstride, int32_t in_coff, int32_t out_cstride,
                                int32_t out_coff, int32_t Ho, int32_t Wo, int32_t stride, int32_t dil, int32_t pad_t,
                                int32_t pad_l, int32_t act, void *stream) {
    return dwconv3x3_launch<_Float16>("dwconv3x3_f16", in, wgt, bias, out, B, H, W, C, in_cstride, in_coff, out_cstride,
                                      out_coff, Ho, Wo, stride, dil, pad_t, pad_l, act, stream);
}

extern "C" int ml_maxpool3x3s2_f32(const float *in, float *out, int32_t B, int32_t H, int32_t W, int32_t C,
                                   int32_t Ho, int32_t Wo, int32_t pad_t, int32_t pad_l, void *stream) {
    return maxpool3x3s2_launch<float>("maxpool", in, out, B, H, W, C, Ho, Wo, pad_t, pad_l, stream);
}

extern "C" int ml_maxpool3x3s2_f16(const void *in, void *out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho,
                                   int32_t Wo, int32_t pad_t, int32_t pad_l, void *stream) {
    return maxpool3x3s2_launch<_Float16>("maxpool_f16", in, out, B, H, W, C, Ho, Wo, pad_t, pad_l, stream);
}

extern "C" int ml_resize_bilinear_ac_f32(const float *in, const float *add, float *out, int32_t B, int32_t H,
                                         int32_t W, int32_t C, int32_t in_cstride, int32_t in_coff, int32_t Ho,
                                         int32_t Wo, int32_t add_cstride, int32_t add_coff, int32_t out_cstride,
                                         int32_t out_coff, void *stream) {
    return resize_bilinear_ac_launch<float>("resize_bilinear", in, add, out, B, H, W, C, in_cstride, in_coff, Ho, Wo, add_cstride,
                                            add_coff, out_cstride, out_coff, stream);
}

extern "C" int ml_resize_bilinear_ac_f16(const void *in, const void *add, void *out, int32_t B, int32_t H, int32_t W,
                                         int32_t C, int32_t in_cstride, int32_t in_coff, int32_t Ho, int32_t Wo,
                                         int32_t add_cstride, int32_t add_coff, int32_t out_cstride, int32_t out_coff,
                                         void *stream) {
    return resize_bilinear_ac_launch<_Float16>("resize_bilinear_f16", in, add, out, B, H, W, C, in_cstride, in_coff, Ho, Wo,
                                               add_cstride, add_coff, out_cstride, out_coff, stream);
}

extern "C" int ml_global_mean_f32(const float *in, float *out, int32_t B, int32_t HW, int32_t C, void *stream) {
    return global_mean_launch<float>("global_mean", in, out, B, HW, C, stream);
}

extern "C" int ml_global_mean_f16(const void *in, void *out, int32_t B, int32_t HW, int32_t C, void *stream) {
    return global_mean_launch<_Float16>("global_mean_f16", in, out, B, HW, C, stream);
}

extern "C" int ml_scale_channels_f32(float *x, const float *s, int32_t B, int32_t HW, int32_t C, void *stream) {
    ML_REQUIRE(x && s && B > 0 && HW > 0 && C > 0 && C % 4 == 0, "scale_channels: bad arguments");
    ML_REQUIRE(ml_aligned16(x) && ml_aligned16(s), "scale_channels: pointers must be 16-byte aligned");
    const long long total = (long long)B * HW * (C / 4);
    hipLaunchKernelGGL(scale_channels_kernel, dim3(grid_for(total)), dim3(TPB), 0, (hipStream_t)stream, x, s, HW, C / 4,
                       total);
    ML_CHECK_LAUNCH("scale_channels");
    return ML_OK;
}

extern "C" int ml_add_f32(float *x, const float *y, int64_t n, void *stream) {
    ML_REQUIRE(x && y && n > 0 && n % 4 == 0, "add: bad arguments (n %% 4)");
    ML_REQUIRE(ml_aligned16(x) && ml_aligned16(y), "add: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(n / 4)), dim3(TPB), 0, (hipStream_t)stream, x, y, (long long)(n / 4));
    ML_CHECK_LAUNCH("add");
    return ML_OK;
}

extern "C" int ml_fill_f32(float *x, float v, int64_t n, void *stream) {
    ML_REQUIRE(x && n >= 0, "fill: bad arguments");
    if (n == 0) return ML_OK;
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(TPB), 0, (hipStream_t)stream, x, v, (long long)n);
    ML_CHECK_LAUNCH("fill");
    return ML_OK;
}
