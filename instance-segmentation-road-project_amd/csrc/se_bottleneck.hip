// Tail of a post-activation bottleneck unit with ChannelSE (thirdparty senet.py SEResNetBottleneck :46-88 /
// SEResNeXtBottleneck :91-134, ChannelSE _common_blocks.py:88-119), NHWC [B,HW,C], one storage type T per entry point:
//   g   = sigmoid(W2 relu(W1 mean_hw(c3) + b1) + b2)     (ChannelSE: two 1x1 convs with bias, once per sample)
//   out = relu(c3 * g + residual)                        (Multiply, then the Add, then the unit's ReLU)
// Three launches, one fixed order for every sum:
//   1. sb_pool: block (sample, pool chunk) sums its chunk's channels in fp64 (each thread its rows in order, then the rows
//      in order) and stores them as the chunk's slab [C] doubles.  Pool chunks follow from (HW, C) alone.
//   2. sb_gate: block n adds sample n's slabs in order, evaluates the mean and both FC layers in fp64 (FC1's C-sum cut into
//      a fixed number of parts that depends on (C, Hd) only, added in order) and stores g as two floats in the
//      workspace: g_hi = g rounded to fp32 and g_lo = (g - g_hi) rounded.  W1 / W2 are read here only: once per sample,
//      never per streaming block.
//   3. sb_tail: block (sample, tail chunk) streams its chunk in fp32.  fp32 tensors: the reference's two fp32 ops,
//      relu(__fadd_rn(__fmul_rn(c3, g_hi), residual)).  Half tensors: relu(fma(c3, g_lo, fma(c3, g_hi, residual))), then
//      one rounding at the store -- the fp32 error is then a few fp32 ulps of the result even where c3 * g and the
//      residual cancel into the half subnormals, where a separate product rounding alone would cost a whole half ulp.
//      out may be c3 itself (every element is read and written by one thread).
// No atomics: eager launches, graph replay and image k of a batch against image k alone give the same bits.
#include "common.h"
#include "ranges.h"

namespace {

constexpr int SB_TPB = 256;               // pool and tail blocks
constexpr int SB_GATE_TPB = 1024;         // gate blocks (one per sample)
constexpr int SB_MAX_C = 2048;
constexpr int SB_MAX_HD = 128;
constexpr int SB_TAIL_ELEMS = 16384;      // elements per tail block (pixels = 16384 / C, at least one)
constexpr int SB_POOL_ELEMS = 32768;      // elements per pool block at least ...
constexpr int SB_MAX_SLABS = 128;         // ... and pool chunks per sample at most: 128, and at most 65536 slab elements
constexpr int SB_SLAB_ELEMS = 65536;      // (512 KB) per sample, which the sample's gate block reads

template <class T> constexpr int VEC = 16 / (int)sizeof(T);      // channels per 16-byte lane: 4 floats or 8 halves
template <class T> constexpr int MAX_LANES = SB_MAX_C / VEC<T> / SB_TPB + (SB_MAX_C / VEC<T> % SB_TPB != 0);

struct SbArgs {
    const void *c3, *residual;
    const float *w1, *b1, *w2, *b2;
    void *out;
    double *slabs;             // [B][npool][C]
    float *gate;               // [2][B][C]: g_hi, then g_lo
    int B;
    int HW, C, Hd, npool, pool_chunk, ntail, tail_chunk;
};

template <class T>
__device__ __forceinline__ void load_f(const T *p, float (&v)[VEC<T>]) {
    typedef T Tv __attribute__((ext_vector_type(VEC<T>)));
    const Tv x = *reinterpret_cast<const Tv *>(p);
#pragma unroll
    for (int e = 0; e < VEC<T>; ++e) v[e] = (float)x[e];
}
template <class T>
__device__ __forceinline__ void store_f(T *p, const float (&v)[VEC<T>]) {
    typedef T Tv __attribute__((ext_vector_type(VEC<T>)));
    Tv x;
#pragma unroll
    for (int e = 0; e < VEC<T>; ++e) x[e] = (T)v[e];
    *reinterpret_cast<Tv *>(p) = x;
}

// A block's threads over one pixel row of CV = C / V lanes: with CV < 256, rpi = 256 / CV rows side by side (thread
// (r, cv)); otherwise one row, thread t taking lanes t, t + 256 (at most MAX_LANES).
struct Lanes {
    int CV, rpi, r, cv0;
    __device__ Lanes(int C, int V, int t) {
        CV = C / V;
        rpi = CV >= SB_TPB ? 1 : SB_TPB / CV;
        r = CV >= SB_TPB ? 0 : t / CV;
        cv0 = CV >= SB_TPB ? t : t % CV;
    }
};

template <class T>
__global__ void __launch_bounds__(SB_TPB) sb_pool(const SbArgs A) {
    constexpr int V = VEC<T>, NL = MAX_LANES<T>;
    __shared__ double red[SB_TPB * V];
    const int n = blockIdx.x / A.npool, k = blockIdx.x % A.npool;
    const int C = A.C, t = threadIdx.x;
    const Lanes L(C, V, t);
    const int p0 = k * A.pool_chunk, p1 = min(A.HW, p0 + A.pool_chunk);
    const T *x = reinterpret_cast<const T *>(A.c3) + (long long)n * A.HW * C;
    double *slab = A.slabs + ((long long)n * A.npool + k) * C;
    double acc[NL][V];
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[l][e] = 0.0;
    if (L.r < L.rpi) {
#pragma unroll 4
        for (int p = p0 + L.r; p < p1; p += L.rpi) {
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const int cv = L.cv0 + l * SB_TPB;
                if (cv < L.CV) {
                    float v[V];
                    load_f<T>(x + (long long)p * C + cv * V, v);
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[l][e] += (double)v[e];
                }
            }
        }
    }
    if (L.rpi == 1) {                               // one row: every channel has one thread, no cross-thread sum
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int cv = L.cv0 + l * SB_TPB;
            if (cv < L.CV)
#pragma unroll
                for (int e = 0; e < V; ++e) slab[cv * V + e] = acc[l][e];
        }
        return;
    }
    if (L.r < L.rpi)
#pragma unroll
        for (int e = 0; e < V; ++e) red[L.r * C + L.cv0 * V + e] = acc[0][e];
    __syncthreads();
    for (int c = t; c < C; c += SB_TPB) {
        double s = 0.0;
        for (int i = 0; i < L.rpi; ++i) s += red[i * C + c];
        slab[c] = s;
    }
}

__global__ void __launch_bounds__(SB_GATE_TPB) sb_gate(const SbArgs A) {
    __shared__ double mean[SB_MAX_C], part[SB_GATE_TPB], hid[SB_MAX_HD];
    const int n = blockIdx.x, C = A.C, Hd = A.Hd, t = threadIdx.x;
    const double *slab = A.slabs + (long long)n * A.npool * C;
    const double inv = 1.0 / (double)A.HW;
    // the loops below keep one accumulator each, in order; unrolled so that their loads are in flight together
    for (int c = t; c < C; c += SB_GATE_TPB) {
        double s = 0.0;
#pragma unroll 16
        for (int i = 0; i < A.npool; ++i) s += slab[(long long)i * C + c];
        mean[c] = s * inv;
    }
    __syncthreads();
    // FC 1 (bias, relu): hidden unit j = t % HP, its C-sum cut into Q = 1024 / HP parts of consecutive channels (t / HP)
    const int HP = Hd <= 16 ? 16 : Hd <= 32 ? 32 : Hd <= 64 ? 64 : 128, Q = SB_GATE_TPB / HP;
    {
        const int j = t % HP, q = t / HP, cq = (C + Q - 1) / Q;
        double a = 0.0;
        if (j < Hd) {
            const int c1 = min(C, (q + 1) * cq);
#pragma unroll 16
            for (int c = q * cq; c < c1; ++c) a = fma(mean[c], (double)A.w1[(long long)c * Hd + j], a);
        }
        part[t] = a;
    }
    __syncthreads();
    if (t < Hd) {
        double a = part[t];
        for (int q = 1; q < Q; ++q) a += part[q * HP + t];
        hid[t] = fmax(a + (double)A.b1[t], 0.0);
    }
    __syncthreads();
    // FC 2 (bias, sigmoid), one channel per thread: g_hi, g_lo
    for (int c = t; c < C; c += SB_GATE_TPB) {
        double a = 0.0;
#pragma unroll 16
        for (int j = 0; j < Hd; ++j) a = fma(hid[j], (double)A.w2[(long long)j * C + c], a);
        const double g = 1.0 / (1.0 + exp(-(a + (double)A.b2[c])));
        const float hi = (float)g;
        A.gate[(long long)n * C + c] = hi;
        A.gate[((long long)A.B + n) * C + c] = (float)(g - (double)hi);
    }
}

// relu(c3 * g + residual) in fp32 (see the file comment for the two forms)
template <class T> struct Tail;
template <> struct Tail<float> {
    static __device__ __forceinline__ float f(float x, float hi, float, float r) {
        return fmaxf(__fadd_rn(__fmul_rn(x, hi), r), 0.f);                       // Multiply, Add, ReLU
    }
};
template <> struct Tail<_Float16> {
    static __device__ __forceinline__ float f(float x, float hi, float lo, float r) {
        return fmaxf(fmaf(x, lo, fmaf(x, hi, r)), 0.f);
    }
};

template <class T>
__global__ void __launch_bounds__(SB_TPB) sb_tail(const SbArgs A) {
    constexpr int V = VEC<T>, NL = MAX_LANES<T>;
    const int n = blockIdx.x / A.ntail, k = blockIdx.x % A.ntail;
    const int C = A.C, t = threadIdx.x;
    const Lanes L(C, V, t);
    if (L.r >= L.rpi) return;
    constexpr bool LO = sizeof(T) == 2;
    float g[NL][V], glo[NL][V];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int cv = min(L.cv0 + l * SB_TPB, L.CV - 1);
        const f32x4 *gp = reinterpret_cast<const f32x4 *>(A.gate + (long long)n * C + cv * V);
        const f32x4 *lp = reinterpret_cast<const f32x4 *>(A.gate + ((long long)A.B + n) * C + cv * V);
#pragma unroll
        for (int h = 0; h < V / 4; ++h) {
            const f32x4 q = gp[h], ql = LO ? lp[h] : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                g[l][h * 4 + e] = q[e];
                glo[l][h * 4 + e] = ql[e];
            }
        }
    }
    const int p0 = k * A.tail_chunk, p1 = min(A.HW, p0 + A.tail_chunk);
    const long long base = (long long)n * A.HW * C;
    const T *x = reinterpret_cast<const T *>(A.c3) + base;
    const T *res = reinterpret_cast<const T *>(A.residual) + base;
    T *out = reinterpret_cast<T *>(A.out) + base;
#pragma unroll 4
    for (int p = p0 + L.r; p < p1; p += L.rpi) {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int cv = L.cv0 + l * SB_TPB;
            if (cv < L.CV) {
                const long long off = (long long)p * C + cv * V;
                float y[V], s[V];
                load_f<T>(x + off, y);
                load_f<T>(res + off, s);
#pragma unroll
                for (int e = 0; e < V; ++e) y[e] = Tail<T>::f(y[e], g[l][e], glo[l][e], s[e]);
                store_f<T>(out + off, y);
            }
        }
    }
}

int64_t sb_tail_chunk(int32_t C) { return C >= SB_TAIL_ELEMS ? 1 : SB_TAIL_ELEMS / C; }
int64_t sb_ntail(int32_t HW, int32_t C) { return ((int64_t)HW + sb_tail_chunk(C) - 1) / sb_tail_chunk(C); }
int64_t sb_pool_chunk(int32_t HW, int32_t C) {
    int64_t want = ((int64_t)HW * C + SB_POOL_ELEMS - 1) / SB_POOL_ELEMS;
    const int64_t cap = SB_SLAB_ELEMS / C < SB_MAX_SLABS ? SB_SLAB_ELEMS / C : SB_MAX_SLABS;
    want = want < 1 ? 1 : (want > cap ? cap : want);
    return ((int64_t)HW + want - 1) / want;
}
int64_t sb_npool(int32_t HW, int32_t C) { return ((int64_t)HW + sb_pool_chunk(HW, C) - 1) / sb_pool_chunk(HW, C); }

template <class T>
int se_bottleneck_launch(const char *what, const ml_se_bottleneck_desc *d, void *workspace, int64_t workspace_bytes,
                         void *stream) {
    constexpr int V = VEC<T>;
    ML_REQUIRE(d, "%s: null descriptor", what);
    ML_REQUIRE(d->c3 && d->residual && d->out && d->w1 && d->b1 && d->w2 && d->b2,
               "%s: c3, residual, out, w1, b1, w2 and b2 are required", what);
    ML_REQUIRE(d->B > 0 && d->HW > 0, "%s: B and HW must be positive", what);
    ML_REQUIRE(d->C >= 4 && d->C <= SB_MAX_C && d->C % V == 0, "%s: C = %d must be a multiple of %d in 4..%d", what, d->C,
               V, SB_MAX_C);
    ML_REQUIRE(d->Hd >= 1 && d->Hd <= SB_MAX_HD, "%s: Hd = %d outside 1..%d", what, d->Hd, SB_MAX_HD);
    ML_REQUIRE((int64_t)d->B * d->HW * d->C < ((int64_t)1 << 40), "%s: tensor too large", what);
    const int64_t ntail = sb_ntail(d->HW, d->C), npool = sb_npool(d->HW, d->C);
    ML_REQUIRE((int64_t)d->B * ntail < ((int64_t)1 << 31) && (int64_t)d->B * npool < ((int64_t)1 << 31),
               "%s: too many blocks", what);
    ML_REQUIRE(ml_aligned16(d->c3) && ml_aligned16(d->residual) && ml_aligned16(d->out),
               "%s: c3, residual and out must be 16-byte aligned", what);
    ML_REQUIRE((((uintptr_t)d->w1 | (uintptr_t)d->b1 | (uintptr_t)d->w2 | (uintptr_t)d->b2) & 3u) == 0,
               "%s: misaligned FC weights", what);
    ML_REQUIRE(workspace && ml_aligned16(workspace), "%s: need a 16-byte aligned workspace", what);
    const int64_t need = ml_se_bottleneck_workspace_bytes(d->B, d->HW, d->C);
    ML_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes, need %lld", what, (long long)workspace_bytes,
               (long long)need);
    // out may be the very buffer of c3 or of residual (each element is read and written by one thread), nothing else
    const int64_t bytes = (int64_t)d->B * d->HW * d->C * (int64_t)sizeof(T);
    ML_REQUIRE(ml_add_or_disjoint(d->out, d->c3, bytes) && ml_add_or_disjoint(d->out, d->residual, bytes),
               "%s: out partially overlaps an input", what);
    ML_REQUIRE(!ml_ranges_overlap(workspace, need, d->out, bytes), "%s: the workspace overlaps out", what);
    SbArgs A;
    A.c3 = d->c3;
    A.residual = d->residual;
    A.w1 = d->w1;
    A.b1 = d->b1;
    A.w2 = d->w2;
    A.b2 = d->b2;
    A.out = d->out;
    A.slabs = reinterpret_cast<double *>(workspace);
    A.gate = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + (int64_t)d->B * npool * d->C * 8);
    A.B = d->B;
    A.HW = d->HW;
    A.C = d->C;
    A.Hd = d->Hd;
    A.npool = (int)npool;
    A.pool_chunk = (int)sb_pool_chunk(d->HW, d->C);
    A.ntail = (int)ntail;
    A.tail_chunk = (int)sb_tail_chunk(d->C);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sb_pool<T>, dim3((unsigned)(d->B * npool)), dim3(SB_TPB), 0, s, A);
    hipLaunchKernelGGL(sb_gate, dim3((unsigned)d->B), dim3(SB_GATE_TPB), 0, s, A);
    hipLaunchKernelGGL(sb_tail<T>, dim3((unsigned)(d->B * ntail)), dim3(SB_TPB), 0, s, A);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

}  // namespace

extern "C" int64_t ml_se_bottleneck_workspace_bytes(int32_t B, int32_t HW, int32_t C) {
    if (B <= 0 || HW <= 0 || C <= 0 || C > SB_MAX_C) return 0;
    return (int64_t)B * sb_npool(HW, C) * C * (int64_t)sizeof(double) + 2 * (int64_t)B * C * (int64_t)sizeof(float);
}

extern "C" int ml_se_bottleneck_f32(const ml_se_bottleneck_desc *d, void *workspace, int64_t workspace_bytes, void *stream) {
    return se_bottleneck_launch<float>("se_bottleneck_f32", d, workspace, workspace_bytes, stream);
}

extern "C" int ml_se_bottleneck_f16(const ml_se_bottleneck_desc *d, void *workspace, int64_t workspace_bytes, void *stream) {
    return se_bottleneck_launch<_Float16>("se_bottleneck_f16", d, workspace, workspace_bytes, stream);
}
