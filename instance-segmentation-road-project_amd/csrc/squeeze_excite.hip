// SqueezeExcite (reference engine/layers/misc.py:24-54) fused into one launch pair for several problems:
// GlobalAveragePooling2D -> Dense(C -> Hd, relu, no bias) -> Dense(Hd -> C, sigmoid, no bias) -> x * gate.
//   1. squeeze_excite_pool[_h]:  block (problem, sample, HW chunk) sums its chunk's channels in fp64, in a fixed order,
//      and stores them as the chunk's slab [C] doubles in the workspace.
//   2. squeeze_excite_scale[_h]: block (problem, sample, HW chunk) adds its sample's slabs in chunk order, divides by HW,
//      evaluates the two Dense layers in fp32 (C x Hd + Hd x C FMAs; mean, hidden and gate held in LDS), then scales its
//      chunk and stores it (a half store is rounded once).
// No atomics: every sum has one fixed order, so a result does not depend on scheduling (eager == graph replay, bit for bit).
// HBM-bound: x is read twice and written once; the slabs (B x chunks x C doubles) stay in L2.
#include "common.h"

namespace {

constexpr int SE_TPB = 256;
constexpr int SE_CHUNK = 256;          // pixels per block
constexpr int SE_MAX_C = 1024;
constexpr int SE_MAX_HD = 64;

struct SeProb {
    const void *x;
    void *out;
    const float *w1, *w2;
    double *slabs;             // [B][nch][C]
    const int *live;
    int B, HW, C, Hd, nch, live_period;
};
struct SeMulti {
    int n;
    int start[ML_SE_MAX_PROBLEMS + 1];
    SeProb p[ML_SE_MAX_PROBLEMS];
};

__device__ __forceinline__ bool se_dead(const SeProb &P, int n) {
    return P.live && (n % P.live_period) >= max(1, *P.live);
}

template <bool HALF> struct SeVec;
template <> struct SeVec<false> {
    static constexpr int W = 4;
    typedef f32x4 T;
    __device__ static void load(const void *p, long long off, float (&v)[4]) {
        const f32x4 x = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(p) + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = x[e];
    }
    __device__ static void store(void *p, long long off, const float (&v)[4]) {
        const f32x4 x = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(p) + off) = x;
    }
};
template <> struct SeVec<true> {
    static constexpr int W = 8;
    __device__ static void load(const void *p, long long off, float (&v)[8]) {
        const f16x8 x = *reinterpret_cast<const f16x8 *>(reinterpret_cast<const _Float16 *>(p) + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
    }
    __device__ static void store(void *p, long long off, const float (&v)[8]) {
        const f16x8 x = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3],
                         (_Float16)v[4], (_Float16)v[5], (_Float16)v[6], (_Float16)v[7]};
        *reinterpret_cast<f16x8 *>(reinterpret_cast<_Float16 *>(p) + off) = x;
    }
};

// block -> (problem, sample, chunk); false for a sample that does not exist (block-uniform)
__device__ __forceinline__ bool se_locate(const SeMulti &A, int &pi, int &n, int &k) {
    pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.start[pi + 1]) ++pi;
    const SeProb &P = A.p[pi];
    const int id = blockIdx.x - A.start[pi];
    n = id / P.nch;
    k = id % P.nch;
    return !se_dead(P, n);
}

template <bool HALF>
__device__ __forceinline__ void se_pool_body(const SeMulti &A) {
    constexpr int W = SeVec<HALF>::W;
    __shared__ double red[SE_TPB * W];
    int pi, n, k;
    if (!se_locate(A, pi, n, k)) return;
    const SeProb &P = A.p[pi];
    const int C = P.C, CV = C / W, rpi = SE_TPB / CV;
    const int t = threadIdx.x, r = t / CV, cv = t % CV;
    const int p0 = k * SE_CHUNK, p1 = min(P.HW, p0 + SE_CHUNK);
    if (r < rpi) {
        double acc[W];
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] = 0.0;
        const long long base = (long long)n * P.HW * C + cv * W;
        for (int p = p0 + r; p < p1; p += rpi) {
            float v[W];
            SeVec<HALF>::load(P.x, base + (long long)p * C, v);
#pragma unroll
            for (int e = 0; e < W; ++e) acc[e] += (double)v[e];
        }
#pragma unroll
        for (int e = 0; e < W; ++e) red[r * C + cv * W + e] = acc[e];
    }
    __syncthreads();
    double *slab = P.slabs + ((long long)n * P.nch + k) * C;
    for (int c = t; c < C; c += SE_TPB) {
        double s = 0.0;
        for (int i = 0; i < rpi; ++i) s += red[i * C + c];
        slab[c] = s;
    }
}

template <bool HALF>
__device__ __forceinline__ void se_scale_body(const SeMulti &A) {
    constexpr int W = SeVec<HALF>::W;
    __shared__ float mean[SE_MAX_C], gate[SE_MAX_C];
    __shared__ float hpart[SE_TPB / 64][SE_MAX_HD], hid[SE_MAX_HD];
    int pi, n, k;
    if (!se_locate(A, pi, n, k)) return;
    const SeProb &P = A.p[pi];
    const int C = P.C, Hd = P.Hd, CV = C / W, rpi = SE_TPB / CV;
    const int t = threadIdx.x;
    // the sample's channel means: its slabs in chunk order
    const double *slab = P.slabs + (long long)n * P.nch * C;
    const double inv = 1.0 / (double)P.HW;
    for (int c = t; c < C; c += SE_TPB) {
        double s = 0.0;
        for (int i = 0; i < P.nch; ++i) s += slab[(long long)i * C + c];
        mean[c] = (float)(s * inv);
    }
    __syncthreads();
    // Dense 1 (relu): hidden unit j = t % 64, its C-sum cut into four fixed quarters (one per wave), added in order
    {
        const int j = t & 63, q = t >> 6, cq = (C + 3) / 4;
        if (j < Hd) {
            float a = 0.f;
            const int c1 = min(C, (q + 1) * cq);
            for (int c = q * cq; c < c1; ++c) a = fmaf(mean[c], P.w1[c * Hd + j], a);
            hpart[q][j] = a;
        }
    }
    __syncthreads();
    if (t < Hd) hid[t] = fmaxf(((hpart[0][t] + hpart[1][t]) + hpart[2][t]) + hpart[3][t], 0.f);
    __syncthreads();
    // Dense 2 (sigmoid)
    for (int c = t; c < C; c += SE_TPB) {
        float a = 0.f;
        for (int j = 0; j < Hd; ++j) a = fmaf(hid[j], P.w2[j * C + c], a);
        gate[c] = 1.f / (1.f + expf(-a));
    }
    __syncthreads();
    const int r = t / CV, cv = t % CV;
    if (r >= rpi) return;
    float g[W];
#pragma unroll
    for (int e = 0; e < W; ++e) g[e] = gate[cv * W + e];
    const int p0 = k * SE_CHUNK, p1 = min(P.HW, p0 + SE_CHUNK);
    const long long base = (long long)n * P.HW * C + cv * W;
    for (int p = p0 + r; p < p1; p += rpi) {
        float v[W];
        SeVec<HALF>::load(P.x, base + (long long)p * C, v);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] *= g[e];
        SeVec<HALF>::store(P.out, base + (long long)p * C, v);
    }
}

__global__ void __launch_bounds__(SE_TPB) squeeze_excite_pool(const SeMulti A) { se_pool_body<false>(A); }
__global__ void __launch_bounds__(SE_TPB) squeeze_excite_pool_h(const SeMulti A) { se_pool_body<true>(A); }
__global__ void __launch_bounds__(SE_TPB) squeeze_excite_scale(const SeMulti A) { se_scale_body<false>(A); }
__global__ void __launch_bounds__(SE_TPB) squeeze_excite_scale_h(const SeMulti A) { se_scale_body<true>(A); }

int64_t se_chunks(int32_t HW) { return ((int64_t)HW + SE_CHUNK - 1) / SE_CHUNK; }

int se_run(const ml_se_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes, void *stream, bool half) {
    const char *what = half ? "squeeze_excite_f16" : "squeeze_excite_f32";
    const int W = half ? 8 : 4;
    ML_REQUIRE(descs && n >= 1 && n <= ML_SE_MAX_PROBLEMS, "%s: need 1..%d problems", what, ML_SE_MAX_PROBLEMS);
    ML_REQUIRE(workspace && ml_aligned16(workspace) && workspace_bytes > 0, "%s: need a 16-byte aligned workspace", what);
    SeMulti A;
    A.n = n;
    A.start[0] = 0;
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const ml_se_desc &d = descs[i];
        ML_REQUIRE(d.x && d.out && d.w1 && d.w2, "%s: problem %d: null pointer", what, i);
        ML_REQUIRE(d.B > 0 && d.HW > 0, "%s: problem %d: B and HW must be positive", what, i);
        ML_REQUIRE(d.C > 0 && d.C <= SE_MAX_C && d.C % W == 0, "%s: problem %d: C = %d must be a multiple of %d in 1..%d",
                   what, i, d.C, W, SE_MAX_C);
        ML_REQUIRE(d.Hd >= 1 && d.Hd <= SE_MAX_HD, "%s: problem %d: Hd = %d outside 1..%d", what, i, d.Hd, SE_MAX_HD);
        ML_REQUIRE(!d.live || (d.live_period > 0 && d.B % d.live_period == 0),
                   "%s: problem %d: live needs B %% live_period == 0", what, i);
        ML_REQUIRE(ml_aligned16(d.x) && ml_aligned16(d.out), "%s: problem %d: x / out must be 16-byte aligned", what, i);
        ML_REQUIRE(((uintptr_t)d.w1 & 3u) == 0 && ((uintptr_t)d.w2 & 3u) == 0, "%s: problem %d: misaligned weights", what, i);
        ML_REQUIRE((int64_t)d.B * d.HW * d.C < ((int64_t)1 << 40), "%s: problem %d: tensor too large", what, i);
        const int64_t nch = se_chunks(d.HW);
        const int64_t need = ml_squeeze_excite_workspace_bytes(d.B, d.HW, d.C);
        ML_REQUIRE(d.ws_offset >= 0 && d.ws_offset % 16 == 0 && d.ws_offset + need <= workspace_bytes,
                   "%s: problem %d: workspace slice [%lld, +%lld) outside the %lld-byte workspace or misaligned", what, i,
                   (long long)d.ws_offset, (long long)need, (long long)workspace_bytes);
        for (int j = 0; j < i; ++j) {
            const int64_t o = descs[j].ws_offset, e = o + ml_squeeze_excite_workspace_bytes(descs[j].B, descs[j].HW, descs[j].C);
            ML_REQUIRE(d.ws_offset + need <= o || e <= d.ws_offset, "%s: problems %d and %d share workspace", what, j, i);
        }
        blocks += (int64_t)d.B * nch;
        ML_REQUIRE(blocks < ((int64_t)1 << 31), "%s: too many blocks", what);
        SeProb &P = A.p[i];
        P.x = d.x;
        P.out = d.out;
        P.w1 = d.w1;
        P.w2 = d.w2;
        P.slabs = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + d.ws_offset);
        P.live = d.live;
        P.B = d.B;
        P.HW = d.HW;
        P.C = d.C;
        P.Hd = d.Hd;
        P.nch = (int)nch;
        P.live_period = d.live ? d.live_period : 1;
        A.start[i + 1] = (int)blocks;
    }
    hipStream_t s = (hipStream_t)stream;
    if (half) {
        hipLaunchKernelGGL(squeeze_excite_pool_h, dim3((unsigned)blocks), dim3(SE_TPB), 0, s, A);
        hipLaunchKernelGGL(squeeze_excite_scale_h, dim3((unsigned)blocks), dim3(SE_TPB), 0, s, A);
    } else {
        hipLaunchKernelGGL(squeeze_excite_pool, dim3((unsigned)blocks), dim3(SE_TPB), 0, s, A);
        hipLaunchKernelGGL(squeeze_excite_scale, dim3((unsigned)blocks), dim3(SE_TPB), 0, s, A);
    }
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

}  // namespace

extern "C" int64_t ml_squeeze_excite_workspace_bytes(int32_t B, int32_t HW, int32_t C) {
    if (B <= 0 || HW <= 0 || C <= 0) return 0;
    return (int64_t)B * se_chunks(HW) * C * (int64_t)sizeof(double);
}

extern "C" int ml_squeeze_excite_f32(const ml_se_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes,
                                     void *stream) {
    return se_run(descs, n, workspace, workspace_bytes, stream, false);
}

extern "C" int ml_squeeze_excite_f16(const ml_se_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes,
                                     void *stream) {
    return se_run(descs, n, workspace, workspace_bytes, stream, true);
}
