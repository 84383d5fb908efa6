// Tail of an SE-ResNet pre-activation basic block (thirdparty resnet.py residual_conv_block :60-109 with ChannelSE,
// _common_blocks.py:88-119) in one launch pair, and the BatchNorm + ReLU of a unit's input on its own:
//   GATE:    g = sigmoid(W2 relu(W1 mean_hw(x) + b1) + b2)       (ChannelSE: two 1x1 convs with bias)
//            y = x * g + shortcut                                (Multiply, then the residual Add; no ReLU after it)
//            out_act = relu(y * scale + shift)                   (the NEXT unit's bn1 + relu1, or the final bn1 + relu1)
//            out_y   = y                                         (only when the next unit takes y as its identity shortcut)
//   BN_RELU: out_act = relu(x * scale + shift)                   (the pooled stem output into stage1_unit1)
// GATE runs two kernels:
//   1. se_residual_pool: block (sample, pool chunk) sums its chunk's channels in fp64, in a fixed order, and stores them as
//      the chunk's slab [C] doubles in the workspace.  A pool chunk is a whole number of tail chunks, sized so that a
//      sample has at most min(64, 4096 / C) slabs: what every tail block re-reads (<= 32 KB) stays small next to the
//      256 KB of tensor it streams.
//   2. se_residual_tail: block (sample, tail chunk of 16384 / C pixels: 256 at C = 64, 32 at C = 512) adds its sample's
//      slabs in one fixed order, evaluates the two FC layers in fp32 in LDS, then streams its chunk: x and shortcut read
//      once, out_act (and out_y) written once.  Chunks are sized in elements, not pixels, so that the small deep maps
//      (17 x 30 x 512 at the serving size) still spread over some blocks.
// No atomics: every sum has one fixed order that depends on neither the batch size nor scheduling, so eager launches,
// graph replay and image k of a batch against image k alone give the same bits.
#include "common.h"
#include "ranges.h"

namespace {

constexpr int SR_TPB = 256;
constexpr int SR_CHUNK_ELEMS = 16384;  // elements per tail block (pixels = 16384 / C)
constexpr int SR_SLAB_ELEMS = 4096;    // slab elements (pool chunks x C) per sample at most ...
constexpr int SR_MAX_SLABS = 64;       // ... and pool chunks per sample at most
constexpr int SR_MAX_C = 512;
constexpr int SR_MAX_HD = 32;

struct SrArgs {
    const float *x, *shortcut, *w1, *b1, *w2, *b2, *scale, *shift;
    float *out_act, *out_y;
    double *slabs;             // [B][npool][C]
    int HW, C, Hd, npool, pool_chunk, ntail, tail_chunk;
};

__device__ __forceinline__ f32x4 ld4(const float *p, long long off) { return *reinterpret_cast<const f32x4 *>(p + off); }
__device__ __forceinline__ void st4(float *p, long long off, const f32x4 v) { *reinterpret_cast<f32x4 *>(p + off) = v; }

__global__ void __launch_bounds__(SR_TPB) se_residual_pool(const SrArgs A) {
    __shared__ double red[SR_TPB * 4];
    const int n = blockIdx.x / A.npool, k = blockIdx.x % A.npool;
    const int C = A.C, CV = C / 4, rpi = SR_TPB / CV;
    const int t = threadIdx.x, r = t / CV, cv = t % CV;
    const int p0 = k * A.pool_chunk, p1 = min(A.HW, p0 + A.pool_chunk);
    if (r < rpi) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        const long long base = (long long)n * A.HW * C + cv * 4;
#pragma unroll 4
        for (int p = p0 + r; p < p1; p += rpi) {
            const f32x4 v = ld4(A.x, base + (long long)p * C);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += (double)v[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) red[r * C + cv * 4 + e] = acc[e];
    }
    __syncthreads();
    double *slab = A.slabs + ((long long)n * A.npool + k) * C;
    for (int c = t; c < C; c += SR_TPB) {
        double s = 0.0;
        for (int i = 0; i < rpi; ++i) s += red[i * C + c];
        slab[c] = s;
    }
}

template <bool GATE, bool DUAL>
__global__ void __launch_bounds__(SR_TPB) se_residual_tail(const SrArgs A) {
    __shared__ float gate[SR_MAX_C];
    const int n = blockIdx.x / A.ntail, k = blockIdx.x % A.ntail;
    const int C = A.C, CV = C / 4, rpi = SR_TPB / CV;
    const int t = threadIdx.x;
    if (GATE) {
        __shared__ double part[SR_TPB];
        __shared__ float mean[SR_MAX_C], hpart[8][SR_MAX_HD], hid[SR_MAX_HD];
        // the sample's channel sums: slab i goes to part q = i % Q, the Q parts are then added in order
        const double *slab = A.slabs + (long long)n * A.npool * C;
        const double inv = 1.0 / (double)A.HW;
        const int Q = C >= SR_TPB ? 1 : SR_TPB / C;
        if (Q == 1) {
            for (int c = t; c < C; c += SR_TPB) {
                double s = 0.0;
                for (int i = 0; i < A.npool; ++i) s += slab[(long long)i * C + c];
                mean[c] = (float)(s * inv);
            }
        } else {
            if (t < Q * C) {
                const int c = t % C, q = t / C;
                double s = 0.0;
                for (int i = q; i < A.npool; i += Q) s += slab[(long long)i * C + c];
                part[t] = s;
            }
            __syncthreads();
            for (int c = t; c < C; c += SR_TPB) {
                double s = 0.0;
                for (int q = 0; q < Q; ++q) s += part[q * C + c];
                mean[c] = (float)(s * inv);
            }
        }
        __syncthreads();
        // FC 1 (bias, relu): hidden unit j = t % 32, its C-sum cut into eight fixed parts (t / 32), added in order
        {
            const int j = t & 31, q = t >> 5, cq = (C + 7) / 8;
            if (j < A.Hd) {
                float a = 0.f;
                const int c1 = min(C, (q + 1) * cq);
                for (int c = q * cq; c < c1; ++c) a = fmaf(mean[c], A.w1[c * A.Hd + j], a);
                hpart[q][j] = a;
            }
        }
        __syncthreads();
        if (t < A.Hd) {
            float a = hpart[0][t];
#pragma unroll
            for (int q = 1; q < 8; ++q) a += hpart[q][t];
            hid[t] = fmaxf(a + A.b1[t], 0.f);
        }
        __syncthreads();
        // FC 2 (bias, sigmoid)
        for (int c = t; c < C; c += SR_TPB) {
            float a = 0.f;
            for (int j = 0; j < A.Hd; ++j) a = fmaf(hid[j], A.w2[j * C + c], a);
            gate[c] = 1.f / (1.f + expf(-(a + A.b2[c])));
        }
        __syncthreads();
    }
    const int r = t / CV, cv = t % CV;
    if (r >= rpi) return;
    const f32x4 s = ld4(A.scale, cv * 4), h = ld4(A.shift, cv * 4);
    f32x4 g = {1.f, 1.f, 1.f, 1.f};
    if (GATE) g = (f32x4){gate[cv * 4], gate[cv * 4 + 1], gate[cv * 4 + 2], gate[cv * 4 + 3]};
    const int p0 = k * A.tail_chunk, p1 = min(A.HW, p0 + A.tail_chunk);
    const long long base = (long long)n * A.HW * C + cv * 4;
#pragma unroll 4
    for (int p = p0 + r; p < p1; p += rpi) {
        const long long off = base + (long long)p * C;
        f32x4 y = ld4(A.x, off);
        if (GATE) {
            const f32x4 sc = ld4(A.shortcut, off);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = __fadd_rn(__fmul_rn(y[e], g[e]), sc[e]);   // Multiply, then Add
        }
        f32x4 a;
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = fmaxf(fmaf(y[e], s[e], h[e]), 0.f);
        st4(A.out_act, off, a);
        if (DUAL) st4(A.out_y, off, y);
    }
}

int64_t sr_tail_chunk(int32_t C) { return SR_CHUNK_ELEMS / C; }
int64_t sr_ntail(int32_t HW, int32_t C) { return ((int64_t)HW + sr_tail_chunk(C) - 1) / sr_tail_chunk(C); }
int64_t sr_pool_chunk(int32_t HW, int32_t C) {
    const int64_t max_slabs = C >= SR_SLAB_ELEMS / SR_MAX_SLABS ? SR_SLAB_ELEMS / C : SR_MAX_SLABS;   // C <= SR_MAX_C
    return sr_tail_chunk(C) * ((sr_ntail(HW, C) + max_slabs - 1) / max_slabs);
}
int64_t sr_npool(int32_t HW, int32_t C) { return ((int64_t)HW + sr_pool_chunk(HW, C) - 1) / sr_pool_chunk(HW, C); }

}  // namespace

extern "C" int64_t ml_se_residual_workspace_bytes(int32_t B, int32_t HW, int32_t C) {
    if (B <= 0 || HW <= 0 || C <= 0) return 0;
    if (C > SR_MAX_C) return 0;
    return (int64_t)B * sr_npool(HW, C) * C * (int64_t)sizeof(double);
}

extern "C" int ml_se_residual_f32(const ml_se_residual_desc *d, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *what = "se_residual_f32";
    ML_REQUIRE(d, "%s: null descriptor", what);
    ML_REQUIRE(d->mode == ML_SE_RES_GATE || d->mode == ML_SE_RES_BN_RELU, "%s: unknown mode %d", what, d->mode);
    const bool gate = d->mode == ML_SE_RES_GATE;
    ML_REQUIRE(d->x && d->out_act && d->scale && d->shift, "%s: x, out_act, scale and shift are required", what);
    ML_REQUIRE(d->B > 0 && d->HW > 0, "%s: B and HW must be positive", what);
    ML_REQUIRE(d->C >= 4 && d->C <= SR_MAX_C && d->C % 4 == 0, "%s: C = %d must be a multiple of 4 in 4..%d", what, d->C,
               SR_MAX_C);
    ML_REQUIRE((int64_t)d->B * d->HW * d->C < ((int64_t)1 << 40), "%s: tensor too large", what);
    const int64_t ntail = sr_ntail(d->HW, d->C);
    ML_REQUIRE((int64_t)d->B * ntail < ((int64_t)1 << 31), "%s: too many blocks", what);
    ML_REQUIRE(ml_aligned16(d->x) && ml_aligned16(d->out_act) && ml_aligned16(d->scale) && ml_aligned16(d->shift),
               "%s: x, out_act, scale and shift must be 16-byte aligned", what);
    const int64_t bytes = (int64_t)d->B * d->HW * d->C * (int64_t)sizeof(float);
    if (gate) {
        ML_REQUIRE(d->shortcut && d->w1 && d->b1 && d->w2 && d->b2, "%s: GATE needs shortcut, w1, b1, w2 and b2", what);
        ML_REQUIRE(d->Hd >= 1 && d->Hd <= SR_MAX_HD, "%s: Hd = %d outside 1..%d", what, d->Hd, SR_MAX_HD);
        ML_REQUIRE(ml_aligned16(d->shortcut) && (!d->out_y || ml_aligned16(d->out_y)),
                   "%s: shortcut and out_y must be 16-byte aligned", what);
        ML_REQUIRE((((uintptr_t)d->w1 | (uintptr_t)d->b1 | (uintptr_t)d->w2 | (uintptr_t)d->b2) & 3u) == 0,
                   "%s: misaligned FC weights", what);
        ML_REQUIRE(workspace && ml_aligned16(workspace), "%s: need a 16-byte aligned workspace", what);
        const int64_t need = ml_se_residual_workspace_bytes(d->B, d->HW, d->C);
        ML_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes, need %lld", what, (long long)workspace_bytes,
                   (long long)need);
    } else {
        ML_REQUIRE(!d->shortcut && !d->out_y, "%s: BN_RELU takes no shortcut and writes no out_y", what);
    }
    // an output may be the very buffer of an input (each element is read and written by one thread), nothing else
    const void *ins[2] = {d->x, d->shortcut};
    const void *outs[2] = {d->out_act, d->out_y};
    for (const void *o : outs)
        for (const void *i : ins)
            ML_REQUIRE(ml_add_or_disjoint(o, i, bytes), "%s: an output partially overlaps an input", what);
    ML_REQUIRE(d->out_act != d->out_y && !ml_ranges_overlap(d->out_act, bytes, d->out_y, bytes),
               "%s: out_act and out_y overlap", what);
    SrArgs A;
    A.x = d->x;
    A.shortcut = d->shortcut;
    A.w1 = d->w1;
    A.b1 = d->b1;
    A.w2 = d->w2;
    A.b2 = d->b2;
    A.scale = d->scale;
    A.shift = d->shift;
    A.out_act = d->out_act;
    A.out_y = d->out_y;
    A.slabs = reinterpret_cast<double *>(workspace);
    A.HW = d->HW;
    A.C = d->C;
    A.Hd = gate ? d->Hd : 0;
    A.npool = (int)sr_npool(d->HW, d->C);
    A.pool_chunk = (int)sr_pool_chunk(d->HW, d->C);
    A.ntail = (int)ntail;
    A.tail_chunk = (int)sr_tail_chunk(d->C);
    hipStream_t s = (hipStream_t)stream;
    const dim3 tail_grid((unsigned)(d->B * ntail));
    if (gate) {
        hipLaunchKernelGGL(se_residual_pool, dim3((unsigned)(d->B * A.npool)), dim3(SR_TPB), 0, s, A);
        if (d->out_y)
            hipLaunchKernelGGL((se_residual_tail<true, true>), tail_grid, dim3(SR_TPB), 0, s, A);
        else
            hipLaunchKernelGGL((se_residual_tail<true, false>), tail_grid, dim3(SR_TPB), 0, s, A);
    } else {
        hipLaunchKernelGGL((se_residual_tail<false, false>), tail_grid, dim3(SR_TPB), 0, s, A);
    }
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}
