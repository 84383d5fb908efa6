// The ResNeXt stem in ONE pass: ZeroPadding2D(3) + Conv 7x7 stride 2 (64 filters, BatchNorm folded) + ReLU +
// ZeroPadding2D(1) + MaxPooling2D(3, stride 2), fp32 NHWC4 image in, pooled map out (reference engine/backbone/ResNext.py:343-352;
// thirdparty/classification_models/models/resnext.py:193-197).  One body, one policy per conv math, each BIT-IDENTICAL to the
// generic kernel in that math followed by maxpool3x3s2 (a caller that asks for the C1 tap gets that unfused pair):
//   stem_pool_f32_kernel  exact fp32 products (ML_MATH_F32), fp32 pooled map;
//   stem_pool_x3_kernel   split-operand products on the f16 pipe (ML_MATH_F32X3), fp32 pooled map;
//   stem_pool_h_kernel    image and weights rounded to half (ML_MATH_F16), ONE rounding to half: the fp16-storage stem.
//
// Why: as two launches the stem's un-pooled output is written and read back by the pool -- 537 MB of fp32 at 8 x 1024^2, 839 MB
// of half at 16 x 1280^2 -- and the generic kernel's row-span packing pads a kernel row of 7 pixels x 3 channels to 8 x 4 = 32
// (K = 224 for 147 real taps).  Here
//   * the conv output lives in LDS only: a block computes the 9 x 33 conv pixels a 4 x 16 pooled tile needs (+16 % for the
//     pool's one-pixel halo), pools them from LDS and stores 64 pooled pixels x 64 channels;
//   * transposed product: A = weights (rows = output channels), B = pixels, so a lane ends up with runs of four consecutive
//     channels of ITS conv pixel -> vector writes into the conv tile;
//   * K order and products are the generic kernel's, bias first, ReLU last.  f32: its v_mfma_f32_32x32x2_f32 number j of
//     k-step ks of a kernel row multiplies (pixel 2 ks, channel j) and (pixel 2 ks + 1, channel j); channel 3 has zero weights
//     -- dropped, it adds +0 -- and pixel 7 too (its partner's products stay): 12 MFMAs per kernel row instead of 16, the B
//     operand one float per lane read from a 3-channel input tile at an immediate offset.  x3 / h: a 16-deep
//     v_mfma_f32_32x32x16_f16 step is half a kernel row, lane half q two of its pixels (one ds_read_b128 of a half NHWC4
//     tile).  x3 splits every image value ONCE on its way into LDS (split_hi_lo_pair: hi = RNE half, lo = (x - hi) 2^11), the
//     weights arrive split (masklab_hip.ops.DeviceConv.wgt_x3); per step hi.hi -> the sums from the bias, then act-hi.wgt-lo
//     and act-lo.wgt-hi -> a cross-term chain, folded in once at the end (2^-11);
//   * a block walks a run of pooled tiles of its row with its weights resident in registers, the next tile's image pixels
//     fetched into registers under the current tile's MFMAs (two barriers per tile); wave w multiplies output channels
//     32 (w >> 1) .. + 31 by every other set of 32 conv pixels -- f32 / x3 two sets at a time (two independent chains).
// Measured: f32 507 us at 8 x 1024^2 against 545 + 143 for the two launches -- 71 % of the MFMA time of the chains it issues
// (8 192 tiles x 20 x 84 MFMAs of 64 cycles = 0.36 ms on 1 024 SIMDs), the same fraction the generic kernel reaches on this
// K = 7-chunk problem; pool, deposit and the two barriers per tile are not covered by matrix work with one block per CU.
// x3 249 us against 336 + 146 at 8 x 1024^2; h 0.35 ms against 0.78 + 0.23 at 16 x 1280^2, where the conv itself is ~90 us of
// fp16 MFMA.  HBM traffic (f32 / x3, 8 x 1024^2) 100 MB in + 134 MB out.
// Measured and not kept (f32): eight waves (two per SIMD, 5 x 16 pooled tile, one chain per wave, runs of two tiles per block):
// 548 us; the B operands read from LDS one kernel row ahead of their MFMAs (pinned with sched_barrier): 524 us -- the LDS
// latency is not what the chains wait for; runs of two tiles per block instead of whole rows: 582 us (the prologue).
#include <type_traits>
#include "common.h"

namespace {

constexpr int PTH = 4, PTW = 16;                  // pooled tile
constexpr int NT = 256;                           // threads: 4 waves, one per SIMD
constexpr int CR = 2 * PTH + 1, CC = 2 * PTW + 1; // conv pixels it needs: 9 x 33
constexpr int IR = 2 * (CR - 1) + 7;              // input rows: 23
constexpr int ICP = 2 * (CC - 1) + 8;             // input pixels per row: 72 (71 used + the zero-weight 8th tap pixel)
constexpr int NCONV = CR * CC;                    // 297
constexpr int NSETS = (NCONV + 31) / 32;          // 10 sets of 32 conv pixels: 5 per wave
constexpr int NIN = (IR * ICP + NT - 1) / NT;     // 7 input pixels per thread and tile
static_assert(NSETS == 10, "the wave -> set map below assumes 10 sets");

// ---- per-math policies: the input tile in LDS and its deposit, the weight fragments, the conv-tile element and the products.
// products(): `ip` = input pixel of kernel row 0, tap 0 for each set's conv pixel; `acc` arrives holding the bias and leaves
// holding the pre-ReLU conv value.

// exact fp32 products: the image tile as 3-channel pixels, the B operand one float per lane
struct StemF32 {
    typedef float Wgt;
    typedef float Conv;
    static constexpr bool PAIRED = true;                        // two sets (accumulator chains) at a time
    static constexpr int CPS = 68;                              // floats per conv pixel in LDS (64 + 4 pad: 272 B)
    static constexpr int IN_BYTES = IR * ICP * 3 * 4;           // 19 872
    // A operand of MFMA (ky, ks, j) = W[output channel 32 nt + p32][kernel row ky][pixel 2 ks + q][channel j], straight from
    // the generic kernel's row-span packing ([64][7 x 32]: 8 pixels x 4 channels per kernel row)
    float wv[7][4][3];
    __device__ __forceinline__ StemF32(const float *wgt, int nt, int p32, int q) {
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int j = 0; j < 3; ++j) wv[ky][ks][j] = wgt[(nt * 32 + p32) * 224 + ky * 32 + (2 * ks + q) * 4 + j];
    }
    __device__ __forceinline__ void deposit(char *lds, const f32x4 (&stage)[NIN], int tid) const {
        float *tin = reinterpret_cast<float *>(lds);                                        // [IR][ICP][3]
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
            const int i = tid + NT * j;
            if (i < IR * ICP) {
                tin[i * 3 + 0] = stage[j][0];
                tin[i * 3 + 1] = stage[j][1];
                tin[i * 3 + 2] = stage[j][2];
            }
        }
    }
    template <int NS>
    __device__ __forceinline__ void products(const char *lds, const int (&ip)[NS], int q, f32x16 (&acc)[NS]) const {
        const float *src[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) src[u] = reinterpret_cast<const float *>(lds) + (ip[u] + q) * 3;   // pixel q of the pair
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int u = 0; u < NS; ++u)
                        acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[ky][ks][j], src[u][(ky * ICP + 2 * ks) * 3 + j], acc[u], 0, 0, 0);
    }
};

// split-operand products: hi and lo half NHWC4 tiles, hi.hi into the sums, the two cross terms into a chain of their own
struct StemX3 {
    typedef _Float16 Wgt;
    typedef float Conv;
    static constexpr bool PAIRED = true;
    static constexpr int CPS = 68;
    static constexpr int IN_HALF = IR * ICP * 8;                // 13 248 per half tile (hi, lo)
    static constexpr int IN_BYTES = 2 * IN_HALF;
    // A fragments.  lane (m = p32, q): output channel 32 nt + m, k = 16 s + 8 q .. + 7 of kernel row s / 2 (hi), + 32 (lo)
    f16x8 wh[14], wl[14];
    __device__ __forceinline__ StemX3(const _Float16 *wgt, int nt, int p32, int q) {
#pragma unroll
        for (int s = 0; s < 14; ++s) {
            const _Float16 *row = wgt + ((nt * 32 + p32) * 7 + (s >> 1)) * 64 + (s & 1) * 16 + q * 8;
            wh[s] = *reinterpret_cast<const f16x8 *>(row);
            wl[s] = *reinterpret_cast<const f16x8 *>(row + 32);
        }
    }
    __device__ __forceinline__ void deposit(char *lds, const f32x4 (&stage)[NIN], int tid) const {
        _Float16 *tin_h = reinterpret_cast<_Float16 *>(lds);                                // [IR][ICP][4] hi halves
        _Float16 *tin_l = reinterpret_cast<_Float16 *>(lds + IN_HALF);                      // [IR][ICP][4] lo halves (x 2^11)
        const float neg_scale = -2048.f;
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
            const int i = tid + NT * j;
            if (i < IR * ICP) {
                unsigned h0, l0, h1, l1;
                split_hi_lo_pair(stage[j][0], stage[j][1], neg_scale, h0, l0);
                split_hi_lo_pair(stage[j][2], stage[j][3], neg_scale, h1, l1);
                *reinterpret_cast<u32x2 *>(tin_h + i * 4) = u32x2{h0, h1};
                *reinterpret_cast<u32x2 *>(tin_l + i * 4) = u32x2{l0, l1};
            }
        }
    }
    template <int NS>
    __device__ __forceinline__ void products(const char *lds, const int (&ip)[NS], int q, f32x16 (&acc)[NS]) const {
        const _Float16 *tin_h = reinterpret_cast<const _Float16 *>(lds), *tin_l = reinterpret_cast<const _Float16 *>(lds + IN_HALF);
        int soff[NS];                                                   // halves: kernel row 0, pixels 2 q, 2 q + 1
        f32x16 acx[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            soff[u] = (ip[u] + 2 * q) * 4;
#pragma unroll
            for (int e = 0; e < 16; ++e) acx[u][e] = 0.f;
        }
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                f16x8 xh[NS], xl[NS];
#pragma unroll
                for (int u = 0; u < NS; ++u) {
                    xh[u] = *reinterpret_cast<const f16x8 *>(tin_h + soff[u] + (ky * ICP + 4 * s2) * 4);
                    xl[u] = *reinterpret_cast<const f16x8 *>(tin_l + soff[u] + (ky * ICP + 4 * s2) * 4);
                }
#pragma unroll
                for (int u = 0; u < NS; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[ky * 2 + s2], xh[u], acc[u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < NS; ++u) acx[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[ky * 2 + s2], xh[u], acx[u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < NS; ++u) acx[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[ky * 2 + s2], xl[u], acx[u], 0, 0, 0);
            }
        // cross terms folded in (units of 2^-11)
#pragma unroll
        for (int u = 0; u < NS; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[u][e] = fmaf(acx[u][e], 0x1p-11f, acc[u][e]);
    }
};

// fp16 operands: the image rounded to half on its way into LDS, one chain per set, the conv tile in half (one rounding)
struct StemH {
    typedef _Float16 Wgt;
    typedef _Float16 Conv;
    static constexpr bool PAIRED = false;                       // one set at a time: 14 weight fragments (56 registers) leave
                                                                // room for the next tile's input in registers
    static constexpr int CPS = 72;                              // halves per conv pixel in LDS (64 + 8 pad: 144 B)
    static constexpr int IN_BYTES = IR * ICP * 8;               // 13 248
    // A fragments.  lane (m = p32, q): output channel 32 nt + m, k = 16 s + 8 q .. + 7
    f16x8 wv[14];
    __device__ __forceinline__ StemH(const _Float16 *wgt, int nt, int p32, int q) {
#pragma unroll
        for (int s = 0; s < 14; ++s) wv[s] = *reinterpret_cast<const f16x8 *>(wgt + (nt * 32 + p32) * 224 + s * 16 + q * 8);
    }
    __device__ __forceinline__ void deposit(char *lds, const f32x4 (&stage)[NIN], int tid) const {
        _Float16 *tin = reinterpret_cast<_Float16 *>(lds);                                  // [IR][ICP][4]
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
            const int i = tid + NT * j;
            if (i < IR * ICP)
                *reinterpret_cast<f16x4 *>(tin + i * 4) = f16x4{(_Float16)stage[j][0], (_Float16)stage[j][1], (_Float16)stage[j][2], (_Float16)stage[j][3]};
        }
    }
    template <int NS>
    __device__ __forceinline__ void products(const char *lds, const int (&ip)[NS], int q, f32x16 (&acc)[NS]) const {
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const _Float16 *src = reinterpret_cast<const _Float16 *>(lds) + (ip[u] + 2 * q) * 4;   // pixels 2 q, 2 q + 1
#pragma unroll
            for (int ky = 0; ky < 7; ++ky) {
                f16x8 xv[2];                                            // a kernel row's two steps: both reads in flight
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) xv[s2] = *reinterpret_cast<const f16x8 *>(src + (ky * ICP + 4 * s2) * 4);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wv[ky * 2 + s2], xv[s2], acc[u], 0, 0, 0);
            }
        }
    }
};

template <class Math>
constexpr int STEM_LDS = Math::IN_BYTES + NSETS * 32 * Math::CPS * (int)sizeof(typename Math::Conv);   // 106 912 / 113 536 / 59 328

template <class Math>
__device__ __forceinline__ void stem_pool_body(const float *img, const typename Math::Wgt *wgt, const float *bias,
                                               typename Math::Conv *out, int H, int W, int Hc, int Wc, int Hp, int Wp,
                                               int tiles_x, int seg) {
    typedef typename Math::Conv CT;
    typedef CT CTx4 __attribute__((ext_vector_type(4)));
    constexpr int V = 16 / sizeof(CT), NG = 64 / V;                     // the pool's 16-byte runs: V channels, NG per pixel
    typedef CT CTxV __attribute__((ext_vector_type(V)));
    constexpr int CPS = Math::CPS;
    extern __shared__ __align__(16) char lds[];
    CT *tconv = reinterpret_cast<CT *>(lds + Math::IN_BYTES);           // [NSETS * 32][CPS]; the input tile before it

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p32 = lane & 31, q = lane >> 5;
    const int ty = blockIdx.x, b = blockIdx.y;
    const int py0 = ty * PTH;
    const int cy0 = 2 * py0 - 1;                                        // conv row of tile-local row 0
    const int iy0 = 2 * cy0 - 3;                                        // input row of tile-local row 0
    const int nt = wave >> 1, s0 = wave & 1;                            // sets s0, s0 + 2, .. + 8 against channels 32 nt ..

    const Math m(wgt, nt, p32, q);
    // bias of the channels this lane's accumulator registers hold: 32 nt + (e & 3) + 8 (e >> 2) + 4 q
    float bv[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) bv[e] = bias ? bias[nt * 32 + (e & 3) + 8 * (e >> 2) + 4 * q] : 0.f;

    // ---- this thread's share of an input tile: pixels tid + 256 j of the [IR][ICP] grid
    int in_c[NIN];
    long long in_off[NIN];                                              // float offset of (row, column 0 of the image), -1: zeros
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
        const int i = tid + NT * j;
        const int in_r = i / ICP;
        in_c[j] = i - in_r * ICP;
        const int iy = iy0 + in_r;
        const bool row_ok = i < IR * ICP && (unsigned)iy < (unsigned)H;
        in_off[j] = row_ok ? ((long long)(b * H + iy) * W) * 4 : -1;
    }
    f32x4 stage[NIN];
    auto fetch = [&](int tx) __attribute__((always_inline)) {         // global -> registers (zeros outside the image)
        const int ix0 = 2 * (2 * tx * PTW - 1) - 3;
#pragma unroll
        for (int j = 0; j < NIN; ++j) {
            const int ix = ix0 + in_c[j];
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (in_off[j] >= 0 && (unsigned)ix < (unsigned)W) v = *reinterpret_cast<const f32x4 *>(img + in_off[j] + (long long)ix * 4);
            stage[j] = v;
        }
    };
    // NS sets of 32 conv pixels (sa, sa + 2, ..) against this wave's 32 output channels
    auto conv_sets = [&](auto nc, int sa, int cx0) __attribute__((always_inline)) {
        constexpr int NS = decltype(nc)::value;
        int ip[NS];
        f32x16 acc[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const int cp = min((sa + 2 * u) * 32 + p32, NCONV - 1);     // (the last set's spare lanes recompute pixel 296)
            const int cyl = cp / CC, cxl = cp - cyl * CC;
            ip[u] = (2 * cyl) * ICP + 2 * cxl;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[u][e] = bv[e];
        }
        m.template products<NS>(lds, ip, q, acc);
        // ReLU; conv pixels outside the conv map are the pool's zero padding
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const int s = sa + 2 * u;
            const int cp = min(s * 32 + p32, NCONV - 1);
            const int cyl = cp / CC, cxl = cp - cyl * CC;
            const int cy = cy0 + cyl, cx = cx0 + cxl;
            const bool inside = (unsigned)cy < (unsigned)Hc && (unsigned)cx < (unsigned)Wc;
            CT *dst = tconv + (s * 32 + p32) * CPS + nt * 32 + 4 * q;
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
                CTx4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = inside ? (CT)fmaxf(acc[u][4 * e4 + e], 0.f) : (CT)0.f;
                *reinterpret_cast<CTx4 *>(dst + 8 * e4) = v;
            }
        }
    };

    // this block's run of pooled tiles in its row: seg of them (the launcher cuts rows so that blocks are many and short)
    const int tx_begin = blockIdx.z * seg, tx_end = min(tiles_x, tx_begin + seg);
    fetch(tx_begin);
    m.deposit(lds, stage, tid);
    __syncthreads();
    for (int tx = tx_begin; tx < tx_end; ++tx) {
        const int px0 = tx * PTW;
        const int cx0 = 2 * px0 - 1;
        if (tx + 1 < tx_end) fetch(tx + 1);                             // the next tile's pixels fly under this tile's MFMAs

        // ---- conv: set s = conv pixels 32 s .. + 31 of the 9 x 33 region (row-major); this wave: s0, s0 + 2, ... (5 sets)
        if constexpr (Math::PAIRED) {
            conv_sets(std::integral_constant<int, 2>{}, s0, cx0);
            conv_sets(std::integral_constant<int, 2>{}, s0 + 4, cx0);
            conv_sets(std::integral_constant<int, 1>{}, s0 + 8, cx0);
        } else {
            for (int s = s0; s < NSETS; s += 2) conv_sets(std::integral_constant<int, 1>{}, s, cx0);
        }
        __syncthreads();                                                // conv tile complete; every wave is done reading the input tile

        // ---- 3 x 3 stride-2 max over the conv tile: 64 pooled pixels x NG runs of V channels
        for (int i = tid; i < PTH * PTW * NG; i += NT) {
            const int cg = i & (NG - 1), pp = i / NG;
            const int ppy = pp / PTW, ppx = pp - ppy * PTW;
            const int oy = py0 + ppy, ox = px0 + ppx;
            if (oy >= Hp || ox >= Wp) continue;
            CTxV mx = *reinterpret_cast<const CTxV *>(tconv + ((2 * ppy) * CC + 2 * ppx) * CPS + cg * V);
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    if (dy == 0 && dx == 0) continue;
                    const CTxV v = *reinterpret_cast<const CTxV *>(tconv + ((2 * ppy + dy) * CC + 2 * ppx + dx) * CPS + cg * V);
#pragma unroll
                    for (int k = 0; k < V; ++k) mx[k] = v[k] > mx[k] ? v[k] : mx[k];
                }
            *reinterpret_cast<CTxV *>(out + ((long long)(b * Hp + oy) * Wp + ox) * 64 + cg * V) = mx;
        }
        if (tx + 1 < tx_end) m.deposit(lds, stage, tid);                // (the input tile is free since the barrier above)
        __syncthreads();                                                // next input tile visible; pool done with `tconv`
    }
}

__global__ void __launch_bounds__(NT, 1)
stem_pool_f32_kernel(const float *__restrict__ img, const float *__restrict__ wgt, const float *__restrict__ bias,
                     float *__restrict__ out, int H, int W, int Hc, int Wc, int Hp, int Wp, int tiles_x, int seg) {
    stem_pool_body<StemF32>(img, wgt, bias, out, H, W, Hc, Wc, Hp, Wp, tiles_x, seg);
}

__global__ void __launch_bounds__(NT, 1)
stem_pool_x3_kernel(const float *__restrict__ img, const _Float16 *__restrict__ wgt, const float *__restrict__ bias,
                    float *__restrict__ out, int H, int W, int Hc, int Wc, int Hp, int Wp, int tiles_x, int seg) {
    stem_pool_body<StemX3>(img, wgt, bias, out, H, W, Hc, Wc, Hp, Wp, tiles_x, seg);
}

__global__ void __launch_bounds__(NT)
stem_pool_h_kernel(const float *__restrict__ img, const _Float16 *__restrict__ wgt, const float *__restrict__ bias,
                   _Float16 *__restrict__ out, int H, int W, int Hc, int Wc, int Hp, int Wp, int tiles_x, int seg) {
    stem_pool_body<StemH>(img, wgt, bias, out, H, W, Hc, Wc, Hp, Wp, tiles_x, seg);
}

template <class Math>
int stem_pool_launch(void (*kernel)(const float *, const typename Math::Wgt *, const float *, typename Math::Conv *, int, int,
                                    int, int, int, int, int, int),
                     const char *name, const float *image, const void *wgt, const float *bias, void *out, int B, int H, int W,
                     int Hp, int Wp, void *stream) {
    constexpr bool wgt_scalar = std::is_same<typename Math::Wgt, float>::value;   // the f32 weights are read a float at a time
    ML_REQUIRE(image && wgt && out, "%s: null pointer", name);
    ML_REQUIRE(B > 0 && B < 65536 && H > 0 && W > 0, "%s: bad dims", name);
    ML_REQUIRE(ml_aligned16(image) && (wgt_scalar || ml_aligned16(wgt)) && ml_aligned16(out), "%s: %s must be 16-byte aligned",
               name, wgt_scalar ? "image and output" : "pointers");
    const int Hc = (H + 6 - 7) / 2 + 1, Wc = (W + 6 - 7) / 2 + 1;       // ZeroPadding2D(3) + 7x7 stride 2 'valid'
    ML_REQUIRE(Hp == (Hc + 2 - 3) / 2 + 1 && Wp == (Wc + 2 - 3) / 2 + 1,
               "%s: output must be [B, %d, %d, 64] (ZeroPadding2D(1) + MaxPooling2D(3, 2))", name, (Hc + 2 - 3) / 2 + 1,
               (Wc + 2 - 3) / 2 + 1);
    ML_REQUIRE((long long)B * H * W < (1ll << 31), "%s: too many pixels", name);
    static std::atomic<unsigned long long> lds_ok{0};                   // one per instantiation: per kernel
    if (int rc = ml_ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), STEM_LDS<Math>, lds_ok, name)) return rc;
    const int tiles_y = (Hp + PTH - 1) / PTH, tiles_x = (Wp + PTW - 1) / PTW;
    // a block keeps its weights in registers over `seg` tiles of a row: whole rows when that gives two blocks per CU or more
    // (its prologue -- 84 strided weight loads per lane in f32 -- wants many tiles behind it: runs of 2 tiles measured 582 us
    // against 507 for whole rows at 8 x 1024^2), shorter runs only for launches that would otherwise leave CUs empty
    int seg = tiles_x;
    while (seg > 1 && (long long)tiles_y * B * ((tiles_x + seg - 1) / seg) < 2ll * ml_resident_blocks(1)) seg = (seg + 1) / 2;
    hipLaunchKernelGGL(kernel, dim3(tiles_y, B, (tiles_x + seg - 1) / seg), dim3(NT), STEM_LDS<Math>, (hipStream_t)stream, image,
                       reinterpret_cast<const typename Math::Wgt *>(wgt), bias, reinterpret_cast<typename Math::Conv *>(out), H, W,
                       Hc, Wc, Hp, Wp, tiles_x, seg);
    ML_CHECK_LAUNCH(name);
    return ML_OK;
}

}  // namespace

extern "C" int ml_stem7x7s2_pool_f32(const float *image, const float *wgt, const float *bias, float *out, int32_t B, int32_t H,
                                     int32_t W, int32_t Hp, int32_t Wp, void *stream) {
    return stem_pool_launch<StemF32>(stem_pool_f32_kernel, "stem7x7s2_pool_f32", image, wgt, bias, out, B, H, W, Hp, Wp, stream);
}

extern "C" int ml_stem7x7s2_pool_x3(const float *image, const void *wgt_x3, const float *bias, float *out, int32_t B, int32_t H,
                                    int32_t W, int32_t Hp, int32_t Wp, void *stream) {
    return stem_pool_launch<StemX3>(stem_pool_x3_kernel, "stem7x7s2_pool_x3", image, wgt_x3, bias, out, B, H, W, Hp, Wp, stream);
}

extern "C" int ml_stem7x7s2_pool_f16(const float *image, const void *wgt_h, const float *bias, void *out, int32_t B, int32_t H,
                                     int32_t W, int32_t Hp, int32_t Wp, void *stream) {
    return stem_pool_launch<StemH>(stem_pool_h_kernel, "stem7x7s2_pool", image, wgt_h, bias, out, B, H, W, Hp, Wp, stream);
}
