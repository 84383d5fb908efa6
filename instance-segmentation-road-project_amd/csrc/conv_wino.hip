// Winograd F(2x2,3x3) convolution on the gfx950 f32 matrix cores (v_mfma_f32_16x16x4_f32), ML_MATH_F32 only.
//
//   For the stride-1 "same" 3x3 convs of the heads (towers, FPN, semantic / decoder convs): an output 2x2 tile is
//   Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A with d_c the 4x4 input patch of channel c, so the 9 taps x Cin x Cout
//   multiplications of a 2x2 tile (36 per channel pair) become 16 (x2.25 fewer MFMAs).  The transforms hold only 0, +-1,
//   +-1/2 (F(2x2,3x3): Lavin & Gray 2016); the weight transform U = G g G^T is done once on the host in fp64 and rounded
//   once to fp32 (masklab_hip/packing.py: pack_winograd).  Per position p = 4a + b the 16 products are independent
//   GEMMs  M_p[tiles, Cout] = V_p[tiles, Cin] . U_p[Cin, Cout], accumulated over the whole K loop (no split-K).
//
//   Block = 256 threads = 4 waves, block tile = 64 Winograd tiles (flattened over image, tile row, tile column) x 32
//   output channels; wave w owns tiles 16w..16w+15 x the 32 channels x all 16 positions: 2 x 16 accumulators of the
//   16x16x4 MFMA = 128 registers, so the output transform runs in registers (a lane holds all 16 positions of its 4
//   tiles x 1 channel per 16-wide half).  K chunk = 8 input channels:
//     * the raw 4x4 patches of the block's 64 tiles, [tile][16 px][8 ch] + 4 floats pad per tile (conflict-free
//       b32 reads: lane (r, kq) hits bank 4r + kq), 33 KB; out-of-image taps are written as zeros;
//     * the transformed weights of the chunk, [8 k][32 n][16 p] + 4 floats pad per k row, 16.5 KB (one contiguous
//       16 KB block of the host layout, copied as is);
//     both loaded to registers one chunk ahead (12 x 16 B per thread) and written to LDS behind a barrier.
//   K step (4 channels): each lane reads its tile's 16 patch values of channel 4s + kq (16 ds_read_b32), applies
//   B^T d B (32 adds) and issues 2 x 16 MFMAs whose B operands come as 8 ds_read_b128 (4 positions each).
//
//   Costing (per CU, 2 blocks resident: 128 accumulators + ~100 other registers <= 256 per lane, 2 x 50 KB LDS):
//     MFMA per chunk and wave: 2 steps x 16 positions x 2 halves = 64 x 32 cycles = 2048 cycles;
//     VALU per chunk and wave: 2 x 32 transform adds + the 16 x 4 output-transform adds once per block: ~1 VALU per MFMA
//       on the K loop, hidden behind the matrix pipe;
//     staged per chunk and block: 32 KB of patches (each input pixel is read by up to 4 overlapping patches: L1 / L2
//       hits) + 16 KB of weights = 48 KB per 2 x 2048 SIMD cycles (two resident blocks share the SIMDs) = ~12 B/clk/CU,
//       against the ~30-39 B/clk the L1 -> LDS path moved in profiles/r04_h256_pmc.md;
//     LDS reads per chunk and wave: 32 x b32 + 16 x b128 = 12 KB for 64 MFMAs.
//   Against the direct kernel (conv_mfma.hip, 9 x 128 / 32 = 36 chunks of 64 32x32x2 MFMAs per 128 x 128 tile): the
//   same output takes 16 / 36 of the MFMA cycles.
//
//   Epilogue: Y = A^T M A per (tile, channel), bias + activation, scalar stores (16 lanes = 64 contiguous bytes) with the
//   generic addressing: out_coff / out_cstride / out_bstride.  gn_partials: on the geometries where a block covers
//   exactly two whole 128-pixel flattened tiles (host check wino_gn_ok), slot nt (the block's 32-channel group) of each
//   of them gets that block's (sum, sum of squares) in fp64; the 4 groups of n_pad = 128 fill all 4 slots.
//   All addressing is 64-bit (no buffer resources): no 2 GiB limit.  Several problems (pyramid levels) per launch; no
//   host reads, no allocation: capturable in a hipGraph.  Fixed-capacity RoI batches (`live`): blocks that hold only
//   non-existing images return at once, so a mask-head conv runs on the same kernel (same bits) with or without `live`.
#include "common.h"

namespace {

constexpr int WMAXP = ML_CONV_MAX_PROBLEMS;
constexpr int WT = 64;        // Winograd tiles per block
constexpr int WN = 32;        // output channels per block
constexpr int WK = 8;         // input channels per chunk
constexpr int PT_LD = 132;    // floats per tile in the patch buffer (16 px x 8 ch + 4 pad)
constexpr int WB_LD = 516;    // floats per k row in the weight buffer (32 n x 16 p + 4 pad)
constexpr int WCHUNK = WK * WN * 16;   // floats of transformed weights per (N block, chunk)

struct WProblem {
    ml_conv2d_desc d;
    int TH, TW, T;            // tile rows / columns per image, tiles in all (B * TH * TW)
    int MB, NB, nchunks;      // 64-tile blocks, 32-channel blocks, 8-channel chunks
};

struct WArgs {
    int n;
    int start[WMAXP + 1];     // prefix sum of blocks per problem
    WProblem p[WMAXP];
};

__device__ __forceinline__ void bt_d_b(const float d[16], float v[16]) {
    // V = B^T d B, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]; d, v row-major 4x4
    float t[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t[0 * 4 + j] = d[0 * 4 + j] - d[2 * 4 + j];
        t[1 * 4 + j] = d[1 * 4 + j] + d[2 * 4 + j];
        t[2 * 4 + j] = d[2 * 4 + j] - d[1 * 4 + j];
        t[3 * 4 + j] = d[1 * 4 + j] - d[3 * 4 + j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i * 4 + 0] = t[i * 4 + 0] - t[i * 4 + 2];
        v[i * 4 + 1] = t[i * 4 + 1] + t[i * 4 + 2];
        v[i * 4 + 2] = t[i * 4 + 2] - t[i * 4 + 1];
        v[i * 4 + 3] = t[i * 4 + 1] - t[i * 4 + 3];
    }
}

__global__ void __launch_bounds__(256, 2) conv_wino_kernel(const WArgs args) {
    __shared__ __attribute__((aligned(16))) float lds_p[WT * PT_LD];
    __shared__ __attribute__((aligned(16))) float lds_w[WK * WB_LD];
    __shared__ double lds_gn[4][4];

    int pi = 0;
    while (pi + 1 < args.n && (int)blockIdx.x >= args.start[pi + 1]) ++pi;
    const WProblem &P = args.p[pi];
    const ml_conv2d_desc &p = P.d;
    // blocks that share one 64-tile panel get ids congruent mod 8 (the same XCD / L2)
    const int b = (int)blockIdx.x - args.start[pi];
    const int g = b / (8 * P.NB), rr = b - g * 8 * P.NB;
    const int nt = rr >> 3;
    const int mt = g * 8 + (rr & 7);
    if (mt >= P.MB) return;
    if (p.live) {
        // fixed-capacity RoI batch: image i exists iff i % live_period < max(1, *live); a block of non-existing images only
        // computes and stores nothing (block-uniform)
        const int lv = max(1, *p.live), tpi0 = P.TH * P.TW;
        const int b0 = mt * WT / tpi0, b1 = min(mt * WT + WT, P.T) - 1;
        bool any = false;
        for (int bi = b0; bi <= b1 / tpi0 && !any; ++bi) any = bi % p.live_period < lv;
        if (!any) return;
    }

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int tpi = P.TH * P.TW;

    // this thread's 8 staged patch slots: pixel index (b*H + y)*W + x, or -1 outside the image / past the last tile
    int pix[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = tid + 256 * i;
        const int tile = idx >> 5, px = (idx >> 1) & 15;
        const int gt = mt * WT + tile;
        pix[i] = -1;
        if (gt < P.T) {
            const int bi = gt / tpi, rem = gt - bi * tpi;
            const int ty = rem / P.TW, tx = rem - ty * P.TW;
            const int y = 2 * ty - 1 + (px >> 2), x = 2 * tx - 1 + (px & 3);
            if (y >= 0 && y < p.H && x >= 0 && x < p.W) pix[i] = (bi * p.H + y) * p.W + x;
        }
    }
    const size_t cstride = (size_t)p.in_cstride;
    const float *in = p.in + p.in_coff + ((tid & 1) << 2);
    const float *wsrc = p.wgt + (size_t)nt * P.nchunks * WCHUNK + tid * 4;

    f32x4 rp[8], rw[4];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            rp[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (pix[i] >= 0) rp[i] = *reinterpret_cast<const f32x4 *>(in + (size_t)pix[i] * cstride + c * WK);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) rw[i] = *reinterpret_cast<const f32x4 *>(wsrc + (size_t)c * WCHUNK + i * 1024);
    };

    f32x4 acc[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_chunk(0);
    for (int c = 0; c < P.nchunks; ++c) {
        __syncthreads();                          // the previous chunk's LDS reads are done
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i;
            *reinterpret_cast<f32x4 *>(lds_p + (idx >> 5) * PT_LD + (idx & 31) * 4) = rp[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i;        // float4 index in the 16 KB chunk: k row = idx >> 7
            *reinterpret_cast<f32x4 *>(lds_w + (idx >> 7) * WB_LD + (idx & 127) * 4) = rw[i];
        }
        __syncthreads();
        if (c + 1 < P.nchunks) load_chunk(c + 1);  // in flight under this chunk's MFMAs
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int ch = 4 * s + kq;
            const float *pa = lds_p + (wave * 16 + r) * PT_LD + ch;
            float d[16], v[16];
#pragma unroll
            for (int px = 0; px < 16; ++px) d[px] = pa[px * WK];
            bt_d_b(d, v);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float *pb = lds_w + ch * WB_LD + (16 * t + r) * 16;
#pragma unroll
                for (int pq = 0; pq < 4; ++pq) {
                    const f32x4 bq = *reinterpret_cast<const f32x4 *>(pb + 4 * pq);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        acc[t][4 * pq + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[4 * pq + e], bq[e], acc[t][4 * pq + e], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: Y = A^T M A, A^T = [1 1 1 0; 0 1 -1 -1]; lane holds tiles wave*16 + kq*4 + i, channel 16t + r
    const bool gn = p.gn_partials != nullptr;      // (block-uniform; host: wino_gn_ok)
    double gs[2] = {0.0, 0.0}, gq[2] = {0.0, 0.0};
    long long f0 = 0;
    if (gn) {
        const int gt0 = mt * WT;
        const int bi = gt0 / tpi, rem = gt0 - bi * tpi, ty = rem / P.TW, tx = rem - ty * P.TW;
        f0 = ((long long)(bi * p.Ho + 2 * ty) * p.Wo + 2 * tx) >> 7;
    }
    const float lo = 0.f, hi = (p.act == ML_ACT_RELU6) ? 6.f : 3.402823466e38f;
    const bool clampv = p.act == ML_ACT_RELU || p.act == ML_ACT_RELU6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gt = mt * WT + wave * 16 + kq * 4 + i;
        if (gt >= P.T) continue;
        const int bi = gt / tpi, rem = gt - bi * tpi;
        const int ty = rem / P.TW, tx = rem - ty * P.TW;
        const int oy = 2 * ty, ox = 2 * tx;
        const bool y1 = oy + 1 < p.Ho, x1 = ox + 1 < p.Wo;
        const size_t img = p.out_bstride ? (size_t)bi * (size_t)p.out_bstride : (size_t)bi * p.Ho * p.Wo * p.out_cstride;
        const size_t pix0 = (size_t)oy * p.Wo + ox;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = nt * WN + 16 * t + r;
            if (n >= p.cout) continue;
            float m[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) m[q] = acc[t][q][i];
            float u[8];                            // A^T M: rows 0, 1 x 4 columns
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u[j] = m[0 * 4 + j] + m[1 * 4 + j] + m[2 * 4 + j];
                u[4 + j] = m[1 * 4 + j] - m[2 * 4 + j] - m[3 * 4 + j];
            }
            float yv[4];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                yv[2 * a] = u[4 * a + 0] + u[4 * a + 1] + u[4 * a + 2];
                yv[2 * a + 1] = u[4 * a + 1] - u[4 * a + 2] - u[4 * a + 3];
            }
            const float bv = p.bias ? p.bias[n] : 0.f;
            float *o = p.out + img + p.out_coff + n;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    if ((a && !y1) || (c2 && !x1)) continue;
                    float val = yv[2 * a + c2] + bv;
                    if (clampv) val = __builtin_amdgcn_fmed3f(val, lo, hi);
                    else if (p.act != ML_ACT_NONE) val = ml_apply_act(val, p.act);
                    o[(pix0 + (size_t)a * p.Wo + c2) * p.out_cstride] = val;
                    if (gn) {
                        const long long m_flat = ((long long)(bi * p.Ho + oy + a) * p.Wo + ox + c2);
                        const int f = (m_flat >> 7) != f0;
                        gs[f] += (double)val;
                        gq[f] += (double)val * (double)val;
                    }
                }
        }
    }
    if (gn) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                gs[f] += __shfl_down(gs[f], o, 64);
                gq[f] += __shfl_down(gq[f], o, 64);
            }
        }
        if (lane == 0) {
            lds_gn[wave][0] = gs[0]; lds_gn[wave][1] = gq[0];
            lds_gn[wave][2] = gs[1]; lds_gn[wave][3] = gq[1];
        }
        __syncthreads();
        if (tid < 2) {
            // the block's second flattened tile: the one holding its last tile's bottom-right pixel
            const int gt1 = mt * WT + WT - 1;
            const int bi = gt1 / tpi, rem = gt1 - bi * tpi, ty = rem / P.TW, tx = rem - ty * P.TW;
            const long long f1 = ((long long)(bi * p.Ho + 2 * ty + 1) * p.Wo + 2 * tx + 1) >> 7;
            const long long ft = tid ? f1 : f0;
            double s = 0.0, q = 0.0;
            for (int w = 0; w < 4; ++w) { s += lds_gn[w][2 * tid]; q += lds_gn[w][2 * tid + 1]; }
            p.gn_partials[2 * (ft * 4 + nt)] = s;
            p.gn_partials[2 * (ft * 4 + nt) + 1] = q;
        }
    }
}

}  // namespace

// The one eligibility rule of the Winograd path (tile code 6): per-problem geometry and math mode only -- never the batch
// size or the launch's tile count, so an image's results do not depend on the batch it is computed in.
extern "C" int ml_conv2d_wino_eligible(const ml_conv2d_desc *d) {
    if (!d) return 0;
    return d->math == ML_MATH_F32 && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->dil == 1 && d->pad_t == 1 &&
           d->pad_l == 1 && d->Ho == d->H && d->Wo == d->W && d->cpp_shift == 30 && d->group_cin_step == 0 &&
           !d->shuffle2x2 && !d->residual && !d->out_f16 && d->span % 32 == 0 && d->span_pad == d->span &&
           d->cout <= 128 && d->n_pad == 128;
}

// gn_partials on the Winograd path: every 64-tile block must cover exactly two whole 128-pixel flattened tiles of one image
// (even Ho / Wo; a block is whole tile rows, or a 128-column piece of one), 4 channel groups of 32 = the 4 slots.
int ml_conv2d_wino_gn_ok(const ml_conv2d_desc &d) {
    if (d.Ho % 2 || d.Wo % 2 || d.cout != 128 || d.out_bstride || d.act == ML_ACT_SIGMOID) return 0;
    const long long TH = d.Ho / 2, TW = d.Wo / 2;
    return (64 % TW == 0 || TW % 64 == 0) && (TH * TW) % 64 == 0;
}

int ml_conv2d_wino_launch(const ml_conv2d_desc *descs, int n, hipStream_t s) {
    ML_REQUIRE(n >= 1 && n <= WMAXP, "conv2d (winograd): need 1..%d problems", WMAXP);
    WArgs args;
    args.n = n;
    long long start = 0;
    for (int i = 0; i < n; ++i) {
        const ml_conv2d_desc &d = descs[i];
        ML_REQUIRE(ml_conv2d_wino_eligible(&d),
                   "conv2d: tile = 6 (Winograd F(2x2,3x3)) needs ML_MATH_F32, a 3x3 stride-1 undilated 'same' conv, no "
                   "groups / shuffle / residual / half output, span %% 32 == 0 and n_pad == 128");
        ML_REQUIRE(((d.in_cstride | d.in_coff) & 3) == 0 && ml_aligned16(d.in) && ml_aligned16(d.wgt),
                   "conv2d (winograd): 16-byte aligned input channels and weights");
        if (d.gn_partials)
            ML_REQUIRE(ml_conv2d_wino_gn_ok(d) && !d.live, "conv2d (winograd): gn_partials needs even Ho / Wo, Wo / 2 dividing or a "
                                                "multiple of 64, (Ho / 2) (Wo / 2) %% 64 == 0, cout = 128, dense output");
        WProblem &P = args.p[i];
        P.d = d;
        P.TH = (d.Ho + 1) / 2;
        P.TW = (d.Wo + 1) / 2;
        const long long T = (long long)d.B * P.TH * P.TW;
        ML_REQUIRE(T < (1ll << 30), "conv2d (winograd): too many tiles");
        P.T = (int)T;
        P.MB = (int)((T + WT - 1) / WT);
        P.NB = d.n_pad / WN;
        P.nchunks = d.span_pad / WK;
        args.start[i] = (int)start;
        start += (long long)(P.MB + 7) / 8 * 8 * P.NB;
        ML_REQUIRE(start < (1ll << 31), "conv2d (winograd): grid too large");
    }
    args.start[n] = (int)start;
    // gn_partials keeps the direct kernel's launch-size rule (ml_conv2d_gn_min_launch_tiles, in 128 x 128 tiles), so the
    // host's choice between epilogue sums and a statistics pass does not depend on which kernel runs the conv
    long long tiles128 = 0;
    bool any_gn = false;
    for (int i = 0; i < n; ++i) {
        tiles128 += ((long long)descs[i].B * descs[i].Ho * descs[i].Wo + 127) / 128 * (descs[i].n_pad / 128);
        any_gn = any_gn || descs[i].gn_partials != nullptr;
    }
    ML_REQUIRE(!any_gn || tiles128 >= ml_conv2d_gn_min_launch_tiles(),
               "conv2d (winograd): gn_partials needs a launch of ml_conv2d_gn_min_launch_tiles() tiles of 128 x 128");
    hipLaunchKernelGGL(conv_wino_kernel, dim3((unsigned)start), dim3(256), 0, s, args);
    ML_CHECK_LAUNCH("conv2d (winograd)");
    return ML_OK;
}
