// The projection unit of a ResNet-50 stage as ONE GEMM over the concatenated K of two source tensors:
//
//   out[b, i, j, n] = relu( sum_k a[b, i, j, k] Wa[k, n] + sum_l x[b, s i, s j, l] Wx[l, n] + bias[n] )
//
// a [B, Ho, Wo, Ka] is the block's 3x3 output, x [B, H, W, Kx] the block's input read IN PLACE at its stride s (1 or 2,
// Ho = (H - 1) / s + 1): no subsample copy, no concatenation buffer, and the shortcut tensor bn(conv_1(x)) never exists in
// memory.  The weights are one operand [N][Ka + Kx] (row n = Wa[:, n] followed by Wx[:, n], both BatchNorms folded),
// bias the sum of the two folded biases.
//
// Tile: 128 pixels x 128 channels per 256-thread block, K in chunks of 128 bytes per row (32 floats / 64 halves): the
// first Ka / chunk chunks come from `a`, the others from `x`, each row with a base of its own -- a "tap" that carries its
// source, span and stride.  Four waves, each 64 channels x 64 pixels as 2 x 2 MFMA tiles; the WEIGHTS are the A operand,
// so a lane ends with 4 consecutive channels of one pixel per accumulator quad and stores them as one vector.
//   float    : v_mfma_f32_32x32x2_f32 -- exact fp32 products, each output one fp32 fma chain in k order
//   _Float16 : v_mfma_f32_32x32x16_f16, fp32 accumulation, bias and ReLU in fp32, one rounding at the store
// Staging: the next chunk's 8 x 16-byte buffer loads per thread are issued before the MFMAs of the current one and written
// to LDS behind the barrier that ends it; 2-3 blocks per CU cover each other's barriers.  LDS rows are 144 bytes (128 + 16):
// the 16-byte fragment reads (row = lane & 31, 16 (lane >> 5) bytes into each 32-byte k-step) and the 16-byte staging
// writes are both conflict-free at that pitch.  Rows past M read pixel M - 1 and are not stored.  No atomics, no split K:
// the same bits run to run, under graph replay and for image k of any batch.
#include "gfx_mem.h"

namespace {

constexpr int DU_TM = 128, DU_TN = 128, DU_TPB = 256;
constexpr int DU_CHUNK = 128;                  // bytes of K per row and chunk
constexpr int DU_ROWB = DU_CHUNK + 16;         // LDS row pitch
constexpr int DU_TILEB = DU_TM * DU_ROWB;

struct DualArgs {
    const void *a, *x, *wgt;
    const float *bias;
    void *out;
    int M, HoWo, Wo, H, W, stride;
    int a_rowb, x_rowb, w_rowb;                // bytes per pixel of a / of x, per channel row of wgt
    int na, nchunks;                           // chunks from a, chunks in all
    int N, tiles_n;
    int a_bytes, x_bytes, w_bytes, out_bytes;
};

// blocks b and b + 8 share an XCD's L2 (for speed only): give each such group a contiguous run of tiles, so that the
// tiles_n blocks that read one pixel panel are neighbours in one L2
__device__ __forceinline__ int xcd_contiguous(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

template <class T>
__global__ void __launch_bounds__(DU_TPB, 2) conv1x1_dual_kernel(const DualArgs A) {
    constexpr bool F32 = sizeof(T) == 4;
    __shared__ __attribute__((aligned(16))) char lds[2 * DU_TILEB];
    char *const s_w = lds, *const s_p = lds + DU_TILEB;       // weight rows, pixel rows

    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x);
    const int n0 = (tile % A.tiles_n) * DU_TN, m0 = (tile / A.tiles_n) * DU_TM;

    const __amdgpu_buffer_rsrc_t ra = rsrc_bytes(A.a, A.a_bytes);
    const __amdgpu_buffer_rsrc_t rx = rsrc_bytes(A.x, A.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = rsrc_bytes(A.wgt, A.w_bytes);
    const __amdgpu_buffer_rsrc_t ro = rsrc_bytes(A.out, A.out_bytes);

    // staging: thread t moves 16-byte piece t & 7 of rows (t >> 3) + 32 i, i = 0..3, of both tiles
    const int piece = (t & 7) * 16, row0 = t >> 3;
    int a_voff[4], x_voff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = min(m0 + row0 + 32 * i, A.M - 1);
        const int b = m / A.HoWo, rem = m - b * A.HoWo, oi = rem / A.Wo, oj = rem - oi * A.Wo;
        a_voff[i] = m * A.a_rowb + piece;
        x_voff[i] = ((b * A.H + oi * A.stride) * A.W + oj * A.stride) * A.x_rowb + piece;
    }
    const int w_voff = (n0 + row0) * A.w_rowb + piece;
    const int st_off = row0 * DU_ROWB + piece;

    u32x4 sp[4], sw[4];
    auto fetch = [&](int c) {
        const bool from_a = c < A.na;                          // block-uniform: a select, never a branch round a load
        const __amdgpu_buffer_rsrc_t rs = from_a ? ra : rx;
        const int soff = (from_a ? c : c - A.na) * DU_CHUNK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sp[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, from_a ? a_voff[i] : x_voff[i], soff, 0);
            sw[i] = __builtin_amdgcn_raw_buffer_load_b128(rw, w_voff, i * 32 * A.w_rowb + c * DU_CHUNK, 0);
        }
    };

    // fragments: the wave's 64 channels (wave >> 1) x 64 pixels (wave & 1); lane -> row lane & 31, k half lane >> 5
    const int frag = (lane & 31) * DU_ROWB + (lane >> 5) * 16;
    const char *const f_w = s_w + (wave >> 1) * 64 * DU_ROWB + frag;
    const char *const f_p = s_p + (wave & 1) * 64 * DU_ROWB + frag;

    f32x16 acc[2][2];                                          // [channel tile][pixel tile]
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ni][mi][e] = 0.f;

    fetch(0);
    for (int c = 0; c < A.nchunks; ++c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<u32x4 *>(s_p + st_off + i * 32 * DU_ROWB) = sp[i];
            *reinterpret_cast<u32x4 *>(s_w + st_off + i * 32 * DU_ROWB) = sw[i];
        }
        __syncthreads();
        if (c + 1 < A.nchunks) fetch(c + 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {                          // 32 bytes of K per row
            f32x4 fw[2], fp[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                fw[q] = *reinterpret_cast<const f32x4 *>(f_w + q * 32 * DU_ROWB + j * 32);
                fp[q] = *reinterpret_cast<const f32x4 *>(f_p + q * 32 * DU_ROWB + j * 32);
            }
            if constexpr (F32) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                        for (int mi = 0; mi < 2; ++mi)
                            acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(fw[ni][e], fp[mi][e], acc[ni][mi], 0, 0, 0);
            } else {
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
                        acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fw[ni]),
                                                                            __builtin_bit_cast(f16x8, fp[mi]), acc[ni][mi], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // C/D layout: column (pixel) = lane & 31, row (channel) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    const int nb = n0 + (wave >> 1) * 64 + (lane >> 5) * 4;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = nb + ni * 32 + g * 8;
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(A.bias + n);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int m = m0 + (wave & 1) * 64 + mi * 32 + (lane & 31);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[ni][mi][4 * g + e] + bv[e], 0.f);
                if (m < A.M) {
                    const int off = (m * A.N + n) * (int)sizeof(T);
                    if constexpr (F32) {
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ro, off, 0, 0);
                    } else {
                        const f16x4 h = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h), ro, off, 0, 0);
                    }
                }
            }
        }
}

template <class T>
int conv1x1_dual_launch(const char *what, const void *a, const void *x, const void *wgt, const float *bias, void *out,
                        int32_t B, int32_t H, int32_t W, int32_t Ka, int32_t Kx, int32_t N, int32_t stride, void *stream) {
    constexpr int ES = (int)sizeof(T), KC = DU_CHUNK / ES;
    constexpr int64_t LIM = (int64_t)1 << 31;              // every tensor is addressed by 32-bit byte offsets
    ML_REQUIRE(a && x && wgt && bias && out, "%s: a, x, wgt, bias and out are required", what);
    ML_REQUIRE(B > 0 && H > 0 && W > 0, "%s: B, H and W must be positive", what);
    ML_REQUIRE(stride == 1 || stride == 2, "%s: stride = %d, must be 1 or 2", what, stride);
    ML_REQUIRE(Ka > 0 && Kx > 0 && Ka % KC == 0 && Kx % KC == 0,
               "%s: Ka = %d and Kx = %d must be positive multiples of the K chunk (%d)", what, Ka, Kx, KC);
    ML_REQUIRE(N > 0 && N % DU_TN == 0, "%s: N = %d must be a positive multiple of %d", what, N, DU_TN);
    ML_REQUIRE(ml_aligned16(a) && ml_aligned16(x) && ml_aligned16(wgt) && ml_aligned16(bias) && ml_aligned16(out),
               "%s: a, x, wgt, bias and out must be 16-byte aligned", what);
    const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1, M = (int64_t)B * Ho * Wo;
    const int64_t a_bytes = M * Ka * ES, x_bytes = (int64_t)B * H * W * Kx * ES, out_bytes = M * N * ES,
                  w_bytes = (int64_t)N * ((int64_t)Ka + Kx) * ES;
    // rows past M are clamped for the loads but still form a store offset (M + 127 rows at the most)
    ML_REQUIRE(a_bytes < LIM && x_bytes < LIM && w_bytes < LIM && (M + DU_TM) * N * ES < LIM,
               "%s: a tensor of 2 GiB or more (32-bit byte offsets)", what);
    const int64_t tiles_n = N / DU_TN, tiles = (M + DU_TM - 1) / DU_TM * tiles_n;
    ML_REQUIRE(tiles < LIM, "%s: too many blocks", what);
    DualArgs A;
    A.a = a;
    A.x = x;
    A.wgt = wgt;
    A.bias = bias;
    A.out = out;
    A.M = (int)M;
    A.HoWo = (int)(Ho * Wo);
    A.Wo = (int)Wo;
    A.H = H;
    A.W = W;
    A.stride = stride;
    A.a_rowb = Ka * ES;
    A.x_rowb = Kx * ES;
    A.w_rowb = (Ka + Kx) * ES;
    A.na = Ka / KC;
    A.nchunks = (Ka + Kx) / KC;
    A.N = N;
    A.tiles_n = (int)tiles_n;
    A.a_bytes = (int)a_bytes;
    A.x_bytes = (int)x_bytes;
    A.w_bytes = (int)w_bytes;
    A.out_bytes = (int)out_bytes;
    hipLaunchKernelGGL(conv1x1_dual_kernel<T>, dim3((unsigned)tiles), dim3(DU_TPB), 0, (hipStream_t)stream, A);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

}  // namespace

extern "C" int ml_conv1x1_dual_f32(const float *a, const float *x, const float *wgt, const float *bias, float *out,
                                   int32_t B, int32_t H, int32_t W, int32_t Ka, int32_t Kx, int32_t N, int32_t stride,
                                   void *stream) {
    return conv1x1_dual_launch<float>("conv1x1_dual_f32", a, x, wgt, bias, out, B, H, W, Ka, Kx, N, stride, stream);
}

extern "C" int ml_conv1x1_dual_f16(const void *a, const void *x, const void *wgt, const float *bias, void *out,
                                   int32_t B, int32_t H, int32_t W, int32_t Ka, int32_t Kx, int32_t N, int32_t stride,
                                   void *stream) {
    return conv1x1_dual_launch<_Float16>("conv1x1_dual_f16", a, x, wgt, bias, out, B, H, W, Ka, Kx, N, stride, stream);
}
