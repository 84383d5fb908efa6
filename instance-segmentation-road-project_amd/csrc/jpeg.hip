// Baseline JPEG encoder on the device: what tf.io.encode_jpeg writes with its defaults (reference
// engine/layers/misc.py:343-351, EncodeImageContent) -- sequential DCT, 8 bit, Y Cb Cr at 2x2 / 1x1 / 1x1 in one
// interleaved scan, the Annex K quantisation tables scaled by the libjpeg quality rule, the four Annex K Huffman tables,
// a JFIF APP0 header, no restart markers.
//
// Sample stage (integers, FIX(x) = int(x * 65536 + 0.5)):
//   Y  = ( FIX(.299) R   + FIX(.587) G   + FIX(.114) B   + 32768) >> 16
//   Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B     + (128 << 16) + 32767) >> 16
//   Cr = ( FIX(.5) R     - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
//   planes padded to a multiple of 16 by replicating the last column and row (the blocks beyond the frame encode those
//   samples; libjpeg writes "dummy" blocks there -- both are valid streams);
//   chroma = 2x2 box (a + b + c + d + bias) >> 2, bias 1 in even output columns, 2 in odd ones;
//   level shift -128, the orthonormal 8x8 DCT of T.81 A.3.3 in fp32 (two 8x8 matrix products),
//   coefficient = trunc(|v| / Q + 0.5) with the sign of v;
//   Q = clamp((base * s + 50) / 100, 1, 255), s = 5000 / q below 50, else 200 - 2 q.
//
// Launches, all on the caller's stream, no host read:
//   1 coefficients   one wave per MCU: colour conversion, subsampling, DCT, quantisation -> int16 [mcu][6][64], zigzag;
//                    the same launch clears the word buffer of launch 4
//   2 bit lengths    one thread per block (DC prediction reads the previous block of the component)
//   3 scan           one workgroup per image: lengths -> bit offsets, total
//   4 pack           one thread per block writes its code words at its offset into zeroed 32-bit words; the first and
//                    the last word of a block are shared with its neighbours (atomicOr), the others are its own
//   5 count          one thread per 64 bytes of the packed scan counts its 0xFF bytes (last byte padded with 1-bits)
//   6 scan           counts -> offsets
//   7 scatter        header, the bytes with 0x00 after every 0xFF, EOI, the image's length
// The per-thread bodies are __host__ __device__ functions of a thread index, so they can be run on a CPU in a loop.
#include "common.h"
#include "ranges.h"
#include <string.h>
#include <initializer_list>

namespace {

constexpr int TPB = 256;
constexpr int SCAN_TPB = 1024;
constexpr int CHUNK = 64;                        // bytes of packed scan per thread of the stuffing passes
constexpr int HEADER_BYTES = 623;                // SOI 2, APP0 18, 2 DQT 138, SOF0 19, 4 DHT 432, SOS 14
// longest DC code 11 bits + 11 magnitude bits; longest AC code 16 bits + 10 magnitude bits (8-bit samples)
constexpr unsigned BLOCK_BITS_MAX = 22 + 63 * 26;

constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t BASE_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61,  12, 12, 14, 19, 26, 58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51, 87, 80, 62,  18, 22, 37, 56, 68, 109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr char AC_LUM_HEX[] =
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa";
constexpr char AC_CHR_HEX[] =
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536"
    "3738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2"
    "a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa";
static_assert(sizeof(AC_LUM_HEX) == 2 * 162 + 1 && sizeof(AC_CHR_HEX) == 2 * 162 + 1, "162 AC symbols per table");
constexpr int hex_digit(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
constexpr uint8_t ac_symbol(int t, int i) {
    const char *s = t ? AC_CHR_HEX : AC_LUM_HEX;
    return (uint8_t)(hex_digit(s[2 * i]) * 16 + hex_digit(s[2 * i + 1]));
}
// dct[u * 8 + x] = C(u) / 2 * cos((2x + 1) u pi / 16), C(0) = 1 / sqrt 2
constexpr float DCT[64] = {
    0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f,
    0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f,
    0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f,
    0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f,
    0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,
    0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f,
    0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f,
    0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f};

// what the kernels look up: the DCT matrix, natural index -> zigzag position, Huffman (code << 8 | length) by symbol
struct Tables {
    float dct[64];
    uint8_t zz_of_nat[64];
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};

constexpr Tables make_tables() {
    Tables t{};
    for (int i = 0; i < 64; ++i) {
        t.dct[i] = DCT[i];
        t.zz_of_nat[ZIGZAG[i]] = (uint8_t)i;
    }
    for (int k = 0; k < 2; ++k) {                                  // T.81 Annex C: codes in order of length
        uint32_t code = 0;
        int n = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int j = 0; j < DC_BITS[k][len - 1]; ++j) t.dc[k][n++] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
        code = 0;
        n = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int j = 0; j < AC_BITS[k][len - 1]; ++j) t.ac[k][ac_symbol(k, n++)] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
    }
    return t;
}

__constant__ Tables d_tables = make_tables();

struct QuantTables {
    uint8_t q[2][64];                                              // natural order
};
struct Header {
    uint8_t bytes[HEADER_BYTES + 1];
};

constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }

template <class T>
__host__ __device__ inline T min_of(T a, T b) { return a < b ? a : b; }

// ----------------------------------------------------------------------------- coefficients: one wave per MCU
struct McuLds {
    float samp[6][64];                                             // level-shifted samples: Y00 Y01 Y10 Y11 Cb Cr
    int cbcr[2][256];                                              // full-resolution chroma of the MCU
    float tmp[6][64];                                              // after the row pass
};

// lane: row lane / 4 of the MCU, four pixels from column (lane % 4) * 4
__host__ __device__ inline void mcu_load(int lane, const uint8_t *img, int H, int W, int my, int mx, McuLds &s) {
    const int r = lane >> 2, c0 = (lane & 3) * 4;
    const int y = min_of(my * 16 + r, H - 1);
    const uint8_t *row = img + (size_t)y * W * 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = c0 + q;
        const int x = min_of(mx * 16 + c, W - 1);
        const int R = row[x * 3], G = row[x * 3 + 1], B = row[x * 3 + 2];
        const int Y = (fix16(.299) * R + fix16(.587) * G + fix16(.114) * B + 32768) >> 16;
        const int Cb = (-fix16(.16874) * R - fix16(.33126) * G + fix16(.5) * B + (128 << 16) + 32767) >> 16;
        const int Cr = (fix16(.5) * R - fix16(.41869) * G - fix16(.08131) * B + (128 << 16) + 32767) >> 16;
        s.samp[(r >> 3) * 2 + (c >> 3)][(r & 7) * 8 + (c & 7)] = (float)(Y - 128);
        s.cbcr[0][r * 16 + c] = Cb;
        s.cbcr[1][r * 16 + c] = Cr;
    }
}

// lane: chroma sample (lane / 8, lane % 8)
__host__ __device__ inline void mcu_chroma(int lane, McuLds &s) {
    const int i = lane >> 3, j = lane & 7;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int *p = &s.cbcr[c][(2 * i) * 16 + 2 * j];
        s.samp[4 + c][lane] = (float)(((p[0] + p[1] + p[16] + p[17] + 1 + (j & 1)) >> 2) - 128);
    }
}

// lane: row lane / 8, frequency u = lane % 8
__host__ __device__ inline void mcu_rows(int lane, const Tables &t, McuLds &s) {
    const int r = lane >> 3, u = lane & 7;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        float acc = 0.f;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += s.samp[b][r * 8 + x] * t.dct[u * 8 + x];
        s.tmp[b][r * 8 + u] = acc;
    }
}

// lane: coefficient (v, u) = (lane / 8, lane % 8)
__host__ __device__ inline void mcu_columns(int lane, const Tables &t, const QuantTables &qt, const McuLds &s, int16_t *coef) {
    const int v = lane >> 3, u = lane & 7;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        float acc = 0.f;
#pragma unroll
        for (int y = 0; y < 8; ++y) acc += s.tmp[b][y * 8 + u] * t.dct[v * 8 + y];
        const float a = (acc < 0.f ? -acc : acc) / (float)qt.q[b >> 2][lane];
        int n = (int)a;                                            // a - n is exact: no rounding decides a near-tie
        n += a - (float)n >= 0.5f;
        coef[b * 64 + t.zz_of_nat[lane]] = (int16_t)(acc < 0.f ? -n : n);
    }
}

// Also clears the image's word buffer for the pack kernel (nwords is a multiple of 4 and the buffer 16-byte aligned).
__global__ __launch_bounds__(TPB) void jpeg_coefficients_kernel(const uint8_t *images, int16_t *coef, uint32_t *words, QuantTables qt,
                                                               int H, int W, int mw, unsigned nmcu, unsigned nwords) {
    __shared__ McuLds lds[TPB / 64];
    uint4 *clear = reinterpret_cast<uint4 *>(words + (size_t)blockIdx.y * nwords);
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < nwords / 4; i += gridDim.x * TPB) clear[i] = make_uint4(0u, 0u, 0u, 0u);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned mcu = blockIdx.x * (TPB / 64) + wave;
    const bool live = mcu < nmcu;                                  // whole waves: the barriers below are reached by all
    const uint8_t *img = images + (size_t)blockIdx.y * H * W * 3;
    McuLds &s = lds[wave];
    if (live) mcu_load(lane, img, H, W, (int)(mcu / mw), (int)(mcu % mw), s);
    __syncthreads();
    if (live) mcu_chroma(lane, s);
    __syncthreads();
    if (live) mcu_rows(lane, d_tables, s);
    __syncthreads();
    if (live) mcu_columns(lane, d_tables, qt, s, coef + ((size_t)blockIdx.y * nmcu + mcu) * 384);
}

// ----------------------------------------------------------------------------- entropy coding: one thread per block
__host__ __device__ inline int bit_size(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}
__host__ __device__ inline uint32_t magnitude_bits(int v, int size) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u); }

// DC of the previous block of the same component in scan order (0 at the start of the image); g = mcu * 6 + block
__host__ __device__ inline int previous_dc(const int16_t *coef, unsigned g) {
    const unsigned b = g % 6;
    if (b >= 1 && b <= 3) return coef[(size_t)(g - 1) * 64];
    if (g < 6) return 0;
    return coef[(size_t)(b == 0 ? g - 3 : g - 6) * 64];
}

// the code words of one block in order; sizes are clamped to what the tables hold, so BLOCK_BITS_MAX bounds any input
template <class Emit>
__host__ __device__ inline void walk_block(const int16_t *coef, unsigned g, const Tables &t, Emit &emit) {
    alignas(16) int16_t c[64];
    __builtin_memcpy(c, __builtin_assume_aligned(coef + (size_t)g * 64, 16), 128);
    const int k = g % 6 >= 4;
    const int d = c[0] - previous_dc(coef, g);
    int size = min_of(bit_size(d), 11);
    emit(t.dc[k][size] >> 8, (int)(t.dc[k][size] & 255u));
    emit(magnitude_bits(d, size), size);
    int run = 0;
#pragma unroll
    for (int i = 1; i < 64; ++i) {
        const int v = c[i];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) emit(t.ac[k][0xF0] >> 8, (int)(t.ac[k][0xF0] & 255u));
        size = min_of(bit_size(v), 10);
        const uint32_t e = t.ac[k][run << 4 | size];
        emit(e >> 8, (int)(e & 255u));
        emit(magnitude_bits(v, size), size);
        run = 0;
    }
    if (run) emit(t.ac[k][0] >> 8, (int)(t.ac[k][0] & 255u));
}

struct CountBits {
    uint32_t n = 0;
    __host__ __device__ void operator()(uint32_t, int len) { n += (uint32_t)len; }
};

__host__ __device__ inline void or_word(uint32_t *p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

// bits go into big-endian 32-bit words: stream byte k is bits 31 - 8 (k % 4) .. of word k / 4
struct PackBits {
    uint32_t *words;
    uint32_t wi;
    uint64_t acc = 0;
    int n;                                                         // bits in acc, the word's bits before this block included
    bool first = true;
    __host__ __device__ PackBits(uint32_t *w, uint32_t bit_offset) : words(w), wi(bit_offset >> 5), n((int)(bit_offset & 31u)) {}
    __host__ __device__ void operator()(uint32_t code, int len) {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            const uint32_t w = (uint32_t)(acc >> (n - 32));
            if (first) or_word(words + wi, w); else words[wi] = w;  // a later word is wholly this block's
            first = false;
            ++wi;
            n -= 32;
            acc &= (1ull << n) - 1ull;
        }
    }
    __host__ __device__ void finish() {
        if (n > 0) or_word(words + wi, (uint32_t)(acc << (32 - n)));
    }
};

__host__ __device__ inline void bit_length_body(unsigned g, const int16_t *coef, uint32_t *lens, const Tables &t) {
    CountBits count;
    walk_block(coef, g, t, count);
    lens[g] = count.n;
}

__host__ __device__ inline void pack_body(unsigned g, const int16_t *coef, const uint32_t *offsets, uint32_t *words, const Tables &t) {
    PackBits pack(words, offsets[g]);
    walk_block(coef, g, t, pack);
    pack.finish();
}

__global__ __launch_bounds__(TPB) void jpeg_bit_lengths_kernel(const int16_t *coef, uint32_t *lens, unsigned nblk, unsigned lens_stride) {
    const unsigned g = blockIdx.x * TPB + threadIdx.x;
    if (g < nblk) bit_length_body(g, coef + (size_t)blockIdx.y * nblk * 64, lens + (size_t)blockIdx.y * lens_stride, d_tables);
}

__global__ __launch_bounds__(TPB) void jpeg_pack_kernel(const int16_t *coef, const uint32_t *offsets, uint32_t *words, unsigned nblk,
                                                       unsigned lens_stride, unsigned words_stride) {
    const unsigned g = blockIdx.x * TPB + threadIdx.x;
    if (g < nblk)
        pack_body(g, coef + (size_t)blockIdx.y * nblk * 64, offsets + (size_t)blockIdx.y * lens_stride,
                  words + (size_t)blockIdx.y * words_stride, d_tables);
}

// ----------------------------------------------------------------------------- exclusive scan, one workgroup per image
__host__ __device__ inline uint32_t chunks_of_bits(uint32_t nbits) { return ((nbits + 7u) / 8u + CHUNK - 1u) / CHUNK; }

// a[image][0..n) -> exclusive prefix sums in place, totals[image * 2 + slot] = the sum.  n = n_fixed, or the number of
// chunks of the image's packed scan when `bits_totals` is given.
__global__ __launch_bounds__(SCAN_TPB) void jpeg_scan_kernel(uint32_t *a, unsigned stride, unsigned n_fixed, const uint32_t *bits_totals,
                                                            uint32_t *totals, int slot) {
    __shared__ uint32_t part[SCAN_TPB];
    const unsigned tid = threadIdx.x;
    a += (size_t)blockIdx.x * stride;
    const unsigned n = bits_totals ? min_of(chunks_of_bits(bits_totals[blockIdx.x * 2]), stride) : n_fixed;
    const unsigned per = (n + SCAN_TPB - 1) / SCAN_TPB;
    const unsigned lo = min_of(tid * per, n), hi = min_of(lo + per, n);
    uint32_t sum = 0;
    for (unsigned i = lo; i < hi; ++i) sum += a[i];
    part[tid] = sum;
    __syncthreads();
    for (unsigned d = 1; d < SCAN_TPB; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
    for (unsigned i = lo; i < hi; ++i) {
        const uint32_t v = a[i];
        a[i] = run;
        run += v;
    }
    if (tid == SCAN_TPB - 1) totals[blockIdx.x * 2 + slot] = part[tid];
}

// ----------------------------------------------------------------------------- byte stuffing: one thread per CHUNK bytes
// byte k of the packed scan; the last byte's unused low bits are 1
__host__ __device__ inline uint32_t scan_byte(const uint32_t *words, uint32_t k, uint32_t nbytes, uint32_t nbits) {
    uint32_t v = (words[k >> 2] >> (24u - 8u * (k & 3u))) & 255u;
    if (k == nbytes - 1u && (nbits & 7u)) v |= (1u << (8u - (nbits & 7u))) - 1u;
    return v;
}

__host__ __device__ inline void count_body(unsigned t, const uint32_t *words, uint32_t nbits, uint32_t *counts) {
    const uint32_t nbytes = (nbits + 7u) / 8u, start = t * CHUNK;
    if (start >= nbytes) return;
    const uint32_t end = min_of(start + CHUNK, nbytes);
    uint32_t n = 0;
    for (uint32_t k = start; k < end; ++k) n += scan_byte(words, k, nbytes, nbits) == 255u;
    counts[t] = n;
}

// `out` has room for HEADER_BYTES + 2 * nbytes + 2 (the capacity bounds nbytes by BLOCK_BITS_MAX per block)
__host__ __device__ inline void scatter_body(unsigned t, const uint32_t *words, uint32_t nbits, const uint32_t *ff_before,
                                             uint32_t ff_total, uint8_t *out, int32_t *length) {
    const uint32_t nbytes = (nbits + 7u) / 8u, start = t * CHUNK;
    if (start >= nbytes) return;
    const uint32_t end = min_of(start + CHUNK, nbytes);
    uint8_t *dst = out + HEADER_BYTES + start + ff_before[t];
    for (uint32_t k = start; k < end; ++k) {
        const uint32_t v = scan_byte(words, k, nbytes, nbits);
        *dst++ = (uint8_t)v;
        if (v == 255u) *dst++ = 0;
    }
    if (end == nbytes) {
        dst[0] = 0xFF;
        dst[1] = 0xD9;
        *length = (int32_t)(HEADER_BYTES + nbytes + ff_total + 2u);
    }
}

__global__ __launch_bounds__(TPB) void jpeg_count_kernel(const uint32_t *words, const uint32_t *totals, uint32_t *counts,
                                                        unsigned nchunks, unsigned words_stride) {
    const unsigned t = blockIdx.x * TPB + threadIdx.x;
    if (t < nchunks)
        count_body(t, words + (size_t)blockIdx.y * words_stride, totals[blockIdx.y * 2], counts + (size_t)blockIdx.y * nchunks);
}

__global__ __launch_bounds__(TPB) void jpeg_scatter_kernel(const uint32_t *words, const uint32_t *totals, const uint32_t *ff_before,
                                                          uint8_t *out, int32_t *lengths, Header header, unsigned nchunks,
                                                          unsigned words_stride, long long capacity) {
    const unsigned t = blockIdx.x * TPB + threadIdx.x;
    uint8_t *o = out + (size_t)blockIdx.y * capacity;
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < HEADER_BYTES; i += TPB) o[i] = header.bytes[i];
    if (t < nchunks)
        scatter_body(t, words + (size_t)blockIdx.y * words_stride, totals[blockIdx.y * 2], ff_before + (size_t)blockIdx.y * nchunks,
                     totals[blockIdx.y * 2 + 1], o, lengths + blockIdx.y);
}

// ----------------------------------------------------------------------------- host side
struct Geometry {
    int mw, mh;
    unsigned nmcu, nblk, nwords, nchunks;                          // per image; nwords and nchunks are multiples of 4
    long long capacity;
};

int geometry(int32_t H, int32_t W, Geometry &g, const char *what) {
    ML_REQUIRE(H > 0 && W > 0, "%s: bad dims (H %d, W %d)", what, H, W);
    ML_REQUIRE(H <= 65535 && W <= 65535, "%s: a JPEG dimension cannot be above 65535 (H %d, W %d)", what, H, W);
    g.mw = (W + 15) / 16;
    g.mh = (H + 15) / 16;
    const long long nblk = 6ll * g.mw * g.mh;
    ML_REQUIRE(nblk * BLOCK_BITS_MAX < (1ll << 31), "%s: frame too large (%d x %d: bit offsets are 32-bit)", what, H, W);
    g.nmcu = (unsigned)(g.mw * g.mh);
    g.nblk = (unsigned)nblk;
    const long long scan_bytes = (nblk * BLOCK_BITS_MAX + 7) / 8;
    g.nwords = (unsigned)(((scan_bytes + 3) / 4 + 1 + 3) / 4 * 4);
    g.nchunks = (unsigned)(((scan_bytes + CHUNK - 1) / CHUNK + 3) / 4 * 4);
    g.capacity = (HEADER_BYTES + 2 * scan_bytes + 2 + 15) / 16 * 16;
    return ML_OK;
}

long long round16(long long n) { return (n + 15) / 16 * 16; }

void quality_tables(int quality, QuantTables &qt) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 64; ++i) {
            const int q = (BASE_Q[k][i] * s + 50) / 100;
            qt.q[k][i] = (uint8_t)(q < 1 ? 1 : q > 255 ? 255 : q);
        }
}

// SOI, APP0 (JFIF 1.01, 300 x 300 dpi: tf.io.encode_jpeg's defaults), DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, SOS
void make_header(int H, int W, const QuantTables &qt, Header &h) {
    uint8_t *p = h.bytes;
    auto put = [&](std::initializer_list<int> v) { for (int b : v) *p++ = (uint8_t)b; };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 1, 0x01, 0x2C, 0x01, 0x2C, 0, 0});
    for (int k = 0; k < 2; ++k) {
        put({0xFF, 0xDB, 0, 67, k});
        for (int i = 0; i < 64; ++i) *p++ = qt.q[k][ZIGZAG[i]];
    }
    put({0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int k = 0; k < 2; ++k) {
        put({0xFF, 0xC4, 0, 31, k});
        for (int i = 0; i < 16; ++i) *p++ = DC_BITS[k][i];
        for (int i = 0; i < 12; ++i) *p++ = (uint8_t)i;
        put({0xFF, 0xC4, 0, 181, 0x10 | k});
        for (int i = 0; i < 16; ++i) *p++ = AC_BITS[k][i];
        for (int i = 0; i < 162; ++i) *p++ = ac_symbol(k, i);
    }
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

}  // namespace

extern "C" int64_t ml_jpeg_encode_capacity(int32_t H, int32_t W) {
    Geometry g;
    const int e = geometry(H, W, g, "jpeg_encode_capacity");
    return e != ML_OK ? e : g.capacity;
}

// per image: coefficients int16 [nblk][64], bit lengths / offsets u32 [nblk], packed words, 0xFF counts; then 2 totals
extern "C" int64_t ml_jpeg_encode_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    Geometry g;
    const int e = geometry(H, W, g, "jpeg_encode_workspace_bytes");
    if (e != ML_OK) return e;
    ML_REQUIRE(B > 0 && B < 65536, "jpeg_encode_workspace_bytes: bad dims (B %d)", B);
    return (long long)B * (g.nblk * 128ll + round16(g.nblk * 4ll) + g.nwords * 4ll + g.nchunks * 4ll) + round16(B * 8ll);
}

extern "C" int ml_jpeg_encode_u8(const uint8_t *images, int32_t B, int32_t H, int32_t W, int32_t quality, uint8_t *out,
                                 int64_t capacity, int32_t *lengths, void *workspace, void *stream) {
    ML_REQUIRE(images && out && lengths && workspace, "jpeg_encode: null pointer");
    ML_REQUIRE(B > 0 && B < 65536, "jpeg_encode: bad dims (B %d)", B);
    Geometry g;
    const int e = geometry(H, W, g, "jpeg_encode");
    if (e != ML_OK) return e;
    ML_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode: quality %d, 1 <= quality <= 100", quality);
    ML_REQUIRE(capacity >= g.capacity, "jpeg_encode: capacity %lld below ml_jpeg_encode_capacity(%d, %d) = %lld",
               (long long)capacity, H, W, g.capacity);
    ML_REQUIRE(ml_aligned16(workspace), "jpeg_encode: workspace must be 16-byte aligned");
    const long long in_bytes = (long long)B * H * W * 3, out_bytes = (long long)B * capacity;
    const long long ws_bytes = ml_jpeg_encode_workspace_bytes(B, H, W);
    ML_REQUIRE(!ml_ranges_overlap(out, out_bytes, images, in_bytes), "jpeg_encode: out overlaps images");
    ML_REQUIRE(!ml_any_overlap({{workspace, ws_bytes}, {lengths, 4ll * B}}, {{images, in_bytes}, {out, out_bytes}}) &&
               !ml_ranges_overlap(workspace, ws_bytes, lengths, 4ll * B),
               "jpeg_encode: workspace or lengths overlaps another buffer");

    const unsigned lens_stride = (unsigned)(round16(g.nblk * 4ll) / 4);
    uint8_t *ws = (uint8_t *)workspace;
    int16_t *coef = (int16_t *)ws;
    ws += (size_t)B * g.nblk * 128;
    uint32_t *lens = (uint32_t *)ws;
    ws += (size_t)B * lens_stride * 4;
    uint32_t *words = (uint32_t *)ws;
    ws += (size_t)B * g.nwords * 4;
    uint32_t *counts = (uint32_t *)ws;
    ws += (size_t)B * g.nchunks * 4;
    uint32_t *totals = (uint32_t *)ws;

    QuantTables qt;
    quality_tables(quality, qt);
    Header header;
    make_header(H, W, qt, header);

    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_coefficients_kernel, dim3((g.nmcu + TPB / 64 - 1) / (TPB / 64), B), dim3(TPB), 0, s, images, coef, words, qt,
                       H, W, g.mw, g.nmcu, g.nwords);
    const dim3 per_block((g.nblk + TPB - 1) / TPB, B), per_chunk((g.nchunks + TPB - 1) / TPB, B);
    hipLaunchKernelGGL(jpeg_bit_lengths_kernel, per_block, dim3(TPB), 0, s, (const int16_t *)coef, lens, g.nblk, lens_stride);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(B), dim3(SCAN_TPB), 0, s, lens, lens_stride, g.nblk, (const uint32_t *)nullptr, totals, 0);
    hipLaunchKernelGGL(jpeg_pack_kernel, per_block, dim3(TPB), 0, s, (const int16_t *)coef, (const uint32_t *)lens, words, g.nblk,
                       lens_stride, g.nwords);
    hipLaunchKernelGGL(jpeg_count_kernel, per_chunk, dim3(TPB), 0, s, (const uint32_t *)words, (const uint32_t *)totals, counts,
                       g.nchunks, g.nwords);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(B), dim3(SCAN_TPB), 0, s, counts, g.nchunks, 0u, (const uint32_t *)totals, totals, 1);
    hipLaunchKernelGGL(jpeg_scatter_kernel, per_chunk, dim3(TPB), 0, s, (const uint32_t *)words, (const uint32_t *)totals,
                       (const uint32_t *)counts, out, lengths, header, g.nchunks, g.nwords, (long long)capacity);
    ML_CHECK_LAUNCH("jpeg_encode");
    return ML_OK;
}
