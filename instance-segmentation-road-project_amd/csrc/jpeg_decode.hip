// Baseline JPEG decoder, split between the host and the device: what libjpeg-turbo produces with its defaults
// (JDCT_ISLOW, fancy upsampling), byte for byte.
//
// Host (no GPU needed): the stream is parsed and Huffman-decoded into a packed, sparse form --
//   PackedHeader (224 bytes: magic, H, W, mode, blocks, entries, bytes, the dequantisation tables of the three
//   components in natural order), block_start uint32 [blocks + 1], one 32-bit word per non-zero coefficient
//   (natural-order index << 16 | the int16 value as 16 bits).  Blocks are in scan order, the DC term is un-predicted and
//   always the block's first word, indices are below 64 and distinct within a block, offsets are monotone.
//
// Device, two launches on the caller's stream, no host read:
//   1 blocks   eight lanes per 8x8 block: gather and dequantise into LDS, the integer IDCT of Loeffler, Ligtenberg and
//              Moschytz (CONST_BITS 13, PASS1_BITS 2) down the columns (descale 11) and along the rows (descale 18),
//              clamp(v + 128) -> planar uint8 Y, Cb, Cr at their own resolution.  A block with one word is the constant
//              clamp(((dc * Q0 + 4) >> 3) + 128), which is what the two passes give.
//   2 pixels   one thread per four output bytes (aligned 32-bit stores over the flat [B,H,W,3] tensor): Y and, for
//              2x2 chroma, the triangle filter over the real chroma plane replicated by one sample on every side --
//              colsum = 3 c[r] + c[r -/+ 1] for output row 2r / 2r + 1, out[2x] = (3 colsum[x] + colsum[x - 1] + 8) >> 4,
//              out[2x + 1] = (3 colsum[x] + colsum[x + 1] + 7) >> 4 -- then with FIX(a) = int(a * 65536 + 0.5):
//              R = clamp(Y + ((FIX(1.402) cr + 32768) >> 16)), G = clamp(Y + ((-FIX(.34414) cb + 32768 - FIX(.71414) cr)
//              >> 16)), B = clamp(Y + ((FIX(1.772) cb + 32768) >> 16)), cb = Cb - 128, cr = Cr - 128.
// Every output byte and every plane byte has one writer; there are no atomics.  The IDCT runs in 64-bit integers, so the
// formulas hold as written for any int16 coefficient (libjpeg itself wraps once pass-1 values leave 16 bits).
// The per-thread bodies are __host__ __device__ functions of a lane / thread index: ml_jpeg_decode_reference_host runs
// them in CPU loops.
#include "common.h"
#include <string.h>

namespace {

constexpr int TPB = 256;
constexpr int LANES = 8;                                           // lanes per 8x8 block
constexpr int BLOCKS_PER_WG = TPB / LANES;
constexpr int PITCH = 9, BLOCK_INTS = 72;                          // LDS: row pitch 9, 72 = 8 (mod 64): both passes hit 64 banks
constexpr uint32_t MAGIC = 0x4B50444Au;                            // "JDPK"
constexpr int MAX_SIDE = 16384;
constexpr int MAX_COMPONENTS = 3;

struct PackedHeader {
    uint32_t magic;
    int32_t height, width, mode;
    uint32_t blocks, entries, bytes, reserved;
    uint8_t q[MAX_COMPONENTS][64];                                 // per component, natural order
};
static_assert(sizeof(PackedHeader) == 224, "the packed header is 224 bytes");

struct Geometry {
    int mode, mw, mh;                                              // MCUs per row / column
    int yw, yh, cw, ch;                                            // padded planes (multiples of 8); cw = 0 for grayscale
    int real_cw, real_ch;                                          // the chroma samples that are real
    unsigned per_mcu, nblk;
    long long y_bytes, c_bytes;                                    // plane sizes, multiples of 16
};

struct Offsets {
    long long at[ML_JPEG_DECODE_MAX_BATCH];                        // byte offset of image b in the packed upload
};

long long round16(long long n) { return (n + 15) / 16 * 16; }

int geometry(int32_t H, int32_t W, int32_t mode, Geometry &g, const char *what) {
    ML_REQUIRE(H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE, "%s: bad dims (H %d, W %d; 1 .. %d)", what, H, W, MAX_SIDE);
    ML_REQUIRE(mode == ML_JPEG_GRAY || mode == ML_JPEG_444 || mode == ML_JPEG_420, "%s: bad mode %d", what, mode);
    const int unit = mode == ML_JPEG_420 ? 16 : 8;
    g.mode = mode;
    g.mw = (W + unit - 1) / unit;
    g.mh = (H + unit - 1) / unit;
    g.yw = g.mw * unit;
    g.yh = g.mh * unit;
    g.cw = mode == ML_JPEG_GRAY ? 0 : g.mw * 8;
    g.ch = mode == ML_JPEG_GRAY ? 0 : g.mh * 8;
    g.real_cw = mode == ML_JPEG_420 ? (W + 1) / 2 : W;
    g.real_ch = mode == ML_JPEG_420 ? (H + 1) / 2 : H;
    g.per_mcu = mode == ML_JPEG_GRAY ? 1u : mode == ML_JPEG_444 ? 3u : 6u;
    g.nblk = g.per_mcu * (unsigned)g.mw * (unsigned)g.mh;
    g.y_bytes = round16((long long)g.yw * g.yh);
    g.c_bytes = round16((long long)g.cw * g.ch);
    return ML_OK;
}

constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }

template <class T>
__host__ __device__ inline T clamp_to(T v, T lo, T hi) { return v < lo ? lo : v > hi ? hi : v; }

// ----------------------------------------------------------------------------- launch 1: eight lanes per block
// scan-order block g -> component and block coordinates in that component's plane
__host__ __device__ inline void block_place(unsigned g, int mode, int mw, int &comp, int &by, int &bx) {
    if (mode == ML_JPEG_420) {
        const unsigned mcu = g / 6u, b = g % 6u;
        const int my = (int)(mcu / (unsigned)mw), mx = (int)(mcu % (unsigned)mw);
        comp = b < 4u ? 0 : (int)b - 3;
        by = b < 4u ? 2 * my + (int)(b >> 1) : my;
        bx = b < 4u ? 2 * mx + (int)(b & 1u) : mx;
    } else {
        const unsigned per = mode == ML_JPEG_444 ? 3u : 1u, mcu = g / per;
        comp = (int)(g % per);
        by = (int)(mcu / (unsigned)mw);
        bx = (int)(mcu % (unsigned)mw);
    }
}

__host__ __device__ inline long long descale(long long x, int n) { return (x + (1ll << (n - 1))) >> n; }

// one 1-D pass of the LLM integer IDCT, in place
__host__ __device__ inline void idct_1d(long long v[8], int shift) {
    long long z1 = (v[2] + v[6]) * 4433;
    const long long t2 = z1 - v[6] * 15137, t3 = z1 + v[2] * 6270;
    const long long t0 = (v[0] + v[4]) * 8192, t1 = (v[0] - v[4]) * 8192;
    const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    long long o0 = v[7], o1 = v[5], o2 = v[3], o3 = v[1];
    z1 = o0 + o3;
    long long z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const long long z5 = (z3 + z4) * 9633;
    o0 *= 2446;
    o1 *= 16819;
    o2 *= 25172;
    o3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o0 += z1 + z3;
    o1 += z2 + z4;
    o2 += z2 + z3;
    o3 += z1 + z4;
    v[0] = descale(t10 + o3, shift);
    v[7] = descale(t10 - o3, shift);
    v[1] = descale(t11 + o2, shift);
    v[6] = descale(t11 - o2, shift);
    v[2] = descale(t12 + o1, shift);
    v[5] = descale(t12 - o1, shift);
    v[3] = descale(t13 + o0, shift);
    v[4] = descale(t13 - o0, shift);
}

// lane: row `lane` of the block's 8 x 9 LDS tile
__host__ __device__ inline void block_clear(int lane, int *w) {
#pragma unroll
    for (int k = 0; k < PITCH; ++k) w[lane * PITCH + k] = 0;
}

// lane: every eighth word of the block.  The host wrote indices below 64, distinct within the block.
__host__ __device__ inline void block_gather(int lane, const uint32_t *entries, uint32_t start, uint32_t end, const uint8_t *q, int *w) {
    for (uint32_t e = start + (uint32_t)lane; e < end; e += LANES) {
        const uint32_t word = entries[e], i = (word >> 16) & 63u;
        w[(i >> 3) * PITCH + (i & 7u)] = (int)(int16_t)(word & 0xFFFFu) * (int)q[i];
    }
}

// lane: column `lane`.  |pass-1 value| < 2^29 for any int16 coefficient and 8-bit table: it fits the int it is kept in.
__host__ __device__ inline void block_columns(int lane, int *w) {
    long long v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = w[r * PITCH + lane];
    idct_1d(v, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r * PITCH + lane] = (int)v[r];
}

__host__ __device__ inline void store_row(uint8_t *dst, uint32_t lo, uint32_t hi) {
#ifdef __HIP_DEVICE_COMPILE__
    *reinterpret_cast<uint2 *>(dst) = make_uint2(lo, hi);          // 8-byte aligned: plane bases, pitches and x are multiples of 8
#else
    const uint32_t v[2] = {lo, hi};
    memcpy(dst, v, 8);
#endif
}

// lane: row `lane` -> eight samples
__host__ __device__ inline void block_rows(int lane, const int *w, uint8_t *dst) {
    long long v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = w[lane * PITCH + k];
    idct_1d(v, 18);
    uint32_t out[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k >> 2] |= (uint32_t)clamp_to<long long>(v[k] + 128, 0, 255) << (8 * (k & 3));
    store_row(dst, out[0], out[1]);
}

__host__ __device__ inline void block_dc_only(uint32_t word, const uint8_t *q, uint8_t *dst) {
    const int dc = (int)(int16_t)(word & 0xFFFFu) * (int)q[0];
    const uint32_t s = (uint32_t)clamp_to(((dc + 4) >> 3) + 128, 0, 255) * 0x01010101u;
    store_row(dst, s, s);
}

struct ImageView {
    const PackedHeader *header;
    const uint32_t *block_start, *entries;
};

__host__ __device__ inline ImageView view_of(const uint8_t *packed, long long at, unsigned nblk) {
    ImageView v;
    v.header = reinterpret_cast<const PackedHeader *>(packed + at);
    v.block_start = reinterpret_cast<const uint32_t *>(packed + at + sizeof(PackedHeader));
    v.entries = v.block_start + nblk + 1;
    return v;
}

// where row `lane` of scan-order block g goes, and the block's dequantisation table
__host__ __device__ inline uint8_t *block_row_ptr(unsigned g, int lane, const Geometry &geo, const ImageView &im, uint8_t *planes,
                                                  const uint8_t *&q) {
    int comp, by, bx;
    block_place(g, geo.mode, geo.mw, comp, by, bx);
    q = im.header->q[comp];
    uint8_t *plane = comp == 0 ? planes : planes + geo.y_bytes + (comp - 1) * geo.c_bytes;
    const int pitch = comp == 0 ? geo.yw : geo.cw;
    return plane + (size_t)(by * 8 + lane) * pitch + bx * 8;
}

__global__ __launch_bounds__(TPB) void jpeg_decode_blocks_kernel(const uint8_t *packed, Offsets offsets, uint8_t *planes, Geometry geo) {
    __shared__ int lds[BLOCKS_PER_WG * BLOCK_INTS];
    const int lane = threadIdx.x & (LANES - 1), slot = threadIdx.x / LANES;
    const unsigned g = blockIdx.x * BLOCKS_PER_WG + slot;
    const bool live = g < geo.nblk;
    const ImageView im = view_of(packed, offsets.at[blockIdx.y], geo.nblk);
    int *w = lds + slot * BLOCK_INTS;
    uint32_t start = 0, end = 0;
    if (live) {
        start = im.block_start[g];
        end = im.block_start[g + 1];
    }
    const bool full = live && end - start != 1u;                   // every thread reaches the barriers
    const uint8_t *q = nullptr;
    uint8_t *dst = nullptr;
    if (live) dst = block_row_ptr(g, lane, geo, im, planes + (size_t)blockIdx.y * (geo.y_bytes + 2 * geo.c_bytes), q);
    if (full) block_clear(lane, w);
    __syncthreads();
    if (full) block_gather(lane, im.entries, start, end, q, w);
    __syncthreads();
    if (full) block_columns(lane, w);
    __syncthreads();
    if (full) block_rows(lane, w, dst);
    else if (live) block_dc_only(im.entries[start], q, dst);
}

// ----------------------------------------------------------------------------- launch 2: four output bytes per thread
__host__ __device__ inline int upsampled(const uint8_t *p, int pitch, int r, int rn, int cx, int xn, int odd_x) {
    const int s0 = 3 * p[(size_t)r * pitch + cx] + p[(size_t)rn * pitch + cx];
    const int s1 = 3 * p[(size_t)r * pitch + xn] + p[(size_t)rn * pitch + xn];
    return (3 * s0 + s1 + (odd_x ? 7 : 8)) >> 4;
}

__host__ __device__ inline void pixel_rgb(const uint8_t *planes, const Geometry &geo, int y, int x, int rgb[3]) {
    const int Y = planes[(size_t)y * geo.yw + x];
    if (geo.mode == ML_JPEG_GRAY) {
        rgb[0] = rgb[1] = rgb[2] = Y;
        return;
    }
    const uint8_t *cbp = planes + geo.y_bytes, *crp = cbp + geo.c_bytes;
    int cb, cr;
    if (geo.mode == ML_JPEG_444) {
        cb = cbp[(size_t)y * geo.cw + x];
        cr = crp[(size_t)y * geo.cw + x];
    } else {
        const int r = y >> 1, cx = x >> 1;
        const int rn = (y & 1) ? (r + 1 < geo.real_ch ? r + 1 : r) : (r > 0 ? r - 1 : 0);
        const int xn = (x & 1) ? (cx + 1 < geo.real_cw ? cx + 1 : cx) : (cx > 0 ? cx - 1 : 0);
        cb = upsampled(cbp, geo.cw, r, rn, cx, xn, x & 1);
        cr = upsampled(crp, geo.cw, r, rn, cx, xn, x & 1);
    }
    cb -= 128;
    cr -= 128;
    rgb[0] = clamp_to(Y + ((fix16(1.402) * cr + 32768) >> 16), 0, 255);
    rgb[1] = clamp_to(Y + ((-fix16(0.34414) * cb + 32768 - fix16(0.71414) * cr) >> 16), 0, 255);
    rgb[2] = clamp_to(Y + ((fix16(1.772) * cb + 32768) >> 16), 0, 255);
}

// t: bytes 4 t .. 4 t + 3 of the flat [B,H,W,3] output (they span at most two pixels); total = B H W 3 < 2^31 (checked by
// the entry point: 32-bit divisions are several times cheaper than 64-bit ones)
typedef uint32_t Index;
__host__ __device__ inline void pixels_body(Index t, const uint8_t *planes, const Geometry &geo, int H, int W, Index total, uint8_t *out) {
    const Index first = 4 * t;
    if (first >= total) return;
    const long long plane_stride = geo.y_bytes + 2 * geo.c_bytes;
    Index pixel = first / 3;
    int channel = (int)(first - pixel * 3);
    int rgb[3];
    bool have = false;
    uint32_t word = 0;
    const int n = total - first < 4 ? (int)(total - first) : 4;
    for (int k = 0; k < n; ++k) {
        if (!have) {
            const Index row = pixel / (Index)W, b = row / (Index)H;   // row over the whole batch
            pixel_rgb(planes + (long long)b * plane_stride, geo, (int)(row - b * (Index)H), (int)(pixel - row * (Index)W), rgb);
            have = true;
        }
        word |= (uint32_t)(channel == 0 ? rgb[0] : channel == 1 ? rgb[1] : rgb[2]) << (8 * k);
        if (++channel == 3) {
            channel = 0;
            ++pixel;
            have = false;
        }
    }
    if (n == 4) {
#ifdef __HIP_DEVICE_COMPILE__
        *reinterpret_cast<uint32_t *>(out + first) = word;         // `out` is 4-byte aligned (checked by the entry point)
#else
        memcpy(out + first, &word, 4);
#endif
    } else {
        for (int k = 0; k < n; ++k) out[first + k] = (uint8_t)(word >> (8 * k));
    }
}

__global__ __launch_bounds__(TPB) void jpeg_decode_pixels_kernel(const uint8_t *planes, Geometry geo, int H, int W, Index total, uint8_t *out) {
    pixels_body((Index)blockIdx.x * TPB + threadIdx.x, planes, geo, H, W, total, out);
}

// ----------------------------------------------------------------------------- host: the stream
constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTable {
    bool defined = false;
    uint16_t fast[512];                                            // 9 bits of lookahead -> length << 8 | symbol, 0: longer
    int32_t maxcode[17];                                           // largest code of each length, -1: none
    int32_t valoff[17];                                            // index of a length's first symbol minus its first code
    int nvals = 0;
    uint8_t vals[256];
};

struct Component {
    int id, h, v, tq, td, ta;
};

struct Stream {
    int H = 0, W = 0, ncomp = 0, mode = -1, restart = 0;
    Component comp[MAX_COMPONENTS];
    bool q_defined[4] = {false, false, false, false};
    uint8_t q[4][64];                                              // natural order
    HuffTable dc[4], ac[4];
    int64_t scan = 0;                                              // first byte of entropy-coded data
};

enum { PARSE_OK = 0, PARSE_UNSUPPORTED = 1, PARSE_MALFORMED = -1 };

#define JD_FAIL(code, ...)          \
    do {                            \
        ml_set_error(__VA_ARGS__);  \
        return code;                \
    } while (0)

int build_huffman(const uint8_t *bits, const uint8_t *vals, int n, HuffTable &t) {
    memset(t.fast, 0, sizeof(t.fast));
    t.defined = false;
    int32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        t.valoff[len] = k - code;
        if (code + bits[len - 1] > (1 << len)) return PARSE_MALFORMED;   // more codes than the length holds: before any store
        for (int j = 0; j < bits[len - 1]; ++j, ++k, ++code) {
            if (len <= 9)
                for (int f = 0; f < (1 << (9 - len)); ++f) t.fast[(code << (9 - len)) | f] = (uint16_t)(len << 8 | vals[k]);
        }
        t.maxcode[len] = bits[len - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t.nvals = n;
    memcpy(t.vals, vals, (size_t)n);
    t.defined = true;
    return PARSE_OK;
}

// Everything up to and including SOS.  PARSE_UNSUPPORTED: a stream the device path does not take (the text says why).
int parse_stream(const uint8_t *d, int64_t n, Stream &s, const char *what) {
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: not a JPEG (no SOI)", what);
    bool jfif = false, adobe = false, have_frame = false;
    int adobe_transform = -1;
    int64_t i = 2;
    for (;;) {
        if (i + 2 > n) JD_FAIL(PARSE_MALFORMED, "%s: truncated: the stream ends before SOS", what);
        if (d[i] != 0xFF) JD_FAIL(PARSE_MALFORMED, "%s: marker expected at byte %lld", what, (long long)i);
        const int m = d[i + 1];
        if (m == 0xFF) {                                           // fill byte
            ++i;
            continue;
        }
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {               // TEM, RSTn: no length
            i += 2;
            continue;
        }
        if (m == 0xD8 || m == 0xD9 || m == 0x00) JD_FAIL(PARSE_MALFORMED, "%s: marker 0xFF%02X before SOS", what, m);
        if (i + 4 > n) JD_FAIL(PARSE_MALFORMED, "%s: truncated segment 0xFF%02X", what, m);
        const int64_t L = (d[i + 2] << 8) | d[i + 3];
        if (L < 2 || i + 2 + L > n) JD_FAIL(PARSE_MALFORMED, "%s: truncated segment 0xFF%02X", what, m);
        const uint8_t *seg = d + i + 4;
        const int64_t len = L - 2;
        if (m == 0xDB) {
            int64_t p = 0;
            while (p < len) {
                if (seg[p] >> 4) JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: 16-bit quantisation table", what);
                const int id = seg[p] & 15;
                if (id > 3 || p + 65 > len) JD_FAIL(PARSE_MALFORMED, "%s: bad DQT segment", what);
                for (int k = 0; k < 64; ++k) s.q[id][ZIGZAG[k]] = seg[p + 1 + k];
                s.q_defined[id] = true;
                p += 65;
            }
        } else if (m == 0xC4) {
            int64_t p = 0;
            while (p < len) {
                if (p + 17 > len) JD_FAIL(PARSE_MALFORMED, "%s: truncated DHT segment", what);
                const int cls = seg[p] >> 4, id = seg[p] & 15;
                int count = 0;
                for (int k = 0; k < 16; ++k) count += seg[p + 1 + k];
                if (cls > 1 || id > 3 || count > 256 || p + 17 + count > len) JD_FAIL(PARSE_MALFORMED, "%s: bad DHT segment", what);
                if (build_huffman(seg + p + 1, seg + p + 17, count, cls ? s.ac[id] : s.dc[id]) != PARSE_OK)
                    JD_FAIL(PARSE_MALFORMED, "%s: bad DHT segment: more codes than their length holds", what);
                p += 17 + count;
            }
        } else if (m == 0xC0) {
            if (have_frame) JD_FAIL(PARSE_MALFORMED, "%s: two frame headers", what);
            if (len < 6) JD_FAIL(PARSE_MALFORMED, "%s: truncated SOF0", what);
            if (seg[0] != 8) JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: %d-bit samples", what, seg[0]);
            s.H = (seg[1] << 8) | seg[2];
            s.W = (seg[3] << 8) | seg[4];
            s.ncomp = seg[5];
            if (s.ncomp != 1 && s.ncomp != 3) JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: %d components", what, s.ncomp);
            if (len < 6 + 3 * s.ncomp) JD_FAIL(PARSE_MALFORMED, "%s: truncated SOF0", what);
            if (s.H == 0 || s.W == 0) JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: a zero dimension in SOF0 (%d x %d)", what, s.H, s.W);
            if (s.H > MAX_SIDE || s.W > MAX_SIDE)
                JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: %d x %d is above %d a side", what, s.H, s.W, MAX_SIDE);
            for (int c = 0; c < s.ncomp; ++c) {
                Component &k = s.comp[c];
                k.id = seg[6 + 3 * c];
                k.h = seg[7 + 3 * c] >> 4;
                k.v = seg[7 + 3 * c] & 15;
                k.tq = seg[8 + 3 * c];
                if (k.tq > 3) JD_FAIL(PARSE_MALFORMED, "%s: quantisation table id %d", what, k.tq);
            }
            have_frame = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC8) {          // (0xC4 was taken above; 0xCC is DAC)
            JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: not a baseline Huffman frame (marker 0xFF%02X)", what, m);
        } else if (m == 0xDD) {
            if (len < 2) JD_FAIL(PARSE_MALFORMED, "%s: truncated DRI", what);
            s.restart = (seg[0] << 8) | seg[1];
        } else if (m == 0xE0) {
            if (len >= 5 && memcmp(seg, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (len >= 12 && memcmp(seg, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = seg[11];
            }
        } else if (m == 0xDA) {
            if (!have_frame) JD_FAIL(PARSE_MALFORMED, "%s: SOS before SOF0", what);
            if (len < 1) JD_FAIL(PARSE_MALFORMED, "%s: truncated SOS", what);
            const int ns = seg[0];
            if (ns != s.ncomp) JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: a scan of %d of the %d components", what, ns, s.ncomp);
            if (len < 1 + 2 * ns + 3) JD_FAIL(PARSE_MALFORMED, "%s: truncated SOS", what);
            for (int c = 0; c < ns; ++c) {
                if (seg[1 + 2 * c] != s.comp[c].id) JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: scan components out of frame order", what);
                s.comp[c].td = seg[2 + 2 * c] >> 4;
                s.comp[c].ta = seg[2 + 2 * c] & 15;
                if (s.comp[c].td > 3 || s.comp[c].ta > 3) JD_FAIL(PARSE_MALFORMED, "%s: Huffman table id above 3", what);
            }
            if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0)
                JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: not a whole-block sequential scan", what);
            s.scan = i + 2 + L;
            break;
        }                                                          // APPn, COM and anything else with a length: skipped
        i += 2 + L;
    }
    if (s.ncomp == 1) {
        if (s.comp[0].h != 1 || s.comp[0].v != 1) JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: grayscale sampled %dx%d", what, s.comp[0].h, s.comp[0].v);
        s.mode = ML_JPEG_GRAY;
    } else {
        if (adobe && adobe_transform != 1) JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: Adobe transform %d (not YCbCr)", what, adobe_transform);
        if (!jfif && !adobe && s.comp[0].id == 'R' && s.comp[1].id == 'G' && s.comp[2].id == 'B')
            JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: components R, G, B without a JFIF marker", what);
        const bool chroma_1x1 = s.comp[1].h == 1 && s.comp[1].v == 1 && s.comp[2].h == 1 && s.comp[2].v == 1;
        if (chroma_1x1 && s.comp[0].h == 2 && s.comp[0].v == 2) s.mode = ML_JPEG_420;
        else if (chroma_1x1 && s.comp[0].h == 1 && s.comp[0].v == 1) s.mode = ML_JPEG_444;
        else
            JD_FAIL(PARSE_UNSUPPORTED, "%s: unsupported: sampling %dx%d / %dx%d / %dx%d", what, s.comp[0].h, s.comp[0].v, s.comp[1].h,
                    s.comp[1].v, s.comp[2].h, s.comp[2].v);
    }
    return PARSE_OK;
}

// Bits of the entropy-coded segment, most significant first; FF 00 is one FF byte, any other marker ends the supply.
struct BitReader {
    const uint8_t *p, *end;
    uint64_t acc = 0;
    int avail = 0;
    bool stopped = false;
    void refill() {
        while (avail <= 56 && !stopped) {
            if (p >= end) {
                stopped = true;
                break;
            }
            const uint8_t b = *p;
            if (b == 0xFF) {
                if (p + 1 >= end || p[1] != 0) {
                    stopped = true;
                    break;
                }
                p += 2;
            } else {
                ++p;
            }
            acc = (acc << 8) | b;
            avail += 8;
        }
    }
    // the next n <= 16 bits, zeros past the end
    uint32_t peek(int n) const {
        const uint64_t v = avail >= n ? acc >> (avail - n) : acc << (n - avail);
        return (uint32_t)(v & ((1u << n) - 1u));
    }
};

enum { BITS_OK = 0, BITS_TRUNCATED = -1, BITS_NO_CODE = -2 };

inline int decode_symbol(BitReader &br, const HuffTable &t) {
    if (br.avail < 16) br.refill();
    const uint16_t e = t.fast[br.peek(9)];
    if (e) {
        const int len = e >> 8;
        if (len > br.avail) return BITS_TRUNCATED;
        br.avail -= len;
        return e & 255;
    }
    for (int len = 10; len <= 16; ++len) {
        const int32_t code = (int32_t)br.peek(len);
        if (t.maxcode[len] >= 0 && code <= t.maxcode[len]) {
            if (len > br.avail) return BITS_TRUNCATED;
            const int32_t at = t.valoff[len] + code;
            if (at < 0 || at >= t.nvals) return BITS_NO_CODE;
            br.avail -= len;
            return t.vals[at];
        }
    }
    return br.avail < 16 ? BITS_TRUNCATED : BITS_NO_CODE;
}

// `size` more bits as the signed value of T.81 F.2.2.1 (EXTEND); ok = false if the scan ends first
inline int receive_extend(BitReader &br, int size, bool &ok) {
    if (size == 0) return 0;
    if (br.avail < size) br.refill();
    if (br.avail < size) {
        ok = false;
        return 0;
    }
    const int v = (int)br.peek(size);
    br.avail -= size;
    return v >> (size - 1) ? v : v - (1 << size) + 1;
}

long long packed_bound(const Geometry &g, int64_t n) {
    // an AC word costs the scan at least two bits (a code and a magnitude bit), a block's DC word is always there
    const long long by_blocks = 64ll * g.nblk, by_bits = (long long)g.nblk + 4ll * n;
    return round16((long long)sizeof(PackedHeader) + 4ll * (g.nblk + 1) + 4ll * (by_blocks < by_bits ? by_blocks : by_bits));
}

}  // namespace

extern "C" int ml_jpeg_decode_info(const uint8_t *data, int64_t n, int32_t *info) {
    ML_REQUIRE(info, "jpeg_decode_info: null pointer");
    info[0] = info[1] = info[3] = 0;
    info[2] = -1;
    if (!data || n <= 0) {
        ml_set_error("jpeg_decode_info: unsupported: not a JPEG (empty)");
        return ML_JPEG_UNSUPPORTED;
    }
    Stream s;
    if (parse_stream(data, n, s, "jpeg_decode_info") != PARSE_OK) return ML_JPEG_UNSUPPORTED;   // a header that cannot be read is not vouched for
    Geometry g;
    if (geometry(s.H, s.W, s.mode, g, "jpeg_decode_info") != ML_OK) return ML_JPEG_UNSUPPORTED;
    info[0] = s.H;
    info[1] = s.W;
    info[2] = s.mode;
    info[3] = (int32_t)g.nblk;
    return ML_OK;
}

extern "C" int64_t ml_jpeg_decode_packed_bytes(const uint8_t *data, int64_t n) {
    ML_REQUIRE(data && n > 0, "jpeg_decode_packed_bytes: null pointer or empty stream");
    Stream s;
    if (parse_stream(data, n, s, "jpeg_decode_packed_bytes") != PARSE_OK) return ML_E_BADARG;
    Geometry g;
    const int e = geometry(s.H, s.W, s.mode, g, "jpeg_decode_packed_bytes");
    return e != ML_OK ? e : packed_bound(g, n);
}

extern "C" int64_t ml_jpeg_decode_entropy(const uint8_t *data, int64_t n, void *packed, int64_t capacity) {
    const char *what = "jpeg_decode_entropy";
    ML_REQUIRE(data && n > 0 && packed, "%s: null pointer or empty stream", what);
    ML_REQUIRE((((uintptr_t)packed) & 3u) == 0, "%s: packed must be 4-byte aligned", what);
    Stream s;
    if (parse_stream(data, n, s, what) != PARSE_OK) return ML_E_BADARG;
    Geometry g;
    int e = geometry(s.H, s.W, s.mode, g, what);
    if (e != ML_OK) return e;
    for (int c = 0; c < s.ncomp; ++c) {
        ML_REQUIRE(s.q_defined[s.comp[c].tq], "%s: quantisation table %d is not defined", what, s.comp[c].tq);
        ML_REQUIRE(s.dc[s.comp[c].td].defined, "%s: DC Huffman table %d is not defined", what, s.comp[c].td);
        ML_REQUIRE(s.ac[s.comp[c].ta].defined, "%s: AC Huffman table %d is not defined", what, s.comp[c].ta);
    }
    const long long fixed = (long long)sizeof(PackedHeader) + 4ll * (g.nblk + 1);
    ML_REQUIRE(capacity >= fixed + 4ll * g.nblk, "%s: capacity %lld is below the header, the offsets and one word a block (%lld)", what,
               (long long)capacity, fixed + 4ll * g.nblk);
    const long long room = (capacity - fixed) / 4;                 // words
    PackedHeader *h = (PackedHeader *)packed;
    uint32_t *block_start = (uint32_t *)((uint8_t *)packed + sizeof(PackedHeader));
    uint32_t *entries = block_start + g.nblk + 1;

    int comp_of[6] = {0, 0, 0, 0, 1, 2};                           // 4:2:0; 4:4:4 is 0 1 2, grayscale 0
    if (s.mode == ML_JPEG_444) comp_of[1] = 1, comp_of[2] = 2;
    BitReader br;
    br.p = data + s.scan;
    br.end = data + n;
    int pred[MAX_COMPONENTS] = {0, 0, 0};
    const unsigned nmcu = (unsigned)g.mw * (unsigned)g.mh;
    long long ne = 0;
    unsigned blk = 0, rst = 0;
    for (unsigned mcu = 0; mcu < nmcu; ++mcu) {
        if (s.restart && mcu && mcu % (unsigned)s.restart == 0) {  // the bits left are padding; the marker follows them
            br.acc = 0;
            br.avail = 0;
            while (br.p + 2 < br.end && br.p[0] == 0xFF && br.p[1] == 0xFF) ++br.p;   // fill bytes before a marker (T.81 B.1.1.2)
            ML_REQUIRE(br.p + 2 <= br.end && br.p[0] == 0xFF && br.p[1] == 0xD0 + (rst & 7u),
                       "%s: RST%u expected before MCU %u (byte %lld)", what, rst & 7u, mcu, (long long)(br.p - data));
            br.p += 2;
            br.stopped = false;
            ++rst;
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (unsigned b = 0; b < g.per_mcu; ++b, ++blk) {
            const int c = comp_of[b];
            const HuffTable &dc = s.dc[s.comp[c].td], &ac = s.ac[s.comp[c].ta];
            block_start[blk] = (uint32_t)ne;
            int sym = decode_symbol(br, dc);
            ML_REQUIRE(sym != BITS_TRUNCATED, "%s: the scan ends inside block %u", what, blk);
            ML_REQUIRE(sym != BITS_NO_CODE, "%s: block %u: a code that is not in DC table %d", what, blk, s.comp[c].td);
            ML_REQUIRE(sym <= 11, "%s: block %u: DC category %d above 11", what, blk, sym);
            bool ok = true;
            pred[c] += receive_extend(br, sym, ok);
            ML_REQUIRE(ok, "%s: the scan ends inside block %u", what, blk);
            ML_REQUIRE(ne < room, "%s: the packed buffer is full at block %u (capacity %lld)", what, blk, (long long)capacity);
            entries[ne++] = (uint32_t)(uint16_t)(int16_t)pred[c];  // index 0
            int k = 1;
            while (k < 64) {
                sym = decode_symbol(br, ac);
                ML_REQUIRE(sym != BITS_TRUNCATED, "%s: the scan ends inside block %u", what, blk);
                ML_REQUIRE(sym != BITS_NO_CODE, "%s: block %u: a code that is not in AC table %d", what, blk, s.comp[c].ta);
                const int run = sym >> 4, size = sym & 15;
                if (size == 0) {
                    if (run == 15) {
                        k += 16;
                        ML_REQUIRE(k <= 64, "%s: block %u: a zero run past coefficient 63", what, blk);
                        continue;
                    }
                    ML_REQUIRE(run == 0, "%s: block %u: run/size symbol 0x%02X", what, blk, sym);
                    break;
                }
                ML_REQUIRE(size <= 10, "%s: block %u: AC size %d above 10", what, blk, size);
                k += run;
                ML_REQUIRE(k <= 63, "%s: block %u: a run past coefficient 63", what, blk);
                const int v = receive_extend(br, size, ok);
                ML_REQUIRE(ok, "%s: the scan ends inside block %u", what, blk);
                ML_REQUIRE(ne < room, "%s: the packed buffer is full at block %u (capacity %lld)", what, blk, (long long)capacity);
                entries[ne++] = (uint32_t)ZIGZAG[k] << 16 | (uint32_t)(uint16_t)(int16_t)v;
                ++k;
            }
        }
    }
    block_start[g.nblk] = (uint32_t)ne;
    // EOI: what is left in the reader is padding; bytes that are no marker are passed over as libjpeg does
    const uint8_t *p = br.p;
    for (;;) {
        ML_REQUIRE(p + 2 <= br.end, "%s: no EOI after the last MCU", what);
        if (p[0] == 0xFF && p[1] == 0xD9) break;
        ML_REQUIRE(!(p[0] == 0xFF && p[1] != 0x00 && p[1] != 0xFF), "%s: marker 0xFF%02X where EOI was expected", what, p[1]);
        ++p;
    }
    const long long bytes = round16(fixed + 4ll * ne);
    h->magic = MAGIC;
    h->height = s.H;
    h->width = s.W;
    h->mode = s.mode;
    h->blocks = g.nblk;
    h->entries = (uint32_t)ne;
    h->bytes = (uint32_t)(bytes <= capacity ? bytes : fixed + 4ll * ne);
    h->reserved = 0;
    memset(h->q, 0, sizeof(h->q));
    for (int c = 0; c < s.ncomp; ++c) memcpy(h->q[c], s.q[s.comp[c].tq], 64);
    if (bytes <= capacity) memset((uint8_t *)packed + fixed + 4ll * ne, 0, (size_t)(bytes - fixed - 4ll * ne));
    return h->bytes;
}

extern "C" int64_t ml_jpeg_decode_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t mode) {
    Geometry g;
    const int e = geometry(H, W, mode, g, "jpeg_decode_workspace_bytes");
    if (e != ML_OK) return e;
    ML_REQUIRE(B > 0 && B <= ML_JPEG_DECODE_MAX_BATCH, "jpeg_decode_workspace_bytes: bad dims (B %d; 1 .. %d)", B, ML_JPEG_DECODE_MAX_BATCH);
    return (long long)B * (g.y_bytes + 2 * g.c_bytes);
}

namespace {
int check_call(const char *what, const void *packed, const int64_t *offsets, int32_t B, int32_t H, int32_t W, int32_t mode,
               const uint8_t *out, const void *workspace, Geometry &g, Offsets &o) {
    ML_REQUIRE(packed && offsets && out && workspace, "%s: null pointer", what);
    ML_REQUIRE(B > 0 && B <= ML_JPEG_DECODE_MAX_BATCH, "%s: bad dims (B %d; 1 .. %d)", what, B, ML_JPEG_DECODE_MAX_BATCH);
    const int e = geometry(H, W, mode, g, what);
    if (e != ML_OK) return e;
    ML_REQUIRE((long long)B * H * W * 3 < (1ll << 31), "%s: the frames of a call must stay below 2^31 bytes (B %d, H %d, W %d)", what, B, H, W);
    ML_REQUIRE(ml_aligned16(packed) && ml_aligned16(workspace), "%s: packed and workspace must be 16-byte aligned", what);
    ML_REQUIRE((((uintptr_t)out) & 3u) == 0, "%s: out must be 4-byte aligned", what);
    const long long least = (long long)sizeof(PackedHeader) + 4ll * (g.nblk + 1) + 4ll * g.nblk;
    for (int b = 0; b < B; ++b) {
        ML_REQUIRE(offsets[b] >= 0 && offsets[b] % 16 == 0 && offsets[b + 1] - offsets[b] >= least,
                   "%s: offsets[%d] = %lld, offsets[%d] = %lld: 16-byte aligned images of at least %lld bytes expected", what, b,
                   (long long)offsets[b], b + 1, (long long)offsets[b + 1], least);
        o.at[b] = offsets[b];
    }
    for (int b = B; b < ML_JPEG_DECODE_MAX_BATCH; ++b) o.at[b] = 0;
    return ML_OK;
}
}  // namespace

extern "C" int ml_jpeg_decode_u8(const void *packed, const int64_t *offsets, int32_t B, int32_t H, int32_t W, int32_t mode,
                                 uint8_t *out, void *workspace, void *stream) {
    Geometry g;
    Offsets o;
    const int e = check_call("jpeg_decode", packed, offsets, B, H, W, mode, out, workspace, g, o);
    if (e != ML_OK) return e;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_decode_blocks_kernel, dim3((g.nblk + BLOCKS_PER_WG - 1) / BLOCKS_PER_WG, B), dim3(TPB), 0, s,
                       (const uint8_t *)packed, o, (uint8_t *)workspace, g);
    const long long total = (long long)B * H * W * 3, threads = (total + 3) / 4;
    hipLaunchKernelGGL(jpeg_decode_pixels_kernel, dim3((unsigned)((threads + TPB - 1) / TPB)), dim3(TPB), 0, s,
                       (const uint8_t *)workspace, g, H, W, (Index)total, out);
    ML_CHECK_LAUNCH("jpeg_decode");
    return ML_OK;
}

// The same per-thread bodies in CPU loops, every pointer in host memory: the arithmetic without a device.  It also
// checks what the kernels rely on (magic, geometry, indices, offsets), since here the packed form can be read.
extern "C" int ml_jpeg_decode_reference_host(const void *packed, const int64_t *offsets, int32_t B, int32_t H, int32_t W,
                                             int32_t mode, uint8_t *out, void *workspace) {
    const char *what = "jpeg_decode_reference_host";
    Geometry g;
    Offsets o;
    const int e = check_call(what, packed, offsets, B, H, W, mode, out, workspace, g, o);
    if (e != ML_OK) return e;
    const long long plane_stride = g.y_bytes + 2 * g.c_bytes;
    for (int b = 0; b < B; ++b) {
        const ImageView im = view_of((const uint8_t *)packed, o.at[b], g.nblk);
        const PackedHeader &h = *im.header;
        ML_REQUIRE(h.magic == MAGIC && h.height == H && h.width == W && h.mode == mode && h.blocks == g.nblk,
                   "%s: image %d is not a packed %d x %d stream of mode %d", what, b, H, W, mode);
        ML_REQUIRE((long long)h.bytes <= offsets[b + 1] - offsets[b] && im.block_start[0] == 0 && im.block_start[g.nblk] == h.entries &&
                   (long long)sizeof(PackedHeader) + 4ll * (g.nblk + 1) + 4ll * h.entries <= (long long)h.bytes,
                   "%s: image %d: sizes disagree", what, b);
        for (unsigned k = 0; k < g.nblk; ++k) {
            const uint32_t n = im.block_start[k + 1] - im.block_start[k];
            ML_REQUIRE(im.block_start[k + 1] > im.block_start[k] && n <= 64 && im.entries[im.block_start[k]] >> 16 == 0,
                       "%s: image %d: block %u has %u words or no DC word", what, b, k, n);
        }
        uint8_t *planes = (uint8_t *)workspace + b * plane_stride;
        int w[BLOCK_INTS];
        for (unsigned k = 0; k < g.nblk; ++k) {
            const uint32_t start = im.block_start[k], end = im.block_start[k + 1];
            const uint8_t *q = nullptr;
            if (end - start == 1u) {
                for (int lane = 0; lane < LANES; ++lane) {
                    uint8_t *dst = block_row_ptr(k, lane, g, im, planes, q);
                    block_dc_only(im.entries[start], q, dst);
                }
                continue;
            }
            block_row_ptr(k, 0, g, im, planes, q);
            for (int lane = 0; lane < LANES; ++lane) block_clear(lane, w);
            for (int lane = 0; lane < LANES; ++lane) block_gather(lane, im.entries, start, end, q, w);
            for (int lane = 0; lane < LANES; ++lane) block_columns(lane, w);
            for (int lane = 0; lane < LANES; ++lane) block_rows(lane, w, block_row_ptr(k, lane, g, im, planes, q));
        }
    }
    const long long total = (long long)B * H * W * 3;
    for (long long t = 0; t < (total + 3) / 4; ++t) pixels_body((Index)t, (const uint8_t *)workspace, g, H, W, (Index)total, out);
    return ML_OK;
}

// ============================================================================= entropy decoding on the device
// The Huffman half of the decoder as kernels: the raw file and a small plan go up, the packed form above comes out, byte
// for byte what ml_jpeg_decode_entropy writes.  Self-synchronising parallel decoding: the scan is cut into subsequences of
// SUB_BYTES raw bytes, one thread each.
//   1 sync    (SYNC_LAUNCHES launches of one kernel) every thread decodes its subsequence from a guessed state (bit 0 of
//             its first byte, block 0 of an MCU, k = 0; thread 0 of a stream holds the true state) and keeps its exit
//             state and counts: words, blocks, the DC differences summed per component since the last restart marker.
//             Then, at most SYNC_ROUNDS times, every thread takes its predecessor's exit state as its entry state and,
//             if that changed it, decodes again; a workgroup whose states all agree stops.  The first thread of a
//             workgroup takes the exit state the previous workgroup's last thread left in the launch before (two
//             buffers, one per launch parity: no workgroup waits on or races with another).
//   2 scan    one workgroup per stream: exclusive prefix of (words, blocks, DC predictors) over the subsequences, the
//             predictors restarting where a subsequence saw a restart marker.
//   3 write   decode once more from the settled entry states, storing block_start and the words (the DC word already
//             un-predicted: the predictor at entry comes from the scan).  Every malformed-stream condition of the host
//             decoder counts here, every store is bounded, and each thread compares its exit state with its successor's
//             entry state: a stream whose states had not settled ends ML_JPEG_ENTROPY_NOT_SYNCED, never with wrong words
//             under status 0.  The thread that completes the last block looks for EOI and writes the header.
//   4 finish  folds the error word and the done flag into the stream's four status words, and clears the packed words of
//             a stream that failed: the block and pixel kernels may follow in the stream before anybody reads a status.
// A state is (raw bit position, k, block in MCU, fresh: nothing decoded since a restart marker, end: the supply ended).
// In a guessed state nothing is an error: a code that is not in the table consumes 16 bits as symbol 0, a bad category
// or run ends the block, a symbol the supply cannot finish jumps over an RSTn marker (block 0, k = 0) or ends the thread.
// The write pass applies the same rules, so its counts are those of the sync pass, and records the error.
// One answer of the host decoder depends on how far its 64-bit reader has read ahead, which no thread can know: whether
// it takes a due restart marker that whole bytes separate from the MCU's last bit.  That ends ML_JPEG_ENTROPY_ASK_HOST:
// the caller runs the host decoder, as for every non-zero status.  (The EOI rule needs no search: the plan names the
// scan's first marker that is no RSTn, and the last RSTn before it.)
namespace {

constexpr int SUB_BYTES = 128, SUB_BITS = 8 * SUB_BYTES;           // one thread's share of the raw scan
constexpr int SYNC_TPB = 256;                                      // subsequences per workgroup
constexpr int SYNC_ROUNDS = SYNC_TPB, SYNC_LAUNCHES = 3;           // a state can cross a whole workgroup in one launch
constexpr int FILL_SKIP = 16;                                      // fill bytes passed over before a marker
constexpr uint32_t PLAN_MAGIC = 0x4E4C504Au;                       // "JPLN"
constexpr int64_t MAX_FILE = 1ll << 28;                            // bit positions stay below 2^31

struct DevTable {
    uint16_t fast[512];
    int32_t maxcode[17], valoff[17], nvals;
    uint8_t vals[256];
};

struct Plan {
    uint32_t magic;
    int32_t height, width, mode;
    uint32_t nblk, per_mcu, restart, scan, n, nsub;
    uint32_t end_marker, last_rst;                                 // first marker of the scan that is no RSTn (n: none); last RSTn before it + 1 (0: none)
    uint8_t q[MAX_COMPONENTS][64];
    uint8_t zigzag[64];
    DevTable dc[MAX_COMPONENTS], ac[MAX_COMPONENTS];               // by component
};
static_assert(sizeof(Plan) % 8 == 0, "plans are copied as words");
constexpr int PLAN_BYTES = (int)((sizeof(Plan) + 15) / 16 * 16);

struct State {
    uint32_t pos, kb;                                              // kb: k | block in MCU << 8 | fresh << 16 | end << 17
};
constexpr uint32_t FRESH = 1u << 16, END = 1u << 17;
__host__ __device__ inline bool same(const State &a, const State &b) { return a.pos == b.pos && a.kb == b.kb; }

struct Count {
    uint32_t words, blocks;
    int32_t dc0, dc1, dc2;
    uint32_t reset;
};

// a then b
__host__ __device__ inline Count combine(const Count &a, const Count &b) {
    Count c;
    c.words = a.words + b.words;
    c.blocks = a.blocks + b.blocks;
    c.dc0 = b.reset ? b.dc0 : a.dc0 + b.dc0;
    c.dc1 = b.reset ? b.dc1 : a.dc1 + b.dc1;
    c.dc2 = b.reset ? b.dc2 : a.dc2 + b.dc2;
    c.reset = a.reset | b.reset;
    return c;
}

// one stream's share of the workspace
struct Region {
    State *entry, *exit, *wg_exit;                                 // [nsub], [nsub], [2][nwg]
    Count *count, *prefix;                                         // [nsub]
    uint32_t *ctl;                                                 // error word (code << 24 | block), done, most rounds, last launch that changed a state
};

__host__ __device__ inline uint32_t sub_cap_of(uint32_t n) { return (n + SUB_BYTES - 1) / SUB_BYTES; }   // whatever the scan's offset
inline uint32_t sub_bound(int64_t n) { return sub_cap_of((uint32_t)n); }
inline uint32_t wg_bound(int64_t n) { return (sub_bound(n) + SYNC_TPB - 1) / SYNC_TPB; }
inline long long region_bytes(int64_t n) {
    return round16((long long)sub_bound(n) * (2 * sizeof(State) + 2 * sizeof(Count)) + 2ll * wg_bound(n) * sizeof(State) + 16);
}
__host__ __device__ inline Region region_of(uint8_t *ws, uint32_t sub_cap, uint32_t wg_cap) {
    Region r;
    r.entry = reinterpret_cast<State *>(ws);
    r.exit = r.entry + sub_cap;
    r.wg_exit = r.exit + sub_cap;
    r.count = reinterpret_cast<Count *>(r.wg_exit + 2 * wg_cap);
    r.prefix = r.count + sub_cap;
    r.ctl = reinterpret_cast<uint32_t *>(r.prefix + sub_cap);
    return r;
}

struct Streams {                                                   // kernel argument: where stream b's buffers are
    long long file_at[ML_JPEG_DECODE_MAX_BATCH], packed_at[ML_JPEG_DECODE_MAX_BATCH], ws_at[ML_JPEG_DECODE_MAX_BATCH];
    uint32_t file_n[ML_JPEG_DECODE_MAX_BATCH], capacity[ML_JPEG_DECODE_MAX_BATCH];
};

// The host decoder's BitReader over the raw file, every read below n.  ff: bit j set if the j-th last byte taken was an
// FF (it stands for two raw bytes), which gives the raw position of the next bit.
#ifdef __HIP_DEVICE_COMPILE__
typedef const __attribute__((address_space(3))) uint8_t *LdsBytes;   // keeps the window's loads LDS loads, not flat ones
#else
typedef const uint8_t *LdsBytes;
#endif

struct DevReader {
    const uint8_t *f;
    LdsBytes win;                                            // bytes [lo, lo + len) of the file, staged in LDS (len 0: none)
    uint32_t lo, len;
    uint32_t n, p;
    uint64_t acc;
    int avail;
    uint32_t ff;
    bool stopped;
};

__host__ __device__ inline void reader_at(DevReader &r, uint32_t byte) {
    r.p = byte;
    r.acc = 0;
    r.avail = 0;
    r.ff = 0;
    r.stopped = false;
}

__host__ __device__ inline uint32_t byte_at(const DevReader &r, uint32_t p) {   // p < n
    const uint32_t x = p - r.lo;
    return x < r.len ? r.win[x] : r.f[p];
}

__host__ __device__ inline void refill(DevReader &r) {
    while (r.avail <= 56 && !r.stopped) {
        if (r.p >= r.n) {
            r.stopped = true;
            break;
        }
        const uint32_t b = byte_at(r, r.p);
        if (b == 0xFFu) {
            if (r.p + 1 >= r.n || byte_at(r, r.p + 1) != 0) {
                r.stopped = true;
                break;
            }
            r.p += 2;
            r.ff = r.ff << 1 | 1u;
        } else {
            ++r.p;
            r.ff <<= 1;
        }
        r.acc = (r.acc << 8) | b;
        r.avail += 8;
    }
}

__host__ __device__ inline uint32_t peek(const DevReader &r, int nbits) {   // nbits 1 .. 16, zeros past the supply
    const uint64_t v = r.avail >= nbits ? r.acc >> (r.avail - nbits) : r.acc << (nbits - r.avail);
    return (uint32_t)(v & ((1u << nbits) - 1u));
}

__host__ __device__ inline int popcount8(uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// raw bit position of the next bit
__host__ __device__ inline uint32_t cursor(const DevReader &r) {
    const int nb = (r.avail + 7) >> 3;                             // bytes taken that still hold unread bits, <= 8
    const uint32_t byte = r.p - (uint32_t)nb - (uint32_t)popcount8(r.ff & ((1u << nb) - 1u));
    return byte * 8u + (uint32_t)((8 - (r.avail & 7)) & 7);
}

__host__ __device__ inline void reader_from(DevReader &r, uint32_t pos) {
    reader_at(r, pos >> 3);
    const int skip = (int)(pos & 7u);
    if (skip) {
        refill(r);
        r.avail = r.avail >= 8 ? r.avail - skip : 0;
    }
}

enum { SYM_NO_CODE = -2, SYM_TRUNCATED = -1 };

__host__ __device__ inline int dev_symbol(DevReader &r, const DevTable &t) {
    if (r.avail < 16) refill(r);
    const uint32_t e = t.fast[peek(r, 9)];
    if (e) {
        const int len = (int)(e >> 8);
        if (len > r.avail) return SYM_TRUNCATED;
        r.avail -= len;
        return (int)(e & 255u);
    }
    for (int len = 10; len <= 16; ++len) {
        const int32_t code = (int32_t)peek(r, len), top = t.maxcode[len];
        if (top >= 0 && code <= top) {
            if (len > r.avail) return SYM_TRUNCATED;
            const int32_t at = t.valoff[len] + code;
            if (at < 0 || at >= t.nvals || at >= 256) return SYM_NO_CODE;
            r.avail -= len;
            return t.vals[at];
        }
    }
    return r.avail < 16 ? SYM_TRUNCATED : SYM_NO_CODE;
}

// `size` <= 15 more bits as a signed value; false if the supply ends first
__host__ __device__ inline bool dev_extend(DevReader &r, int size, int &v) {
    v = 0;
    if (size == 0) return true;
    if (r.avail < size) refill(r);
    if (r.avail < size) return false;
    const int u = (int)peek(r, size);
    r.avail -= size;
    v = u >> (size - 1) ? u : u - (1 << size) + 1;
    return true;
}

// The reader has stopped: the RSTn number if that is what stopped it (after at most FILL_SKIP fill bytes), else -1.
__host__ __device__ inline int restart_marker(const DevReader &r, uint32_t &after) {
    uint32_t q = r.p;
    for (int i = 0; i < FILL_SKIP && q + 2 < r.n && byte_at(r, q) == 0xFF && byte_at(r, q + 1) == 0xFF; ++i) ++q;
    if (q + 2 > r.n || byte_at(r, q) != 0xFF) return -1;
    const int m = (int)byte_at(r, q + 1);
    after = q + 2;
    return m >= 0xD0 && m <= 0xD7 ? m - 0xD0 : -1;
}

__host__ __device__ inline State guess_state(const Plan &pl, const uint8_t *f, uint32_t i) {
    State s;
    uint32_t byte = pl.scan + i * SUB_BYTES;
    s.kb = 0;
    if (i > 0 && byte < pl.n && f[byte - 1] == 0xFF) {             // begins inside a pair: on a stuffed 00, or on RSTn's number
        const uint32_t b = f[byte];
        if (b == 0) ++byte;
        else if (b >= 0xD0 && b <= 0xD7) ++byte, s.kb = FRESH;
    }
    s.pos = byte * 8u;
    return s;
}

__host__ __device__ inline void raise_to(uint32_t *at, uint32_t word) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicMax(at, word);
#else
    if (word > *at) *at = word;
#endif
}
__host__ __device__ inline void flag(uint32_t *ctl, int code, uint32_t blk) {
    raise_to(ctl, (uint32_t)code << 24 | (blk < 0xFFFFFFu ? blk : 0xFFFFFFu));
}

struct Window {                                                    // a workgroup's part of the file in LDS
    LdsBytes bytes;
    uint32_t lo, len;
};

struct WriteTo {                                                   // the write pass only
    uint8_t *packed;
    uint32_t capacity;
    Count base;                                                    // words, blocks and DC predictors at entry
    uint32_t *ctl;
    State next;                                                    // the successor's entry state
    bool has_next;
};

// Thread i of a stream: its subsequence from `entry`.  Decodes every symbol that starts below its last bit.
template <bool WRITE>
__host__ __device__ inline void decode_subsequence(const Plan &pl, const uint8_t *f, const Window &win, uint32_t i, State entry, State &exit,
                                                   Count &count, const WriteTo &w) {
    count.words = count.blocks = count.reset = 0;
    count.dc0 = count.dc1 = count.dc2 = 0;
    exit = entry;
    if (entry.kb & END) return;
    const uint32_t last = pl.scan + (i + 1) * SUB_BYTES;
    const uint32_t end_bits = (last < pl.n ? last : pl.n) * 8u;
    const uint32_t fixed = (uint32_t)sizeof(PackedHeader) + 4u * (pl.nblk + 1u);
    const uint32_t room = WRITE ? (w.capacity - fixed) / 4u : 0u;  // capacity >= fixed + 4 nblk: checked by the entry point
    uint32_t *block_start = WRITE ? reinterpret_cast<uint32_t *>(w.packed + sizeof(PackedHeader)) : nullptr;
    uint32_t *entries = WRITE ? block_start + pl.nblk + 1 : nullptr;
    uint32_t blk = WRITE ? w.base.blocks : 0u, widx = WRITE ? w.base.words : 0u;
    int pred0 = WRITE ? w.base.dc0 : 0, pred1 = WRITE ? w.base.dc1 : 0, pred2 = WRITE ? w.base.dc2 : 0;
    if (WRITE && blk > pl.nblk) return;                            // past the last block: whoever got there has spoken
    DevReader r;
    r.f = f;
    r.win = win.bytes;
    r.lo = win.lo;
    r.len = win.len;
    r.n = pl.n;
    reader_from(r, entry.pos);
    uint32_t k = entry.kb & 255u, b = (entry.kb >> 8) & 255u;
    bool fresh = (entry.kb & FRESH) != 0, ended = false, done = false;
    for (int step = 0; step < SUB_BITS + 64; ++step) {             // every step consumes a bit, passes a marker or ends
        if (r.avail < 16) refill(r);
        if (cursor(r) >= end_bits) break;
        bool stop = false;                                         // the supply cannot finish the symbol
        if (k == 0 && b == 0) {                                    // between MCUs
            if (WRITE && blk >= pl.nblk) {
                done = true;
                break;
            }
            const uint32_t mcu = WRITE ? blk / pl.per_mcu : 0u;
            const bool due = WRITE && pl.restart && mcu && mcu % pl.restart == 0 && !fresh;
            if (r.stopped && r.avail < 8) {
                uint32_t after = 0;
                const int m = restart_marker(r, after);
                if (m >= 0) {
                    if (WRITE && (fresh || !due || (uint32_t)m != ((mcu / pl.restart - 1u) & 7u))) flag(w.ctl, ML_JPEG_ENTROPY_RESTART, blk);
                    reader_at(r, after);
                    fresh = true;
                    count.reset = 1;
                    count.dc0 = count.dc1 = count.dc2 = 0;
                    pred0 = pred1 = pred2 = 0;
                    continue;
                }
            }
            if (due) flag(w.ctl, ML_JPEG_ENTROPY_ASK_HOST, blk);   // the host takes the marker if its reader has reached it
        }
        const uint32_t comp = pl.mode == ML_JPEG_420 ? (b < 4u ? 0u : b - 3u) : pl.mode == ML_JPEG_444 ? b : 0u;
        const uint32_t c = comp < (uint32_t)MAX_COMPONENTS ? comp : 0u;
        bool block_ends = false;
        if (k == 0) {
            int sym = dev_symbol(r, pl.dc[c]);
            if (sym == SYM_TRUNCATED) {
                stop = true;
            } else {
                if (sym == SYM_NO_CODE) {
                    if (WRITE) flag(w.ctl, ML_JPEG_ENTROPY_BAD_CODE, blk);
                    r.avail -= r.avail < 16 ? r.avail : 16;
                    sym = 0;
                }
                if (sym > 11) {
                    if (WRITE) flag(w.ctl, ML_JPEG_ENTROPY_BAD_DC, blk);
                    sym = 0;
                }
                int diff;
                if (!dev_extend(r, sym, diff)) {
                    stop = true;
                } else {
                    if (c == 0) count.dc0 += diff, pred0 += diff;
                    else if (c == 1) count.dc1 += diff, pred1 += diff;
                    else count.dc2 += diff, pred2 += diff;
                    if (WRITE) {
                        if (blk < pl.nblk) block_start[blk] = widx;
                        const int pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
                        if (widx < room) entries[widx] = (uint32_t)(uint16_t)(int16_t)pred;
                        else flag(w.ctl, ML_JPEG_ENTROPY_CAPACITY, blk);
                        ++widx;
                        ++blk;                                     // blk: the block after the one being decoded
                    }
                    ++count.words;
                    ++count.blocks;
                    fresh = false;
                    k = 1;
                }
            }
        } else {
            const uint32_t at = WRITE ? blk - 1u : 0u;             // the block these coefficients belong to
            int sym = dev_symbol(r, pl.ac[c]);
            if (sym == SYM_TRUNCATED) {
                stop = true;
            } else {
                if (sym == SYM_NO_CODE) {
                    if (WRITE) flag(w.ctl, ML_JPEG_ENTROPY_BAD_CODE, at);
                    r.avail -= r.avail < 16 ? r.avail : 16;
                    sym = 0;
                }
                const uint32_t run = (uint32_t)sym >> 4, size = (uint32_t)sym & 15u;
                if (size == 0) {
                    if (run == 15u) {
                        k += 16;
                        if (k > 64u && WRITE) flag(w.ctl, ML_JPEG_ENTROPY_RUN, at);
                        block_ends = k >= 64u;
                    } else {
                        if (run != 0u && WRITE) flag(w.ctl, ML_JPEG_ENTROPY_BAD_AC, at);
                        block_ends = true;
                    }
                } else {
                    if (size > 10u && WRITE) flag(w.ctl, ML_JPEG_ENTROPY_BAD_AC, at);
                    k += run;
                    int v;
                    if (!dev_extend(r, (int)size, v)) {
                        stop = true;
                    } else if (k > 63u) {
                        if (WRITE) flag(w.ctl, ML_JPEG_ENTROPY_RUN, at);
                        block_ends = true;
                    } else {
                        if (WRITE) {
                            if (widx < room) entries[widx] = (uint32_t)pl.zigzag[k] << 16 | (uint32_t)(uint16_t)(int16_t)v;
                            else flag(w.ctl, ML_JPEG_ENTROPY_CAPACITY, at);
                            ++widx;
                        }
                        ++count.words;
                        ++k;
                        block_ends = k >= 64u;
                    }
                }
            }
        }
        if (stop) {                                                // the reader has stopped short of the symbol
            if (WRITE) flag(w.ctl, ML_JPEG_ENTROPY_TRUNCATED, k ? blk - 1u : blk);
            uint32_t after = 0;
            if (restart_marker(r, after) >= 0) {
                reader_at(r, after);
                fresh = true;
                count.reset = 1;
                count.dc0 = count.dc1 = count.dc2 = 0;
                pred0 = pred1 = pred2 = 0;
                k = b = 0;
                continue;
            }
            ended = true;
            break;
        }
        if (block_ends) {
            k = 0;
            b = b + 1u >= pl.per_mcu ? 0u : b + 1u;
        }
    }
    exit.pos = ended ? r.p * 8u : cursor(r);                       // (the bits left before a stop are never read again)
    exit.kb = (k & 255u) | b << 8 | (fresh ? FRESH : 0u) | (ended ? END : 0u);
    if (!WRITE) return;
    if (!done) {
        if (ended) return;                                         // flagged where it ended
        if (!w.has_next) flag(w.ctl, blk >= pl.nblk && k == 0 && b == 0 ? ML_JPEG_ENTROPY_NO_EOI : ML_JPEG_ENTROPY_TRUNCATED, blk);
        else if (!same(exit, w.next)) flag(w.ctl, ML_JPEG_ENTROPY_NOT_SYNCED, blk);
        return;
    }
    // The last block is complete.  The host passes over bytes that are no marker: EOI must be the first marker from
    // here on, which is the scan's first marker that is no RSTn (no decoder gets past that one) unless an RSTn lies between.
    const uint32_t here = cursor(r) >> 3;
    if (pl.end_marker + 2u > pl.n || f[pl.end_marker + 1u] != 0xD9 || pl.last_rst > here) flag(w.ctl, ML_JPEG_ENTROPY_NO_EOI, blk);
    block_start[pl.nblk] = widx;
    const uint32_t used = fixed + 4u * widx, bytes = (used + 15u) / 16u * 16u;
    PackedHeader *h = reinterpret_cast<PackedHeader *>(w.packed);
    h->magic = MAGIC;
    h->height = pl.height;
    h->width = pl.width;
    h->mode = pl.mode;
    h->blocks = pl.nblk;
    h->entries = widx;
    h->bytes = bytes <= w.capacity ? bytes : used;
    h->reserved = 0;
    for (int c = 0; c < MAX_COMPONENTS; ++c)
        for (int x = 0; x < 64; ++x) h->q[c][x] = pl.q[c][x];
    if (bytes <= w.capacity)
        for (uint32_t x = widx; fixed + 4u * x < bytes; ++x) entries[x] = 0u;
    w.ctl[1] = 1u;
}

// what the kernels rely on in a plan that came from device memory: the file's length, the subsequence count the
// workspace was sized for, a capacity that holds the fixed part and one word a block
__host__ __device__ inline bool plan_fits(const Plan &pl, uint32_t file_n, uint32_t capacity) {
    if (pl.magic != PLAN_MAGIC || pl.n != file_n || pl.scan > pl.n || pl.nsub != sub_cap_of(pl.n - pl.scan)) return false;
    if (pl.end_marker > pl.n || pl.last_rst > pl.n) return false;
    if (pl.per_mcu != 1u && pl.per_mcu != 3u && pl.per_mcu != 6u) return false;
    if (pl.nblk == 0u || pl.nblk > (1u << 24)) return false;
    return (unsigned long long)capacity >= sizeof(PackedHeader) + 4ull * (pl.nblk + 1u) + 4ull * pl.nblk;
}

// one stream's exclusive prefix, chunk by chunk: thread t of nt takes subsequences [t per, (t + 1) per)
__host__ __device__ inline Count chunk_sum(const Count *count, uint32_t lo, uint32_t hi) {
    Count s = {0u, 0u, 0, 0, 0, 0u};
    for (uint32_t i = lo; i < hi; ++i) s = combine(s, count[i]);
    return s;
}
__host__ __device__ inline void chunk_prefix(const Count *count, Count *prefix, uint32_t lo, uint32_t hi, Count run) {
    for (uint32_t i = lo; i < hi; ++i) {
        prefix[i] = run;
        run = combine(run, count[i]);
    }
}

// A stream that did not end with status 0: thread g clears its share of everything behind the header, so that the
// block and pixel kernels, which may run before anybody reads the status, find every block empty.
constexpr uint32_t CLEAR_BYTES = 16;
__host__ __device__ inline void clear_packed(uint8_t *packed, uint32_t capacity, uint32_t g) {
    const uint32_t words = (capacity - (uint32_t)sizeof(PackedHeader)) / 4u;
    uint32_t *w = reinterpret_cast<uint32_t *>(packed + sizeof(PackedHeader));
    for (uint32_t x = g * (CLEAR_BYTES / 4u); x < (g + 1u) * (CLEAR_BYTES / 4u) && x < words; ++x) w[x] = 0u;
}

__host__ __device__ inline void finish_stream(const uint32_t *ctl, int32_t *status) {
    const uint32_t err = ctl[0];
    status[0] = err ? (int32_t)(err >> 24) : ctl[1] ? ML_JPEG_ENTROPY_OK : ML_JPEG_ENTROPY_BLOCKS;
    status[1] = err ? (int32_t)(err & 0xFFFFFFu) : -1;
    status[2] = (int32_t)ctl[2];
    status[3] = (int32_t)ctl[3];
}

__device__ inline void load_plan(Plan &lds, const uint8_t *plans, int b) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(plans + (size_t)b * PLAN_BYTES);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&lds);
    for (uint32_t x = threadIdx.x; x < sizeof(Plan) / 4; x += blockDim.x) dst[x] = src[x];
    __syncthreads();
}

// The workgroup's subsequences and WINDOW_TAIL bytes beyond them (a thread's last symbol, a marker and its fill bytes)
// go to LDS in aligned 32-bit loads; what a thread reads outside the window it reads from memory.
constexpr uint32_t WINDOW_TAIL = 256, WINDOW_WORDS = (SYNC_TPB * SUB_BYTES + WINDOW_TAIL + 4) / 4;
__device__ inline Window stage_window(uint32_t *lds, const uint8_t *f, uint32_t first, uint32_t n) {
    const uint32_t lo = first - (uint32_t)((uintptr_t)(f + first) & 3u);   // first >= scan > 3: the headers precede it
    const uint32_t *src = reinterpret_cast<const uint32_t *>(f + lo);
    uint32_t words = 0;
    if (lo <= first && lo < n) words = min((n - lo) / 4u, WINDOW_WORDS);   // whole words inside the file only
    for (uint32_t x = threadIdx.x; x < words; x += blockDim.x) lds[x] = src[x];
    __syncthreads();
    Window w;
    w.bytes = (LdsBytes)lds;
    w.lo = lo;
    w.len = 4u * words;
    return w;
}

// Every stream's four control words, cleared in a launch of their own in front of the first sync launch: the workgroups of
// one launch run in no order, so a workgroup that clears them itself can wipe the rounds another one has already raised
// into ctl[2] (and the workspace holds whatever the call before left there).  One thread per stream.
__global__ void jpeg_entropy_clear_kernel(uint8_t *workspace, Streams st, int B) {
    const int b = (int)threadIdx.x;
    if (b >= B) return;
    const uint32_t sub_cap = sub_cap_of(st.file_n[b]), wg_cap = (sub_cap + SYNC_TPB - 1) / SYNC_TPB;
    uint32_t *ctl = region_of(workspace + st.ws_at[b], sub_cap, wg_cap).ctl;
    ctl[0] = ctl[1] = ctl[2] = ctl[3] = 0u;
}

__global__ __launch_bounds__(SYNC_TPB) void jpeg_entropy_sync_kernel(const uint8_t *files, const uint8_t *plans, uint8_t *workspace,
                                                                     Streams st, int launch) {
    __shared__ Plan pl;
    __shared__ State handed[SYNC_TPB];
    __shared__ uint32_t staged[WINDOW_WORDS];
    const int b = blockIdx.y, t = threadIdx.x;
    load_plan(pl, plans, b);
    const uint32_t nsub = pl.nsub, wg = blockIdx.x, i = wg * SYNC_TPB + t;
    if (!plan_fits(pl, st.file_n[b], st.capacity[b]) || wg * SYNC_TPB >= nsub) return;   // uniform over the workgroup
    const uint32_t sub_cap = sub_cap_of(st.file_n[b]), wg_cap = (sub_cap + SYNC_TPB - 1) / SYNC_TPB;
    const Region rg = region_of(workspace + st.ws_at[b], sub_cap, wg_cap);
    const uint8_t *f = files + st.file_at[b];
    const bool live = i < nsub;
    const WriteTo none = {};
    const Window win = stage_window(staged, f, pl.scan + wg * SYNC_TPB * SUB_BYTES, pl.n);
    State entry = {0u, END}, exit = entry;
    Count count = {0u, 0u, 0, 0, 0, 0u};
    bool decode = false;                                           // one call site: the decoder is inlined once
    if (launch == 0) {
        if (live) entry = guess_state(pl, f, i);                   // (ctl: cleared by jpeg_entropy_clear_kernel)
        decode = live;
    } else if (live) {
        entry = rg.entry[i];
        exit = rg.exit[i];
        count = rg.count[i];
        if (t == 0 && wg > 0) {
            const State got = rg.wg_exit[((launch - 1) & 1) * wg_cap + wg - 1];
            decode = !same(got, entry);
            if (decode) {
                entry = got;
                raise_to(rg.ctl + 3, (uint32_t)launch);
            }
        }
    }
    int round = 0;
    for (;; ++round) {
        if (decode) decode_subsequence<false>(pl, f, win, i, entry, exit, count, none);
        if (round == SYNC_ROUNDS) break;
        handed[t] = exit;
        __syncthreads();
        decode = live && t > 0 && !same(handed[t - 1], entry);
        if (decode) entry = handed[t - 1];
        if (!__syncthreads_or(decode)) break;
    }
    if (t == 0 && round) raise_to(rg.ctl + 2, (uint32_t)round);
    if (live) {
        rg.entry[i] = entry;
        rg.exit[i] = exit;
        rg.count[i] = count;
        if (t == SYNC_TPB - 1 || i == nsub - 1) rg.wg_exit[(launch & 1) * wg_cap + wg] = exit;
    }
}

constexpr int SCAN_TPB = 256;
__global__ __launch_bounds__(SCAN_TPB) void jpeg_entropy_scan_kernel(const uint8_t *plans, uint8_t *workspace, Streams st) {
    __shared__ Count part[SCAN_TPB];
    const int b = blockIdx.x, t = threadIdx.x;
    const Plan *pl = reinterpret_cast<const Plan *>(plans + (size_t)b * PLAN_BYTES);
    const uint32_t sub_cap = sub_cap_of(st.file_n[b]), wg_cap = (sub_cap + SYNC_TPB - 1) / SYNC_TPB;
    const uint32_t nsub = plan_fits(*pl, st.file_n[b], st.capacity[b]) ? pl->nsub : 0u;
    const Region rg = region_of(workspace + st.ws_at[b], sub_cap, wg_cap);
    const uint32_t per = (nsub + SCAN_TPB - 1) / SCAN_TPB;
    const uint32_t lo = min(nsub, (uint32_t)t * per), hi = min(nsub, lo + per);
    part[t] = chunk_sum(rg.count, lo, hi);
    __syncthreads();
    for (int d = 1; d < SCAN_TPB; d <<= 1) {                       // inclusive scan of the chunk sums, in order
        Count v = part[t];
        if (t >= d) v = combine(part[t - d], v);
        __syncthreads();
        part[t] = v;
        __syncthreads();
    }
    const Count zero = {0u, 0u, 0, 0, 0, 0u};
    chunk_prefix(rg.count, rg.prefix, lo, hi, t ? part[t - 1] : zero);
}

__global__ __launch_bounds__(SYNC_TPB) void jpeg_entropy_write_kernel(const uint8_t *files, const uint8_t *plans, uint8_t *workspace,
                                                                      uint8_t *packed, Streams st) {
    __shared__ Plan pl;
    __shared__ uint32_t staged[WINDOW_WORDS];
    const int b = blockIdx.y;
    load_plan(pl, plans, b);
    const uint32_t nsub = pl.nsub, i = blockIdx.x * SYNC_TPB + threadIdx.x;
    const uint32_t sub_cap = sub_cap_of(st.file_n[b]), wg_cap = (sub_cap + SYNC_TPB - 1) / SYNC_TPB;
    if (!plan_fits(pl, st.file_n[b], st.capacity[b]) || blockIdx.x * SYNC_TPB >= nsub) return;   // uniform over the workgroup
    const Window win = stage_window(staged, files + st.file_at[b], pl.scan + blockIdx.x * SYNC_TPB * SUB_BYTES, pl.n);
    if (i >= nsub) return;
    const Region rg = region_of(workspace + st.ws_at[b], sub_cap, wg_cap);
    WriteTo w;
    w.packed = packed + st.packed_at[b];
    w.capacity = st.capacity[b];
    w.base = rg.prefix[i];
    w.ctl = rg.ctl;
    w.has_next = i + 1 < nsub;
    w.next = w.has_next ? rg.entry[i + 1] : rg.entry[i];
    State exit;
    Count count;
    decode_subsequence<true>(pl, files + st.file_at[b], win, i, rg.entry[i], exit, count, w);
}

__global__ __launch_bounds__(SYNC_TPB) void jpeg_entropy_finish_kernel(const uint8_t *plans, uint8_t *workspace, uint8_t *packed, Streams st,
                                                                       int32_t *status) {
    const int b = blockIdx.y;
    const uint32_t g = blockIdx.x * SYNC_TPB + threadIdx.x;
    const uint32_t sub_cap = sub_cap_of(st.file_n[b]), wg_cap = (sub_cap + SYNC_TPB - 1) / SYNC_TPB;
    int32_t out[4] = {ML_JPEG_ENTROPY_BAD_PLAN, -1, 0, 0};
    if (plan_fits(*reinterpret_cast<const Plan *>(plans + (size_t)b * PLAN_BYTES), st.file_n[b], st.capacity[b]))
        finish_stream(region_of(workspace + st.ws_at[b], sub_cap, wg_cap).ctl, out);
    if (g == 0) *reinterpret_cast<int4 *>(status + 4 * b) = make_int4(out[0], out[1], out[2], out[3]);
    if (out[0] != ML_JPEG_ENTROPY_OK) clear_packed(packed + st.packed_at[b], st.capacity[b], g);
}

void device_table(const HuffTable &t, DevTable &d) {
    memcpy(d.fast, t.fast, sizeof(d.fast));
    memcpy(d.maxcode, t.maxcode, sizeof(d.maxcode));
    memcpy(d.valoff, t.valoff, sizeof(d.valoff));
    d.maxcode[0] = -1;
    d.valoff[0] = 0;
    d.nvals = t.nvals;
    memset(d.vals, 0, sizeof(d.vals));
    memcpy(d.vals, t.vals, (size_t)t.nvals);
}

int check_plan(const char *what, const void *plan, const Plan *&pl, int64_t n, int64_t capacity) {
    pl = (const Plan *)plan;
    ML_REQUIRE(capacity > 0 && capacity < (1ll << 32) && plan_fits(*pl, (uint32_t)n, (uint32_t)capacity),
               "%s: not the plan of this %lld-byte stream, or a capacity (%lld) below the header, the offsets and one word a block", what,
               (long long)n, (long long)capacity);
    return ML_OK;
}

}  // namespace

extern "C" int ml_jpeg_entropy_geometry(int32_t *geometry) {
    ML_REQUIRE(geometry, "jpeg_entropy_geometry: null pointer");
    geometry[0] = SUB_BITS;
    geometry[1] = SYNC_TPB;
    return ML_OK;
}

extern "C" int64_t ml_jpeg_entropy_plan_bytes(void) { return PLAN_BYTES; }

extern "C" int ml_jpeg_entropy_plan(const uint8_t *data, int64_t n, void *plan) {
    const char *what = "jpeg_entropy_plan";
    ML_REQUIRE(data && n > 0 && plan, "%s: null pointer or empty stream", what);
    ML_REQUIRE((((uintptr_t)plan) & 7u) == 0, "%s: plan must be 8-byte aligned", what);
    ML_REQUIRE(n < MAX_FILE, "%s: a stream of %lld bytes (below %lld)", what, (long long)n, (long long)MAX_FILE);
    Stream s;
    if (parse_stream(data, n, s, what) != PARSE_OK) return ML_E_BADARG;
    Geometry g;
    const int e = geometry(s.H, s.W, s.mode, g, what);
    if (e != ML_OK) return e;
    for (int c = 0; c < s.ncomp; ++c) {
        ML_REQUIRE(s.q_defined[s.comp[c].tq], "%s: quantisation table %d is not defined", what, s.comp[c].tq);
        ML_REQUIRE(s.dc[s.comp[c].td].defined, "%s: DC Huffman table %d is not defined", what, s.comp[c].td);
        ML_REQUIRE(s.ac[s.comp[c].ta].defined, "%s: AC Huffman table %d is not defined", what, s.comp[c].ta);
    }
    memset(plan, 0, PLAN_BYTES);
    Plan *pl = (Plan *)plan;
    pl->magic = PLAN_MAGIC;
    pl->height = s.H;
    pl->width = s.W;
    pl->mode = s.mode;
    pl->nblk = g.nblk;
    pl->per_mcu = g.per_mcu;
    pl->restart = (uint32_t)s.restart;
    pl->scan = (uint32_t)s.scan;
    pl->n = (uint32_t)n;
    pl->nsub = sub_bound(n - s.scan);
    pl->end_marker = (uint32_t)n;
    for (const uint8_t *p = data + s.scan, *end = data + n; (p = (const uint8_t *)memchr(p, 0xFF, (size_t)(end - p))) != nullptr; ++p) {
        if (p + 2 > end) break;
        if (p[1] == 0x00 || p[1] == 0xFF) continue;               // a stuffed FF, a fill byte
        if (p[1] < 0xD0 || p[1] > 0xD7) {
            pl->end_marker = (uint32_t)(p - data);
            break;
        }
        pl->last_rst = (uint32_t)(p - data) + 1u;
    }
    memcpy(pl->zigzag, ZIGZAG, 64);
    for (int c = 0; c < MAX_COMPONENTS; ++c) {
        const Component &k = s.comp[c < s.ncomp ? c : 0];
        memcpy(pl->q[c], c < s.ncomp ? s.q[k.tq] : pl->q[c], 64);
        device_table(s.dc[k.td], pl->dc[c]);
        device_table(s.ac[k.ta], pl->ac[c]);
    }
    return ML_OK;
}

namespace {
int entropy_streams(const char *what, const int64_t *file_offsets, int32_t B, Streams &st, long long &ws_total, uint32_t &max_wg) {
    ML_REQUIRE(file_offsets, "%s: null pointer", what);
    ML_REQUIRE(B > 0 && B <= ML_JPEG_DECODE_MAX_BATCH, "%s: bad dims (B %d; 1 .. %d)", what, B, ML_JPEG_DECODE_MAX_BATCH);
    memset(&st, 0, sizeof(st));
    ws_total = 0;
    max_wg = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = file_offsets[b + 1] - file_offsets[b];
        ML_REQUIRE(file_offsets[b] >= 0 && n > 0 && n < MAX_FILE, "%s: file_offsets[%d] = %lld, file_offsets[%d] = %lld", what, b,
                   (long long)file_offsets[b], b + 1, (long long)file_offsets[b + 1]);
        st.file_at[b] = file_offsets[b];
        st.file_n[b] = (uint32_t)n;
        st.ws_at[b] = ws_total;
        ws_total += region_bytes(n);
        if (wg_bound(n) > max_wg) max_wg = wg_bound(n);
    }
    return ML_OK;
}
}  // namespace

extern "C" int64_t ml_jpeg_entropy_workspace_bytes(const int64_t *file_offsets, int32_t B) {
    Streams st;
    long long total;
    uint32_t max_wg;
    const int e = entropy_streams("jpeg_entropy_workspace_bytes", file_offsets, B, st, total, max_wg);
    return e != ML_OK ? e : total;
}

extern "C" int ml_jpeg_entropy_device(const uint8_t *files, const int64_t *file_offsets, const void *plans, int32_t B, void *packed,
                                      const int64_t *packed_offsets, int32_t *status, void *workspace, void *stream) {
    const char *what = "jpeg_entropy_device";
    ML_REQUIRE(files && plans && packed && packed_offsets && status && workspace, "%s: null pointer", what);
    Streams st;
    long long total;
    uint32_t max_wg;
    const int e = entropy_streams(what, file_offsets, B, st, total, max_wg);
    if (e != ML_OK) return e;
    ML_REQUIRE(ml_aligned16(packed) && ml_aligned16(workspace) && ml_aligned16(plans) && ml_aligned16(status),
               "%s: plans, packed, status and workspace must be 16-byte aligned", what);
    for (int b = 0; b < B; ++b) {
        const int64_t cap = packed_offsets[b + 1] - packed_offsets[b];
        ML_REQUIRE(packed_offsets[b] >= 0 && packed_offsets[b] % 16 == 0 && cap >= (long long)sizeof(PackedHeader) + 8 && cap < (1ll << 32),
                   "%s: packed_offsets[%d] = %lld, packed_offsets[%d] = %lld", what, b, (long long)packed_offsets[b], b + 1,
                   (long long)packed_offsets[b + 1]);
        st.packed_at[b] = packed_offsets[b];
        st.capacity[b] = (uint32_t)cap;
    }
    uint32_t max_cap = 0;
    for (int b = 0; b < B; ++b) max_cap = st.capacity[b] > max_cap ? st.capacity[b] : max_cap;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_entropy_clear_kernel, dim3(1), dim3(ML_JPEG_DECODE_MAX_BATCH), 0, s, (uint8_t *)workspace, st, B);
    for (int launch = 0; launch < SYNC_LAUNCHES; ++launch)
        hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3(max_wg, B), dim3(SYNC_TPB), 0, s, files, (const uint8_t *)plans,
                           (uint8_t *)workspace, st, launch);
    hipLaunchKernelGGL(jpeg_entropy_scan_kernel, dim3(B), dim3(SCAN_TPB), 0, s, (const uint8_t *)plans, (uint8_t *)workspace, st);
    hipLaunchKernelGGL(jpeg_entropy_write_kernel, dim3(max_wg, B), dim3(SYNC_TPB), 0, s, files, (const uint8_t *)plans,
                       (uint8_t *)workspace, (uint8_t *)packed, st);
    hipLaunchKernelGGL(jpeg_entropy_finish_kernel, dim3((max_cap / CLEAR_BYTES + SYNC_TPB) / SYNC_TPB, B), dim3(SYNC_TPB), 0, s,
                       (const uint8_t *)plans, (uint8_t *)workspace, (uint8_t *)packed, st, status);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

// The same stages in CPU loops over one stream, every pointer in host memory.
extern "C" int ml_jpeg_entropy_reference_host(const uint8_t *file, int64_t n, const void *plan, void *packed, int64_t capacity,
                                              int32_t *status, void *workspace) {
    const char *what = "jpeg_entropy_reference_host";
    ML_REQUIRE(file && n > 0 && n < MAX_FILE && plan && packed && status && workspace, "%s: null pointer or bad length", what);
    ML_REQUIRE((((uintptr_t)status) & 3u) == 0 && (((uintptr_t)packed) & 3u) == 0 && (((uintptr_t)workspace) & 7u) == 0 && (((uintptr_t)plan) & 7u) == 0,
               "%s: plan and workspace must be 8-byte, packed 4-byte aligned", what);
    const Plan *plp;
    const int e = check_plan(what, plan, plp, n, capacity);
    if (e != ML_OK) return e;
    const Plan &pl = *plp;
    const uint32_t sub_cap = sub_bound(n), wg_cap = wg_bound(n), nsub = pl.nsub;
    const Region rg = region_of((uint8_t *)workspace, sub_cap, wg_cap);
    const WriteTo none = {};
    const Window win = {nullptr, 0u, 0u};
    rg.ctl[0] = rg.ctl[1] = rg.ctl[2] = rg.ctl[3] = 0u;
    for (int launch = 0; launch < SYNC_LAUNCHES; ++launch) {
        for (uint32_t wg = 0; wg * SYNC_TPB < nsub; ++wg) {
            const uint32_t first = wg * SYNC_TPB, live = nsub - first < (uint32_t)SYNC_TPB ? nsub - first : (uint32_t)SYNC_TPB;
            State handed[SYNC_TPB];
            if (launch == 0) {
                for (uint32_t t = 0; t < live; ++t) {
                    rg.entry[first + t] = guess_state(pl, file, first + t);
                    decode_subsequence<false>(pl, file, win, first + t, rg.entry[first + t], rg.exit[first + t], rg.count[first + t], none);
                }
            } else if (wg > 0) {
                const State got = rg.wg_exit[((launch - 1) & 1) * wg_cap + wg - 1];
                if (!same(got, rg.entry[first])) {
                    raise_to(rg.ctl + 3, (uint32_t)launch);
                    rg.entry[first] = got;
                    decode_subsequence<false>(pl, file, win, first, got, rg.exit[first], rg.count[first], none);
                }
            }
            int round = 0;
            for (; round < SYNC_ROUNDS; ++round) {
                bool any = false;
                for (uint32_t t = 0; t < live; ++t) handed[t] = rg.exit[first + t];
                for (uint32_t t = 1; t < live; ++t) {
                    if (same(handed[t - 1], rg.entry[first + t])) continue;
                    any = true;
                    rg.entry[first + t] = handed[t - 1];
                    decode_subsequence<false>(pl, file, win, first + t, handed[t - 1], rg.exit[first + t], rg.count[first + t], none);
                }
                if (!any) break;
            }
            if (round) raise_to(rg.ctl + 2, (uint32_t)round);
            rg.wg_exit[(launch & 1) * wg_cap + wg] = rg.exit[first + live - 1];
        }
    }
    const Count zero = {0u, 0u, 0, 0, 0, 0u};
    chunk_prefix(rg.count, rg.prefix, 0, nsub, zero);
    for (uint32_t i = 0; i < nsub; ++i) {
        WriteTo w;
        w.packed = (uint8_t *)packed;
        w.capacity = (uint32_t)capacity;
        w.base = rg.prefix[i];
        w.ctl = rg.ctl;
        w.has_next = i + 1 < nsub;
        w.next = w.has_next ? rg.entry[i + 1] : rg.entry[i];
        State exit;
        Count count;
        decode_subsequence<true>(pl, file, win, i, rg.entry[i], exit, count, w);
    }
    finish_stream(rg.ctl, status);
    if (status[0] != ML_JPEG_ENTROPY_OK)
        for (uint32_t g = 0; g * CLEAR_BYTES < (uint32_t)capacity; ++g) clear_packed((uint8_t *)packed, (uint32_t)capacity, g);
    return ML_OK;
}
