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
constexpr int MAX_SIDE = 16384, MAX_BATCH = 32;
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
    long long at[MAX_BATCH];                                       // byte offset of image b in the packed upload
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
    ML_REQUIRE(B > 0 && B <= MAX_BATCH, "jpeg_decode_workspace_bytes: bad dims (B %d; 1 .. %d)", B, MAX_BATCH);
    return (long long)B * (g.y_bytes + 2 * g.c_bytes);
}

namespace {
int check_call(const char *what, const void *packed, const int64_t *offsets, int32_t B, int32_t H, int32_t W, int32_t mode,
               const uint8_t *out, const void *workspace, Geometry &g, Offsets &o) {
    ML_REQUIRE(packed && offsets && out && workspace, "%s: null pointer", what);
    ML_REQUIRE(B > 0 && B <= MAX_BATCH, "%s: bad dims (B %d; 1 .. %d)", what, B, MAX_BATCH);
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
    for (int b = B; b < MAX_BATCH; ++b) o.at[b] = 0;
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
