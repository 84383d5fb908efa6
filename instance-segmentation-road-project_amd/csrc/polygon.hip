// The dataset's polygon labels rasterised straight into the batch's device tensors: the instance planes int8 [B,n,H,W]
// and the semantic maps uint8 [B,H,W,S] that the reference makes with skimage.draw.polygon, one PNG per label, and reads
// back with cv2.imread.  The contract is in include/masklab_hip.h ("Dataset polygons"); what matters here:
//
//   * skimage parity is unpinned: the even-odd crossing rule below is the contract, restated in NumPy in
//     tests/polygon_ref.py and held by exact equality, not by a run of skimage.
//   * a pixel (x, y) is inside iff an odd number of edges (j -> i) cross its row (half open in y) with
//     x < (xp[j] - xp[i]) * (y - yp[i]) / (yp[j] - yp[i]) + xp[i], float64, multiply, divide, add, FP contraction OFF.
//     The right-hand side e depends on the row and the edge only, and for an integer x, x < e is x < ceil(e): an edge
//     that crosses the row toggles the row's first ceil(e) pixels.
//   * block = (column chunk of CW pixels, ROWS rows, plane / image).  Vertices are clipped and staged through LDS VCHUNK at a
//     time (any vertex count).  Wave w owns rows w, w + 4, ...: its lanes take one edge each and, for an edge that toggles
//     the chunk's first s pixels, flip bit s - 1 of the row's CW-bit LDS bitmap (an LDS atomic; nothing is capped, and the
//     order of the flips does not matter).  The inside mask is then the suffix XOR of that bitmap: inside one 32-bit word by
//     shifts, across the 64 words of the row (one per lane) by a ballot of the words' parities.
//   * stores: the mask words go back to LDS and every lane expands the 16 bits of one ALIGNED 16-byte destination word
//     (so one wave instruction writes 1 KiB contiguously), byte by byte at a row's ragged head and tail.  W and a plane's
//     start need not be multiples of 16.  Every output byte is written exactly once, the zeros and the -1 planes included.
//   * no workspace, no atomics to global memory, no host read.  Offsets that point outside `verts` cannot make a kernel read
//     out of bounds: every range is clamped to the array it indexes.
//   * ml_polygon_reference_host runs the same edge, scan and store functions in CPU loops.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {
namespace plk {

constexpr int TPB = 256;
constexpr int WAVE = 64;
constexpr int WAVES = TPB / WAVE;
constexpr int ROWS = 8;                   // rows of one block: the vertices are staged once for all of them
constexpr int CW = 2048;                  // pixels of one column chunk: one 32-bit bitmap word per lane
constexpr int WORDS = CW / 32;
constexpr int PADW = WORDS + 3;           // a row's bitmap with one word in front and two behind: the store's 64-bit window
constexpr int VCHUNK = 256;               // vertices staged per step
constexpr int PCACHE = 512;               // polygon offsets of one image kept in LDS by the semantic kernel
constexpr int MAX_GRID_Y = 65535;
static_assert(WORDS == WAVE, "one bitmap word per lane");

struct P2 { double x, y; };
struct alignas(16) U4 { uint32_t v[4]; };

__host__ __device__ inline double clip(double v, double hi) {
    v = v < 0.0 ? 0.0 : v;
    return v > hi ? hi : v;
}

__host__ __device__ inline P2 clipped(const double *verts, long long i, int H, int W) {
    return {clip(verts[2 * i], (double)(W - 1)), clip(verts[2 * i + 1], (double)(H - 1))};
}

__host__ __device__ inline int clampi(long long v, long long lo, long long hi) { return (int)(v < lo ? lo : v > hi ? hi : v); }

// How many leading pixels of the chunk [x0, x0 + len) the edge (j -> i) toggles in row y: 0 when it does not cross the row.
__host__ __device__ inline int edge_span(const P2 vi, const P2 vj, double y, int x0, int len) {
    if (!((vi.y <= y && y < vj.y) || (vj.y <= y && y < vi.y))) return 0;
    const double e = (vj.x - vi.x) * (y - vi.y) / (vj.y - vi.y) + vi.x;
    if (!(e > (double)x0)) return 0;                       // also a NaN
    if (e >= (double)(x0 + len)) return len;
    return (int)ceil(e) - x0;
}

// bit k of the result = XOR of bits k..31 of v
__host__ __device__ inline uint32_t suffix_xor(uint32_t v) {
    v ^= v >> 1; v ^= v >> 2; v ^= v >> 4; v ^= v >> 8; v ^= v >> 16;
    return v;
}

__host__ __device__ inline int popcount32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// 16 bits -> 16 bytes of 0 / 1
__host__ __device__ inline U4 expand16(uint32_t b) {
    U4 w;
#pragma unroll
    for (int d = 0; d < 4; ++d) w.v[d] = (((b >> (4 * d)) & 15u) * 0x00204081u) & 0x01010101u;
    return w;
}

// Store bytes [q, q + 16) of a row segment of `len` bytes: one aligned 16-byte word, or its bytes inside [0, len).
__host__ __device__ inline void store16(uint8_t *seg, int q, int len, const U4 &w) {
    if (q >= 0 && q + 16 <= len) {
        *reinterpret_cast<U4 *>(seg + q) = w;
        return;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (q + k >= 0 && q + k < len) seg[q + k] = (uint8_t)(w.v[k >> 2] >> (8 * (k & 3)));
}

struct Window { int x1, y1, x2, y2; };        // inclusive, x2 / y2 already cut to W - 1 / H - 1

// Vector k of one instance row segment (`seg`: its first byte, a = seg & 15, `len` pixels from column x0 on).  m: the
// row's padded inside mask (bit c of word 1 + c / 32 = pixel x0 + c), unread when the row is not `live`.
__host__ __device__ inline void instance_vector(uint8_t *seg, const uint32_t *m, int k, int a, int len, int x0, const Window &win,
                                                bool live, bool minus_one) {
    const int q = 16 * k - a;
    if (q >= len) return;
    U4 w = {{~0u, ~0u, ~0u, ~0u}};
    if (!minus_one) {
        uint32_t b = 0;
        if (live) {
            const int pos = q + 32;
            const uint64_t two = (uint64_t)m[pos >> 5] | (uint64_t)m[(pos >> 5) + 1] << 32;
            int lo = win.x1 - (x0 + q), hi = win.x2 - (x0 + q);
            lo = lo < 0 ? 0 : lo;
            hi = hi > 15 ? 15 : hi;
            const uint32_t inwin = hi < lo ? 0u : ((2u << hi) - 1u) & ~((1u << lo) - 1u);
            b = (uint32_t)(two >> (pos & 31)) & inwin;
        }
        w = expand16(b);
    }
    store16(seg, q, len, w);
}

// Vector k of one semantic row segment: len * S bytes, byte e = pixel e / S, channel e % S.  acc: channel s's inside mask
// of this row (the except group already taken out) at acc + s * stride.
__host__ __device__ inline void semantic_vector(uint8_t *seg, const uint32_t *acc, int stride, int k, int a, int nbytes, int S) {
    const int q = 16 * k - a;
    if (q >= nbytes) return;
    const int first = q < 0 ? 0 : q;
    int px = first / S, ch = first - px * S;
    U4 w = {{0u, 0u, 0u, 0u}};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        if (q + kk < first || q + kk >= nbytes) continue;
        w.v[kk >> 2] |= ((acc[ch * stride + (px >> 5)] >> (px & 31)) & 1u) << (8 * (kk & 3));
        if (++ch == S) { ch = 0; ++px; }
    }
    store16(seg, q, nbytes, w);
}

struct Block {                                // what one block works on
    int x0, len, y0, nrows;
};

__host__ __device__ inline Block make_block(int cx, int ry, int H, int W) {
    const int x0 = cx * CW, y0 = ry * ROWS;
    return {x0, W - x0 < CW ? W - x0 : CW, y0, H - y0 < ROWS ? H - y0 : ROWS};
}

#if defined(__HIPCC__)
// One polygon (vertices [vb, ve) of verts) into the rows' bitmaps: bits[r][1 + c / 32] ^= the toggles of row y0 + r, for
// the rows rowmask names.  All threads of the block call it with the same arguments.
__device__ inline void toggle_polygon(const double *verts, long long vb, long long ve, int H, int W, const Block &bk, unsigned rowmask,
                                      P2 *sv, uint32_t (*bits)[PADW]) {
    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const long long V = ve - vb;
    for (long long c0 = 0; c0 < V; c0 += VCHUNK) {
        const int nv = V - c0 < VCHUNK ? (int)(V - c0) : VCHUNK;
        __syncthreads();                                   // the last step's readers are done with sv
        if (tid < nv) sv[tid + 1] = clipped(verts, vb + c0 + tid, H, W);
        if (tid == 0) sv[0] = clipped(verts, vb + (c0 == 0 ? V - 1 : c0 - 1), H, W);
        __syncthreads();
        for (int r = wave; r < bk.nrows; r += WAVES) {
            if (!((rowmask >> r) & 1u)) continue;
            const double y = (double)(bk.y0 + r);
            for (int e = lane; e < nv; e += WAVE) {
                const int s = edge_span(sv[e + 1], sv[e], y, bk.x0, bk.len);
                if (s) atomicXor(&bits[r][1 + ((s - 1) >> 5)], 1u << ((s - 1) & 31));
            }
        }
    }
    __syncthreads();
}

// The toggles of one row (a lane's word v) -> the lane's word of the inside mask.  The whole wave calls it.
__device__ inline uint32_t wave_suffix(uint32_t v, int lane) {
    const unsigned long long odd = __ballot(popcount32(v) & 1);
    const unsigned long long above = lane == WAVE - 1 ? 0ull : odd >> (lane + 1);
    const uint32_t s = suffix_xor(v);
    return (__popcll(above) & 1) ? ~s : s;
}

__global__ __launch_bounds__(TPB) void instance_kernel(const double *verts, long long total, const int32_t *offsets, const int32_t *windows,
                                                       int H, int W, int colchunks, int8_t *out) {
    __shared__ P2 sv[VCHUNK + 1];
    __shared__ uint32_t bits[ROWS][PADW];
    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const long long p = blockIdx.y;
    const Block bk = make_block((int)(blockIdx.x % colchunks), (int)(blockIdx.x / colchunks), H, W);
    const long long vb = clampi(offsets[p], 0, total), ve = clampi(offsets[p + 1], vb, total);
    const bool minus_one = vb == ve;
    Window win = {windows[4 * p], windows[4 * p + 1], windows[4 * p + 2], windows[4 * p + 3]};
    win.x2 = win.x2 < W - 1 ? win.x2 : W - 1;
    win.y2 = win.y2 < H - 1 ? win.y2 : H - 1;
    unsigned rowmask = 0;
    if (!minus_one && win.x1 <= bk.x0 + bk.len - 1 && win.x2 >= bk.x0)
        for (int r = 0; r < bk.nrows; ++r)
            if (bk.y0 + r >= win.y1 && bk.y0 + r <= win.y2) rowmask |= 1u << r;
    if (rowmask) {                                         // uniform over the block
        for (int i = tid; i < ROWS * PADW; i += TPB) (&bits[0][0])[i] = 0u;
        toggle_polygon(verts, vb, ve, H, W, bk, rowmask, sv, bits);
        for (int r = wave; r < bk.nrows; r += WAVES)
            if ((rowmask >> r) & 1u) bits[r][1 + lane] = wave_suffix(bits[r][1 + lane], lane);
        __syncthreads();
    }
    for (int r = wave; r < bk.nrows; r += WAVES) {
        uint8_t *seg = reinterpret_cast<uint8_t *>(out) + (p * H + bk.y0 + r) * (long long)W + bk.x0;
        const int a = (int)((uintptr_t)seg & 15u), nvec = (bk.len + a + 15) / 16;
        for (int k = lane; k < nvec; k += WAVE) instance_vector(seg, bits[r], k, a, bk.len, bk.x0, win, (rowmask >> r) & 1u, minus_one);
    }
}

__global__ __launch_bounds__(TPB) void semantic_kernel(const double *verts, long long total, const int32_t *poly_offsets, int P,
                                                       const int32_t *group_offsets, int S, int H, int W, int colchunks, uint8_t *out) {
    __shared__ P2 sv[VCHUNK + 1];
    __shared__ uint32_t bits[ROWS][PADW];
    __shared__ int32_t sgo[ML_EVAL_MAX_CLASSES + 2], spo[PCACHE + 1];
    extern __shared__ uint32_t acc[];                      // [S + 1][ROWS][WORDS]
    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const long long b = blockIdx.y;
    const Block bk = make_block((int)(blockIdx.x % colchunks), (int)(blockIdx.x / colchunks), H, W);
    const unsigned rowmask = (1u << bk.nrows) - 1u;
    for (int i = tid; i < ROWS * PADW; i += TPB) (&bits[0][0])[i] = 0u;
    for (int i = tid; i < (S + 1) * ROWS * WORDS; i += TPB) acc[i] = 0u;
    // The image's offsets once into LDS: the polygon loop below is one serial chain per block, and a global round trip per
    // offset would sit in it.  Images with more than PCACHE polygons read the later offsets from global memory.
    if (tid <= S + 1) sgo[tid] = clampi(group_offsets[b * (S + 1) + tid], 0, P);
    __syncthreads();
    const int p_first = sgo[0];
    for (int i = tid; i <= PCACHE; i += TPB)
        if ((long long)p_first + i <= P) spo[i] = poly_offsets[p_first + i];
    __syncthreads();
    auto offset_of = [&](int q) -> int {                   // poly_offsets[q], 0 <= q <= P
        const int i = q - p_first;
        return i >= 0 && i <= PCACHE ? spo[i] : poly_offsets[q];
    };
    for (int g = 0; g <= S; ++g) {
        const int pb = sgo[g], pe = sgo[g + 1] > pb ? sgo[g + 1] : pb;
        for (int poly = pb; poly < pe; ++poly) {
            const long long vb = clampi(offset_of(poly), 0, total), ve = clampi(offset_of(poly + 1), vb, total);
            if (vb == ve) continue;
            toggle_polygon(verts, vb, ve, H, W, bk, rowmask, sv, bits);
            for (int r = wave; r < bk.nrows; r += WAVES) {  // union across polygons; the bitmap is clear for the next one
                acc[(g * ROWS + r) * WORDS + lane] |= wave_suffix(bits[r][1 + lane], lane);
                bits[r][1 + lane] = 0u;
            }
        }
    }
    __syncthreads();
    for (int r = wave; r < bk.nrows; r += WAVES) {
        const uint32_t except = acc[(S * ROWS + r) * WORDS + lane];
        for (int s = 0; s < S; ++s) acc[(s * ROWS + r) * WORDS + lane] &= ~except;
    }
    __syncthreads();
    for (int r = wave; r < bk.nrows; r += WAVES) {
        uint8_t *seg = out + ((b * H + bk.y0 + r) * (long long)W + bk.x0) * S;
        const int a = (int)((uintptr_t)seg & 15u), nbytes = bk.len * S, nvec = (nbytes + a + 15) / 16;
        for (int k = lane; k < nvec; k += WAVE) semantic_vector(seg, acc + r * WORDS, ROWS * WORDS, k, a, nbytes, S);
    }
}
#endif

// ---- the same functions in CPU loops
void host_toggle(const double *verts, long long vb, long long ve, int H, int W, const Block &bk, int r, uint32_t *bits) {
    const long long V = ve - vb;
    const double y = (double)(bk.y0 + r);
    for (long long i = 0; i < V; ++i) {
        const int s = edge_span(clipped(verts, vb + i, H, W), clipped(verts, vb + (i == 0 ? V - 1 : i - 1), H, W), y, bk.x0, bk.len);
        if (s) bits[1 + ((s - 1) >> 5)] ^= 1u << ((s - 1) & 31);
    }
}

void host_suffix(uint32_t *bits) {                          // the toggles of one row -> its inside mask, in place
    int above = 0;
    for (int w = WORDS - 1; w >= 0; --w) {
        const uint32_t v = bits[1 + w], s = suffix_xor(v);
        bits[1 + w] = above ? ~s : s;
        above ^= popcount32(v) & 1;
    }
}

void host_instance(const double *verts, const int32_t *offsets, const int32_t *windows, long long planes, int H, int W, int8_t *out) {
    const int colchunks = (W + CW - 1) / CW, rowgroups = (H + ROWS - 1) / ROWS;
    for (long long p = 0; p < planes; ++p) {
        const long long vb = offsets[p], ve = offsets[p + 1];
        const bool minus_one = vb == ve;
        Window win = {windows[4 * p], windows[4 * p + 1], windows[4 * p + 2], windows[4 * p + 3]};
        win.x2 = win.x2 < W - 1 ? win.x2 : W - 1;
        win.y2 = win.y2 < H - 1 ? win.y2 : H - 1;
        for (int ry = 0; ry < rowgroups; ++ry)
            for (int cx = 0; cx < colchunks; ++cx) {
                const Block bk = make_block(cx, ry, H, W);
                for (int r = 0; r < bk.nrows; ++r) {
                    uint32_t bits[PADW] = {0};
                    const bool live = !minus_one && win.x1 <= bk.x0 + bk.len - 1 && win.x2 >= bk.x0 && bk.y0 + r >= win.y1 &&
                                      bk.y0 + r <= win.y2;
                    if (live) {
                        host_toggle(verts, vb, ve, H, W, bk, r, bits);
                        host_suffix(bits);
                    }
                    uint8_t *seg = reinterpret_cast<uint8_t *>(out) + (p * H + bk.y0 + r) * (long long)W + bk.x0;
                    const int a = (int)((uintptr_t)seg & 15u), nvec = (bk.len + a + 15) / 16;
                    for (int k = 0; k < nvec; ++k) instance_vector(seg, bits, k, a, bk.len, bk.x0, win, live, minus_one);
                }
            }
    }
}

void host_semantic(const double *verts, const int32_t *poly_offsets, const int32_t *group_offsets, int B, int S, int H, int W, uint8_t *out) {
    const int colchunks = (W + CW - 1) / CW, rowgroups = (H + ROWS - 1) / ROWS;
    for (long long b = 0; b < B; ++b)
        for (int ry = 0; ry < rowgroups; ++ry)
            for (int cx = 0; cx < colchunks; ++cx) {
                const Block bk = make_block(cx, ry, H, W);
                for (int r = 0; r < bk.nrows; ++r) {
                    uint32_t acc[(ML_EVAL_MAX_CLASSES + 1) * WORDS] = {0};
                    for (int g = 0; g <= S; ++g)
                        for (int poly = group_offsets[b * (S + 1) + g]; poly < group_offsets[b * (S + 1) + g + 1]; ++poly) {
                            if (poly_offsets[poly] == poly_offsets[poly + 1]) continue;
                            uint32_t bits[PADW] = {0};
                            host_toggle(verts, poly_offsets[poly], poly_offsets[poly + 1], H, W, bk, r, bits);
                            host_suffix(bits);
                            for (int w = 0; w < WORDS; ++w) acc[g * WORDS + w] |= bits[1 + w];
                        }
                    for (int s = 0; s < S; ++s)
                        for (int w = 0; w < WORDS; ++w) acc[s * WORDS + w] &= ~acc[S * WORDS + w];
                    uint8_t *seg = out + ((b * H + bk.y0 + r) * (long long)W + bk.x0) * S;
                    const int a = (int)((uintptr_t)seg & 15u), nbytes = bk.len * S, nvec = (nbytes + a + 15) / 16;
                    for (int k = 0; k < nvec; ++k) semantic_vector(seg, acc, WORDS, k, a, nbytes, S);
                }
            }
}

// ---- argument checks
int check_dims(const char *what, int B, int H, int W, long long total, const void *verts, const void *out, bool work) {
    ML_REQUIRE(B >= 0 && H >= 1 && W >= 1, "%s: bad dims B=%d H=%d W=%d", what, B, H, W);
    ML_REQUIRE((long long)H * W < (1ll << 31), "%s: a plane of %d x %d is too large (H*W < 2^31)", what, H, W);
    ML_REQUIRE(total >= 0 && total < (1ll << 31), "%s: %lld vertices (0 <= total < 2^31)", what, total);
    ML_REQUIRE(!work || out, "%s: null output pointer", what);
    ML_REQUIRE(!work || total == 0 || verts, "%s: null vertex pointer with %lld vertices", what, total);
    return ML_OK;
}

int check_instance(const char *what, const void *verts, long long total, const void *offsets, const void *windows, int B, int n, int H,
                   int W, const void *out) {
    ML_REQUIRE(n >= 0 && (long long)B * (n > 0 ? n : 0) < (1ll << 31) - 1, "%s: bad plane count B=%d n=%d", what, B, n);
    const bool work = B > 0 && n > 0;
    const int e = check_dims(what, B, H, W, total, verts, out, work);
    if (e != ML_OK) return e;
    ML_REQUIRE(!work || (offsets && windows), "%s: null plane_offsets or windows pointer", what);
    return ML_OK;
}

int check_semantic(const char *what, const void *verts, long long total, const void *poly_offsets, int P, const void *group_offsets, int B,
                   int S, int H, int W, const void *out) {
    ML_REQUIRE(S >= 0 && S <= ML_EVAL_MAX_CLASSES, "%s: S=%d semantic labels (0 <= S <= %d)", what, S, ML_EVAL_MAX_CLASSES);
    ML_REQUIRE(P >= 0 && P < (1 << 30) && (long long)B * (S + 1) < (1ll << 31) - 1, "%s: bad polygon or group count P=%d B=%d S=%d",
               what, P, B, S);
    const bool work = B > 0 && S > 0;
    const int e = check_dims(what, B, H, W, total, verts, out, work);
    if (e != ML_OK) return e;
    ML_REQUIRE(!work || (poly_offsets && group_offsets), "%s: null poly_offsets or group_offsets pointer", what);
    return ML_OK;
}

// offsets[0..count] in host memory: starts at >= 0, never decreases, ends at <= limit
int check_offsets(const char *what, const char *name, const int32_t *offsets, long long count, long long limit) {
    ML_REQUIRE(offsets[0] >= 0, "%s: %s[0] = %d is negative", what, name, offsets[0]);
    for (long long i = 0; i < count; ++i)
        ML_REQUIRE(offsets[i] <= offsets[i + 1], "%s: %s is not monotonic at %lld (%d > %d)", what, name, i, offsets[i], offsets[i + 1]);
    ML_REQUIRE(offsets[count] <= limit, "%s: %s ends at %d, past the %lld entries it indexes", what, name, offsets[count], limit);
    return ML_OK;
}

unsigned grid_x(int H, int W) { return (unsigned)(((W + CW - 1) / CW) * (long long)((H + ROWS - 1) / ROWS)); }

}  // namespace plk
}  // namespace

using namespace plk;

extern "C" int ml_polygon_instance_masks(const double *verts, int64_t total, const int32_t *plane_offsets, const int32_t *windows,
                                         int32_t B, int32_t n, int32_t H, int32_t W, void *out, void *stream) {
    const char *what = "polygon_instance_masks";
    const int e = check_instance(what, verts, total, plane_offsets, windows, B, n, H, W, out);
    if (e != ML_OK || B == 0 || n == 0) return e;
    const long long planes = (long long)B * n, plane = (long long)H * W;
    for (long long p0 = 0; p0 < planes; p0 += MAX_GRID_Y) {
        const long long np_ = planes - p0 < MAX_GRID_Y ? planes - p0 : MAX_GRID_Y;
        hipLaunchKernelGGL(instance_kernel, dim3(grid_x(H, W), (unsigned)np_), dim3(TPB), 0, (hipStream_t)stream, verts, (long long)total,
                           plane_offsets + p0, windows + 4 * p0, H, W, (W + CW - 1) / CW, (int8_t *)out + p0 * plane);
    }
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_polygon_semantic_maps(const double *verts, int64_t total, const int32_t *poly_offsets, int32_t P,
                                        const int32_t *group_offsets, int32_t B, int32_t S, int32_t H, int32_t W, void *out, void *stream) {
    const char *what = "polygon_semantic_maps";
    const int e = check_semantic(what, verts, total, poly_offsets, P, group_offsets, B, S, H, W, out);
    if (e != ML_OK || B == 0 || S == 0) return e;
    const size_t lds = (size_t)(S + 1) * ROWS * WORDS * sizeof(uint32_t);
    const long long image = (long long)H * W * S;
    for (long long b0 = 0; b0 < B; b0 += MAX_GRID_Y) {
        const long long nb = B - b0 < MAX_GRID_Y ? B - b0 : MAX_GRID_Y;
        hipLaunchKernelGGL(semantic_kernel, dim3(grid_x(H, W), (unsigned)nb), dim3(TPB), lds, (hipStream_t)stream, verts, (long long)total,
                           poly_offsets, P, group_offsets + b0 * (S + 1), S, H, W, (W + CW - 1) / CW, (uint8_t *)out + b0 * image);
    }
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_polygon_reference_host(int32_t kind, const double *verts, int64_t total, const int32_t *offsets, int32_t P,
                                         const int32_t *group_offsets, const int32_t *windows, int32_t B, int32_t n_or_S, int32_t H,
                                         int32_t W, void *out) {
    const char *what = "polygon_reference_host";
    ML_REQUIRE(kind == ML_POLYGON_INSTANCE || kind == ML_POLYGON_SEMANTIC, "%s: kind %d", what, kind);
    if (kind == ML_POLYGON_INSTANCE) {
        int e = check_instance(what, verts, total, offsets, windows, B, n_or_S, H, W, out);
        if (e != ML_OK || B == 0 || n_or_S == 0) return e;
        e = check_offsets(what, "plane_offsets", offsets, (long long)B * n_or_S, total);
        if (e != ML_OK) return e;
        host_instance(verts, offsets, windows, (long long)B * n_or_S, H, W, (int8_t *)out);
        return ML_OK;
    }
    int e = check_semantic(what, verts, total, offsets, P, group_offsets, B, n_or_S, H, W, out);
    if (e != ML_OK || B == 0 || n_or_S == 0) return e;
    e = check_offsets(what, "group_offsets", group_offsets, (long long)B * (n_or_S + 1), P);
    if (e == ML_OK) e = check_offsets(what, "poly_offsets", offsets, P, total);
    if (e != ML_OK) return e;
    host_semantic(verts, offsets, group_offsets, B, n_or_S, H, W, (uint8_t *)out);
    return ML_OK;
}
