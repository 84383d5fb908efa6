// The serving model's 'visualize' output (reference road_project/setup/serving.py:30-40, engine/layers/misc.py:404-503):
//   v1 = DrawBoxes(images, det)                          1-pixel white outlines (tf.image.draw_bounding_boxes)
//   v2 = DrawInstance(colors_i, alpha_i)(v1, det, cpm)   per class: sum of the pasted masks of its rows > 0.5, blended
//   v3 = DrawSegmentation(colors_s, alpha_s)(v2, seg)    sum_k colour_k * map_k, blended
// with blend(v, S, alpha) = uint8(trunc(clip(v + S * alpha, 0, 255))), fp32, no fused multiply-add.
// The layer kernels run the literal chain (cpm = CropAndPadMask's [B,n,H,W] fp32 canvases); serving_visualize_kernel
// computes v3 from (images, det, instance masks, seg) in one pass: every pasted value is recomputed with
// CropAndPadMask's arithmetic (paste.h) only inside its box, so the [B,n,H,W] canvases are never built and the result
// is the same bytes.
#include "common.h"
#include "paste.h"
#include "ranges.h"
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int KMAX = ML_DRAW_MAX_CLASSES;

// colours of one Draw* layer, [K][3] fp32, and its alpha.  Indexed with compile-time k only (unrolled loops guarded by
// k < K): a run-time index into a by-value kernel argument would move it to scratch.
struct Palette {
    float col[KMAX][3];
    float alpha;
    int K;
};

__device__ __forceinline__ unsigned blend_u8(float v, float S, float alpha) {
    return (unsigned)(int)fminf(fmaxf(v + S * alpha, 0.f), 255.f);        // tf.clip_by_value, then tf.cast truncates
}

// ------------------------------------------------------------------ DrawBoxes outline (TF draw_bounding_boxes rule)
// box = max(det[:4], 0); corners normalised by H / W with correctly rounded fp32 division; line rows / columns
// trunc(corner * (H-1 | W-1)) in 64 bits.  `top` / `bot` / `left` / `right` = -1 when that line is not drawn.
struct Outline {
    int top, bot, left, right;
    int c_lo, c_hi, r_lo, r_hi;      // columns of the horizontal lines, rows of the vertical ones (clamped)
};
__device__ __forceinline__ bool outline_of(const int32_t *d, int H, int W, Outline &o) {
    const float cx = (float)max(d[0], 0), cy = (float)max(d[1], 0), w = (float)max(d[2], 0), h = (float)max(d[3], 0);
    const float fH = (float)H, fW = (float)W;
    const float xmin = (cx - w / 2.f) / fW, xmax = (cx + w / 2.f) / fW;
    const float ymin = (cy - h / 2.f) / fH, ymax = (cy + h / 2.f) / fH;
    const long long r0 = (long long)(ymin * (float)(H - 1)), r1 = (long long)(ymax * (float)(H - 1));
    const long long c0 = (long long)(xmin * (float)(W - 1)), c1 = (long long)(xmax * (float)(W - 1));
    if (r0 > r1 || c0 > c1 || r0 >= H || r1 < 0 || c0 >= W || c1 < 0) return false;
    o.top = r0 >= 0 ? (int)r0 : -1;
    o.bot = r1 < H ? (int)r1 : -1;
    o.left = c0 >= 0 ? (int)c0 : -1;
    o.right = c1 < W ? (int)c1 : -1;
    o.c_lo = (int)max(c0, 0ll);
    o.c_hi = (int)min(c1, (long long)W - 1);
    o.r_lo = (int)max(r0, 0ll);
    o.r_hi = (int)min(r1, (long long)H - 1);
    return true;
}
__device__ __forceinline__ bool on_outline(const Outline &o, int y, int x) {
    return (x >= o.c_lo && x <= o.c_hi && (y == o.top || y == o.bot)) ||
           (y >= o.r_lo && y <= o.r_hi && (x == o.left || x == o.right));
}

// one block per (row, image): the four lines of one box.  Colliding writes all store 255.
__global__ void __launch_bounds__(TPB) draw_outlines_kernel(const int32_t *__restrict__ det, uint8_t *__restrict__ out, int n,
                                                            int H, int W) {
    const int i = blockIdx.x, b = blockIdx.y;
    Outline o;
    if (!outline_of(det + ((long long)b * n + i) * 6, H, W, o)) return;
    uint8_t *img = out + (long long)b * H * W * 3;
    auto paint = [&](int y, int x) {
        uint8_t *p = img + ((long long)y * W + x) * 3;
        p[0] = 255; p[1] = 255; p[2] = 255;
    };
    for (int x = o.c_lo + (int)threadIdx.x; x <= o.c_hi; x += TPB) {
        if (o.top >= 0) paint(o.top, x);
        if (o.bot >= 0) paint(o.bot, x);
    }
    for (int y = o.r_lo + (int)threadIdx.x; y <= o.r_hi; y += TPB) {
        if (o.left >= 0) paint(y, o.left);
        if (o.right >= 0) paint(y, o.right);
    }
}

// ------------------------------------------------------------------ DrawInstance from fp32 canvases, one thread per pixel
// per class: the canvases of its rows summed in row order from 0.0f; mask = sum > 0.5; then DrawSegmentation's blend
__global__ void __launch_bounds__(TPB) draw_instance_kernel(const uint8_t *img, const int32_t *__restrict__ det,
                                                            const float *__restrict__ cpm, uint8_t *out, Palette pal, int n,
                                                            long long HW, long long total) {
    const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
    if (p >= total) return;
    const long long b = p / HW, yx = p - b * HW;
    float acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.f;
    for (int i = 0; i < n; ++i) {
        const int cls = det[(b * n + i) * 6 + 4];
        if (cls < 0 || cls >= pal.K) continue;                       // never drawn (padding: class -1)
        const float v = cpm[(b * n + i) * HW + yx];
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k == cls) acc[k] += v;
    }
    float S[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < pal.K) {
            const float m = acc[k] > 0.5f ? 1.f : 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) S[c] += pal.col[k][c] * m;
        }
    unsigned v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = blend_u8((float)img[p * 3 + c], S[c], pal.alpha);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = (uint8_t)v[c];
}

// ------------------------------------------------------------------ DrawSegmentation from int32 or fp32 maps [B,H,W,K]
template <bool F32>
__global__ void __launch_bounds__(TPB) draw_segmentation_kernel(const uint8_t *img, const void *__restrict__ maps_, uint8_t *out,
                                                                Palette pal, long long total) {
    const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
    if (p >= total) return;
    float S[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < pal.K) {
            const long long e = p * pal.K + k;
            const float m = F32 ? reinterpret_cast<const float *>(maps_)[e] : (float)reinterpret_cast<const int32_t *>(maps_)[e];
#pragma unroll
            for (int c = 0; c < 3; ++c) S[c] += pal.col[k][c] * m;
        }
    unsigned v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = blend_u8((float)img[p * 3 + c], S[c], pal.alpha);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = (uint8_t)v[c];
}

// ------------------------------------------------------------------ the fused render
// One block per VIS_TY x VIS_TX tile of one image; a thread owns 4 consecutive pixels of one row.  KS > 0: the vector
// path (W % 4 == 0, aligned buffers): 12 B of frame and output and 16 * KS B of seg per lane; KS == 0: any W, scalar
// accesses, run-time K.  The frame and seg loads are issued before the staging so their latency overlaps it.
// The image's rows are staged VIS_CH at a time: each row's paste box and outline; an ordered compaction keeps, in row
// order, the rows of a drawn class whose paste box meets the tile and the outlines that meet it.  Per pixel the class sums
// run over the kept rows in row order across the chunks -- a row that misses the pixel adds exactly 0.0f in the literal
// chain and is skipped here -- so the bytes equal DrawBoxes -> CropAndPadMask -> DrawInstance -> DrawSegmentation.
constexpr int VIS_TX = 128, VIS_TY = 8, VIS_CH = 256;

template <int KS>
__global__ void __launch_bounds__(TPB) serving_visualize_kernel(const uint8_t *img, const int32_t *__restrict__ det,
                                                                const int32_t *__restrict__ ins,
                                                                const int32_t *__restrict__ seg,
                                                                const int32_t *__restrict__ thr_ws, uint8_t *out,
                                                                Palette pi, Palette ps, int ks_rt, int n, int mh, int mw,
                                                                int H, int W) {
    constexpr bool VEC = KS > 0;
    __shared__ PasteBox s_box[VIS_CH];
    __shared__ int s_row[VIS_CH], s_cls[VIS_CH];
    __shared__ Outline s_out[VIS_CH];
    __shared__ int s_tot[2][TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * VIS_TX, ty0 = blockIdx.y * VIS_TY;
    const int tx1 = min(tx0 + VIS_TX, W), ty1 = min(ty0 + VIS_TY, H);
    const int y = ty0 + tid / (VIS_TX / 4), x0 = tx0 + (tid % (VIS_TX / 4)) * 4;
    const bool live = y < ty1 && x0 < tx1;
    const long long p0 = ((long long)b * H + y) * W + x0;        // first pixel of this thread

    // ---- frame and seg of the 4 pixels
    float pix[4][3];                                        // scalar path
    unsigned w3[3] = {0u, 0u, 0u};                          // vector path: the 12 bytes as loaded
    constexpr int KV = VEC ? KS : 1;
    int sv[4][KV];
    if (VEC) {
        int4 s4[KV];
        if (live) {
            const unsigned *iw = reinterpret_cast<const unsigned *>(img) + p0 / 4 * 3;
#pragma unroll
            for (int j = 0; j < 3; ++j) w3[j] = iw[j];
            const int4 *sw = reinterpret_cast<const int4 *>(seg) + p0 / 4 * KV;
#pragma unroll
            for (int j = 0; j < KV; ++j) s4[j] = sw[j];
        } else {
#pragma unroll
            for (int j = 0; j < KV; ++j) s4[j] = make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4 * KV; ++e) {
            const int4 v = s4[e / 4];
            sv[e / KV][e % KV] = (e % 4 == 0) ? v.x : (e % 4 == 1) ? v.y : (e % 4 == 2) ? v.z : v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool ok = live && x0 + q < W;
#pragma unroll
            for (int c = 0; c < 3; ++c) pix[q][c] = ok ? (float)img[(p0 + q) * 3 + c] : 0.f;
        }
    }

    // ---- instance class sums (rows in row order) and outline hits, the image's rows staged VIS_CH at a time
    const int thr = *thr_ws;
    float acc[4][KMAX];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < KMAX; ++k) acc[q][k] = 0.f;
    bool hit[4] = {false, false, false, false};
    const int32_t *dets = det + (long long)b * n * 6;
    for (int r0 = 0; r0 < n; r0 += VIS_CH) {
        const int r = r0 + tid;
        bool keep_p = false, keep_o = false;
        PasteBox pb = {0, 0, 0, 0, 0.f, 0.f};
        Outline ol = {-1, -1, -1, -1, 0, -1, 0, -1};
        int cls = -1;
        if (r < n) {
            const int32_t *d = dets + (long long)r * 6;
            cls = d[4];
            if (cls >= 0 && cls < pi.K) {
                pb = paste_box(d, thr, mh, mw, H, W);
                keep_p = pb.ymin < ty1 && pb.ymax > ty0 && pb.xmin < tx1 && pb.xmax > tx0;
            }
            if (outline_of(d, H, W, ol))             // a horizontal or a vertical line crosses the tile
                keep_o = (((ol.top >= ty0 && ol.top < ty1) || (ol.bot >= ty0 && ol.bot < ty1)) && ol.c_lo < tx1 && ol.c_hi >= tx0) ||
                         (((ol.left >= tx0 && ol.left < tx1) || (ol.right >= tx0 && ol.right < tx1)) && ol.r_lo < ty1 && ol.r_hi >= ty0);
        }
        const unsigned long long mp = __ballot(keep_p), mo = __ballot(keep_o);
        if (lane == 0) { s_tot[0][wave] = __popcll(mp); s_tot[1][wave] = __popcll(mo); }
        __syncthreads();
        int bp = 0, bo = 0, np = 0, no = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) {
            if (w < wave) { bp += s_tot[0][w]; bo += s_tot[1][w]; }
            np += s_tot[0][w];
            no += s_tot[1][w];
        }
        const unsigned long long below = (1ull << lane) - 1;
        if (keep_p) {
            const int at = bp + __popcll(mp & below);
            s_box[at] = pb; s_row[at] = r; s_cls[at] = cls;
        }
        if (keep_o) s_out[bo + __popcll(mo & below)] = ol;
        __syncthreads();
        if (live) {
            for (int j = 0; j < no; ++j) {
                const Outline o = s_out[j];
#pragma unroll
                for (int q = 0; q < 4; ++q) hit[q] = hit[q] || on_outline(o, y, x0 + q);
            }
            for (int j = 0; j < np; ++j) {
                const int c = __builtin_amdgcn_readfirstlane(s_cls[j]);
                const PasteBox bx = s_box[j];
                if (y < bx.ymin || y >= bx.ymax || x0 + 3 < bx.xmin || x0 >= bx.xmax) continue;   // adds 0.0f x 4
                const int32_t *m = ins + ((long long)b * n + s_row[j]) * mh * mw;
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = paste_value(bx, m, mh, mw, y, x0 + q);
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k == c)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q][k] += v[q];
            }
        }
        __syncthreads();                                    // the next chunk overwrites the staged rows
    }
    if (!live) return;

    // ---- per pixel: outline, instance blend (uint8), semantic blend, store
    unsigned o8[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float Si[3] = {0.f, 0.f, 0.f}, Ss[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < pi.K) {
                const float mk = acc[q][k] > 0.5f ? 1.f : 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) Si[c] += pi.col[k][c] * mk;
            }
        const int ks = VEC ? KS : ks_rt;
#pragma unroll
        for (int k = 0; k < (VEC ? KS : KMAX); ++k)
            if (k < ks) {
                float mk;
                if (VEC) mk = (float)sv[q][VEC ? k : 0];
                else mk = (live && x0 + q < W) ? (float)seg[(p0 + q) * ks + k] : 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) Ss[c] += ps.col[k][c] * mk;
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int e = 3 * q + c;
            const float v0 = VEC ? (float)((w3[e / 4] >> (8 * (e % 4))) & 255u) : pix[q][c];
            const float v1 = hit[q] ? 255.f : v0;
            const unsigned v2 = blend_u8(v1, Si[c], pi.alpha);
            o8[q][c] = blend_u8((float)v2, Ss[c], ps.alpha);
        }
    }
    if (VEC) {
#pragma unroll
        for (int j = 0; j < 3; ++j) w3[j] = 0u;
#pragma unroll
        for (int e = 0; e < 12; ++e) w3[e / 4] |= o8[e / 3][e % 3] << (8 * (e % 4));
        unsigned *ow = reinterpret_cast<unsigned *>(out) + p0 / 4 * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) ow[j] = w3[j];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x0 + q < W)
#pragma unroll
                for (int c = 0; c < 3; ++c) out[(p0 + q) * 3 + c] = (uint8_t)o8[q][c];
    }
}

typedef void (*VisKernel)(const uint8_t *, const int32_t *, const int32_t *, const int32_t *, const int32_t *, uint8_t *,
                          Palette, Palette, int, int, int, int, int, int);
template <int... K>
struct VisTable {
    static constexpr VisKernel fns[] = {serving_visualize_kernel<K>...};
};
template <int... K>
constexpr VisKernel VisTable<K...>::fns[];
using VisKernels = VisTable<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>;

inline unsigned grid_for(long long n) { return (unsigned)((n + TPB - 1) / TPB); }

int make_palette(const float *colors, int32_t K, float alpha, Palette &p, const char *what) {
    ML_REQUIRE(colors, "%s: null colour table", what);
    ML_REQUIRE(K >= 1 && K <= KMAX, "%s: %d colours, 1 <= K <= %d", what, K, KMAX);
    for (int k = 0; k < KMAX; ++k)
        for (int c = 0; c < 3; ++c) p.col[k][c] = k < K ? colors[k * 3 + c] : 0.f;
    p.alpha = alpha;
    p.K = K;
    return ML_OK;
}

}  // namespace

extern "C" int ml_draw_boxes_u8(const uint8_t *images, const int32_t *det, uint8_t *out, int32_t B, int32_t n, int32_t H,
                                int32_t W, void *stream) {
    ML_REQUIRE(images && det && out, "draw_boxes: null pointer");
    ML_REQUIRE(B > 0 && B < 65536 && n >= 0 && H > 0 && W > 0, "draw_boxes: bad dims");
    const long long bytes = (long long)B * H * W * 3;
    ML_REQUIRE(ml_add_or_disjoint(out, images, bytes), "draw_boxes: out overlaps images (only out == images is allowed)");
    ML_REQUIRE(!ml_ranges_overlap(out, bytes, det, (long long)B * n * 24), "draw_boxes: out overlaps det");
    hipStream_t s = (hipStream_t)stream;
    if (out != images)
        ML_REQUIRE(hipMemcpyAsync(out, images, (size_t)bytes, hipMemcpyDeviceToDevice, s) == hipSuccess, "draw_boxes: copy failed");
    if (n > 0) hipLaunchKernelGGL(draw_outlines_kernel, dim3(n, B), dim3(TPB), 0, s, det, out, n, H, W);
    ML_CHECK_LAUNCH("draw_boxes");
    return ML_OK;
}

extern "C" int ml_draw_instance_u8(const uint8_t *images, const int32_t *det, const float *masks, uint8_t *out,
                                   const float *colors, int32_t K, float alpha, int32_t B, int32_t n, int32_t H, int32_t W,
                                   void *stream) {
    ML_REQUIRE(images && det && masks && out, "draw_instance: null pointer");
    ML_REQUIRE(B > 0 && n >= 0 && H > 0 && W > 0, "draw_instance: bad dims");
    Palette pal;
    const int e = make_palette(colors, K, alpha, pal, "draw_instance");
    if (e != ML_OK) return e;
    const long long px = (long long)B * H * W;
    ML_REQUIRE(ml_add_or_disjoint(out, images, px * 3), "draw_instance: out overlaps images (only out == images is allowed)");
    ML_REQUIRE(!ml_any_overlap({{out, px * 3}}, {{det, (long long)B * n * 24}, {masks, px * n * 4}}),
               "draw_instance: out overlaps det or masks");
    ML_REQUIRE(grid_for(px) < (1u << 31), "draw_instance: frame too large for one launch");
    hipLaunchKernelGGL(draw_instance_kernel, dim3(grid_for(px)), dim3(TPB), 0, (hipStream_t)stream, images, det, masks, out,
                       pal, n, (long long)H * W, px);
    ML_CHECK_LAUNCH("draw_instance");
    return ML_OK;
}

extern "C" int ml_draw_segmentation_u8(const uint8_t *images, const void *maps, int32_t maps_are_f32, uint8_t *out,
                                       const float *colors, int32_t K, float alpha, int32_t B, int32_t H, int32_t W,
                                       void *stream) {
    ML_REQUIRE(images && maps && out, "draw_segmentation: null pointer");
    ML_REQUIRE(B > 0 && H > 0 && W > 0, "draw_segmentation: bad dims");
    Palette pal;
    const int e = make_palette(colors, K, alpha, pal, "draw_segmentation");
    if (e != ML_OK) return e;
    const long long px = (long long)B * H * W;
    ML_REQUIRE(ml_add_or_disjoint(out, images, px * 3), "draw_segmentation: out overlaps images (only out == images is allowed)");
    ML_REQUIRE(!ml_ranges_overlap(out, px * 3, maps, px * K * 4), "draw_segmentation: out overlaps maps");
    ML_REQUIRE(grid_for(px) < (1u << 31), "draw_segmentation: frame too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    if (maps_are_f32)
        hipLaunchKernelGGL(draw_segmentation_kernel<true>, dim3(grid_for(px)), dim3(TPB), 0, s, images, maps, out, pal, px);
    else
        hipLaunchKernelGGL(draw_segmentation_kernel<false>, dim3(grid_for(px)), dim3(TPB), 0, s, images, maps, out, pal, px);
    ML_CHECK_LAUNCH("draw_segmentation");
    return ML_OK;
}

extern "C" int ml_serving_visualize_u8(const uint8_t *images, const int32_t *det, const int32_t *ins, const int32_t *seg,
                                       uint8_t *out, int32_t *threshold_ws, const float *instance_colors, int32_t Ki,
                                       float instance_alpha, const float *semantic_colors, int32_t Ks, float semantic_alpha,
                                       int32_t B, int32_t n, int32_t mh, int32_t mw, int32_t H, int32_t W, void *stream) {
    ML_REQUIRE(images && det && ins && seg && out && threshold_ws, "serving_visualize: null pointer");
    ML_REQUIRE(B > 0 && B < 65536 && n >= 0 && mh > 0 && mw > 0 && H > 0 && W > 0 && (H + VIS_TY - 1) / VIS_TY < 65536,
               "serving_visualize: bad dims");
    Palette pi, ps;
    int e = make_palette(instance_colors, Ki, instance_alpha, pi, "serving_visualize");
    if (e != ML_OK) return e;
    e = make_palette(semantic_colors, Ks, semantic_alpha, ps, "serving_visualize");
    if (e != ML_OK) return e;
    const long long px = (long long)B * H * W;
    ML_REQUIRE(ml_add_or_disjoint(out, images, px * 3), "serving_visualize: out overlaps images (only out == images is allowed)");
    const ml_range r_det = {det, (long long)B * n * 24}, r_ins = {ins, (long long)B * n * mh * mw * 4}, r_seg = {seg, px * Ks * 4};
    ML_REQUIRE(!ml_any_overlap({{out, px * 3}}, {r_det, r_ins, r_seg, {threshold_ws, 4}}),
               "serving_visualize: out overlaps an input or the threshold workspace");
    ML_REQUIRE(!ml_any_overlap({{threshold_ws, 4}}, {{images, px * 3}, r_det, r_ins, r_seg}),
               "serving_visualize: threshold_ws overlaps an input");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(conf_threshold_kernel, dim3(1), dim3(256), 0, s, det, B * n, threshold_ws);
    const bool vec = W % 4 == 0 && ((uintptr_t)images & 3) == 0 && ((uintptr_t)out & 3) == 0 && ml_aligned16(seg);
    const dim3 grid((W + VIS_TX - 1) / VIS_TX, (H + VIS_TY - 1) / VIS_TY, B);
    hipLaunchKernelGGL(VisKernels::fns[vec ? Ks : 0], grid, dim3(TPB), 0, s, images, det, ins, seg, (const int32_t *)threshold_ws,
                       out, pi, ps, (int)Ks, n, mh, mw, H, W);
    ML_CHECK_LAUNCH("serving_visualize");
    return ML_OK;
}
