// Backward of the depthwise 3x3 convolution (pointwise.hip: dwconv3x3_kernel), fp32: the weight and bias gradient and the
// data gradient.  For y = dwconv(x, w) (+ b), kernel [3,3,C,1] held as pack_depthwise's [9][C], stride s in {1, 2},
// dilation d, leading pads (pad_t, pad_l), dy at the PRE-activation:
//
//   dw[kh,kw,c]   = sum over (b,oy,ox) of x[b, oy*s + kh*d - pad_t, ox*s + kw*d - pad_l, c] * dy[b,oy,ox,c]   (0 outside the image)
//   db[c]         = sum over (b,oy,ox) of dy[b,oy,ox,c]
//   dx[b,iy,ix,c] = sum over the taps (kh,kw) for which ty = iy + pad_t - kh*d and tx = ix + pad_l - kw*d are multiples of s
//                   with (ty/s, tx/s) inside [0,Ho) x [0,Wo), of w[kh,kw,c] * dy[b, ty/s, tx/s, c]
//
// Weight gradient.  Lanes run along channels, 16 bytes each: a block of 256 threads is PG pixel rows x CL channel lanes
// (CL = the channel quads C / 4 rounded up to a power of two, at most 64; PG = 256 / CL), and covers one SLICE of the
// pixel axis (b, oy, ox ascending) for one tile of CL channel quads.  A thread keeps the nine tap sums and the dy sum of
// its four channels in registers; per pixel it reads dy once and the nine shifted x pixels, a tap that leaves the image is
// predicated away (never loaded, never added).  x is NOT staged in LDS: at the dilations of the ASPP (6, 12, 18 on a 32 x 32
// map) the nine taps of a pixel lie up to 36 rows apart, so the pixels that share an x read belong to other slices -- other
// blocks, mostly other compute units -- and an LDS image would need the whole map as its halo; the re-reads are served
// by L2 and the infinity cache.  The PG rows of a block are added by a halving tree in LDS (a fixed
// order), and the block writes its fp32 partial [10][C] (nine taps, then the dy sums) to the workspace.
//
// No float atomics.  The slices are ceil(P / 64) pixels rounded up to a multiple of 16, at least DW_SLICE_MIN = 64 and at
// most DW_SLICE_MAX = 1024: a function of the problem's pixel count alone, never of the launch, the other problems or the
// device.  The finish kernel adds an element's partials in ascending slice order in fp64, rounds once, adds `add` with one
// fp32 addition and writes dkernel [3,3,C,1] (the Keras layout; the same memory order as [9][C]) and dbias.  Every element
// of a partial that the finish kernel reads is written by its block; a tap that only meets padding sums nothing: exact 0.
//
// Data gradient.  A gather: one thread per (input pixel, channel quad) walks the nine taps in (kh, kw) order; stride 2 is
// a divisibility test.  out = add + gradient with one fp32 addition; out may be add itself (a thread reads its own element
// before it writes it).
#include "slice_sum.h"

namespace {

constexpr int DW_TPB = 256;
constexpr int DW_ROWS = 10;            // rows of a partial: nine taps, then the dy sums
constexpr int DW_ROUND = 16;           // slice lengths are multiples of this
constexpr int DW_SLICE_MIN = 64;
constexpr int DW_SLICE_MAX = 1024;

struct DwProblem {
    const float *x, *dy, *wgt;
    float *part;                       // [slices][DW_ROWS][C]
    const float *add_k, *add_b, *add_x;
    float *dk, *db, *dx;
    int H, W, Ho, Wo, HoWo, P;         // P = B*Ho*Wo
    int C, CQ, in_cs, in_co, dy_cs, dy_co;
    int stride, dil, pad_t, pad_l;
    int slices, sp, cl_shift, ctiles;  // CL = 1 << cl_shift channel lanes, ctiles tiles of CL channel quads
    int first_block, first_fblock;
    long long threads;                 // of the data gradient: B*H*W*CQ
};
struct DwArgs {
    DwProblem p[ML_DWCONV_GRAD_MAX_PROBLEMS];
    int n;
};

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }

__global__ void __launch_bounds__(DW_TPB) dw_wgrad_partial_kernel(const DwArgs A) {
    __shared__ f32x4 sm[DW_ROWS][DW_TPB];
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.p[pi + 1].first_block) ++pi;
    const DwProblem &p = A.p[pi];
    const int id = blockIdx.x - p.first_block;
    const int ct = id % p.ctiles, slice = id / p.ctiles;
    const int tid = threadIdx.x;
    const int CL = 1 << p.cl_shift, PG = DW_TPB >> p.cl_shift;
    const int cl = tid & (CL - 1), prow = tid >> p.cl_shift;
    const int cq = ct * CL + cl;
    const bool active = cq < p.CQ;
    const int c = cq * 4;
    const int H = p.H, W = p.W, Wo = p.Wo, HoWo = p.HoWo, stride = p.stride, dil = p.dil;
    const int q_begin = slice * p.sp, q_end = min(q_begin + p.sp, p.P);
    const float *xc = p.x + p.in_co + c, *dyc = p.dy + p.dy_co + c;

    f32x4 acc[9], bacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (active) {
        for (int q = q_begin + prow; q < q_end; q += PG) {
            const int b = q / HoWo, rem = q - b * HoWo;
            const int oy = rem / Wo, ox = rem - oy * Wo;
            const int iy0 = oy * stride - p.pad_t, ix0 = ox * stride - p.pad_l;
            const f32x4 g = ld4(dyc + (long long)q * p.dy_cs);
            bool ok[9];
            f32x4 xv[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = iy0 + (t / 3) * dil, ix = ix0 + (t % 3) * dil;
                ok[t] = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                xv[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (ok[t]) xv[t] = ld4(xc + (((long long)b * H + iy) * W + ix) * p.in_cs);
            }
            bacc += g;
#pragma unroll
            for (int t = 0; t < 9; ++t)
                if (ok[t]) acc[t] += xv[t] * g;
        }
    }
    // the PG pixel rows of the block, added by halves: row r takes row r + s for s = PG / 2, PG / 4, ..., 1
#pragma unroll
    for (int t = 0; t < 9; ++t) sm[t][tid] = acc[t];
    sm[9][tid] = bacc;
    __syncthreads();
    for (int s = PG >> 1; s >= 1; s >>= 1) {
        if (prow < s) {
#pragma unroll
            for (int t = 0; t < DW_ROWS; ++t) sm[t][tid] += sm[t][tid + (s << p.cl_shift)];
        }
        __syncthreads();
    }
    if (prow == 0 && active) {
        float *part = p.part + (long long)slice * DW_ROWS * p.C + c;
        const int rows = p.db ? DW_ROWS : 9;
        for (int t = 0; t < rows; ++t) *reinterpret_cast<f32x4 *>(part + (long long)t * p.C) = sm[t][tid];
    }
}

// element i of a problem: i < 9 C -> dkernel[i] (tap-major: [3,3,C,1]), else dbias[i - 9 C]
__global__ void __launch_bounds__(DW_TPB) dw_wgrad_finish_kernel(const DwArgs A) {
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.p[pi + 1].first_fblock) ++pi;
    const DwProblem &p = A.p[pi];
    const int i = (blockIdx.x - p.first_fblock) * DW_TPB + threadIdx.x;
    const int nk = 9 * p.C;
    if (i >= nk + (p.db ? p.C : 0)) return;
    const long long pitch = (long long)DW_ROWS * p.C;
    float v = (float)ml_sum_slices_f64(p.part + i, pitch, p.slices);
    if (i < nk) {
        if (p.add_k) v = p.add_k[i] + v;
        p.dk[i] = v;
    } else {
        if (p.add_b) v = p.add_b[i - nk] + v;
        p.db[i - nk] = v;
    }
}

__global__ void __launch_bounds__(DW_TPB) dw_dgrad_kernel(const DwArgs A) {
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.p[pi + 1].first_block) ++pi;
    const DwProblem &p = A.p[pi];
    const long long idx = (long long)(blockIdx.x - p.first_block) * DW_TPB + threadIdx.x;
    if (idx >= p.threads) return;
    const int cq = (int)(idx % p.CQ);
    long long pix = idx / p.CQ;
    const int ix = (int)(pix % p.W);
    const long long row = pix / p.W;
    const int iy = (int)(row % p.H), b = (int)(row / p.H);
    const int c = cq * 4;
    const int Ho = p.Ho, Wo = p.Wo, dil = p.dil;
    const int sh = p.stride - 1;                              // stride 1 or 2: a shift and a mask
    const float *dyc = p.dy + p.dy_co + c, *wc = p.wgt + c;
    bool ok[9];
    f32x4 g[9], w[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int ty = iy + p.pad_t - (t / 3) * dil, tx = ix + p.pad_l - (t % 3) * dil;
        const int oy = ty >> sh, ox = tx >> sh;
        ok[t] = ty >= 0 && tx >= 0 && ((ty | tx) & sh) == 0 && oy < Ho && ox < Wo;
        g[t] = w[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (ok[t]) {
            g[t] = ld4(dyc + (((long long)b * Ho + oy) * Wo + ox) * p.dy_cs);
            w[t] = ld4(wc + t * p.C);
        }
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t)
        if (ok[t]) acc += w[t] * g[t];
    const long long o = pix * p.C + c;
    if (p.add_x) acc = ld4(p.add_x + o) + acc;
    *reinterpret_cast<f32x4 *>(p.dx + o) = acc;
}

// the gradient in front of a ReLU whose output is y: dy where y > 0, else 0 (the ASPP's pooled branch: a conv + ReLU with no
// GroupNormalization behind it to carry the mask)
__global__ void __launch_bounds__(DW_TPB) relu_grad_kernel(const float *__restrict__ y, const float *dy, float *out, long long n) {
    const long long i = (long long)blockIdx.x * DW_TPB + threadIdx.x;
    if (i < n) out[i] = y[i] > 0.f ? dy[i] : 0.f;
}

struct DwPlan {
    int slices, sp, cl_shift, ctiles;
    long long P, bytes;
};

// the geometry both directions share
int dw_geometry(const char *what, const ml_dwconv3x3_grad_desc &d) {
    ML_REQUIRE(d.B > 0 && d.H > 0 && d.W > 0 && d.Ho > 0 && d.Wo > 0, "%s: bad dims", what);
    ML_REQUIRE(d.C > 0 && d.C % 4 == 0, "%s: C = %d must be a multiple of 4 (16-byte accesses)", what, d.C);
    ML_REQUIRE(d.stride == 1 || d.stride == 2, "%s: stride %d: 1 or 2", what, d.stride);
    ML_REQUIRE(d.dil >= 1, "%s: bad dilation", what);
    ML_REQUIRE(d.pad_t >= 0 && d.pad_l >= 0, "%s: bad padding", what);
    ML_REQUIRE(d.dy_cstride % 4 == 0 && d.dy_coff % 4 == 0 && d.dy_coff >= 0 && d.dy_coff + d.C <= d.dy_cstride,
               "%s: dy: channels [%d, %d) must be a 4-aligned slice of its %d", what, d.dy_coff, d.dy_coff + d.C, d.dy_cstride);
    // every window starts inside the padded image: the output size belongs to this input
    ML_REQUIRE((long long)(d.Ho - 1) * d.stride - d.pad_t < d.H && (long long)(d.Wo - 1) * d.stride - d.pad_l < d.W,
               "%s: the %d x %d output does not belong to the %d x %d input", what, d.Ho, d.Wo, d.H, d.W);
    ML_REQUIRE((long long)d.B * d.Ho * d.Wo < (1ll << 31) - DW_SLICE_MAX && (long long)d.B * d.H * d.W < (1ll << 31),
               "%s: too many pixels", what);
    ML_REQUIRE((long long)d.C * 9 + d.C < (1ll << 31), "%s: too many channels", what);
    return ML_OK;
}

int dw_wgrad_plan(const ml_dwconv3x3_grad_desc &d, DwPlan &pl) {
    const char *what = "dwconv3x3_wgrad";
    const int rc = dw_geometry(what, d);
    if (rc != ML_OK) return rc;
    ML_REQUIRE(d.in_cstride % 4 == 0 && d.in_coff % 4 == 0 && d.in_coff >= 0 && d.in_coff + d.C <= d.in_cstride,
               "%s: x: channels [%d, %d) must be a 4-aligned slice of its %d", what, d.in_coff, d.in_coff + d.C, d.in_cstride);
    pl.P = (long long)d.B * d.Ho * d.Wo;
    const long long sp = ml_slice_pixels(pl.P, 64, DW_ROUND, DW_SLICE_MIN, DW_SLICE_MAX);
    pl.sp = (int)sp;
    pl.slices = (int)((pl.P + sp - 1) / sp);
    const int CQ = d.C / 4;
    pl.cl_shift = 0;
    while ((1 << pl.cl_shift) < CQ && pl.cl_shift < 6) ++pl.cl_shift;
    pl.ctiles = (CQ + (1 << pl.cl_shift) - 1) >> pl.cl_shift;
    pl.bytes = ml_align256((long long)pl.slices * DW_ROWS * d.C * 4);
    return ML_OK;
}

void dw_fill(DwProblem &p, const ml_dwconv3x3_grad_desc &d) {
    p.x = d.x; p.dy = d.dy; p.wgt = d.wgt;
    p.part = nullptr;
    p.add_k = d.add_kernel; p.add_b = d.dbias ? d.add_bias : nullptr; p.add_x = d.add_x;
    p.dk = d.dkernel; p.db = d.dbias; p.dx = d.dx;
    p.H = d.H; p.W = d.W; p.Ho = d.Ho; p.Wo = d.Wo; p.HoWo = d.Ho * d.Wo; p.P = d.B * d.Ho * d.Wo;
    p.C = d.C; p.CQ = d.C / 4; p.in_cs = d.in_cstride; p.in_co = d.in_coff; p.dy_cs = d.dy_cstride; p.dy_co = d.dy_coff;
    p.stride = d.stride; p.dil = d.dil; p.pad_t = d.pad_t; p.pad_l = d.pad_l;
    p.slices = p.sp = p.cl_shift = p.ctiles = 0;
    p.first_block = p.first_fblock = 0;
    p.threads = 0;
}

}  // namespace

extern "C" int ml_dwconv3x3_wgrad_plan(const ml_dwconv3x3_grad_desc *desc, int32_t *slices, int32_t *slice_pixels,
                                       int64_t *workspace_bytes) {
    ML_REQUIRE(desc, "dwconv3x3_wgrad_plan: null descriptor");
    DwPlan pl;
    const int rc = dw_wgrad_plan(*desc, pl);
    if (rc != ML_OK) return rc;
    ml_plan_out(pl.slices, pl.sp, pl.bytes, slices, slice_pixels, workspace_bytes);
    return ML_OK;
}

extern "C" int ml_dwconv3x3_wgrad_multi_f32(const ml_dwconv3x3_grad_desc *descs, int32_t n, void *workspace,
                                            int64_t workspace_bytes, void *stream) {
    const char *what = "dwconv3x3_wgrad";
    ML_REQUIRE(descs && n >= 1 && n <= ML_DWCONV_GRAD_MAX_PROBLEMS, "%s: need 1..%d problems", what, ML_DWCONV_GRAD_MAX_PROBLEMS);
    ML_REQUIRE(workspace && (((uintptr_t)workspace) & 255) == 0, "%s: needs a 256-byte aligned workspace", what);
    DwArgs A;
    long long used = 0, blocks = 0, fblocks = 0;
    for (int i = 0; i < n; ++i) {
        const ml_dwconv3x3_grad_desc &d = descs[i];
        DwPlan pl;
        const int rc = dw_wgrad_plan(d, pl);
        if (rc != ML_OK) return rc;
        ML_REQUIRE(d.x && d.dy && d.dkernel, "%s: problem %d: null pointer", what, i);
        ML_REQUIRE(ml_aligned16(d.x) && ml_aligned16(d.dy), "%s: problem %d: x and dy must be 16-byte aligned", what, i);
        ML_REQUIRE((((uintptr_t)d.dkernel | (uintptr_t)d.dbias | (uintptr_t)d.add_kernel | (uintptr_t)d.add_bias) & 3) == 0,
                   "%s: problem %d: 4-byte alignment", what, i);
        const long long x_bytes = (long long)d.B * d.H * d.W * d.in_cstride * 4, dy_bytes = pl.P * d.dy_cstride * 4;
        const long long dk_bytes = 9ll * d.C * 4, db_bytes = (long long)d.C * 4;
        ML_REQUIRE(!ml_any_overlap({{d.dkernel, dk_bytes}, {d.dbias, db_bytes}}, {{d.x, x_bytes}, {d.dy, dy_bytes}}) &&
                   !ml_ranges_overlap(d.dbias, db_bytes, d.dkernel, dk_bytes), "%s: problem %d: the outputs may not overlap x, dy or "
                   "each other", what, i);
        ML_REQUIRE(ml_add_or_disjoint(d.dkernel, d.add_kernel, dk_bytes),
                   "%s: problem %d: dkernel may be add itself, not a shifted view of it", what, i);
        ML_REQUIRE(ml_add_or_disjoint(d.dbias, d.add_bias, db_bytes),
                   "%s: problem %d: dbias may be add itself, not a shifted view of it", what, i);
        DwProblem &p = A.p[i];
        dw_fill(p, d);
        p.part = ml_carve_partials(what, i, workspace, workspace_bytes, used, pl.bytes);
        if (!p.part) return ML_E_BADARG;
        p.slices = pl.slices; p.sp = pl.sp; p.cl_shift = pl.cl_shift; p.ctiles = pl.ctiles;
        p.first_block = (int)blocks; p.first_fblock = (int)fblocks;
        blocks += (long long)pl.slices * pl.ctiles;
        fblocks += (10ll * d.C + DW_TPB - 1) / DW_TPB;
        ML_REQUIRE(blocks < (1ll << 31) && fblocks < (1ll << 31), "%s: grid too large", what);
    }
    A.n = n;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dw_wgrad_partial_kernel, dim3((unsigned)blocks), dim3(DW_TPB), 0, s, A);
    hipLaunchKernelGGL(dw_wgrad_finish_kernel, dim3((unsigned)fblocks), dim3(DW_TPB), 0, s, A);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_dwconv3x3_dgrad_multi_f32(const ml_dwconv3x3_grad_desc *descs, int32_t n, void *stream) {
    const char *what = "dwconv3x3_dgrad";
    ML_REQUIRE(descs && n >= 1 && n <= ML_DWCONV_GRAD_MAX_PROBLEMS, "%s: need 1..%d problems", what, ML_DWCONV_GRAD_MAX_PROBLEMS);
    DwArgs A;
    long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        const ml_dwconv3x3_grad_desc &d = descs[i];
        const int rc = dw_geometry(what, d);
        if (rc != ML_OK) return rc;
        ML_REQUIRE(d.dy && d.wgt && d.dx, "%s: problem %d: null pointer", what, i);
        ML_REQUIRE(ml_aligned16(d.dy) && ml_aligned16(d.wgt) && ml_aligned16(d.dx) && ml_aligned16(d.add_x),
                   "%s: problem %d: pointers must be 16-byte aligned", what, i);
        const long long dx_bytes = (long long)d.B * d.H * d.W * d.C * 4;
        ML_REQUIRE(!ml_any_overlap({{d.dx, dx_bytes}}, {{d.dy, (long long)d.B * d.Ho * d.Wo * d.dy_cstride * 4}, {d.wgt, 9ll * d.C * 4}}),
                   "%s: problem %d: dx may not overlap dy or the kernel", what, i);
        ML_REQUIRE(ml_add_or_disjoint(d.dx, d.add_x, dx_bytes),
                   "%s: problem %d: dx may be add itself, not a shifted view of it", what, i);
        for (int j = 0; j < i; ++j)
            ML_REQUIRE(!ml_ranges_overlap(d.dx, dx_bytes, descs[j].dx, (long long)descs[j].B * descs[j].H * descs[j].W * descs[j].C * 4),
                       "%s: problems %d and %d write the same dx (chain them through add= in separate launches)", what, j, i);
        DwProblem &p = A.p[i];
        dw_fill(p, d);
        p.threads = (long long)d.B * d.H * d.W * (d.C / 4);
        p.first_block = (int)blocks;
        blocks += (p.threads + DW_TPB - 1) / DW_TPB;
        ML_REQUIRE(blocks < (1ll << 31), "%s: grid too large", what);
    }
    A.n = n;
    hipLaunchKernelGGL(dw_dgrad_kernel, dim3((unsigned)blocks), dim3(DW_TPB), 0, (hipStream_t)stream, A);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_relu_grad_f32(const float *y, const float *dy, float *out, int64_t n, void *stream) {
    ML_REQUIRE(y && dy && out && n > 0 && n < (1ll << 31) * DW_TPB, "relu_grad: bad arguments");
    ML_REQUIRE(ml_add_or_disjoint(out, dy, n * 4), "relu_grad: out may be dy itself, not a shifted view of it");
    ML_REQUIRE(!ml_ranges_overlap(out, n * 4, y, n * 4), "relu_grad: out may not overlap y");
    hipLaunchKernelGGL(relu_grad_kernel, dim3((unsigned)((n + DW_TPB - 1) / DW_TPB)), dim3(DW_TPB), 0, (hipStream_t)stream, y, dy,
                       out, (long long)n);
    ML_CHECK_LAUNCH("relu_grad");
    return ML_OK;
}
