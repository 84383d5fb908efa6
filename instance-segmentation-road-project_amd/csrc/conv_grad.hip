// Backward of the dense convolutions, fp32: the weight and bias gradient (this file's GEMM kernel), the small gather
// that brings a `dy` view into the form the stride-1 data gradient reads, and the STRIDE-2 data gradient (second half of the
// file).  The stride-1 data gradient is the FORWARD kernels on transposed weights (masklab_hip/packing.py
// pack_dense_transposed, ops.conv2d_dgrad): nothing of it lives here.
//
//   dW[kh,kw,ci,co] = sum over (b,oy,ox) of x[b, oy*s + kh*d - pad_t, ox*s + kw*d - pad_l, ci] * dy[b,oy,ox,co]
//   db[co]          = sum over (b,oy,ox) of dy[b,oy,ox,co]
//
// Per tap a GEMM with M = cin, N = cout and K = the B*Ho*Wo output pixels, on v_mfma_f32_32x32x2_f32 (exact fp32 products,
// a k-ordered fp32 fma chain).  Both operands are NHWC, so a [pixel][channel] LDS image feeds A (x: row = ci) and B (dy:
// column = co) with consecutive-dword reads: lane l takes (channel l % 32, pixel l / 32) of a 2-pixel step, no transpose.
//
// Work units.  A UNIT is (32-channel cin tile, tap); a block holds up to WG_UNITS = 9 units as accumulators (the nine taps of
// one cin tile of a 3x3 conv; the cin tiles of a 1x1 conv; three groups for 5x5) for a 128-wide cout tile -- 4 waves x 32
// columns -- over ONE slice of the pixels.  Per 16-pixel chunk the dy tile is staged once and shared by the units; x is
// staged per unit (the shifted pixels of its tap), zeros where a tap leaves the image; two staging buffers, so the next
// chunk's requests fly under this chunk's 72 MFMAs per wave.  x and an aligned dy arrive by
// LDS-DMA (gfx_mem.h); a dy view whose rows are not 16-byte aligned (the towers' 75- and 60-wide output convs write into
// [B, A, d] predictions) is read with dword loads.
//
// No float atomics.  K is cut into slices of about 1 / 128 of the problem's pixels, at least WG_SLICE_MIN = 512 and at most
// WG_SLICE_MAX = 1024 pixels (longer only where the partials of a problem would exceed WG_SHARE bytes of the conv workspace):
// a function of the problem's geometry alone, never of the launch, the other problems or the device.  A block accumulates
// its slice in fp32 in pixel order and writes a partial; the finish kernel adds the partials of an element in ascending
// slice order in fp64, rounds once, adds `add` with one fp32 addition and writes dkernel [kh,kw,cin,cout] (the Keras
// layout) and dbias.  The column sums of dy ride in the blocks of unit group 0 (fp64 over the
// slice, from the staged tile: dy is read once).  Every element is written; a tap that only meets padding gets exact zeros.
#include "gfx_mem.h"
#include "slice_sum.h"

namespace {

constexpr int WG_TPB = 256;
constexpr int WG_BM = 32;            // cin per unit
constexpr int WG_BN = 128;           // cout per block: 4 waves x 32
constexpr int WG_KP = 16;            // pixels per staged chunk
constexpr int WG_ROUND = 32;         // slice lengths are multiples of this (and of WG_KP)
constexpr int WG_UNITS = 9;          // (cin tile, tap) units a block accumulates
constexpr int WG_SLICE_MIN = 512;    // pixels per slice (multiples of WG_KP): P / 128 clamped to [MIN, MAX] -- the 8 x 128 x 128
constexpr int WG_SLICE_MAX = 1024;   // map of a tower is 128 slices x 4 unit groups = two blocks on each of 256 CUs
constexpr long long WG_SHARE = 96ll << 20;   // bytes of partials one problem may take: beyond, its slices grow
constexpr int WG_OOB = (int)0x80000000;      // a buffer offset beyond every extent (< 2 GiB): the lane reads zeros

struct WgProblem {
    const float *x, *dy;             // dy: the view's first element (channel offset applied)
    float *part, *bpart;             // [slices][T*cin*cout], [slices][cout]
    const float *add_k, *add_b;
    float *dk, *db;
    long long dy_bs;                 // floats between images of dy
    int H, W, Wo, HoWo, P;           // P = B*Ho*Wo
    int in_cs, in_co, cin, cout, dy_cs;
    int KW, T, stride, dil, pad_t, pad_l;
    int x_bytes, dy_bytes;
    int slices, sp;
    int NT, units, ugroups;          // cout tiles, (cin tile, tap) units, groups of WG_UNITS units
    int dy_vec;                      // 1: 16-byte rows (LDS-DMA), 0: dword loads
    int first_block, first_fblock;   // of the partial / finish launch
    int tcc;                         // T*cin*cout
};
struct WgArgs {
    WgProblem p[ML_CONV_WGRAD_MAX_PROBLEMS];
    int n;
};

__global__ void __launch_bounds__(WG_TPB, 2) conv_wgrad_partial_kernel(const WgArgs A) {
    // two staging buffers: chunk i + 1 is on its way into one while the MFMAs read chunk i from the other
    __shared__ __align__(16) float sx[2][WG_UNITS][WG_KP * WG_BM];
    __shared__ __align__(16) float sy[2][WG_KP * WG_BN];
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.p[pi + 1].first_block) ++pi;
    const WgProblem &p = A.p[pi];
    int id = blockIdx.x - p.first_block;
    const int nt = id % p.NT; id /= p.NT;
    const int ug = id % p.ugroups;
    const int slice = id / p.ugroups;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int H = p.H, W = p.W, Wo = p.Wo, HoWo = p.HoWo, cin = p.cin, cout = p.cout, T = p.T;
    const int in_cs = p.in_cs, in_co = p.in_co, dy_cs = p.dy_cs, stride = p.stride, pad_t = p.pad_t, pad_l = p.pad_l;
    const long long dy_bs = p.dy_bs;
    const float *dyp = p.dy;
    const bool dy_vec = p.dy_vec != 0;
    const int n0 = nt * WG_BN;
    const int wn0 = n0 + wave * 32;                          // this wave's first column
    const int nu = min(WG_UNITS, p.units - ug * WG_UNITS);   // units of this block
    const int q_begin = slice * p.sp, q_end = min(q_begin + p.sp, p.P);
    const bool do_bias = ug == 0;

    // per unit: its tap's pixel offset (dy, dx) and its cin tile, wave-uniform (past the problem's last unit: that unit again)
    int u_dy[WG_UNITS], u_dx[WG_UNITS], u_c[WG_UNITS];
#pragma unroll
    for (int u = 0; u < WG_UNITS; ++u) {
        const int U = min(ug * WG_UNITS + u, p.units - 1);
        const int mt = U / T, tap = U - mt * T;
        const int kh = tap / p.KW, kw = tap - kh * p.KW;
        u_dy[u] = kh * p.dil; u_dx[u] = kw * p.dil; u_c[u] = mt * WG_BM;
    }

    const __amdgpu_buffer_rsrc_t rsrc_x = rsrc_bytes(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_y = rsrc_bytes(p.dy, p.dy_bytes);
    // x staging: a unit's tile is 16 pixels x 32 channels = two 1 KB DMAs (8 pixels each).  Waves 0 / 1 bring the two halves
    // of the even units, waves 2 / 3 those of the odd units; a lane's pixel row and channels are the same for every unit.
    const int xhalf = wave & 1, xpar = wave >> 1;
    const int xrow = xhalf * 8 + (lane >> 3), xc4 = (lane & 7) * 4;
    constexpr int YS = WG_KP * WG_BN / WG_TPB;               // floats of a dy tile per thread on the dword path
    float yreg[YS];

    // requests chunk `base` into buffer `buf`; on the dword path the dy tile comes into registers (commit() stores it)
    auto issue = [&](int buf, int base) {
        {
            const int q = base + xrow;
            const bool valid = q < q_end;
            const int b = q / HoWo, rem = q - b * HoWo;
            const int oy = rem / Wo, ox = rem - oy * Wo;
            const int iy0 = oy * stride - pad_t, ix0 = ox * stride - pad_l;
            const long long pix0 = ((long long)b * H + iy0) * W + ix0;
#pragma unroll
            for (int u = 0; u < WG_UNITS; ++u) {
                if ((u & 1) != xpar) continue;               // wave-uniform
                const int iy = iy0 + u_dy[u], ix = ix0 + u_dx[u];
                const int c = u_c[u] + xc4;
                const bool ok = valid && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W && c < cin;
                const long long off = (pix0 + (long long)u_dy[u] * W + u_dx[u]) * in_cs + in_co + c;
                lds_dma16(rsrc_x, (char *)(&sx[buf][u][0] + xhalf * 8 * WG_BM), ok ? (int)(off * 4) : WG_OOB, 0);
            }
        }
        // dy: [16 pixels][128 columns], zeros past the slice and past cout
        if (dy_vec) {
#pragma unroll
            for (int j = 0; j < WG_KP / 8; ++j) {
                const int row = j * 8 + wave * 2;
                const int q = base + row + h;
                const int b = q / HoWo, rem = q - b * HoWo;
                const int c = n0 + r * 4;
                const bool ok = q < q_end && c < cout;
                const long long off = (long long)b * dy_bs + (long long)rem * dy_cs + c;
                lds_dma16(rsrc_y, (char *)(&sy[buf][0] + row * WG_BN), ok ? (int)(off * 4) : WG_OOB, 0);
            }
        } else {
            const int c = n0 + (tid & 127);
#pragma unroll
            for (int j = 0; j < YS; ++j) {
                const int q = base + j * 2 + (tid >> 7);
                const int b = q / HoWo, rem = q - b * HoWo;
                float v = 0.f;
                if (q < q_end && c < cout) v = dyp[(long long)b * dy_bs + (long long)rem * dy_cs + c];
                yreg[j] = v;
            }
        }
    };
    auto commit = [&](int buf) {
        if (!dy_vec) {
#pragma unroll
            for (int j = 0; j < YS; ++j) sy[buf][(j * 2 + (tid >> 7)) * WG_BN + (tid & 127)] = yreg[j];
        }
    };

    f32x16 acc[WG_UNITS];
#pragma unroll
    for (int u = 0; u < WG_UNITS; ++u)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[u][e] = 0.f;
    double bacc = 0.0;

    issue(0, q_begin);
    commit(0);
    int buf = 0;
    for (int base = q_begin; base < q_end; base += WG_KP) {
        // this chunk has landed (every wave waits for its own requests, then for the others), and every wave is past its
        // reads of the other buffer
        wait_vmcnt<0>();
        __syncthreads();
        const bool more = base + WG_KP < q_end;
        if (more) issue(buf ^ 1, base + WG_KP);
        const float *cy = &sy[buf][0];
        if (do_bias && tid < WG_BN) {
#pragma unroll
            for (int k = 0; k < WG_KP; ++k) bacc += (double)cy[k * WG_BN + tid];
        }
        if (wn0 < cout) {                                    // wave-uniform: a 32-column quarter past cout runs no MFMA
            // No test per unit: it would put every LDS read behind the MFMA before it, and each MFMA behind its read's
            // latency.  The units a last, partial group lacks repeat the problem's last unit; their sums are not stored.
#pragma unroll
            for (int ks = 0; ks < WG_KP / 2; ++ks) {
                const int k = 2 * ks + h;
                const float bv = cy[k * WG_BN + wave * 32 + r];
                static_for<0, WG_UNITS>([&](auto uc) {
                    constexpr int u = decltype(uc)::value;
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(sx[buf][u][k * WG_BM + r], bv, acc[u], 0, 0, 0);
                });
            }
        }
        if (more) commit(buf ^ 1);
        buf ^= 1;
    }

    // ---- the partial.  C/D layout: col = lane & 31 (cout), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (cin)
    float *part = p.part + (long long)slice * p.tcc;
    const int co = wn0 + r;
    if (co < cout) {
        static_for<0, WG_UNITS>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            if (u < nu) {
                const int U = ug * WG_UNITS + u;
                const int mt = U / T, tap = U - mt * T;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int ci = mt * WG_BM + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (ci < cin) part[((long long)tap * cin + ci) * cout + co] = acc[u][e];
                }
            }
        });
    }
    if (do_bias && tid < WG_BN && n0 + tid < cout) p.bpart[(long long)slice * cout + n0 + tid] = (float)bacc;
}

// element i of a problem: i < tcc -> dkernel[i], else dbias[i - tcc]; partials added in ascending slice order in fp64
__global__ void __launch_bounds__(WG_TPB) conv_wgrad_finish_kernel(const WgArgs A) {
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.p[pi + 1].first_fblock) ++pi;
    const WgProblem &p = A.p[pi];
    const int i = (blockIdx.x - p.first_fblock) * WG_TPB + threadIdx.x;
    const int total = p.tcc + (p.db ? p.cout : 0);
    if (i >= total) return;
    const bool bias = i >= p.tcc;
    const int j = bias ? i - p.tcc : i;
    const float *src = bias ? p.bpart : p.part;
    const long long pitch = bias ? p.cout : p.tcc;
    float v = (float)ml_sum_slices_f64(src + j, pitch, p.slices);
    const float *add = bias ? p.add_b : p.add_k;
    if (add) v = add[j] + v;
    (bias ? p.db : p.dk)[j] = v;
}

__global__ void __launch_bounds__(WG_TPB)
gather_dy_kernel(const float *__restrict__ dy, float *__restrict__ out, int HW, int cout, int cp, int dy_cs, long long dy_bs,
                 long long total) {
    const long long i = (long long)blockIdx.x * WG_TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % cp);
    const long long pix = i / cp;
    const int b = (int)(pix / HW), rem = (int)(pix - (long long)b * HW);
    out[i] = c < cout ? dy[(long long)b * dy_bs + (long long)rem * dy_cs + c] : 0.f;
}

struct WgPlan {
    int slices, sp, T, MT, NT, units, ugroups;
    long long tcc, bytes, dy_bs, P;
};

// the checks of one problem and its slices: geometry only
int wg_plan(const ml_conv2d_desc &d, WgPlan &pl) {
    const char *what = "conv2d_wgrad";
    ML_REQUIRE(d.math != ML_MATH_F16S && !d.out_f16, "%s: half tensors are refused (the backward is float32 only)", what);
    ML_REQUIRE(!d.group_cin_step, "%s: grouped / depthwise problems are refused (dense convolutions only)", what);
    ML_REQUIRE(d.cpp_shift == 30, "%s: row-span (image input) problems are refused (dense convolutions only)", what);
    ML_REQUIRE(!d.shuffle2x2, "%s: shuffle2x2 (Conv2DTranspose) problems are refused (dense convolutions only)", what);
    ML_REQUIRE(d.B > 0 && d.H > 0 && d.W > 0 && d.Ho > 0 && d.Wo > 0, "%s: bad dims", what);
    ML_REQUIRE(d.KH >= 1 && d.KH <= 5 && d.KW >= 1 && d.KW <= 5, "%s: kernel %d x %d: at most 5 x 5", what, d.KH, d.KW);
    ML_REQUIRE(d.stride == 1 || d.stride == 2, "%s: stride %d: 1 or 2", what, d.stride);
    ML_REQUIRE(d.dil >= 1, "%s: bad dilation", what);
    ML_REQUIRE(d.span > 0 && d.span % 4 == 0 && d.in_cstride % 4 == 0 && d.in_coff % 4 == 0 && d.in_coff >= 0 &&
               d.in_coff + d.span <= d.in_cstride, "%s: cin, the input's channel stride and offset must be multiples of 4, "
               "the slice inside the buffer", what);
    ML_REQUIRE(d.cout >= 1 && d.out_coff >= 0 && d.out_coff + d.cout <= d.out_cstride, "%s: dy: cout channels from its offset "
               "must fit its channel stride", what);
    const long long HoWo = (long long)d.Ho * d.Wo;
    ML_REQUIRE(d.out_bstride == 0 || d.out_bstride >= HoWo * d.out_cstride, "%s: dy: images overlap", what);
    pl.dy_bs = d.out_bstride ? d.out_bstride : HoWo * d.out_cstride;
    pl.P = (long long)d.B * HoWo;
    ML_REQUIRE(pl.P < (1ll << 31) - WG_SLICE_MAX, "%s: too many pixels", what);
    ML_REQUIRE((long long)d.B * d.H * d.W * d.in_cstride * 4 < (1ll << 31), "%s: x must be smaller than 2 GiB", what);
    ML_REQUIRE((((long long)d.B - 1) * pl.dy_bs + HoWo * d.out_cstride) * 4 < (1ll << 31), "%s: dy must span less than 2 GiB", what);
    pl.T = d.KH * d.KW;
    pl.tcc = (long long)pl.T * d.span * d.cout;
    ML_REQUIRE(pl.tcc + d.cout < (1ll << 31), "%s: too many weights", what);
    pl.MT = (d.span + WG_BM - 1) / WG_BM;
    pl.NT = (d.cout + WG_BN - 1) / WG_BN;
    pl.units = pl.MT * pl.T;
    pl.ugroups = (pl.units + WG_UNITS - 1) / WG_UNITS;
    // a problem's partials may take WG_SHARE bytes of the conv workspace (the five levels of a tower depth take 170 MiB)
    const long long per_slice = (pl.tcc + d.cout) * 4;
    const long long max_slices = (WG_SHARE - 512) / per_slice;
    ML_REQUIRE(max_slices >= 1, "%s: one partial (%lld bytes) exceeds a problem's share of the conv workspace", what, per_slice);
    long long sp = ml_slice_pixels(pl.P, 128, WG_ROUND, WG_SLICE_MIN, WG_SLICE_MAX);
    if ((pl.P + sp - 1) / sp > max_slices) sp = ((pl.P + max_slices - 1) / max_slices + WG_ROUND - 1) / WG_ROUND * WG_ROUND;
    pl.sp = (int)sp;
    pl.slices = (int)((pl.P + sp - 1) / sp);
    pl.bytes = ml_align256(pl.slices * pl.tcc * 4) + ml_align256((long long)pl.slices * d.cout * 4);
    return ML_OK;
}

}  // namespace

extern "C" int ml_conv2d_wgrad_plan(const ml_conv2d_wgrad_desc *desc, int32_t *slices, int32_t *slice_pixels,
                                    int64_t *workspace_bytes) {
    ML_REQUIRE(desc, "conv2d_wgrad_plan: null descriptor");
    WgPlan pl;
    const int rc = wg_plan(desc->conv, pl);
    if (rc != ML_OK) return rc;
    ml_plan_out(pl.slices, pl.sp, pl.bytes, slices, slice_pixels, workspace_bytes);
    return ML_OK;
}

extern "C" int ml_conv2d_wgrad_multi_f32(const ml_conv2d_wgrad_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes,
                                         void *stream) {
    const char *what = "conv2d_wgrad";
    ML_REQUIRE(descs && n >= 1 && n <= ML_CONV_WGRAD_MAX_PROBLEMS, "%s: need 1..%d problems", what, ML_CONV_WGRAD_MAX_PROBLEMS);
    ML_REQUIRE(workspace && (((uintptr_t)workspace) & 255) == 0, "%s: needs a 256-byte aligned workspace", what);
    WgArgs A;
    long long used = 0, blocks = 0, fblocks = 0;
    for (int i = 0; i < n; ++i) {
        const ml_conv2d_wgrad_desc &g = descs[i];
        const ml_conv2d_desc &d = g.conv;
        WgPlan pl;
        const int rc = wg_plan(d, pl);
        if (rc != ML_OK) return rc;
        ML_REQUIRE(d.in && d.out && g.dkernel, "%s: problem %d: null pointer", what, i);
        ML_REQUIRE(ml_aligned16(d.in), "%s: problem %d: x must be 16-byte aligned", what, i);
        ML_REQUIRE((((uintptr_t)d.out | (uintptr_t)g.dkernel | (uintptr_t)g.dbias | (uintptr_t)g.add_kernel |
                     (uintptr_t)g.add_bias) & 3) == 0, "%s: problem %d: 4-byte alignment", what, i);
        const long long x_bytes = (long long)d.B * d.H * d.W * d.in_cstride * 4;
        // dy's resource extent (what the hardware clamps): whole channel strides from d.out on, past the view's last element
        const long long dy_bytes = (((long long)d.B - 1) * pl.dy_bs + (long long)d.Ho * d.Wo * d.out_cstride) * 4;
        const long long dk_bytes = pl.tcc * 4, db_bytes = (long long)d.cout * 4;
        // what can alias: x from its buffer's base, dy from the view's first element to its last
        const ml_range r_x = {d.in, x_bytes}, r_dk = {g.dkernel, dk_bytes}, r_db = {g.dbias, db_bytes};
        const ml_range r_dy = {d.out + d.out_coff, ml_view_elems(d.B, pl.dy_bs, (long long)d.Ho * d.Wo, d.out_cstride, d.cout) * 4};
        ML_REQUIRE(!ml_any_overlap({r_dk}, {r_x, r_dy}), "%s: problem %d: dkernel may not overlap x or dy", what, i);
        ML_REQUIRE(ml_add_or_disjoint(g.dkernel, g.add_kernel, dk_bytes), "%s: problem %d: dkernel may be add itself, not a shifted "
                   "view of it", what, i);
        ML_REQUIRE(!ml_any_overlap({r_db}, {r_x, r_dy, r_dk}), "%s: problem %d: dbias may not overlap x, dy or dkernel", what, i);
        ML_REQUIRE(ml_add_or_disjoint(g.dbias, g.add_bias, db_bytes), "%s: problem %d: dbias may be add itself, not a shifted view "
                   "of it", what, i);
        WgProblem &p = A.p[i];
        p.x = d.in; p.dy = d.out + d.out_coff;
        p.part = ml_carve_partials(what, i, workspace, workspace_bytes, used, pl.bytes);
        if (!p.part) return ML_E_BADARG;
        p.bpart = p.part + ml_align256(pl.slices * pl.tcc * 4) / 4;
        p.add_k = g.add_kernel; p.add_b = g.dbias ? g.add_bias : nullptr; p.dk = g.dkernel; p.db = g.dbias;
        p.dy_bs = pl.dy_bs;
        p.H = d.H; p.W = d.W; p.Wo = d.Wo; p.HoWo = d.Ho * d.Wo; p.P = (int)pl.P;
        p.in_cs = d.in_cstride; p.in_co = d.in_coff; p.cin = d.span; p.cout = d.cout; p.dy_cs = d.out_cstride;
        p.KW = d.KW; p.T = pl.T; p.stride = d.stride; p.dil = d.dil; p.pad_t = d.pad_t; p.pad_l = d.pad_l;
        p.x_bytes = (int)x_bytes; p.dy_bytes = (int)(dy_bytes - (long long)d.out_coff * 4);
        p.slices = pl.slices; p.sp = pl.sp; p.NT = pl.NT; p.units = pl.units; p.ugroups = pl.ugroups;
        p.dy_vec = d.cout % 4 == 0 && d.out_cstride % 4 == 0 && d.out_coff % 4 == 0 && pl.dy_bs % 4 == 0 && ml_aligned16(d.out);
        p.tcc = (int)pl.tcc;
        p.first_block = (int)blocks; p.first_fblock = (int)fblocks;
        blocks += (long long)pl.slices * pl.ugroups * pl.NT;
        fblocks += (pl.tcc + d.cout + WG_TPB - 1) / WG_TPB;
        ML_REQUIRE(blocks < (1ll << 31) && fblocks < (1ll << 31), "%s: grid too large", what);
    }
    A.n = n;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(conv_wgrad_partial_kernel, dim3((unsigned)blocks), dim3(WG_TPB), 0, s, A);
    hipLaunchKernelGGL(conv_wgrad_finish_kernel, dim3((unsigned)fblocks), dim3(WG_TPB), 0, s, A);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_conv2d_grad_gather_dy_f32(const float *dy, float *out, int32_t B, int32_t HW, int32_t cout, int32_t dy_cstride,
                                            int64_t dy_bstride, void *stream) {
    const char *what = "conv2d_grad_gather_dy";
    ML_REQUIRE(dy && out && B > 0 && HW > 0 && cout > 0, "%s: bad arguments", what);
    ML_REQUIRE(dy_cstride >= cout && (dy_bstride == 0 || dy_bstride >= (long long)HW * dy_cstride), "%s: bad view", what);
    const int cp = (cout + 3) / 4 * 4;
    const long long bs = dy_bstride ? dy_bstride : (long long)HW * dy_cstride;
    const long long total = (long long)B * HW * cp;
    ML_REQUIRE((long long)B * HW < (1ll << 31) && total < (1ll << 31) * WG_TPB, "%s: too many pixels", what);
    ML_REQUIRE(!ml_ranges_overlap(out, total * 4, dy, ml_view_elems(B, bs, HW, dy_cstride, cout) * 4), "%s: out may not overlap dy", what);
    hipLaunchKernelGGL(gather_dy_kernel, dim3((unsigned)((total + WG_TPB - 1) / WG_TPB)), dim3(WG_TPB), 0, (hipStream_t)stream, dy,
                       out, HW, cout, cp, dy_cstride, bs, total);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

// ---------------------------------------------------------------------------------------------- stride-2 data gradient
//   dx[b,iy,ix,ci] = (add +) sum over the taps (ky,kx) with iy + pad_t - ky*d and ix + pad_l - kx*d both even and
//                    oy = (iy + pad_t - ky*d) / 2 in [0,Ho), ox likewise in [0,Wo), of sum_co dy[b,oy,ox,co] * w[ky,kx,ci,co]
// The parity of (iy, ix) fixes which taps are live, so the input pixels fall into four CLASSES (class = 2 (iy & 1) + (ix & 1));
// inside a class the gradient is a stride-1 walk over dy: pixel (2 cy + py, 2 cx + px) reads dy at (cy + off_y, cx + off_x)
// with one offset pair per live tap.  Per class a GEMM with M = cin, N = the class's pixels (b, cy, cx ascending) and
// K = live taps x cout on v_mfma_f32_32x32x2_f32 -- the weights as operand A, so a lane's four accumulator registers of a
// row group are four consecutive cin of ONE pixel and dx is stored as float4 straight from registers.  No zero-inserted dy,
// no MFMA for a dead tap: the MACs are the forward's.
//
// A block: DG_BM = 128 pixels of one class (4 waves x 32) by NT x 32 input channels (NT = 1 .. 4: the instantiation is picked
// by cin), its K loop over (live tap ascending, cout ascending in chunks of DG_KC = 32).  Per chunk dy [128 pixels][32 co] and
// w [NT x 32 ci][32 co] -- the Keras kernel as it stands, co contiguous -- arrive by LDS-DMA (gfx_mem.h) into one of two
// staging buffers; window positions outside [0,Ho) x [0,Wo), pixels past the class, channels past cin / cout are requested
// beyond the resource's extent and land as zeros.  A row is 8 granules of 16 bytes; granule j of row r sits at position
// j ^ ((r >> 1) & 7), so the ds_read_b128 of a lane's (row, j) is conflict-free in every 16-lane group (two rows share a
// 256-byte bank row; the rows of a group take 16 different slots).  Both lane halves read the granule and take
// co = 4j + h and 4j + 2 + h of it: an accumulator sees co ascending.  No atomics, no split along K, nothing read from
// another block's output: the same bits run to run, and `out` may be `add`.  Every dx element is written by the launch: a
// class without live taps, or a pixel whose taps all fall outside dy, gets add (bit for bit) or +0.0.
namespace {

constexpr int DG_TPB = 256;
constexpr int DG_BM = 128;           // pixels per block: 4 waves x 32
constexpr int DG_KC = 32;            // cout per staged chunk
constexpr int DG_MAXK = 5;           // kernel extent per axis

struct DgAxis {                      // the live taps of one parity along one axis, ascending: output index = (input index >> 1) + off
    int n;
    int k[DG_MAXK], off[DG_MAXK];
};
struct DgArgs {
    const float *dy, *w, *add;
    float *dx;
    int B, H, W, Ho, Wo, cin, cout, KW;
    int dy_bytes, w_bytes;
    int ntn;                         // N (cin) tiles
    int first_tile[5];               // pixel tiles before class c; [4] = all
    int Hc[2], Wc[2];                // rows / columns of each parity
    DgAxis ay[2], ax[2];
};

template <int NT>
__global__ void __launch_bounds__(DG_TPB, 2) conv_dgrad_s2_kernel(const DgArgs A) {
    __shared__ __align__(16) float sy[2][DG_BM * DG_KC];
    __shared__ __align__(16) float sw[2][NT * 32 * DG_KC];
    const int nt = blockIdx.x % A.ntn;
    int mt = blockIdx.x / A.ntn;
    int cls = 0;
    while (cls < 3 && mt >= A.first_tile[cls + 1]) ++cls;
    mt -= A.first_tile[cls];
    const int py = cls >> 1, px = cls & 1;
    const DgAxis &ay = A.ay[py], &ax = A.ax[px];
    const int ny = ay.n, nx = ax.n;
    if (ny * nx == 0 && A.add == A.dx) return;               // in place, no live tap: the class already holds add

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int H = A.H, W = A.W, Ho = A.Ho, Wo = A.Wo, cin = A.cin, cout = A.cout;
    const int Wc = A.Wc[px], HcWc = A.Hc[py] * Wc, Mc = A.B * HcWc;
    const int m0 = mt * DG_BM, n0 = nt * NT * 32;

    // staging: one DMA of the block brings 32 rows (8 per wave, 8 granules each); a lane's row within its wave's 8 and its
    // granule position are the same for every DMA, and so is the granule it fetches (the swizzle repeats every 16 rows)
    const int g_row = lane >> 3;
    const int g_j = (lane & 7) ^ ((4 * (wave & 1) + (g_row >> 1)) & 7);
    int y_base[4], y_cy[4], y_cx[4];                         // per dy DMA: the row's image base in dy pixels (-1: past the class)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + (i * 4 + wave) * 8 + g_row;
        const int b = m / HcWc, rem = m - b * HcWc;
        y_cy[i] = rem / Wc;
        y_cx[i] = rem - y_cy[i] * Wc;
        y_base[i] = m < Mc ? b * Ho * Wo : -1;
    }
    const __amdgpu_buffer_rsrc_t rsrc_y = rsrc_bytes(A.dy, A.dy_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = rsrc_bytes(A.w, A.w_bytes);

    // requests chunk (live tap ty, tx; channels c0 ..) into buffer `buf`
    auto issue = [&](int buf, int ty, int tx, int c0) {
        const int oyo = ay.off[ty], oxo = ax.off[tx];
        const int tap = ay.k[ty] * A.KW + ax.k[tx];
        const int c = c0 + 4 * g_j;
        const bool cok = c < cout;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int oy = y_cy[i] + oyo, ox = y_cx[i] + oxo;
            const bool ok = cok && y_base[i] >= 0 && (unsigned)oy < (unsigned)Ho && (unsigned)ox < (unsigned)Wo;
            const int off = ((y_base[i] + oy * Wo + ox) * cout + c) * 4;
            lds_dma16(rsrc_y, (char *)(&sy[buf][0] + (i * 4 + wave) * 8 * DG_KC), ok ? off : WG_OOB, 0);
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int ci = n0 + (i * 4 + wave) * 8 + g_row;
            const bool ok = cok && ci < cin;
            const int off = ((tap * cin + ci) * cout + c) * 4;
            lds_dma16(rsrc_w, (char *)(&sw[buf][0] + (i * 4 + wave) * 8 * DG_KC), ok ? off : WG_OOB, 0);
        }
    };

    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;

    const int kchunks = (cout + DG_KC - 1) / DG_KC;
    const int chunks = ny * nx * kchunks;
    int ty = 0, tx = 0, kc = 0;                              // the next chunk to request
    auto advance = [&]() {
        if (++kc == kchunks) {
            kc = 0;
            if (++tx == nx) { tx = 0; ++ty; }
        }
    };
    if (chunks > 0) {
        issue(0, ty, tx, kc * DG_KC);
        advance();
    }
    const int rd = (wave * 32 + r) * DG_KC, sz = (r >> 1) & 7;   // this lane's dy row; rows 32 apart share the swizzle
    int buf = 0;
    for (int it = 0; it < chunks; ++it) {
        // this chunk has landed (every wave waits for its own requests, then for the others), and every wave is past its
        // reads of the other buffer
        wait_vmcnt<0>();
        __syncthreads();
        if (it + 1 < chunks) {
            issue(buf ^ 1, ty, tx, kc * DG_KC);
            advance();
        }
        const float *cy = &sy[buf][0] + rd;
        const float *cw = &sw[buf][0] + r * DG_KC;
#pragma unroll
        for (int j = 0; j < DG_KC / 4; ++j) {
            const int g = (j ^ sz) * 4;
            const f32x4 yv = *(const f32x4 *)(cy + g);
            const float b0 = h ? yv[1] : yv[0], b1 = h ? yv[3] : yv[2];
            float a0[NT], a1[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const f32x4 wv = *(const f32x4 *)(cw + n * 32 * DG_KC + g);
                a0[n] = h ? wv[1] : wv[0];
                a1[n] = h ? wv[3] : wv[2];
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[n], b0, acc[n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[n], b1, acc[n], 0, 0, 0);
        }
        buf ^= 1;
    }

    // ---- dx.  C/D layout: col = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (cin): float4 per reg >> 2
    const int m = m0 + wave * 32 + r;
    if (m >= Mc) return;
    const int b = m / HcWc, rem = m - b * HcWc;
    const int cyy = rem / Wc, cxx = rem - cyy * Wc;
    const long long pix = ((long long)b * H + 2 * cyy + py) * W + 2 * cxx + px;
    float *dst = A.dx + pix * cin;
    const float *add = A.add ? A.add + pix * cin : nullptr;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ci = n0 + n * 32 + 8 * q + 4 * h;
            if (ci >= cin) continue;
            f32x4 v = {acc[n][4 * q], acc[n][4 * q + 1], acc[n][4 * q + 2], acc[n][4 * q + 3]};
            if (add) {
                const f32x4 a = *(const f32x4 *)(add + ci);
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = v[t] == 0.f ? a[t] : a[t] + v[t];   // an exact zero leaves add's bits
            }
            *(f32x4 *)(dst + ci) = v;
        }
}

struct DgPlan {
    DgAxis ay[2], ax[2];
    int Hc[2], Wc[2];
    long long pixels[4];
};

DgAxis dg_axis(int parity, int pad, int K, int dil) {
    DgAxis a = {};
    for (int k = 0; k < K; ++k) {
        const int t = parity + pad - k * dil;
        if (t & 1) continue;
        a.k[a.n] = k;
        a.off[a.n] = t >> 1;         // t is even: exact for a negative t too
        ++a.n;
    }
    return a;
}

// the checks of one problem and its classes: geometry only
int dg_plan(const ml_conv2d_desc &d, DgPlan &pl) {
    const char *what = "conv2d_dgrad_s2";
    ML_REQUIRE(d.math != ML_MATH_F16S && !d.out_f16, "%s: half tensors are refused (the backward is float32 only)", what);
    ML_REQUIRE(!d.group_cin_step, "%s: grouped / depthwise problems are refused (dense convolutions only)", what);
    ML_REQUIRE(d.cpp_shift == 30, "%s: row-span (image input) problems are refused (dense convolutions only)", what);
    ML_REQUIRE(!d.shuffle2x2, "%s: shuffle2x2 (Conv2DTranspose) problems are refused (dense convolutions only)", what);
    ML_REQUIRE(d.stride == 2, "%s: stride %d: stride 2 only (stride 1 is the forward kernels on transposed weights)", what, d.stride);
    ML_REQUIRE(d.KH >= 1 && d.KH <= DG_MAXK && d.KW >= 1 && d.KW <= DG_MAXK, "%s: kernel %d x %d: at most 5 x 5", what, d.KH, d.KW);
    ML_REQUIRE(d.dil >= 1, "%s: bad dilation", what);
    ML_REQUIRE(d.span > 0 && d.span % 4 == 0, "%s: cin (%d) must be a multiple of 4", what, d.span);
    ML_REQUIRE(d.cout > 0 && d.cout % 4 == 0, "%s: cout (%d) must be a multiple of 4", what, d.cout);
    ML_REQUIRE(d.B > 0 && d.H > 0 && d.W > 0, "%s: bad dims", what);
    ML_REQUIRE(d.pad_t >= 0 && d.pad_l >= 0 && d.pad_t <= (d.KH - 1) * d.dil && d.pad_l <= (d.KW - 1) * d.dil,
               "%s: leading pads (%d, %d) outside the kernel's extent", what, d.pad_t, d.pad_l);
    // the last window starts inside the padded map
    ML_REQUIRE(d.Ho >= 1 && d.Wo >= 1 && 2 * (d.Ho - 1) - d.pad_t < d.H && 2 * (d.Wo - 1) - d.pad_l < d.W,
               "%s: the kernel does not fit the map: %d x %d outputs from a %d x %d input", what, d.Ho, d.Wo, d.H, d.W);
    ML_REQUIRE((long long)d.B * d.H * d.W < (1ll << 31) - DG_BM, "%s: too many pixels", what);
    ML_REQUIRE((long long)d.B * d.Ho * d.Wo * d.cout * 4 < (1ll << 31), "%s: dy must be smaller than 2 GiB", what);
    ML_REQUIRE((long long)d.KH * d.KW * d.span * d.cout * 4 < (1ll << 31), "%s: the kernel must be smaller than 2 GiB", what);
    for (int p = 0; p < 2; ++p) {
        pl.ay[p] = dg_axis(p, d.pad_t, d.KH, d.dil);
        pl.ax[p] = dg_axis(p, d.pad_l, d.KW, d.dil);
        pl.Hc[p] = (d.H + 1 - p) / 2;
        pl.Wc[p] = (d.W + 1 - p) / 2;
    }
    for (int c = 0; c < 4; ++c) pl.pixels[c] = (long long)d.B * pl.Hc[c >> 1] * pl.Wc[c & 1];
    return ML_OK;
}

}  // namespace

extern "C" int ml_conv2d_dgrad_s2_classes(const ml_conv2d_desc *desc, int64_t *pixels, int32_t *ntaps, int32_t *taps) {
    ML_REQUIRE(desc && pixels && ntaps && taps, "conv2d_dgrad_s2_classes: null argument");
    DgPlan pl;
    const int rc = dg_plan(*desc, pl);
    if (rc != ML_OK) return rc;
    for (int c = 0; c < 4; ++c) {
        const DgAxis &ay = pl.ay[c >> 1], &ax = pl.ax[c & 1];
        pixels[c] = pl.pixels[c];
        ntaps[c] = ay.n * ax.n;
        int32_t *t = taps + c * ML_CONV_DGRAD_S2_MAX_TAPS * 4;
        for (int i = 0; i < ay.n; ++i)
            for (int j = 0; j < ax.n; ++j, t += 4) {
                t[0] = ay.k[i]; t[1] = ax.k[j]; t[2] = ay.off[i]; t[3] = ax.off[j];
            }
    }
    return ML_OK;
}

extern "C" int ml_conv2d_dgrad_s2_f32(const ml_conv2d_desc *desc, float *dx, const float *add, void *stream) {
    const char *what = "conv2d_dgrad_s2";
    ML_REQUIRE(desc, "%s: null descriptor", what);
    const ml_conv2d_desc &d = *desc;
    DgPlan pl;
    const int rc = dg_plan(d, pl);
    if (rc != ML_OK) return rc;
    ML_REQUIRE(d.out && d.wgt && dx, "%s: null pointer", what);
    ML_REQUIRE(d.out_cstride == d.cout && d.out_coff == 0 && (d.out_bstride == 0 || d.out_bstride == (long long)d.Ho * d.Wo * d.cout),
               "%s: dy must be a dense [B,Ho,Wo,cout] tensor, not a view", what);
    ML_REQUIRE(ml_aligned16(d.out) && ml_aligned16(d.wgt) && ml_aligned16(dx) && ml_aligned16(add),
               "%s: dy, the kernel, dx and add must be 16-byte aligned", what);
    const long long dy_bytes = (long long)d.B * d.Ho * d.Wo * d.cout * 4, w_bytes = (long long)d.KH * d.KW * d.span * d.cout * 4;
    const long long dx_bytes = (long long)d.B * d.H * d.W * d.span * 4;
    const ml_range r_dy = {d.out, dy_bytes}, r_w = {d.wgt, w_bytes}, r_dx = {dx, dx_bytes};
    ML_REQUIRE(!ml_any_overlap({r_dx}, {r_dy, r_w}), "%s: dx may not overlap dy or the kernel", what);
    ML_REQUIRE(ml_add_or_disjoint(dx, add, dx_bytes), "%s: dx may be add itself, not a shifted view of it", what);
    DgArgs A;
    A.dy = d.out; A.w = d.wgt; A.add = add; A.dx = dx;
    A.B = d.B; A.H = d.H; A.W = d.W; A.Ho = d.Ho; A.Wo = d.Wo; A.cin = d.span; A.cout = d.cout; A.KW = d.KW;
    A.dy_bytes = (int)dy_bytes; A.w_bytes = (int)w_bytes;
    const int nsub = (d.span + 31) / 32, NT = nsub < 4 ? nsub : 4;
    A.ntn = (nsub + NT - 1) / NT;
    long long tiles = 0;
    for (int c = 0; c < 4; ++c) {
        A.first_tile[c] = (int)tiles;
        tiles += (pl.pixels[c] + DG_BM - 1) / DG_BM;
    }
    A.first_tile[4] = (int)tiles;
    ML_REQUIRE(tiles * A.ntn < (1ll << 31), "%s: grid too large", what);
    for (int p = 0; p < 2; ++p) {
        A.Hc[p] = pl.Hc[p]; A.Wc[p] = pl.Wc[p]; A.ay[p] = pl.ay[p]; A.ax[p] = pl.ax[p];
    }
    const dim3 grid((unsigned)(tiles * A.ntn)), block(DG_TPB);
    hipStream_t s = (hipStream_t)stream;
    switch (NT) {
    case 1: hipLaunchKernelGGL(conv_dgrad_s2_kernel<1>, grid, block, 0, s, A); break;
    case 2: hipLaunchKernelGGL(conv_dgrad_s2_kernel<2>, grid, block, 0, s, A); break;
    case 3: hipLaunchKernelGGL(conv_dgrad_s2_kernel<3>, grid, block, 0, s, A); break;
    default: hipLaunchKernelGGL(conv_dgrad_s2_kernel<4>, grid, block, 0, s, A); break;
    }
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}
