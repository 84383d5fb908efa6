// Backward of the mask head's fused tail (deconv_out.hip), fp32: Conv2DTranspose(2x2, s2) + ReLU -> Conv2D 1x1, from the
// gradient dy at the 1x1 conv's PRE-activation and the tape T [M][4][C] (M = R h w input pixels, q = 2a + b the output
// position, C = C_mid) that the forward's tape launch kept.  One pass over T gives
//
//   dT[m,q,c] = T[m,q,c] > 0 ? sum_k dy[pixel(m,q), k] * Wo[c,k] : 0      (the gradient at the transposed conv's pre-activation,
//                                                                          in T's layout; `out` may be T itself)
//   dWo[c,k]  = sum over (m,q) of T[m,q,c] * dy[pixel(m,q), k]
//   dbo[k]    = sum over (m,q) of dy[pixel(m,q), k]
//
// and what is left of the transposed conv is a 1x1 conv with 4 C outputs on dT viewed [R,h,w,4C]: its weight, bias and
// data gradients are conv_grad.hip's and the forward kernels' (DESIGN 7a-train-mask).  dy is read in place in the
// [B, total, 2h, 2w, ncls] tensor with the forward's addressing (out_base / image stride / RoIs per image).
//
// The kernel streams: T is read once, dT written once, dy read once.  Lanes run along channels, 16 bytes each: a block of
// 256 threads is PG pixel groups x CL channel lanes (CL = C / 4 rounded up to a power of two, at most 64; PG = 256 / CL)
// and covers one SLICE of the pixel axis.  A group takes pixels m = first + g, first + g + PG, ...; per pixel the index
// arithmetic runs once and the four rows q = 0..3 (4 C consecutive floats of T) are in flight together.  A lane keeps
// the rows of Wo for its four channels and the dWo sums of those channels in registers (template over cp = the power of
// two >= ncls); a row's ncls dy values are the same address for every lane of the row (one broadcast load each, the whole
// wave at C = 256).
// A row whose dy is all zero -- mask_loss's gradient is non-zero in one class channel of the selected RoIs only -- loads no
// T and stores zeros: the sums would have added T * 0, so the bits are the same for every finite T.
//
// No float atomics.  The slices are ceil(M / 512) pixels rounded up to a multiple of 32, at least 128: a function of the
// problem's pixel count alone.  A group adds its pixels in ascending order (q ascending inside a pixel); the block adds
// its groups in ascending order through LDS and writes the partial of its slice, [ncls][C] fp32 + [ncls] fp64 (the dy sums
// are kept in fp64 from the first addition: they cost ncls additions per row and make dbias the rounded exact sum); the
// finish kernel adds an element's partials in ascending slice order in fp64, rounds once and writes dkernel [1,1,C,ncls]
// (the Keras layout) and dbias [ncls].  Every element of a partial that the finish kernel reads is written by its block.
//
// ml_deconv2x2_grad_relayout_f32: the transposed conv's weight gradient comes back from conv_grad.hip as the 1x1 view's
// [1,1,cin,4C] and [4C]; the layer's own shapes are kernel [2,2,C,cin] (a transposition, no arithmetic) and bias [C] =
// ((b[0C + c] + b[1C + c]) + b[2C + c]) + b[3C + c]: three fp32 additions in the order q = 0..3.
#include "slice_sum.h"

namespace {

constexpr int TG_TPB = 256;
constexpr int TG_ROUND = 32;           // slice lengths are multiples of this
constexpr int TG_SLICE_MIN = 128;
constexpr int TG_SLICE_DIV = 512;      // at most this many slices per problem

struct TgProb {
    const float *T, *dy, *wo;
    float *out, *part, *dk, *db;
    int M, hw, w, n_l, C;
    float r_hw, r_w, r_nl;
    long long img_stride, base;        // dy elements: between images / of this level's first RoI in image 0
    int cl_shift, sp, slices, first_block, first_fblock;
};
struct TgArgs {
    TgProb p[ML_DECONV_OUT_MAX_PROBLEMS];
    int n, ncls;
};

__device__ __forceinline__ f32x4 tg_ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }

// n / d for 0 <= n < 2^24 (exact in float), d >= 1: one multiply and a two-sided correction (as deconv_out.hip)
__device__ __forceinline__ int tg_div(int n, int d, float rd) {
    int q = (int)((float)n * rd);
    if (q * d > n) --q;
    if ((q + 1) * d <= n) ++q;
    return q;
}

template <int CP>
__global__ void __launch_bounds__(TG_TPB) tail_grad_kernel(const TgArgs A) {
    constexpr int KCH = CP < 8 ? CP : 8;              // columns per pass of the block's sum through LDS
    constexpr int UQ = CP <= 8 ? 4 : (CP == 16 ? 2 : 1);   // rows of a pixel in flight together
    __shared__ f32x4 sm[KCH][TG_TPB];
    double *smb = reinterpret_cast<double *>(&sm[0][0]);      // [KCH][PG]: the dy sums, after the dWo sums have left
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.p[pi + 1].first_block) ++pi;
    const TgProb &p = A.p[pi];
    const int slice = blockIdx.x - p.first_block;
    const int tid = threadIdx.x;
    const int CL = 1 << p.cl_shift, PG = TG_TPB >> p.cl_shift;
    const int cl = tid & (CL - 1), grp = tid >> p.cl_shift;
    const int C = p.C, ncls = A.ncls;
    const int c = cl * 4;
    const bool active = c < C;
    const int m_begin = slice * p.sp, m_end = min(m_begin + p.sp, p.M);
    // the slice's rows of T and dT: offsets inside a slice fit 32 bits (the launcher checks)
    const float *Tb = p.T + (long long)m_begin * 4 * C + c;
    float *Ob = p.out + (long long)m_begin * 4 * C + c;

    f32x4 wo4[CP], accW[CP];
    double accB[CP];                       // dbo is summed in fp64 all the way: its partials are doubles, rounded once at the end
#pragma unroll
    for (int k = 0; k < CP; ++k) {
        wo4[k] = accW[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        accB[k] = 0.0;
        if (active && k < ncls) {
            const float *w = p.wo + (long long)c * ncls + k;
            wo4[k] = (f32x4){w[0], w[ncls], w[2 * ncls], w[3 * ncls]};
        }
    }
    const int per_roi = 4 * p.hw * ncls;
    for (int mi = m_begin + grp; mi < m_end; mi += PG) {
        const int roi = tg_div(mi, p.hw, p.r_hw), rem = mi - roi * p.hw;
        const int y = tg_div(rem, p.w, p.r_w), x = rem - y * p.w;
        const int img = tg_div(roi, p.n_l, p.r_nl), j = roi - img * p.n_l;
        const float *dy0 = p.dy + ((long long)img * p.img_stride + p.base + (long long)j * per_roi +
                                   (long long)((2 * y * 2 * p.w + 2 * x) * ncls));
        const int row0 = (mi - m_begin) * 4 * C;
#pragma unroll
        for (int q0 = 0; q0 < 4; q0 += UQ) {
            float g[UQ][CP];
            bool nz[UQ];
            f32x4 t[UQ];
#pragma unroll
            for (int u = 0; u < UQ; ++u) {
                const int q = q0 + u;
                const float *dyp = dy0 + ((q >> 1) * 2 * p.w + (q & 1)) * ncls;
                nz[u] = false;
#pragma unroll
                for (int k = 0; k < CP; ++k) {
                    g[u][k] = k < ncls ? dyp[k] : 0.f;
                    nz[u] = nz[u] || g[u][k] != 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < UQ; ++u) {
                t[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (nz[u] && active) t[u] = tg_ld4(Tb + row0 + (q0 + u) * C);
            }
#pragma unroll
            for (int u = 0; u < UQ; ++u) {
                f32x4 d = {0.f, 0.f, 0.f, 0.f};
                if (nz[u]) {
#pragma unroll
                    for (int k = 0; k < CP; ++k) {
                        d += g[u][k] * wo4[k];
                        accW[k] += t[u] * g[u][k];
                        accB[k] += (double)g[u][k];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = t[u][e] > 0.f ? d[e] : 0.f;
                }
                if (active) *reinterpret_cast<f32x4 *>(Ob + row0 + (q0 + u) * C) = d;
            }
        }
    }

    // the block's PG groups, added in ascending group order, KCH columns per pass
    float *part = p.part + (long long)slice * ((long long)ncls * C + ((2 * ncls + 3) & ~3));
    double *part_b = reinterpret_cast<double *>(part + (long long)ncls * C);
#pragma unroll
    for (int k0 = 0; k0 < CP; k0 += KCH) {
        if (k0 >= ncls) break;
        if (k0) __syncthreads();
#pragma unroll
        for (int k = 0; k < KCH; ++k) sm[k][tid] = accW[k0 + k];
        __syncthreads();
        if (grp == 0 && active) {
#pragma unroll
            for (int k = 0; k < KCH; ++k) {
                if (k0 + k >= ncls) break;
                f32x4 v = sm[k][tid];
                for (int r = 1; r < PG; ++r) v += sm[k][tid + (r << p.cl_shift)];
                *reinterpret_cast<f32x4 *>(part + (long long)(k0 + k) * C + c) = v;
            }
        }
        __syncthreads();
        if (cl == 0) {                                    // dy is the same in every lane of a group: lane 0 speaks for it
#pragma unroll
            for (int k = 0; k < KCH; ++k) smb[k * PG + grp] = accB[k0 + k];
        }
        __syncthreads();
        if (tid < KCH && k0 + tid < ncls) {
            double v = smb[tid * PG];
            for (int r = 1; r < PG; ++r) v += smb[tid * PG + r];
            part_b[k0 + tid] = v;
        }
    }
}

// element i of a problem: i < C ncls -> dkernel[c][k] (i = c ncls + k), else dbias[i - C ncls]
__global__ void __launch_bounds__(TG_TPB) tail_grad_finish_kernel(const TgArgs A) {
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.p[pi + 1].first_fblock) ++pi;
    const TgProb &p = A.p[pi];
    const int i = (blockIdx.x - p.first_fblock) * TG_TPB + threadIdx.x;
    const int ncls = A.ncls, nk = p.C * ncls;
    if (i >= nk + ncls) return;
    const long long pitch = (long long)nk + ((2 * ncls + 3) & ~3);
    if (i >= nk) {                                        // dbias: the slices' fp64 sums, rounded once
        const double *src = reinterpret_cast<const double *>(p.part + nk) + (i - nk);
        double t = 0.0;
        for (int s = 0; s < p.slices; ++s) t += src[(long long)s * (pitch / 2)];
        p.db[i - nk] = (float)t;
        return;
    }
    p.dk[i] = (float)ml_sum_slices_f64(p.part + (long long)(i % ncls) * p.C + i / ncls, pitch, p.slices);
}

// dk1 [cin][4][C] -> dkernel [4][C][cin]; db4 [4][C] -> dbias [C]
__global__ void __launch_bounds__(TG_TPB) deconv_grad_relayout_kernel(const float *__restrict__ dk1, const float *__restrict__ db4,
                                                                       float *__restrict__ dkernel, float *__restrict__ dbias,
                                                                       int cin, int C4) {
    const long long i = (long long)blockIdx.x * TG_TPB + threadIdx.x;
    const long long nk = (long long)cin * C4;
    if (i < nk) {
        const int ci = (int)(i % cin);
        const long long qc = i / cin;
        dkernel[i] = dk1[(long long)ci * C4 + qc];
    } else if (i < nk + C4 / 4 && db4 && dbias) {
        const int c = (int)(i - nk), C = C4 / 4;
        dbias[c] = ((db4[c] + db4[C + c]) + db4[2 * C + c]) + db4[3 * C + c];
    }
}

struct TgPlan {
    int slices, sp, cl_shift;
    long long bytes;
};

int tg_plan(const ml_deconv_out_grad_problem &d, int ncls, TgPlan &pl) {
    const char *what = "deconv2x2_out1x1_grad";
    ML_REQUIRE(ncls >= 1 && ncls <= 32, "%s: 1..32 classes (got %d)", what, ncls);
    ML_REQUIRE(d.c_mid >= 4 && d.c_mid % 4 == 0 && d.c_mid <= 256, "%s: C_mid = %d must be a multiple of 4 (16-byte accesses), at "
               "most 256", what, d.c_mid);
    ML_REQUIRE(d.M >= 1 && d.M < (1ll << 24), "%s: 1 <= input pixels < 2^24 per problem (got %lld)", what, (long long)d.M);
    ML_REQUIRE(d.w >= 1 && d.hw >= d.w && d.hw % d.w == 0 && d.rois_per_image >= 1 && d.M % d.hw == 0 &&
                   (d.M / d.hw) % d.rois_per_image == 0,
               "%s: pixels (%lld) must be whole maps of %d (width %d) for whole images of %d RoIs", what, (long long)d.M, d.hw, d.w,
               d.rois_per_image);
    const long long sp = ml_slice_pixels(d.M, TG_SLICE_DIV, TG_ROUND, TG_SLICE_MIN, 0);
    pl.sp = (int)sp;
    pl.slices = (int)((d.M + sp - 1) / sp);
    // a slice's rows of T: 32-bit byte offsets inside it
    ML_REQUIRE(sp * 4 * d.c_mid * 4 < (1ll << 31), "%s: a slice of %lld pixels x 4 x %d channels exceeds 32-bit byte offsets", what,
               sp, d.c_mid);
    ML_REQUIRE((long long)d.hw * 4 * ncls < (1ll << 31), "%s: a RoI's output map exceeds 32-bit offsets", what);
    pl.cl_shift = 0;
    while ((1 << pl.cl_shift) < d.c_mid / 4) ++pl.cl_shift;
    pl.bytes = ml_align256((long long)pl.slices * ((long long)ncls * d.c_mid + ((2 * ncls + 3) & ~3)) * 4);
    return ML_OK;
}

template <int CP>
void tg_launch(const TgArgs &A, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(tail_grad_kernel<CP>, dim3(blocks), dim3(TG_TPB), 0, s, A);
}

}  // namespace

extern "C" int ml_deconv2x2_out1x1_grad_plan(const ml_deconv_out_grad_problem *prob, int32_t ncls, int32_t *slices,
                                             int32_t *slice_pixels, int64_t *workspace_bytes) {
    ML_REQUIRE(prob, "deconv2x2_out1x1_grad_plan: null problem");
    TgPlan pl;
    const int rc = tg_plan(*prob, ncls, pl);
    if (rc != ML_OK) return rc;
    ml_plan_out(pl.slices, pl.sp, pl.bytes, slices, slice_pixels, workspace_bytes);
    return ML_OK;
}

extern "C" int ml_deconv2x2_out1x1_grad_f32(const ml_deconv_out_grad_problem *probs, int32_t nprob, int32_t ncls, void *workspace,
                                            int64_t workspace_bytes, void *stream) {
    const char *what = "deconv2x2_out1x1_grad";
    ML_REQUIRE(probs && nprob >= 1 && nprob <= ML_DECONV_OUT_MAX_PROBLEMS, "%s: 1..%d problems per launch", what, ML_DECONV_OUT_MAX_PROBLEMS);
    ML_REQUIRE(workspace && (((uintptr_t)workspace) & 255) == 0, "%s: needs a 256-byte aligned workspace", what);
    TgArgs A;
    long long used = 0, blocks = 0, fblocks = 0;
    ml_range writes[ML_DECONV_OUT_MAX_PROBLEMS][3];
    for (int i = 0; i < nprob; ++i) {
        const ml_deconv_out_grad_problem &d = probs[i];
        TgPlan pl;
        const int rc = tg_plan(d, ncls, pl);
        if (rc != ML_OK) return rc;
        ML_REQUIRE(d.dy && d.t && d.wo && d.out && d.dkernel && d.dbias, "%s: problem %d: null pointer", what, i);
        ML_REQUIRE(ml_aligned16(d.t) && ml_aligned16(d.out), "%s: problem %d: T and out must be 16-byte aligned", what, i);
        ML_REQUIRE((((uintptr_t)d.dy | (uintptr_t)d.wo | (uintptr_t)d.dkernel | (uintptr_t)d.dbias) & 3) == 0,
                   "%s: problem %d: 4-byte alignment", what, i);
        ML_REQUIRE(d.dy_base >= 0 && d.dy_image_stride >= 0, "%s: problem %d: negative dy offsets", what, i);
        const long long t_bytes = d.M * 4 * d.c_mid * 4, dk_bytes = (long long)d.c_mid * ncls * 4, db_bytes = (long long)ncls * 4;
        const long long images = d.M / d.hw / d.rois_per_image;
        const float *dy_lo = d.dy + d.dy_base;
        const long long dy_bytes = ((images - 1) * d.dy_image_stride + (long long)d.rois_per_image * 4 * d.hw * ncls) * 4;
        ML_REQUIRE(ml_add_or_disjoint(d.out, d.t, t_bytes), "%s: problem %d: out may be T itself, not a shifted "
                   "view of it", what, i);
        const ml_range r_t = {d.t, t_bytes}, r_dy = {dy_lo, dy_bytes}, r_wo = {d.wo, dk_bytes}, r_ws = {workspace, workspace_bytes};
        writes[i][0] = {d.out, t_bytes}; writes[i][1] = {d.dkernel, dk_bytes}; writes[i][2] = {d.dbias, db_bytes};
        ML_REQUIRE(!ml_any_overlap({writes[i][0]}, {r_dy, r_wo}), "%s: problem %d: out may not overlap dy or the 1x1 kernel", what, i);
        ML_REQUIRE(!ml_any_overlap({writes[i][1], writes[i][2]}, {r_t, r_dy, r_wo, writes[i][0], r_ws}),
                   "%s: problem %d: dkernel / dbias may not overlap T, dy, the 1x1 kernel, out or the workspace", what, i);
        ML_REQUIRE(!ml_ranges_overlap(d.dkernel, dk_bytes, d.dbias, db_bytes), "%s: problem %d: dkernel overlaps dbias", what, i);
        ML_REQUIRE(!ml_any_overlap({writes[i][0], r_t}, {r_ws}), "%s: problem %d: T / out overlap the workspace", what, i);
        for (int j = 0; j < i; ++j)
            ML_REQUIRE(!ml_any_overlap(writes[i], 3, writes[j], 3), "%s: problems %d and %d write the same tensor", what, j, i);
        for (int j = 0; j < nprob; ++j)
            if (j != i)
                ML_REQUIRE(!ml_ranges_overlap(d.out, t_bytes, probs[j].t, probs[j].M * 4 * probs[j].c_mid * 4),
                           "%s: problem %d writes the T of problem %d", what, i, j);
        TgProb &p = A.p[i];
        p.T = d.t; p.dy = d.dy; p.wo = d.wo; p.out = d.out; p.dk = d.dkernel; p.db = d.dbias;
        p.part = ml_carve_partials(what, i, workspace, workspace_bytes, used, pl.bytes);
        if (!p.part) return ML_E_BADARG;
        p.M = (int)d.M; p.hw = d.hw; p.w = d.w; p.n_l = d.rois_per_image; p.C = d.c_mid;
        p.r_hw = 1.f / (float)d.hw; p.r_w = 1.f / (float)d.w; p.r_nl = 1.f / (float)d.rois_per_image;
        p.img_stride = d.dy_image_stride; p.base = d.dy_base;
        p.cl_shift = pl.cl_shift; p.sp = pl.sp; p.slices = pl.slices;
        p.first_block = (int)blocks; p.first_fblock = (int)fblocks;
        blocks += pl.slices;
        fblocks += ((long long)d.c_mid * ncls + ncls + TG_TPB - 1) / TG_TPB;
    }
    for (int i = nprob; i < ML_DECONV_OUT_MAX_PROBLEMS; ++i) A.p[i] = A.p[0];
    A.n = nprob; A.ncls = ncls;
    hipStream_t s = (hipStream_t)stream;
    int cp = 1;
    while (cp < ncls) cp *= 2;
    switch (cp) {
        case 1: tg_launch<1>(A, (unsigned)blocks, s); break;
        case 2: tg_launch<2>(A, (unsigned)blocks, s); break;
        case 4: tg_launch<4>(A, (unsigned)blocks, s); break;
        case 8: tg_launch<8>(A, (unsigned)blocks, s); break;
        case 16: tg_launch<16>(A, (unsigned)blocks, s); break;
        default: tg_launch<32>(A, (unsigned)blocks, s); break;
    }
    hipLaunchKernelGGL(tail_grad_finish_kernel, dim3((unsigned)fblocks), dim3(TG_TPB), 0, s, A);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_deconv2x2_grad_relayout_f32(const float *dk1x1, const float *db4, float *dkernel, float *dbias, int32_t cin,
                                              int32_t c_mid, void *stream) {
    const char *what = "deconv2x2_grad_relayout";
    ML_REQUIRE(dk1x1 && dkernel && cin >= 1 && c_mid >= 1, "%s: bad arguments", what);
    ML_REQUIRE((db4 == nullptr) == (dbias == nullptr), "%s: give both bias tensors or neither", what);
    const long long nk = (long long)cin * 4 * c_mid, n = nk + c_mid;
    ML_REQUIRE(n < (1ll << 31), "%s: too large", what);
    ML_REQUIRE(!ml_any_overlap({{dkernel, nk * 4}, {dbias, c_mid * 4ll}}, {{dk1x1, nk * 4}, {db4, c_mid * 16ll}}) &&
               !ml_ranges_overlap(dkernel, nk * 4, dbias, c_mid * 4ll), "%s: the tensors may not overlap", what);
    hipLaunchKernelGGL(deconv_grad_relayout_kernel, dim3((unsigned)((n + TG_TPB - 1) / TG_TPB)), dim3(TG_TPB), 0, (hipStream_t)stream,
                       dk1x1, db4, dkernel, dbias, cin, 4 * c_mid);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}
