// BatchNormalization in Keras's training mode, forward and backward, and its inference arithmetic on device-resident moving
// statistics: NHWC fp32, the reduction runs over all N = B*H*W pixels of a channel c (include/masklab_hip.h,
// "BatchNormalization, training"):
//   mean_b = sum x / N,  var_b = sum (x - mean_b)^2 / N (biased),  r = 1/sqrt(var_b + eps)
//   scale = gamma * r,  shift = beta - mean_b * scale          (fp64, rounded once to float)
//   y = x * scale + shift [+ residual], max(., 0) with a fused ReLU
//   moving <- moving - (moving - f32(stat)) * f32(1 - momentum),  stat = mean_b resp. var_u = var_b * N / (N - 1);
//            three float32 operations, each rounded (this file is built with -ffp-contract=off)
//   g = dy * [y > 0] with a fused ReLU (strict, on the forward's own y), else dy;  xhat = (x - mean_b) * r
//   dbeta = sum g,  dgamma = sum g * xhat,  dx = scale * (g - dbeta/N - xhat * dgamma/N),  d_residual = g
// Lanes run along the channels: a block owns a tile of BN_TILE = 64 channels (16 lanes of one 16-byte access each) and a slice
// of the pixel axis, its 16 rows of lanes take every 16th pixel of the slice.  The slice plan (bn_plan) is a function of
// (N, C) alone.  Passes (HBM-bound):
//   statistics       block (slice, tile) -> record (sum x, sum x^2) per channel               x read
//   finish           block (tile) folds the records -> saved (mean_b, r), scale, shift, batch_mean, batch_var, moving update;
//                    its inference arm derives scale / shift from the moving statistics, no records
//   apply            y                                                                       x [residual] read, y written
//   backward reduce  block (slice, tile) -> record (sum g, sum g * x)                         x dy [y] read
//   backward finish  dgamma = r * (sum g x - mean_b * sum g), dbeta, and the coefficients of dx
//   backward apply   dx = scale * g - c0 - c1 * (x - mean_b)  [d_residual = g]                x dy [y] read, dx written
// Sums: a thread adds into fp64 running sums (the products x*x and g*x are exact in fp64, so sum x^2 / N - mean_b^2 loses
// nothing that matters even with a channel mean 40 standard deviations out); the 16 rows of a block are added in row order
// through LDS; the records of a channel are added in ascending slice order (four contiguous runs, then the four in order).
// No atomics, no host read: two launches give the same bits, whatever outputs and workspace held, and a captured forward +
// backward replays.
#include "common.h"
#include "ranges.h"

namespace {

constexpr int BN_TPB = 256;
constexpr int BN_TILE = 64;             // channels per block: 16 lanes x one 16-byte access
constexpr int BN_LANES = BN_TILE / 4;
constexpr int BN_ROWS = BN_TPB / BN_LANES;
constexpr int BN_MIN_SLICE = 64;        // pixels: four sweeps of a block at least
constexpr int BN_MAX_SLICES = 1024;
constexpr int BN_PARTS = BN_TPB / BN_TILE;

struct BnPlan {
    int tiles, S;
    long long slice, rec_bytes, coef_bytes;
};

constexpr long long bn_align(long long b) { return (b + 255) / 256 * 256; }

// The pixel axis in S slices of `slice` pixels (a multiple of the 16 rows; the last one ragged): about 2048 blocks on the chip,
// BN_MIN_SLICE pixels per block at least, BN_MAX_SLICES slices at most.  A function of (N, C) alone.
static BnPlan bn_plan(long long N, int C) {
    BnPlan p;
    p.tiles = (C + BN_TILE - 1) / BN_TILE;
    long long want = (2048 + p.tiles - 1) / p.tiles;
    if (want > BN_MAX_SLICES) want = BN_MAX_SLICES;
    long long slice = (N + want - 1) / want;
    if (slice < BN_MIN_SLICE) slice = BN_MIN_SLICE;
    p.slice = (slice + BN_ROWS - 1) / BN_ROWS * BN_ROWS;
    p.S = (int)((N + p.slice - 1) / p.slice);
    p.rec_bytes = bn_align((long long)p.tiles * p.S * 2 * BN_TILE * (long long)sizeof(double));
    p.coef_bytes = bn_align(4ll * p.tiles * BN_TILE * (long long)sizeof(float));
    return p;
}

struct BnGeom {
    long long N, slice;
    int C, S, Cp;                       // Cp = tiles * BN_TILE: the stride of the coefficient vectors
};

// The block's 16 rows of (a, b) per channel, added in row order -> rec[0][ch] = sum a, rec[1][ch] = sum b.  All 64 channels of
// the tile are written (lanes past C hold zeros): a record has no stale part.
__device__ __forceinline__ void bn_store_record(const double (&a)[4], const double (&b)[4], double *rec,
                                                double (*sh)[BN_TPB * 4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[0][t * 4 + e] = a[e]; sh[1][t * 4 + e] = b[e]; }
    __syncthreads();
    if (t < 2 * BN_TILE) {
        const int k = t / BN_TILE, ch = t % BN_TILE;          // thread (row, lane), element e sits at row * 64 + lane * 4 + e
        double s = 0;
#pragma unroll
        for (int r = 0; r < BN_ROWS; ++r) s += sh[k][r * BN_TILE + ch];
        rec[k * BN_TILE + ch] = s;
    }
}

// The S records of the tile's channel ch = t % 64, in ascending order: part t / 64 adds a contiguous quarter, thread ch then
// adds the four parts in order.  -> (A, B) in the threads t < 64.
__device__ __forceinline__ void bn_fold_records(const double *rec_tile, int S, double &A, double &B, double (*sh)[BN_TPB]) {
    const int t = threadIdx.x, ch = t % BN_TILE, q = t / BN_TILE;
    const int per = (S + BN_PARTS - 1) / BN_PARTS;
    const int s0 = q * per, s1 = min(S, s0 + per);
    double a = 0, b = 0;
    for (int s = s0; s < s1; ++s) {
        a += rec_tile[(long long)s * 2 * BN_TILE + ch];
        b += rec_tile[(long long)s * 2 * BN_TILE + BN_TILE + ch];
    }
    sh[0][t] = a;
    sh[1][t] = b;
    __syncthreads();
    A = B = 0;
    if (t < BN_TILE) {
#pragma unroll
        for (int p = 0; p < BN_PARTS; ++p) { A += sh[0][p * BN_TILE + ch]; B += sh[1][p * BN_TILE + ch]; }
    }
}

// ---- statistics: block (slice, tile) -> record (sum x, sum x^2)
__global__ void __launch_bounds__(BN_TPB)
bn_stats_kernel(const float *__restrict__ x, double *__restrict__ rec, const BnGeom G) {
    __shared__ double sh[2][BN_TPB * 4];
    const int s = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x % BN_LANES, row = threadIdx.x / BN_LANES;
    const int c = tile * BN_TILE + lane * 4;
    double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    if (c < G.C) {
        const long long lo = (long long)s * G.slice, hi = min(lo + G.slice, G.N);
        const float *p = x + c;
#pragma unroll 4
        for (long long i = lo + row; i < hi; i += BN_ROWS) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(p + i * G.C);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[e];
                a[e] += d;
                b[e] = fma(d, d, b[e]);
            }
        }
    }
    bn_store_record(a, b, rec + ((long long)tile * G.S + s) * 2 * BN_TILE, sh);
}

// ---- finish: block (tile).  coef: scale at [0][c], shift at [1][c] (stride Cp).
struct BnFinish {
    const double *rec;
    const float *gamma, *beta;
    float *moving_mean, *moving_var;        // training: updated in place, or NULL; inference: read
    double *saved;                          // [C][2]: mean_b, r
    float *coef, *batch_mean, *batch_var;
    float eps, one_minus_momentum;
    int infer;
};

__global__ void __launch_bounds__(BN_TPB)
bn_finish_kernel(const BnFinish A, const BnGeom G) {
    __shared__ double sh[2][BN_TPB];
    const int tile = blockIdx.x, t = threadIdx.x, c = tile * BN_TILE + t;
    double mean, r;
    if (A.infer) {
        if (t >= BN_TILE || c >= G.C) return;
        mean = (double)A.moving_mean[c];
        r = 1.0 / sqrt((double)A.moving_var[c] + (double)A.eps);
    } else {
        double sum, sq;
        bn_fold_records(A.rec + (long long)tile * G.S * 2 * BN_TILE, G.S, sum, sq, sh);
        if (t >= BN_TILE || c >= G.C) return;
        const double n = (double)G.N;
        mean = sum / n;
        double var = sq / n - mean * mean;
        if (var < 0) var = 0;
        r = 1.0 / sqrt(var + (double)A.eps);
        const float bm = (float)mean, bv = (float)(var * (n / (n - 1.0)));
        A.saved[c * 2 + 0] = mean;
        A.saved[c * 2 + 1] = r;
        A.batch_mean[c] = bm;
        A.batch_var[c] = bv;
        if (A.moving_mean) {                 // three float32 operations each, as written (no contraction in this file)
            const float m = A.moving_mean[c], v = A.moving_var[c];
            const float dm = m - bm, dv = v - bv;
            const float um = dm * A.one_minus_momentum, uv = dv * A.one_minus_momentum;
            A.moving_mean[c] = m - um;
            A.moving_var[c] = v - uv;
        }
    }
    const double scale = (A.gamma ? (double)A.gamma[c] : 1.0) * r;
    const float scale_f = (float)scale;
    A.coef[c] = scale_f;
    A.coef[G.Cp + c] = (float)((A.beta ? (double)A.beta[c] : 0.0) - mean * scale);
}

// ---- apply: block (slice, tile) writes its part of y.  Index i is read and written by the same thread: y may be x.
__global__ void __launch_bounds__(BN_TPB)
bn_apply_kernel(const float *x, const float *residual, float *y, const float *__restrict__ coef, const BnGeom G, const int relu) {
    const int s = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x % BN_LANES, row = threadIdx.x / BN_LANES;
    const int c = tile * BN_TILE + lane * 4;
    if (c >= G.C) return;
    const f32x4 sc = *reinterpret_cast<const f32x4 *>(coef + c), sf = *reinterpret_cast<const f32x4 *>(coef + G.Cp + c);
    const long long lo = (long long)s * G.slice, hi = min(lo + G.slice, G.N);
#pragma unroll 4
    for (long long i = lo + row; i < hi; i += BN_ROWS) {
        const long long at = i * G.C + c;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(x + at);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(v[e], sc[e], sf[e]);
        if (residual) o += *reinterpret_cast<const f32x4 *>(residual + at);
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
        }
        *reinterpret_cast<f32x4 *>(y + at) = o;
    }
}

// the gradient behind the forward's fused ReLU: strict, decided by the forward's own y
__device__ __forceinline__ f32x4 bn_g(const f32x4 dy, const float *y, long long at) {
    if (!y) return dy;
    const f32x4 yv = *reinterpret_cast<const f32x4 *>(y + at);
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = yv[e] > 0.f ? dy[e] : 0.f;
    return g;
}

// ---- backward reduce: block (slice, tile) -> record (sum g, sum g * x).  y: NULL without a fused ReLU.
__global__ void __launch_bounds__(BN_TPB)
bn_grad_reduce_kernel(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ y,
                      double *__restrict__ rec, const BnGeom G) {
    __shared__ double sh[2][BN_TPB * 4];
    const int s = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x % BN_LANES, row = threadIdx.x / BN_LANES;
    const int c = tile * BN_TILE + lane * 4;
    double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    if (c < G.C) {
        const long long lo = (long long)s * G.slice, hi = min(lo + G.slice, G.N);
#pragma unroll 2
        for (long long i = lo + row; i < hi; i += BN_ROWS) {
            const long long at = i * G.C + c;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(x + at);
            const f32x4 g = bn_g(*reinterpret_cast<const f32x4 *>(dy + at), y, at);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)g[e];
                a[e] += d;
                b[e] = fma(d, (double)v[e], b[e]);
            }
        }
    }
    bn_store_record(a, b, rec + ((long long)tile * G.S + s) * 2 * BN_TILE, sh);
}

// ---- backward finish: block (tile).  coef: scale, c0 = scale * dbeta / N, c1 = scale * r * dgamma / N, f32(mean_b) (stride Cp)
__global__ void __launch_bounds__(BN_TPB)
bn_grad_finish_kernel(const double *__restrict__ rec, const double *__restrict__ saved, const float *__restrict__ gamma,
                      float *__restrict__ dgamma, float *__restrict__ dbeta, float *__restrict__ coef, const BnGeom G) {
    __shared__ double sh[2][BN_TPB];
    const int tile = blockIdx.x, t = threadIdx.x, c = tile * BN_TILE + t;
    double sg, sgx;
    bn_fold_records(rec + (long long)tile * G.S * 2 * BN_TILE, G.S, sg, sgx, sh);
    if (t >= BN_TILE || c >= G.C) return;
    const double mean = saved[c * 2 + 0], r = saved[c * 2 + 1], n = (double)G.N;
    const double dg = r * (sgx - mean * sg);
    const double scale = (double)(float)((gamma ? (double)gamma[c] : 1.0) * r);          // the forward's float32 scale
    if (dbeta) dbeta[c] = (float)sg;
    if (dgamma) dgamma[c] = (float)dg;
    coef[c] = (float)scale;
    coef[G.Cp + c] = (float)(scale * (sg / n));
    coef[2 * G.Cp + c] = (float)(scale * r * (dg / n));
    coef[3 * G.Cp + c] = (float)mean;
}

// ---- backward apply: block (slice, tile) writes its part of dx (and of d_residual).  Index i is read and written by the same
// thread: dx, or else d_residual, may be dy.
__global__ void __launch_bounds__(BN_TPB)
bn_grad_apply_kernel(const float *x, const float *dy, const float *y, float *dx, float *d_residual,
                     const float *__restrict__ coef, const BnGeom G) {
    const int s = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x % BN_LANES, row = threadIdx.x / BN_LANES;
    const int c = tile * BN_TILE + lane * 4;
    if (c >= G.C) return;
    const f32x4 sc = *reinterpret_cast<const f32x4 *>(coef + c), c0 = *reinterpret_cast<const f32x4 *>(coef + G.Cp + c),
                c1 = *reinterpret_cast<const f32x4 *>(coef + 2 * G.Cp + c), mu = *reinterpret_cast<const f32x4 *>(coef + 3 * G.Cp + c);
    const long long lo = (long long)s * G.slice, hi = min(lo + G.slice, G.N);
#pragma unroll 2
    for (long long i = lo + row; i < hi; i += BN_ROWS) {
        const long long at = i * G.C + c;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(x + at);
        const f32x4 g = bn_g(*reinterpret_cast<const f32x4 *>(dy + at), y, at);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(sc[e], g[e], -c0[e]) - c1[e] * (v[e] - mu[e]);
        *reinterpret_cast<f32x4 *>(dx + at) = o;
        if (d_residual) *reinterpret_cast<f32x4 *>(d_residual + at) = g;
    }
}

// ------------------------------------------------------------------ host
static int bn_geometry(const char *what, int64_t N, int32_t C, bool training, BnPlan &plan, BnGeom &G) {
    ML_REQUIRE(C > 0 && C % 4 == 0 && C <= (1 << 20),
               "%s: C (%d) must be a positive multiple of 4, at most 2^20: lanes run along the channels with 16-byte accesses", what, C);
    ML_REQUIRE(N >= 1 && N <= (1ll << 40) / C, "%s: N (%lld pixels per channel) must be positive, N*C at most 2^40", what, (long long)N);
    ML_REQUIRE(!training || N >= 2, "%s: N (%lld pixels per channel) must be at least 2: the moving variance takes var_b*N/(N-1)",
               what, (long long)N);
    plan = bn_plan(N, C);
    G.N = N; G.slice = plan.slice; G.C = C; G.S = plan.S; G.Cp = plan.tiles * BN_TILE;
    return ML_OK;
}

static int bn_workspace(const char *what, const BnPlan &plan, void *workspace, int64_t workspace_bytes) {
    ML_REQUIRE(workspace && ml_aligned16(workspace), "%s: workspace must be a 16-byte aligned pointer", what);
    ML_REQUIRE(workspace_bytes >= plan.rec_bytes + plan.coef_bytes, "%s: workspace too small (%lld bytes given, %lld needed)", what,
               (long long)workspace_bytes, plan.rec_bytes + plan.coef_bytes);
    return ML_OK;
}

#define BN_REQUIRE_MAP(p, name) ML_REQUIRE((p) && ml_aligned16(p), "%s: %s must be a 16-byte aligned pointer", what, name)
#define BN_REQUIRE_VEC(p, name) ML_REQUIRE(p, "%s: %s is a null pointer", what, name)

// the forward's x / residual / y ranges and its apply launch (training and inference)
static int bn_check_forward_maps(const char *what, const float *x, const float *residual, float *y, long long bytes) {
    BN_REQUIRE_MAP(x, "x");
    BN_REQUIRE_MAP(y, "y");
    ML_REQUIRE(!residual || ml_aligned16(residual), "%s: residual must be a 16-byte aligned pointer", what);
    ML_REQUIRE(ml_add_or_disjoint(y, x, bytes), "%s: y may be x itself (in place), not a shifted view of it", what);
    ML_REQUIRE(!ml_ranges_overlap(y, bytes, residual, bytes), "%s: y may not alias residual", what);
    return ML_OK;
}

}  // namespace

extern "C" int ml_batchnorm_plan(int64_t N, int32_t C, int32_t *slices, int64_t *pixels_per_slice, int64_t *bytes) {
    const char *what = "batchnorm_plan";
    BnPlan plan;
    BnGeom G;
    if (int rc = bn_geometry(what, N, C, false, plan, G)) return rc;
    if (slices) *slices = plan.S;
    if (pixels_per_slice) *pixels_per_slice = plan.slice;
    if (bytes) *bytes = plan.rec_bytes + plan.coef_bytes;
    return ML_OK;
}

extern "C" int64_t ml_batchnorm_workspace_bytes(int64_t N, int32_t C) {
    int64_t bytes = 0;
    return ml_batchnorm_plan(N, C, nullptr, nullptr, &bytes) == ML_OK ? bytes : -1;
}

extern "C" int ml_batchnorm_train_f32(const float *x, const float *residual, float *y, const float *gamma, const float *beta,
                                      float *moving_mean, float *moving_var, double *saved, float *batch_mean,
                                      float *batch_var, int64_t N, int32_t C, float eps, double momentum, int32_t relu,
                                      void *workspace, int64_t workspace_bytes, void *stream) {
    const char *what = "batchnorm_train";
    BnPlan plan;
    BnGeom G;
    if (int rc = bn_geometry(what, N, C, true, plan, G)) return rc;
    const long long bytes = (long long)N * C * (long long)sizeof(float), vec = (long long)C * (long long)sizeof(float);
    if (int rc = bn_check_forward_maps(what, x, residual, y, bytes)) return rc;
    BN_REQUIRE_VEC(saved, "saved");
    BN_REQUIRE_VEC(batch_mean, "batch_mean");
    BN_REQUIRE_VEC(batch_var, "batch_var");
    ML_REQUIRE((moving_mean == nullptr) == (moving_var == nullptr), "%s: moving_mean and moving_var come together or not at all", what);
    ML_REQUIRE(eps >= 0.f && momentum >= 0.0 && momentum <= 1.0, "%s: eps must be non-negative, momentum in [0, 1]", what);
    if (int rc = bn_workspace(what, plan, workspace, workspace_bytes)) return rc;
    const long long ws_bytes = plan.rec_bytes + plan.coef_bytes;
    const long long saved_bytes = 2ll * C * (long long)sizeof(double);
    ML_REQUIRE(!ml_any_overlap({{saved, saved_bytes}, {batch_mean, vec}, {batch_var, vec}, {moving_mean, vec}, {moving_var, vec},
                                {workspace, ws_bytes}},
                               {{x, bytes}, {residual, bytes}, {gamma, vec}, {beta, vec}}) &&
                   !ml_any_overlap({{y, bytes}}, {{gamma, vec}, {beta, vec}}),
               "%s: an output (y, saved, batch_mean, batch_var, moving_mean, moving_var, workspace) overlaps an input", what);
    const ml_range outs[] = {{y, bytes}, {saved, saved_bytes}, {batch_mean, vec}, {batch_var, vec}, {moving_mean, vec},
                             {moving_var, vec}, {workspace, ws_bytes}};
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            ML_REQUIRE(!ml_ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes),
                       "%s: two outputs (y, saved, batch_mean, batch_var, moving_mean, moving_var, workspace) overlap", what);
    double *rec = reinterpret_cast<double *>(workspace);
    float *coef = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + plan.rec_bytes);
    BnFinish F = {};
    F.rec = rec; F.gamma = gamma; F.beta = beta; F.moving_mean = moving_mean; F.moving_var = moving_var; F.saved = saved;
    F.coef = coef; F.batch_mean = batch_mean; F.batch_var = batch_var; F.eps = eps;
    F.one_minus_momentum = (float)(1.0 - momentum);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)plan.S, (unsigned)plan.tiles);
    hipLaunchKernelGGL(bn_stats_kernel, grid, dim3(BN_TPB), 0, s, x, rec, G);
    hipLaunchKernelGGL(bn_finish_kernel, dim3((unsigned)plan.tiles), dim3(BN_TPB), 0, s, F, G);
    hipLaunchKernelGGL(bn_apply_kernel, grid, dim3(BN_TPB), 0, s, x, residual, y, coef, G, (int)(relu != 0));
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_batchnorm_infer_f32(const float *x, const float *residual, float *y, const float *gamma, const float *beta,
                                      const float *moving_mean, const float *moving_var, int64_t N, int32_t C, float eps,
                                      int32_t relu, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *what = "batchnorm_infer";
    BnPlan plan;
    BnGeom G;
    if (int rc = bn_geometry(what, N, C, false, plan, G)) return rc;
    const long long bytes = (long long)N * C * (long long)sizeof(float), vec = (long long)C * (long long)sizeof(float);
    if (int rc = bn_check_forward_maps(what, x, residual, y, bytes)) return rc;
    BN_REQUIRE_VEC(moving_mean, "moving_mean");
    BN_REQUIRE_VEC(moving_var, "moving_var");
    ML_REQUIRE(eps >= 0.f, "%s: eps must be non-negative", what);
    if (int rc = bn_workspace(what, plan, workspace, workspace_bytes)) return rc;
    const long long ws_bytes = plan.rec_bytes + plan.coef_bytes;
    ML_REQUIRE(!ml_any_overlap({{y, bytes}, {workspace, ws_bytes}},
                               {{gamma, vec}, {beta, vec}, {moving_mean, vec}, {moving_var, vec}, {residual, bytes}}) &&
                   !ml_ranges_overlap(workspace, ws_bytes, x, bytes) && !ml_ranges_overlap(workspace, ws_bytes, y, bytes),
               "%s: an output (y, workspace) overlaps an input or the other output", what);
    float *coef = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + plan.rec_bytes);
    BnFinish F = {};
    F.gamma = gamma; F.beta = beta; F.moving_mean = const_cast<float *>(moving_mean); F.moving_var = const_cast<float *>(moving_var);
    F.coef = coef; F.eps = eps; F.infer = 1;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_finish_kernel, dim3((unsigned)plan.tiles), dim3(BN_TPB), 0, s, F, G);
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)plan.S, (unsigned)plan.tiles), dim3(BN_TPB), 0, s, x, residual, y, coef, G,
                       (int)(relu != 0));
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

extern "C" int ml_batchnorm_grad_f32(const float *x, const float *dy, const float *y, const double *saved, const float *gamma,
                                     float *dx, float *d_residual, float *dgamma, float *dbeta, int64_t N, int32_t C,
                                     int32_t relu, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *what = "batchnorm_grad";
    BnPlan plan;
    BnGeom G;
    if (int rc = bn_geometry(what, N, C, true, plan, G)) return rc;
    const long long bytes = (long long)N * C * (long long)sizeof(float), vec = (long long)C * (long long)sizeof(float);
    BN_REQUIRE_MAP(x, "x");
    BN_REQUIRE_MAP(dy, "dy");
    BN_REQUIRE_MAP(dx, "dx");
    ML_REQUIRE(!relu || (y && ml_aligned16(y)), "%s: y (the forward's output, a 16-byte aligned pointer) is needed with relu: the mask "
               "is decided on it", what);
    ML_REQUIRE(!d_residual || ml_aligned16(d_residual), "%s: d_residual must be a 16-byte aligned pointer", what);
    BN_REQUIRE_VEC(saved, "saved");
    if (!relu) y = nullptr;
    if (int rc = bn_workspace(what, plan, workspace, workspace_bytes)) return rc;
    const long long ws_bytes = plan.rec_bytes + plan.coef_bytes;
    ML_REQUIRE(ml_add_or_disjoint(dx, dy, bytes), "%s: dx may be dy itself (in place), not a shifted view of it", what);
    ML_REQUIRE(ml_add_or_disjoint(d_residual, dy, bytes), "%s: d_residual may be dy itself, not a shifted view of it", what);
    ML_REQUIRE(!ml_ranges_overlap(dx, bytes, d_residual, bytes), "%s: dx and d_residual may not alias (only one of them may be dy)", what);
    ML_REQUIRE(!ml_any_overlap({{dx, bytes}, {d_residual, bytes}, {dgamma, vec}, {dbeta, vec}, {workspace, ws_bytes}},
                               {{x, bytes}, {y, bytes}, {saved, 2ll * C * (long long)sizeof(double)}, {gamma, vec}}),
               "%s: an output (dx, d_residual, dgamma, dbeta, workspace) overlaps x, y, saved or gamma", what);
    ML_REQUIRE(!ml_any_overlap({{dgamma, vec}, {dbeta, vec}, {workspace, ws_bytes}}, {{dy, bytes}, {dx, bytes}, {d_residual, bytes}}) &&
                   !ml_ranges_overlap(dgamma, vec, dbeta, vec) &&
                   !ml_any_overlap({{workspace, ws_bytes}}, {{dgamma, vec}, {dbeta, vec}}),
               "%s: dgamma, dbeta and workspace may overlap neither dy, dx, d_residual nor each other", what);
    double *rec = reinterpret_cast<double *>(workspace);
    float *coef = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + plan.rec_bytes);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)plan.S, (unsigned)plan.tiles);
    hipLaunchKernelGGL(bn_grad_reduce_kernel, grid, dim3(BN_TPB), 0, s, x, dy, y, rec, G);
    hipLaunchKernelGGL(bn_grad_finish_kernel, dim3((unsigned)plan.tiles), dim3(BN_TPB), 0, s, rec, saved, gamma, dgamma, dbeta, coef, G);
    hipLaunchKernelGGL(bn_grad_apply_kernel, grid, dim3(BN_TPB), 0, s, x, dy, y, dx, d_residual, coef, G);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}
