// Backward of the reference's chunk-wise GroupNormalization (groupnorm.hip; engine/normalization.py:116-160), fp32.
// For the chunk (n, g) of L = HWC/G values, element i has gamma / beta index j = g*cg + rho, rho = i mod cg, cg = C/G
// (the chunk starts at flat index g*L, a multiple of cg, and cg divides C: (g*L + i) mod C mod cg = i mod cg).  With
//   xhat = (x - mean) * r,  y = xhat * gamma[j] + beta[j],  d = dy * [y > 0 if relu],  gi = d * gamma[j]:
//   dx = r * (gi - mean_i(gi) - xhat * mean_i(gi * xhat)) * [x > 0 if input_relu],  dbeta[j] = sum d,  dgamma[j] = sum d * xhat.
// Per chunk and residue rho the kernels sum A[rho] = sum d and Bx[rho] = sum d * x; everything else follows in fp64:
//   sum gi = sum_rho gamma * A,   sum gi * xhat = r * (sum_rho gamma * Bx - mean * sum gi),
//   dbeta[j] = sum_n A[n,g,rho],  dgamma[j] = sum_n r_ng * (Bx[n,g,rho] - mean_ng * A[n,g,rho]).
// Passes (HBM-bound; algorithmic traffic = x and dy read, dx written = 12 B/elt):
//   one-pass  chunks of <= GN_ONEPASS_MAX floats with 16-byte accesses: one block per chunk holds x and dy in registers,
//             sums, writes its A / Bx record and dx.  12 B/elt.
//   sliced    reduce: one block per (chunk, slice of gn_plan) -> record (A, Bx) and, unless given, the slice's (sum x, sum x^2);
//             apply: folds the records of its chunk, writes its slice of dx.  x and dy are read twice: 20 B/elt.
//             With relu the mask needs mean and r BEFORE the reduce: a statistics pass runs first unless `stats` is given.
//   finish    one block per j folds the (n, slice) records into dgamma[j], dbeta[j].
// Sums: a thread adds fp32 terms into fp64 running sums; blocks reduce by a fixed tree (wave shuffle, the four waves in
// order); records are folded in index order.  No atomics: two launches give the same bits.  (sum x, sum x^2) are formed by the
// forward's own code (gn_common.h) over the forward's slices, so they have the bits of ml_groupnorm_chunk_stats_f32 and of the
// sliced forward, and the mask is decided by the forward's gn_y().
#include "gn_common.h"
#include "ranges.h"

namespace {

struct GgProb {
    const float *x, *dy;
    float *dx;
    const float *gamma, *beta;
    float *dgamma, *dbeta;
    const double *st;         // (sum x, sum x^2) pairs, Sp per chunk: the caller's (Sp = 1), the statistics pass's or the
    double *st_w;             //   reduce pass's (Sp = S; st_w = where the reduce pass writes them, else NULL); NULL: one-pass sums its own
    double *rec;              // per (chunk, slice): A[cg], Bx[cg]
    double *mr;               // per chunk: mean, r (fp64), written by the pass that writes dx, read by `finish`
    long long L, slice;       // slice: elements per block (sliced) / per slice of the forward's statistics plan (one-pass)
    int NG, N, S, Sp, C, G, relu, input_relu, vec, fast, onepass_vpt;
    float eps;
};
struct GgMulti {
    int n;
    int start[ML_GN_MAX_PROBLEMS + 1];
    GgProb p[ML_GN_MAX_PROBLEMS];
};

__device__ __forceinline__ const GgProb &gg_find(const GgMulti &A, int &id) {
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.start[pi + 1]) ++pi;
    id = blockIdx.x - A.start[pi];
    return A.p[pi];
}

// upstream gradient behind the forward's fused ReLU (strict, as tf.nn.relu's gradient)
__device__ __forceinline__ float gg_d(float x, float dy, const GgProb &P, float mean, float rstd, float gam, float bet) {
    if (!P.relu) return dy;
    return gn_y_val(x, mean, rstd, P.gamma != nullptr, gam, P.beta != nullptr, bet) > 0.f ? dy : 0.f;
}
// gamma[j] (1 without scale) and beta[j] (0 unless the mask needs it: P.beta is NULL then)
__device__ __forceinline__ float gg_gam(const GgProb &P, int j) { return P.gamma ? P.gamma[j] : 1.f; }
__device__ __forceinline__ float gg_bet(const GgProb &P, int j) { return P.beta ? P.beta[j] : 0.f; }

// ---- per-residue sums of a block -> its record.
// Cheap case (P.fast: 16-byte accesses, cg a power of two <= 256): a block sweeps 1024 elements, a multiple of cg, so
// slot e of thread t meets the residue (4t + e) mod cg in every sweep and keeps two fp64 sums for it.  The 1024 slots are
// folded per residue in a fixed order: part p = t / cg adds the 4 slots rho + (4p + q) cg, then residue t adds its parts.
__device__ __forceinline__ void gg_fold_slots(const double (&a)[4], const double (&b)[4], int cg, double *rec,
                                              double (*sh)[GN_TPB * 4]) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) { sh[0][t * 4 + e] = a[e]; sh[1][t * 4 + e] = b[e]; }
    __syncthreads();
    const int rho = t & (cg - 1), part = t / cg;
    double pa = 0, pb = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = rho + (part * 4 + q) * cg;
        pa += sh[0][idx];
        pb += sh[1][idx];
    }
    __syncthreads();
    sh[0][t] = pa;
    sh[1][t] = pb;
    __syncthreads();
    if (t < cg) {
        double A = 0, B = 0;
        for (int p = 0; p < GN_TPB / cg; ++p) { A += sh[0][t + p * cg]; B += sh[1][t + p * cg]; }
        rec[t] = A;
        rec[cg + t] = B;
    }
}

// General case (any cg, any alignment): thread t takes residue r0 + t mod span and every nparts-th of its elements of
// [lo, hi), scalar reads; residue rho then adds its parts in order.  Not fast; the shipped heads never come here.
__device__ __forceinline__ void gg_residues_general(const GgProb &P, const float *x, const float *dy, long long lo,
                                                    long long hi, int g, float mean, float rstd, double *rec,
                                                    double (*sh)[GN_TPB * 4]) {
    const int cg = P.C / P.G, t = threadIdx.x;
    const int span = min(cg, GN_TPB), nparts = GN_TPB / span;
    const int rl = t % span, part = t / span;
    for (int r0 = 0; r0 < cg; r0 += GN_TPB) {
        const int rho = r0 + rl;
        double a = 0, b = 0;
        if (part < nparts && rho < cg) {
            const float gam = gg_gam(P, g * cg + rho), bet = gg_bet(P, g * cg + rho);
            const long long i0 = lo + ((rho - (int)(lo % cg)) + cg) % cg;       // first element of the range with residue rho
            for (long long i = i0 + (long long)part * cg; i < hi; i += (long long)nparts * cg) {
                const float xv = x[i];
                const float d = gg_d(xv, dy[i], P, mean, rstd, gam, bet);
                a += (double)d;
                b += (double)(d * xv);
            }
        }
        __syncthreads();
        sh[0][t] = a;
        sh[1][t] = b;
        __syncthreads();
        if (part == 0 && rho < cg) {
            double A = 0, B = 0;
            for (int p = 0; p < nparts; ++p) { A += sh[0][rl + p * span]; B += sh[1][rl + p * span]; }
            rec[rho] = A;
            rec[cg + rho] = B;
        }
    }
}

// ---- sliced form, pass 1: block (ng, s) -> record, and the slice's (sum x, sum x^2) where nobody has them yet
__device__ __forceinline__ void gg_reduce_body(const GgProb &P, int ng, int s, double (*sh)[GN_TPB * 4]) {
    const int cg = P.C / P.G, g = ng % P.G;
    const float *x = P.x + (long long)ng * P.L, *dy = P.dy + (long long)ng * P.L;
    const long long lo = (long long)s * P.slice, hi = min(lo + P.slice, P.L);
    double *rec = P.rec + ((long long)ng * P.S + s) * 2 * cg;
    float mean = 0.f, rstd = 0.f;
    if (P.relu) {                            // (then the statistics are there: st_w == NULL)
        const GnMoments m = gn_moments(P.st, ng, P.Sp, P.L, P.eps);
        mean = m.mean; rstd = m.rstd;
    }
    if (P.fast) {
        float gam[4], bet[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = g * cg + ((threadIdx.x * 4 + e) & (cg - 1));
            gam[e] = gg_gam(P, j);
            bet[e] = gg_bet(P, j);
        }
        double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0}, sum = 0, sq = 0;
        for (long long i = lo + threadIdx.x * 4; i < hi; i += GN_TPB * 4) {
            float v[4], w[4];
            vload<float>(x + i, v);
            vload<float>(dy + i, w);
            if (P.st_w) gn_stats_add<4>(v, sum, sq);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = gg_d(v[e], w[e], P, mean, rstd, gam[e], bet[e]);
                a[e] += (double)d;
                b[e] += (double)(d * v[e]);
            }
        }
        if (P.st_w) gn_stats_store(sum, sq, P.st_w, P.S, ng, s);
        gg_fold_slots(a, b, cg, rec, sh);
    } else {
        if (P.st_w) {
            if (P.vec) gn_stats_body<float, true>(P.x, P.st_w, P.L, P.slice, P.S, ng, s);
            else gn_stats_body<float, false>(P.x, P.st_w, P.L, P.slice, P.S, ng, s);
        }
        gg_residues_general(P, x, dy, lo, hi, g, mean, rstd, rec, sh);
    }
}

// ---- the chunk's coefficients from its S records: k1 = mean(gi), k2 = mean(gi * xhat).  Flat fold over (slice, residue)
// in index order per thread, then the block tree.
struct GgCoef { float mean, rstd, k1, k2; };
__device__ __forceinline__ GgCoef gg_coef(const GgProb &P, int ng, const GnMoments &m, int S, double *red) {
    const int cg = P.C / P.G, g = ng % P.G;
    const double *rec = P.rec + (long long)ng * S * 2 * cg;
    double pa = 0, pb = 0;
    for (int p = threadIdx.x; p < S * cg; p += GN_TPB) {
        const int s = p / cg, rho = p - s * cg;
        const double gam = P.gamma ? (double)P.gamma[g * cg + rho] : 1.0;
        pa += gam * rec[(long long)s * 2 * cg + rho];
        pb += gam * rec[(long long)s * 2 * cg + cg + rho];
    }
    const double Sg = block_sum<GN_TPB>(pa, red);
    const double Sgx = block_sum<GN_TPB>(pb, red);
    const double k1 = Sg / (double)P.L;
    const double k2 = m.rstdd * (Sgx - m.meand * Sg) / (double)P.L;
    return {m.mean, m.rstd, (float)k1, (float)k2};
}

__device__ __forceinline__ float gg_dx(float x, float dy, const GgProb &P, const GgCoef &c, float gam, float bet) {
    const float xhat = (x - c.mean) * c.rstd;
    const float gi = gg_d(x, dy, P, c.mean, c.rstd, gam, bet) * gam;
    const float o = c.rstd * (gi - c.k1 - xhat * c.k2);
    return (P.input_relu && !(x > 0.f)) ? 0.f : o;
}

// ---- sliced form, pass 2: block (ng, s) writes its slice of dx.  Reads and writes index i in the same thread: dx may be dy.
__device__ __forceinline__ void gg_apply_body(const GgProb &P, int ng, int s, double *red) {
    const int cg = P.C / P.G, g = ng % P.G;
    const GnMoments m = gn_moments(P.st, ng, P.Sp, P.L, P.eps);
    const GgCoef c = gg_coef(P, ng, m, P.S, red);
    if (s == 0 && threadIdx.x == 0) { P.mr[ng * 2 + 0] = m.meand; P.mr[ng * 2 + 1] = m.rstdd; }
    const float *x = P.x + (long long)ng * P.L, *dy = P.dy + (long long)ng * P.L;
    float *dx = P.dx + (long long)ng * P.L;
    const long long lo = (long long)s * P.slice, hi = min(lo + P.slice, P.L);
    if (P.vec) {
        // the residues of a thread's four elements: the same in every sweep where cg divides the sweep (P.fast), else
        // they advance by 1024 mod cg and gamma / beta are read again
        int rho = (int)((lo + threadIdx.x * 4) % cg);
        const int step = (GN_TPB * 4) % cg;
        float gam[4], bet[4];
        for (long long i = lo + threadIdx.x * 4; i < hi; i += GN_TPB * 4) {
            float v[4], w[4], o[4];
            vload<float>(x + i, v);
            vload<float>(dy + i, w);
            if (step != 0 || i < lo + GN_TPB * 4) {
                int r = rho;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    gam[e] = gg_gam(P, g * cg + r);
                    bet[e] = gg_bet(P, g * cg + r);
                    if (++r == cg) r = 0;
                }
                rho += step;
                if (rho >= cg) rho -= cg;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = gg_dx(v[e], w[e], P, c, gam[e], bet[e]);
            vstore<float>(dx + i, o);
        }
    } else {
        for (long long i = lo + threadIdx.x; i < hi; i += GN_TPB) {
            const int j = g * cg + (int)(i % cg);
            dx[i] = gg_dx(x[i], dy[i], P, c, gg_gam(P, j), gg_bet(P, j));
        }
    }
}

// ---- one-pass form: block = one chunk, x and dy in registers (VPT float4 each per thread)
template <int VPT>
__device__ __forceinline__ void gg_onepass_body(const GgProb &P, int ng, double (*sh)[GN_TPB * 4], double *red) {
    const int cg = P.C / P.G, g = ng % P.G, L = (int)P.L;
    const float *x = P.x + (long long)ng * L, *dy = P.dy + (long long)ng * L;
    float *dx = P.dx + (long long)ng * L;
    double *rec = P.rec + (long long)ng * 2 * cg;
    float v[VPT][4], w[VPT][4];
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int i = (k * GN_TPB + threadIdx.x) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = w[k][e] = 0.f;
        if (i < L) { vload<float>(x + i, v[k]); vload<float>(dy + i, w[k]); }
    }
    GnMoments m;
    if (P.st) {
        m = gn_moments(P.st, ng, P.Sp, P.L, P.eps);
    } else {
        // (sum x, sum x^2) with the bits of the statistics kernel: its slices are whole sweeps, so slice s is the vectors
        // k = s * vps .. of every thread; per slice the thread sums in k order, the block reduces, the slices add in order
        const int vps = (int)(P.slice / (GN_TPB * 4));
        double sum = 0, sq = 0, tsum = 0, tsq = 0;
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            if ((k * GN_TPB + threadIdx.x) * 4 < L) gn_stats_add<4>(v[k], sum, sq);
            if ((k + 1) % vps == 0 || k == VPT - 1) {
                tsum += block_sum<GN_TPB>(sum, red);         // (a slice past the chunk's end adds an exact zero)
                tsq += block_sum<GN_TPB>(sq, red);
                sum = sq = 0;
            }
        }
        __shared__ double tot[2];
        __syncthreads();
        if (threadIdx.x == 0) { tot[0] = tsum; tot[1] = tsq; }
        __syncthreads();
        m = gn_moments(tot, 0, 1, P.L, P.eps);
    }
    if (P.fast) {
        float gam[4], bet[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = g * cg + ((threadIdx.x * 4 + e) & (cg - 1));
            gam[e] = gg_gam(P, j);
            bet[e] = gg_bet(P, j);
        }
        double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            if ((k * GN_TPB + threadIdx.x) * 4 >= L) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = gg_d(v[k][e], w[k][e], P, m.mean, m.rstd, gam[e], bet[e]);
                a[e] += (double)d;
                b[e] += (double)(d * v[k][e]);
            }
        }
        gg_fold_slots(a, b, cg, rec, sh);
    } else {
        gg_residues_general(P, x, dy, 0, L, g, m.mean, m.rstd, rec, sh);   // (reads dy before any dx is written)
    }
    __syncthreads();                         // the record, written by other threads of this block
    const GgCoef c = gg_coef(P, ng, m, 1, red);
    if (threadIdx.x == 0) { P.mr[ng * 2 + 0] = m.meand; P.mr[ng * 2 + 1] = m.rstdd; }
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int i = (k * GN_TPB + threadIdx.x) * 4;
        if (i >= L) continue;
        int r = i % cg;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = gg_dx(v[k][e], w[k][e], P, c, gg_gam(P, g * cg + r), gg_bet(P, g * cg + r));
            if (++r == cg) r = 0;
        }
        vstore<float>(dx + i, o);
    }
}

// ------------------------------------------------------------------ the launches: several problems each
__global__ void __launch_bounds__(GN_TPB)
gn_grad_stats_kernel(const GgMulti A) {
    int id;
    const GgProb &P = gg_find(A, id);
    if (P.vec) gn_stats_body<float, true>(P.x, const_cast<double *>(P.st), P.L, P.slice, P.S, id / P.S, id % P.S);
    else gn_stats_body<float, false>(P.x, const_cast<double *>(P.st), P.L, P.slice, P.S, id / P.S, id % P.S);
}

__global__ void __launch_bounds__(GN_TPB)
gn_grad_reduce_kernel(const GgMulti A) {
    __shared__ double sh[2][GN_TPB * 4];
    int id;
    const GgProb &P = gg_find(A, id);
    gg_reduce_body(P, id / P.S, id % P.S, sh);
}

__global__ void __launch_bounds__(GN_TPB)
gn_grad_apply_kernel(const GgMulti A) {
    __shared__ double sh[2][GN_TPB * 4];
    __shared__ double red[GN_TPB / 64];
    int id;
    const GgProb &P = gg_find(A, id);
    if (P.onepass_vpt == 0) gg_apply_body(P, id / P.S, id % P.S, red);
    else if (P.onepass_vpt == 1) gg_onepass_body<1>(P, id, sh, red);
    else if (P.onepass_vpt == 2) gg_onepass_body<2>(P, id, sh, red);
    else gg_onepass_body<4>(P, id, sh, red);
}

// block = one j of one problem: the (n, slice) records in index order per thread, then the block tree
__global__ void __launch_bounds__(GN_TPB)
gn_grad_finish_kernel(const GgMulti A) {
    __shared__ double red[GN_TPB / 64];
    int j;
    const GgProb &P = gg_find(A, j);
    const int cg = P.C / P.G, g = j / cg, rho = j - g * cg;
    double db = 0, dg = 0;
    for (int p = threadIdx.x; p < P.N * P.S; p += GN_TPB) {
        const int n = p / P.S, s = p - n * P.S, ng = n * P.G + g;
        const double *rec = P.rec + ((long long)ng * P.S + s) * 2 * cg;
        const double a = rec[rho], bx = rec[cg + rho];
        db += a;
        dg += P.mr[ng * 2 + 1] * (bx - P.mr[ng * 2 + 0] * a);
    }
    db = block_sum<GN_TPB>(db, red);
    dg = block_sum<GN_TPB>(dg, red);
    if (threadIdx.x == 0) {
        if (P.dbeta) P.dbeta[j] = (float)db;
        if (P.dgamma) P.dgamma[j] = (float)dg;
    }
}

// the S partial pairs of every chunk, added in index order -> stats[chunk] (ml_groupnorm_chunk_stats_f32)
__global__ void gn_stats_fold_kernel(const double *__restrict__ ws, double *__restrict__ stats, int NG, int S) {
    const int ng = blockIdx.x * blockDim.x + threadIdx.x;
    if (ng >= NG) return;
    double sum = 0, sq = 0;
    for (int i = 0; i < S; ++i) {
        sum += ws[((long long)ng * S + i) * 2 + 0];
        sq += ws[((long long)ng * S + i) * 2 + 1];
    }
    stats[ng * 2 + 0] = sum;
    stats[ng * 2 + 1] = sq;
}

constexpr long long gg_align(long long b) { return (b + 255) / 256 * 256; }
static long long gg_stats_bytes(long long N, long long G) { return gg_align(N * G * GN_MAX_SPLIT * 2 * (long long)sizeof(double)); }
static long long gg_rec_bytes(long long N, long long C) { return gg_align(N * GN_MAX_SPLIT * 2 * C * (long long)sizeof(double)); }
static long long gg_mr_bytes(long long N, long long G) { return gg_align(N * G * 2 * (long long)sizeof(double)); }

static int gg_validate_dims(const void *x, int32_t N, int64_t HWC, int32_t C, int32_t G, const char *what) {
    ML_REQUIRE(x, "%s: null pointer", what);
    ML_REQUIRE(N > 0 && HWC > 0 && C > 0 && G > 0, "%s: bad dims", what);
    ML_REQUIRE(C >= G, "%s: Number of groups (%d) cannot be more than the number of channels (%d).", what, G, C);
    ML_REQUIRE(C % G == 0, "%s: Number of groups (%d) must be a multiple of the number of channels (%d).", what, G, C);
    ML_REQUIRE(HWC % C == 0 && HWC % G == 0, "%s: H*W*C (%lld) must be divisible by C and by G", what, (long long)HWC);
    ML_REQUIRE((long long)N * G * GN_MAX_SPLIT < (1ll << 31), "%s: N*G too large", what);
    return ML_OK;
}

static int gg_run(const ml_gn_grad_desc *descs, int32_t n, const char *what, void *workspace, int64_t workspace_bytes,
                  void *stream) {
    GgMulti st, rd, ap, fi;
    st.n = rd.n = fi.n = 0;
    ap.n = n;
    long long sb = 0, rb = 0, ab = 0, fb = 0, ws_off = 0;
    for (int i = 0; i < n; ++i) {
        const ml_gn_grad_desc &d = descs[i];
        if (int rc = gg_validate_dims(d.x, d.N, d.HWC, d.C, d.G, what)) return rc;
        ML_REQUIRE(d.dy && d.dx, "%s: null pointer", what);
        const long long bytes = (long long)d.N * d.HWC * (long long)sizeof(float);
        ML_REQUIRE(!ml_ranges_overlap(d.x, bytes, d.dx, bytes), "%s: dx may not alias x (the layer's input is needed as it was)", what);
        ML_REQUIRE(ml_add_or_disjoint(d.dx, d.dy, bytes), "%s: dx may be dy itself, not a shifted view of it", what);
        const long long L = d.HWC / d.G;
        const int cg = d.C / d.G;
        GgProb P;
        P.x = d.x; P.dy = d.dy; P.dx = d.dx; P.gamma = d.gamma; P.beta = d.relu ? d.beta : nullptr;
        P.dgamma = d.dgamma; P.dbeta = d.dbeta;
        P.L = L; P.N = d.N; P.NG = d.N * d.G; P.C = d.C; P.G = d.G; P.relu = d.relu != 0; P.input_relu = d.input_relu != 0;
        P.eps = d.eps;
        P.vec = (L % 4 == 0) && (d.C % 4 == 0) && ml_aligned16(d.x) && ml_aligned16(d.dy) && ml_aligned16(d.dx);
        P.fast = P.vec && (cg & (cg - 1)) == 0 && cg <= GN_TPB;
        const GnPlan plan = gn_plan(L, P.NG, 4);         // the forward's slices (vec or not)
        const bool onepass = P.vec && L <= GN_ONEPASS_MAX;
        P.S = onepass ? 1 : plan.S;
        P.slice = plan.slice;
        P.onepass_vpt = 0;
        if (onepass) {
            const int vn = (int)((L + 3) / 4);
            P.onepass_vpt = vn <= 256 ? 1 : (vn <= 512 ? 2 : 4);
        }
        const long long need = gg_stats_bytes(d.N, d.G) + gg_rec_bytes(d.N, d.C) + gg_mr_bytes(d.N, d.G);
        ML_REQUIRE(ws_off + need <= workspace_bytes, "%s: workspace too small (%lld bytes needed so far)", what, ws_off + need);
        char *base = reinterpret_cast<char *>(workspace) + ws_off;
        ws_off += need;
        double *ws_st = reinterpret_cast<double *>(base);
        P.rec = reinterpret_cast<double *>(base + gg_stats_bytes(d.N, d.G));
        P.mr = reinterpret_cast<double *>(base + gg_stats_bytes(d.N, d.G) + gg_rec_bytes(d.N, d.C));
        P.st = nullptr; P.st_w = nullptr; P.Sp = 1;
        bool stats_pass = false;
        if (d.stats) {
            P.st = d.stats;
        } else if (!onepass) {
            P.st = ws_st; P.Sp = plan.S;
            if (P.relu) stats_pass = true;
            else P.st_w = ws_st;
        }
        if (stats_pass) {
            st.start[st.n] = (int)sb;
            st.p[st.n++] = P;
            sb += (long long)P.NG * P.S;
        }
        if (!onepass) {
            rd.start[rd.n] = (int)rb;
            rd.p[rd.n++] = P;
            rb += (long long)P.NG * P.S;
        }
        ap.start[i] = (int)ab;
        ap.p[i] = P;
        ab += (long long)P.NG * P.S;
        if (d.dgamma || d.dbeta) {
            fi.start[fi.n] = (int)fb;
            fi.p[fi.n++] = P;
            fb += d.C;
        }
        ML_REQUIRE(ab < (1ll << 31) && fb < (1ll << 31), "%s: grid too large", what);
    }
    st.start[st.n] = (int)sb;
    rd.start[rd.n] = (int)rb;
    ap.start[n] = (int)ab;
    fi.start[fi.n] = (int)fb;
    hipStream_t s = (hipStream_t)stream;
    if (st.n > 0) hipLaunchKernelGGL(gn_grad_stats_kernel, dim3((unsigned)sb), dim3(GN_TPB), 0, s, st);
    if (rd.n > 0) hipLaunchKernelGGL(gn_grad_reduce_kernel, dim3((unsigned)rb), dim3(GN_TPB), 0, s, rd);
    hipLaunchKernelGGL(gn_grad_apply_kernel, dim3((unsigned)ab), dim3(GN_TPB), 0, s, ap);
    if (fi.n > 0) hipLaunchKernelGGL(gn_grad_finish_kernel, dim3((unsigned)fb), dim3(GN_TPB), 0, s, fi);
    ML_CHECK_LAUNCH(what);
    return ML_OK;
}

}  // namespace

extern "C" int64_t ml_groupnorm_grad_workspace_bytes(int32_t N, int32_t G, int32_t C) {
    return gg_stats_bytes(N, G) + gg_rec_bytes(N, C) + gg_mr_bytes(N, G);
}

extern "C" int ml_groupnorm_chunk_grad_f32(const float *x, const float *dy, const float *gamma, const float *beta, float *dx,
                                           float *dgamma, float *dbeta, const double *stats, int32_t N, int64_t HWC,
                                           int32_t C, int32_t G, float eps, int32_t relu, int32_t input_relu,
                                           void *workspace, void *stream) {
    ML_REQUIRE(workspace, "groupnorm_grad: null pointer");
    ml_gn_grad_desc d = {};
    d.x = x; d.dy = dy; d.gamma = gamma; d.beta = beta; d.dx = dx; d.dgamma = dgamma; d.dbeta = dbeta; d.stats = stats;
    d.HWC = HWC; d.N = N; d.C = C; d.G = G; d.eps = eps; d.relu = relu; d.input_relu = input_relu;
    if (int rc = gg_validate_dims(x, N, HWC, C, G, "groupnorm_grad")) return rc;
    return gg_run(&d, 1, "groupnorm_grad", workspace, ml_groupnorm_grad_workspace_bytes(N, G, C), stream);
}

extern "C" int ml_groupnorm_grad_multi_f32(const ml_gn_grad_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes,
                                           void *stream) {
    ML_REQUIRE(descs && n >= 1 && n <= ML_GN_MAX_PROBLEMS && workspace, "groupnorm_grad_multi: need 1..%d problems and a workspace",
               ML_GN_MAX_PROBLEMS);
    return gg_run(descs, n, "groupnorm_grad_multi", workspace, workspace_bytes, stream);
}

extern "C" int ml_groupnorm_chunk_stats_f32(const float *x, double *stats, int32_t N, int64_t HWC, int32_t C, int32_t G,
                                            void *workspace, void *stream) {
    ML_REQUIRE(stats && workspace, "groupnorm_stats: null pointer");
    if (int rc = gg_validate_dims(x, N, HWC, C, G, "groupnorm_stats")) return rc;
    const long long L = HWC / G;
    const int NG = N * G;
    const bool vec = (L % 4 == 0) && (C % 4 == 0) && ml_aligned16(x);
    const GnPlan plan = gn_plan(L, NG, 4);
    GgMulti st;
    st.n = 1;
    st.start[0] = 0;
    st.start[1] = NG * plan.S;
    GgProb &P = st.p[0];
    P = GgProb{};
    P.x = x; P.st = reinterpret_cast<double *>(workspace); P.L = L; P.slice = plan.slice; P.S = plan.S; P.vec = vec;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_grad_stats_kernel, dim3((unsigned)(NG * plan.S)), dim3(GN_TPB), 0, s, st);
    hipLaunchKernelGGL(gn_stats_fold_kernel, dim3((NG + 255) / 256), dim3(256), 0, s, reinterpret_cast<const double *>(workspace),
                       stats, NG, plan.S);
    ML_CHECK_LAUNCH("groupnorm_stats");
    return ML_OK;
}
