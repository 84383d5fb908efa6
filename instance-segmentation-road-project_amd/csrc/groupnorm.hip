// The reference's chunk-wise GroupNormalization (engine/normalization.py:116-160).
// Sample n's flat H*W*C vector is cut into G contiguous chunks of L = HWC/G floats;
//   y = (x - mean_g) / sqrt(var_g + eps) * gamma[j] + beta[j],  j = g*(C/G) + (c mod C/G).
// HBM-bound: algorithmic traffic = 1 read + 1 write of x (8 B/elt).
// Chunks of up to 4096 floats (the small pyramid levels, all RoI maps) take the ONE-PASS kernel: one
// block per (sample, chunk) holds the chunk in registers (<= 4 float4 per thread), reduces mean and
// then sum((x-mean)^2) across the block, normalises and writes -- 8 B/elt, one launch.
// Larger chunks read x twice (stats pass + apply pass) = 12 B/elt, the second read usually served by
// L2/Infinity Cache:
//   pass 1: grid (S, N*G): each block sums a slice of one chunk in fp64 (sum, sum of squares)
//           -> workspace[(n*G+g)*S + s]   (fp64 partials: no cancellation issue in E[x^2]-mean^2)
//   pass 2: grid (S2, N*G): each block folds the S partials, then normalises its slice.
// Storage type T: float, or IEEE half (the heads of the fp16 path: x and y are half, 8 per 16-byte access; statistics
// are fp64 sums of the stored values, the normalisation runs in fp32 and is rounded ONCE at the store).
#include "gn_common.h"

namespace {

template <class T, bool VEC4>
__global__ void gn_stats_kernel(const T *__restrict__ x, double *__restrict__ ws, long long L, long long slice,
                                int S) {
    gn_stats_body<T, VEC4>(x, ws, L, slice, S, blockIdx.y, blockIdx.x);
}

template <class T, bool VEC4 = true>
__device__ __forceinline__ void gn_apply_body(const T *x, T *y, const float *__restrict__ gamma,
                                              const float *__restrict__ beta, const double *__restrict__ ws, long long L,
                                              long long slice, int S, int C, int G, float eps, int relu, int out_cs,
                                              int out_co, int ng, int s, int Sp = -1) {
    constexpr int W = VW<T>::value;
    const int g = ng % G;
    const int cg = C / G;
    if (Sp < 0) Sp = S;
    const GnMoments m = gn_moments(ws, ng, Sp, L, eps);
    const float mean = m.mean, rstd = m.rstd;
    const T *p = x + (long long)ng * L;
    const bool dense = (out_cs == C);
    // dense: y has x's layout.  sliced: element f of the sample -> y[n][f / C][out_co + f % C]
    const long long HWC = L * G;
    T *q = dense ? y + (long long)ng * L : y + (long long)(ng / G) * (HWC / C) * out_cs + out_co;
    const long long lo = (long long)s * slice;
    const long long hi = min(lo + slice, L);
    // flat index inside the sample = g*L + i ; channel = that mod C
    const long long gbase = (long long)g * L;
    if (VEC4 && (cg % W == 0) && HWC < (1ll << 31)) {
        // Hot form: a vector never straddles a gamma period (cg % W == 0) and the flat index fits 32 bits, so
        // channel / pixel / gamma offset advance incrementally -- no division or modulo inside the loop (the
        // 64-bit `%` and `/` per vector made this pass VALU-bound)
        const unsigned Cu = (unsigned)C, cgu = (unsigned)cg;
        const long long i0 = lo + threadIdx.x * W;
        const unsigned f0 = (unsigned)(gbase + i0);
        unsigned c0 = f0 % Cu, pix = f0 / Cu, cm = c0 % cgu;
        const unsigned stepc = (GN_TPB * (unsigned)W) % Cu, steppix = (GN_TPB * (unsigned)W) / Cu, stepm = (GN_TPB * (unsigned)W) % cgu;
        const float *gp = gamma ? gamma + g * cg : nullptr;
        const float *bp = beta ? beta + g * cg : nullptr;
        for (long long i = i0; i < hi; i += GN_TPB * W) {
            float v[W], o[W];
            vload<T>(p + i, v);
#pragma unroll
            for (int e = 0; e < W; ++e) o[e] = (v[e] - mean) * rstd;
            if (gp) {
#pragma unroll
                for (int e4 = 0; e4 < W; e4 += 4) {
                    const f32x4 gv = *reinterpret_cast<const f32x4 *>(gp + cm + e4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e4 + e] *= gv[e];
                }
            }
            if (bp) {
#pragma unroll
                for (int e4 = 0; e4 < W; e4 += 4) {
                    const f32x4 bv = *reinterpret_cast<const f32x4 *>(bp + cm + e4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e4 + e] += bv[e];
                }
            }
            if (relu) {
#pragma unroll
                for (int e = 0; e < W; ++e) o[e] = fmaxf(o[e], 0.f);
            }
            if (dense) vstore<T>(q + i, o);
            else vstore<T>(q + (long long)pix * out_cs + c0, o);
            c0 += stepc;
            pix += steppix;
            if (c0 >= Cu) { c0 -= Cu; ++pix; }
            cm += stepm;
            if (cm >= cgu) cm -= cgu;
        }
    } else if (VEC4) {
        for (long long i = lo + threadIdx.x * W; i < hi; i += GN_TPB * W) {
            float v[W], o[W];
            vload<T>(p + i, v);
            const int c0 = (int)((gbase + i) % C);
#pragma unroll
            for (int e = 0; e < W; ++e) {
                int c = c0 + e;
                if (c >= C) c -= C;
                const int j = g * cg + (c % cg);
                const float t = gn_y(v[e], mean, rstd, gamma, beta, j);
                o[e] = relu ? fmaxf(t, 0.f) : t;
            }
            if (dense) vstore<T>(q + i, o);
            else vstore<T>(q + ((gbase + i) / C) * out_cs + c0, o);
        }
    } else {
        for (long long i = lo + threadIdx.x; i < hi; i += GN_TPB) {
            const int c = (int)((gbase + i) % C);
            const int j = g * cg + (c % cg);
            const float t = gn_y((float)p[i], mean, rstd, gamma, beta, j);
            const float r = relu ? fmaxf(t, 0.f) : t;
            if (dense) q[i] = (T)r;
            else q[((gbase + i) / C) * out_cs + c] = (T)r;
        }
    }
}

template <class T, bool VEC4>
__global__ void gn_apply_kernel(const T *x, T *y, const float *__restrict__ gamma,
                                const float *__restrict__ beta, const double *__restrict__ ws, long long L,
                                long long slice, int S, int C, int G, float eps, int relu, int out_cs, int out_co) {
    gn_apply_body<T, VEC4>(x, y, gamma, beta, ws, L, slice, S, C, G, eps, relu, out_cs, out_co, blockIdx.y, blockIdx.x);
}

// ---- one-pass form: the chunk lives in registers.  Block (TPB threads) = one (sample, chunk).
template <class T, int TPB, int VPT>
__device__ __forceinline__ void gn_onepass_body(const T *__restrict__ x, T *__restrict__ y,
                                                const float *__restrict__ gamma, const float *__restrict__ beta, int L,
                                                int C, int G, float eps, int relu, int out_cs, int out_co, int ng) {
    constexpr int W = VW<T>::value;
    __shared__ double red[TPB / 64];
    const int g = ng % G;
    const int cg = C / G;
    const T *p = x + (long long)ng * L;
    float v[VPT][W];
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int i = (k * TPB + threadIdx.x) * W;
#pragma unroll
        for (int e = 0; e < W; ++e) v[k][e] = 0.f;
        if (i < L) {
            vload<T>(p + i, v[k]);
            sum += ((double)v[k][0] + (double)v[k][1]) + ((double)v[k][2] + (double)v[k][3]);
            if constexpr (W == 8) sum += ((double)v[k][4] + (double)v[k][5]) + ((double)v[k][6] + (double)v[k][7]);
        }
    }
    const double meand = block_sum<TPB>(sum, red) / (double)L;
    const float mean = (float)meand;
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int i = (k * TPB + threadIdx.x) * W;
        if (i < L) {
#pragma unroll
            for (int e = 0; e < W; ++e) { const double d = (double)v[k][e] - meand; sq += d * d; }
        }
    }
    const double vard = block_sum<TPB>(sq, red) / (double)L;
    const float rstd = (float)(1.0 / sqrt(vard + (double)eps));
    const bool dense = (out_cs == C);
    const long long HWC = (long long)L * G;
    T *q = dense ? y + (long long)ng * L : y + (long long)(ng / G) * (HWC / C) * out_cs + out_co;
    const long long gbase = (long long)g * L;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int i = (k * TPB + threadIdx.x) * W;
        if (i >= L) continue;
        const int c0 = (int)((gbase + i) % C);
        float o[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            int c = c0 + e;
            if (c >= C) c -= C;
            const int j = g * cg + (c % cg);
            const float t = gn_y(v[k][e], mean, rstd, gamma, beta, j);
            o[e] = relu ? fmaxf(t, 0.f) : t;
        }
        if (dense) vstore<T>(q + i, o);
        else vstore<T>(q + ((gbase + i) / C) * out_cs + c0, o);
    }
}

template <class T, int TPB, int VPT>
__global__ void __launch_bounds__(TPB)
gn_onepass_kernel(const T *__restrict__ x, T *__restrict__ y, const float *__restrict__ gamma,
                  const float *__restrict__ beta, int L, int C, int G, float eps, int relu, int out_cs, int out_co) {
    gn_onepass_body<T, TPB, VPT>(x, y, gamma, beta, L, C, G, eps, relu, out_cs, out_co, blockIdx.x);
}

template <class T, int TPB, int VPT>
void launch_onepass(const T *x, T *y, const float *gamma, const float *beta, int NG, int L, int C, int G,
                    float eps, int relu, int out_cs, int out_co, hipStream_t s) {
    hipLaunchKernelGGL((gn_onepass_kernel<T, TPB, VPT>), dim3(NG), dim3(TPB), 0, s, x, y, gamma, beta, L, C, G, eps, relu,
                       out_cs, out_co);
}


// ------------------------------------------------------------------ several problems in one launch pair
// The un-shared towers normalise five pyramid levels (and the mask head three RoI levels) one after the other:
// the two coarsest levels are a few thousand floats each, i.e. a ~10 us launch apiece behind the 46 us P3 launch.
// ml_groupnorm_multi_f32 runs all of them as (1) one statistics launch over the two-pass problems and (2) one launch
// that applies those AND normalises the small-chunk problems in their register-resident one-pass form.  A problem
// without 16-byte accesses (onepass_vpt = -1) runs the two passes with scalar ones beside the others.  Same plan and arithmetic
// per problem as the single-problem kernels (bit-identical results).  The single-problem kernels stay: a launch of one
// through these kernels was measured slower (the GroupNormalization kernel row).
struct GnProb {
    const void *x;            // T = float or _Float16 (one type per launch)
    void *y;
    const float *gamma, *beta;
    double *ws;               // partials of this problem (two-pass only)
    long long L, slice;
    int NG, S, C, G, relu, out_cs, out_co, onepass_vpt;   // onepass_vpt: 0 = two-pass, > 0: float4 per thread,
                                                          // -1 = two-pass with scalar accesses (no 16-byte ones)
    int Sp;                   // (sum, sum of squares) pairs per chunk in `ws`: S from gn_stats, or the producing conv's tiles
    float eps;
    const int *live;          // fixed-capacity RoI batches: sample n is live iff n % live_period < max(1, *live)
    int live_period;
};
__device__ __forceinline__ bool gn_dead(const GnProb &P, int ng) {
    return P.live && ((ng / P.G) % P.live_period) >= max(1, *P.live);
}
struct GnMulti {
    int n;
    int start[ML_GN_MAX_PROBLEMS + 1];
    GnProb p[ML_GN_MAX_PROBLEMS];
};

template <class T>
__global__ void __launch_bounds__(GN_TPB)
gn_multi_stats_kernel(const GnMulti A) {
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.start[pi + 1]) ++pi;
    const GnProb &P = A.p[pi];
    const int id = blockIdx.x - A.start[pi];
    if (gn_dead(P, id / P.S)) return;
    const T *x = reinterpret_cast<const T *>(P.x);
    if (P.onepass_vpt == 0) gn_stats_body<T, true>(x, P.ws, P.L, P.slice, P.S, id / P.S, id % P.S);          // (block-uniform)
    else gn_stats_body<T, false>(x, P.ws, P.L, P.slice, P.S, id / P.S, id % P.S);
}

template <class T>
__global__ void __launch_bounds__(GN_TPB)
gn_multi_apply_kernel(const GnMulti A) {
    int pi = 0;
    while (pi + 1 < A.n && (int)blockIdx.x >= A.start[pi + 1]) ++pi;
    const GnProb &P = A.p[pi];
    const int id = blockIdx.x - A.start[pi];
    const T *x = reinterpret_cast<const T *>(P.x);
    T *y = reinterpret_cast<T *>(P.y);
    if (gn_dead(P, P.onepass_vpt <= 0 ? id / P.S : id)) return;          // (block-uniform)
    if (P.onepass_vpt == 0) {
        gn_apply_body<T>(x, y, P.gamma, P.beta, P.ws, P.L, P.slice, P.S, P.C, P.G, P.eps, P.relu, P.out_cs, P.out_co,
                         id / P.S, id % P.S, P.Sp);
    } else if (P.onepass_vpt == 1) {
        gn_onepass_body<T, GN_TPB, 1>(x, y, P.gamma, P.beta, (int)P.L, P.C, P.G, P.eps, P.relu, P.out_cs, P.out_co, id);
    } else if (P.onepass_vpt == 2) {
        gn_onepass_body<T, GN_TPB, 2>(x, y, P.gamma, P.beta, (int)P.L, P.C, P.G, P.eps, P.relu, P.out_cs, P.out_co, id);
    } else if (P.onepass_vpt < 0) {
        gn_apply_body<T, false>(x, y, P.gamma, P.beta, P.ws, P.L, P.slice, P.S, P.C, P.G, P.eps, P.relu, P.out_cs, P.out_co,
                                id / P.S, id % P.S, P.Sp);
    } else {
        if constexpr (std::is_same<T, float>::value)
            gn_onepass_body<T, GN_TPB, 4>(x, y, P.gamma, P.beta, (int)P.L, P.C, P.G, P.eps, P.relu, P.out_cs, P.out_co, id);
    }
}

}  // namespace

extern "C" int64_t ml_groupnorm_workspace_bytes(int32_t N, int32_t G) {
    return (int64_t)N * G * GN_MAX_SPLIT * 2 * (int64_t)sizeof(double);
}

static int gn_validate(const void *x, void *y, int32_t N, int64_t HWC, int32_t C, int32_t G, int32_t out_cstride,
                       int32_t out_coff) {
    ML_REQUIRE(x && y, "groupnorm: null pointer");
    ML_REQUIRE(N > 0 && HWC > 0 && C > 0 && G > 0, "groupnorm: bad dims");
    ML_REQUIRE(C >= G, "groupnorm: Number of groups (%d) cannot be more than the number of channels (%d).", G, C);
    ML_REQUIRE(C % G == 0, "groupnorm: Number of groups (%d) must be a multiple of the number of channels (%d).", G, C);
    ML_REQUIRE(HWC % C == 0 && HWC % G == 0, "groupnorm: H*W*C (%lld) must be divisible by C and by G", (long long)HWC);
    ML_REQUIRE((long long)N * G < (1ll << 31), "groupnorm: N*G too large");
    ML_REQUIRE(out_cstride >= C && out_coff >= 0 && out_coff + C <= out_cstride, "groupnorm: bad output slice");
    ML_REQUIRE(out_cstride == C ? out_coff == 0 : true, "groupnorm: dense output must have out_coff 0");
    return ML_OK;
}

template <class T>
static int gn_multi(const ml_gn_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes, void *stream) {
    constexpr int W = VW<T>::value;
    GnMulti st, ap;
    st.n = 0;
    ap.n = n;
    long long sb = 0, ab = 0, ws_off = 0;
    for (int i = 0; i < n; ++i) {
        const ml_gn_desc &d = descs[i];
        if (int rc = gn_validate(d.x, d.y, d.N, d.HWC, d.C, d.G, d.out_cstride, d.out_coff)) return rc;
        const long long L = d.HWC / d.G;
        GnProb P;
        P.x = d.x; P.y = d.y; P.gamma = d.gamma; P.beta = d.beta;
        P.L = L; P.NG = d.N * d.G; P.C = d.C; P.G = d.G; P.relu = d.relu; P.out_cs = d.out_cstride; P.out_co = d.out_coff;
        P.eps = d.eps;
        const bool vec = (L % W == 0) && (d.C % W == 0) && (d.out_cstride % W == 0) && (d.out_coff % W == 0) &&
                         ml_aligned16(d.x) && ml_aligned16(d.y);
        P.live = d.live; P.live_period = d.live_period;
        if (d.live) ML_REQUIRE(d.live_period >= 1 && d.N % d.live_period == 0, "groupnorm_multi: live_period must divide N");
        P.ws = nullptr; P.S = 1; P.slice = L; P.onepass_vpt = 0; P.Sp = -1;
        if (vec && L <= GN_ONEPASS_MAX) {
            const int vn = (int)((L + W - 1) / W);
            P.onepass_vpt = vn <= 256 ? 1 : (vn <= 512 ? 2 : 4);
        } else {
            // gn_single's slices: they fix the order of the fp64 partial sums, hence the bits (scalar: cut as floats are)
            const GnPlan plan = gn_plan(L, P.NG, vec ? W : 4);
            P.S = plan.S; P.slice = plan.slice;
            if (!vec) P.onepass_vpt = -1;
        }
        if (P.onepass_vpt <= 0 && d.partials) {
            // the producing conv summed its tiles (ml_conv2d_desc.gn_partials): no statistics pass over this tensor
            ML_REQUIRE(d.n_partials >= 1 && d.n_partials <= 4096,
                       "groupnorm_multi: problem %d: 1..4096 fp64 (sum, sum of squares) pairs per chunk", i);
            P.ws = const_cast<double *>(d.partials);
            P.Sp = d.n_partials;
        } else if (P.onepass_vpt <= 0) {
            const long long bytes = (long long)P.NG * P.S * 2 * (long long)sizeof(double);
            ML_REQUIRE(ws_off + bytes <= workspace_bytes, "groupnorm_multi: workspace too small (%lld bytes needed so far)",
                       ws_off + bytes);
            P.ws = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + ws_off);
            ws_off += (bytes + 255) / 256 * 256;
            st.start[st.n] = (int)sb;
            st.p[st.n++] = P;
            sb += (long long)P.NG * P.S;
        }
        ap.start[i] = (int)ab;
        ab += (long long)P.NG * P.S;
        ap.p[i] = P;
        ML_REQUIRE(ab < (1ll << 31) && sb < (1ll << 31), "groupnorm_multi: grid too large");
    }
    st.start[st.n] = (int)sb;
    ap.start[n] = (int)ab;
    hipStream_t s = (hipStream_t)stream;
    if (st.n > 0) hipLaunchKernelGGL(gn_multi_stats_kernel<T>, dim3((unsigned)sb), dim3(GN_TPB), 0, s, st);
    hipLaunchKernelGGL(gn_multi_apply_kernel<T>, dim3((unsigned)ab), dim3(GN_TPB), 0, s, ap);
    ML_CHECK_LAUNCH("groupnorm_multi");
    return ML_OK;
}

extern "C" int ml_groupnorm_multi_f32(const ml_gn_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes,
                                      void *stream) {
    ML_REQUIRE(descs && n >= 1 && n <= ML_GN_MAX_PROBLEMS && workspace, "groupnorm_multi: need 1..%d problems and a workspace",
               ML_GN_MAX_PROBLEMS);
    for (int i = 1; i < n; ++i)
        ML_REQUIRE(descs[i].dtype == descs[0].dtype, "groupnorm_multi: the problems of one launch must share the storage type");
    ML_REQUIRE(descs[0].dtype == 0 || descs[0].dtype == 1, "groupnorm_multi: dtype must be 0 (float) or 1 (half)");
    return descs[0].dtype ? gn_multi<_Float16>(descs, n, workspace, workspace_bytes, stream)
                          : gn_multi<float>(descs, n, workspace, workspace_bytes, stream);
}

template <class T>
static int gn_single(const T *x, T *y, const float *gamma, const float *beta, int32_t N, int64_t HWC, int32_t C, int32_t G,
                     float eps, int32_t relu, int32_t out_cstride, int32_t out_coff, void *workspace, void *stream) {
    constexpr int W = VW<T>::value;
    ML_REQUIRE(workspace, "groupnorm: null pointer");
    if (int rc = gn_validate(x, y, N, HWC, C, G, out_cstride, out_coff)) return rc;
    if ((long long)N * G >= 65536) {         // more chunks than grid.y holds: the one-dimensional launch pair, same bits
        ml_gn_desc d = {};
        d.x = reinterpret_cast<const float *>(x); d.y = reinterpret_cast<float *>(y); d.gamma = gamma; d.beta = beta;
        d.HWC = HWC; d.N = N; d.C = C; d.G = G; d.relu = relu; d.out_cstride = out_cstride; d.out_coff = out_coff; d.eps = eps;
        return gn_multi<T>(&d, 1, workspace, ml_groupnorm_workspace_bytes(N, G), stream);
    }
    const long long L = HWC / G;
    const bool vec = (L % W == 0) && (C % W == 0) && (out_cstride % W == 0) && (out_coff % W == 0) &&
                     ml_aligned16(x) && ml_aligned16(y);
    const GnPlan plan = gn_plan(L, N * G, vec ? W : 4);
    hipStream_t s = (hipStream_t)stream;
    double *ws = reinterpret_cast<double *>(workspace);
    const dim3 grid(plan.S, N * G);
    if (vec && L <= GN_ONEPASS_MAX) {
        // one pass, chunk in registers: vectors per thread chosen so that 256 * VPT * W >= L
        const int NG = N * G, Li = (int)L;
        const int vn = (Li + W - 1) / W;
#define GN1(TPB, VPT) launch_onepass<T, TPB, VPT>(x, y, gamma, beta, NG, Li, C, G, eps, relu, out_cstride, out_coff, s)
        if (vn <= 256) GN1(256, 1);
        else if (vn <= 512) GN1(256, 2);
        else if constexpr (W == 4) GN1(256, 4);
#undef GN1
    } else if (vec) {
        hipLaunchKernelGGL((gn_stats_kernel<T, true>), grid, dim3(GN_TPB), 0, s, x, ws, L, plan.slice, plan.S);
        hipLaunchKernelGGL((gn_apply_kernel<T, true>), grid, dim3(GN_TPB), 0, s, x, y, gamma, beta, ws, L, plan.slice, plan.S, C,
                           G, eps, relu, out_cstride, out_coff);
    } else {
        hipLaunchKernelGGL((gn_stats_kernel<T, false>), grid, dim3(GN_TPB), 0, s, x, ws, L, plan.slice, plan.S);
        hipLaunchKernelGGL((gn_apply_kernel<T, false>), grid, dim3(GN_TPB), 0, s, x, y, gamma, beta, ws, L, plan.slice, plan.S,
                           C, G, eps, relu, out_cstride, out_coff);
    }
    ML_CHECK_LAUNCH("groupnorm");
    return ML_OK;
}

extern "C" int ml_groupnorm_chunk_f32(const float *x, float *y, const float *gamma, const float *beta, int32_t N,
                                      int64_t HWC, int32_t C, int32_t G, float eps, int32_t relu, int32_t out_cstride,
                                      int32_t out_coff, void *workspace, void *stream) {
    return gn_single<float>(x, y, gamma, beta, N, HWC, C, G, eps, relu, out_cstride, out_coff, workspace, stream);
}

extern "C" int ml_groupnorm_chunk_f16(const void *x, void *y, const float *gamma, const float *beta, int32_t N,
                                      int64_t HWC, int32_t C, int32_t G, float eps, int32_t relu, int32_t out_cstride,
                                      int32_t out_coff, void *workspace, void *stream) {
    return gn_single<_Float16>(reinterpret_cast<const _Float16 *>(x), reinterpret_cast<_Float16 *>(y), gamma, beta, N, HWC, C,
                               G, eps, relu, out_cstride, out_coff, workspace, stream);
}
