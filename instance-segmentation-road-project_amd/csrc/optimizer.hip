// The reference's RectifiedAdam and AdamW (engine/optimizers.py) as one step over any number of float32 tensors; the
// formulas and their operation order are in include/masklab_hip.h.  Two launches a step:
//   opt_scalars_kernel  one thread: (iterations, lr) on the device -> the step's scalars (float64 arithmetic, stored as
//                       floats) and the branch flag; iterations += 1.  Nothing of a step is read on the host, so a captured
//                       step replays with the lr and the iteration count of its replay.
//   opt_apply_kernel    pure streaming, 28 B per element (p, g, m, v read; p, m, v written).  The elements of all tensors
//                       are cut into chunks of ML_OPT_CHUNK = 256 lanes x 4 vectors x 4 floats; a block grid-strides over
//                       the chunks and finds a chunk's tensor by bisection over the table's first_chunk (a prefix sum, so
//                       the table has one entry per tensor however large it is).  A lane issues its 16 loads of a chunk
//                       before the first use.  Tensors whose four pointers are not all 16-byte aligned, and the last n mod 4
//                       elements of every tensor, go element by element.  Every element belongs to one lane: no atomics, no
//                       workspace, and the bits do not depend on the grid or on which tensors share the launch.
// This file is compiled with FP contraction off (Makefile): a * b + c below is two roundings, as written.
#include "common.h"

namespace {

constexpr int OPT_TPB = 256;
constexpr int OPT_VPT = ML_OPT_CHUNK / (OPT_TPB * 4);       // 16-byte vectors per lane and array in a chunk
constexpr int OPT_MAX_BLOCKS = 2048;
static_assert(OPT_VPT * OPT_TPB * 4 == ML_OPT_CHUNK, "a chunk is a whole number of vectors per lane");

// The table's pointers are read from memory, so the compiler takes them for generic addresses (flat_load); they are device
// memory by contract: global_load / global_store.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

__global__ void opt_scalars_kernel(int kind, ml_opt_state *state, ml_opt_scalars *out, double b1, double b2, double eps,
                                   double decay, double wd, double init_lr) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long long it = state->iterations;
    const double t = (double)(it + 1);
    double lr = (double)state->lr;
    if (decay > 0) lr = lr / (1.0 + decay * (double)it);
    const double b1t = pow(b1, t), b2t = pow(b2, t);
    ml_opt_scalars s = {};
    s.beta_1 = (float)b1; s.one_minus_beta_1 = (float)(1.0 - b1);
    s.beta_2 = (float)b2; s.one_minus_beta_2 = (float)(1.0 - b2);
    s.epsilon = (float)eps;
    s.lr = (float)lr;
    s.decays = wd != 0.0;
    if (kind == ML_OPT_RADAM) {
        const double nmax = 2.0 / (1.0 - b2) - 1.0;
        const double N = nmax - 2.0 * t * b2t / (1.0 - b2t);
        s.rectified = N > 5.0;
        s.step = (float)(s.rectified ? lr * sqrt((1.0 - b2t) * (N - 4.0) / (nmax - 4.0) * (N - 2.0) / N * nmax / (nmax - 2.0)) / (1.0 - b1t)
                                     : lr / (1.0 - b1t));
        s.wd_lr = (float)(wd * lr);
    } else {
        s.rectified = 1;
        s.lr_t = (float)(lr * sqrt(1.0 - b2t) / (1.0 - b1t));
        s.eta_wd = (float)(lr / init_lr * wd);
    }
    *out = s;
    state->iterations = it + 1;
}

// one element; p, m, v in and out
template <int KIND>
__device__ __forceinline__ void opt_element(const ml_opt_scalars &s, float &p, const float g, float &m, float &v) {
    const float m1 = s.beta_1 * m + s.one_minus_beta_1 * g;
    const float v1 = s.beta_2 * v + s.one_minus_beta_2 * (g * g);
    if (KIND == ML_OPT_RADAM) {
        const float p_ = s.decays ? p - s.wd_lr * p : p;
        p = s.rectified ? p_ - s.step * (m1 / (sqrtf(v1) + s.epsilon)) : p_ - s.step * m1;
    } else {
        p = p - s.lr_t * m1 / (sqrtf(v1) + s.epsilon) - s.eta_wd * p;
    }
    m = m1;
    v = v1;
}

template <int KIND>
__global__ void __launch_bounds__(OPT_TPB)
opt_apply_kernel(const ml_opt_tensor *__restrict__ table, int n_tensors, long long total_chunks,
                 const ml_opt_scalars *__restrict__ scalars) {
    const ml_opt_scalars s = *scalars;
    const int tid = threadIdx.x;
    for (long long c = blockIdx.x; c < total_chunks; c += gridDim.x) {
        // the last tensor whose first_chunk <= c (tensors without elements share their successor's first_chunk)
        int lo = 0, hi = n_tensors - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
        }
        const ml_opt_tensor T = table[lo];
        const long long base = (c - T.first_chunk) * ML_OPT_CHUNK;
        if (base < 0 || base >= T.n) continue;                    // (a table and a chunk count that do not belong together)
        const int count = (int)min((long long)ML_OPT_CHUNK, T.n - base);
        gfloat *p = (gfloat *)(T.p + base), *m = (gfloat *)(T.m + base), *v = (gfloat *)(T.v + base);
        const gfloat *g = (const gfloat *)(T.g + base);
        const bool vec = ((((uintptr_t)T.p) | ((uintptr_t)T.g) | ((uintptr_t)T.m) | ((uintptr_t)T.v)) & 15u) == 0;
        int done = 0;                                             // elements the vector part covers
        if (vec && count >= 4) {
            const int nv = count >> 2;
            done = nv << 2;
            // a lane past the end loads the chunk's last vector and stores nothing: the 16 loads are unconditional, so all
            // of them are in flight before the first wait
            f32x4 P[OPT_VPT], G[OPT_VPT], M[OPT_VPT], V[OPT_VPT];
#pragma unroll
            for (int k = 0; k < OPT_VPT; ++k) {
                const int i = min(k * OPT_TPB + tid, nv - 1);
                P[k] = ((const gf32x4 *)p)[i];
                G[k] = ((const gf32x4 *)g)[i];
                M[k] = ((const gf32x4 *)m)[i];
                V[k] = ((const gf32x4 *)v)[i];
            }
#pragma unroll
            for (int k = 0; k < OPT_VPT; ++k) {
                const int i = k * OPT_TPB + tid;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = P[k][e], me = M[k][e], ve = V[k][e];
                    opt_element<KIND>(s, pe, G[k][e], me, ve);
                    P[k][e] = pe; M[k][e] = me; V[k][e] = ve;
                }
                if (i < nv) {
                    ((gf32x4 *)p)[i] = P[k];
                    ((gf32x4 *)m)[i] = M[k];
                    ((gf32x4 *)v)[i] = V[k];
                }
            }
        }
        // element by element: a misaligned tensor's whole chunk, an aligned one's last n mod 4 elements
        for (int i0 = done; i0 < count; i0 += 4 * OPT_TPB) {
            float pe[4], ge[4], me[4], ve[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = min(i0 + k * OPT_TPB + tid, count - 1);
                pe[k] = p[i]; ge[k] = g[i]; me[k] = m[i]; ve[k] = v[i];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + k * OPT_TPB + tid;
                opt_element<KIND>(s, pe[k], ge[k], me[k], ve[k]);
                if (i < count) { p[i] = pe[k]; m[i] = me[k]; v[i] = ve[k]; }
            }
        }
    }
}

}  // namespace

extern "C" int64_t ml_optimizer_plan(ml_opt_tensor *host_table, int32_t n) {
    ML_REQUIRE(n >= 0 && (host_table || n == 0), "optimizer_plan: need a table of n >= 0 tensors");
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        ml_opt_tensor &T = host_table[i];
        ML_REQUIRE(T.n >= 0, "optimizer_plan: tensor %d has a negative element count", i);
        ML_REQUIRE(T.n == 0 || (T.p && T.g && T.m && T.v), "optimizer_plan: tensor %d has a null pointer", i);
        T.first_chunk = chunks;
        chunks += (T.n + ML_OPT_CHUNK - 1) / ML_OPT_CHUNK;
    }
    return chunks;
}

extern "C" int ml_optimizer_scalars(int32_t kind, ml_opt_state *state, ml_opt_scalars *scalars, double beta_1, double beta_2,
                                    double epsilon, double decay, double weight_decay, double init_lr, void *stream) {
    ML_REQUIRE(kind == ML_OPT_RADAM || kind == ML_OPT_ADAMW, "optimizer_scalars: kind must be ML_OPT_RADAM or ML_OPT_ADAMW");
    ML_REQUIRE(state && scalars, "optimizer_scalars: null pointer");
    ML_REQUIRE(beta_1 >= 0 && beta_1 < 1 && beta_2 >= 0 && beta_2 < 1, "optimizer_scalars: beta_1 and beta_2 must be in [0, 1)");
    ML_REQUIRE(kind != ML_OPT_ADAMW || init_lr != 0, "optimizer_scalars: AdamW divides by init_lr, which is 0");
    hipLaunchKernelGGL(opt_scalars_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, kind, state, scalars, beta_1, beta_2, epsilon,
                       decay, weight_decay, init_lr);
    ML_CHECK_LAUNCH("optimizer_scalars");
    return ML_OK;
}

extern "C" int ml_optimizer_apply_f32(int32_t kind, const ml_opt_tensor *table, int32_t n, int64_t total_chunks,
                                      const ml_opt_scalars *scalars, void *stream) {
    ML_REQUIRE(kind == ML_OPT_RADAM || kind == ML_OPT_ADAMW, "optimizer_apply: kind must be ML_OPT_RADAM or ML_OPT_ADAMW");
    ML_REQUIRE(n >= 0 && total_chunks >= 0 && scalars && (table || n == 0), "optimizer_apply: bad arguments");
    if (n == 0 || total_chunks == 0) return ML_OK;
    const unsigned grid = (unsigned)(total_chunks < OPT_MAX_BLOCKS ? total_chunks : OPT_MAX_BLOCKS);
    if (kind == ML_OPT_RADAM)
        hipLaunchKernelGGL(opt_apply_kernel<ML_OPT_RADAM>, dim3(grid), dim3(OPT_TPB), 0, (hipStream_t)stream, table, (int)n,
                           (long long)total_chunks, scalars);
    else
        hipLaunchKernelGGL(opt_apply_kernel<ML_OPT_ADAMW>, dim3(grid), dim3(OPT_TPB), 0, (hipStream_t)stream, table, (int)n,
                           (long long)total_chunks, scalars);
    ML_CHECK_LAUNCH("optimizer_apply");
    return ML_OK;
}
