// Re-packing stepped weights on the device: master weights in the Keras layout -> every packed form a layer's kernels read,
// written in place, all layers of a call in one launch (include/masklab_hip.h: "Re-pack").  The forms are defined by the
// host functions of masklab_hip/packing.py and ops.DeviceConv; this file restates each of them, bit for bit.
//
// One work unit = a [32 outputs n][32 channels c][taps] tile of a job's master, staged once in LDS and written out to every
// form of both orientations the job asks for:
//   forward     wgt[n][tap][c]                 lanes run along c: a half wave writes one 128-byte segment
//   transposed  wgt'[c][taps - 1 - tap][n]     lanes run along n: the same, on the other axis of the tile
// so neither side gathers with a stride.  The tile is [tap][c][n] floats with a pitch of 33: lanes along n read consecutive
// banks, lanes along c read banks 33 apart -- both free of conflicts.  3x3 and smaller kernels stage all taps at once (9 x 32
// x 33 floats = 37 KB, which the Winograd transform needs); 5x5 kernels go in runs of nine taps.  The master is loaded with
// lanes along whichever of its two channel axes has stride 1 (cout for Conv2D, cin for Conv2DTranspose).
// The tile grid of a job covers the largest padded extent any of its forms has, and a tile writes every form's elements
// inside that form's own extent, zeros for what lies past the master: every element of every destination is written exactly
// once, by one lane, whatever the memory held.  A job with a bias has one more unit (the bias copy, repeated `bias_reps`
// times); a table job (the fused mask tail's lane table and padded bias) is one unit.
// A block finds its unit's job by bisection over the table's first_unit, as the optimizer's apply kernel finds a chunk's tensor.
// No atomics, no workspace, plain vector stores.  Compiled with FP contraction off (Makefile): w - hi(w) of the split form and
// the fp64 sums of G g G^T are the operations written here, one rounding each.
#include "common.h"
#include "ranges.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int RP_TPB = 256;
constexpr int RP_T = 32;                 // tile edge, outputs and channels
constexpr int RP_PITCH = RP_T + 1;
constexpr int RP_TAPS = 9;               // taps staged at a time
constexpr int RP_WINO_BLOCK = 8 * 32 * 16;   // floats of one (32-output block, 8-channel chunk) of the Winograd form

typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) unsigned gword;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

// two floats -> the halves (lo 16 bits: a) of hi(w) or of 2^11 (w - hi(w)), round to nearest even both times
__device__ __forceinline__ unsigned rp_half_pair(const float a, const float b) {
    const f16x2 h = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ unsigned rp_split_word(const float a, const float b, const bool low) {
    if (!low) return rp_half_pair(a, b);
    const float ra = (a - (float)(_Float16)a) * 2048.f, rb = (b - (float)(_Float16)b) * 2048.f;
    return rp_half_pair(ra, rb);
}

// U = G g G^T in fp64, rounded once; g[3 i + j], U[4 a + b]
// Summed in the order of the host's einsum: from +0.0, the terms (G[a][i] g[i][j]) G[b][j] in ascending (i, j).  Unlike the
// einsum it leaves out the terms whose coefficient is zero.  For finite weights that changes no bit (they add +-0.0 to a sum
// that started at +0.0); for an Inf or NaN weight it does: the host's 0 * Inf makes every position of that (c, n) pair NaN,
// here only the positions whose coefficient is not zero become Inf / NaN.  Either way the bad weight stays loud.  Starting at
// +0.0 matters: a lone -0.0 weight gives +0.0, as on the host.
__device__ __forceinline__ void rp_winograd(const float *g, float *U) {
    constexpr double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (G[a][i] != 0.0 && G[b][j] != 0.0) acc += (G[a][i] * (double)g[3 * i + j]) * G[b][j];
            U[4 * a + b] = (float)acc;
        }
}

__device__ __forceinline__ void rp_store16(gfloat *dst, const float *U) {
#pragma unroll
    for (int v = 0; v < 4; ++v) ((gf32x4 *)dst)[v] = (f32x4){U[4 * v], U[4 * v + 1], U[4 * v + 2], U[4 * v + 3]};
}

// One orientation of a tile.  TR = false: rows are outputs n, the K axis is c; TR = true: rows are c, K is n and the taps run
// backwards.  `row0` / `k0`: the tile's first row / K index in this orientation; tile element (tap t, row r, K index k) is
// tile[t][k][r] for the forward side and tile[t][r][k] for the transposed one.
template <bool TR>
__device__ __forceinline__ void rp_write_side(const float (*tile)[RP_T][RP_PITCH], const int tid, const int tap0, const int ntap,
                                              const int taps, const int row0, const int k0, float *wgt, float *wgt_x3,
                                              void *wgt_h, float *wgt_wino, const int n_pad, const int span_pad,
                                              const int span_pad_h) {
    auto at = [&](int t, int r, int k) -> float { return TR ? tile[t][r][k] : tile[t][k][r]; };
    auto tap_of = [&](int t) -> int { return TR ? taps - 1 - (tap0 + t) : tap0 + t; };
    const int lane = tid & 31;
    if (wgt && row0 < n_pad && k0 < span_pad) {
        gfloat *dst = (gfloat *)wgt;
        for (int i = tid >> 5; i < ntap * RP_T; i += RP_TPB / 32) {
            const int t = i >> 5, r = i & 31;
            if (row0 + r < n_pad)
                dst[((long long)(row0 + r) * taps + tap_of(t)) * span_pad + k0 + lane] = at(t, r, lane);
        }
    }
    if (wgt_x3 && row0 < n_pad && k0 < span_pad) {
        gword *dst = (gword *)wgt_x3;
        const int q = 2 * (lane & 15);
        for (int i = tid >> 5; i < ntap * RP_T; i += RP_TPB / 32) {
            const int t = i >> 5, r = i & 31;
            if (row0 + r < n_pad)
                dst[((long long)(row0 + r) * taps + tap_of(t)) * span_pad + k0 + lane] =
                    rp_split_word(at(t, r, q), at(t, r, q + 1), lane >= 16);
        }
    }
    if (wgt_h && row0 < n_pad && k0 < span_pad_h) {
        gword *dst = (gword *)wgt_h;                        // two halves a word
        const int w = tid & 15;
        for (int i = tid >> 4; i < ntap * RP_T; i += RP_TPB / 16) {
            const int t = i >> 5, r = i & 31;
            if (row0 + r < n_pad)
                dst[(((long long)(row0 + r) * taps + tap_of(t)) * span_pad_h + k0) / 2 + w] =
                    rp_half_pair(at(t, r, 2 * w), at(t, r, 2 * w + 1));
        }
    }
    // [row block][K chunk of 8][8][32 rows][16]: this tile is four whole chunks of one row block, 64 KB in a piece.  A lane
    // stores the 16 positions of its (k, r) pair from its own registers: four 16-byte stores, 64 bytes apart from lane to lane.
    // Exchanging them through LDS so that a wave's store instruction writes 1 KB in one piece cut the L2 write requests and
    // was SLOWER (0.125 against 0.114 ms over the head convolutions; DESIGN.md, "Re-pack"): L2 merges the pieces of a line.
    if (wgt_wino && tap0 == 0 && row0 < max(n_pad, 128) && k0 < span_pad) {
        gfloat *dst = (gfloat *)wgt_wino + ((long long)(row0 / 32) * (span_pad / 8) + k0 / 8) * RP_WINO_BLOCK;
        for (int i = tid; i < RP_T * RP_T; i += RP_TPB) {
            const int r = i & 31, k = i >> 5;
            float g[9], U[16];
#pragma unroll
            for (int t = 0; t < 9; ++t) g[t] = at(TR ? 8 - t : t, r, k);
            rp_winograd(g, U);
            rp_store16(dst + (k * 32 + r) * 16, U);
        }
    }
}

__global__ void __launch_bounds__(RP_TPB)
repack_kernel(const ml_repack_job *__restrict__ table, const int n_jobs, const long long total_units) {
    __shared__ float tile[RP_TAPS][RP_T][RP_PITCH];
    const int tid = threadIdx.x;
    for (long long u = blockIdx.x; u < total_units; u += gridDim.x) {
        int lo = 0, hi = n_jobs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[mid].first_unit <= u) lo = mid; else hi = mid - 1;
        }
        const ml_repack_job J = table[lo];
        const long long unit = u - J.first_unit;
        if (unit < 0) continue;
        const gfloat *src = (const gfloat *)J.src;
        const gfloat *src_bias = (const gfloat *)J.src_bias;
        if (J.kind == ML_REPACK_TABLE) {
            // [C / 32][16][2][cp], entry (t, e, half, c) = kernel[32 t + (e & 3) + 8 (e >> 2) + 4 half][c]
            if (unit != 0) continue;
            const int cp = J.cp, total = J.C * cp;
            for (int i = tid; i < total; i += RP_TPB) {
                const int c = i % cp, slot = i / cp, half = slot & 1, e = (slot >> 1) & 15, t = slot >> 5;
                const int ch = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * half;
                ((gfloat *)J.table)[i] = c < J.N ? src[(long long)ch * J.s_c + (long long)c * J.s_n] : 0.f;
            }
            if (J.table_bias)
                for (int c = tid; c < cp; c += RP_TPB) ((gfloat *)J.table_bias)[c] = (c < J.N && src_bias) ? src_bias[c] : 0.f;
            continue;
        }
        const long long tiles = (long long)J.nb * J.cb;
        if (unit >= tiles) {
            if (unit == tiles && J.bias)
                for (int i = tid; i < J.bias_n * J.bias_reps; i += RP_TPB) ((gfloat *)J.bias)[i] = src_bias[i % J.bias_n];
            continue;
        }
        const int n0 = (int)(unit / J.cb) * RP_T, c0 = (int)(unit % J.cb) * RP_T;
        const int taps = J.KH * J.KW;
        const bool c_fast = J.s_c == 1;
        for (int tap0 = 0; tap0 < taps; tap0 += RP_TAPS) {
            const int ntap = min(RP_TAPS, taps - tap0);
            __syncthreads();                                 // the last run's (or unit's) readers are done
            for (int i = tid; i < ntap * RP_T * RP_T; i += RP_TPB) {
                const int fast = i & 31, slow = (i >> 5) & 31, t = i >> 10;
                const int n = c_fast ? slow : fast, c = c_fast ? fast : slow;
                float v = 0.f;
                if (n0 + n < J.N && c0 + c < J.C)
                    v = src[(long long)(tap0 + t) * J.s_tap + (long long)(c0 + c) * J.s_c + (long long)(n0 + n) * J.s_n];
                tile[t][c][n] = v;
            }
            __syncthreads();
            rp_write_side<false>(tile, tid, tap0, ntap, taps, n0, c0, J.fwd_wgt, J.fwd_x3, J.fwd_h, J.fwd_wino, J.fwd_n_pad,
                                 J.fwd_span_pad, J.fwd_span_pad_h);
            rp_write_side<true>(tile, tid, tap0, ntap, taps, c0, n0, J.tr_wgt, J.tr_x3, J.tr_h, J.tr_wino, J.tr_n_pad,
                                J.tr_span_pad, J.tr_span_pad_h);
        }
    }
}

struct rp_range {
    const void *p;
    long long bytes;
    int job;
    bool dst;
    const char *name;
};

inline int rp_round_up(int v, int m) { return (v + m - 1) / m * m; }

// one orientation's checks and its destinations; rows / depth: the real extents in this orientation
int rp_check_side(int i, const char *side, int rows, int depth, int taps, bool k3, float *wgt, float *x3, void *h, float *wino,
                  int n_pad, int span_pad, int span_pad_h, std::vector<rp_range> &ranges, int &row_blocks, int &k_blocks) {
    row_blocks = k_blocks = 0;
    if (!wgt && !x3 && !h && !wino) return ML_OK;
    ML_REQUIRE(n_pad >= rows && n_pad % 32 == 0, "repack_plan: job %d: %s n_pad %d must be a multiple of 32 and at least %d", i, side,
               n_pad, rows);
    ML_REQUIRE(span_pad >= depth && span_pad % 32 == 0, "repack_plan: job %d: %s span_pad %d must be a multiple of 32 and at least %d",
               i, side, span_pad, depth);
    ML_REQUIRE(!h || (span_pad_h >= depth && span_pad_h % 64 == 0),
               "repack_plan: job %d: %s span_pad_h %d must be a multiple of 64 and at least %d", i, side, span_pad_h, depth);
    ML_REQUIRE(!wino || k3, "repack_plan: job %d: winograd packing needs a dense 3x3 conv (%s side)", i, side);
    ML_REQUIRE(!wino || ml_aligned16(wino), "repack_plan: job %d: the %s winograd form must be 16-byte aligned", i, side);
    ML_REQUIRE(((((uintptr_t)wgt) | ((uintptr_t)x3) | ((uintptr_t)h)) & 3u) == 0, "repack_plan: job %d: %s forms must be 4-byte aligned",
               i, side);
    const long long dense = (long long)n_pad * taps * span_pad * 4;
    if (wgt) ranges.push_back({wgt, dense, i, true, "wgt"});
    if (x3) ranges.push_back({x3, dense, i, true, "wgt_x3"});
    if (h) ranges.push_back({h, (long long)n_pad * taps * span_pad_h * 2, i, true, "wgt_h"});
    if (wino) ranges.push_back({wino, (long long)std::max(n_pad, 128) * span_pad * 16 * 4, i, true, "wgt_wino"});
    row_blocks = std::max(n_pad, wino ? 128 : 0) / 32;
    k_blocks = std::max(span_pad, h ? span_pad_h : 0) / 32;
    return ML_OK;
}

}  // namespace

extern "C" int64_t ml_repack_plan(ml_repack_job *host_table, int32_t n) {
    ML_REQUIRE(n >= 0 && (host_table || n == 0), "repack_plan: need a table of n >= 0 jobs");
    std::vector<rp_range> ranges;
    int64_t units = 0;
    for (int i = 0; i < n; ++i) {
        ml_repack_job &J = host_table[i];
        ML_REQUIRE(J.kind == ML_REPACK_CONV || J.kind == ML_REPACK_TABLE, "repack_plan: job %d: kind must be ML_REPACK_CONV or _TABLE", i);
        ML_REQUIRE(J.cpp_shift == 30, "repack_plan: job %d: a row-span (image_input) packing is not re-packed on the device", i);
        ML_REQUIRE(J.group_cin_step == 0, "repack_plan: job %d: a grouped packing is not re-packed on the device", i);
        ML_REQUIRE(J.KH >= 1 && J.KW >= 1 && J.KH <= 5 && J.KW <= 5, "repack_plan: job %d: %d x %d taps; at most 5 x 5 are built", i, J.KH,
                   J.KW);
        ML_REQUIRE(J.src && J.N >= 1 && J.C >= 1 && J.s_n >= 1 && J.s_c >= 1 && J.s_tap >= 0,
                   "repack_plan: job %d: needs a master with N, C >= 1 and positive strides", i);
        ML_REQUIRE(((uintptr_t)J.src & 3u) == 0 && ((uintptr_t)J.src_bias & 3u) == 0, "repack_plan: job %d: the master must be 4-byte aligned", i);
        const int taps = J.KH * J.KW;
        const long long src_floats = (long long)(taps - 1) * J.s_tap + (long long)(J.C - 1) * J.s_c + (long long)(J.N - 1) * J.s_n + 1;
        ranges.push_back({J.src, src_floats * 4, i, false, "kernel"});
        ML_REQUIRE(J.kind == ML_REPACK_TABLE || !J.src_bias || J.bias_n >= 1, "repack_plan: job %d: a master bias needs bias_n >= 1", i);
        if (J.src_bias) ranges.push_back({J.src_bias, (long long)(J.kind == ML_REPACK_TABLE ? J.N : J.bias_n) * 4, i, false, "bias"});
        J.first_unit = units;
        if (J.kind == ML_REPACK_TABLE) {
            ML_REQUIRE(taps == 1 && J.C % 32 == 0 && J.N <= 32, "repack_plan: job %d: fused mask-head tail needs a 1x1 kernel, C_mid %% 32 == 0 "
                       "and at most 32 classes", i);
            int cp = 1;
            while (cp < J.N) cp *= 2;
            ML_REQUIRE(J.table && J.cp == cp, "repack_plan: job %d: the table needs a destination and cp = %d, the power of two >= %d", i, cp, J.N);
            ML_REQUIRE(!J.fwd_wgt && !J.fwd_x3 && !J.fwd_h && !J.fwd_wino && !J.tr_wgt && !J.tr_x3 && !J.tr_h && !J.tr_wino && !J.bias,
                       "repack_plan: job %d: a table job has no conv forms", i);
            ranges.push_back({J.table, (long long)J.C * cp * 4, i, true, "table"});
            if (J.table_bias) ranges.push_back({J.table_bias, (long long)cp * 4, i, true, "table bias"});
            J.nb = J.cb = 0;
            units += 1;
            continue;
        }
        ML_REQUIRE(J.C % 4 == 0, "repack_plan: job %d: dense conv needs cin %% 4 == 0 (got %d)", i, J.C);
        ML_REQUIRE(!J.table && !J.table_bias, "repack_plan: job %d: a conv job has no table", i);
        ML_REQUIRE(!J.bias || (J.src_bias && J.bias_reps >= 1), "repack_plan: job %d: a bias form needs a master bias and bias_reps >= 1", i);
        int fr, fk, tr, tk;
        const bool k3 = J.KH == 3 && J.KW == 3;
        int st = rp_check_side(i, "forward", J.N, J.C, taps, k3, J.fwd_wgt, J.fwd_x3, J.fwd_h, J.fwd_wino, J.fwd_n_pad, J.fwd_span_pad,
                               J.fwd_span_pad_h, ranges, fr, fk);
        if (st != ML_OK) return st;
        st = rp_check_side(i, "transposed", J.C, rp_round_up(J.N, 4), taps, k3, J.tr_wgt, J.tr_x3, J.tr_h, J.tr_wino, J.tr_n_pad,
                           J.tr_span_pad, J.tr_span_pad_h, ranges, tr, tk);
        if (st != ML_OK) return st;
        if (J.bias) ranges.push_back({J.bias, (long long)J.bias_n * J.bias_reps * 4, i, true, "bias"});
        J.nb = std::max(fr, tk);
        J.cb = std::max(fk, tr);
        units += (long long)J.nb * J.cb + (J.bias ? 1 : 0);
    }
    // a destination apart from every master and every other destination (masters may share: the slices of one kernel)
    std::vector<int> order(ranges.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = (int)k;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return (uintptr_t)ranges[a].p < (uintptr_t)ranges[b].p; });
    uintptr_t end = 0;          // the furthest end among the ranges in front, and that of the destinations among them
    int end_at = -1;
    uintptr_t dst_end = 0;
    int dst_at = -1;
    for (int k : order) {
        const rp_range &R = ranges[k];
        const int hit = R.dst ? end_at : dst_at;
        if (hit >= 0 && ml_ranges_overlap(R.p, R.bytes, ranges[hit].p, ranges[hit].bytes)) {
            const rp_range &O = ranges[hit];
            ml_set_error("repack_plan: `%s` of job %d overlaps `%s` of job %d: every destination must lie apart from every master "
                         "and every other destination", R.name, R.job, O.name, O.job);
            return ML_E_BADARG;
        }
        const uintptr_t e = (uintptr_t)R.p + (uintptr_t)R.bytes;
        if (end_at < 0 || e > end) end = e, end_at = k;
        if (R.dst && (dst_at < 0 || e > dst_end)) dst_end = e, dst_at = k;
    }
    return units;
}

extern "C" int ml_repack_f32(const ml_repack_job *table, int32_t n, int64_t total_units, void *stream) {
    ML_REQUIRE(n >= 0 && total_units >= 0 && (table || n == 0), "repack: bad arguments");
    if (n == 0 || total_units == 0) return ML_OK;
    ML_REQUIRE(total_units < (1ll << 31), "repack: %lld work units; fewer than 2^31 fit one launch", (long long)total_units);
    hipLaunchKernelGGL(repack_kernel, dim3((unsigned)total_units), dim3(RP_TPB), 0, (hipStream_t)stream, table, (int)n,
                       (long long)total_units);
    ML_CHECK_LAUNCH("repack");
    return ML_OK;
}
