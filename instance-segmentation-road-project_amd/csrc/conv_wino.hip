// Winograd F(2x2,3x3) convolution on the gfx950 f32 matrix cores (v_mfma_f32_16x16x4_f32), ML_MATH_F32 only.
//
//   For the stride-1 "same" 3x3 convs of the heads (towers, FPN, semantic / decoder convs): an output 2x2 tile is
//   Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A with d_c the 4x4 input patch of channel c, so the 9 taps x Cin x Cout
//   multiplications of a 2x2 tile (36 per channel pair) become 16 (x2.25 fewer MFMAs).  The transforms hold only 0, +-1,
//   +-1/2 (F(2x2,3x3): Lavin & Gray 2016); the weight transform U = G g G^T is done once on the host in fp64 and rounded
//   once to fp32 (masklab_hip/packing.py: pack_winograd).  Per position p = 4a + b the 16 products are independent
//   GEMMs  M_p[tiles, Cout] = V_p[tiles, Cin] . U_p[Cin, Cout], accumulated over the whole K loop (no split-K).
//
//   Block = 512 threads = 8 waves, one block per CU; block tile = 64 Winograd tiles (flattened over image, tile row, tile
//   column) x 64 output channels (two 32-channel blocks of the host layout); ceil(cout / 64) such channel blocks per tile block.  Wave w owns tile group tg = w & 3 (tiles
//   16 tg .. 16 tg + 15) x channel half h = w >> 2 (32 channels) x all 16 positions: 2 x 16 accumulators of the 16x16x4
//   MFMA = 128 registers, so the output transform runs in registers (a lane holds all 16 positions of 1 tile x 4
//   channels per 16-wide half: the B fragment is the MFMA's first operand, see Epilogue).  The patches of a tile group are
//   staged once and read by both channel halves.
//   K step = 4 input channels = 32 MFMAs per wave.  Staging is by LDS DMA (buffer_load_dwordx4 ... lds, 16 B per lane, 1 KB
//   per wave instruction) straight from global memory into two rings, with ONE barrier per two K steps:
//     * patches in chunks of 8 channels (two K steps), 3 slots of 32 KB, 4 DMA instructions per wave and chunk.  A slot holds
//       the raw 4x4 patches of the block's 64 tiles as [tg 4][px 16][tile 16][8 ch]; one DMA instruction = 2 px x 16 tiles x
//       8 channels, a pixel's 32 contiguous bytes fetched by two ADJACENT lanes, so the instruction touches 32 lines of 128 B
//       where a 4-channel chunk (one pixel per lane) touched 64: half the texture-path work per staged byte.  The two 16-byte
//       channel quads of tile r sit in the order (q ^ (r >> 2 & 1)): lane (r, kq) reads channel kq of its K step's quad at a
//       per-lane base + px x 512 B (ds_read2st64_b32), and a b32 read's 32-lane group hits 16 banks (2-way, as with the
//       4-channel slots; unswizzled 8-channel tiles would be 4-way).  Out-of-image taps and tiles past the end carry an
//       out-of-range buffer offset and land as zeros;
//     * transformed weights per K step, 4 slots of 16 KB, 2 DMA instructions per wave and step: both channel halves as
//       [h 2][k 4][t 2][pq 4][r 16][4 p] float4s (n = 16 t + r), one DMA instruction = one contiguous 1 KB (k, t) row of the
//       host layout; a b128 read's 16-lane group covers r = 0..15 once: conflict-free.
//   3 x 32 KB + 4 x 16 KB = 160 KB, all of the CU's LDS; the gn_partials exchange (256 B) reuses the ring's head after the
//   loop.  Why these counts: operands are read into registers one K step ahead, so during iteration j (steps 2j, 2j + 1)
//   the waves read patch chunks j and j + 1 and the weights of steps 2j + 1 and 2j + 2 while chunk j + 2 and the weights of
//   steps 2j + 3 and 2j + 4 are written: 3 patch slots and 4 weight slots are the fewest that need no second barrier.  (Two
//   64 KB slots of 8 channels each would have to be written while still being read.)  A DMA has one whole iteration, two K
//   steps, to land: the distance the 4-slot ring of 4-channel chunks gave, now at a shorter step.
//   Iteration j: s_waitcnt vmcnt(0) lgkmcnt(0) (this wave's DMAs of iteration j - 1 have landed, its LDS reads are done);
//   s_barrier (every wave's); then two K steps.  A step is 32 MFMAs on operands that are already in registers AND already
//   transformed, so it opens on the matrix pipe; placed among them and pinned there by sched_barriers:
//     after the 4th MFMA    the LDS reads of the next step (16 patch values + 8 B fragments, into the other register set);
//     after the 6th, 12th.. one DMA instruction each, 6 MFMAs apart: 5 in the iteration's first step (the 4 patch pieces,
//                           which may miss L2, then weights), 3 in its second, the last one 14 MFMAs before the barrier;
//     after the 17th..32nd  two adds each of the next step's input transform B^T d B (32 adds, kept scalar:
//                           -fno-slp-vectorize in the Makefile), in the shadow of this step's MFMAs.
//   The patch resource is rebased per block (its first tap row) and per chunk (+8 channels), so the per-lane offsets are
//   32-bit and constant over the K loop while the tensor itself may exceed 4 GiB (the host checks that a block's rows
//   span less than 2 GiB).  No staging registers and no exec-masked loads; the DMA of the chunks past the last one goes
//   through empty resources, so the loop body is one basic block.
//
//   Costing (per CU: one block, 2 waves per SIMD; 234 VGPRs, no scratch, no spills; 163840 B of LDS):
//     MFMA per K step and SIMD: 2 waves x 16 positions x 2 halves = 64 x 32 cycles = 2048 cycles;
//     VALU per step and wave: 32 transform adds (+ the output transform once per block), 2 per MFMA gap;
//     staged per step and block: 16 KB of patches + 16 KB of weights; per two steps 32 patch DMA instructions of 32 lines
//       and 32 weight DMA instructions of 8 lines;
//     LDS reads per step and wave: 16 x b32 + 8 x b128 = 6 KB for 32 MFMAs.
//   Where a step's time went before this layout (profiles/r09_wino_staging.md; one K step measured as the difference of the
//   160- and 128-channel launches of the same 1024-block grid, / 8 steps / 4 rounds): 1.54 us = ~3700 cycles at 2.4 GHz
//   for 2048 cycles of MFMA.  With the patch DMAs sent through empty resources (same instructions, no line fetched) the
//   old kernel took 1.20 us per step, with the weight DMAs 1.60 (no change), with its 4 DMAs moved from the step's head to
//   after the 16th MFMA 1.23: the loss was the patch DMAs' texture-path work, queued by all 8 waves at the head of every
//   step in front of their MFMAs.  This kernel: 1.21 us per step (~2900 cycles); with empty patch resources 1.10, with
//   every DMA empty 1.05; with a step's DMAs in one burst at its head instead of spread 1.31.  So halving the lines per
//   patch instruction and spreading the issue each pay, ~0.1 us of texture-path queueing is left, and ~480 cycles per step
//   beyond the MFMAs remain with no memory traffic at all (barrier, LDS reads, transform).  s_setprio 1 for waves 4-7
//   measured as no gain and is left out; a second copy of the loop with another DMA phase for waves 4-7 spills.
//   Against the direct kernel (conv_mfma.hip, 9 x 128 / 32 = 36 chunks of 64 32x32x2 MFMAs per 128 x 128 tile): the
//   same output takes 16 / 36 of the MFMA cycles.
//
//   Channel blocks and the dead half (profiles/r14_wino_narrow.md).  The weight layout is always four 32-output blocks
//   (n_pad = 128, rows >= cout zero), but a problem is given NB = ceil(cout / 64) channel blocks per 64-tile block, not
//   n_pad / 64: a block whose 64 channels are all >= cout is never launched.  In a launched block whose second 32-channel
//   half lies wholly >= cout (cout <= 32, or 65..96: the 75-channel class output of the towers), waves 4-7 run a second
//   copy of the K loop, chosen once before the loop by a wave-uniform branch: their 4 patch DMA instructions per
//   iteration (the patches serve both halves), their 4 weight DMA instructions through an empty resource, the same
//   s_waitcnt and s_barrier -- so the rings, the counted waits and the barriers per iteration are those of the live
//   loop for all eight waves -- and no B-fragment or patch read, no transform, no MFMA, no epilogue.  Their DMAs are
//   s_sleep 3 (~192 cycles, the live loop's 6 MFMAs) apart, not a burst.  Wave w + 4 shares a SIMD with wave w, so a
//   dead half leaves that SIMD 1024 instead of 2048 cycles of MFMA per K step.  The live loop is the same instruction
//   sequence as before, and every cout = 128 launch gives the same bits.  Which narrow classes run here instead of on the
//   direct kernel is decided per cout class by measurement and written as cout ranges in ml_conv2d_wino_narrow below,
//   never as a launch-size heuristic.  Measured, the towers' five-level output launch of 8 x 1024^2 alone on the chip, direct
//   kernel -> this one, two runs each: cout 32 (one block, dead half) 152-154 -> 108-109 us; 60 (one block) 258-261 ->
//   156-159; 75 (two blocks, the second half-dead, sigmoid) 412-414 -> 290-295; 96 393-397 -> 277-278; the full 128 -> 128
//   tower launch takes 280-290.  So a half-dead block costs 0.69 of a full one (0.65 was the estimate from 1024 of 2048 MFMA
//   cycles plus the step's 0.20-0.36 us beyond them), and all three classes (<= 32, 33..64, 65..96) are faster here; the
//   predicate leaves out only cout = 32 and 64 themselves, for the reason given there.
//
//   Epilogue (profiles/r18_wino_epilogue.md).  v_mfma_f32_16x16x4_f32 takes one float per lane for each operand with the
//   same lane map [l & 15][l >> 4], so with the B fragment as its FIRST operand and the transformed patch value as its
//   second the 16 x 16 tile comes out transposed -- the same products in the same k order, the same bits -- and lane
//   (r, kq) owns tile 16 tg + r and channels 16 t + 4 kq .. + 3 of its half as the four floats of each accumulator.  So: one
//   set of tile-to-address arithmetic per lane (it was four), Y = A^T M A on f32x4 values, bias as one 16-byte load, and per
//   half and output pixel one 16-byte store with the generic addressing (out_coff / out_cstride / out_bstride): 8 store
//   instructions per lane where the tile-major accumulators needed 32 dword stores.  The 16-byte accesses are dword-aligned
//   (f32x4d: the hardware's global_store_dwordx4 asks no more), so the class tower's output at a channel stride of 75 and
//   an out_view offset that is no multiple of 4 take the same path as a dense 128-wide tensor.  Only a quad that reaches
//   past cout (cout % 4 != 0: 72..74 of 75) is stored channel by channel; a quad wholly past cout stores nothing.
//   Measured against the dword epilogue, alternating in one job: the 128^2 launch 204-206 -> 194-197 us, the tower launch
//   287-291 -> 278-280, cout 75 293-296 -> 282-285, cout 60 157-159 -> 151; with the stores sent through an empty resource
//   (make wino-exp, bit 3) either epilogue loses another 4-8 us per launch, so what the rewrite saved is issue and address
//   work, not bytes.
//   gn_partials: on the geometries where a block covers exactly two whole 128-pixel flattened tiles (host check
//   wino_gn_ok), slots 2 nt2 + h (the block's two 32-channel groups) of each of them get that group's (sum, sum of
//   squares) in fp64: a lane adds the 2 halves x 4 channels x 4 pixels it stores, each value widened first, the wave folds
//   its lanes, and the group's 4 waves are added in tile-group order; the 2 blocks of cout = 128 fill all 4 slots.  About
//   6 us of a tower launch (bit 4 of WINO_EXP skips it).  Output addressing is 64-bit.  Several problems (pyramid levels) per
//   launch; no host reads, no allocation: capturable in a hipGraph.  Fixed-capacity RoI batches (`live`): blocks that hold
//   only non-existing images return at once, so a mask-head conv runs on the same kernel (same bits) with or without
//   `live`.
#include "gfx_mem.h"

namespace {

constexpr int WMAXP = ML_CONV_MAX_PROBLEMS;
constexpr int WT = 64;        // Winograd tiles per block
constexpr int WN = 64;        // output channels per block
constexpr int WK = 8;         // input channels per 8-channel block of the host weight layout = one patch chunk (two K steps)
constexpr int WCHUNK = WK * 32 * 16;   // floats of transformed weights per (32-channel block, 8-channel block) of the host layout
constexpr int WSTEP = 4 * 32 * 16;     // floats of transformed weights per (32-channel block, 4-channel K step)
constexpr int NSLOT_P = 3;             // patch ring: slots of one 8-channel chunk (two K steps) each
constexpr int SLOT_P = WT * 16 * 8;    // floats of patches per patch slot (32 KB)
constexpr int NSLOT_W = 4;             // weight ring: slots of one 4-channel K step each
constexpr int SLOT_W = 2 * WSTEP;      // floats of weights per weight slot (both channel halves, 16 KB)
constexpr int RING_W = NSLOT_P * SLOT_P;   // the weight ring follows the patch ring
constexpr int LDS_BYTES = (RING_W + NSLOT_W * SLOT_W) * 4;   // 160 KB: all of a CU's LDS; the gn exchange reuses its head
static_assert(LDS_BYTES == 160 * 1024, "the two rings fill the CU's LDS");
// Experiment builds (make wino-exp; never the default library): WINO_EXP bit 0 sends the patch DMAs, bit 1 the weight
// DMAs through empty resources (same instructions, no line fetched, WRONG outputs: for timing only); WINO_EXP = 4 issues
// a step's DMAs in one burst at the step's head instead of spread through its MFMAs.  Two bits split the time outside the
// K loop: bit 3 (8) sends the epilogue's stores through an empty buffer resource (the same count and width of store
// instructions, no byte written), bit 4 (16) skips the gn_partials sums and their exchange.
#ifndef WINO_EXP
#define WINO_EXP 0
#endif
constexpr unsigned OOB = 0x80000000u;  // buffer offset of an out-of-image tap: >= the patch resource's num_records
constexpr long long SPAN_MAX = 0x7fffff00ll;   // bytes a block's patch offsets may reach (< OOB)

struct WProblem {
    ml_conv2d_desc d;
    int TH, TW, T;            // tile rows / columns per image, tiles in all (B * TH * TW)
    int MB, NB, nchunks;      // 64-tile blocks, 64-channel blocks, 8-channel chunks (2 K steps each)
};

struct WArgs {
    int n;
    int start[WMAXP + 1];     // prefix sum of blocks per problem
    WProblem p[WMAXP];
};

// Four consecutive channels of one pixel at a dword-aligned address: a channel stride or offset that is no multiple of 4
// (the 75 classes written into cls_pred) takes the same 16-byte global instruction as an aligned destination.
typedef f32x4 f32x4d __attribute__((aligned(4)));

// One store of the epilogue (a float, or the four channels of a lane).  WINO_EXP bit 3: as a buffer store through
// an empty resource, which the hardware drops.
__device__ __forceinline__ void out_store(float *base, float *ptr, float val) {
#if (WINO_EXP & 8) && defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t none = rsrc_bytes(base, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), none, (int)((ptr - base) * 4), 0, 0);
#else
    *ptr = val;
#endif
}
__device__ __forceinline__ void out_store(float *base, float *ptr, f32x4 val) {
#if (WINO_EXP & 8) && defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t none = rsrc_bytes(base, 0);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, val), none, (int)((ptr - base) * 4), 0, 0);
#else
    *reinterpret_cast<f32x4d *>(ptr) = val;
#endif
}

// Operation k of 32 of V = B^T d B, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1] (d, t, v row-major 4x4): 0..15 the column
// pass t = B^T d (column k >> 2), 16..31 the row pass v = t B (row (k - 16) >> 2).  One add each, so the K loop can place
// them singly among its MFMAs; k is a constant after unrolling.
__device__ __forceinline__ void bt_d_b_op(int k, const float d[16], float t[16], float v[16]) {
    if (k < 16) {
        const int j = k >> 2;
        switch (k & 3) {
            case 0: t[0 * 4 + j] = d[0 * 4 + j] - d[2 * 4 + j]; break;
            case 1: t[1 * 4 + j] = d[1 * 4 + j] + d[2 * 4 + j]; break;
            case 2: t[2 * 4 + j] = d[2 * 4 + j] - d[1 * 4 + j]; break;
            default: t[3 * 4 + j] = d[1 * 4 + j] - d[3 * 4 + j]; break;
        }
    } else {
        const int i = (k - 16) >> 2;
        switch (k & 3) {
            case 0: v[i * 4 + 0] = t[i * 4 + 0] - t[i * 4 + 2]; break;
            case 1: v[i * 4 + 1] = t[i * 4 + 1] + t[i * 4 + 2]; break;
            case 2: v[i * 4 + 2] = t[i * 4 + 2] - t[i * 4 + 1]; break;
            default: v[i * 4 + 3] = t[i * 4 + 1] - t[i * 4 + 3]; break;
        }
    }
}

__global__ void __launch_bounds__(512, 1) conv_wino_kernel(const WArgs args) {
    extern __shared__ __align__(16) float lds[];       // ONE LDS object: the patch ring, then the weight ring

    int pi = 0;
    while (pi + 1 < args.n && (int)blockIdx.x >= args.start[pi + 1]) ++pi;
    const WProblem &P = args.p[pi];
    const ml_conv2d_desc &p = P.d;
    // blocks that share one 64-tile panel get ids congruent mod 8 (the same XCD / L2)
    const int b = (int)blockIdx.x - args.start[pi];
    const int g = b / (8 * P.NB), rr = b - g * 8 * P.NB;
    const int nt2 = rr >> 3;
    const int mt = g * 8 + (rr & 7);
    if (mt >= P.MB) return;
    if (p.live) {
        // fixed-capacity RoI batch: image i exists iff i % live_period < max(1, *live); a block of non-existing images only
        // computes and stores nothing (block-uniform)
        const int lv = max(1, *p.live), tpi0 = P.TH * P.TW;
        const int b0 = mt * WT / tpi0, b1 = min(mt * WT + WT, P.T) - 1;
        bool any = false;
        for (int bi = b0; bi <= b1 / tpi0 && !any; ++bi) any = bi % p.live_period < lv;
        if (!any) return;
    }

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tg = wave & 3, h = wave >> 2;            // compute role: tile group x channel half
    const int r = lane & 15, kq = lane >> 4;
    const int tpi = P.TH * P.TW;

    // ---- staging geometry (constant over the K loop).  Patch pieces of this wave: tile group wave >> 1, px pairs
    // 4 (wave & 1) + i; lane l: px = 8 (wave & 1) + 2 i + (l >> 5), tile 16 (wave >> 1) + rt with rt = (l >> 1) & 15, channel
    // quad (l & 1) ^ (rt >> 2 & 1) of the chunk's 8 channels: a lane pair fetches one pixel's 32 contiguous bytes.
    const int gt0 = mt * WT;
    long long base_pix;                                // the block's first tap row, flattened (b * H + y) * W
    {
        const int bi = gt0 / tpi, rem = gt0 - bi * tpi, ty = rem / P.TW;
        base_pix = ((long long)bi * p.H + max(2 * ty - 1, 0)) * p.W;
    }
    const size_t cstride = (size_t)p.in_cstride;
    const float *pin = p.in + p.in_coff + (size_t)base_pix * cstride;
    int voff_p[4];
    {
        const int rt = (lane >> 1) & 15;
        const int quad = (lane & 1) ^ ((rt >> 2) & 1);
        const int gt = gt0 + (wave >> 1) * 16 + rt;
        int bi = 0, ty = 0, tx = 0;
        if (gt < P.T) {
            bi = gt / tpi;
            const int rem = gt - bi * tpi;
            ty = rem / P.TW;
            tx = rem - ty * P.TW;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int px = 8 * (wave & 1) + 2 * i + (lane >> 5);
            const int y = 2 * ty - 1 + (px >> 2), x = 2 * tx - 1 + (px & 3);
            voff_p[i] = (int)OOB;
            if (gt < P.T && y >= 0 && y < p.H && x >= 0 && x < p.W)
                voff_p[i] = (int)((((long long)bi * p.H + y) * p.W + x - base_pix) * (long long)cstride * 4) + quad * 16;
        }
    }
    // weight pieces of this wave: channel half wave >> 2, k row wave & 3, t = i (+1024 B); lane (pq = lane >> 4, r)
    // takes host float4 (16 t + r) * 4 + pq of that k row.  A K step of 4 channels is half an 8-channel block of the host
    // layout, so step s of a 32-channel block starts s * WSTEP floats in.
    const int voff_w = ((wave & 3) * 512 + r * 16 + kq * 4) * 4;
    const float *wsrc = p.wgt + (size_t)(2 * nt2 + (wave >> 2)) * P.nchunks * WCHUNK;
    float *dst_p = lds + (wave >> 1) * 2048 + (wave & 1) * 1024;
    float *dst_w = lds + RING_W + (wave >> 2) * WSTEP + (wave & 3) * 512;
    const int nch = P.nchunks, nsteps = 2 * P.nchunks;
    // A half whose 32 channels are all >= cout (only h = 1: blocks are launched for ceil(cout / 64) channel blocks, so a
    // launched block's first half is live) is dead: its waves stage their share of the patches and go through every wait
    // and barrier of the loop, and do nothing else.  Wave-uniform.
    const bool dead = (2 * nt2 + h) * 32 >= p.cout;

    // resources of patch chunk j (8 channels) and of the weights of K step s; past the end empty (nothing lands, nothing
    // of it is used), so the loop body is one basic block.  The weights of a dead half: empty too (this wave's weight DMAs
    // fill the rows of its own half h, which nobody reads)
    auto rsrc_p = [&](int j) __attribute__((always_inline)) {
        const bool real = j < nch && !(WINO_EXP & 1);
        return rsrc_bytes(pin + j * 8, real ? (int)OOB : 0);
    };
    auto rsrc_w = [&](int s) __attribute__((always_inline)) {
        const bool real = s < nsteps && !dead && !(WINO_EXP & 2);
        return rsrc_bytes(wsrc + (size_t)s * WSTEP, real ? WSTEP * 4 : 0);
    };

    f32x4 acc[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};

    // lane (r, kq) reads channel kq of K step `half` of tile r: its quad sits at 4 (half ^ (r >> 2 & 1)) of the tile's 8
    const float *pa_lane0 = lds + tg * 2048 + r * 8 + 4 * ((r >> 2) & 1) + kq;          // + px * 128
    const float *pa_lane1 = lds + tg * 2048 + r * 8 + 4 * (((r >> 2) & 1) ^ 1) + kq;
    const float *pb_lane = lds + RING_W + h * WSTEP + kq * 512 + r * 4;                 // + t * 256 + pq * 64
    // the LDS operands of one K step: the lane's 16 patch values (d, transformed to v during the step before their use)
    // and its 8 B fragments
    struct Ops {
        float d[16], t[16], v[16];
        f32x4 b[2][4];
    };
    auto read_ops = [&](const float *pa, const float *pb, Ops &o) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int pq = 0; pq < 4; ++pq) o.b[t][pq] = *reinterpret_cast<const f32x4 *>(pb + t * 256 + pq * 64);
#pragma unroll
        for (int px = 0; px < 16; ++px) o.d[px] = pa[px * 128];
    };

    // One K step: 32 MFMAs on operands whose patch values were transformed during the previous step, so the step opens on
    // the matrix pipe.  Among them, pinned by sched_barriers: after the 4th the LDS reads of the next step (issued before
    // the first MFMA they would be waited for by it: hipcc waits for its own count of outstanding reads); after the 6th,
    // 12th, ... one DMA instruction each (NDMA of them, 6 MFMAs apart: the texture path takes one at a time and a burst of
    // them queues the waves in front of their MFMAs); after the 17th .. 32nd two adds each of the next step's input
    // transform, in the shadow of this step's MFMAs.
    auto step = [&](const Ops &cur, Ops &nxt, const float *pa, const float *pb, const int ndma, auto dma) __attribute__((always_inline)) {
#if WINO_EXP == 4
#pragma unroll
        for (int q = 0; q < ndma; ++q) dma(q);
        __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
        for (int m = 0; m < 32; ++m) {
            const int t = m >> 4, pq = (m >> 2) & 3, e = m & 3;
            acc[t][4 * pq + e] =
                __builtin_amdgcn_mfma_f32_16x16x4f32(cur.b[t][pq][e], cur.v[4 * pq + e], acc[t][4 * pq + e], 0, 0, 0);
            if (m == 3) {
                __builtin_amdgcn_sched_barrier(0);
                read_ops(pa, pb, nxt);
                __builtin_amdgcn_sched_barrier(0);
            }
#if WINO_EXP != 4
            if (m % 6 == 5 && m / 6 < ndma) {
                __builtin_amdgcn_sched_barrier(0);
                dma(m / 6);
                __builtin_amdgcn_sched_barrier(0);
            }
#endif
            if (m >= 16) {
                bt_d_b_op(2 * (m - 16), nxt.d, nxt.t, nxt.v);
                bt_d_b_op(2 * (m - 16) + 1, nxt.d, nxt.t, nxt.v);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // prologue: chunk 0 and K step 0 first, then what iteration 0's barrier needs.  (Everywhere below the second half of a
    // weight step goes through voff + 1024, not through the instruction's immediate offset: that is added to the LDS
    // address as well.)
    {
        const __amdgpu_buffer_rsrc_t rp0 = rsrc_p(0), rp1 = rsrc_p(1), rw0 = rsrc_w(0), rw1 = rsrc_w(1), rw2 = rsrc_w(2);
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma16(rp0, (char *)(dst_p + i * 256), voff_p[i], 0);
        lds_dma16(rw0, (char *)dst_w, voff_w, 0);
        lds_dma16(rw0, (char *)(dst_w + 256), voff_w + 1024, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma16(rp1, (char *)(dst_p + SLOT_P + i * 256), voff_p[i], 0);
        lds_dma16(rw1, (char *)(dst_w + SLOT_W), voff_w, 0);
        lds_dma16(rw1, (char *)(dst_w + SLOT_W + 256), voff_w + 1024, 0);
        lds_dma16(rw2, (char *)(dst_w + 2 * SLOT_W), voff_w, 0);
        lds_dma16(rw2, (char *)(dst_w + 2 * SLOT_W + 256), voff_w + 1024, 0);
    }
    wait_vmcnt<8>();
    __builtin_amdgcn_s_barrier();

    // ---- the dead half's K loop: the waits, the barrier and the 8 DMA instructions of the live loop below (same slots, same
    // resources, so the rings, the counted waits and the barriers per iteration are the same for all eight waves), and no
    // LDS read, no transform, no MFMA; then no epilogue.  The branch is wave-uniform and taken once, here.  The DMAs keep
    // about the live loop's distance (6 MFMAs of the live wave that shares the SIMD = 192 cycles = s_sleep 3) instead of
    // queueing at the texture path in one burst, and the sleeping wave leaves the SIMD's issue slots to the live one.  All 8
    // are out after ~1500 cycles of an iteration of >= 2048, so a dead wave is never the last one at the barrier.
    // (gn_partials needs cout = 128: no dead half there, so the block-wide barriers of its exchange see all 8 waves.)
    if (dead) {
        int ps2 = 2 * SLOT_P;                          // patch slot of chunk j + 2
        for (int j = 0; j < nch; ++j) {
            const int w0 = (2 * j) & 3;
            const int wa = ((w0 ^ 2) + 1) * SLOT_W, wb = w0 * SLOT_W;
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const __amdgpu_buffer_rsrc_t rp = rsrc_p(j + 2), rwa = rsrc_w(2 * j + 3), rwb = rsrc_w(2 * j + 4);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (q < 4) lds_dma16(rp, (char *)(dst_p + ps2 + q * 256), voff_p[q], 0);
                else if (q < 6) lds_dma16(rwa, (char *)(dst_w + wa + (q - 4) * 256), voff_w + (q - 4) * 1024, 0);
                else lds_dma16(rwb, (char *)(dst_w + wb + (q - 6) * 256), voff_w + (q - 6) * 1024, 0);
                __builtin_amdgcn_s_sleep(3);
            }
            ps2 = ps2 == 2 * SLOT_P ? 0 : ps2 + SLOT_P;
        }
        wait_vmcnt<0>();
        return;
    }

    Ops oa, ob;
    read_ops(pa_lane0, pb_lane, oa);
#pragma unroll
    for (int k = 0; k < 32; ++k) bt_d_b_op(k, oa.d, oa.t, oa.v);

    // Iteration j = K steps 2 j and 2 j + 1 = patch chunk j.  At its barrier every wave's DMA of patch chunk j + 1 and of
    // the weights of steps 2 j + 1 and 2 j + 2 has landed (vmcnt(0): all were issued during iteration j - 1, the last of
    // them 14 MFMAs before its end), and every wave has read chunk j - 1 and the weights up to step 2 j (lgkmcnt(0)), so
    // chunk j + 2 and the weights of steps 2 j + 3 and 2 j + 4 may go into their slots.  A raw s_barrier: __syncthreads()'s
    // fence is not needed, the waits are explicit.
    int ps0 = 0, ps1 = SLOT_P, ps2 = 2 * SLOT_P;       // patch slots of chunks j, j + 1, j + 2
    for (int j = 0; j < nch; ++j) {
        const int w0 = (2 * j) & 3;                    // weight slot of step 2 j (0 or 2) and of step 2 j + 4
        const int wa = ((w0 ^ 2) + 1) * SLOT_W, wb = w0 * SLOT_W;   // weight slots of steps 2 j + 3 and 2 j + 4
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const __amdgpu_buffer_rsrc_t rp = rsrc_p(j + 2), rwa = rsrc_w(2 * j + 3), rwb = rsrc_w(2 * j + 4);
        // the 8 DMA instructions of the iteration: 5 in its first step (the patches first: they may miss L2), 3 in its second
        auto dma = [&](int q) __attribute__((always_inline)) {
            if (q < 4) lds_dma16(rp, (char *)(dst_p + ps2 + q * 256), voff_p[q], 0);
            else if (q < 6) lds_dma16(rwa, (char *)(dst_w + wa + (q - 4) * 256), voff_w + (q - 4) * 1024, 0);
            else lds_dma16(rwb, (char *)(dst_w + wb + (q - 6) * 256), voff_w + (q - 6) * 1024, 0);
        };
        step(oa, ob, pa_lane1 + ps0, pb_lane + (w0 + 1) * SLOT_W, 5, dma);
        step(ob, oa, pa_lane0 + ps1, pb_lane + (w0 ^ 2) * SLOT_W, 3, [&](int q) __attribute__((always_inline)) { dma(q + 5); });
        const int ps = ps0;
        ps0 = ps1;
        ps1 = ps2;
        ps2 = ps;
    }
    wait_vmcnt<0>();   // the empty DMAs past the last chunk

    // ---- epilogue: Y = A^T M A, A^T = [1 1 1 0; 0 1 -1 -1], on the four channels of a lane at once.  The B fragment is the
    // MFMA's first operand, so the tile comes out transposed: lane (r, kq) holds tile tg * 16 + r and channels
    // 16 t + 4 kq .. + 3 of its half as the four floats of acc[t][position].
    const int nt = 2 * nt2 + h;                        // this wave's 32-channel group
    const bool gn = p.gn_partials != nullptr && !(WINO_EXP & 16);   // (block-uniform; host: wino_gn_ok)
    double gs[2] = {0.0, 0.0}, gq[2] = {0.0, 0.0};
    long long f0 = 0;
    if (gn) {
        const int bi = gt0 / tpi, rem = gt0 - bi * tpi, ty = rem / P.TW, tx = rem - ty * P.TW;
        f0 = ((long long)(bi * p.Ho + 2 * ty) * p.Wo + 2 * tx) >> 7;
    }
    const float lo = 0.f, hi = (p.act == ML_ACT_RELU6) ? 6.f : 3.402823466e38f;
    const bool clampv = p.act == ML_ACT_RELU || p.act == ML_ACT_RELU6;
    const int gt = gt0 + tg * 16 + r;
    if (gt < P.T) {
        const int bi = gt / tpi, rem = gt - bi * tpi;
        const int ty = rem / P.TW, tx = rem - ty * P.TW;
        const int oy = 2 * ty, ox = 2 * tx;
        const bool y1 = oy + 1 < p.Ho, x1 = ox + 1 < p.Wo;
        const size_t img = p.out_bstride ? (size_t)bi * (size_t)p.out_bstride : (size_t)bi * p.Ho * p.Wo * p.out_cstride;
        const size_t pix0 = (size_t)oy * p.Wo + ox;
        const long long m_flat0 = (long long)(bi * p.Ho + oy) * p.Wo + ox;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = nt * 32 + 16 * t + 4 * kq;   // the lane's first channel of this half
            if (n >= p.cout) continue;
            const bool quad = n + 4 <= p.cout;         // else cout % 4 of the four are live: stored one by one
            f32x4 u[8];                                // A^T M: rows 0, 1 x 4 columns
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u[j] = acc[t][0 * 4 + j] + acc[t][1 * 4 + j] + acc[t][2 * 4 + j];
                u[4 + j] = acc[t][1 * 4 + j] - acc[t][2 * 4 + j] - acc[t][3 * 4 + j];
            }
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) {
                if (quad) bv = *reinterpret_cast<const f32x4d *>(p.bias + n);
                else
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (n + c < p.cout) bv[c] = p.bias[n + c];
            }
            float *o = p.out + img + p.out_coff + n;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    if ((a && !y1) || (c2 && !x1)) continue;
                    f32x4 val = (c2 ? u[4 * a + 1] - u[4 * a + 2] - u[4 * a + 3] : u[4 * a + 0] + u[4 * a + 1] + u[4 * a + 2]) + bv;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (clampv) val[c] = __builtin_amdgcn_fmed3f(val[c], lo, hi);
                        else if (p.act != ML_ACT_NONE) val[c] = ml_apply_act(val[c], p.act);
                    }
                    float *op = o + (pix0 + (size_t)a * p.Wo + c2) * p.out_cstride;
                    if (quad) out_store(p.out, op, val);
                    else
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            if (n + c < p.cout) out_store(p.out, op + c, val[c]);
                    if (gn) {                          // (cout = 128: every channel of the quad is stored)
                        const int f = ((m_flat0 + (long long)a * p.Wo + c2) >> 7) != f0;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            gs[f] += (double)val[c];
                            gq[f] += (double)val[c] * (double)val[c];
                        }
                    }
                }
        }
    }
    if (gn) {
        double *lds_gn = reinterpret_cast<double *>(lds);   // [wave 8][4], over the ring's head: every wave is past its
        __syncthreads();                                    // last LDS read and its last DMA has landed (vmcnt(0) above)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                gs[f] += __shfl_down(gs[f], o, 64);
                gq[f] += __shfl_down(gq[f], o, 64);
            }
        }
        if (lane == 0) {
            lds_gn[wave * 4 + 0] = gs[0]; lds_gn[wave * 4 + 1] = gq[0];
            lds_gn[wave * 4 + 2] = gs[1]; lds_gn[wave * 4 + 3] = gq[1];
        }
        __syncthreads();
        if (tid < 4) {
            // thread (half hh, flattened tile ff); the block's second flattened tile: the one holding its last tile's
            // bottom-right pixel
            const int hh = tid >> 1, ff = tid & 1;
            const int gt1 = gt0 + WT - 1;
            const int bi = gt1 / tpi, rem = gt1 - bi * tpi, ty = rem / P.TW, tx = rem - ty * P.TW;
            const long long f1 = ((long long)(bi * p.Ho + 2 * ty + 1) * p.Wo + 2 * tx + 1) >> 7;
            const long long ft = ff ? f1 : f0;
            const int slot = 2 * nt2 + hh;
            double s = 0.0, q = 0.0;
            for (int w = 0; w < 4; ++w) { s += lds_gn[(hh * 4 + w) * 4 + 2 * ff]; q += lds_gn[(hh * 4 + w) * 4 + 2 * ff + 1]; }
            p.gn_partials[2 * (ft * 4 + slot)] = s;
            p.gn_partials[2 * (ft * 4 + slot) + 1] = q;
        }
    }
}

}  // namespace

// The one eligibility rule of the Winograd path (tile code 6): per-problem geometry and math mode only -- never the batch
// size or the launch's tile count, so an image's results do not depend on the batch it is computed in.
extern "C" int ml_conv2d_wino_eligible(const ml_conv2d_desc *d) {
    if (!d) return 0;
    return d->math == ML_MATH_F32 && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->dil == 1 && d->pad_t == 1 &&
           d->pad_l == 1 && d->Ho == d->H && d->Wo == d->W && d->cpp_shift == 30 && d->group_cin_step == 0 &&
           !d->shuffle2x2 && !d->residual && !d->out_f16 && d->span % 32 == 0 && d->span_pad == d->span &&
           d->cout <= 128 && d->n_pad == 128;
}

// The narrow case: a problem that fails the rule above ONLY on n_pad -- a conv of at most 96 output channels in its
// automatic packing of 32, 64 or 96 rows (ml_conv2d_ntile), the last conv of the class and box towers -- without `live` and
// without gn_partials.  The host hands such a problem to the kernel with n_pad = 128 and weights padded to four 32-output
// blocks (packing.py pack_winograd); the kernel launches ceil(cout / 64) channel blocks and runs a dead half without
// MFMAs, so the padding costs no matrix work.  Per-problem geometry only, like the rule itself.  Which cout classes are
// taken is a measured, per-class decision (kernel header), written as cout ranges here and never as a launch-size heuristic:
// 1..32, 33..64 and 65..96 were each faster here than on the direct kernel.  Taken: cout 1..31, 33..63 and 65..96.  cout = 32
// and cout = 64 stay on the direct kernel: the fixed-capacity RoI batches of these two widths (`live`, not taken here) are
// held to the bits and the K slices of their `live`-less launch (tests/test_gpu_live_slots.py
// test_conv3x3_split_k_with_live), so that launch keeps the kernel its `live` twin runs on.
extern "C" int ml_conv2d_wino_narrow(const ml_conv2d_desc *d) {
    if (!d || d->live || d->gn_partials) return 0;
    if (d->n_pad != 32 && d->n_pad != 64 && d->n_pad != 96) return 0;
    if (d->cout < 1 || d->cout > d->n_pad || d->cout == 32 || d->cout == 64) return 0;
    ml_conv2d_desc w = *d;
    w.n_pad = 128;
    return ml_conv2d_wino_eligible(&w);
}

// gn_partials on the Winograd path: every 64-tile block must cover exactly two whole 128-pixel flattened tiles of one image
// (even Ho / Wo; a block is whole tile rows, or a 128-column piece of one), 4 channel groups of 32 = the 4 slots.
int ml_conv2d_wino_gn_ok(const ml_conv2d_desc &d) {
    if (d.Ho % 2 || d.Wo % 2 || d.cout != 128 || d.out_bstride || d.act == ML_ACT_SIGMOID) return 0;
    const long long TH = d.Ho / 2, TW = d.Wo / 2;
    return (64 % TW == 0 || TW % 64 == 0) && (TH * TW) % 64 == 0;
}

int ml_conv2d_wino_launch(const ml_conv2d_desc *descs, int n, hipStream_t s) {
    ML_REQUIRE(n >= 1 && n <= WMAXP, "conv2d (winograd): need 1..%d problems", WMAXP);
    WArgs args;
    args.n = n;
    long long start = 0;
    for (int i = 0; i < n; ++i) {
        const ml_conv2d_desc &d = descs[i];
        ML_REQUIRE(ml_conv2d_wino_eligible(&d),
                   "conv2d: tile = 6 (Winograd F(2x2,3x3)) needs ML_MATH_F32, a 3x3 stride-1 undilated 'same' conv, no "
                   "groups / shuffle / residual / half output, span %% 32 == 0 and n_pad == 128");
        ML_REQUIRE(((d.in_cstride | d.in_coff) & 3) == 0 && ml_aligned16(d.in) && ml_aligned16(d.wgt),
                   "conv2d (winograd): 16-byte aligned input channels and weights");
        if (d.gn_partials)
            ML_REQUIRE(ml_conv2d_wino_gn_ok(d) && !d.live, "conv2d (winograd): gn_partials needs even Ho / Wo, Wo / 2 dividing or a "
                                                "multiple of 64, (Ho / 2) (Wo / 2) %% 64 == 0, cout = 128, dense output");
        WProblem &P = args.p[i];
        P.d = d;
        P.TH = (d.Ho + 1) / 2;
        P.TW = (d.Wo + 1) / 2;
        const long long T = (long long)d.B * P.TH * P.TW;
        ML_REQUIRE(T < (1ll << 30), "conv2d (winograd): too many tiles");
        P.T = (int)T;
        P.MB = (int)((T + WT - 1) / WT);
        P.NB = (d.cout + WN - 1) / WN;                 // channel blocks that hold a channel < cout: a dead block is never launched
        P.nchunks = d.span_pad / WK;
        // a block's patch offsets are 32-bit from its first tap row: its 64 tiles cover at most 64 / TW + 2 flattened tile
        // rows, i.e. 2 (64 / TW + 2) + 2 pixel rows with the taps above and below
        const long long span = (2ll * (WT / P.TW + 2) + 2) * d.W * d.in_cstride * 4;
        ML_REQUIRE(span <= SPAN_MAX, "conv2d (winograd): a block's input rows exceed 2 GiB (W x in_cstride too large)");
        args.start[i] = (int)start;
        start += (long long)(P.MB + 7) / 8 * 8 * P.NB;
        ML_REQUIRE(start < (1ll << 31), "conv2d (winograd): grid too large");
    }
    args.start[n] = (int)start;
    // gn_partials keeps the direct kernel's launch-size rule (ml_conv2d_gn_min_launch_tiles, in 128 x 128 tiles), so the
    // host's choice between epilogue sums and a statistics pass does not depend on which kernel runs the conv
    long long tiles128 = 0;
    bool any_gn = false;
    for (int i = 0; i < n; ++i) {
        tiles128 += ((long long)descs[i].B * descs[i].Ho * descs[i].Wo + 127) / 128 * (descs[i].n_pad / 128);
        any_gn = any_gn || descs[i].gn_partials != nullptr;
    }
    ML_REQUIRE(!any_gn || tiles128 >= ml_conv2d_gn_min_launch_tiles(),
               "conv2d (winograd): gn_partials needs a launch of ml_conv2d_gn_min_launch_tiles() tiles of 128 x 128");
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = ml_ensure_dynamic_lds(reinterpret_cast<const void *>(conv_wino_kernel), LDS_BYTES, lds_ok, "conv2d (winograd)"))
        return rc;
    hipLaunchKernelGGL(conv_wino_kernel, dim3((unsigned)start), dim3(512), LDS_BYTES, s, args);
    ML_CHECK_LAUNCH("conv2d (winograd)");
    return ML_OK;
}
