/*
 * masklab_hip.h -- C ABI of libmasklab_hip.so (gfx950 / MI355X).
 *
 * The reference (craftsangjae/instance-segmentation-road-project) is pure Python on
 * tensorflow.keras and has NO FFI of its own: every arithmetic step of
 * its inference path is a TensorFlow op.  Each entry point below therefore replaces
 * the TF op(s) behind the cited reference call site (paths relative to the reference
 * root).  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller (the library never
 *     allocates persistent memory; scratch is a caller-provided workspace);
 *   - tensors are NHWC float32 unless stated; "cstride" = channels of the buffer a
 *     tensor view lives in, "coff" = first channel of the view (lets a kernel read or
 *     write a slice of a concat buffer without a copy);
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work;
 *   - return value: 0 = ok, negative = ML_E_* (no exceptions cross the boundary);
 *   - thread-safe per stream; the only global state is the per-thread error string, per
 *     kernel an atomic bitmask of the devices whose dynamic-LDS limit has been raised
 *     (hipFuncSetAttribute is a per-device setting; racing threads set the same value), and
 *     a per-device cache of the compute-unit count (sizes the persistent kernels' grids;
 *     never changes what is computed).
 *
 * masklab_hip/_lib.py binds this file by hand and tests/test_abi_cpu.py holds that binding to it: every prototype,
 * struct and ML_* constant, parsed from here.  A new entry point needs its declaration here and a row in
 * _lib.SIGNATURES (a new struct: a mirror in _lib.STRUCTS), and nothing in any test file.
 */
#ifndef MASKLAB_HIP_H
#define MASKLAB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ML_OK 0
#define ML_E_BADARG (-1)   /* shape / alignment / range precondition violated */
#define ML_E_LAUNCH (-2)   /* hipLaunchKernel or attribute call failed        */
#define ML_E_NOGPU  (-3)   /* no gfx950 device visible                        */

enum { ML_ACT_NONE = 0, ML_ACT_RELU = 1, ML_ACT_RELU6 = 2, ML_ACT_SIGMOID = 3 };
enum { ML_MATH_F32 = 0, ML_MATH_F16 = 1, ML_MATH_F16S = 2, ML_MATH_F32X3 = 3 };

#define ML_ABI_VERSION 7              /* 2: ml_conv2d_desc gained `math` / `reserved0`
                                         3: detection gather payload, mask_distribute level_max,
                                            fp16 tensor storage
                                         4: fp16 storage in the heads: ML_MATH_F16S on the generic conv,
                                            ml_gn_desc.dtype, the *_f16 entry points of GroupNorm, resize,
                                            depthwise conv, global mean, RoI crop and the mask-head tail
                                         5: fixed-capacity RoI batches (`live`) in conv / GroupNorm / RoI crop /
                                            mask-head tail descriptors, ml_mold_levels_f32
                                         6: ml_conv2d_launch_splits, ml_conv2d_gn_min_launch_tiles (reporting /
                                            the size rule of gn_partials asked of the library, not restated by callers)
                                         7: ml_stem7x7s2_pool_f16 / _f32 / _x3; ml_gconv3x3_f16 takes groups of 32 channels;
                                            ML_MATH_F32X3 on the persistent 1x1 kernel (ml_conv2d_uses_pipe);
                                            ml_mold_levels_dev_f32; (additive, same version) ml_se_desc,
                                            ml_squeeze_excite_f32 / _f16 / _workspace_bytes, ml_add_f16;
                                            (additive, same version) ml_se_residual_desc,
                                            ml_se_residual_f32 / _workspace_bytes;
                                            (additive, same version) ml_draw_boxes_u8, ml_draw_instance_u8,
                                            ml_draw_segmentation_u8, ml_serving_visualize_u8;
                                            (additive, same version) ml_se_bottleneck_desc,
                                            ml_se_bottleneck_f32 / _f16 / _workspace_bytes;
                                            (additive, same version) ml_jpeg_encode_u8 / _capacity /
                                            _workspace_bytes;
                                            (additive, same version) ml_jpeg_decode_info / _packed_bytes /
                                            _entropy / _workspace_bytes / _u8 / _reference_host;
                                            (additive, same version) ml_jpeg_entropy_geometry / _plan_bytes /
                                            _plan / _workspace_bytes / _device / _reference_host;
                                            (additive, same version) ml_conv1x1_dual_f32 / _f16;
                                            (additive, same version) ml_gn_grad_desc, ml_groupnorm_chunk_grad_f32 /
                                            _grad_multi_f32 / _grad_workspace_bytes, ml_groupnorm_chunk_stats_f32;
                                            (additive, same version) ml_opt_tensor / _state / _scalars,
                                            ml_optimizer_plan / _scalars / _apply_f32;
                                            (additive, same version) ml_roi_grad_level, ml_roi_crop_resize_grad_f32,
                                            ml_resize_bilinear_ac_grad_f32 / _grad_workspace_bytes,
                                            ml_global_mean_grad_f32;
                                            (additive, same version) ml_gconv3x3_launch_plan;
                                            (additive, same version) ml_conv2d_wgrad_desc, ml_conv2d_wgrad_multi_f32 /
                                            _wgrad_plan, ml_conv2d_grad_gather_dy_f32;
                                            (additive, same version) ml_dwconv3x3_grad_desc, ml_dwconv3x3_wgrad_multi_f32 /
                                            _wgrad_plan, ml_dwconv3x3_dgrad_multi_f32, ml_relu_grad_f32;
                                            (additive, same version) ml_deconv2x2_out1x1_tape_f32, ml_deconv_out_grad_problem,
                                            ml_deconv2x2_out1x1_grad_f32 / _grad_plan, ml_deconv2x2_grad_relayout_f32;
                                            (additive, same version) ml_repack_job, ml_repack_plan, ml_repack_f32;
                                            (additive, same version) ml_batchnorm_train_f32 / _infer_f32 / _grad_f32 /
                                            _workspace_bytes / _plan;
                                            (additive, same version) ML_DECONV_OUT_MAX_PROBLEMS, ML_JPEG_DECODE_MAX_BATCH:
                                            names for limits the entry points already had;
                                            (additive, same version) ml_conv2d_dgrad_s2_f32 / _classes,
                                            ML_CONV_DGRAD_S2_MAX_TAPS */
int ml_version(void);                 /* returns ML_ABI_VERSION of the library that was built */
const char *ml_last_error(void);      /* text of the last failure on the calling thread   */
int ml_device_check(void);            /* ML_OK iff device 0.. current is gfx950           */

/* ---------------------------------------------------------------- convolution (MFMA)
 * Implicit-GEMM convolution on v_mfma_f32_32x32x2_f32: M = B*Ho*Wo output pixels,
 * N = cout, K = taps * span_pad.  Replaces tf.keras Conv2D (+folded BatchNormalization,
 * +Add, +activation), the ResNeXt grouped 3x3 and Conv2DTranspose(2,2,s2):
 *   engine/backbone/ResNext.py:200-231,343-349   engine/backbone/base.py:294-312
 *   engine/layers/detection.py:42-48,56,64,120-128,190-200
 *   engine/layers/instance.py:188-199            engine/layers/semantic.py:66,112,126,133,199,213,219
 * Weights are pre-packed by the host as wgt[n_pad][taps*span_pad] (k contiguous,
 * k = tap*span_pad + c, zero padded; see masklab_hip/packing.py).
 */
typedef struct ml_conv2d_desc {
    const float *in;        /* [B,H,W,in_cstride] view starting at channel in_coff            */
    const float *wgt;       /* packed weights, n_pad rows of ktot floats                      */
    const float *bias;      /* [cout] or NULL                                                 */
    const float *residual;  /* optional tensor added before the activation, or NULL          */
    float *out;             /* [B,Ho,Wo,out_cstride] view starting at channel out_coff        */
    int32_t B, H, W;        /* input batch / height / width                                   */
    int32_t in_cstride, in_coff;
    int32_t span;           /* K floats per tap actually read (cin; 32 for the NHWC4 stem)    */
    int32_t span_pad;       /* span rounded up to 32                                          */
    int32_t cpp_shift;      /* stem: log2(floats per pixel) so a tap spans pixels; else 30    */
    int32_t Ho, Wo;
    int32_t KH, KW, stride, dil, pad_t, pad_l;
    int32_t cout;           /* real N                                                         */
    int32_t n_pad;          /* rows in wgt (multiple of the N tile)                           */
    int32_t out_cstride, out_coff;
    int32_t res_cstride, res_coff;
    int32_t act;            /* ML_ACT_*                                                       */
    int32_t group_cin_step; /* grouped 3x3: input-channel offset per 32-wide N block; else 0  */
    int32_t shuffle2x2;     /* 1: Conv2DTranspose epilogue, column = (a*2+b)*cout_real + o    */
    int32_t tile;           /* 0 auto, 1 = 128x128, 2 = 128x64, 3 = 128x32, 4 = pipelined 1x1 (128x128), 5 = half 1x1 on 256x256 tiles,
                               6 = Winograd F(2x2,3x3) (conv_wino.hip; ml_conv2d_wino_eligible problems only, every problem of
                               the launch): `wgt` then points to the transformed weights U = G g G^T (fp64, rounded once),
                               [4][span_pad / 8][8 channels][32 outputs][16 positions] floats (packing.py
                               pack_winograd; n_pad = 128 says no more than that: four 32-output blocks, rows >= cout zero);
                               the kernel launches ceil(cout / 64) blocks of 64 channels and a 32-channel half of a block
                               that lies wholly >= cout issues no MFMA; never split along K; gn_partials on even maps whose
                               Wo / 2 divides or is a multiple of 64 with (Ho / 2)(Wo / 2) % 64 == 0 (slot = 32-channel
                               group)                                                                             */
    int32_t math;           /* ML_MATH_F32: v_mfma_f32_32x32x2_f32 (exact fp32 products);
                               ML_MATH_F16: operands rounded to fp16 on their way into LDS,
                               v_mfma_f32_32x32x16_f16 with fp32 accumulation (BASELINE config 5);
                               tensors in HBM stay fp32 either way;
                               ML_MATH_F16S: fp16 STORAGE -- in / wgt / residual point to IEEE half data
                               (element counts and strides unchanged; span_pad = span rounded up to 64,
                               span / in_cstride / in_coff multiples of 8), fp16 MFMA, fp32 accumulation,
                               bias (fp32) + residual + activation in fp32, one rounding at the store.
                               1x1 stride-1 problems with cout % 128 == 0 and span % 64 == 0 run on the
                               persistent kernel (conv1x1_pipe.hip: half output, optional half residual);
                               every other shape on the generic kernel (no residual; output half or fp32
                               by `out_f16`);
                               ML_MATH_F32X3: fp32 tensors, fp32-grade arithmetic on the f16 matrix pipe: each
                               operand x = hi + 2^-11 lo (two halves), each product hi hi + 2^-11 (hi lo + lo hi)
                               with fp32 accumulation (operands to 2^-22 relative for 2^-14 <= |x| < 65520, 2^-36
                               absolute below; the dropped term is <= 2^-22 |a b|).
                               Activations are split inside the kernel (|x| < 65520, else Inf / NaN); `wgt` points to
                               weights split BEFOREHAND: the fp32 packing with every 32-float chunk of a row
                               replaced, in place, by 32 halves hi(w) followed by 32 halves 2^11 (w - hi(w))
                               (same bytes, same strides; masklab_hip/ops.py DeviceConv.wgt_x3).  Generic
                               kernel only (every shape, residual, split-K, gn_partials as ML_MATH_F32)   */
    int32_t out_f16;        /* 1 = `out` is IEEE half: ML_MATH_F16 (the stem feeding an fp16-storage body)
                               and ML_MATH_F16S on the generic kernel (0 there = fp32 `out`: the prediction
                               tensors); dense fast epilogue only (no residual / shuffle2x2 / out_bstride /
                               sigmoid, cout % 4 == 0).  The persistent kernel always writes half.      */
    int64_t out_bstride;    /* floats between images in `out`; 0 = Ho*Wo*out_cstride (dense).
                               Lets a level's head write straight into the concatenated
                               [B, A, classes] prediction (detection.py:210-212 Reshape+Concatenate) */
    const int32_t *live;    /* NULL, or a DEVICE int: the batch is a fixed-capacity RoI batch (the mask head run
                               without a host read of the RoI counts, instance.py:121-134 + MoldBatch misc.py:231-286)
                               in which image i exists iff i % live_period < max(1, *live); tiles that hold only
                               non-existing images compute and store nothing (a tile = the 128 consecutive output rows
                               of a block, 256 on the 256-row ML_MATH_F32X3 form, the 64 tiles of a Winograd block).
                               Rows of non-existing images inside a tile that runs are computed from whatever their
                               input holds and may be stored (NaN from NaN): nobody may read them; a launch cut along
                               K leaves them unwritten.  No row of an existing image depends on a non-existing one.
                               Generic and Winograd kernels. */
    int32_t live_period;    /* RoI slots per image (B % live_period == 0, Ho * Wo * live_period >= 128: an image's
                               slots fill at least one 128-row tile); ignored when live == NULL          */
    int32_t reserved1;
    double *gn_partials;    /* NULL, or [ceil(M/128)][4][2] DEVICE doubles: the epilogue also writes (sum, sum of squares)
                               of the values each 128-row tile stores, one pair per wave of the block (4 per tile) --
                               what the GroupNormalization behind a head conv
                               needs (detection.py:120-125): ml_gn_desc.partials then replaces the statistics pass.
                               fp32, cout = n_pad = 128, M % 128 == 0, dense destination, no residual, and a launch
                               that is neither narrowed nor split along K (>= 257 tiles in all)                 */
} ml_conv2d_desc;

int ml_conv2d_f32(const ml_conv2d_desc *d, void *stream);

/* Several independent conv problems of the SAME tile shape in one launch (the un-shared head
 * towers run the same conv at every pyramid level: detection.py:109-130,179-202, instance.py:177-201).
 * With a workspace, a launch with few output tiles in total and a long K is split along K
 * (partials in the workspace, fixed-order reduction: deterministic).  workspace may be NULL.   */
#define ML_CONV_MAX_PROBLEMS 12
int64_t ml_conv2d_workspace_bytes(void);
int ml_conv2d_multi_f32(const ml_conv2d_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes,
                        void *stream);
/* N-tile width the auto heuristic picks for `cout` (host packs n_pad from it). */
int ml_conv2d_ntile(int32_t cout, int32_t tile);
/* The four reporting entries below read the launch plan of ml_conv2d_multi_f32 -- the one function that decides which
 * kernel a launch runs, on which tiles and with how many K slices -- for these problems (tensor pointers may be NULL:
 * nothing is dereferenced).  ml_conv2d_launch_splits checks the descriptors as the launch does: where the launch would
 * be refused (the Winograd kernel's own checks excepted) it returns the same ML_E_BADARG and message.  The other three
 * report the kernel and tiles the plan picks without checking the descriptors' arguments, and 0 where no kernel can be
 * picked (mixed tile shapes or math modes, a `live` problem of >= 2 GiB, ...).
 * N-tile width (128 / 64 / 32) of the generic implicit-GEMM kernel that ml_conv2d_multi_f32 will run for these
 * problems: launches too small to fill the chip with 128-wide tiles run on narrower ones (bit-identical results:
 * same k-ordered chains, split-K cut at the same k).  For reporting only; 0 as above, or when the launch runs
 * another kernel (Winograd, the persistent 1x1 kernels). */
int ml_conv2d_launch_ntile(const ml_conv2d_desc *descs, int32_t n, int32_t has_workspace);
/* M-tile height (128 / 256) of the same launch: ML_MATH_F32X3 launches that fill the chip with 256 x 128 tiles run the
 * 8-wave software-pipelined form of the kernel (bit-identical results).  For reporting only; 0 as for the N tile. */
int ml_conv2d_launch_mtile(const ml_conv2d_desc *descs, int32_t n, int32_t has_workspace);
/* Which persistent 1x1 kernel ml_conv2d_multi_f32 runs this single problem on: 1 = the tile-pipelined 128 x 128 kernel
 * (conv1x1_pipe.hip: the short-K bottleneck convs of engine/backbone/ResNext.py:199-231; fp32 or half tensors),
 * 2 = the 256 x 256-tile kernel for half tensors with K >= 256 (conv1x1_h256.hip: the ResNeXt-101 stage 2-4 convs of
 * BASELINE configs[4]), 0 = neither (the generic implicit-GEMM kernel).  `tile` = 4 / 5 force 1 / 2 where they apply. */
int ml_conv2d_uses_pipe(const ml_conv2d_desc *d);
/* K slices (1 = not split) of every problem of the launch ml_conv2d_multi_f32 would make for these problems with a
 * workspace of `workspace_bytes` (0 = none): launches of fewer than 192 tiles with a long K are cut along K, so a shard
 * of a batch may sum K in other pieces than the whole batch does (fp32 rounding; reference DP merge
 * engine/parallel.py:64-107).  splits: n host ints, one per problem given (a problem cut into image groups: the most
 * slices of any of its groups).  For reporting / tests. */
int ml_conv2d_launch_splits(const ml_conv2d_desc *descs, int32_t n, int64_t workspace_bytes, int32_t *splits);
/* 1 iff the problem may run on the Winograd F(2x2,3x3) kernel (tile = 6): ML_MATH_F32, 3x3, stride 1, dilation 1, 'same'
 * padding (pad 1, Ho = H, Wo = W), dense input (no row-span / grouped windows), no shuffle2x2 / residual / half
 * output, span % 32 == 0, n_pad == 128.  Per-problem geometry and math mode only (never the batch or the launch).    */
int ml_conv2d_wino_eligible(const ml_conv2d_desc *d);
/* 1 iff the problem fails that rule ONLY on n_pad: cout <= n_pad, n_pad in {32, 64, 96} (the automatic packing of a conv of
 * at most 96 output channels), cout not 32 or 64 (kept on the direct kernel beside their `live` launches), no `live`, no
 * gn_partials.  Such a problem runs on the Winograd kernel when the caller sets
 * tile = 6, n_pad = 128 and points `wgt` to the transformed weights padded with zero rows to four 32-output blocks.  Per-
 * problem geometry only.                                                                                              */
int ml_conv2d_wino_narrow(const ml_conv2d_desc *d);
/* Smallest launch, in 128 x 128 tiles over all its problems, that ml_conv2d_multi_f32 neither narrows to 128 x 64 / 128 x 32
 * tiles nor cuts along K on the current device: the size from which ml_conv2d_desc.gn_partials may be set. */
int64_t ml_conv2d_gn_min_launch_tiles(void);

/* ---------------------------------------------------------------- dense convolution, backward (fp32 only)
 * Weight and bias gradient of a dense ml_conv2d_desc problem (csrc/conv_grad.hip):
 *   dkernel[kh,kw,ci,co] = sum over (b,oy,ox) of x[b, oy*stride + kh*dil - pad_t, ox*stride + kw*dil - pad_l, ci] * dy[b,oy,ox,co]
 *   dbias[co]            = sum over (b,oy,ox) of dy[b,oy,ox,co]
 * (samples outside the image contribute zero), on v_mfma_f32_32x32x2_f32: per tap a GEMM with M = cin, N = cout and
 * K = B*Ho*Wo pixels.  `conv` is the FORWARD problem: `in` = x with in_cstride / in_coff, span = cin (% 4 == 0; any
 * multiple), KH x KW up to 5 x 5, stride 1 or 2, any dilation, pad_t / pad_l, cout >= 1; `out` with out_cstride / out_coff /
 * out_bstride is the dy VIEW and is only read (rows that are not 16-byte aligned -- the towers' [B, A, d] predictions -- are
 * read with dword loads).  wgt, bias, residual, act, n_pad, span_pad, tile, live and gn_partials are ignored.  Refused by
 * name: half tensors (math = ML_MATH_F16S or out_f16), grouped / depthwise (group_cin_step), row-span (cpp_shift != 30) and
 * shuffle2x2 problems, and a workspace that is too small.
 * dkernel: contiguous [KH,KW,cin,cout], the Keras layout; dbias: [cout] or NULL (skipped).  add_kernel / add_bias: NULL, or
 * like the output: output = add + gradient with one fp32 addition; an output may be its add itself (in place).
 * No float atomics: the pixels are cut into slices (ml_conv2d_wgrad_plan: 1 / 128 of the problem's pixels rounded up to a
 * multiple of 32, at least 512 and at most 1024; longer only where a problem's partials would exceed 96 MiB) -- a function
 * of the problem's geometry alone.  A block sums a slice in fp32 in pixel order; the finish kernel adds an element's partials in ascending
 * slice order in fp64 and rounds once.  Every element is written (exact zeros for a tap that only meets padding); the same
 * bits run to run, alone or inside a multi launch, and whatever outputs and workspace held.
 * workspace: the conv workspace, 256-byte aligned, >= the sum of the problems' ml_conv2d_wgrad_plan bytes (a set that
 * needs more than ml_conv2d_workspace_bytes() goes in several launches: the results are the same bits); nothing in it needs
 * initialising. */
#define ML_CONV_WGRAD_MAX_PROBLEMS 8
typedef struct ml_conv2d_wgrad_desc {
    ml_conv2d_desc conv;            /* the forward problem: in = x, out = the dy view                */
    float *dkernel;                 /* [KH,KW,cin,cout]                                              */
    float *dbias;                   /* [cout] or NULL                                                */
    const float *add_kernel;        /* NULL or like dkernel                                          */
    const float *add_bias;          /* NULL or like dbias                                            */
} ml_conv2d_wgrad_desc;
int ml_conv2d_wgrad_multi_f32(const ml_conv2d_wgrad_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes,
                              void *stream);
/* Host only: the slices of one problem (count, pixels per slice; the last slice may be shorter) and the bytes of its
 * partials.  Checks the descriptor's geometry as the launch does (tensor pointers may be NULL). */
int ml_conv2d_wgrad_plan(const ml_conv2d_wgrad_desc *desc, int32_t *slices, int32_t *slice_pixels, int64_t *workspace_bytes);
/* A dy view [B, HW pixels, cout] (channel stride dy_cstride, dy_bstride floats between images, 0 = dense) -> contiguous
 * [B, HW, roundup4(cout)] with zeros in the pad channels: what the data gradient -- the forward kernels on the transposed
 * weights (packing.pack_dense_transposed) -- reads.  Every element of `out` is written. */
int ml_conv2d_grad_gather_dy_f32(const float *dy, float *out, int32_t B, int32_t HW, int32_t cout, int32_t dy_cstride,
                                 int64_t dy_bstride, void *stream);

/* Data gradient of a dense STRIDE-2 ml_conv2d_desc problem (csrc/conv_grad.hip), float32.  For the forward
 *   y[b,oy,ox,co] = sum of x[b, 2 oy + ky*dil - pad_t, 2 ox + kx*dil - pad_l, ci] * w[ky,kx,ci,co]:
 *   dx[b,iy,ix,ci] = (add[b,iy,ix,ci] +) sum over the taps (ky,kx) with iy + pad_t - ky*dil and ix + pad_l - kx*dil both even
 *                    and oy = (iy + pad_t - ky*dil) / 2 in [0,Ho), ox likewise in [0,Wo), of sum_co dy[b,oy,ox,co] * w[ky,kx,ci,co]
 * The parity of (iy, ix) fixes the live taps: the input pixels fall into four classes, class = 2 (iy & 1) + (ix & 1), and
 * inside a class the gradient is a stride-1 walk over dy -- pixel (iy, ix) reads dy at ((iy >> 1) + off_y, (ix >> 1) + off_x),
 * one offset pair per live tap (3x3: 2x2, 2x1, 1x2 and 1x1 taps; 1x1: one class with one tap, three with none).  Per class
 * a GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products): a block holds 128 pixels of ONE class by up to 128 input
 * channels; no MFMA is issued for a dead tap and no zero-inserted dy exists, so the MACs are the forward's
 * (B*Ho*Wo*KH*KW*cin*cout).
 * `desc` is the FORWARD problem: span = cin (% 4 == 0; any multiple), cout % 4 == 0, KH x KW up to 5 x 5, any dilation,
 * stride exactly 2, pad_t / pad_l as the forward resolved them (TF `same` on even maps: 0), B, H, W the input's and Ho, Wo
 * the output's dims.  `out` (out_cstride = cout, out_coff = 0, out_bstride 0 or dense) is dy, a DENSE [B,Ho,Wo,cout] tensor
 * that is only read; `wgt` is the KERAS-LAYOUT kernel [KH,KW,cin,cout] as it stands (the master a training step updates:
 * no packed form, no re-pack).  in, bias, residual, act, n_pad, span_pad, tile, live and gn_partials are ignored.  dx: a
 * dense [B,H,W,cin]; add: NULL, or like dx -- dx = add + gradient with one fp32 addition, and dx may be add itself (no
 * block reads what another writes).  (dx and add are parameters, not descriptor fields: the structs of ABI 7 are a
 * closed set.)  All four tensors 16-byte aligned; dy and the kernel smaller than 2 GiB each.
 * Refused by name: half tensors (math = ML_MATH_F16S or out_f16), grouped / depthwise (group_cin_step), row-span
 * (cpp_shift != 30) and shuffle2x2 problems, a stride other than 2, cin % 4 or cout % 4, kernels above 5 x 5, a map the
 * kernel does not fit (Ho or Wo < 1, or a last window that starts beyond the map), a dy view.
 * fp32 accumulation in a fixed order -- live taps ascending (ky, then kx), cout ascending -- no atomics, no split along K:
 * the same bits run to run, whatever dx held.  Every element of dx is written by the launch; a pixel no tap reaches
 * (a class without live taps, the last row or column under `valid`) gets add bit for bit, or +0.0. */
#define ML_CONV_DGRAD_S2_MAX_TAPS 25
int ml_conv2d_dgrad_s2_f32(const ml_conv2d_desc *desc, float *dx, const float *add, void *stream);
/* Host only: the four classes of that problem (checked as the launch checks it; tensor pointers may be NULL).
 * pixels[4]: input pixels of class c = 2 (iy & 1) + (ix & 1) over the batch (they sum to B*H*W); ntaps[4]: its live taps;
 * taps[4][ML_CONV_DGRAD_S2_MAX_TAPS][4]: per live tap, ascending, (ky, kx, off_y, off_x). */
int ml_conv2d_dgrad_s2_classes(const ml_conv2d_desc *desc, int64_t *pixels, int32_t *ntaps, int32_t *taps);

/* ---------------------------------------------------------------- depthwise 3x3, backward (csrc/dwconv_grad.hip), fp32
 * For y = ml_dwconv3x3_f32(x, w) (+ b) with stride 1 or 2, any dilation and leading pads (pad_t, pad_l); dy is the gradient
 * at the PRE-activation output, read at channels dy_coff : dy_coff + C of a [B,Ho,Wo,dy_cstride] buffer:
 *   dkernel[kh,kw,c] = sum over (b,oy,ox) of x[b, oy*stride + kh*dil - pad_t, ox*stride + kw*dil - pad_l, c] * dy[b,oy,ox,c]
 *   dbias[c]         = sum over (b,oy,ox) of dy[b,oy,ox,c]
 *   dx[b,iy,ix,c]    = sum over the taps whose ty = iy + pad_t - kh*dil and tx = ix + pad_l - kw*dil are multiples of stride
 *                      with (ty/stride, tx/stride) inside the output, of wgt[kh*3+kw][c] * dy[b, ty/stride, tx/stride, c]
 * (samples outside the image contribute zero and are never loaded).  C, the channel strides and offsets are multiples of 4.
 * Weight gradient: x is read at in_cstride / in_coff; dkernel is contiguous [3,3,C,1] (the Keras layout), dbias [C] or NULL
 * (skipped); add_kernel / add_bias: NULL, or like the output: output = add + gradient with one fp32 addition, an output may
 * be its add itself.  No float atomics: the pixels (b, oy, ox ascending) are cut into slices of ceil(P / 64) pixels rounded
 * up to a multiple of 16, at least 64 and at most 1024 -- a function of the problem's pixel count alone; a block sums a slice
 * in fp32 in a fixed order, the finish kernel adds an element's partials in ascending slice order in fp64 and rounds once.
 * Every element is written (an exact 0 for a tap that only meets padding); the same bits run to run, alone or in a multi
 * launch, whatever outputs and workspace held.  workspace: 256-byte aligned, >= the sum of the problems'
 * ml_dwconv3x3_wgrad_plan bytes; nothing in it needs initialising.
 * Data gradient: wgt is the forward's [9][C] (packing.pack_depthwise); dx is a dense [B,H,W,C]; add_x: NULL or like dx
 * (dx = add_x + gradient, dx may be add_x itself).  The problems of one launch write different dx tensors.
 * Fields a direction does not use are ignored. */
#define ML_DWCONV_GRAD_MAX_PROBLEMS 8
typedef struct ml_dwconv3x3_grad_desc {
    const float *x;                 /* wgrad: [B,H,W,in_cstride]                                     */
    const float *dy;                /* [B,Ho,Wo,dy_cstride]                                          */
    const float *wgt;               /* dgrad: [9][C]                                                 */
    float *dkernel;                 /* wgrad: [3,3,C,1]                                              */
    float *dbias;                   /* wgrad: [C] or NULL                                            */
    const float *add_kernel;        /* NULL or like dkernel                                          */
    const float *add_bias;          /* NULL or like dbias                                            */
    float *dx;                      /* dgrad: [B,H,W,C]                                              */
    const float *add_x;             /* NULL or like dx                                               */
    int32_t B, H, W, C, in_cstride, in_coff, Ho, Wo, dy_cstride, dy_coff, stride, dil, pad_t, pad_l;
} ml_dwconv3x3_grad_desc;
int ml_dwconv3x3_wgrad_multi_f32(const ml_dwconv3x3_grad_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes,
                                 void *stream);
/* Host only: the slices of one weight-gradient problem (count, pixels per slice; the last slice may be shorter) and the
 * bytes of its partials.  Checks the geometry as the launch does (tensor pointers may be NULL). */
int ml_dwconv3x3_wgrad_plan(const ml_dwconv3x3_grad_desc *desc, int32_t *slices, int32_t *slice_pixels,
                            int64_t *workspace_bytes);
int ml_dwconv3x3_dgrad_multi_f32(const ml_dwconv3x3_grad_desc *descs, int32_t n, void *stream);
/* The gradient in front of a ReLU whose OUTPUT is y: out[i] = y[i] > 0 ? dy[i] : 0, n floats; out may be dy itself. */
int ml_relu_grad_f32(const float *y, const float *dy, float *out, int64_t n, void *stream);

/* ResNeXt grouped 3x3 (reference engine/backbone/ResNext.py:212-219: DepthwiseConv2D(depth_multiplier=c)
 * + SplitGroups/ReduceGroups/MergeGroups), c = channels per group in {4,8,16}, C % 64 == 0, on
 * v_mfma_f32_4x4x1 (16 independent 4x4 blocks per instruction: no block-diagonal padding waste).
 * wgt is [C][9][c]: wgt[g*c+m][tap][i] = K[tap][g*c+i][m] (BatchNorm scale folded), bias [C] or NULL. */
int ml_gconv3x3_f32(const float *in, const float *wgt, const float *bias, float *out,
                    int32_t B, int32_t H, int32_t W, int32_t C, int32_t c, int32_t Ho, int32_t Wo,
                    int32_t stride, int32_t pad_t, int32_t pad_l, int32_t act, void *stream);

/* The same on fp16 tensors (in / out IEEE half, weights / bias / arithmetic fp32): the grouped conv of an
 * fp16-STORAGE ResNeXt body (BASELINE config 5).  Also c = 32 (the last stage, filters = 1024: two
 * v_mfma_f32_32x32x16_f16 per tap contract a group).                                                 */
int ml_gconv3x3_f16(const void *in, const float *wgt, const float *bias, void *out,
                    int32_t B, int32_t H, int32_t W, int32_t C, int32_t c, int32_t Ho, int32_t Wo,
                    int32_t stride, int32_t pad_t, int32_t pad_l, int32_t act, void *stream);

/* Host only, launches nothing: the launch ml_gconv3x3_f32 (is_half = 0) / ml_gconv3x3_f16 (is_half = 1) would make for
 * this problem on the current device (256 compute units where there is none), from the code the launchers themselves use:
 * plan = {tile_h, tile_w, tiles_x, tiles_y, run, blocks}.  A block covers `run` tile_h x tile_w output tiles down one tile
 * column of an image and 64-channel slab (c = 32: the whole column, run = tiles_y); blocks = tiles_x * ceil(tiles_y / run)
 * * (C / 64) * B, saturated at INT32_MAX.  Refuses, with ML_E_BADARG and the same message, every shape the launch refuses. */
int ml_gconv3x3_launch_plan(int32_t B, int32_t H, int32_t W, int32_t C, int32_t c, int32_t stride, int32_t Ho, int32_t Wo,
                            int32_t is_half, int32_t plan[6]);

/* ---------------------------------------------------------------- fp16-storage helpers (BASELINE config 5)
 * ZeroPadding2D(1)+MaxPooling2D(3,2) on an fp16 map (ResNext.py:351-352; resnext.py:196-197), C % 8 == 0. */
int ml_maxpool3x3s2_f16(const void *in, void *out, int32_t B, int32_t H, int32_t W, int32_t C,
                        int32_t Ho, int32_t Wo, int32_t pad_t, int32_t pad_l, void *stream);
/* out[b,oy,ox,:] = in[b,2oy,2ox,:] on fp16 [B,H,W,C] -> [B,ceil(H/2),ceil(W/2),C]: the sampling of a 1x1
 * stride-2 conv (the strided shortcuts, ResNext.py:199-203), which then runs as a stride-1 ML_MATH_F16S conv. */
int ml_subsample2_f16(const void *in, void *out, int32_t B, int32_t H, int32_t W, int32_t C, void *stream);
/* n halves -> n floats / n floats -> n halves (tensors crossing between an fp16-storage and an fp32 part), n % 8 == 0 */
int ml_cast_f16_to_f32(const void *in, float *out, int64_t n, void *stream);
int ml_cast_f32_to_f16(const float *in, void *out, int64_t n, void *stream);
/* The heads on IEEE-half tensors (fp16 storage beyond the backbone body, BASELINE configs[4]): the arithmetic of
 * ml_resize_bilinear_ac_f32 (engine/layers/misc.py:306 + the FPN Add detection.py:58-60 / concat-slice store
 * semantic.py:154,227), ml_dwconv3x3_f32 (semantic.py:63-64) and ml_global_mean_f32 (semantic.py:149) on half
 * in / add / out (weights and bias fp32), computed in fp32 with one rounding at the store; channel counts, strides
 * and offsets multiples of 8.                                                                                    */
int ml_resize_bilinear_ac_f16(const void *in, const void *add, void *out,
                              int32_t B, int32_t H, int32_t W, int32_t C, int32_t in_cstride, int32_t in_coff,
                              int32_t Ho, int32_t Wo, int32_t add_cstride, int32_t add_coff,
                              int32_t out_cstride, int32_t out_coff, void *stream);
int ml_dwconv3x3_f16(const void *in, const float *wgt, const float *bias, void *out,
                     int32_t B, int32_t H, int32_t W, int32_t C, int32_t in_cstride, int32_t in_coff,
                     int32_t out_cstride, int32_t out_coff, int32_t Ho, int32_t Wo,
                     int32_t stride, int32_t dil, int32_t pad_t, int32_t pad_l, int32_t act, void *stream);
int ml_global_mean_f16(const void *in, void *out, int32_t B, int32_t HW, int32_t C, void *stream);

/* The ResNeXt stem of the fp16-storage mode in one pass (engine/backbone/ResNext.py:343-352; thirdparty/classification_models/
 * models/resnext.py:193-197): ZeroPadding2D(3) + Conv2D(64, 7x7, stride 2, BatchNorm folded) + ReLU + ZeroPadding2D(1) +
 * MaxPooling2D(3, 2).  image: fp32 NHWC4 [B,H,W,4] (ml_preprocess_f32 with out_c = 4); wgt_h: IEEE half [64][7][8][4] =
 * the row-span packing of the stem (k = kernel row * 32 + pixel * 4 + channel, 8th pixel / 4th channel zero) rounded to
 * half; bias fp32 [64] or NULL; out: IEEE half [B,Hp,Wp,64].  Operands rounded to half, fp32 accumulation from the bias,
 * one rounding: bit-identical to ml_conv2d_f32 (ML_MATH_F16, out_f16) followed by ml_maxpool3x3s2_f16, without the
 * un-pooled map (839 MB at 16 x 1280^2) ever reaching memory.                                                     */
int ml_stem7x7s2_pool_f16(const float *image, const void *wgt_h, const float *bias, void *out, int32_t B, int32_t H,
                          int32_t W, int32_t Hp, int32_t Wp, void *stream);
/* The same stem on fp32 tensors with exact fp32 products (the default math): wgt = the fp32 row-span packing itself
 * ([64][7 x 32]), out fp32 [B,Hp,Wp,64].  Only the products with a non-zero weight are issued (12 of the generic kernel's
 * 16 MFMAs per kernel row), in the generic kernel's pairs and order: bit-identical to ml_conv2d_f32 (ML_MATH_F32, ReLU)
 * followed by ml_maxpool3x3s2_f32, without the un-pooled map (537 MB at 8 x 1024^2) ever reaching memory.            */
int ml_stem7x7s2_pool_f32(const float *image, const float *wgt, const float *bias, float *out, int32_t B, int32_t H,
                          int32_t W, int32_t Hp, int32_t Wp, void *stream);
/* ... and with ML_MATH_F32X3 products: wgt_x3 = the split row-span packing (per kernel row 32 hi halves, then 32 halves
 * 2^11 (w - hi)); the image values are split once, on their way into LDS.  Same steps, products and order as the generic
 * kernel's X3 path: bit-identical to ml_conv2d_f32 (ML_MATH_F32X3, ReLU) followed by ml_maxpool3x3s2_f32.            */
int ml_stem7x7s2_pool_x3(const float *image, const void *wgt_x3, const float *bias, float *out, int32_t B, int32_t H,
                         int32_t W, int32_t Hp, int32_t Wp, void *stream);

/* ---------------------------------------------------------------- fused mask-head tail
 * Conv2DTranspose(C_mid, (2,2), (2,2)) + bias + act_mid followed by Conv2D(ncls, (1,1)) + bias + act_out in one
 * kernel (reference engine/layers/instance.py:196-201 constructs the pair, :226-233 calls it; replaces the
 * tf.nn.conv2d_transpose -> tf.nn.conv2d pair).  Up to ML_DECONV_OUT_MAX_PROBLEMS problems (RoI levels, each with its own
 * weights) per launch.
 *   x        [M, K] fp32, M = rois * hw input pixels (whole h x w maps, RoIs grouped per image: rois = B * rois_per_image)
 *   wd       [4][C_mid][K]: position q = dy*2+dx major, k contiguous (the ml_conv2d_desc packing of the transposed conv)
 *   bd       [C_mid] or NULL;   bo [ncls] or NULL
 *   wo_table [C_mid/32][16][2][cp]: entry (t, e, half, c) = W_out[32 t + (e & 3) + 8 (e >> 2) + 4 half][c] (0 for
 *            c >= ncls) -- the 1x1 kernel's rows in the order the matrix cores' accumulator registers hold channels;
 *            cp = power of two >= ncls
 *   out      element (img, j, 2y+dy, 2x+dx, c) of RoI j of image img at
 *            out[img * out_image_stride + out_base + j * (4 hw ncls) + ((2y+dy) * 2w + 2x+dx) * ncls + c]
 * K % 32 == 0, C_mid in {128, 256}, ncls <= 32, M < 2^24 per problem. */
#define ML_DECONV_OUT_MAX_PROBLEMS 4   /* problems per launch of the tail, forward and backward */
typedef struct ml_deconv_out_problem {
    const float *x, *wd, *bd, *wo_table, *bo;
    float *out;
    int64_t M;
    int32_t hw, w, rois_per_image, reserved0;
    int64_t out_image_stride, out_base;
    const int32_t *live;   /* NULL, or a device int: RoI slot j of an image exists iff j < max(1, *live) (fixed-capacity
                              batch with rois_per_image = the capacity, hw * rois_per_image >= 128); 128-pixel tiles
                              that hold only non-existing slots are skipped: nothing of them is read or written.
                              Non-existing slots inside a tile that runs are computed from whatever x holds there */
} ml_deconv_out_problem;
int ml_deconv2x2_out1x1_f32(const ml_deconv_out_problem *probs, int32_t nprob, int32_t K, int32_t c_mid, int32_t ncls,
                            int32_t cp, int32_t act_mid, int32_t act_out, void *stream);
/* The same with `x` and `wd` in IEEE half (the fp16-storage mask head; K % 64 == 0): the transposed conv runs on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation; bias, the 1x1 conv (fp32 table), sigmoid and `out` stay fp32. */
int ml_deconv2x2_out1x1_f16(const ml_deconv_out_problem *probs, int32_t nprob, int32_t K, int32_t c_mid, int32_t ncls,
                            int32_t cp, int32_t act_mid, int32_t act_out, void *stream);
/* The fp32 launch that also keeps T, the transposed conv's post-activation output, for the backward: tapes[i] is problem
 * i's float32 [M, 4, C_mid] (q = 2 dy + dx the output position; column q * C_mid + c: the column order of the transposed
 * conv's GEMM packing), 16-byte aligned, disjoint from x and from each other.  `out` is bit-equal to ml_deconv2x2_out1x1_f32's
 * (the same arithmetic in the same order); rows past a problem's end are not stored.  `live` problems are refused; the
 * fp16-storage launch keeps no tape. */
int ml_deconv2x2_out1x1_tape_f32(const ml_deconv_out_problem *probs, float *const *tapes, int32_t nprob, int32_t K,
                                 int32_t c_mid, int32_t ncls, int32_t cp, int32_t act_mid, int32_t act_out, void *stream);

/* ---------------------------------------------------------------- fused mask-head tail, backward (csrc/deconv_out_grad.hip), fp32
 * For the tail above with act_mid = ReLU; dy is the gradient at the 1x1 conv's PRE-activation, read in place in the
 * [B, total, 2h, 2w, ncls] tensor with the forward's addressing (dy_base / dy_image_stride / rois_per_image):
 *   out[m,q,c]   = t[m,q,c] > 0 ? sum_k dy[pixel(m,q), k] * wo[c,k] : 0     ([M, 4, C_mid]; out may be t itself)
 *   dkernel[c,k] = sum over (m,q) of t[m,q,c] * dy[pixel(m,q), k]           ([1,1,C_mid,ncls], the Keras layout)
 *   dbias[k]     = sum over (m,q) of dy[pixel(m,q), k]
 * in ONE pass over t (read once; out written once; dy read once).  wo is the 1x1 kernel itself, [C_mid, ncls].  Up to
 * ML_DECONV_OUT_MAX_PROBLEMS problems per launch.  C_mid % 4 == 0, C_mid <= 256, ncls <= 32, M < 2^24.  A row whose dy is all
 * zero loads no t and stores zeros (the same bits for every finite t).
 * No float atomics: the pixels are cut into slices of ceil(M / 512) pixels rounded up to a multiple of 32, at least 128 -- a
 * function of the problem's pixel count alone (ml_deconv2x2_out1x1_grad_plan); a block sums a slice in a fixed order (dkernel
 * in fp32, the dy sums of dbias in fp64), the finish kernel adds an element's partials in ascending slice order in fp64 and
 * rounds once.  The same bits run
 * to run, alone or in a multi launch, whatever out, dkernel, dbias and the workspace held.  workspace: 256-byte aligned,
 * >= the sum of the problems' plan bytes; nothing in it needs initialising.  The problems of one launch write different
 * tensors. */
typedef struct ml_deconv_out_grad_problem {
    const float *dy, *t, *wo;
    float *out, *dkernel, *dbias;
    int64_t M;                      /* input pixels = rois * hw                                       */
    int32_t hw, w, rois_per_image, c_mid;
    int64_t dy_image_stride, dy_base;
} ml_deconv_out_grad_problem;
int ml_deconv2x2_out1x1_grad_f32(const ml_deconv_out_grad_problem *probs, int32_t nprob, int32_t ncls, void *workspace,
                                 int64_t workspace_bytes, void *stream);
/* Host only: the slices of one problem (count, pixels per slice; the last may be shorter) and the bytes of its partials.
 * Checks the geometry as the launch does (tensor pointers may be NULL). */
int ml_deconv2x2_out1x1_grad_plan(const ml_deconv_out_grad_problem *prob, int32_t ncls, int32_t *slices, int32_t *slice_pixels,
                                  int64_t *workspace_bytes);
/* The transposed conv's weight gradient from its 1x1 view (ml_conv2d_wgrad_multi_f32 on dy = `out` above viewed
 * [R,h,w,4 C_mid]): dk1x1 [1,1,cin,4 C_mid] -> dkernel [2,2,C_mid,cin] (a transposition), db4 [4 C_mid] -> dbias [C_mid] =
 * ((db4[c] + db4[C_mid + c]) + db4[2 C_mid + c]) + db4[3 C_mid + c] in fp32 (both NULL: skipped). */
int ml_deconv2x2_grad_relayout_f32(const float *dk1x1, const float *db4, float *dkernel, float *dbias, int32_t cin,
                                   int32_t c_mid, void *stream);

/* ---------------------------------------------------------------- depthwise / pooling
 * 3x3 DepthwiseConv2D (depth_multiplier 1), stride 1/2, dilation, explicit pads, +bias
 * (folded BN) +activation.  tf.keras.applications MobileNet body; semantic.py:63; misc.py:85.
 * wgt is [9][C] (tap major).                                                              */
int ml_dwconv3x3_f32(const float *in, const float *wgt, const float *bias, float *out,
                     int32_t B, int32_t H, int32_t W, int32_t C,
                     int32_t in_cstride, int32_t in_coff, int32_t out_cstride, int32_t out_coff,
                     int32_t Ho, int32_t Wo, int32_t stride, int32_t dil,
                     int32_t pad_t, int32_t pad_l, int32_t act, void *stream);

/* ZeroPadding2D(1)+MaxPooling2D(3,2) on a non-negative (post-ReLU) map: ResNext.py:351-352 */
int ml_maxpool3x3s2_f32(const float *in, float *out, int32_t B, int32_t H, int32_t W, int32_t C,
                        int32_t Ho, int32_t Wo, int32_t pad_t, int32_t pad_l, void *stream);

/* BackBonePreProcess (engine/backbone/base.py:57-75) fused with the NHWC->NHWC4 repack the
 * MFMA stem wants: out[...,k] = (in[..., flip?2-k:k] - mean[k]) / div[k] + shift[k], out[...,3]=0
 * (per-channel div covers normalize=3 :71-73 and the ResNeXt-101 `bn_data` input BatchNorm,
 * thirdparty/classification_models/models/resnext.py:194, which precedes the zero padding).
 * in is uint8 (is_u8=1) or float32 RGB [B,H,W,3]; out_c is 3 or 4; mean/div/shift: 3 host floats. */
int ml_preprocess_f32(const void *in, int32_t is_u8, float *out, int64_t npix, int32_t out_c,
                      int32_t flip, const float *mean, const float *div, const float *shift,
                      void *stream);

/* ---------------------------------------------------------------- GroupNormalization
 * The reference's chunk-wise GroupNormalization (engine/normalization.py:116-160):
 * per sample, the flat H*W*C vector is cut into G contiguous chunks; y=(x-mean_g)/sqrt(var_g+eps)
 * * gamma[j] + beta[j], j = g*(C/G) + (c mod C/G).  Optional fused ReLU (semantic.py:72-73,
 * 116,137,202).  workspace: >= ml_groupnorm_workspace_bytes() bytes.  In-place (y==x) allowed. */
int64_t ml_groupnorm_workspace_bytes(int32_t N, int32_t G);
int ml_groupnorm_chunk_f32(const float *x, float *y, const float *gamma, const float *beta,
                           int32_t N, int64_t HWC, int32_t C, int32_t G, float eps, int32_t relu,
                           int32_t out_cstride, int32_t out_coff, /* y view: channels of the buffer / first channel; (C,0) = dense */
                           void *workspace, void *stream);
/* The same on IEEE-half tensors (x, y half; gamma / beta float): the heads of the fp16 path (BASELINE configs[4]).
 * Statistics are fp64 sums of the stored values, the normalisation runs in fp32, one rounding at the store. */
int ml_groupnorm_chunk_f16(const void *x, void *y, const float *gamma, const float *beta,
                           int32_t N, int64_t HWC, int32_t C, int32_t G, float eps, int32_t relu,
                           int32_t out_cstride, int32_t out_coff, void *workspace, void *stream);

/* Several independent GroupNormalizations in one launch pair (the five pyramid levels of a tower depth,
 * detection.py:124,194; the three RoI levels of the mask head, instance.py:192): the few-thousand-float problems of
 * the coarse levels ride along instead of being ~10 us launches of their own.  A problem has the bits of
 * ml_groupnorm_chunk_f32 / _f16, alone and in any company.  A problem with 16-byte aligned tensors
 * and HWC/G, C, out_cstride and out_coff multiples of 4 (8 for half) runs 16-byte accesses, any other one scalar accesses
 * in the same launches.  workspace_bytes >= the sum over the problems of ml_groupnorm_workspace_bytes(N, G).         */
typedef struct ml_gn_desc {
    const float *x;
    float *y;
    const float *gamma, *beta;     /* [C] or NULL                                   */
    int64_t HWC;                   /* floats per sample                             */
    int32_t N, C, G, relu;
    int32_t out_cstride, out_coff; /* y view, as in ml_groupnorm_chunk_f32          */
    float eps;
    int32_t dtype;                 /* 0: x / y are float; 1: x / y point to IEEE half (fp16-storage heads);
                                      gamma / beta are float either way */
    const int32_t *live;           /* NULL, or a device int: sample n exists iff n % live_period < max(1, *live)
                                      (fixed-capacity RoI batches, as ml_conv2d_desc.live); nothing of the others
                                      is read or written, in place or not                                        */
    int32_t live_period, reserved; /* N % live_period == 0                                                       */
    const double *partials;        /* NULL, or per chunk (n * G + g) `n_partials` consecutive (sum, sum of squares) pairs
                                      written by the producing conv (ml_conv2d_desc.gn_partials: the chunk's 128-row
                                      tiles, HWC/G a multiple of 128 * C): added in that order, no statistics pass    */
    int32_t n_partials, reserved2;
} ml_gn_desc;
#define ML_GN_MAX_PROBLEMS 8
int ml_groupnorm_multi_f32(const ml_gn_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- GroupNormalization, backward (fp32 only)
 * TensorFlow's gradient of the expression above.  For the chunk (n, g) with values x_i, i < L = HWC/G:
 *   j_i = g*(C/G) + (i mod C/G)    (= the forward's index: chunks start at multiples of C/G)
 *   xhat_i = (x_i - mean) * r,  r = 1/sqrt(var + eps)  (biased statistics of the chunk),  y_i = xhat_i*gamma[j_i] + beta[j_i]
 *   d_i  = dy_i * [y_i > 0]   if relu (the forward's fused ReLU; strict), else dy_i;      g_i = d_i * gamma[j_i]
 *   dx_i = r * (g_i - mean_i(g) - xhat_i * mean_i(g * xhat))                              (* [x_i > 0] if input_relu)
 *   dbeta[j] = sum d_i,  dgamma[j] = sum d_i * xhat_i   over all samples, chunks and positions with j_i = j.
 * input_relu: x is the ReLU output of the layer below (the towers' Conv3x3 + ReLU -> GroupNormalization) and dx is wanted
 * at that layer's pre-activation.
 * gamma == NULL: ones (scale=False).  beta is read only when relu (NULL: zeros).  dgamma / dbeta: [C] or NULL (skipped; both
 * are written in full otherwise).  dx may be dy itself (in place on the gradient buffer); it may not overlap x.
 * stats: NULL, or the [N*G][2] (sum x, sum x^2) of ml_groupnorm_chunk_stats_f32 -- with relu and chunks of more than 4096
 * floats the mask needs them before anything is summed, and without `stats` a statistics pass over x runs first.  The results
 * have the same bits with and without `stats`.
 * All sums are fp64, reduced in a fixed order; no atomics: two launches give the same bits.
 * workspace: >= ml_groupnorm_grad_workspace_bytes(N, G, C) bytes; nothing in it needs initialising. */
int64_t ml_groupnorm_grad_workspace_bytes(int32_t N, int32_t G, int32_t C);
int ml_groupnorm_chunk_grad_f32(const float *x, const float *dy, const float *gamma, const float *beta, float *dx,
                                float *dgamma, float *dbeta, const double *stats, int32_t N, int64_t HWC,
                                int32_t C, int32_t G, float eps, int32_t relu, int32_t input_relu,
                                void *workspace, void *stream);
/* (sum x, sum x^2) of every chunk in fp64, stats[(n*G + g)*2 + {0, 1}]: the forward's statistics pass on its own.
 * workspace: >= ml_groupnorm_workspace_bytes(N, G) bytes. */
int ml_groupnorm_chunk_stats_f32(const float *x, double *stats, int32_t N, int64_t HWC, int32_t C, int32_t G,
                                 void *workspace, void *stream);
/* Several backward problems in one launch set (the five pyramid levels of a tower depth), as ml_groupnorm_multi_f32: up to
 * ML_GN_MAX_PROBLEMS problems of any shape and alignment (16-byte accesses where a problem has them); the same bits as the
 * single calls.  workspace_bytes >= the sum over the problems of ml_groupnorm_grad_workspace_bytes(N, G, C). */
typedef struct ml_gn_grad_desc {
    const float *x, *dy;           /* the layer's input, the gradient at its output                */
    const float *gamma, *beta;     /* [C] or NULL                                                  */
    float *dx;                     /* like x; may be dy                                            */
    float *dgamma, *dbeta;         /* [C] or NULL                                                  */
    const double *stats;           /* [N*G][2] or NULL                                             */
    int64_t HWC;                   /* floats per sample                                            */
    int32_t N, C, G, relu, input_relu;
    float eps;
} ml_gn_grad_desc;
int ml_groupnorm_grad_multi_f32(const ml_gn_grad_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes,
                                void *stream);

/* ---------------------------------------------------------------- BatchNormalization, training (fp32 only; csrc/batchnorm.hip)
 * tf.keras.layers.BatchNormalization in training mode on NHWC tensors, axis = -1: every sum runs over all N = B*H*W pixels
 * of a channel c.  The moving-statistics rule is tf.keras's fused path as remembered from the 1.x releases; parity with
 * TensorFlow is UNPINNED (README).
 *   mean_b = sum x / N,   var_b = sum (x - mean_b)^2 / N   (biased)
 *   r = 1/sqrt(var_b + eps),   scale = gamma * r,   shift = beta - mean_b * scale      (fp64, each rounded once to float32)
 *   y = x * scale + shift [+ residual],   then max(., 0) when relu
 *   var_u = var_b * N / (N - 1);   batch_mean = f32(mean_b),  batch_var = f32(var_u)    (rounded once from fp64)
 *   moving <- moving - (moving - batch_stat) * f32(1 - momentum)                         three float32 operations, each
 *                                                                                        rounded, no fused multiply-add
 * Backward, with the forward's saved (mean_b, r) in fp64:
 *   g = dy * [y > 0] when relu (strict, as tf.nn.relu's; decided on the forward's own y), else g = dy
 *   xhat = (x - mean_b) * r,   dbeta = sum g,   dgamma = sum g * xhat
 *   dx = scale * (g - dbeta/N - xhat * dgamma/N),   d_residual = g
 * Inference: scale = gamma / sqrt(moving_var + eps), shift = beta - moving_mean * scale (fp64, rounded once), the same y.
 * gamma == NULL: ones (scale=False).  beta == NULL: zeros (center=False).  residual == NULL: none.
 * Sums are fp64 in a fixed order (thread, block rows in order, slices in ascending order), no atomics, no host read: two
 * launches give the same bits whatever outputs and workspace held; the launches can be captured in a graph.
 * Refused (ML_E_BADARG, the message names the argument): C no multiple of 4 (lanes run along the channels with 16-byte
 * accesses), N < 2 in training (var_u divides by N - 1), maps that are not 16-byte aligned, a workspace smaller than
 * ml_batchnorm_workspace_bytes(N, C), and every aliasing but: y may be x itself; dx may be dy itself; d_residual may be dy
 * itself when dx is not.
 * saved: [C][2] doubles (mean_b, r), written by _train, read by _grad.  batch_mean / batch_var: [C] floats.
 * moving_mean / moving_var: [C], updated in place; both NULL: no update.  d_residual, dgamma, dbeta: NULL = not wanted.
 * y of _grad is read only when relu.  Nothing in the workspace needs initialising. */
int64_t ml_batchnorm_workspace_bytes(int64_t N, int32_t C);        /* -1: refused, ml_last_error() says why */
/* host only: the slice plan, a function of (N, C) alone -- slices of the pixel axis, pixels per slice (the last one may be
 * shorter), workspace bytes.  Any of the three pointers may be NULL. */
int ml_batchnorm_plan(int64_t N, int32_t C, int32_t *slices, int64_t *pixels_per_slice, int64_t *bytes);
int ml_batchnorm_train_f32(const float *x, const float *residual, float *y, const float *gamma, const float *beta,
                           float *moving_mean, float *moving_var, double *saved, float *batch_mean, float *batch_var,
                           int64_t N, int32_t C, float eps, double momentum, int32_t relu,
                           void *workspace, int64_t workspace_bytes, void *stream);
int ml_batchnorm_infer_f32(const float *x, const float *residual, float *y, const float *gamma, const float *beta,
                           const float *moving_mean, const float *moving_var, int64_t N, int32_t C, float eps,
                           int32_t relu, void *workspace, int64_t workspace_bytes, void *stream);
int ml_batchnorm_grad_f32(const float *x, const float *dy, const float *y, const double *saved, const float *gamma,
                          float *dx, float *d_residual, float *dgamma, float *dbeta, int64_t N, int32_t C,
                          int32_t relu, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- resampling / reductions
 * tf.compat.v1.image.resize_bilinear(align_corners=True) (engine/layers/misc.py:306), with the
 * FPN `Add` (detection.py:58-60) or a concat-slice write (semantic.py:154,227) fused.        */
int ml_resize_bilinear_ac_f32(const float *in, const float *add, float *out,
                              int32_t B, int32_t H, int32_t W, int32_t C, int32_t in_cstride, int32_t in_coff,
                              int32_t Ho, int32_t Wo, int32_t add_cstride, int32_t add_coff,
                              int32_t out_cstride, int32_t out_coff, void *stream);

/* tf.reduce_mean over H,W (semantic.py:149; GlobalAveragePooling2D misc.py:43): [B,HW,C]->[B,C] */
int ml_global_mean_f32(const float *in, float *out, int32_t B, int32_t HW, int32_t C, void *stream);

/* ---------------------------------------------------------------- resampling, backward (fp32 only, C % 4 == 0)
 * The three layers are linear: their backward needs shapes and the RoI tables, no saved activation.  Every kernel is a
 * GATHER: a thread owns 4 channels of one pixel of the input-side gradient and adds the output samples that reach it in a
 * fixed order.  No float atomics and no zero-fill: every element of dx is written, exact zeros where no sample reaches, and
 * two launches give the same bits whatever dx and the workspace held.  The sample coordinates are the forward kernels'
 * expressions evaluated in float32, one rounding per operation.  `add` (NULL, or like dx): dx = add + gradient; dx may be
 * add itself (in place), it may not overlap dy.
 *
 * ml_resize_bilinear_ac_grad_f32: dy [B,Ho,Wo,dy_cstride], read at channels dy_coff .. dy_coff + C (the forward writes
 * concat slices) -> dx [B,H,W,C]; per element oy ascending, then ox.  A 1x1 source (every output pixel is that pixel) is
 * summed in fp64 over slices of the pixels and folded in slice order; only this form needs the workspace
 * (ml_resize_bilinear_ac_grad_workspace_bytes, 0 otherwise; nothing in it needs initialising).                        */
int64_t ml_resize_bilinear_ac_grad_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo);
int ml_resize_bilinear_ac_grad_f32(const float *dy, const float *add, float *dx, int32_t B, int32_t H, int32_t W,
                                   int32_t C, int32_t Ho, int32_t Wo, int32_t dy_cstride, int32_t dy_coff,
                                   void *workspace, int64_t workspace_bytes, void *stream);
/* dx[b,p,c] = dpool[b,c] / HW (+ add): dpool [B,C] -> dx [B,HW,C] */
int ml_global_mean_grad_f32(const float *dpool, const float *add, float *dx, int32_t B, int32_t HW, int32_t C,
                            void *stream);

/* x[b,h,w,c] *= s[b,c]  (SqueezeExcite scale, misc.py:46-47)                                 */
int ml_scale_channels_f32(float *x, const float *s, int32_t B, int32_t HW, int32_t C, void *stream);

/* SqueezeExcite whole (engine/layers/misc.py:24-54): GlobalAveragePooling2D (:43) -> Dense(Hd, relu, no bias) (:44) ->
 * Dense(C, sigmoid, no bias) (:45) -> Multiply (:46-47), for up to ML_SE_MAX_PROBLEMS problems (the pyramid / RoI levels
 * of one tower depth, detection.py:111-125, instance.py:179-193) in ONE launch pair:
 *   squeeze_excite_pool[_h]  per (sample, 256-pixel chunk) the channel sums, fp64, stored as a slab in the workspace;
 *   squeeze_excite_scale[_h] per (sample, chunk) the sample's slabs added in chunk order, mean = sum / HW, the two Dense
 *                            layers in fp32 (w1 [C][Hd], w2 [Hd][C]), then out = x * gate over the chunk.
 * No atomics: the result is the same bits run to run and under graph replay.  `out` may equal `x`; anything else must
 * not overlap it.  x / out: NHWC [B,HW,C] float (_f32) or IEEE half (_f16: fp32 weights and gate, one rounding at the
 * store), 16-byte aligned, C a multiple of 4 (_f32) / 8 (_f16), C <= 1024, 1 <= Hd <= 64.  `live` as in
 * ml_conv2d_desc: sample n exists iff n % live_period < max(1, *live); nothing of the others is read or written.
 * Problem i's slabs are workspace[ws_offset, + ml_squeeze_excite_workspace_bytes(B, HW, C)): 16-byte aligned, disjoint,
 * inside workspace_bytes.                                                                                        */
typedef struct ml_se_desc {
    const void *x;
    void *out;
    const float *w1;              /* [C][Hd] (Dense 1 kernel, misc.py:34-36) */
    const float *w2;              /* [Hd][C] (Dense 2 kernel, misc.py:37-40) */
    int32_t B, HW, C, Hd;
    const int32_t *live;          /* NULL, or a device int (fixed-capacity RoI batches) */
    int32_t live_period, reserved;
    int64_t ws_offset;            /* bytes into the call's workspace */
} ml_se_desc;
#define ML_SE_MAX_PROBLEMS 8
int64_t ml_squeeze_excite_workspace_bytes(int32_t B, int32_t HW, int32_t C);
int ml_squeeze_excite_f32(const ml_se_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes, void *stream);
int ml_squeeze_excite_f16(const ml_se_desc *descs, int32_t n, void *workspace, int64_t workspace_bytes, void *stream);

/* SE-ResNet pre-activation basic block tail (thirdparty resnet.py residual_conv_block :60-109 + ChannelSE,
 * _common_blocks.py:88-119), fp32 NHWC [B,HW,C], one problem per call:
 *   ML_SE_RES_GATE     g = sigmoid(W2 relu(W1 mean_hw(x) + b1) + b2)  (ChannelSE's two 1x1 convs, with bias)
 *                      y = x * g + shortcut                          (Multiply, then Add; no ReLU after the add)
 *                      out_act = relu(y * scale + shift)             (the next unit's bn1 + relu1, or the final bn1 + relu1)
 *                      out_y = y                                     (optional: NULL unless the next unit takes y as
 *                                                                     its identity shortcut)
 *                      two launches: se_residual_pool per (sample, pool chunk) the channel sums, fp64, stored as a slab
 *                      in the workspace (a pool chunk is a whole number of tail chunks, at most min(64, 4096 / C) of
 *                      them per sample); se_residual_tail per (sample, tail chunk of 16384 / C pixels) the sample's
 *                      slabs added in one fixed order, the two FC layers in fp32, then the chunk streamed once.
 *   ML_SE_RES_BN_RELU  out_act = relu(x * scale + shift): one launch, no workspace; shortcut / w* / out_y unused
 *                      (shortcut and out_y must be NULL).
 * scale / shift [C] are an inference BatchNorm folded on the host (gamma / sqrt(var + eps), beta - mean * scale).
 * w1 [C][Hd] (the 1x1 kernel [1,1,C,Hd]), b1 [Hd], w2 [Hd][C], b2 [C].  4 <= C <= 512, C % 4 == 0, 1 <= Hd <= 32.
 * x / shortcut / out_act / out_y / scale / shift 16-byte aligned.  An output may be the very buffer of an input; no
 * other overlap.  No atomics: the same bits run to run, under graph replay, and for image k of any batch.
 * GATE needs workspace_bytes >= ml_se_residual_workspace_bytes(B, HW, C), 16-byte aligned; BN_RELU takes NULL.   */
enum { ML_SE_RES_GATE = 0, ML_SE_RES_BN_RELU = 1 };
typedef struct ml_se_residual_desc {
    const float *x;               /* conv2 output (GATE) or the tensor to normalise (BN_RELU) */
    const float *shortcut;        /* GATE: added after the gate; BN_RELU: NULL */
    const float *w1, *b1;         /* [C][Hd], [Hd] */
    const float *w2, *b2;         /* [Hd][C], [C] */
    const float *scale, *shift;   /* [C] */
    float *out_act;               /* relu(y * scale + shift) */
    float *out_y;                 /* y, or NULL */
    int32_t B, HW, C, Hd;
    int32_t mode, reserved;
} ml_se_residual_desc;
int64_t ml_se_residual_workspace_bytes(int32_t B, int32_t HW, int32_t C);
int ml_se_residual_f32(const ml_se_residual_desc *desc, void *workspace, int64_t workspace_bytes, void *stream);

/* SE-ResNet-50 / SE-ResNeXt-50 post-activation bottleneck tail (thirdparty senet.py SEResNetBottleneck :46-88,
 * SEResNeXtBottleneck :91-134, ChannelSE _common_blocks.py:88-119), NHWC [B,HW,C], one problem per call:
 *   g   = sigmoid(W2 relu(W1 mean_hw(c3) + b1) + b2)   (ChannelSE's two 1x1 convs with bias; fp64, once per sample,
 *                                                        kept as g_hi = fp32(g) and g_lo = fp32(g - g_hi))
 *   out = relu(c3 * g + residual)                      fp32: the reference's two fp32 ops, Multiply (c3 * g_hi), then
 *                                                      Add; half: fma(c3, g_lo, fma(c3, g_hi, residual)) in fp32; ReLU,
 *                                                      one rounding at the store
 * three launches: per (sample, pool chunk) fp64 channel sums into workspace slabs; per sample the gate into the
 * workspace; per (sample, chunk) the stream.  _f32: float tensors; _f16: IEEE-half c3 / residual / out.
 * w1 [C][Hd] (the 1x1 kernel [1,1,C,Hd]), b1 [Hd], w2 [Hd][C], b2 [C], fp32 in both.  4 <= C <= 2048, C % 4 == 0
 * (C % 8 == 0 for _f16), 1 <= Hd <= 128.  c3 / residual / out 16-byte aligned.  out may be the very buffer of c3 or of
 * residual; no other overlap.  No atomics: the same bits run to run, under graph replay, and for image k of any batch.
 * workspace_bytes >= ml_se_bottleneck_workspace_bytes(B, HW, C), 16-byte aligned.                                  */
typedef struct ml_se_bottleneck_desc {
    const void *c3;               /* bn3(conv3(.)): float or half */
    const void *residual;         /* the unit's shortcut, same type */
    const float *w1, *b1;         /* [C][Hd], [Hd] */
    const float *w2, *b2;         /* [Hd][C], [C] */
    void *out;                    /* relu(c3 * g + residual), same type */
    int32_t B, HW, C, Hd;
} ml_se_bottleneck_desc;
int64_t ml_se_bottleneck_workspace_bytes(int32_t B, int32_t HW, int32_t C);
int ml_se_bottleneck_f32(const ml_se_bottleneck_desc *desc, void *workspace, int64_t workspace_bytes, void *stream);
int ml_se_bottleneck_f16(const ml_se_bottleneck_desc *desc, void *workspace, int64_t workspace_bytes, void *stream);

/* The projection unit of a ResNet-50 stage (Keras-Applications resnet50.py conv_block: Add(bn(res*_branch2c(a)),
 * bn(res*_branch1(x))) + ReLU) as ONE GEMM over the concatenated K of two source tensors, NHWC:
 *   out[b, i, j, n] = relu( sum_k a[b, i, j, k] Wa[k, n] + sum_l x[b, s i, s j, l] Wx[l, n] + bias[n] )
 * a [B, Ho, Wo, Ka], x [B, H, W, Kx] read in place at stride s in {1, 2} (Ho = (H - 1) / s + 1, Wo likewise; no subsample
 * copy, no concatenation buffer, no shortcut tensor), out [B, Ho, Wo, N].  wgt [N][Ka + Kx]: row n holds Wa[:, n] then
 * Wx[:, n], both BatchNorms folded; bias [N] fp32 = the sum of the two folded biases.
 * _f32: float tensors and weights, exact fp32 products (v_mfma_f32_32x32x2_f32), each output one fp32 fma chain in k order.
 * _f16: IEEE-half a / x / wgt / out, fp16 MFMA with fp32 accumulation, bias and ReLU in fp32, one rounding at the store.
 * Ka and Kx positive multiples of the K chunk (32 floats / 64 halves), N a multiple of 128, every pointer 16-byte aligned,
 * every tensor below 2 GiB; anything else is ML_E_BADARG (nothing is launched), and the caller runs the unit as two convs.
 * No atomics, no split K: the same bits run to run, under graph replay, and for image k of any batch.             */
int ml_conv1x1_dual_f32(const float *a, const float *x, const float *wgt, const float *bias, float *out,
                        int32_t B, int32_t H, int32_t W, int32_t Ka, int32_t Kx, int32_t N, int32_t stride, void *stream);
int ml_conv1x1_dual_f16(const void *a, const void *x, const void *wgt, const float *bias, void *out,
                        int32_t B, int32_t H, int32_t W, int32_t Ka, int32_t Kx, int32_t N, int32_t stride, void *stream);

/* ---------------------------------------------------------------- detection post-process
 * RestoreBoxes (engine/layers/detection.py:325-344): priors int32 [A,4] (cx,cy,w,h) shared by
 * the batch; loc [B,A,4] -> boxes [B,A,4].                                                    */
int ml_restore_boxes_f32(const float *loc, const int32_t *priors, float *boxes,
                         int32_t B, int32_t A, void *stream);

/* DetectionProposal (detection.py:482-567) in fixed capacity: threshold -> per-(image,class)
 * greedy NMS -> per-image cross-class NMS -> rows (cx,cy,w,h,class,conf), -1 padded.
 *   cls_pred [B,A,C], boxes [B,A,4] -> proposed [B,max_out,6], counts [B] (int32),
 *   kept [B,max_out,2] (anchor, class) int32 or NULL,
 *   gather_payload [B, max_out*6 + 1] or NULL: per image the 6*max_out floats of `proposed` followed
 *   by the count bit-cast to float -- the fixed-size record one RCCL all-gather merges across GPUs
 *   (the reference's DP merge is Concatenate(axis=0), engine/parallel.py:92-107).
 * C <= 64; C*max_out <= 2048 keeps the cross-class stage in LDS, larger values (the constructor
 * default nms_max_output_size=1000, detection.py:472) run it through the workspace.
 * workspace: >= ml_detection_workspace_bytes(B,A,C,max_out) bytes.                            */
int64_t ml_detection_workspace_bytes(int32_t B, int32_t A, int32_t C, int32_t max_out);
int ml_detection_proposal_f32(const float *cls_pred, const float *boxes, float *proposed,
                              int32_t *counts, int32_t *kept, float *gather_payload,
                              int32_t B, int32_t A, int32_t C,
                              float min_confidence, float nms_iou, float post_iou, int32_t max_out,
                              void *workspace, void *stream);

/* MaskDistribute (engine/layers/instance.py:52-66) + the per-level `tf.where` of
 * PyramidRoiAlign (instance.py:121): proposed [B,cap,6] -> level_slots [B,L,cap] (row indices,
 * ascending), level_counts [B,L], level_max [L] or NULL = max over the images of level_counts
 * (the second axis MoldBatch gives each level's crops, misc.py:235-236: the one host read of
 * the forward).  L = max_k+1.                                                                  */
int ml_mask_distribute_i32(const float *rows, int32_t row_stride, int32_t has_k,
                           float *kvals /* [B,cap] or NULL */, int32_t *level_slots,
                           int32_t *level_counts, int32_t *level_max, int32_t B, int32_t cap,
                           int32_t max_k, float base_size, void *stream);
/* rows: [B,cap,row_stride]; has_k=0: rows are (cx,cy,w,h,cls,conf) and k is computed
 * (MaskDistribute); has_k=1: rows are dist_boxes (k,cx,cy,w,h,cls,conf) and k is read.        */

/* tf.image.crop_and_resize + MoldBatch(-1) for one pyramid level (instance.py:115-134):
 * fmap [B,Hf,Wf,C]; rows [B,cap,row_stride] with (cx,cy,w,h,cls,conf) starting at column row_off;
 * writes roi_fmaps [B,n_l,ch,cw,C] and roi_boxes[b, box_off+j, 0..5]
 * (row stride box_rows*6); slots j >= level_counts[b,level] are filled with -1.              */
int ml_roi_crop_resize_f32(const float *fmap, const float *rows, int32_t row_stride, int32_t row_off,
                           const int32_t *level_slots,
                           const int32_t *level_counts, float *roi_fmaps, float *roi_boxes,
                           int32_t B, int32_t Hf, int32_t Wf, int32_t C, int32_t cap, int32_t L,
                           int32_t level, int32_t n_l, int32_t ch, int32_t cw,
                           float img_h, float img_w, int32_t box_off, int32_t box_rows,
                           const int32_t *live /* NULL, or a device int: with n_l = cap (no host read of the counts) only
                                                  slots j < max(1, *live) are written (crop or -1 fill), in roi_fmaps
                                                  and in roi_boxes; the others keep what they held */,
                           void *stream);
/* The same with fmap / roi_fmaps in IEEE half (C % 8 == 0): the mask head of the fp16 path; boxes and rows stay fp32. */
int ml_roi_crop_resize_f16(const void *fmap, const float *rows, int32_t row_stride, int32_t row_off,
                           const int32_t *level_slots, const int32_t *level_counts, void *roi_fmaps, float *roi_boxes,
                           int32_t B, int32_t Hf, int32_t Wf, int32_t C, int32_t cap, int32_t L,
                           int32_t level, int32_t n_l, int32_t ch, int32_t cw,
                           float img_h, float img_w, int32_t box_off, int32_t box_rows, const int32_t *live,
                           void *stream);

/* Backward of ml_roi_crop_resize_f32 for ALL levels in one launch: levels[l] is pyramid level l (l < n_levels <= L), dy the
 * gradient at its molded crops [B, n_l, ch, cw, C] (n_l: the host-sized value, or cap from a fixed-capacity forward), dx the
 * gradient at its feature map [B, Hf, Wf, C].  rows / level_slots / level_counts: what the forward read.  The boxes carry no
 * gradient (DetectionProposal ends in tf.stop_gradient).  Rows j >= level_counts[b, l] are MoldBatch padding: their dy is
 * never read.  Per element the sum runs over slot j ascending, then oy, then ox; a sample outside [0, Hf-1] x [0, Wf-1]
 * was the extrapolation value and contributes nothing.  See "resampling, backward" above for add / dx and the guarantees. */
#define ML_RESAMPLE_MAX_LEVELS 8
typedef struct ml_roi_grad_level {
    const float *dy;               /* [B, n_l, ch, cw, C]                                          */
    const float *add;              /* [B, Hf, Wf, C] or NULL                                       */
    float *dx;                     /* [B, Hf, Wf, C]; may be add                                   */
    int32_t Hf, Wf, n_l, reserved;
} ml_roi_grad_level;
int ml_roi_crop_resize_grad_f32(const ml_roi_grad_level *levels, int32_t n_levels, const float *rows, int32_t row_stride,
                                int32_t row_off, const int32_t *level_slots, const int32_t *level_counts, int32_t B,
                                int32_t C, int32_t cap, int32_t L, int32_t ch, int32_t cw, float img_h, float img_w,
                                void *stream);

/* MoldBatch + Concatenate(axis=1) of a fixed-capacity stage 2 (instance.py:222-225, misc.py:231-286): src [B, L*cap, E]
 * holds level l's RoIs at rows l*cap ..; dst [B, sum n_l, E] receives rows [l*cap, l*cap + n_l) of every image, the
 * levels next to each other.  n_l: L HOST ints (1 <= n_l <= cap) -- the one read of the forward, done after all of it
 * has been enqueued.  E % 4 == 0.                                                                                 */
int ml_mold_levels_f32(const float *src, float *dst, int32_t B, int32_t L, int32_t cap, int64_t E,
                       const int32_t *n_l, void *stream);
/* The same with the level sizes read ON THE DEVICE: lmax_dev = the L per-level RoI maxima ml_mask_distribute_f32 wrote
 * (n_l = min(max(1, lmax), cap), as the host computes them) -- no host value enters the launch, so it can be part of a
 * captured hipGraph; dst is a capacity buffer of B * L * cap * E floats whose FRONT receives the [B, sum n_l, E] tensor
 * (the host, once it has read lmax, takes that front as a view: no launch after the graph).  Any E.                */
int ml_mold_levels_dev_f32(const float *src, float *dst, int32_t B, int32_t L, int32_t cap, int64_t E,
                           const int32_t *lmax_dev, void *stream);

/* x += y over n floats (n % 4 == 0): the `Add` of MobileSeparableConv2D (misc.py:92,105) */
int ml_add_f32(float *x, const float *y, int64_t n, void *stream);
/* the same on IEEE half x / y (fp16-storage heads): summed in fp32, rounded once; any n > 0, 16-byte aligned pointers */
int ml_add_f16(void *x, const void *y, int64_t n, void *stream);

/* fill n floats with v */
int ml_fill_f32(float *x, float v, int64_t n, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Deploy wrapper either side of the forward (reference engine/retinamasklab.py:598-643) --
 * SURVEY section 8(f) ranks 1 and 2.
 * ------------------------------------------------------------------------------------------- */
#define ML_SMOOTH_MAX_CLASSES 16

/* tf.compat.v1.image.resize_bilinear(align_corners=True) for any channel count: replaces the resize
 * inside DownSampleInput.call (engine/layers/misc.py:143-154; uint8 or float images, cast to f32
 * first), ResizeLike on the 3-channel semantic map (retinamasklab.py:628) and the semantic resize of
 * UpSampleOutput.call (misc.py:190-193).  in: [B,H,W,C] u8 (in_is_u8) or f32.  Writes the f32 result
 * to out_f32 and/or `value > threshold ? 1 : 0` to out_i32 (either may be NULL), both [B,Ho,Wo,C]. */
int ml_resize_image_ac(const void *in, int32_t in_is_u8, float *out_f32, int32_t *out_i32, float threshold,
                       int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, void *stream);

/* TrimInstances.call (engine/layers/instance.py:258-277) with mold=True, fixed capacity: per image the
 * rows of roi_boxes [B,N,6] whose class (column 4) != -1 are moved to the front in order, their mask
 * is the class channel of roi_masks [B,N,mh,mw,C]; out_boxes [B,N,6] / out_masks [B,N,mh,mw] are
 * -1 padded (MoldBatch, misc.py:231-286) and counts[b] = rows kept.  The reference's dynamic second
 * axis is max(counts): the caller slices.                                                         */
int ml_trim_instances_f32(const float *roi_boxes, const float *roi_masks, float *out_boxes, float *out_masks,
                          int32_t *counts, int32_t B, int32_t N, int32_t mh, int32_t mw, int32_t C, void *stream);

/* UpSampleOutput.call box part (engine/layers/misc.py:178-187): rows (cx,cy,w,h,label,conf) f32 ->
 * int32 (cx*ratio0, cy*ratio1, w*ratio0, h*ratio1, label, conf*100), truncating like tf.cast.
 * ratio0 is the HEIGHT ratio and ratio1 the width ratio, as in the reference.                       */
int ml_upsample_boxes_i32(const float *rows, int32_t *out, int64_t n_rows, float ratio0, float ratio1, void *stream);

/* out[i] = in[i] > threshold ? 1 : 0  (tf.cast(x > 0.5, tf.int32), misc.py:189,194) */
int ml_threshold_i32(const float *in, int32_t *out, float threshold, int64_t n, void *stream);

/* SemanticSmoothing.call (engine/layers/semantic.py:270-285) for all classes at once: per channel c a
 * grey opening -- tf.nn.erosion2d then tf.nn.dilation2d with an all-zero kernel_sizes[c]^2 element,
 * stride 1, SAME (window rows y-(k-1)/2 .. +k-1, positions outside the map ignored) -- times
 * weights[c]; kernel_sizes[c] <= 0 only applies the weight.  in/out/tmp: three distinct [B,H,W,C]
 * buffers; kernel_sizes / weights are HOST arrays of C entries (C <= ML_SMOOTH_MAX_CLASSES).        */
int ml_semantic_smoothing_f32(const float *in, float *out, float *tmp, int32_t B, int32_t H, int32_t W, int32_t C,
                              const int32_t *kernel_sizes, const float *weights, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Serving post-processing (reference road_project/setup/serving.py:28-50) -- SURVEY section 8(f) rank 4.
 * Only the arithmetic layers: JPEG decode / drawing / encode are outside this library.
 * ------------------------------------------------------------------------------------------- */

/* CropAndPadMask.call (engine/layers/misc.py:358-401): det [B,n,6] int32 (cx,cy,w,h,label,conf*100 from
 * UpSampleOutput), masks [B,n,mh,mw] int32 -> out [B,n,H,W] f32: for every row with conf >= threshold
 * (threshold = 50 if max(conf) > 50 else -100) the mask resized bilinear(align_corners=True) to its box
 * (box = max(box, 1); corners ceil(c -+ size/2) clipped to the canvas) and zero padded to H x W; other
 * rows zero.  A box clipped to zero size pastes nothing (the reference's resize would raise).
 * threshold_ws: one int32 of device scratch.                                                       */
int ml_crop_pad_mask_f32(const int32_t *det, const int32_t *masks, float *out, int32_t *threshold_ws,
                         int32_t B, int32_t n, int32_t mh, int32_t mw, int32_t H, int32_t W, void *stream);

/* CrackToInstance.call bounding box (engine/layers/misc.py:533-541): min / max (y, x) of the non-zero
 * entries of channel `coff` of an int32 [B,H,W,cstride] map over the WHOLE batch.  box5 (device, caller
 * initialises to {INT32_MAX, INT32_MAX, -1, -1, 0}) receives {ymin, xmin, ymax, xmax, any}.           */
int ml_nonzero_bbox_i32(const int32_t *map, int32_t B, int32_t H, int32_t W, int32_t cstride, int32_t coff,
                        int32_t *box5, void *stream);

/* SummaryOutput's per-instance numbers (engine/layers/misc.py:574-589): CalculateInstanceSize (:632-718:
 * per image row the min / max x of the `road_channel` pixels > 0, rows with min != max, 15 % dropped at
 * both ends, least-squares lines x(y) of the left and right edge -- float32 normal equations, 2x2 LU with
 * partial pivoting like tf.linalg.inv --, unit[y] = default_road_size / clip(right - left, 1, inf)) and
 * IncludeMyRoad (:601-618).  seg [B,H,W,seg_channels] int32, masks [B,n,H,W] f32 (CropAndPadMask output)
 * -> out5 [B,n,5] = {pixel sum, instance size, horizontal size, vertical size, include_my_road}.     */
int64_t ml_instance_summary_workspace_bytes(int32_t B, int32_t H);
int ml_instance_summary_f32(const int32_t *seg, int32_t seg_channels, int32_t road_channel, const float *masks,
                            float *out5, int32_t B, int32_t n, int32_t H, int32_t W, float default_road_size,
                            float ioi_threshold, void *workspace, void *stream);
/* The same numbers WITHOUT the padded canvases: CropAndPadMask (misc.py:358-401) and SummaryOutput's arithmetic
 * (:574-589) in one pass.  det [B,n,6] int32 and roi_masks [B,n,mh,mw] int32 are CropAndPadMask's inputs; every canvas
 * value is recomputed on the fly with that layer's arithmetic and only the rows / columns a box covers are visited
 * (what is skipped is exactly zero), so out5 is bit-identical to ml_crop_pad_mask_f32 followed by
 * ml_instance_summary_f32 while the [B,n,H,W] tensor (3.4 GB at 8 x 100 x 1024^2) is never written or read.
 * Same workspace size as ml_instance_summary_f32.                                                        */
int ml_instance_summary_rois_f32(const int32_t *seg, int32_t seg_channels, int32_t road_channel, const int32_t *det,
                                 const int32_t *roi_masks, float *out5, int32_t B, int32_t n, int32_t mh, int32_t mw,
                                 int32_t H, int32_t W, float default_road_size, float ioi_threshold, void *workspace,
                                 void *stream);

/* ---------------------------------------------------------------------------------------------
 * Serving 'visualize' output (road_project/setup/serving.py:30-40; engine/layers/misc.py:404-503).
 * Frames are uint8 [B,H,W,3]; det int32 [B,n,6] = (cx, cy, w, h, class, conf) as UpSampleOutput writes it.
 * blend(v, S, alpha) = uint8(trunc(clip(v + S * alpha, 0, 255))) in fp32 without fused multiply-add, S = sum over k in
 * order of colors[k] * map_k.  Colour tables are HOST arrays [K][3] of fp32, 1 <= K <= ML_DRAW_MAX_CLASSES.
 * `out` may be the input frame buffer itself; no other overlap is allowed.
 * ------------------------------------------------------------------------------------------- */
#define ML_DRAW_MAX_CLASSES 16

/* DrawBoxes.call (misc.py:478-503): out = images with every row's box drawn as a white 1-pixel outline by the rule
 * of tf.image.draw_bounding_boxes: box = max(det[:4], 0), normalised corners (c -+ size/2) / (W | H), line rows /
 * columns trunc(corner * (H-1 | W-1)) in 64 bits; boxes that are inverted or wholly outside are skipped, lines
 * outside the frame are not drawn.  Every row is drawn whatever its class or confidence.                   */
int ml_draw_boxes_u8(const uint8_t *images, const int32_t *det, uint8_t *out, int32_t B, int32_t n, int32_t H, int32_t W,
                     void *stream);
/* DrawInstance.call (misc.py:434-475): masks = CropAndPadMask's fp32 [B,n,H,W]; per class k < K the masks of the rows
 * with det class == k summed in row order from 0.0f, > 0.5 -> 1; then DrawSegmentation's blend.  Rows of any other
 * class (padding: -1) are never drawn.                                                                      */
int ml_draw_instance_u8(const uint8_t *images, const int32_t *det, const float *masks, uint8_t *out, const float *colors,
                        int32_t K, float alpha, int32_t B, int32_t n, int32_t H, int32_t W, void *stream);
/* DrawSegmentation.call (misc.py:404-431): maps [B,H,W,K], int32 (maps_are_f32 = 0) or fp32.                  */
int ml_draw_segmentation_u8(const uint8_t *images, const void *maps, int32_t maps_are_f32, uint8_t *out,
                            const float *colors, int32_t K, float alpha, int32_t B, int32_t H, int32_t W, void *stream);
/* The whole 'visualize' output in one pass: DrawBoxes -> DrawInstance(instance colours) over CropAndPadMask of
 * (det, ins [B,n,mh,mw] int32) -> DrawSegmentation(semantic colours) of seg [B,H,W,Ks] int32.  The pasted values are
 * recomputed inside their boxes with CropAndPadMask's arithmetic (threshold: 50 if the batch's max conf > 50, else
 * -100, computed on the device into threshold_ws, one int32), so the bytes equal the three layers over
 * ml_crop_pad_mask_f32's canvases without building them.  No host synchronisation: graph-capturable.        */
int ml_serving_visualize_u8(const uint8_t *images, const int32_t *det, const int32_t *ins, const int32_t *seg, uint8_t *out,
                            int32_t *threshold_ws, const float *instance_colors, int32_t Ki, float instance_alpha,
                            const float *semantic_colors, int32_t Ks, float semantic_alpha, int32_t B, int32_t n,
                            int32_t mh, int32_t mw, int32_t H, int32_t W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Serving 'visualize' content: EncodeImageContent (engine/layers/misc.py:343-351, tf.io.encode_jpeg with its
 * defaults).  Baseline sequential DCT, 8 bit, Y Cb Cr sampled 2x2 / 1x1 / 1x1 in one interleaved scan, no restart
 * markers, the Annex K quantisation tables scaled by the libjpeg quality rule (s = 5000 / q below 50, else 200 - 2 q;
 * Q = clamp((base * s + 50) / 100, 1, 255)), the four Annex K Huffman tables, a JFIF APP0 header (300 x 300 dpi).
 * Samples: Y = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16, Cb = (-FIX(.16874) R - FIX(.33126) G +
 * FIX(.5) B + (128 << 16) + 32767) >> 16, Cr = (FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
 * with FIX(x) = int(x * 65536 + 0.5); planes padded to a multiple of 16 by replicating the last column and row (those
 * samples are encoded: no "dummy" blocks); chroma the 2x2 box (a + b + c + d + bias) >> 2, bias 1 / 2 in even / odd
 * output columns; level shift -128; the orthonormal 8x8 DCT of T.81 A.3.3 in fp32; coefficient = trunc(|v| / Q + 0.5)
 * with the sign of v.
 * ------------------------------------------------------------------------------------------- */
/* Bytes per image that no H x W frame can exceed at any quality: the header, twice (byte stuffing) the scan at the
 * longest code plus magnitude bits for every coefficient (DC 11 + 11, AC 16 + 10 bits), EOI; a multiple of 16.
 * ML_E_BADARG for a non-positive dimension, one above 65535 or a frame whose bit offsets pass 32 bits.       */
int64_t ml_jpeg_encode_capacity(int32_t H, int32_t W);
int64_t ml_jpeg_encode_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* images uint8 [B,H,W,3] -> out uint8 [B,capacity]: image b's file is out[b][0 .. lengths[b]), lengths int32 [B].
 * 1 <= quality <= 100 (the reference uses 95), capacity >= ml_jpeg_encode_capacity(H, W), workspace 16-byte
 * aligned and of ml_jpeg_encode_workspace_bytes(B, H, W); no buffer may overlap another.  The bytes depend only on
 * (frame, quality).  No host synchronisation: graph-capturable.                                              */
int ml_jpeg_encode_u8(const uint8_t *images, int32_t B, int32_t H, int32_t W, int32_t quality, uint8_t *out,
                      int64_t capacity, int32_t *lengths, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Serving request: DecodeImageContent for baseline JPEG, the bytes libjpeg-turbo's default decode gives (JDCT_ISLOW,
 * fancy upsampling: what Pillow and tf.io.decode_jpeg use).  The host parses and Huffman-decodes the stream into a
 * packed sparse form (no device needed); the device does the per-pixel work.  All of it is integer arithmetic, >> is
 * arithmetic, DESCALE(x, n) = (x + (1 << (n - 1))) >> n:
 *   dequantise c[i] = coef[i] * Q[i] (natural order);
 *   the 8x8 IDCT of Loeffler, Ligtenberg and Moschytz with CONST_BITS 13, PASS1_BITS 2 (constants round(x * 8192):
 *   2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172), down the columns with DESCALE 11, then along
 *   the rows with DESCALE 18; sample = clamp(v + 128, 0, 255).  A block with only a DC term is the constant
 *   clamp(((dc * Q0 + 4) >> 3) + 128);
 *   of a component's padded plane only the first ceil(H v / vmax) rows and ceil(W h / hmax) columns are read;
 *   2x2 chroma ("h2v2 fancy"): the real plane replicated by one sample on every side, colsum = 3 c[r][x] + c[r - 1][x]
 *   for output row 2r and 3 c[r][x] + c[r + 1][x] for row 2r + 1, out[2x] = (3 colsum[x] + colsum[x - 1] + 8) >> 4,
 *   out[2x + 1] = (3 colsum[x] + colsum[x + 1] + 7) >> 4;
 *   with FIX(a) = int(a * 65536 + 0.5), cb = Cb - 128, cr = Cr - 128: R = clamp(Y + ((FIX(1.402) cr + 32768) >> 16)),
 *   G = clamp(Y + ((-FIX(.34414) cb + 32768 - FIX(.71414) cr) >> 16)), B = clamp(Y + ((FIX(1.772) cb + 32768) >> 16));
 *   4:4:4 has no upsampling step, grayscale writes Y to the three channels.
 * The IDCT runs in 64-bit integers: the formulas hold as written for every int16 coefficient (libjpeg itself wraps
 * once dequantised or pass-1 values leave 16 bits, which no stream encoded from pixels does).
 *
 * Taken: SOF0, 8 bit, Huffman, one interleaved scan of three components sampled 2x2/1x1/1x1 (ML_JPEG_420) or all 1x1
 * (ML_JPEG_444), or one 1x1 component (ML_JPEG_GRAY); any table ids and contents (8-bit DQT); DRI restart intervals;
 * APPn / COM are skipped; a side of at most 16384.  Not taken ("unsupported", a normal answer): progressive, extended,
 * lossless and arithmetic frames, other sampling, 4 components, an Adobe APP14 transform other than YCbCr, components
 * 'R' 'G' 'B' without a JFIF marker, scans of fewer components than the frame, 16-bit DQT, anything that is not a JPEG.
 *
 * Packed form of one image (16-byte aligned, a multiple of 16 bytes): 224-byte header { u32 magic, i32 H, W, mode,
 * u32 blocks, entries, bytes, reserved, u8 Q[3][64] per component in natural order }, u32 block_start[blocks + 1],
 * u32 word[entries]: natural-order index << 16 | the int16 value's 16 bits.  Blocks in scan order; a block's first
 * word is its un-predicted DC term (always present); indices < 64, distinct within a block; offsets monotone.
 * ------------------------------------------------------------------------------------------- */
enum { ML_JPEG_GRAY = 0, ML_JPEG_444 = 1, ML_JPEG_420 = 2 };
#define ML_JPEG_UNSUPPORTED 1
#define ML_JPEG_DECODE_MAX_BATCH 32    /* streams per call of the device entries below (decode and entropy) */
/* Host.  info int32[4] = { H, W, mode, blocks }.  ML_OK: the device path takes the stream; ML_JPEG_UNSUPPORTED: it does
 * not (ml_last_error says why; also for a header that cannot be read) -- decode it elsewhere.                */
int ml_jpeg_decode_info(const uint8_t *data, int64_t n, int32_t *info);
/* Host.  Bytes no packed form of this stream exceeds (the header, the offsets, and per block the smaller of 64 words
 * and what n bytes of scan can hold at two bits a word); ML_E_BADARG if the stream is not taken.              */
int64_t ml_jpeg_decode_packed_bytes(const uint8_t *data, int64_t n);
/* Host.  Huffman-decodes the whole scan into `packed` (4-byte aligned, `capacity` bytes) and returns the bytes
 * written, or ML_E_BADARG with the reason: a truncated segment or scan, an undefined table, a code that is not in
 * its table, a run past coefficient 63, a DC category above 11 or an AC size above 10, a wrong or missing RSTn, a
 * missing EOI, a full buffer.  Never reads beyond data[n) or writes beyond packed[capacity).                 */
int64_t ml_jpeg_decode_entropy(const uint8_t *data, int64_t n, void *packed, int64_t capacity);
/* Device.  Planar uint8 Y, Cb, Cr of B images (1 <= B <= ML_JPEG_DECODE_MAX_BATCH) between the two launches. */
int64_t ml_jpeg_decode_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t mode);
/* Device.  `packed`: B packed images of the same H, W and mode in one device buffer, image b at byte offsets[b]
 * (host array of B + 1, offsets[B] = the end; 16-byte aligned) -> out uint8 [B,H,W,3] (4-byte aligned, below 2^31
 * bytes).  Two
 * launches on `stream`, no host read, no atomics: one writer per byte.  H, W, mode must be those of the packed images
 * (the kernels trust the packed form as ml_jpeg_decode_entropy writes it).                                    */
int ml_jpeg_decode_u8(const void *packed, const int64_t *offsets, int32_t B, int32_t H, int32_t W, int32_t mode,
                      uint8_t *out, void *workspace, void *stream);
/* Host.  The same per-thread code in CPU loops, every pointer in host memory; it also verifies the packed form's
 * invariants.  For checking the arithmetic without a device -- not a product path.                            */
int ml_jpeg_decode_reference_host(const void *packed, const int64_t *offsets, int32_t B, int32_t H, int32_t W,
                                  int32_t mode, uint8_t *out, void *workspace);

/* ---------------------------------------------------------------------------------------------
 * The entropy half of the request decoder on the device.  Contract: for every stream ml_jpeg_decode_info answers
 * ML_OK for, status 0 means that `packed` holds the packed form ml_jpeg_decode_entropy writes, byte for byte over the
 * `bytes` of its header (the 224-byte header, block_start[blocks + 1], one word per non-zero coefficient with the DC
 * term un-predicted and first, the zero padding to 16 bytes): ml_jpeg_decode_u8 then runs on it unchanged.  A non-zero
 * status means: run the host decoder, which stays the oracle and says what is wrong, if anything is.
 *
 * Self-synchronising parallel Huffman decoding.  The raw scan is cut into subsequences of geometry[0] bits, one
 * thread each, geometry[1] subsequences a workgroup.  Every thread decodes from a guessed state, takes over its
 * predecessor's exit state until the two agree (inside a workgroup in rounds, across workgroups in a fixed number of
 * launches: no workgroup waits on another), a prefix sum gives each subsequence its word and block positions and DC
 * predictors, and a last pass decodes from the settled states, stores, checks every condition the host decoder
 * checks and that each thread ends in the state its successor began in.  FF 00 stuffing is undone in place; an RSTn
 * marker resets a thread to block 0 of an MCU.  Every read is bounded by the file's length, every store by the
 * capacity.  Launches on `stream`, no host read; the statuses are in device memory.  Where the status is not 0 the
 * words behind the header are cleared (every block reads as empty: ml_jpeg_decode_u8 may safely follow in the stream).
 *
 * Outcome, int32 status[4 b ..]: the status below; the block index it refers to, or -1; the most rounds a
 * workgroup needed to settle; the last launch (0 ..) in which a state crossed a workgroup boundary.           */
enum {
    ML_JPEG_ENTROPY_OK = 0,
    ML_JPEG_ENTROPY_BAD_CODE = 1,    /* a code that is not in its table                                        */
    ML_JPEG_ENTROPY_BAD_DC = 2,      /* DC category above 11                                                   */
    ML_JPEG_ENTROPY_BAD_AC = 3,      /* AC size above 10, or a run/size symbol n0 other than EOB and ZRL       */
    ML_JPEG_ENTROPY_RUN = 4,         /* a run past coefficient 63                                              */
    ML_JPEG_ENTROPY_TRUNCATED = 5,   /* the scan ends inside a block                                           */
    ML_JPEG_ENTROPY_BLOCKS = 6,      /* the scan does not hold `blocks` blocks                                 */
    ML_JPEG_ENTROPY_RESTART = 7,     /* an RSTn that is not due, out of sequence or repeated                   */
    ML_JPEG_ENTROPY_NO_EOI = 8,      /* no EOI after the last MCU                                              */
    ML_JPEG_ENTROPY_CAPACITY = 9,    /* a store beyond `capacity` was withheld                                 */
    ML_JPEG_ENTROPY_ASK_HOST = 10,   /* whole bytes between an MCU's last bit and a due RSTn: whether the host decoder
                                        takes the marker depends on how far its reader had read ahead          */
    ML_JPEG_ENTROPY_NOT_SYNCED = 11, /* the states had not settled within the fixed rounds: a well-formed stream
                                        may end so; it takes precedence over the codes above, which may follow from it */
    ML_JPEG_ENTROPY_BAD_PLAN = 12    /* the plan is not this file's, or the capacity is below the fixed part   */
};
/* Host.  geometry int32[2] = { bits per subsequence, subsequences per workgroup }.                            */
int ml_jpeg_entropy_geometry(int32_t *geometry);
/* Host.  The plan of one stream (ml_jpeg_entropy_plan_bytes() bytes, 8-byte aligned; 16-byte aligned slots in a batch):
 * geometry, the scan's offset, its first marker that is no RSTn, the restart interval, the dequantisation tables, and per component the DC and AC
 * Huffman tables in lookup form (9-bit `fast` table, maxcode / valoff / vals for longer codes).  ML_E_BADARG with the
 * host decoder's reason for a stream that is not taken, truncated before SOS or without one of its tables.    */
int64_t ml_jpeg_entropy_plan_bytes(void);
int ml_jpeg_entropy_plan(const uint8_t *data, int64_t n, void *plan);
/* Host.  Workspace of a call over B streams (1 <= B <= ML_JPEG_DECODE_MAX_BATCH), stream b being
 * file_offsets[b + 1] - file_offsets[b] bytes. */
int64_t ml_jpeg_entropy_workspace_bytes(const int64_t *file_offsets, int32_t B);
/* Device.  files: the raw files in one device buffer, stream b at byte file_offsets[b] (host array of B + 1);
 * plans: B plans, ml_jpeg_entropy_plan_bytes() apart; packed: stream b's packed form goes to byte packed_offsets[b]
 * (host array of B + 1, multiples of 16; the room up to packed_offsets[b + 1] is its capacity, at least
 * ml_jpeg_decode_packed_bytes); status int32 [4 B] and workspace in device memory, plans / packed / status / workspace 16-byte
 * aligned.  Six launches, graph-capturable.                                                                    */
int ml_jpeg_entropy_device(const uint8_t *files, const int64_t *file_offsets, const void *plans, int32_t B, void *packed,
                           const int64_t *packed_offsets, int32_t *status, void *workspace, void *stream);
/* Host.  The same stages in CPU loops over one stream, every pointer in host memory (workspace:
 * ml_jpeg_entropy_workspace_bytes of {0, n}, 8-byte aligned; status int32[4]).  Not a product path.            */
int ml_jpeg_entropy_reference_host(const uint8_t *file, int64_t n, const void *plan, void *packed, int64_t capacity,
                                   int32_t *status, void *workspace);

/* ---------------------------------------------------------------------------------------------
 * Evaluation: the reference's evaluation loop (road_project/train.py:101-209) and its metric layers
 * (engine/metrics.py) as integer counting kernels (csrc/evaluate.hip).  Every kernel counts into zeroed int64
 * outputs with integer atomics: the same bits run to run; no float atomics.  All on `stream`, no host read.
 *
 * The loop's contract per image (what masklab_hip/evaluate.py and tests/evaluate_ref.py both follow):
 *   boxes     matched on the HOST in float64 (train.py:144-182): iou = intersection / union of the (cx, cy, w, h) boxes,
 *             times label equality, pairs = np.where(iou > 0.5) in row-major order; NaN compares false; a predicted
 *             row with conf < 0 and a ground-truth row with label < 0 never pair.
 *   pred mask of detection row j (train.py:125-141): in float64 xmin = clip(cx - w/2, 0, W), xmax, ymin, ymax likewise;
 *             start / end = those truncated to int32; bw = end.x - start.x, bh = end.y - start.y.  Canvas pixel (y, x) is
 *             set iff it lies in [start.y, end.y) x [start.x, end.x) and the bilinear sample of max(mask_j, 0) at
 *             (y - start.y, x - start.x) of a bh x bw resize is > 0.5.  The resize is OpenCV's INTER_LINEAR for a float64
 *             image, restated per axis: scale = 1 / (dst / src) in float64; f = float32((d + 0.5) * scale - 0.5);
 *             s = floor(f); f -= s in float32; s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0; weights
 *             1.f - f and f (float32); the two taps of a source row are combined first, then the two rows, in float64.
 *             bw <= 0 or bh <= 0 is an EMPTY mask (the reference raises inside cv2.resize).  This restatement, not a run
 *             of OpenCV, is what the kernels are held to.
 *   gt mask   pixel set iff its byte is non-zero (int8 -1 from a 0 / 255 mask counts).
 *   pair      intersection and union = pred area + gt area - intersection as integers; the host divides in float64
 *             (0 for an empty union, where the reference adds NaN).
 *   semantic  per class, #(gt > 0.5 and pr > 0.5) and #(gt > 0.5 or pr > 0.5).
 * ------------------------------------------------------------------------------------------- */
#define ML_EVAL_MAX_CLASSES 16
#define ML_EVAL_MAX_MASK 16368      /* mh * mw of ml_eval_mask_pairs: 64 KiB of LDS less the reduction's own words */
enum { ML_EVAL_F32 = 0, ML_EVAL_F16 = 1, ML_EVAL_I32 = 2, ML_EVAL_U8 = 3 };
/* gt [B,G,H,W] int8 or uint8 (H*W < 2^31) -> out int64 [B,G]: non-zero bytes per mask.  HBM-bound: 16-byte loads,
 * scalar bytes in front of the first 16-byte boundary and for the last (H*W - head) mod 16.                      */
int ml_eval_mask_area(const void *gt, int32_t B, int32_t G, int32_t H, int32_t W, int64_t *out, void *stream);
/* det [B,n,6] int32, ins [B,n,mh,mw] int32 (mh*mw <= ML_EVAL_MAX_MASK: the mask is held in LDS), gt as above, gt_area from
 * ml_eval_mask_area, pairs int32 [P,3] = (b, pr_i, gt_i) on the device -> out int64 [P,2] = (intersection, union).
 * The blocks of a pair walk only its box.  A pair with an index out of range gets (-1, -1) and reads nothing.     */
int ml_eval_mask_pairs(const int32_t *det, const int32_t *ins, const void *gt, const int64_t *gt_area, const int32_t *pairs,
                       int32_t P, int32_t B, int32_t n, int32_t mh, int32_t mw, int32_t G, int32_t H, int32_t W, int64_t *out,
                       void *stream);
/* pr int32 [B,H,W,C], gt uint8 [B,H,W,C] (16-byte aligned, C <= ML_EVAL_MAX_CLASSES, H*W*C < 2^31, B <= 65535)
 * -> out int64 [B,C,2] = (intersection, union) of gt > 0.5 and pr > 0.5.                                           */
int ml_eval_semantic_counts(const int32_t *pr, const uint8_t *gt, int32_t B, int32_t H, int32_t W, int32_t C, int64_t *out,
                            void *stream);
/* ClassBinaryIOU.call (engine/metrics.py:83-99): seg_true, seg_pred [B,HW,C] of dtype ML_EVAL_* (both the same, or u8
 * truth with i32 predictions; limits as above) -> counts int64 [B,C,3] = #(true > thr), #(pred > thr), #(both), and
 * iou float32 [C,B] = intersection / (area_true + area_pred - intersection) in float32, 1 where the union is 0.  Values are
 * compared with the float32 threshold as they are (f16 widened exactly); TensorFlow would round the threshold to the
 * map's type first, the same thing at 0.5.                                                                          */
int ml_eval_class_binary_iou(const void *seg_true, int32_t true_dtype, const void *seg_pred, int32_t pred_dtype, int32_t B,
                             int64_t HW, int32_t C, float threshold, int64_t *counts, float *iou, void *stream);
/* DetectionIOUMetric.call (engine/metrics.py:118-165): proposed [B,n_proposed,6], gt [B,n_gt,6] float32, rows padded
 * with -1 -> out float32 [3,B] = precision, recall, fmeasure.  Float32 with FP contraction off: CalculateIOU with its
 * + 1e-5, the logical_or ignore mask as written, K.epsilon() = 1e-7 -- the bits of oracle/metrics.py.             */
int ml_eval_detection_metric_f32(const float *proposed, const float *gt, int32_t B, int32_t n_proposed, int32_t n_gt, float *out,
                                 void *stream);
/* ConfusionMatrixMetric.call (engine/metrics.py:16-60): cls_true, cls_pred float32 [N,C], mask float32 [N] -> counts
 * int64 [4] = tp, fp, fn, tn (argmax per anchor, the first maximum wins; the prediction counts as background unless its
 * row maximum > threshold, the truth unless mask == 0; anchors with mask == -1 are dropped) and metrics float32 [4] =
 * precision, recall, accuracy, fmeasure from them in float32.                                                      */
int ml_eval_confusion_f32(const float *cls_true, const float *cls_pred, const float *mask, int64_t N, int32_t C, float threshold,
                          int64_t *counts, float *metrics, void *stream);
/* Host.  The per-thread code of the mask-area, mask-pair and semantic kernels in CPU loops, every pointer in host
 * memory; a section whose inputs are null is skipped (gt -> out_area; pairs -> out_pairs, which needs det, ins, gt;
 * pr_sem, gt_sem -> out_sem).  For checking the arithmetic without a device -- not a product path.                 */
int ml_eval_reference_host(const int32_t *det, const int32_t *ins, const void *gt, const int32_t *pairs, int32_t P,
                           const int32_t *pr_sem, const uint8_t *gt_sem, int32_t B, int32_t n, int32_t mh, int32_t mw, int32_t G,
                           int32_t H, int32_t W, int32_t C, int64_t *out_area, int64_t *out_pairs, int64_t *out_sem);

/* ---------------------------------------------------------------------------------------------
 * Trainer forward: the reference's target assignment (AssignBoxes engine/layers/detection.py:589-697, AssignMasks
 * instance.py:296-386, AssignSeg semantic.py:304-311) and its four loss layers (engine/losses.py), forward only
 * (assignment: csrc/train_targets.hip; losses: csrc/train_losses.hip; the losses' gradients are the next block).  All on `stream`, no host read.  No float atomics: a sum is float64 partials per block in
 * `workspace` (ml_train_workspace_bytes) added in block order by a finishing kernel -- the same bits run to run.  Per-element
 * terms are float32 with FP contraction off, as tests/trainer_ref.py evaluates them; sums are float64.
 * Gradients stop at the head outputs ("Trainer backward: the losses").  NOT supported: predictions or truths in float16
 * (cast first); more than ML_EVAL_MAX_CLASSES semantic classes;
 * more than 32 images in ml_train_mask_loss_f32 (MoldBatch); gt_masks other than int8 / uint8; NaN boxes (a NaN IoU orders
 * above every number in the packed maximum, where tf.argmax leaves it unspecified).
 * The reference's quirks are kept: a ground truth whose best prior also has IoU >= 0.5 enters that prior twice (loc_true
 * is a SUM over match entries, the label is the LAST entry's); an IoU in [0.4, 0.5) to ANY ground truth makes the anchor
 * ignored even if it is positive for another; a valid ground truth with IoU 0 everywhere is assigned to prior 0; BoxLoss
 * updates its moving statistics on every call and picks the quadratic branch where |d| - beta/2 < beta.
 * ------------------------------------------------------------------------------------------- */
#define ML_TRAIN_MAX_BLOCKS 512     /* partial sums per image */
enum { ML_TRAIN_MASK_I8 = 0, ML_TRAIN_MASK_U8 = 1 };
/* bytes of `workspace` for the loss kernels below on B images and C classes (C = 1 serves ml_train_box_loss_f32)     */
int64_t ml_train_workspace_bytes(int32_t B, int32_t C);
/* CalculateIOU.call (detection.py:391-422): aa [n, aa_stride], bb [m, bb_stride] float32 rows of (cx, cy, w, h, ...)
 * -> out float32 [n,m], the bits of oracle/metrics.py::calculate_iou.                                                 */
int ml_train_calculate_iou_f32(const float *aa, int32_t aa_stride, int32_t n, const float *bb, int32_t bb_stride, int32_t m, float *out,
                               void *stream);
/* gt_boxes [B,G,6] float32 (cx, cy, w, h, class, conf; rows padded with -1), pr_boxes [A,4] int32 (one table for the batch)
 * -> best int32 [B,G]: the FIRST index of the row maximum of iou[b,g,:] = CalculateIOU * (gt cx != -1); a row of zeros
 * gives 0.  keys: uint64 [B,G] scratch (packed (IoU bits, ~index) under an integer atomic maximum).                   */
int ml_train_best_prior_f32(const float *gt_boxes, const int32_t *pr_boxes, int32_t B, int32_t G, int32_t A, void *keys, int32_t *best,
                            void *stream);
/* AssignBoxes.call: -> cls_true [B,A,C] (one-hot without the background column), loc_true [B,A,4], assign_mask [B,A]
 * (-1 ignored, 0 positive, 1 negative), all float32.  One thread per anchor, the ground truths tiled through LDS.    */
int ml_train_assign_boxes_f32(const float *gt_boxes, const int32_t *pr_boxes, const int32_t *best, int32_t B, int32_t G, int32_t A,
                              int32_t C, float *cls_true, float *loc_true, float *assign_mask, void *stream);
/* ClassLoss.call (losses.py:21-41): cls_true, cls_pred [B,A,C], assign_mask [B,A], cls_exists [B,C] float32 -> out [B].  */
int ml_train_class_loss_f32(const float *cls_true, const float *cls_pred, const float *assign_mask, const float *cls_exists, int32_t B,
                            int32_t A, int32_t C, float weight, float alpha, float gamma, void *workspace, float *out, void *stream);
/* BoxLoss.call (losses.py:76-104): loc_true, loc_pred [B,A,4] (16-byte aligned), assign_mask [B,A] -> out [B].  With
 * use_adjust, `state` float32 [8] = moving_mean[4], moving_var[4] in device memory is read AND updated (three passes:
 * mean, variance, loss); without, beta is the constant and `state` may be null (one pass).                           */
int ml_train_box_loss_f32(const float *loc_true, const float *loc_pred, const float *assign_mask, int32_t B, int32_t A, float weight,
                          float momentum, float one_minus_momentum, float beta, int32_t use_adjust, float *state, void *workspace,
                          float *out, void *stream);
/* AssignMasks.call: roi_boxes [B,R,6], gt_boxes [B,G,6] float32, gt_masks [B,G,H,W] int8 / uint8 (ML_TRAIN_MASK_*)
 * -> out int32 [B,R,mh,mw]: the matched class where the crop sample is > 0.5, otherwise C; an unmatched RoI is C.      */
int ml_train_assign_masks(const float *roi_boxes, const float *gt_boxes, const void *gt_masks, int32_t mask_dtype, int32_t B, int32_t R,
                          int32_t G, int32_t H, int32_t W, int32_t mh, int32_t mw, int32_t C, float threshold, int32_t *out,
                          void *stream);
/* MaskLoss.call (losses.py:126-159): mask_true int32 [B,R,mh,mw], mask_pred float32 [B,R,mh,mw,C] -> out [B];
 * keep = 1 - label_smoothing, half_smooth = label_smoothing / 2; roi_loss: float32 [B,R] scratch (the per-RoI means).  */
int ml_train_mask_loss_f32(const int32_t *mask_true, const float *mask_pred, int32_t B, int32_t R, int32_t mh, int32_t mw, int32_t C,
                           float weight, float keep, float half_smooth, float *roi_loss, float *out, void *stream);
/* AssignSeg.call: gt_seg [B,H,W,C] float32 or uint8 (ML_EVAL_F32 / ML_EVAL_U8) -> out float32 [B,oh,ow,C] =
 * round-half-to-even of resize_bilinear(align_corners=True).                                                          */
int ml_train_assign_seg(const void *gt_seg, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, int32_t oh, int32_t ow, float *out,
                        void *stream);
/* SegLoss.call (losses.py:179-193): seg_true, seg_pred [B,HW,C], seg_exist [B,C] float32 (C <= ML_EVAL_MAX_CLASSES) -> out [B]. */
int ml_train_seg_loss_f32(const float *seg_true, const float *seg_pred, const float *seg_exist, int32_t B, int64_t HW, int32_t C,
                          float weight, float keep, float half_smooth, void *workspace, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Trainer backward: the losses (csrc/train_losses.hip, the forward's own kernel source).  Each call is its forward twin above -- the same arguments, the same
 * `workspace`, the same loss in `out`, BIT FOR BIT -- plus
 *   upstream         float32 [B] on the device: d(scalar) / d(loss[b]); 1 / B for the scalar the reference compiles
 *                    (add_loss(K.mean(loss)) per loss layer);
 *   through_sigmoid  non-zero: the gradient is additionally multiplied by pred * (1 - pred), which makes it the gradient at
 *                    the pre-activation of the sigmoid the 1x1 output convs fuse (BoxLoss has no such argument);
 *   grad             float32, shaped like the prediction: d(sum_b upstream[b] * loss[b]) / d(prediction).  EVERY element is
 *                    written in the pass that sums the loss, the zeros included (ignored anchors, non-positive anchors of
 *                    the box gradient, RoIs that are not selected, the other class channels of a selected RoI).
 * These are the gradients TensorFlow gives for the reference's expressions.  Whatever reaches a loss only through a count, a
 * comparison or an assigned variable is a CONSTANT: num_tot, num_pos, MaskLoss's count_nonzero + 1, the branch of the clip
 * and of smooth-L1, and BoxLoss's beta (the read of an assigned variable).  With c_b = weight * upstream[b]:
 *   ClassLoss  p = clip(pred, eps, 1 - eps), t = (cls_true != 0), pt = t ? p : 1 - p;
 *              grad = c_b / (num_tot_b + eps) * keep * cls_exists[b,c] * (t ? 1 : -1)
 *                     * alpha * (gamma * (1 - pt)^(gamma - 1) * log pt - (1 - pt)^gamma / pt),
 *              and 0 where pred < eps or pred > 1 - eps (equality passes, as tf.clip_by_value's gradient does);
 *   BoxLoss    d = true - pred on positive anchors; grad = c_b / (num_pos_b + eps) / 4 * (|d| - beta/2 < beta ? -d / beta
 *              : -sign(d)); zeros elsewhere, so an image without a positive anchor gets exact zeros.  With use_adjust the
 *              moving statistics move ONCE per call, as by one forward call, and beta is this call's;
 *   MaskLoss   for an RoI whose class cls = min(target) < C, channel cls only:
 *              grad = c_b / (nz_b + 1) / (mh * mw) * dBCE, nz_b = the image's RoIs with a non-zero loss;
 *   SegLoss    grad = c_b * seg_exist[b,c] / (C * HW) * dBCE;
 *   dBCE/dp = -(y / (p + eps) - (1 - y) / (1 - p + eps)), y = keep * t + half_smooth.
 * No float atomics, float32 terms with FP contraction off, float64 partial sums in block order; on `stream`, no host read.
 * ------------------------------------------------------------------------------------------- */
int ml_train_class_loss_grad_f32(const float *cls_true, const float *cls_pred, const float *assign_mask, const float *cls_exists,
                                 int32_t B, int32_t A, int32_t C, float weight, float alpha, float gamma, void *workspace, float *out,
                                 const float *upstream, int32_t through_sigmoid, float *grad, void *stream);
/* grad [B,A,4], 16-byte aligned like loc_true and loc_pred                                                            */
int ml_train_box_loss_grad_f32(const float *loc_true, const float *loc_pred, const float *assign_mask, int32_t B, int32_t A, float weight,
                               float momentum, float one_minus_momentum, float beta, int32_t use_adjust, float *state, void *workspace,
                               float *out, const float *upstream, float *grad, void *stream);
/* grad [B,R,mh,mw,C]; B <= 32 as in the forward call                                                                  */
int ml_train_mask_loss_grad_f32(const int32_t *mask_true, const float *mask_pred, int32_t B, int32_t R, int32_t mh, int32_t mw, int32_t C,
                                float weight, float keep, float half_smooth, float *roi_loss, float *out, const float *upstream,
                                int32_t through_sigmoid, float *grad, void *stream);
/* grad [B,HW,C]                                                                                                       */
int ml_train_seg_loss_grad_f32(const float *seg_true, const float *seg_pred, const float *seg_exist, int32_t B, int64_t HW, int32_t C,
                               float weight, float keep, float half_smooth, void *workspace, float *out, const float *upstream,
                               int32_t through_sigmoid, float *grad, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Generator resizes: the cv2.resize(x, (ow, oh)) calls of the reference's MaskLabGenerator (engine/utils/generator/
 * masklab.py), default INTER_LINEAR, on uint8 planes (csrc/cv_resize.hip).  OpenCV parity is unpinned: the arithmetic
 * below is restated from OpenCV's plain C++ path and held to tests/generator_ref.py, not to a run of OpenCV.
 *   axis      as in "Evaluation": scale = 1 / (dst / src) in float64; f = float32((d + 0.5) * scale - 0.5); s = floor(f);
 *             f -= s in float32; s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0; taps (s, min(s + 1, src - 1))
 *             with float32 weights (1.f - f, f).
 *   uint8     fixed point: every weight becomes (short)rint(w * 2048), half to even, each on its own; per source row
 *             r = S[x0] * a0 + S[x1] * a1 in int32; dst = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.
 *   float64   weights widened to double; h = S[x0] * wx0 + S[x1] * wx1 per source row, value = h0 * wy0 + h1 * wy1, FP
 *             contraction off; the kernel reads the uint8 source, applies np.round (rint, half to even) and writes the
 *             integer 0..255 as float32 or uint8 (both lossless).
 *   exactly 2x on BOTH axes (H == 2 * oh and W == 2 * ow): cv::resize switches to INTER_AREA -- uint8
 *             (S00 + S01 + S10 + S11 + 2) >> 2, float64 (S00 + S01 + S10 + S11) * 0.25, then the rounding.
 * src [planes,H,W,C] -> dst [planes,oh,ow,C], any alignment, plane offsets 64-bit; H*W*C < 2^31, oh*ow*C < 2^31,
 * oh <= 65535; planes == 0 is a no-op.  No workspace, no atomics, no host read; every output element is written once.
 * ------------------------------------------------------------------------------------------- */
enum { ML_CV_RESIZE_U8 = 0, ML_CV_RESIZE_ROUND_U8 = 1, ML_CV_RESIZE_ROUND_F32 = 2 };
/* The uint8 path.  With skip_minus_one a plane whose first byte is 0xFF (int8 -1, the reference's `mask[0,0] == -1.`) is
 * filled with 0xFF and nothing else of it is read.                                                                    */
int ml_cv_resize_linear_u8(const void *src, void *dst, int64_t planes, int32_t H, int32_t W, int32_t C, int32_t oh, int32_t ow,
                           int32_t skip_minus_one, void *stream);
/* The float64 path plus np.round; dst is float32 (dst_is_f32, 4-byte aligned) or uint8.                               */
int ml_cv_resize_linear_round_u8(const void *src, void *dst, int32_t dst_is_f32, int64_t planes, int32_t H, int32_t W, int32_t C,
                                 int32_t oh, int32_t ow, void *stream);
/* Host.  The kernels' per-thread code in CPU loops, both pointers in host memory; mode = ML_CV_RESIZE_*.  For checking the
 * arithmetic without a device, and the generator's device="cpu" path -- not a product path.                           */
int ml_cv_resize_reference_host(const void *src, void *dst, int32_t mode, int64_t planes, int32_t H, int32_t W, int32_t C,
                                int32_t oh, int32_t ow, int32_t skip_minus_one);

/* ---------------------------------------------------------------------------------------------
 * Dataset polygons: the polygon labels of the reference's dataset (road_project/setup/process.py draws each with
 * skimage.draw.polygon into a PNG; engine/utils/dataset/masklab.py reads the PNGs back) rasterised straight into the
 * batch's instance planes and semantic maps (csrc/polygon.hip).  skimage parity is unpinned: the rule below was written
 * down from memory of skimage's 2019 releases (later releases also count pixels lying exactly on an edge or vertex) and
 * is held to its NumPy restatement in tests/polygon_ref.py, not to a run of skimage.
 *   clip      every vertex (xp, yp), float64, first becomes (min(max(xp, 0), W - 1), min(max(yp, 0), H - 1)), as the
 *             reference clips before it draws; the library does it, on the device and on the host.
 *   inside    pixel (x, y), integer column and row taken as float64, is inside iff an odd number of edges (j -> i),
 *             j = i - 1 cyclically, satisfy both
 *                 (yp[i] <= y and y < yp[j]) or (yp[j] <= y and y < yp[i])
 *                 x < (xp[j] - xp[i]) * (y - yp[i]) / (yp[j] - yp[i]) + xp[i]
 *             in float64, evaluated in that order (multiply, divide, add), FP contraction off.
 * verts float64 [total,2] (x, y), total < 2^31; every offsets array is int32, starts at >= 0 and never decreases.  One
 * launch per call on `stream` (per 65 535 planes / images), no workspace, no atomics to global memory, no host read; every
 * output byte is written exactly once, zeros and -1 planes included; `out` needs no alignment, plane offsets are 64-bit,
 * H*W < 2^31; any vertex count per polygon.  The device entries cannot read their offsets (device memory) before the
 * launch: the kernels clamp every range to the array it indexes, so wrong offsets give wrong masks and never a read out
 * of bounds; the host entry and the Python wrappers refuse offsets that decrease or point past the end.
 * ------------------------------------------------------------------------------------------- */
enum { ML_POLYGON_INSTANCE = 0, ML_POLYGON_SEMANTIC = 1 };
/* Instance planes.  plane_offsets [B*n+1] into verts, windows [B*n,4] = (x1, y1, x2, y2) inclusive -> out int8 [B,n,H,W]:
 * a plane with an empty vertex range is padding, every byte -1; any other is 1 where the pixel is inside its polygon and
 * x1 <= x <= min(x2, W-1) and y1 <= y <= min(y2, H-1), 0 elsewhere.  B == 0 or n == 0 is a no-op.                     */
int ml_polygon_instance_masks(const double *verts, int64_t total, const int32_t *plane_offsets, const int32_t *windows, int32_t B,
                              int32_t n, int32_t H, int32_t W, void *out, void *stream);
/* Semantic maps.  poly_offsets [P+1] into verts; group_offsets [B*(S+1)+1] into the polygons, group (b, s) for s < S is
 * label s of image b and group (b, S) its "except" group -> out uint8 [B,H,W,S]: channel s is 1 where the pixel is inside
 * ANY polygon of group s (a union across polygons, even-odd within one) and inside NO polygon of the except group, else
 * 0.  S <= ML_EVAL_MAX_CLASSES; B == 0 or S == 0 is a no-op.                                                            */
int ml_polygon_semantic_maps(const double *verts, int64_t total, const int32_t *poly_offsets, int32_t P, const int32_t *group_offsets,
                             int32_t B, int32_t S, int32_t H, int32_t W, void *out, void *stream);
/* Host.  The kernels' edge, scan and store functions in CPU loops, every pointer in host memory; kind = ML_POLYGON_*:
 * INSTANCE takes offsets = plane_offsets, windows and n_or_S = n (P and group_offsets unused), SEMANTIC takes offsets =
 * poly_offsets, P, group_offsets and n_or_S = S (windows unused).  For checking the arithmetic without a device and the
 * dataset's device="cpu" path -- not a product path.                                                                   */
int ml_polygon_reference_host(int32_t kind, const double *verts, int64_t total, const int32_t *offsets, int32_t P,
                              const int32_t *group_offsets, const int32_t *windows, int32_t B, int32_t n_or_S, int32_t H, int32_t W,
                              void *out);

/* ---------------------------------------------------------------------------------------------
 * Optimizers: the reference's RectifiedAdam and AdamW (engine/optimizers.py) as one step over any number of float32
 * tensors (csrc/optimizer.hip).  A step is two launches on `stream`, no workspace, no atomics, no host read:
 *   scalars   one thread reads `state` (iterations and lr live on the device, so a captured step replays with the values
 *             of its replay), forms the step's scalars in float64, writes them as floats into `scalars`, then adds 1 to
 *             state->iterations.  With it = iterations before the add, t = it + 1, lr' = lr / (1 + decay * it) if decay > 0:
 *               RectifiedAdam  N_max = 2 / (1 - beta_2) - 1,  N = N_max - 2 t beta_2^t / (1 - beta_2^t),  rectified = N > 5,
 *                              step = lr' sqrt((1 - beta_2^t) (N - 4) / (N_max - 4) (N - 2) / N N_max / (N_max - 2)) / (1 - beta_1^t)
 *                              if rectified, else lr' / (1 - beta_1^t);  wd_lr = weight_decay lr'
 *               AdamW          lr_t = lr' sqrt(1 - beta_2^t) / (1 - beta_1^t),  eta_wd = (lr' / init_lr) weight_decay
 *   apply     per element, float32, one rounding per operation in this order (FP contraction off, correctly rounded
 *             divide and square root):
 *               m' = beta_1 m + (1 - beta_1) g,   v' = beta_2 v + (1 - beta_2) (g g)
 *               RectifiedAdam  p_ = p - wd_lr p (only if weight_decay != 0, else p_ = p)
 *                              p' = p_ - step (m' / (sqrt(v') + epsilon)) if rectified, else p' = p_ - step m'
 *               AdamW          p' = p - lr_t m' / (sqrt(v') + epsilon) - eta_wd p
 *             One launch for every tensor of the device table: the elements are cut into chunks of ML_OPT_CHUNK, a block
 *             finds its chunk's tensor by a search over `first_chunk` and grid-strides over the chunks.  16-byte accesses
 *             where p, g, m, v of a tensor are all 16-byte aligned, scalar ones otherwise and for the last n mod 4 elements.
 *             Every element is read and written by one lane; n = 0 is legal.  The kernel clamps every chunk to its tensor's
 *             n, so a wrong `total_chunks` skips or repeats nothing out of bounds.
 * ------------------------------------------------------------------------------------------- */
enum { ML_OPT_RADAM = 0, ML_OPT_ADAMW = 1 };
#define ML_OPT_CHUNK 4096
typedef struct ml_opt_tensor {
    float *p;                      /* the weights, updated in place                                 */
    const float *g;                /* their gradient                                                */
    float *m, *v;                  /* first and second moment, updated in place                     */
    int64_t n;                     /* floats in each of the four                                    */
    int64_t first_chunk;           /* chunks of the tensors in front (ml_optimizer_plan fills it)   */
} ml_opt_tensor;
typedef struct ml_opt_state {
    int64_t iterations;            /* steps taken                                                   */
    float lr;                      /* the learning rate the next step reads                         */
    int32_t reserved;
} ml_opt_state;
typedef struct ml_opt_scalars {
    float beta_1, one_minus_beta_1, beta_2, one_minus_beta_2, epsilon;
    float lr;                      /* lr' (after `decay`)                                           */
    float step, wd_lr;             /* RectifiedAdam (0 for AdamW)                                   */
    float lr_t, eta_wd;            /* AdamW (0 for RectifiedAdam)                                   */
    int32_t rectified;             /* RectifiedAdam: N > 5; AdamW: 1                                */
    int32_t decays;                /* weight_decay != 0                                             */
} ml_opt_scalars;
/* Host.  Fills first_chunk of the n entries of a table in HOST memory -> the number of chunks, or ML_E_BADARG for a null
 * pointer with n > 0 elements or a negative count.                                                                       */
int64_t ml_optimizer_plan(ml_opt_tensor *host_table, int32_t n);
/* state, scalars: device memory.  kind = ML_OPT_*; init_lr is read by AdamW only.                                       */
int ml_optimizer_scalars(int32_t kind, ml_opt_state *state, ml_opt_scalars *scalars, double beta_1, double beta_2, double epsilon,
                         double decay, double weight_decay, double init_lr, void *stream);
/* table [n] and scalars: device memory; total_chunks as ml_optimizer_plan returned it for this table.                   */
int ml_optimizer_apply_f32(int32_t kind, const ml_opt_tensor *table, int32_t n, int64_t total_chunks, const ml_opt_scalars *scalars,
                           void *stream);

/* ---------------------------------------------------------------------------------------------
 * Re-pack: master weights on the device in the Keras layout -> every packed form the kernels read, written in place into
 * the tensors that already hold them (csrc/repack.hip).  What a training step runs after the optimizer: the addresses stay,
 * so a captured graph replays with the new weights.  One launch on `stream` for every job of the device table, no
 * workspace, no atomics, no host read.  Every element of every destination is written exactly once, pads and zero blocks
 * included: the result does not depend on what the memory held.
 * A job is one master seen as element (tap, c, n) = src[tap s_tap + c s_c + n s_n] (strides in floats), N outputs, C input
 * channels, KH x KW taps:
 *   Conv2D kernel[kh,kw,cin,cout]            N = cout, C = cin, s_n = 1, s_c = cout, s_tap = cin cout; a cin slice of a
 *                                            1x1 kernel moves src by c0 cout and takes C = the slice's width
 *   Conv2DTranspose kernel[2,2,cout,cin]     N = 4 cout (column (a 2 + b) cout + o), C = cin, s_n = cin, s_c = 1, one tap;
 *                                            bias_n = cout; bias_reps = 4 for the bias of the same GEMM run as a 1x1 conv
 * and up to nine destinations, each optional, each the bits of the host function that defines it (masklab_hip/packing.py,
 * ops.DeviceConv):
 *   fwd_wgt     pack_dense: [fwd_n_pad][taps][fwd_span_pad], zero padded
 *   fwd_x3      the same, every 32-float chunk as 32 halves hi(w) then 32 halves 2^11 (w - hi(w)), round to nearest even
 *   fwd_h       [fwd_n_pad][taps][fwd_span_pad_h] halves
 *   fwd_wino    pack_winograd: U = G g G^T in fp64 rounded once, [max(4, fwd_n_pad / 32)][fwd_span_pad / 8][8][32][16]
 *               (3x3 only; each sum starts at +0.0 as the host's does, so the bits are the host's wherever the fp64 sums
 *               are exact, and differ at most by the order of the additions elsewhere; terms with a zero coefficient of
 *               G are left out, so an Inf / NaN weight spoils only the positions it has a coefficient in, where the
 *               host's 0 * Inf spoils all sixteen)
 *   bias        [bias_reps][bias_n] copies of src_bias [bias_n]
 *   tr_*        the four forms of pack_dense_transposed (the data gradient's weights): element (tap, c, n) at row c, tap
 *               taps - 1 - tap, channel n; tr_n_pad >= C rows, tr_span_pad >= N rounded up to 4
 * or, kind = ML_REPACK_TABLE, pack_out1x1_table of a 1x1 kernel [1,1,C,N]: `table` [C / 32][16][2][cp] and `table_bias` [cp]
 * (zeros where src_bias is NULL), cp = the power of two >= N.
 * Work units: a conv job is cut into [32 n][32 c][taps] tiles over the largest padded extent any of its forms has, nb x cb
 * of them, plus one unit for a bias; a table job is one unit.  A tile is read once and feeds every form of the job.
 * ------------------------------------------------------------------------------------------- */
enum { ML_REPACK_CONV = 0, ML_REPACK_TABLE = 1 };
typedef struct ml_repack_job {
    const float *src;              /* the master's element (0, 0, 0)                                 */
    const float *src_bias;         /* [bias_n] or NULL                                                   */
    int64_t s_n, s_c, s_tap;       /* strides in floats                                              */
    int32_t kind;                  /* ML_REPACK_*                                                    */
    int32_t N, C, KH, KW;
    int32_t cpp_shift;             /* of the packing: 30, a row-span (image) packing is refused      */
    int32_t group_cin_step;        /* of the packing: 0, a grouped packing is refused                */
    int32_t bias_reps;
    float *fwd_wgt, *fwd_x3;
    void *fwd_h;
    float *fwd_wino;
    float *bias;
    float *tr_wgt, *tr_x3;
    void *tr_h;
    float *tr_wino;
    float *table, *table_bias;
    int32_t fwd_n_pad, fwd_span_pad, fwd_span_pad_h;
    int32_t tr_n_pad, tr_span_pad, tr_span_pad_h;
    int32_t cp;
    int32_t nb, cb;                /* tiles along n and c (ml_repack_plan fills them)                */
    int32_t bias_n;                /* floats of src_bias (conv jobs; a table job's bias has N)       */
    int64_t first_unit;            /* units of the jobs in front (ml_repack_plan fills it)           */
} ml_repack_job;
/* Host.  Validates the n jobs of a table in HOST memory and fills nb, cb, first_unit -> the number of work units, or
 * ML_E_BADARG, each refusal by name: a destination that overlaps a master or another destination (masters may share
 * memory), a row-span or grouped packing, more than 5 x 5 taps, a Winograd form of a kernel that is not 3x3, extents that
 * do not hold the kernel.                                                                                               */
int64_t ml_repack_plan(ml_repack_job *host_table, int32_t n);
/* table [n]: device memory; total_units as ml_repack_plan returned it for this table.                                    */
int ml_repack_f32(const ml_repack_job *table, int32_t n, int64_t total_units, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MASKLAB_HIP_H */
