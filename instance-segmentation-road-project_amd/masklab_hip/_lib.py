"""ctypes binding of libmasklab_hip.so (the C ABI declared in include/masklab_hip.h).

Hand-written and checked: tests/test_abi_cpu.py parses the header and holds every row of SIGNATURES, every mirror of
STRUCTS and every upper-case integer below (`X` here is `ML_X` there) to it, type by type.

The product path has NO CPU fallback: if the shared library is missing or a kernel
call fails, a RuntimeError is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# The ONE library the product path loads: the in-tree build.  No environment override -- an experiment that wants another
# build assigns `_lib.LIB_PATH` in its own script before the first load() (scripts/h256_ab.py); bench.py prints the
# resolved path into its JSON line.
LIB_PATH = os.path.join(_HERE, "libmasklab_hip.so")

ABI_VERSION = 7
ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SIGMOID = 0, 1, 2, 3
MATH_F32, MATH_F16, MATH_F16S, MATH_F32X3 = 0, 1, 2, 3
ACT_BY_NAME = {None: ACT_NONE, "linear": ACT_NONE, "relu": ACT_RELU, "relu6": ACT_RELU6,
               "sigmoid": ACT_SIGMOID}


class ConvDesc(C.Structure):
    """Mirror of `ml_conv2d_desc` (include/masklab_hip.h)."""
    _fields_ = [
        ("in_", C.c_void_p), ("wgt", C.c_void_p), ("bias", C.c_void_p),
        ("residual", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("in_cstride", C.c_int32), ("in_coff", C.c_int32),
        ("span", C.c_int32), ("span_pad", C.c_int32), ("cpp_shift", C.c_int32),
        ("Ho", C.c_int32), ("Wo", C.c_int32),
        ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("dil", C.c_int32),
        ("pad_t", C.c_int32), ("pad_l", C.c_int32),
        ("cout", C.c_int32), ("n_pad", C.c_int32),
        ("out_cstride", C.c_int32), ("out_coff", C.c_int32),
        ("res_cstride", C.c_int32), ("res_coff", C.c_int32),
        ("act", C.c_int32), ("group_cin_step", C.c_int32), ("shuffle2x2", C.c_int32),
        ("tile", C.c_int32), ("math", C.c_int32), ("out_f16", C.c_int32),
        ("out_bstride", C.c_int64),
        ("live", C.c_void_p), ("live_period", C.c_int32), ("reserved1", C.c_int32),
        ("gn_partials", C.c_void_p),
    ]


class ConvWgradDesc(C.Structure):
    """Mirror of `ml_conv2d_wgrad_desc` (include/masklab_hip.h)."""
    _fields_ = [("conv", ConvDesc), ("dkernel", C.c_void_p), ("dbias", C.c_void_p), ("add_kernel", C.c_void_p),
                ("add_bias", C.c_void_p)]


class DwGradDesc(C.Structure):
    """Mirror of `ml_dwconv3x3_grad_desc` (include/masklab_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("dy", C.c_void_p), ("wgt", C.c_void_p), ("dkernel", C.c_void_p), ("dbias", C.c_void_p),
                ("add_kernel", C.c_void_p), ("add_bias", C.c_void_p), ("dx", C.c_void_p), ("add_x", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("in_cstride", C.c_int32),
                ("in_coff", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("dy_cstride", C.c_int32),
                ("dy_coff", C.c_int32), ("stride", C.c_int32), ("dil", C.c_int32), ("pad_t", C.c_int32), ("pad_l", C.c_int32)]


class GnDesc(C.Structure):
    """Mirror of `ml_gn_desc` (include/masklab_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("HWC", C.c_int64), ("N", C.c_int32), ("C", C.c_int32), ("G", C.c_int32), ("relu", C.c_int32),
                ("out_cstride", C.c_int32), ("out_coff", C.c_int32), ("eps", C.c_float), ("dtype", C.c_int32),
                ("live", C.c_void_p), ("live_period", C.c_int32), ("reserved", C.c_int32),
                ("partials", C.c_void_p), ("n_partials", C.c_int32), ("reserved2", C.c_int32)]


class GnGradDesc(C.Structure):
    """Mirror of `ml_gn_grad_desc` (include/masklab_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("dy", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("dx", C.c_void_p),
                ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("stats", C.c_void_p), ("HWC", C.c_int64),
                ("N", C.c_int32), ("C", C.c_int32), ("G", C.c_int32), ("relu", C.c_int32), ("input_relu", C.c_int32),
                ("eps", C.c_float)]


class RoiGradLevel(C.Structure):
    """Mirror of `ml_roi_grad_level` (include/masklab_hip.h)."""
    _fields_ = [("dy", C.c_void_p), ("add", C.c_void_p), ("dx", C.c_void_p), ("Hf", C.c_int32), ("Wf", C.c_int32),
                ("n_l", C.c_int32), ("reserved", C.c_int32)]


class DeconvOutProblem(C.Structure):
    """Mirror of `ml_deconv_out_problem` (include/masklab_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("wd", C.c_void_p), ("bd", C.c_void_p), ("wo_table", C.c_void_p),
                ("bo", C.c_void_p), ("out", C.c_void_p), ("M", C.c_int64), ("hw", C.c_int32), ("w", C.c_int32),
                ("rois_per_image", C.c_int32), ("reserved0", C.c_int32), ("out_image_stride", C.c_int64),
                ("out_base", C.c_int64), ("live", C.c_void_p)]


class DeconvOutGradProblem(C.Structure):
    """Mirror of `ml_deconv_out_grad_problem` (include/masklab_hip.h)."""
    _fields_ = [("dy", C.c_void_p), ("t", C.c_void_p), ("wo", C.c_void_p), ("out", C.c_void_p), ("dkernel", C.c_void_p),
                ("dbias", C.c_void_p), ("M", C.c_int64), ("hw", C.c_int32), ("w", C.c_int32), ("rois_per_image", C.c_int32),
                ("c_mid", C.c_int32), ("dy_image_stride", C.c_int64), ("dy_base", C.c_int64)]


class SeDesc(C.Structure):
    """Mirror of `ml_se_desc` (include/masklab_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("w1", C.c_void_p), ("w2", C.c_void_p),
                ("B", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32), ("Hd", C.c_int32),
                ("live", C.c_void_p), ("live_period", C.c_int32), ("reserved", C.c_int32), ("ws_offset", C.c_int64)]


class SeResidualDesc(C.Structure):
    """Mirror of `ml_se_residual_desc` (include/masklab_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("shortcut", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p),
                ("w2", C.c_void_p), ("b2", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
                ("out_act", C.c_void_p), ("out_y", C.c_void_p),
                ("B", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32), ("Hd", C.c_int32),
                ("mode", C.c_int32), ("reserved", C.c_int32)]


class SeBottleneckDesc(C.Structure):
    """Mirror of `ml_se_bottleneck_desc` (include/masklab_hip.h)."""
    _fields_ = [("c3", C.c_void_p), ("residual", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p),
                ("w2", C.c_void_p), ("b2", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32), ("Hd", C.c_int32)]


class OptTensor(C.Structure):
    """Mirror of `ml_opt_tensor` (include/masklab_hip.h)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64),
                ("first_chunk", C.c_int64)]


class OptState(C.Structure):
    """Mirror of `ml_opt_state` (include/masklab_hip.h)."""
    _fields_ = [("iterations", C.c_int64), ("lr", C.c_float), ("reserved", C.c_int32)]


class OptScalars(C.Structure):
    """Mirror of `ml_opt_scalars` (include/masklab_hip.h)."""
    _fields_ = [("beta_1", C.c_float), ("one_minus_beta_1", C.c_float), ("beta_2", C.c_float), ("one_minus_beta_2", C.c_float),
                ("epsilon", C.c_float), ("lr", C.c_float), ("step", C.c_float), ("wd_lr", C.c_float), ("lr_t", C.c_float),
                ("eta_wd", C.c_float), ("rectified", C.c_int32), ("decays", C.c_int32)]


class RepackJob(C.Structure):
    """Mirror of `ml_repack_job` (include/masklab_hip.h)."""
    _fields_ = [("src", C.c_void_p), ("src_bias", C.c_void_p), ("s_n", C.c_int64), ("s_c", C.c_int64), ("s_tap", C.c_int64),
                ("kind", C.c_int32), ("N", C.c_int32), ("C", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32),
                ("cpp_shift", C.c_int32), ("group_cin_step", C.c_int32), ("bias_reps", C.c_int32),
                ("fwd_wgt", C.c_void_p), ("fwd_x3", C.c_void_p), ("fwd_h", C.c_void_p), ("fwd_wino", C.c_void_p),
                ("bias", C.c_void_p), ("tr_wgt", C.c_void_p), ("tr_x3", C.c_void_p), ("tr_h", C.c_void_p),
                ("tr_wino", C.c_void_p), ("table", C.c_void_p), ("table_bias", C.c_void_p),
                ("fwd_n_pad", C.c_int32), ("fwd_span_pad", C.c_int32), ("fwd_span_pad_h", C.c_int32),
                ("tr_n_pad", C.c_int32), ("tr_span_pad", C.c_int32), ("tr_span_pad_h", C.c_int32),
                ("cp", C.c_int32), ("nb", C.c_int32), ("cb", C.c_int32), ("bias_n", C.c_int32), ("first_unit", C.c_int64)]


# C struct -> its mirror; every struct of the header
STRUCTS = {
    "ml_conv2d_desc": ConvDesc, "ml_conv2d_wgrad_desc": ConvWgradDesc, "ml_dwconv3x3_grad_desc": DwGradDesc,
    "ml_gn_desc": GnDesc, "ml_gn_grad_desc": GnGradDesc, "ml_roi_grad_level": RoiGradLevel,
    "ml_deconv_out_problem": DeconvOutProblem, "ml_deconv_out_grad_problem": DeconvOutGradProblem,
    "ml_se_desc": SeDesc, "ml_se_residual_desc": SeResidualDesc, "ml_se_bottleneck_desc": SeBottleneckDesc,
    "ml_opt_tensor": OptTensor, "ml_opt_state": OptState, "ml_opt_scalars": OptScalars, "ml_repack_job": RepackJob,
}

SE_RES_GATE, SE_RES_BN_RELU = 0, 1
CONV_MAX_PROBLEMS = 12
GN_MAX_PROBLEMS = 8
CONV_WGRAD_MAX_PROBLEMS = 8
CONV_DGRAD_S2_MAX_TAPS = 25
DWCONV_GRAD_MAX_PROBLEMS = 8
SE_MAX_PROBLEMS = 8
RESAMPLE_MAX_LEVELS = 8
DECONV_OUT_MAX_PROBLEMS = 4
_i32, _i64, _f32, _f64, _vp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p

# name -> (restype, argtypes); every prototype of the header
SIGNATURES = {
    "ml_version": (C.c_int, []),
    "ml_last_error": (C.c_char_p, []),
    "ml_device_check": (C.c_int, []),
    "ml_conv2d_f32": (C.c_int, [C.POINTER(ConvDesc), _vp]),
    "ml_conv2d_ntile": (C.c_int, [_i32, _i32]),
    "ml_conv2d_uses_pipe": (C.c_int, [C.POINTER(ConvDesc)]),
    "ml_conv2d_launch_ntile": (C.c_int, [C.POINTER(ConvDesc), _i32, _i32]),
    "ml_conv2d_launch_mtile": (C.c_int, [C.POINTER(ConvDesc), _i32, _i32]),
    "ml_conv2d_launch_splits": (C.c_int, [C.POINTER(ConvDesc), _i32, _i64, C.POINTER(C.c_int32)]),
    "ml_conv2d_wino_eligible": (C.c_int, [C.POINTER(ConvDesc)]),
    "ml_conv2d_wino_narrow": (C.c_int, [C.POINTER(ConvDesc)]),
    "ml_conv2d_gn_min_launch_tiles": (_i64, []),
    "ml_conv2d_workspace_bytes": (_i64, []),
    "ml_conv2d_multi_f32": (C.c_int, [C.POINTER(ConvDesc), _i32, _vp, _i64, _vp]),
    "ml_conv2d_wgrad_multi_f32": (C.c_int, [C.POINTER(ConvWgradDesc), _i32, _vp, _i64, _vp]),
    "ml_conv2d_wgrad_plan": (C.c_int, [C.POINTER(ConvWgradDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "ml_conv2d_grad_gather_dy_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i64, _vp]),
    "ml_conv2d_dgrad_s2_f32": (C.c_int, [C.POINTER(ConvDesc), _vp, _vp, _vp]),
    "ml_conv2d_dgrad_s2_classes": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ml_dwconv3x3_wgrad_multi_f32": (C.c_int, [C.POINTER(DwGradDesc), _i32, _vp, _i64, _vp]),
    "ml_dwconv3x3_wgrad_plan": (C.c_int, [C.POINTER(DwGradDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "ml_dwconv3x3_dgrad_multi_f32": (C.c_int, [C.POINTER(DwGradDesc), _i32, _vp]),
    "ml_relu_grad_f32": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "ml_deconv2x2_out1x1_f32": (C.c_int, [C.POINTER(DeconvOutProblem), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ml_deconv2x2_out1x1_tape_f32": (C.c_int, [C.POINTER(DeconvOutProblem), C.POINTER(C.c_void_p)] + [_i32] * 7 + [_vp]),
    "ml_deconv2x2_out1x1_grad_f32": (C.c_int, [C.POINTER(DeconvOutGradProblem), _i32, _i32, _vp, _i64, _vp]),
    "ml_deconv2x2_out1x1_grad_plan": (C.c_int, [C.POINTER(DeconvOutGradProblem), _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                C.POINTER(C.c_int64)]),
    "ml_deconv2x2_grad_relayout_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "ml_gconv3x3_f32": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 11 + [_vp]),
    "ml_gconv3x3_f16": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 11 + [_vp]),
    "ml_gconv3x3_launch_plan": (C.c_int, [_i32] * 9 + [C.POINTER(C.c_int32)]),
    "ml_maxpool3x3s2_f16": (C.c_int, [_vp, _vp] + [_i32] * 8 + [_vp]),
    "ml_stem7x7s2_pool_f16": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 5 + [_vp]),
    "ml_stem7x7s2_pool_f32": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 5 + [_vp]),
    "ml_stem7x7s2_pool_x3": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 5 + [_vp]),
    "ml_subsample2_f16": (C.c_int, [_vp, _vp] + [_i32] * 4 + [_vp]),
    "ml_cast_f16_to_f32": (C.c_int, [_vp, _vp, _i64, _vp]),
    "ml_cast_f32_to_f16": (C.c_int, [_vp, _vp, _i64, _vp]),
    "ml_resize_bilinear_ac_f16": (C.c_int, [_vp, _vp, _vp] + [_i32] * 12 + [_vp]),
    "ml_dwconv3x3_f16": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 15 + [_vp]),
    "ml_global_mean_f16": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "ml_groupnorm_chunk_f16": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _i32, _i32, _i32, _vp, _vp]),
    "ml_roi_crop_resize_f16": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp] + [_i32] * 10 + [_f32, _f32, _i32, _i32, _vp, _vp]),
    "ml_deconv2x2_out1x1_f16": (C.c_int, [C.POINTER(DeconvOutProblem), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ml_dwconv3x3_f32": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 15 + [_vp]),
    "ml_maxpool3x3s2_f32": (C.c_int, [_vp, _vp] + [_i32] * 8 + [_vp]),
    "ml_preprocess_f32": (C.c_int, [_vp, _i32, _vp, _i64, _i32, _i32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), _vp]),
    "ml_groupnorm_workspace_bytes": (_i64, [_i32, _i32]),
    "ml_groupnorm_multi_f32": (C.c_int, [C.POINTER(GnDesc), _i32, _vp, _i64, _vp]),
    "ml_groupnorm_chunk_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _i32, _i32, _i32, _vp, _vp]),
    "ml_groupnorm_grad_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "ml_groupnorm_chunk_grad_f32": (C.c_int, [_vp] * 8 + [_i32, _i64, _i32, _i32, _f32, _i32, _i32, _vp, _vp]),
    "ml_groupnorm_chunk_stats_f32": (C.c_int, [_vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp]),
    "ml_groupnorm_grad_multi_f32": (C.c_int, [C.POINTER(GnGradDesc), _i32, _vp, _i64, _vp]),
    "ml_batchnorm_workspace_bytes": (_i64, [_i64, _i32]),
    "ml_batchnorm_plan": (C.c_int, [_i64, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ml_batchnorm_train_f32": (C.c_int, [_vp] * 10 + [_i64, _i32, _f32, _f64, _i32, _vp, _i64, _vp]),
    "ml_batchnorm_infer_f32": (C.c_int, [_vp] * 7 + [_i64, _i32, _f32, _i32, _vp, _i64, _vp]),
    "ml_batchnorm_grad_f32": (C.c_int, [_vp] * 9 + [_i64, _i32, _i32, _vp, _i64, _vp]),
    "ml_resize_bilinear_ac_f32": (C.c_int, [_vp, _vp, _vp] + [_i32] * 12 + [_vp]),
    "ml_resize_bilinear_ac_grad_workspace_bytes": (_i64, [_i32] * 6),
    "ml_resize_bilinear_ac_grad_f32": (C.c_int, [_vp, _vp, _vp] + [_i32] * 8 + [_vp, _i64, _vp]),
    "ml_global_mean_grad_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "ml_global_mean_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "ml_scale_channels_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "ml_squeeze_excite_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "ml_squeeze_excite_f32": (C.c_int, [C.POINTER(SeDesc), _i32, _vp, _i64, _vp]),
    "ml_squeeze_excite_f16": (C.c_int, [C.POINTER(SeDesc), _i32, _vp, _i64, _vp]),
    "ml_se_residual_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "ml_se_residual_f32": (C.c_int, [C.POINTER(SeResidualDesc), _vp, _i64, _vp]),
    "ml_se_bottleneck_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "ml_se_bottleneck_f32": (C.c_int, [C.POINTER(SeBottleneckDesc), _vp, _i64, _vp]),
    "ml_se_bottleneck_f16": (C.c_int, [C.POINTER(SeBottleneckDesc), _vp, _i64, _vp]),
    "ml_conv1x1_dual_f32": (C.c_int, [_vp] * 5 + [_i32] * 7 + [_vp]),
    "ml_conv1x1_dual_f16": (C.c_int, [_vp] * 5 + [_i32] * 7 + [_vp]),
    "ml_restore_boxes_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "ml_detection_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "ml_detection_proposal_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _f32, _i32, _vp, _vp]),
    "ml_mask_distribute_i32": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "ml_roi_crop_resize_f32": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp] + [_i32] * 10 + [_f32, _f32, _i32, _i32, _vp, _vp]),
    "ml_roi_crop_resize_grad_f32": (C.c_int, [C.POINTER(RoiGradLevel), _i32, _vp, _i32, _i32, _vp, _vp] + [_i32] * 6 +
                                    [_f32, _f32, _vp]),
    "ml_mold_levels_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, C.POINTER(C.c_int32), _vp]),
    "ml_mold_levels_dev_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp]),
    "ml_add_f32": (C.c_int, [_vp, _vp, _i64, _vp]),
    "ml_add_f16": (C.c_int, [_vp, _vp, _i64, _vp]),
    "ml_fill_f32": (C.c_int, [_vp, _f32, _i64, _vp]),
    "ml_resize_image_ac": (C.c_int, [_vp, _i32, _vp, _vp, _f32] + [_i32] * 6 + [_vp]),
    "ml_trim_instances_f32": (C.c_int, [_vp] * 5 + [_i32] * 5 + [_vp]),
    "ml_upsample_boxes_i32": (C.c_int, [_vp, _vp, _i64, _f32, _f32, _vp]),
    "ml_threshold_i32": (C.c_int, [_vp, _vp, _f32, _i64, _vp]),
    "ml_semantic_smoothing_f32": (C.c_int, [_vp, _vp, _vp] + [_i32] * 4 + [_vp, _vp, _vp]),
    "ml_crop_pad_mask_f32": (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 6 + [_vp]),
    "ml_nonzero_bbox_i32": (C.c_int, [_vp] + [_i32] * 5 + [_vp, _vp]),
    "ml_instance_summary_workspace_bytes": (_i64, [_i32, _i32]),
    "ml_instance_summary_f32": (C.c_int, [_vp, _i32, _i32, _vp, _vp] + [_i32] * 4 + [_f32, _f32, _vp, _vp]),
    "ml_instance_summary_rois_f32": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp] + [_i32] * 6 + [_f32, _f32, _vp, _vp]),
    "ml_draw_boxes_u8": (C.c_int, [_vp, _vp, _vp] + [_i32] * 4 + [_vp]),
    "ml_draw_instance_u8": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _f32] + [_i32] * 4 + [_vp]),
    "ml_draw_segmentation_u8": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _f32] + [_i32] * 3 + [_vp]),
    "ml_serving_visualize_u8": (C.c_int, [_vp] * 7 + [_i32, _f32, _vp, _i32, _f32] + [_i32] * 6 + [_vp]),
    "ml_jpeg_encode_capacity": (_i64, [_i32, _i32]),
    "ml_jpeg_encode_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "ml_jpeg_encode_u8": (C.c_int, [_vp] + [_i32] * 4 + [_vp, _i64, _vp, _vp, _vp]),
    "ml_jpeg_decode_info": (C.c_int, [_vp, _i64, _vp]),
    "ml_jpeg_decode_packed_bytes": (_i64, [_vp, _i64]),
    "ml_jpeg_decode_entropy": (_i64, [_vp, _i64, _vp, _i64]),
    "ml_jpeg_decode_workspace_bytes": (_i64, [_i32] * 4),
    "ml_jpeg_decode_u8": (C.c_int, [_vp, _vp] + [_i32] * 4 + [_vp, _vp, _vp]),
    "ml_jpeg_decode_reference_host": (C.c_int, [_vp, _vp] + [_i32] * 4 + [_vp, _vp]),
    "ml_jpeg_entropy_geometry": (C.c_int, [_vp]),
    "ml_jpeg_entropy_plan_bytes": (_i64, []),
    "ml_jpeg_entropy_plan": (C.c_int, [_vp, _i64, _vp]),
    "ml_jpeg_entropy_workspace_bytes": (_i64, [_vp, _i32]),
    "ml_jpeg_entropy_device": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ml_jpeg_entropy_reference_host": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "ml_eval_mask_area": (C.c_int, [_vp] + [_i32] * 4 + [_vp, _vp]),
    "ml_eval_mask_pairs": (C.c_int, [_vp] * 5 + [_i32] * 8 + [_vp, _vp]),
    "ml_eval_semantic_counts": (C.c_int, [_vp, _vp] + [_i32] * 4 + [_vp, _vp]),
    "ml_eval_class_binary_iou": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i64, _i32, _f32, _vp, _vp, _vp]),
    "ml_eval_detection_metric_f32": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ml_eval_confusion_f32": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _f32, _vp, _vp, _vp]),
    "ml_eval_reference_host": (C.c_int, [_vp] * 4 + [_i32, _vp, _vp] + [_i32] * 8 + [_vp] * 3),
    "ml_train_workspace_bytes": (_i64, [_i32, _i32]),
    "ml_train_calculate_iou_f32": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "ml_train_best_prior_f32": (C.c_int, [_vp, _vp] + [_i32] * 3 + [_vp, _vp, _vp]),
    "ml_train_assign_boxes_f32": (C.c_int, [_vp, _vp, _vp] + [_i32] * 4 + [_vp] * 4),
    "ml_train_class_loss_f32": (C.c_int, [_vp] * 4 + [_i32] * 3 + [_f32] * 3 + [_vp] * 3),
    "ml_train_box_loss_f32": (C.c_int, [_vp] * 3 + [_i32] * 2 + [_f32] * 4 + [_i32] + [_vp] * 4),
    "ml_train_assign_masks": (C.c_int, [_vp] * 3 + [_i32] * 9 + [_f32, _vp, _vp]),
    "ml_train_mask_loss_f32": (C.c_int, [_vp, _vp] + [_i32] * 5 + [_f32] * 3 + [_vp] * 3),
    "ml_train_assign_seg": (C.c_int, [_vp] + [_i32] * 7 + [_vp, _vp]),
    "ml_train_seg_loss_f32": (C.c_int, [_vp] * 3 + [_i32, _i64, _i32] + [_f32] * 3 + [_vp] * 3),
    "ml_train_class_loss_grad_f32": (C.c_int, [_vp] * 4 + [_i32] * 3 + [_f32] * 3 + [_vp] * 3 + [_i32, _vp, _vp]),
    "ml_train_box_loss_grad_f32": (C.c_int, [_vp] * 3 + [_i32] * 2 + [_f32] * 4 + [_i32] + [_vp] * 6),
    "ml_train_mask_loss_grad_f32": (C.c_int, [_vp, _vp] + [_i32] * 5 + [_f32] * 3 + [_vp] * 3 + [_i32, _vp, _vp]),
    "ml_train_seg_loss_grad_f32": (C.c_int, [_vp] * 3 + [_i32, _i64, _i32] + [_f32] * 3 + [_vp] * 3 + [_i32, _vp, _vp]),
    "ml_cv_resize_linear_u8": (C.c_int, [_vp, _vp, _i64] + [_i32] * 6 + [_vp]),
    "ml_cv_resize_linear_round_u8": (C.c_int, [_vp, _vp, _i32, _i64] + [_i32] * 5 + [_vp]),
    "ml_cv_resize_reference_host": (C.c_int, [_vp, _vp, _i32, _i64] + [_i32] * 6),
    "ml_polygon_instance_masks": (C.c_int, [_vp, _i64, _vp, _vp] + [_i32] * 4 + [_vp, _vp]),
    "ml_polygon_semantic_maps": (C.c_int, [_vp, _i64, _vp, _i32, _vp] + [_i32] * 4 + [_vp, _vp]),
    "ml_polygon_reference_host": (C.c_int, [_i32, _vp, _i64, _vp, _i32, _vp, _vp] + [_i32] * 4 + [_vp]),
    "ml_optimizer_plan": (_i64, [C.POINTER(OptTensor), _i32]),
    "ml_optimizer_scalars": (C.c_int, [_i32, C.POINTER(OptState), C.POINTER(OptScalars)] + [_f64] * 6 + [_vp]),
    "ml_optimizer_apply_f32": (C.c_int, [_i32, C.POINTER(OptTensor), _i32, _i64, C.POINTER(OptScalars), _vp]),
    "ml_repack_plan": (_i64, [C.POINTER(RepackJob), _i32]),
    "ml_repack_f32": (C.c_int, [C.POINTER(RepackJob), _i32, _i64, _vp]),
}
REPACK_CONV, REPACK_TABLE = 0, 1
OPT_RADAM, OPT_ADAMW = 0, 1
OPT_CHUNK = 4096
POLYGON_INSTANCE, POLYGON_SEMANTIC = 0, 1
CV_RESIZE_U8, CV_RESIZE_ROUND_U8, CV_RESIZE_ROUND_F32 = 0, 1, 2
TRAIN_MASK_I8, TRAIN_MASK_U8 = 0, 1
TRAIN_MAX_BLOCKS = 512
EVAL_F32, EVAL_F16, EVAL_I32, EVAL_U8 = 0, 1, 2, 3
EVAL_MAX_CLASSES = 16
JPEG_GRAY, JPEG_444, JPEG_420 = 0, 1, 2
JPEG_UNSUPPORTED = 1
JPEG_DECODE_MAX_BATCH = 32
JPEG_ENTROPY_OK, JPEG_ENTROPY_ASK_HOST, JPEG_ENTROPY_NOT_SYNCED = 0, 10, 11
DRAW_MAX_CLASSES = 16

_lib = None


def load():
    """Load the shared library (once) and bind every declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"masklab_hip: {LIB_PATH} is missing -- build it with "
            f"`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            f"There is no CPU fallback for the product path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.ml_version() != ABI_VERSION:       # e.g. a stale .so from before ml_conv2d_desc changed layout
        raise RuntimeError(f"masklab_hip: {LIB_PATH} has ABI version {lib.ml_version()}, this package binds "
                           f"version {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().ml_last_error()
        raise RuntimeError(f"masklab_hip: {what} failed with status {status}: "
                           f"{msg.decode() if msg else '?'}")
