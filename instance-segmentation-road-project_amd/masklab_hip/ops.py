"""Operator launchers: torch tensors (device memory + streams only) -> libmasklab_hip.so.

Every function enqueues HIP kernels on torch's CURRENT stream and returns the output tensor.
Tensors are NHWC float32, contiguous.  A `(buffer, channel_offset)` pair addresses a channel
slice of a wider buffer so concat / add are fused into the producing kernel.
There is no torch compute and no CPU fallback here.
"""
import ctypes as C
import dataclasses
import threading

import numpy as np
import torch

from . import _lib
from .packing import (NO_PIX_SPAN, PackedConv, dgrad_padding, pack_dense_transposed, pack_winograd, resolve_padding,
                      transposed_geometry, unpack_dense)

import weakref

_ws_cache = {}
_ws_retired = []     # superseded scratch buffers stay allocated WHILE some model holds a captured hipGraph (which may
                     # replay with their addresses); released once the last graph owner has dropped its graphs
_graph_owners = weakref.WeakSet()


def graph_owner_registered(model):
    _graph_owners.add(model)


def graph_owner_released(model):
    """A model dropped its captured graphs: with no owner left nothing can replay with a retired buffer's address."""
    _graph_owners.discard(model)
    if not len(_graph_owners):
        _ws_retired.clear()

# When set to a list, every launcher appends {"kernel", "flops", "bytes", "start", "end"} with
# torch.cuda.Event pairs recorded on the launch stream (bench.py's roofline leg).  `bytes` /
# `flops` are ALGORITHMIC: inputs read once + outputs written once (+ weights once), 2*MACs.
PROFILE = None
# When set to a list, every dense-conv launch appends (shape label, K slices per problem) as the library reports them
# (ml_conv2d_launch_splits): tests use it to name the launches whose K sum is cut differently when the batch changes.
LAUNCH_LOG = None


class _Prof:
    def __init__(self, kernel, flops, nbytes, shape=""):
        self.on = PROFILE is not None
        if self.on:
            self.rec = {"kernel": kernel, "flops": float(flops), "bytes": float(nbytes), "shape": shape,
                        "start": torch.cuda.Event(enable_timing=True), "end": torch.cuda.Event(enable_timing=True)}

    def __enter__(self):
        if self.on:
            self.rec["start"].record()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.rec["end"].record()
            PROFILE.append(self.rec)
        return False


# Arithmetic of the dense (MFMA) convolutions: "f32" = exact fp32 products (the default; configs 1-4),
# "f16" = fp16 MFMA operands (rounded to fp16 on their way into LDS), fp32 accumulation, tensors stay fp32,
# "f16s" = the fp16 MFMA path of BASELINE config 5 with fp16 STORAGE: the ResNeXt body AND the heads keep activations
# and weights in IEEE half in HBM (the stem writes half; every conv, GroupNorm, resize, RoI crop reads and writes half;
# accumulation, statistics, bias and activation are fp32 with one rounding at the store); only what detect.hip reads
# and what the model returns -- cls_pred, loc_pred, roi_boxes, roi_masks, seg_pred -- is fp32.  Kernels follow the
# dtype of the tensor they are given: an fp32 tensor in this mode (MobileNet's body) runs like "f16".
# "f32x3" = fp32 tensors and fp32-grade arithmetic on the f16 matrix pipe (ML_MATH_F32X3): every operand is split into
# two halves (22 bits), every product is three f16 MFMAs with fp32 accumulation; 1x1 convs with K <= 256 (or a residual)
# on maps of >= 4 096 pixels run on the persistent pipelined kernel, every other conv on the generic one.
# Process-wide switch, read when a conv is launched; set it through set_conv_math().
CONV_MATH = "f32"
# per-launch code of fp32-tensor convs; half tensors select ML_MATH_F16S
_MATH_CODE = {"f32": _lib.MATH_F32, "f16": _lib.MATH_F16, "f16s": _lib.MATH_F16, "f32x3": _lib.MATH_F32X3}


def set_conv_math(mode):
    global CONV_MATH
    if mode not in _MATH_CODE:
        raise ValueError(f"conv math must be one of {sorted(_MATH_CODE)}, got {mode!r}")
    CONV_MATH = mode


def dtype_label():
    """The arithmetic type the dense-conv path computes in (bench.py's `dtype`)."""
    return {"f32": "f32", "f32x3": "f32 tensors, products as 3 x f16 MFMA on split operands (22-bit), f32 accumulate",
            "f16": "f16 MFMA operands, f32 accumulate, f32 tensors",
            "f16s": "f16 MFMA, f32 accumulate, f16 tensors in backbone body and heads (f32 predictions)"}[CONV_MATH]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _ptr_as(t, struct):
    """The address of tensor `t`, which holds `struct` records (a table or a state in device memory); None -> NULL."""
    return C.cast(t.data_ptr(), C.POINTER(struct)) if t is not None else None


def half_storage():
    """True in the "f16s" mode: backbone bodies keep their tensors in IEEE half."""
    return CONV_MATH == "f16s"


def _require_dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"masklab_hip: `{name}` must be a CUDA/HIP torch tensor -- the product path "
                           f"runs only on the MI355X kernels (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError(f"masklab_hip: `{name}` must be contiguous NHWC")


def workspace(nbytes, device, tag="ws"):
    """Grow-only scratch buffer per (device, tag, stream); 256-byte aligned by the torch allocator.
    Keyed by the launch stream too: work enqueued on two streams must not share scratch memory.  A buffer that is
    outgrown is retired, never freed (graphs captured earlier replay with its address)."""
    key = (str(device), tag, torch.cuda.current_stream().cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _ws_retired.append(buf)
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# Counts every event after which a layer's list of re-pack jobs may differ: a packing made, bound, or a lazy form materialised.
# Layer.repack() keeps its job list while this stands still, so that RepackTable's identity fast path applies to it.
_forms_epoch = [0]


def forms_epoch():
    return _forms_epoch[0]


class DeviceConv:
    """A PackedConv uploaded to the GPU."""

    def __init__(self, packed: PackedConv, device):
        self.p = packed
        self.wgt = torch.from_numpy(np.ascontiguousarray(packed.wgt)).to(device)
        self.bias = None if packed.bias is None else torch.from_numpy(packed.bias).to(device)
        self._init_forms()

    def _init_forms(self):
        _forms_epoch[0] += 1
        self._wgt_h = None
        self._wgt_x3 = None
        self._wgt_wino = None
        self._wgt_stem_h = None
        self._dgrad = None
        self._keras_kernel = None   # keras_kernel: the uploaded [kh,kw,cin,cout] copy of a packing that follows no master
        self._master = None         # bind_master: the device tensors this packing follows
        self._tr_of = None          # a data-gradient packing: the DeviceConv it is the `dgrad` of

    @property
    def dgrad(self):
        """The DeviceConv whose FORWARD is this dense conv's data gradient at stride 1 (packing.pack_dense_transposed: the
        kernel rotated by 180 degrees, cin / cout swapped, the new cin padded to a multiple of 4 with zero weights; no
        bias); made on first use -- on the device from the master once the packing follows one (bind_master; repack_jobs() then
        lists it), from the host weights otherwise."""
        if self._dgrad is None:
            if self._master is not None:
                self._dgrad = self._dgrad_from_master()
            else:
                self._dgrad = DeviceConv(pack_dense_transposed(unpack_dense(self.p)), self.wgt.device)
                self._dgrad._tr_of = self
        return self._dgrad

    @property
    def keras_kernel(self):
        """The dense conv's kernel in the Keras layout [kh,kw,cin,cout] on the device -- what the stride-2 data gradient reads
        (conv2d_dgrad_s2): the bound master itself where the packing follows one (a stepped kernel is seen at once: no packed
        form, no re-pack job), else a copy uploaded on first use from the host weights and kept (dropped by bind_master)."""
        m = self._master
        if m is not None:
            if m["offset"] or tuple(m["kernel"].shape) != (m["KH"], m["KW"], m["C"], m["N"]):
                raise NotImplementedError("DeviceConv.keras_kernel: the packing follows a cin slice or a transposed-conv master; "
                                          "the stride-2 data gradient reads a whole [kh,kw,cin,cout] kernel")
            return m["kernel"]
        if self._keras_kernel is None:
            self._keras_kernel = torch.from_numpy(unpack_dense(self.p)).to(self.wgt.device)
        return self._keras_kernel

    @property
    def wgt_wino(self):
        """The Winograd F(2x2,3x3) weights U = G g G^T (packing.pack_winograd: fp64, rounded once) of a dense 3x3 conv, four
        32-output blocks (a packing narrower than 128 rows is padded with zero blocks) -- what ml_conv2d_desc.tile = 6 reads
        with n_pad = 128; made on first use."""
        if self._wgt_wino is None:
            _forms_epoch[0] += 1
            self._wgt_wino = self._form_from_master("wino") if self.follows_master else \
                torch.from_numpy(pack_winograd(self.p)).to(self.wgt.device)
        return self._wgt_wino

    @property
    def wgt_x3(self):
        """The packed weights split for ML_MATH_F32X3 (include/masklab_hip.h): every 32-float chunk of a row becomes 32
        halves hi(w) followed by 32 halves 2^11 (w - hi(w)) -- same bytes, same strides; made on first use."""
        if self._wgt_x3 is None:
            _forms_epoch[0] += 1
        if self._wgt_x3 is None and self.follows_master:
            self._wgt_x3 = self._form_from_master("x3")
        if self._wgt_x3 is None:
            w = np.ascontiguousarray(self.p.wgt, dtype=np.float32)
            rows, ktot = w.shape
            if ktot % 32:
                raise RuntimeError("f32x3: the packed row length must be a multiple of 32 floats")
            c = w.reshape(rows, ktot // 32, 32)
            hi = c.astype(np.float16)
            lo = ((c - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
            both = np.ascontiguousarray(np.concatenate([hi, lo], axis=2))            # [rows, chunks, 64] halves
            self._wgt_x3 = torch.from_numpy(both.view(np.float32).reshape(rows, ktot)).to(self.wgt.device)
        return self._wgt_x3

    @property
    def wgt_stem_h(self):
        """The row-span stem packing rounded to IEEE half, same layout ([64][7 x 32]) -- what the fused fp16-storage stem
        (stem_pool in "f16s") reads; made on first use."""
        if self._wgt_stem_h is None:
            self._wgt_stem_h = torch.from_numpy(np.ascontiguousarray(self.p.wgt, np.float32).astype(np.float16)).to(self.wgt.device)
        return self._wgt_stem_h

    @property
    def span_pad_h(self):
        """K floats per tap of the half packing: the span rounded up to a 64-deep chunk (128 bytes per row)."""
        return -(-self.p.span // 64) * 64

    @property
    def wgt_h(self):
        """The packed weights rounded to IEEE half (fp16-storage convs), every tap padded to span_pad_h; made on first
        use."""
        if self._wgt_h is None:
            _forms_epoch[0] += 1
        if self._wgt_h is None and self.follows_master:
            self._wgt_h = self._form_from_master("h")
        if self._wgt_h is None:
            p = self.p
            if p.cpp_shift != 30 or p.group_cin_step:
                raise RuntimeError("fp16 storage: image (row-span) and grouped-window convs have no half packing")
            taps = p.KH * p.KW
            w = p.wgt.reshape(p.n_pad, taps, p.span_pad)[:, :, :p.span]
            wh = np.zeros((p.n_pad, taps, self.span_pad_h), np.float16)
            wh[:, :, :p.span] = w
            self._wgt_h = torch.from_numpy(np.ascontiguousarray(wh.reshape(p.n_pad, taps * self.span_pad_h))).to(self.wgt.device)
        return self._wgt_h


    # ---- a packing that follows master weights on the device (csrc/repack.hip; DESIGN 7a-train, "Re-pack")
    @property
    def follows_master(self):
        """True once bind_master() was called on this packing, or on the packing this one is the `dgrad` of."""
        return self._master is not None or (self._tr_of is not None and self._tr_of._master is not None)

    def bind_master(self, kernel, bias=None, layout="conv", cin_slice=None, bias_reps=1):
        """From now on this packing follows `kernel` (and `bias`), float32 tensors on the packing's device in the Keras
        layout: [kh,kw,cin,cout] for layout="conv" (cin_slice=(c0, c1): this packing is that cin slice of the kernel, packed
        as a conv of its own), [2,2,cout,cin] for layout="deconv" (pack_transpose2x2's GEMM; bias_reps=4 where the packing
        holds the bias tiled four times).  repack_jobs() then describes every form this packing has materialised, `dgrad` and
        its forms included, for ops.repack_weights; a form first asked for later is made on the device from the master.  The
        host copy of the weights (self.p.wgt / .bias) is dropped: after a step it would be stale, so nothing may read it
        (packing.unpack_dense raises).  Nothing is launched here: the forms hold what they held."""
        what, p = "DeviceConv.bind_master", self.p
        if self._tr_of is not None:
            raise ValueError(f"{what}: a data-gradient packing follows the master of the packing it belongs to; bind that one")
        if p.cpp_shift != NO_PIX_SPAN:
            raise NotImplementedError(f"{what}: a row-span (image_input) packing is not re-packed on the device")
        if p.group_cin_step:
            raise NotImplementedError(f"{what}: a grouped packing is not re-packed on the device")
        if layout not in ("conv", "deconv"):
            raise ValueError(f"{what}: layout must be 'conv' or 'deconv', got {layout!r}")
        for name, t in (("kernel", kernel), ("bias", bias)):
            if t is None and name == "bias":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError(f"{what}: `{name}` must be a contiguous float32 torch tensor")
            if t.device != self.wgt.device:
                raise RuntimeError(f"{what}: `{name}` is on {t.device}, the packing on {self.wgt.device}")
        if kernel.dim() != 4:
            raise ValueError(f"{what}: `kernel` must have four axes, got {tuple(kernel.shape)}")
        if layout == "conv":
            kh, kw, cin, cout = (int(v) for v in kernel.shape)
            c0, c1 = (0, cin) if cin_slice is None else (int(cin_slice[0]), int(cin_slice[1]))
            if not 0 <= c0 < c1 <= cin:
                raise ValueError(f"{what}: cin_slice {cin_slice} is not inside the kernel's {cin} input channels")
            geom = dict(N=cout, C=c1 - c0, KH=kh, KW=kw, s_n=1, s_c=cout, s_tap=cin * cout, offset=c0 * cout)
        else:
            if tuple(kernel.shape[:2]) != (2, 2) or cin_slice is not None:
                raise ValueError(f"{what}: layout 'deconv' takes a whole [2,2,cout,cin] kernel, got {tuple(kernel.shape)}")
            cout, cin = int(kernel.shape[2]), int(kernel.shape[3])
            geom = dict(N=4 * cout, C=cin, KH=1, KW=1, s_n=cin, s_c=1, s_tap=0, offset=0)
        if (geom["N"], geom["C"], geom["KH"], geom["KW"]) != (p.cout, p.span, p.KH, p.KW):
            raise ValueError(f"{what}: the master is a {geom['KH']}x{geom['KW']} kernel of {geom['C']} -> {geom['N']} channels, the "
                             f"packing one of {p.KH}x{p.KW}, {p.span} -> {p.cout}")
        if (bias is None) != (self.bias is None):
            raise ValueError(f"{what}: the packing has {'no' if self.bias is None else 'a'} bias, the master "
                             f"{'none' if bias is None else 'one'}")
        if bias is not None and (bias_reps < 1 or bias.numel() * bias_reps != self.bias.numel()):
            raise ValueError(f"{what}: a bias of {bias.numel()} elements x {bias_reps} is not the packing's {self.bias.numel()}")
        self._master = dict(kernel=kernel, bias=bias, bias_reps=int(bias_reps), **geom)
        self._keras_kernel = None
        _forms_epoch[0] += 1
        self.p = dataclasses.replace(p, wgt=None, bias=None)
        if self._dgrad is not None:
            self._dgrad.p = dataclasses.replace(self._dgrad.p, wgt=None)

    def _side(self, forms=None):
        """This packing's destinations as one orientation of a re-pack job: every materialised form, or those of `forms`."""
        have = {"wgt": self.wgt, "x3": self._wgt_x3, "h": self._wgt_h, "wino": self._wgt_wino}
        side = {k: v for k, v in (have if forms is None else forms).items() if v is not None}
        side.update(n_pad=self.p.n_pad, span_pad=self.p.span_pad, span_pad_h=self.span_pad_h)
        return side

    def _job(self, fwd=None, tr=None, bias=None):
        m = self._master
        return dict(kind="conv", src=m["kernel"], src_bias=m["bias"], bias=bias, cpp_shift=self.p.cpp_shift,
                    group_cin_step=self.p.group_cin_step, fwd=fwd, tr=tr,
                    **{k: m[k] for k in ("N", "C", "KH", "KW", "s_n", "s_c", "s_tap", "offset", "bias_reps")})

    def repack_jobs(self):
        """The jobs (one) that bring every materialised form of this packing, and of its `dgrad` if that exists, up to the
        master it is bound to: what ops.repack_weights takes."""
        if self._master is None:
            raise RuntimeError("DeviceConv.repack_jobs: the packing follows no master (bind_master)")
        return [self._job(fwd=self._side(), tr=None if self._dgrad is None else self._dgrad._side(), bias=self.bias)]

    def _empty_form(self, form, dev=None):
        p, dev = self.p, (self.wgt.device if dev is None else dev)
        taps = p.KH * p.KW
        if form == "wino":
            if (p.KH, p.KW) != (3, 3) or p.shuffle2x2 or p.n_pad % 32 or p.span_pad % 8:
                raise ValueError("winograd packing needs a dense 3x3 conv (n_pad % 32 == 0)")
            return torch.empty((max(4, p.n_pad // 32), p.span_pad // 8, 8, 32, 16), dtype=torch.float32, device=dev)
        if form == "h":
            return torch.empty((p.n_pad, taps * self.span_pad_h), dtype=torch.float16, device=dev)
        return torch.empty((p.n_pad, taps * p.span_pad), dtype=torch.float32, device=dev)

    def _form_from_master(self, form):
        """A form first asked for after binding: made on the device from the master, never from the stale host weights."""
        t = self._empty_form(form)
        if self._master is not None:
            repack_weights([self._job(fwd=self._side({form: t}))])
        else:
            repack_weights([self._tr_of._job(tr=self._side({form: t}))])
        return t

    def _dgrad_from_master(self):
        m, p = self._master, self.p
        if p.shuffle2x2:
            raise ValueError("unpack_dense: a dense packing only (no row-span, grouped or shuffle2x2 packing)")
        tp = transposed_geometry(p.KH, p.KW, m["C"], m["N"])
        d = DeviceConv.__new__(DeviceConv)
        d.p, d.bias = tp, None
        d._init_forms()
        d._tr_of = self
        d.wgt = d._empty_form("wgt", self.wgt.device)
        repack_weights([self._job(tr=d._side())])
        return d


def _conv_desc(x, dc, stride=1, padding="same", dilation=1, act=_lib.ACT_NONE, residual=None, out=None,
               out_coff=0, in_coff=0, out_view=None, out_dtype=None, live=None, gn_partials=None):
    """Build the ml_conv2d_desc for one problem.  -> (desc, result tensor, profile record args).
    A float16 `x` selects the fp16-storage kernels (ML_MATH_F16S: half weights, half residual); the output is half
    unless the destination says otherwise (`out` / `out_view` tensor of dtype float32, out_dtype=torch.float32, or a
    sigmoid activation: the predictions the model returns are fp32).  out_dtype=torch.float16 on an fp32 `x` makes the
    generic kernel store half (the stem of an fp16-storage body)."""
    p = dc.p
    _require_dev(x, "x")
    half_in = x.dtype == torch.float16
    if out is not None:
        odt = out.dtype
    elif out_view is not None:
        odt = out_view[0].dtype
    elif out_dtype is not None:
        odt = out_dtype
    else:
        odt = torch.float16 if (half_in and act != _lib.ACT_SIGMOID) else torch.float32
    if odt not in (torch.float16, torch.float32):
        raise ValueError(f"conv2d: output dtype {odt} not supported")
    if half_in and residual is not None and residual.dtype != torch.float16:
        raise ValueError("conv2d: an fp16-storage conv takes a float16 residual")
    es_o = 2 if odt == torch.float16 else 4
    B, H, W, Cbuf = x.shape
    if p.cpp_shift != 30:
        if Cbuf != p.cin_buffer:
            raise ValueError(f"row-span conv expects a {p.cin_buffer}-channel padded image, got {Cbuf}")
    elif not p.group_cin_step and in_coff + p.span > Cbuf:
        raise ValueError(f"conv2d: input has {Cbuf} channels, kernel needs [{in_coff},{in_coff + p.span})")
    Ho, Wo, pt, pl = resolve_padding(H, W, p.kh_real, p.kw_real, stride, dilation, padding)
    co = p.cout // 4 if p.shuffle2x2 else p.cout
    oh, ow = (2 * Ho, 2 * Wo) if p.shuffle2x2 else (Ho, Wo)
    d = _lib.ConvDesc()
    if out_view is not None:
        vt, elem_off, vcs, vbs = out_view
        _require_dev(vt, "out_view")
        if p.shuffle2x2 or vcs < co or vbs < oh * ow * vcs:
            raise ValueError("conv2d: bad out_view")
        if elem_off + (B - 1) * vbs + oh * ow * vcs > vt.numel():
            raise ValueError("conv2d: out_view exceeds the destination tensor")
        ret = vt
        d.out = vt.data_ptr() + es_o * elem_off
        d.out_cstride, d.out_coff, d.out_bstride = vcs, 0, vbs
    else:
        if out is None:
            out = torch.empty((B, oh, ow, co), dtype=odt, device=x.device)
            out_coff = 0
        else:
            _require_dev(out, "out")
            if tuple(out.shape[:3]) != (B, oh, ow) or out.dtype != odt:
                raise ValueError(f"conv2d: out buffer {tuple(out.shape)} / {out.dtype} does not match {(B, oh, ow)} / {odt}")
        ret = out
        d.out = out.data_ptr()
        d.out_cstride, d.out_coff, d.out_bstride = out.shape[3], out_coff, 0
    x3 = CONV_MATH == "f32x3" and not half_in
    d.in_, d.wgt, d.bias = x.data_ptr(), (dc.wgt_h if half_in else (dc.wgt_x3 if x3 else dc.wgt)).data_ptr(), \
        (dc.bias.data_ptr() if dc.bias is not None else None)
    if residual is not None:
        _require_dev(residual, "residual")
        if tuple(residual.shape[:3]) != (B, Ho, Wo):
            raise ValueError("conv2d: residual spatial shape mismatch")
        d.residual, d.res_cstride, d.res_coff = residual.data_ptr(), residual.shape[3], 0
    d.B, d.H, d.W = B, H, W
    d.in_cstride, d.in_coff = Cbuf, in_coff
    d.span, d.span_pad, d.cpp_shift = p.span, (dc.span_pad_h if half_in else p.span_pad), p.cpp_shift
    d.Ho, d.Wo = Ho, Wo
    d.KH, d.KW, d.stride, d.dil, d.pad_t, d.pad_l = p.KH, p.KW, stride, dilation, pt, pl
    d.cout, d.n_pad = p.cout, p.n_pad
    d.act, d.group_cin_step, d.shuffle2x2, d.tile = act, p.group_cin_step, p.shuffle2x2, p.tile
    if gn_partials is not None:        # float64 [tiles, 4, 2]: the epilogue also sums what each 128-row tile stores (per wave)
        _require_dev(gn_partials, "gn_partials")
        if gn_partials.dtype != torch.float64 or gn_partials.numel() < 8 * ((B * Ho * Wo + 127) // 128):
            raise ValueError("conv2d: gn_partials must be a float64 tensor of 4 x 2 values per 128-row tile")
        if d.out_coff % 4 or d.out_cstride % 4:        # only the vector epilogue writes the partial sums
            raise ValueError("conv2d: gn_partials needs a destination slice aligned to 4 channels")
        d.gn_partials = gn_partials.data_ptr()
    if live is not None:               # (device int32 tensor [1], slots per image): a fixed-capacity RoI batch
        lv, period = live
        _require_dev(lv, "live")
        d.live, d.live_period = lv.data_ptr(), int(period)
    if half_in:
        d.math, d.out_f16 = _lib.MATH_F16S, int(odt == torch.float16)
    else:
        d.math, d.out_f16 = _MATH_CODE[CONV_MATH], int(odt == torch.float16)
        if d.out_f16 and d.math != _lib.MATH_F16:
            raise ValueError("conv2d: a half output from fp32 input needs the fp16 MFMA mode (set_conv_math('f16s'))")
    M = B * Ho * Wo
    real_cin = p.span if p.cpp_shift == 30 else 3
    es_in, es_out = x.element_size(), (2 if odt == torch.float16 else 4)
    nbytes = (es_in * B * H * W * real_cin * (1 if not p.group_cin_step else p.n_pad // 32) + es_out * M * p.cout +
              es_in * p.cout * p.k_real + (es_out * M * p.cout if residual is not None else 0))
    shape = f"M={M} N={p.cout} K={p.KH * p.KW * d.span_pad} k{p.kh_real}x{p.kw_real} s{stride} d{dilation} HxW={H}x{W}"
    return d, ret, (2.0 * M * p.cout * p.k_real, nbytes, shape)


def _conv_kernel_name(descs, n, p, half):
    """Name of the kernel a (non-Winograd) launch runs on (profiling hook only), as the library plans the launch: the
    persistent 1x1 kernels, or the generic kernel's instantiation -- small launches run on narrower tiles than the weights
    were packed for."""
    lib = _lib.load()
    which = lib.ml_conv2d_uses_pipe(descs) if n == 1 else 0      # 1: the 128 x 128 pipelined kernel, 2: the half 256 x 256 one
    if which:
        return "conv1x1_h256_h" if which == 2 else (
            "conv1x1_pipe_h" if half else ("conv1x1_pipe_x3" if CONV_MATH == "f32x3" else "conv1x1_pipe"))
    bn = lib.ml_conv2d_launch_ntile(descs, n, 1) or lib.ml_conv2d_ntile(p.cout, p.tile)
    bm = lib.ml_conv2d_launch_mtile(descs, n, 1) or 128
    return "conv_mfma_%dx%d%s%s" % (bm, bn, "_grouped" if p.group_cin_step else "",
                                     "_h" if half else {"f32": "", "f32x3": "_x3"}.get(CONV_MATH, "_f16"))


def _launch_conv(descs, problems, flops, nbytes, shapes, multi):
    """One ml_conv2d_multi_f32 launch of `descs` (problems: their (x, dc) pairs), moved onto the Winograd kernel when every
    problem qualifies.  Its profile name (PROFILE) and K slices (LAUNCH_LOG) are the library's plan of this launch."""
    lib = _lib.load()
    n = len(problems)
    x, dc = problems[0]
    wino = _wino_select(descs, n, problems)
    label = ("multi x%d" % n if multi else shapes[0]) + (" wino direct_flop=%.0f" % flops if wino else "")
    if wino:
        flops = sum(_wino_flops(descs[i]) for i in range(n))
    ws = workspace(int(lib.ml_conv2d_workspace_bytes()), x.device, "conv")
    if LAUNCH_LOG is not None:
        sp = (C.c_int32 * n)()
        _lib.check(lib.ml_conv2d_launch_splits(descs, n, ws.numel(), sp), "ml_conv2d_launch_splits")
        LAUNCH_LOG.append((" | ".join(shapes) if multi else label, tuple(int(v) for v in sp)))
    name = None
    if PROFILE is not None:
        name = "conv_wino_f32" if wino else _conv_kernel_name(descs, n, dc.p, x.dtype == torch.float16)
    with _Prof(name, flops, nbytes, label) as prof:
        if prof.on and name == "conv1x1_h256_h":
            # bytes this launch stages through the CUs' L1 -> LDS path: every 256-row tile takes its 256 x K activation rows
            # and the 256 x K weight rows of its N tile, 2 bytes each (what bounds that kernel: profiles/r04_h256_pmc.md)
            d = descs[0]
            M, N, K = d.B * d.Ho * d.Wo, d.cout, d.span
            prof.rec["staged_bytes"] = float(-(-M // 256) * (N // 256) * 2 * 256 * K * 2)
        _lib.check(lib.ml_conv2d_multi_f32(descs, n, _ptr(ws), ws.numel(), _stream()), "ml_conv2d_multi_f32")


def _wino_select(descs, n, problems):
    """Move a launch onto the Winograd F(2x2,3x3) kernel (tile = 6) when the conv math is "f32" and every problem holds fp32
    tensors, was packed for the automatic tile choice and passes one of the library's two predicates: the eligibility rule
    (ml_conv2d_wino_eligible: n_pad = 128) or the narrow case (ml_conv2d_wino_narrow: the same rule failed on n_pad alone --
    the 75- and 60-channel output convs of the towers, packed 96 and 64 wide).  A narrow problem is handed over with
    n_pad = 128 and DeviceConv.wgt_wino, which pads its weights to four 32-output blocks; the kernel launches
    ceil(cout / 64) channel blocks and runs no MFMA for a 32-channel half past cout.  The direct-path weights (dc.wgt, wgt_x3,
    wgt_h) are untouched.  A mixed launch stays on the direct kernel.  -> True if it was moved."""
    if CONV_MATH != "f32":
        return False
    lib = _lib.load()
    for i, (x, dc) in enumerate(problems):
        if x.dtype != torch.float32 or dc.p.tile != 0:
            return False
        if not (lib.ml_conv2d_wino_eligible(C.byref(descs[i])) or lib.ml_conv2d_wino_narrow(C.byref(descs[i]))):
            return False
    for i, (x, dc) in enumerate(problems):
        descs[i].tile, descs[i].n_pad = 6, 128
        descs[i].wgt = dc.wgt_wino.data_ptr()
    return True


def _wino_flops(d):
    """FLOP the Winograd kernel's MFMAs execute for one problem: 2 x tiles x 16 positions x Cin x Cout."""
    return 2.0 * d.B * ((d.Ho + 1) // 2) * ((d.Wo + 1) // 2) * 16 * d.span * d.cout


def _wino_gn_ok(out_shape):
    """Host copy of the library's gn_partials rule on the Winograd path (conv_wino.hip ml_conv2d_wino_gn_ok): every
    64-tile block covers two whole 128-pixel flattened tiles."""
    _, Ho, Wo = out_shape
    if Ho % 2 or Wo % 2:
        return False
    th, tw = Ho // 2, Wo // 2
    return (64 % tw == 0 or tw % 64 == 0) and (th * tw) % 64 == 0


def gn_fusable(out_shape, C_out, groups, dc, launch_tiles, dtype):
    """Can the GroupNormalization behind this conv take its statistics from the conv's epilogue (ml_conv2d_desc.gn_partials)?
    out_shape = (B, Ho, Wo): whole 128-row tiles per image and per chunk, one 128-wide N tile, fp32, and a launch big
    enough that the library neither narrows its tiles nor cuts K (ml_conv2d_gn_min_launch_tiles(): 257 tiles of 128 x 128 in
    all on a 256-CU part).
    -> (sum, sum of squares) pairs per chunk (4 per tile: one per wave), or 0."""
    B, Ho, Wo = out_shape
    hw = Ho * Wo
    p = dc.p
    # fp32 tensors on the exact / split-operand products, or half tensors (the heads of the fp16-storage mode: the sums are
    # then of the ROUNDED values the conv stores, which is what that mode's GroupNorm statistics pass reads)
    math_ok = (CONV_MATH in ("f32", "f32x3") and dtype == torch.float32) or (CONV_MATH == "f16s" and dtype == torch.float16)
    ok = (math_ok and C_out == 128 and p.cout == 128 and p.n_pad == 128 and
          not p.shuffle2x2 and not p.group_cin_step and hw % 128 == 0 and hw % groups == 0 and (hw // groups) % 128 == 0 and
          launch_tiles >= _gn_min_launch_tiles())
    # a conv the Winograd kernel may take ("f32", dense 3x3 'same' at stride 1 -- the towers): its blocks must also cover
    # whole 128-pixel tiles, whichever kernel the launch ends up on
    if ok and CONV_MATH == "f32" and p.KH == 3 and p.KW == 3 and p.cpp_shift == 30 and p.tile == 0:
        ok = _wino_gn_ok(out_shape)
    return 4 * ((hw // groups) // 128) if ok else 0


_GN_MIN_TILES = None


def _gn_min_launch_tiles():
    """The launch size from which the LIBRARY neither narrows the tiles nor cuts K on this device (asked once; not a
    constant of this file: it follows the device's compute-unit count)."""
    global _GN_MIN_TILES
    if _GN_MIN_TILES is None:
        _GN_MIN_TILES = int(_lib.load().ml_conv2d_gn_min_launch_tiles())
    return _GN_MIN_TILES


def conv2d(x, dc: DeviceConv, stride=1, padding="same", dilation=1, act=_lib.ACT_NONE,
           residual=None, out=None, out_coff=0, in_coff=0, out_view=None, out_dtype=None, gn_partials=None):
    """ml_conv2d_multi_f32 with one problem (split-K enabled through the shared workspace).
    `x` [B,H,W,Cbuf]; reads channels [in_coff, in_coff+cin).  Writes into
    `out[..., out_coff:out_coff+cout]` when given, else allocates.  `out_view=(tensor, elem_off,
    cstride, bstride)` writes image b's pixels at tensor.data + elem_off + b*bstride with row
    pitch cstride (used to land a level's head directly in the concatenated prediction)."""
    if x.dtype == torch.float16 and stride == 2 and dc.p.kh_real == 1 and dc.p.kw_real == 1:
        # a strided 1x1 conv on half tensors = the stride-1 kernel on the sampled pixels (ResNext.py:199-203 shortcuts)
        x, stride = subsample2_h(x), 1
    d, ret, (flops, nbytes, shape) = _conv_desc(x, dc, stride, padding, dilation, act, residual, out, out_coff,
                                                in_coff, out_view, out_dtype, gn_partials=gn_partials)
    _launch_conv((_lib.ConvDesc * 1)(d), [(x, dc)], flops, nbytes, [shape], multi=False)
    return ret


def conv2d_multi(problems):
    """One launch for several independent convs of the same tile shape.
    problems: list of dicts with keys x, dc and the keyword arguments of conv2d().  -> list of results."""
    n = len(problems)
    if n == 0:
        return []
    if n > _lib.CONV_MAX_PROBLEMS:
        return conv2d_multi(problems[:_lib.CONV_MAX_PROBLEMS]) + conv2d_multi(problems[_lib.CONV_MAX_PROBLEMS:])
    arr = (_lib.ConvDesc * n)()
    rets, flops, nbytes, shapes = [], 0.0, 0.0, []
    for i, pr in enumerate(problems):
        pr = dict(pr)
        d, ret, (f, nb, shape) = _conv_desc(pr.pop("x"), pr.pop("dc"), **pr)
        arr[i] = d
        rets.append(ret)
        flops += f
        nbytes += nb
        shapes.append(shape)
    _launch_conv(arr, [(pr["x"], pr["dc"]) for pr in problems], flops, nbytes, shapes, multi=True)
    return rets


def deconv2x2_out1x1_multi(problems, ncls, act_mid, act_out, tape=None):
    """ml_deconv2x2_out1x1_f32: Conv2DTranspose(2x2, s2) + act_mid -> Conv2D 1x1 + act_out, up to 4 RoI levels per launch.
    problems: dicts x [R,h,w,K] fp32 (R = images * rois_per_image), dc (DeviceConv of the transposed conv), wo_table,
    bo (device tensors from packing.pack_out1x1_table), out (the [B,total,2h,2w,ncls] tensor), out_base (elements),
    rois_per_image.
    tape: None, or a list that receives, per problem, T = the transposed conv's post-activation output as float32
    [R*h*w, 4, C_mid] (the GEMM layout; ml_deconv2x2_out1x1_tape_f32) for deconv2x2_out1x1_grad; `out` is bit-equal to
    the plain launch's.  float32 problems without `live` only.  A problem may name the tensor to store into ("tape_out")."""
    lib = _lib.load()
    n = len(problems)
    if n == 0:
        return
    if n > _lib.DECONV_OUT_MAX_PROBLEMS:
        deconv2x2_out1x1_multi(problems[:_lib.DECONV_OUT_MAX_PROBLEMS], ncls, act_mid, act_out, tape)
        deconv2x2_out1x1_multi(problems[_lib.DECONV_OUT_MAX_PROBLEMS:], ncls, act_mid, act_out, tape)
        return
    if tape is not None:
        if not isinstance(tape, list):
            raise TypeError("deconv2x2_out1x1: `tape` must be a list (it receives one tensor per problem)")
        for pr in problems:
            if isinstance(pr["x"], torch.Tensor) and pr["x"].dtype != torch.float32:
                raise TypeError(f"deconv2x2_out1x1: x is {pr['x'].dtype}; the tape launch is float32 only")
            if pr.get("live") is not None:
                raise ValueError("deconv2x2_out1x1: the fixed-capacity form (`live`) keeps no tape")
    arr = (_lib.DeconvOutProblem * n)()
    flops = nbytes = 0.0
    K = cmid = cp = None
    for i, pr in enumerate(problems):
        x, dc, out = pr["x"], pr["dc"], pr["out"]
        _require_dev(x, "x")
        _require_dev(out, "out")
        if x.dtype not in (torch.float32, torch.float16) or not x.is_contiguous() or out.dtype != torch.float32:
            raise ValueError("deconv2x2_out1x1: x must be a contiguous fp32 / fp16 [R,h,w,K] tensor, out fp32")
        if x.dtype != problems[0]["x"].dtype:
            raise ValueError("deconv2x2_out1x1: the problems of one launch must share the storage type")
        R, h, w, Kx = x.shape
        p = dc.p
        half = x.dtype == torch.float16
        if not p.shuffle2x2 or p.span != Kx or p.span_pad != Kx or p.cout % 4 or p.n_pad != p.cout or (half and Kx % 64):
            raise ValueError("deconv2x2_out1x1: `dc` must be a packed Conv2DTranspose whose input width is a multiple of "
                             "32 (64 for fp16 tensors)")
        if K is None:
            K, cmid, cp = Kx, p.cout // 4, int(pr["wo_table"].shape[-1])
        elif (K, cmid, cp) != (Kx, p.cout // 4, int(pr["wo_table"].shape[-1])):
            raise ValueError("deconv2x2_out1x1: the problems of one launch must share K, C_mid and the table width")
        if tuple(pr["wo_table"].shape) != (cmid // 32, 16, 2, cp):
            raise ValueError("deconv2x2_out1x1: wo_table has the wrong shape")
        n_l = int(pr["rois_per_image"])
        d = arr[i]
        d.x, d.wd, d.bd = x.data_ptr(), (dc.wgt_h if half else dc.wgt).data_ptr(), (dc.bias.data_ptr() if dc.bias is not None else None)
        d.wo_table, d.bo, d.out = pr["wo_table"].data_ptr(), pr["bo"].data_ptr(), out.data_ptr()
        d.M, d.hw, d.w, d.rois_per_image, d.reserved0 = R * h * w, h * w, w, n_l, 0
        d.out_image_stride, d.out_base = out.stride(0), int(pr["out_base"])
        if pr.get("live") is not None:
            d.live = pr["live"].data_ptr()
        last = (R // n_l - 1) * out.stride(0) + int(pr["out_base"]) + n_l * 4 * h * w * ncls
        if R % n_l or last > out.numel():
            raise ValueError("deconv2x2_out1x1: the RoI block does not fit the output tensor")
        flops += 2.0 * R * h * w * (4 * cmid * Kx + 4 * cmid * ncls)
        nbytes += x.element_size() * (x.numel() + 4 * cmid * Kx) + 4.0 * 4 * R * h * w * ncls
    half = problems[0]["x"].dtype == torch.float16
    if tape is not None:
        ts = []
        for i, pr in enumerate(problems):
            t = pr.get("tape_out")                # (tests: a tape inside a guarded buffer)
            if t is None:
                t = torch.empty((int(arr[i].M), 4, cmid), dtype=torch.float32, device=pr["x"].device)
            else:
                _grad_tensor("deconv2x2_out1x1", "tape_out", t, (int(arr[i].M), 4, cmid))
                _require_dev(t, "tape_out")
            ts.append(t)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        with _Prof("deconv2x2_out1x1_tape", flops, nbytes + sum(4.0 * t.numel() for t in ts), f"multi x{n}"):
            _lib.check(lib.ml_deconv2x2_out1x1_tape_f32(arr, ptrs, n, K, cmid, ncls, cp, act_mid, act_out, _stream()),
                       "ml_deconv2x2_out1x1_tape_f32")
        tape.extend(ts)
        return
    fn = lib.ml_deconv2x2_out1x1_f16 if half else lib.ml_deconv2x2_out1x1_f32
    with _Prof("deconv2x2_out1x1_h" if half else "deconv2x2_out1x1", flops, nbytes, f"multi x{n}"):
        _lib.check(fn(arr, n, K, cmid, ncls, cp, act_mid, act_out, _stream()), "ml_deconv2x2_out1x1")


# ------------------------------------------------------------------ slice-sum weight gradients (csrc/slice_sum.h)
def _slice_plan(entry_name, desc, *extra):
    """-> (slices, pixels per slice, bytes of the partials) of one problem, from the library's plan entry: host only"""
    slices, sp, nbytes = C.c_int32(), C.c_int32(), C.c_int64()
    _lib.check(getattr(_lib.load(), entry_name)(C.byref(desc), *extra, C.byref(slices), C.byref(sp), C.byref(nbytes)), entry_name)
    return slices.value, sp.value, nbytes.value


def _wgrad_pair(what, v, name):
    if v is None:
        return None, None
    if isinstance(v, torch.Tensor):
        return v, None
    if len(v) != 2:
        raise ValueError(f"{what}: `{name}` is a kernel tensor or a (kernel, bias) pair")
    return v[0], v[1]


def _wgrad_outputs(what, device, kshape, bshape, want_bias, add, out):
    """add / out of a weight gradient, each a kernel tensor or a (kernel, bias) pair (out = add + gradient; out may be add
    itself): shapes and dtypes first, they need no device -> (dkernel, dbias or None, add kernel, add bias)"""
    add_k, add_b = _wgrad_pair(what, add, "add")
    out_k, out_b = _wgrad_pair(what, out, "out")
    named = (("add kernel", add_k, kshape), ("out kernel", out_k, kshape), ("add bias", add_b, bshape), ("out bias", out_b, bshape))
    for name, t, shape in named:
        if t is not None:
            _grad_tensor(what, name, t, shape)
    if not want_bias and (add_b is not None or out_b is not None):
        raise ValueError(f"{what}: a bias `add` / `out` with want_bias=False")
    for name, t, _ in named:
        if t is not None:
            _require_dev(t, name)
    dk = torch.empty(kshape, dtype=torch.float32, device=device) if out_k is None else out_k
    db = None if not want_bias else (torch.empty(bshape, dtype=torch.float32, device=device) if out_b is None else out_b)
    return dk, db, add_k, add_b


def _slice_sum_multi(prof, made, device, limit, desc_type, plan_entry, launch_entry, extra=(), workspace_bytes=None):
    """The launch pairs of the weight-gradient problems `made`, a list of (descriptor, outputs, (flops, bytes, shape or None)):
    at most `limit` problems ride in one pair, and a pair is cut where its partials would exceed the conv workspace (more
    launches, the same bits).  extra: what the plan and launch entries take between the problems and the workspace;
    workspace_bytes: None, or the size to give the launch (tests).  -> the problems' outputs"""
    def split(cut):
        return (_slice_sum_multi(prof, made[:cut], device, limit, desc_type, plan_entry, launch_entry, extra, workspace_bytes) +
                _slice_sum_multi(prof, made[cut:], device, limit, desc_type, plan_entry, launch_entry, extra, workspace_bytes))

    n = len(made)
    if n == 0:
        return []
    if n > limit:
        return split(limit)
    lib = _lib.load()
    plan = getattr(lib, plan_entry)
    ws_bytes = int(lib.ml_conv2d_workspace_bytes())
    arr = (desc_type * n)()
    need, flops, nbytes = [], 0.0, 0.0
    for i, (d, _, (f, nb, _)) in enumerate(made):
        arr[i] = d
        ws_i = C.c_int64()
        _lib.check(plan(C.byref(d), *extra, None, None, C.byref(ws_i)), plan_entry)
        need.append(ws_i.value)
        flops += f
        nbytes += nb
    if n > 1 and sum(need) > ws_bytes:
        # more partials than the conv workspace holds (maps far larger than the towers'): two launches, the same bits
        return split(max(1, next(i for i in range(1, n + 1) if sum(need[:i]) > ws_bytes) - 1))
    ws = workspace(ws_bytes, device, "conv")
    given = ws.numel() if workspace_bytes is None else int(workspace_bytes)
    with _Prof(prof, flops, nbytes, made[0][2][2] if n == 1 and made[0][2][2] else "multi x%d" % n):
        _lib.check(getattr(lib, launch_entry)(arr, n, *extra, _ptr(ws), given, _stream()), launch_entry)
    return [outs for _, outs, _ in made]


# ------------------------------------------------------------------ fused mask-head tail, backward (csrc/deconv_out_grad.hip)
def deconv2x2_out1x1_grad_geometry(M, hw, w, rois_per_image, c_mid, dy_image_stride=0, dy_base=0):
    """The ml_deconv_out_grad_problem of a problem without its tensors: geometry only (what the plan reads)."""
    d = _lib.DeconvOutGradProblem()
    d.M, d.hw, d.w, d.rois_per_image, d.c_mid = int(M), int(hw), int(w), int(rois_per_image), int(c_mid)
    d.dy_image_stride, d.dy_base = int(dy_image_stride), int(dy_base)
    return d


def deconv2x2_out1x1_grad_plan(M, hw, w, rois_per_image, c_mid, ncls):
    """-> (slices, pixels per slice, bytes of the partials) of one tail-backward problem: ml_deconv2x2_out1x1_grad_plan, host
    only.  A function of the problem's geometry alone."""
    return _slice_plan("ml_deconv2x2_out1x1_grad_plan", deconv2x2_out1x1_grad_geometry(M, hw, w, rois_per_image, c_mid), int(ncls))


def _tail_grad_problem(dy, T, wo, hw, rois_per_image, dy_base=0, out=None, out_kernel=None, out_bias=None):
    """The checks of one tail-backward problem (dtypes and shapes first: they need no device) -> (descriptor, (dT, dkernel,
    dbias), (flops, bytes, None))"""
    what = "deconv2x2_out1x1_grad"
    for name, t in (("dy", dy), ("T", T), ("wo", wo)):
        _grad_tensor(what, name, t)
    if dy.dim() != 5:
        raise ValueError(f"{what}: `dy` must be the [B, total, 2h, 2w, ncls] tensor, got {tuple(dy.shape)}")
    B, total, oh, ow, ncls = (int(v) for v in dy.shape)
    h, w = (int(v) for v in hw)
    if (oh, ow) != (2 * h, 2 * w):
        raise ValueError(f"{what}: dy maps are {oh} x {ow}, the crops {h} x {w}")
    if T.dim() != 3 or T.shape[1] != 4:
        raise ValueError(f"{what}: `T` must be [M, 4, C_mid], got {tuple(T.shape)}")
    M, _, cmid = (int(v) for v in T.shape)
    n_l, dy_base = int(rois_per_image), int(dy_base)
    if n_l < 1 or M != B * n_l * h * w:
        raise ValueError(f"{what}: T has {M} pixels, {B} images x {n_l} RoIs x {h} x {w} are {B * n_l * h * w}")
    if cmid % 4 or cmid > 256:
        raise ValueError(f"{what}: C_mid = {cmid} must be a multiple of 4, at most 256")
    if ncls > 32:
        raise ValueError(f"{what}: {ncls} classes: at most 32")
    if M >= 1 << 24:
        raise ValueError(f"{what}: {M} input pixels: fewer than 2^24 per problem")
    if tuple(wo.shape[-2:]) != (cmid, ncls) or wo.numel() != cmid * ncls:
        raise ValueError(f"{what}: `wo` is {tuple(wo.shape)}, expected the 1x1 kernel [1, 1, {cmid}, {ncls}]")
    per_roi = 4 * h * w * ncls
    if dy_base < 0 or dy_base % per_roi or dy_base // per_roi + n_l > total:
        raise ValueError(f"{what}: dy_base {dy_base} with {n_l} RoIs per image is no RoI block of {total} RoIs")
    for name, t, shape in (("out", out, (M, 4, cmid)), ("out_kernel", out_kernel, (1, 1, cmid, ncls)), ("out_bias", out_bias, (ncls,))):
        if t is not None:
            _grad_tensor(what, name, t, shape)
    for name, t in (("dy", dy), ("T", T), ("wo", wo), ("out", out), ("out_kernel", out_kernel), ("out_bias", out_bias)):
        if t is not None:
            _require_dev(t, name)
    dT = torch.empty((M, 4, cmid), dtype=torch.float32, device=T.device) if out is None else out
    dk = torch.empty((1, 1, cmid, ncls), dtype=torch.float32, device=T.device) if out_kernel is None else out_kernel
    db = torch.empty((ncls,), dtype=torch.float32, device=T.device) if out_bias is None else out_bias
    d = deconv2x2_out1x1_grad_geometry(M, h * w, w, n_l, cmid, dy.stride(0), dy_base)
    d.dy, d.t, d.wo, d.out, d.dkernel, d.dbias = (t.data_ptr() for t in (dy, T, wo, dT, dk, db))
    flops = 2.0 * M * 4 * cmid * ncls * 2
    nbytes = 4.0 * (2 * T.numel() + M * 4 * ncls)
    return d, (dT, dk, db), (flops, nbytes, None)


def deconv2x2_out1x1_grad(dy, T, wo, hw, rois_per_image, dy_base=0, out=None, out_kernel=None, out_bias=None,
                          workspace_bytes=None):
    """Backward of the fused mask-head tail (csrc/deconv_out_grad.hip), float32, in one pass over T: dy [B,total,2h,2w,ncls]
    is the gradient at the 1x1 conv's PRE-activation, read in place (this problem's RoIs are rows dy_base / (4 h w ncls) ..
    + rois_per_image of every image); T [M,4,C_mid] the tape of deconv2x2_out1x1_multi(tape=); wo the 1x1 kernel
    [1,1,C_mid,ncls]; hw = (h, w) of the crops.  -> (dT [M,4,C_mid], the gradient at the transposed conv's pre-activation in
    T's layout -- out=T writes it over the tape --, dkernel [1,1,C_mid,ncls], dbias [ncls]).  A fixed summation order: two
    launches give the same bits, alone or in deconv2x2_out1x1_grad_multi.  workspace_bytes: None, or the size to give the
    launch (tests)."""
    return deconv2x2_out1x1_grad_multi([dict(dy=dy, T=T, wo=wo, hw=hw, rois_per_image=rois_per_image, dy_base=dy_base, out=out,
                                             out_kernel=out_kernel, out_bias=out_bias)], workspace_bytes)[0]


def deconv2x2_out1x1_grad_multi(problems, workspace_bytes=None):
    """ml_deconv2x2_out1x1_grad_f32: up to 4 RoI levels in one launch pair (more go in several launches).  problems: list
    of dicts with deconv2x2_out1x1_grad's arguments -> list of (dT, dkernel, dbias), the bits of the single calls."""
    if not problems:
        return []
    what = "deconv2x2_out1x1_grad"
    for pr in problems:
        _grad_tensor(what, "dy", pr["dy"])
    ncls = int(problems[0]["dy"].shape[-1])
    if any(int(pr["dy"].shape[-1]) != ncls for pr in problems):
        raise ValueError(f"{what}: the problems of one launch must share the class count")
    return _slice_sum_multi(what, [_tail_grad_problem(**pr) for pr in problems], problems[0]["T"].device,
                            _lib.DECONV_OUT_MAX_PROBLEMS, _lib.DeconvOutGradProblem, "ml_deconv2x2_out1x1_grad_plan",
                            "ml_deconv2x2_out1x1_grad_f32", (ncls,), workspace_bytes)


def deconv2x2_grad_relayout(dk1x1, db4):
    """The transposed conv's weight gradient in the layer's own shapes (ml_deconv2x2_grad_relayout_f32): dk1x1
    [1,1,cin,4*C_mid] -> [2,2,C_mid,cin]; db4 [4*C_mid] (or None) -> [C_mid], the four positions added in the order 0..3."""
    what = "deconv2x2_grad_relayout"
    _grad_tensor(what, "dk1x1", dk1x1)
    if dk1x1.dim() != 4 or tuple(dk1x1.shape[:2]) != (1, 1) or dk1x1.shape[3] % 4:
        raise ValueError(f"{what}: `dk1x1` must be [1, 1, cin, 4*C_mid], got {tuple(dk1x1.shape)}")
    cin, cmid = int(dk1x1.shape[2]), int(dk1x1.shape[3]) // 4
    if db4 is not None:
        _grad_tensor(what, "db4", db4, (4 * cmid,))
        _require_dev(db4, "db4")
    _require_dev(dk1x1, "dk1x1")
    dk = torch.empty((2, 2, cmid, cin), dtype=torch.float32, device=dk1x1.device)
    db = None if db4 is None else torch.empty((cmid,), dtype=torch.float32, device=dk1x1.device)
    _lib.check(_lib.load().ml_deconv2x2_grad_relayout_f32(_ptr(dk1x1), _ptr(db4), _ptr(dk), _ptr(db), cin, cmid, _stream()),
               "ml_deconv2x2_grad_relayout_f32")
    return dk, db


def gconv3x3(x, wgt, bias, c, stride=1, padding=((1, 1), (1, 1)), act=_lib.ACT_NONE):
    """ml_gconv3x3_f32: ResNeXt grouped 3x3, wgt [C,9,c] (packing.pack_grouped_mfma4)."""
    lib = _lib.load()
    _require_dev(x, "x")
    B, H, W, Cc = x.shape
    Ho, Wo, pt, pl = resolve_padding(H, W, 3, 3, stride, 1, padding)
    half = x.dtype == torch.float16
    out = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    fn = lib.ml_gconv3x3_f16 if half else lib.ml_gconv3x3_f32
    with _Prof("gconv3x3_mfma4_h" if half else "gconv3x3_mfma4", 2.0 * B * Ho * Wo * Cc * 9 * c,
               x.element_size() * (x.numel() + out.numel()) + 4 * wgt.numel(),
               f"M={B * Ho * Wo} C={Cc} c={c} s{stride} HxW={H}x{W}"):
        _lib.check(fn(_ptr(x), _ptr(wgt), _ptr(bias), _ptr(out), B, H, W, Cc, c, Ho, Wo, stride, pt, pl, act, _stream()),
                   "ml_gconv3x3")
    return out


def dwconv3x3(x, wgt, bias, stride=1, padding="same", dilation=1, act=_lib.ACT_NONE, out=None, out_coff=0):
    lib = _lib.load()
    _require_dev(x, "x")
    B, H, W, Cc = x.shape
    Ho, Wo, pt, pl = resolve_padding(H, W, 3, 3, stride, dilation, padding)
    half = x.dtype == torch.float16
    if out is None:
        out = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
        out_coff = 0
    elif out.dtype != x.dtype:
        raise ValueError("dwconv3x3: out must have the input's dtype")
    fn = lib.ml_dwconv3x3_f16 if half else lib.ml_dwconv3x3_f32
    with _Prof("dwconv3x3_h" if half else "dwconv3x3", 18.0 * B * Ho * Wo * Cc,
               x.element_size() * (x.numel() + B * Ho * Wo * Cc) + 4 * 9 * Cc):
        _lib.check(fn(_ptr(x), _ptr(wgt), _ptr(bias), _ptr(out), B, H, W, Cc, Cc, 0,
                      out.shape[3], out_coff, Ho, Wo, stride, dilation, pt, pl, act, _stream()), "ml_dwconv3x3")
    return out


def has_fused_stem():
    """True when the current conv math has the fused stem + max-pool kernel (stem_pool): "f32", "f32x3" and "f16s".
    "f16" (fp32 tensors, f16 operands) has none: its stem runs as conv2d + maxpool3x3s2."""
    return CONV_MATH in ("f32", "f32x3", "f16s")


def stem_pool(x4, dc: "DeviceConv"):
    """ml_stem7x7s2_pool_f32 / _x3 / _f16: the ResNeXt stem (7x7 stride-2 conv + folded BN + ReLU) and the 3x3 stride-2
    max-pool behind it in ONE kernel, fp32 NHWC4 image in, the un-pooled stem output never written -- in the current conv
    math: "f32" exact fp32 products (only those with a non-zero weight), "f32x3" the split-operand products, "f16s" operands
    rounded to half and a half pooled map.  The same bits as conv2d(stem, relu) + maxpool3x3s2 in that math.
    `dc` = the stem's row-span DeviceConv."""
    lib = _lib.load()
    _require_dev(x4, "x4")
    p = dc.p
    B, H, W, c4 = x4.shape
    if x4.dtype != torch.float32 or c4 != 4 or p.cpp_shift == 30 or p.KH != 7 or p.span_pad != 32 or p.cout != 64 or p.n_pad != 64:
        raise ValueError("stem_pool: needs the fp32 NHWC4 image and the 7x7 / 64-filter row-span stem packing")
    if not has_fused_stem():
        raise ValueError(f"stem_pool: no fused stem in conv math {CONV_MATH!r}")
    if CONV_MATH == "f16s":
        label, fn, w, dtype = "stem7x7s2_pool_h", lib.ml_stem7x7s2_pool_f16, dc.wgt_stem_h, torch.float16
    elif CONV_MATH == "f32x3":
        label, fn, w, dtype = "stem7x7s2_pool_x3", lib.ml_stem7x7s2_pool_x3, dc.wgt_x3, torch.float32
    else:
        label, fn, w, dtype = "stem7x7s2_pool", lib.ml_stem7x7s2_pool_f32, dc.wgt, torch.float32
    Hc, Wc = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    Hp, Wp = (Hc + 2 - 3) // 2 + 1, (Wc + 2 - 3) // 2 + 1
    out = torch.empty((B, Hp, Wp, 64), dtype=dtype, device=x4.device)
    es = out.element_size()
    with _Prof(label, 2.0 * B * Hc * Wc * 64 * 147, 16 * B * H * W + es * out.numel() + es * 64 * 224,
               f"B={B} HxW={H}x{W} -> {Hp}x{Wp}x64"):
        _lib.check(fn(_ptr(x4), _ptr(w), _ptr(dc.bias), _ptr(out), B, H, W, Hp, Wp, _stream()), "ml_stem7x7s2_pool")
    return out


def maxpool3x3s2(x, pad=1):
    lib = _lib.load()
    _require_dev(x, "x")
    B, H, W, Cc = x.shape
    Ho = (H + 2 * pad - 3) // 2 + 1
    Wo = (W + 2 * pad - 3) // 2 + 1
    half = x.dtype == torch.float16
    out = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    fn = lib.ml_maxpool3x3s2_f16 if half else lib.ml_maxpool3x3s2_f32
    with _Prof("maxpool3x3s2_h" if half else "maxpool3x3s2", 0, x.element_size() * (x.numel() + out.numel())):
        _lib.check(fn(_ptr(x), _ptr(out), B, H, W, Cc, Ho, Wo, pad, pad, _stream()), "ml_maxpool3x3s2")
    return out


def subsample2_h(x):
    """ml_subsample2_f16: x[:, ::2, ::2, :] of a float16 NHWC tensor (what a 1x1 stride-2 conv reads)."""
    lib = _lib.load()
    _require_dev(x, "x")
    if x.dtype != torch.float16:
        raise RuntimeError("subsample2_h: float16 tensor expected")
    B, H, W, Cc = x.shape
    out = torch.empty((B, (H + 1) // 2, (W + 1) // 2, Cc), dtype=torch.float16, device=x.device)
    with _Prof("subsample2_h", 0, 2 * 2 * out.numel()):
        _lib.check(lib.ml_subsample2_f16(_ptr(x), _ptr(out), B, H, W, Cc, _stream()), "ml_subsample2_f16")
    return out


def cast_h2f(x):
    """ml_cast_f16_to_f32: a float16 tensor as float32 (the backbone taps handed to the fp32 heads)."""
    lib = _lib.load()
    _require_dev(x, "x")
    if x.dtype != torch.float16:
        raise RuntimeError("cast_h2f: float16 tensor expected")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with _Prof("cast_h2f", 0, 6 * x.numel()):
        _lib.check(lib.ml_cast_f16_to_f32(_ptr(x), _ptr(out), x.numel(), _stream()), "ml_cast_f16_to_f32")
    return out


def cast_f2h(x):
    """ml_cast_f32_to_f16: a float32 tensor as float16 (an fp32 tensor entering an fp16-storage part)."""
    lib = _lib.load()
    _require_dev(x, "x")
    if x.dtype != torch.float32:
        raise RuntimeError("cast_f2h: float32 tensor expected")
    out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    with _Prof("cast_f2h", 0, 6 * x.numel()):
        _lib.check(lib.ml_cast_f32_to_f16(_ptr(x), _ptr(out), x.numel(), _stream()), "ml_cast_f32_to_f16")
    return out


def preprocess(images, flip, mean, divisor, shift, out_channels=4):
    """BackBonePreProcess fused with the NHWC4 repack.  images: uint8 or float32 [B,H,W,3]."""
    lib = _lib.load()
    _require_dev(images, "images")
    if images.dtype not in (torch.uint8, torch.float32):
        raise TypeError("images must be uint8 or float32")
    B, H, W, ch = images.shape
    if ch != 3:
        raise ValueError("images must have 3 channels (RGB, 0..255)")
    out = torch.empty((B, H, W, out_channels), dtype=torch.float32, device=images.device)
    f3 = C.c_float * 3
    div3 = [float(divisor)] * 3 if np.isscalar(divisor) else [float(v) for v in divisor]
    sh3 = [float(shift)] * 3 if np.isscalar(shift) else [float(v) for v in shift]
    with _Prof("preprocess", 0, images.numel() * images.element_size() + 4 * out.numel()):
        _lib.check(lib.ml_preprocess_f32(_ptr(images), int(images.dtype == torch.uint8), _ptr(out), B * H * W,
                                         out_channels, int(flip), f3(*[float(m) for m in mean]), f3(*div3), f3(*sh3),
                                         _stream()), "ml_preprocess_f32")
    return out


def _gn_output(x, out, out_coff, dtype):
    """The output and dtype checks of one forward problem (`dtype`: the launch's) -> out"""
    _require_dev(x, "x")
    if out is None:
        out = torch.empty_like(x)
    _require_dev(out, "out")
    if out.shape[-1] == x.shape[-1]:
        if out.numel() != x.numel() or out_coff != 0:
            raise ValueError("groupnorm: dense output must match the input size")
    elif tuple(out.shape[:-1]) != tuple(x.shape[:-1]):
        raise ValueError("groupnorm: concat buffer spatial shape mismatch")
    if out.dtype != x.dtype or x.dtype != dtype or x.dtype not in (torch.float32, torch.float16):
        raise ValueError("groupnorm: every x / out of one launch must share a dtype (float32 or float16)")
    return out


def groupnorm_chunk(x, gamma, beta, groups, eps=1e-5, relu=False, out=None, out_coff=0):
    """`out` may be x itself (in place), a same-shape tensor, or a wider concat buffer
    [N,H,W,Cbuf] written at channels [out_coff, out_coff+C).  The single-problem kernels (a launch of one through
    groupnorm_chunk_multi has the same bits and is a little slower)."""
    lib = _lib.load()
    out = _gn_output(x, out, out_coff, x.dtype)
    N, Cc, hwc = x.shape[0], x.shape[-1], x.numel() // x.shape[0]
    half = x.dtype == torch.float16
    ws = workspace(lib.ml_groupnorm_workspace_bytes(N, groups), x.device, "gn")
    fn = lib.ml_groupnorm_chunk_f16 if half else lib.ml_groupnorm_chunk_f32
    with _Prof("groupnorm_chunk_h" if half else "groupnorm_chunk", 0, 2 * x.element_size() * x.numel(),
               f"N={N} HWC={hwc} G={groups}"):
        _lib.check(fn(_ptr(x), _ptr(out), _ptr(gamma), _ptr(beta), N, hwc, Cc, groups,
                      float(eps), int(relu), out.shape[-1], out_coff, _ptr(ws), _stream()), "ml_groupnorm_chunk")
    return out


def groupnorm_chunk_multi(problems):
    """ml_groupnorm_multi_f32: several independent GroupNormalizations in one launch pair, whatever their shapes (a
    problem that has no 16-byte accesses runs scalar ones beside the others).
    problems: list of dicts (x, gamma, beta, groups, eps, relu=False, out=None, out_coff=0) -> list of outputs."""
    lib = _lib.load()
    n = len(problems)
    if n == 0:
        return []
    if n > _lib.GN_MAX_PROBLEMS:
        return groupnorm_chunk_multi(problems[:_lib.GN_MAX_PROBLEMS]) + groupnorm_chunk_multi(problems[_lib.GN_MAX_PROBLEMS:])
    arr = (_lib.GnDesc * n)()
    outs, nbytes, ws_bytes = [], 0, 0
    for i, pr in enumerate(problems):
        x, out_coff = pr["x"], pr.get("out_coff", 0)
        out = _gn_output(x, pr.get("out"), out_coff, problems[0]["x"].dtype)
        N, Cc, out_cs = x.shape[0], x.shape[-1], out.shape[-1]
        d = arr[i]
        d.x, d.y = x.data_ptr(), out.data_ptr()
        d.gamma = pr["gamma"].data_ptr() if pr.get("gamma") is not None else None
        d.beta = pr["beta"].data_ptr() if pr.get("beta") is not None else None
        d.HWC, d.N, d.C, d.G = x.numel() // N, N, Cc, pr["groups"]
        d.relu, d.out_cstride, d.out_coff, d.eps = int(pr.get("relu", False)), out_cs, out_coff, float(pr.get("eps", 1e-5))
        d.dtype = int(x.dtype == torch.float16)
        if pr.get("live") is not None:
            lv, period = pr["live"]
            d.live, d.live_period = lv.data_ptr(), int(period)
        if pr.get("partials") is not None:         # (float64 [chunks * n, 2] written by the producing conv, n per chunk)
            pt, npc = pr["partials"]
            d.partials, d.n_partials = pt.data_ptr(), int(npc)
            nbytes -= x.element_size() * x.numel() // 3       # (algorithmic bytes stay 1R + 1W; the pass that is gone was the 3rd)
        ws_bytes += (int(lib.ml_groupnorm_workspace_bytes(N, pr["groups"])) + 255) // 256 * 256
        nbytes += 2 * x.element_size() * x.numel()
        outs.append(out)
    ws = workspace(ws_bytes, problems[0]["x"].device, "gn_multi")
    with _Prof("groupnorm_chunk_h" if problems[0]["x"].dtype == torch.float16 else "groupnorm_chunk", 0, nbytes, f"multi x{n}"):
        _lib.check(lib.ml_groupnorm_multi_f32(arr, n, _ptr(ws), ws.numel(), _stream()), "ml_groupnorm_multi_f32")
    return outs


def groupnorm_chunk_stats(x, groups):
    """(sum x, sum x^2) of every chunk of the chunk-wise GroupNormalization, float64 [N*groups, 2]: the forward's statistics
    pass on its own.  Accepted as `stats=` by groupnorm_chunk_grad, whose relu=True form then needs no pass of its own."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 2:
        raise ValueError("groupnorm_stats: x must be a float32 tensor [N, ..., C]")
    N, Cc = x.shape[0], x.shape[-1]
    if groups < 1 or Cc % groups:
        raise ValueError(f"groupnorm_stats: Number of groups ({groups}) must be a multiple of the number of channels ({Cc}).")
    _require_dev(x, "x")
    lib = _lib.load()
    stats = torch.empty((N * groups, 2), dtype=torch.float64, device=x.device)
    ws = workspace(lib.ml_groupnorm_workspace_bytes(N, groups), x.device, "gn")
    with _Prof("groupnorm_stats", 0, x.element_size() * x.numel(), f"N={N} HWC={x.numel() // N} G={groups}"):
        _lib.check(lib.ml_groupnorm_chunk_stats_f32(_ptr(x), _ptr(stats), N, x.numel() // N, Cc, groups, _ptr(ws), _stream()),
                   "ml_groupnorm_chunk_stats_f32")
    return stats


def _gn_grad_problem(x, dy, gamma, beta, groups, eps=1e-5, relu=False, input_relu=False, stats=None, out=None,
                     want_param_grads=True):
    """The argument checks of one backward problem (shapes and dtypes first: they need no device), and its outputs.
    -> (dx, dgamma, dbeta)"""
    for name, t in (("x", x), ("dy", dy)):
        if not isinstance(t, torch.Tensor) or t.dim() < 2:
            raise ValueError(f"groupnorm_grad: `{name}` must be a tensor [N, ..., C]")
        if t.dtype != torch.float32:
            raise TypeError(f"groupnorm_grad: `{name}` is {t.dtype}; the backward is float32 only")
    if tuple(dy.shape) != tuple(x.shape):
        raise ValueError(f"groupnorm_grad: dy {tuple(dy.shape)} must have x's shape {tuple(x.shape)}")
    N, Cc = x.shape[0], x.shape[-1]
    if groups < 1 or groups > Cc or Cc % groups:
        raise ValueError(f"groupnorm_grad: Number of groups ({groups}) must be a multiple of the number of channels ({Cc}).")
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (Cc,)):
            raise ValueError(f"groupnorm_grad: `{name}` must be float32 [{Cc}]")
    if stats is not None and (stats.dtype != torch.float64 or tuple(stats.shape) != (N * groups, 2)):
        raise ValueError(f"groupnorm_grad: `stats` must be float64 [{N * groups}, 2] (groupnorm_chunk_stats)")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != tuple(x.shape)):
        raise ValueError("groupnorm_grad: `out` must be a float32 tensor of x's shape (dy itself: in place)")
    for name, t in (("x", x), ("dy", dy), ("gamma", gamma), ("beta", beta), ("stats", stats), ("out", out)):
        if t is not None:
            _require_dev(t, name)
    if out is not None and out.data_ptr() == x.data_ptr():
        raise ValueError("groupnorm_grad: `out` may be dy, not x (the layer's input is read while dx is written)")
    dx = torch.empty_like(x) if out is None else out
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device) if want_param_grads else None
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device) if want_param_grads else None
    return dx, dgamma, dbeta


def groupnorm_chunk_grad(x, dy, gamma, beta, groups, eps=1e-5, relu=False, input_relu=False, stats=None, out=None,
                         want_param_grads=True):
    """Backward of groupnorm_chunk (csrc/groupnorm_grad.hip), float32: x is the layer's INPUT (the inference forward
    normalises in place and destroys it: run it with out=None and keep x), dy the gradient at its output.
    relu: the forward fused a ReLU behind the normalisation; input_relu: x is a ReLU's output and the gradient is wanted in
    front of that ReLU (the towers' Conv3x3 + ReLU -> GroupNormalization).  gamma=None: ones.  stats: groupnorm_chunk_stats(x,
    groups), saves the statistics pass of relu=True on large chunks.  out: None, or dy (in place on the gradient buffer).
    -> (dx, dgamma, dbeta); the last two are None unless want_param_grads."""
    dx, dgamma, dbeta = _gn_grad_problem(x, dy, gamma, beta, groups, eps, relu, input_relu, stats, out, want_param_grads)
    lib = _lib.load()
    N, Cc = x.shape[0], x.shape[-1]
    hwc = x.numel() // N
    ws = workspace(lib.ml_groupnorm_grad_workspace_bytes(N, groups, Cc), x.device, "gn")
    with _Prof("groupnorm_chunk_grad", 0, 3 * x.element_size() * x.numel(), f"N={N} HWC={hwc} G={groups}"):
        _lib.check(lib.ml_groupnorm_chunk_grad_f32(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(beta), _ptr(dx), _ptr(dgamma),
                                                   _ptr(dbeta), _ptr(stats), N, hwc, Cc, groups, float(eps), int(relu),
                                                   int(input_relu), _ptr(ws), _stream()), "ml_groupnorm_chunk_grad_f32")
    return dx, dgamma, dbeta


def groupnorm_chunk_grad_multi(problems):
    """ml_groupnorm_grad_multi_f32: several backward problems in one launch set.  problems: list of dicts with
    groupnorm_chunk_grad's arguments (x, dy, gamma, beta, groups, ...) -> list of (dx, dgamma, dbeta), the bits of the
    single calls, whatever the shapes."""
    n = len(problems)
    if n == 0:
        return []
    if n > _lib.GN_MAX_PROBLEMS:
        return (groupnorm_chunk_grad_multi(problems[:_lib.GN_MAX_PROBLEMS]) +
                groupnorm_chunk_grad_multi(problems[_lib.GN_MAX_PROBLEMS:]))
    outs = [_gn_grad_problem(**pr) for pr in problems]
    lib = _lib.load()
    arr = (_lib.GnGradDesc * n)()
    nbytes, ws_bytes = 0, 0
    for d, pr, (dx, dgamma, dbeta) in zip(arr, problems, outs):
        x = pr["x"]
        N, Cc = x.shape[0], x.shape[-1]
        d.x, d.dy, d.dx = x.data_ptr(), pr["dy"].data_ptr(), dx.data_ptr()
        for name, t in (("gamma", pr.get("gamma")), ("beta", pr.get("beta")), ("dgamma", dgamma), ("dbeta", dbeta),
                        ("stats", pr.get("stats"))):
            setattr(d, name, t.data_ptr() if t is not None else None)
        d.HWC, d.N, d.C, d.G = x.numel() // N, N, Cc, pr["groups"]
        d.relu, d.input_relu, d.eps = int(pr.get("relu", False)), int(pr.get("input_relu", False)), float(pr.get("eps", 1e-5))
        ws_bytes += int(lib.ml_groupnorm_grad_workspace_bytes(N, pr["groups"], Cc))
        nbytes += 3 * x.element_size() * x.numel()
    ws = workspace(ws_bytes, problems[0]["x"].device, "gn_multi")
    with _Prof("groupnorm_chunk_grad", 0, nbytes, f"multi x{n}"):
        _lib.check(lib.ml_groupnorm_grad_multi_f32(arr, n, _ptr(ws), ws.numel(), _stream()), "ml_groupnorm_grad_multi_f32")
    return outs


def batchnorm_plan(pixels, channels):
    """The slice plan of the BatchNormalization kernels (ml_batchnorm_plan), host only, a function of the geometry alone:
    pixels = B*H*W values per channel.  -> {"slices", "pixels_per_slice", "bytes"} (bytes: the workspace)."""
    slices, per, nbytes = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    lib = _lib.load()
    if lib.ml_batchnorm_plan(int(pixels), int(channels), C.byref(slices), C.byref(per), C.byref(nbytes)) != 0:
        raise ValueError(lib.ml_last_error().decode())
    return {"slices": slices.value, "pixels_per_slice": per.value, "bytes": nbytes.value}


def _bn_problem(what, maps, vectors, training=True, out=None, out_may_be=(), also=None):
    """The argument checks the three BatchNormalization ops share (shapes and dtypes first: they need no device), with the
    exception types of _gn_grad_problem.  maps: {name: tensor or None} of x's shape, x first; vectors: {name: tensor or
    None} of [C].  out: None or a float32 tensor of x's shape, which may be one of the maps named in out_may_be.  also(C):
    the op's own host checks, run before the first check that needs a device.
    -> (pixels, C)"""
    x = maps["x"]
    for name, t in maps.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dim() < 2:
            raise ValueError(f"{what}: `{name}` must be a tensor [..., C]")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: `{name}` is {t.dtype}; BatchNormalization's training kernels are float32 only")
        if tuple(t.shape) != tuple(x.shape):
            raise ValueError(f"{what}: `{name}` {tuple(t.shape)} must have x's shape {tuple(x.shape)}")
    Cc = x.shape[-1]
    N = x.numel() // max(Cc, 1)
    if Cc < 1 or Cc % 4:
        raise ValueError(f"{what}: C ({Cc}) must be a multiple of 4: lanes run along the channels with 16-byte accesses")
    if N < (2 if training else 1):
        raise ValueError(f"{what}: N ({N} pixels per channel) must be at least 2: the moving variance takes var_b*N/(N-1)")
    for name, t in vectors.items():
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (Cc,)):
            raise ValueError(f"{what}: `{name}` must be a float32 tensor [{Cc}]")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != tuple(x.shape)):
        raise ValueError(f"{what}: `out` must be a float32 tensor of x's shape")
    if also is not None:
        also(Cc)
    for name, t in list(maps.items()) + list(vectors.items()) + [("out", out)]:
        if t is not None:
            _require_dev(t, name)
    if out is not None:
        for name, t in maps.items():
            if t is not None and name not in out_may_be and out.data_ptr() == t.data_ptr():
                allowed = " or ".join(out_may_be)
                raise ValueError(f"{what}: `out` may be {allowed}, not {name}")
    return N, Cc


def _bn_forward_bytes(x, residual):
    """algorithmic: x (and the residual) read once, y written once"""
    return x.element_size() * x.numel() * (2 + (residual is not None))


def batchnorm_train(x, gamma, beta, moving_mean, moving_var, momentum, eps, relu=False, residual=None, out=None,
                    update_moving=True):
    """BatchNormalization in Keras's training mode (csrc/batchnorm.hip; include/masklab_hip.h has the arithmetic), float32
    NHWC: normalises with the statistics of the batch, y = x*scale + shift [+ residual] [ReLU], and moves moving_mean /
    moving_var toward the batch's (in place; update_moving=False: they are not touched and may be None).
    gamma / beta = None: scale=False / center=False.  out: None, or x itself (in place: then x is gone, no backward).
    -> (y, saved, batch_mean, batch_var): saved = float64 [C, 2] (mean_b, r) for batchnorm_grad; batch_var is the
    Bessel-corrected variance, as TF returns it."""
    what = "batchnorm_train"

    def also(Cc):
        if update_moving and (moving_mean is None or moving_var is None):
            raise ValueError(f"{what}: `moving_mean` and `moving_var` are needed with update_moving")
        if not 0.0 <= float(momentum) <= 1.0:
            raise ValueError(f"{what}: `momentum` ({momentum}) must be in [0, 1]")

    N, Cc = _bn_problem(what, {"x": x, "residual": residual}, {"gamma": gamma, "beta": beta, "moving_mean": moving_mean,
                                                               "moving_var": moving_var}, out=out, out_may_be=("x",), also=also)
    lib = _lib.load()
    y = torch.empty_like(x) if out is None else out
    saved = torch.empty((Cc, 2), dtype=torch.float64, device=x.device)
    batch_mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
    batch_var = torch.empty(Cc, dtype=torch.float32, device=x.device)
    ws = workspace(lib.ml_batchnorm_workspace_bytes(N, Cc), x.device, "gn")        # the normalisation layers' scratch
    mm, mv = (moving_mean, moving_var) if update_moving else (None, None)
    with _Prof("batchnorm_train", 0, _bn_forward_bytes(x, residual), f"N={N} C={Cc}"):
        _lib.check(lib.ml_batchnorm_train_f32(_ptr(x), _ptr(residual), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(mm), _ptr(mv),
                                              _ptr(saved), _ptr(batch_mean), _ptr(batch_var), N, Cc, float(eps),
                                              float(momentum), int(relu), _ptr(ws), ws.numel(), _stream()),
                   "ml_batchnorm_train_f32")
    return y, saved, batch_mean, batch_var


def batchnorm_infer(x, gamma, beta, moving_mean, moving_var, eps, relu=False, residual=None, out=None):
    """BatchNormalization's inference arithmetic on device-resident moving statistics (no host copy of them, no fold into a
    conv): y = x*scale + shift [+ residual] [ReLU], scale = gamma/sqrt(moving_var + eps), shift = beta - moving_mean*scale.
    out: None, or x itself."""
    what = "batchnorm_infer"

    def also(Cc):
        if moving_mean is None or moving_var is None:
            raise ValueError(f"{what}: `moving_mean` and `moving_var` are needed")

    N, Cc = _bn_problem(what, {"x": x, "residual": residual}, {"gamma": gamma, "beta": beta, "moving_mean": moving_mean,
                                                               "moving_var": moving_var}, training=False, out=out,
                        out_may_be=("x",), also=also)
    lib = _lib.load()
    y = torch.empty_like(x) if out is None else out
    ws = workspace(lib.ml_batchnorm_workspace_bytes(N, Cc), x.device, "gn")        # the normalisation layers' scratch
    with _Prof("batchnorm_infer", 0, _bn_forward_bytes(x, residual), f"N={N} C={Cc}"):
        _lib.check(lib.ml_batchnorm_infer_f32(_ptr(x), _ptr(residual), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(moving_mean),
                                              _ptr(moving_var), N, Cc, float(eps), int(relu), _ptr(ws), ws.numel(), _stream()),
                   "ml_batchnorm_infer_f32")
    return y


def batchnorm_grad(x, dy, saved, gamma, y=None, relu=False, out=None, want_residual_grad=False, want_param_grads=True):
    """Backward of batchnorm_train: x its input, dy the gradient at its output, saved its second result, gamma as given to it.
    relu: the forward fused a ReLU; y, the forward's output, is then needed (the mask is decided on it; with a residual it
    cannot be recomputed from x).  out: None, or dy (in place on the gradient buffer).  want_residual_grad: the gradient of
    the forward's residual (= g), a tensor of its own.
    -> (dx, d_residual | None, dgamma | None, dbeta | None)"""
    what = "batchnorm_grad"
    if relu and y is None:
        raise ValueError(f"{what}: `y` (the forward's output) is needed with relu: the mask is decided on it")

    def also(Cc):
        if not isinstance(saved, torch.Tensor) or saved.dtype != torch.float64 or tuple(saved.shape) != (Cc, 2):
            raise ValueError(f"{what}: `saved` must be float64 [{Cc}, 2] (batchnorm_train's second result)")

    N, Cc = _bn_problem(what, {"x": x, "dy": dy, "y": y if relu else None}, {"gamma": gamma}, out=out, out_may_be=("dy",),
                        also=also)
    _require_dev(saved, "saved")
    lib = _lib.load()
    dx = torch.empty_like(x) if out is None else out
    dres = torch.empty_like(x) if want_residual_grad else None
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device) if want_param_grads else None
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device) if want_param_grads else None
    ws = workspace(lib.ml_batchnorm_workspace_bytes(N, Cc), x.device, "gn")        # the normalisation layers' scratch
    nbytes = x.element_size() * x.numel() * (3 + int(relu) + int(want_residual_grad))
    with _Prof("batchnorm_grad", 0, nbytes, f"N={N} C={Cc}"):
        _lib.check(lib.ml_batchnorm_grad_f32(_ptr(x), _ptr(dy), _ptr(y if relu else None), _ptr(saved), _ptr(gamma), _ptr(dx),
                                             _ptr(dres), _ptr(dgamma), _ptr(dbeta), N, Cc, int(relu), _ptr(ws), ws.numel(),
                                             _stream()), "ml_batchnorm_grad_f32")
    return dx, dres, dgamma, dbeta


def resize_bilinear_ac(x, oh, ow, add=None, out=None, out_coff=0):
    lib = _lib.load()
    _require_dev(x, "x")
    B, H, W, Cc = x.shape
    half = x.dtype == torch.float16
    if Cc % 4 != 0:                    # e.g. the 3-class semantic map: scalar kernel, no add / concat view
        if add is not None or out is not None or half:
            raise RuntimeError("resize_bilinear_ac: add=/out=/float16 need a channel count that is a multiple of 4 (8)")
        return resize_image_ac(x, oh, ow)
    if out is None:
        out = torch.empty((B, oh, ow, Cc), dtype=x.dtype, device=x.device)
        out_coff = 0
    if out.dtype != x.dtype or (add is not None and add.dtype != x.dtype):
        raise ValueError("resize_bilinear_ac: x, add and out must share a dtype")
    add_cs = add.shape[3] if add is not None else 0
    fn = lib.ml_resize_bilinear_ac_f16 if half else lib.ml_resize_bilinear_ac_f32
    with _Prof("resize_bilinear_h" if half else "resize_bilinear", 0,
               x.element_size() * (x.numel() + B * oh * ow * Cc * (2 if add is not None else 1))):
        _lib.check(fn(_ptr(x), _ptr(add), _ptr(out), B, H, W, Cc, Cc, 0, oh, ow,
                      add_cs, 0, out.shape[3], out_coff, _stream()), "ml_resize_bilinear_ac")
    return out


def global_mean(x):
    lib = _lib.load()
    _require_dev(x, "x")
    B, H, W, Cc = x.shape
    out = torch.empty((B, 1, 1, Cc), dtype=x.dtype, device=x.device)
    fn = lib.ml_global_mean_f16 if x.dtype == torch.float16 else lib.ml_global_mean_f32
    _lib.check(fn(_ptr(x), _ptr(out), B, H * W, Cc, _stream()), "ml_global_mean")
    return out


def _grad_tensor(what, name, t, shape=None):
    """The checks every gradient tensor of the resampling backward passes: a float32 tensor (of `shape`)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: `{name}` must be a tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: `{name}` is {t.dtype}; the backward is float32 only")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: `{name}` is {tuple(t.shape)}, expected {tuple(shape)}")


def _grad_out(what, shape, device, add, out):
    """add / out of a resampling backward (out = add + gradient; out may be add itself) -> the tensor to write"""
    if shape[-1] % 4:
        raise ValueError(f"{what}: the channel count ({shape[-1]}) must be a multiple of 4 (16-byte accesses)")
    for name, t in (("add", add), ("out", out)):
        if t is not None:
            _grad_tensor(what, name, t, shape)
            _require_dev(t, name)
    return torch.empty(tuple(shape), dtype=torch.float32, device=device) if out is None else out


def resize_bilinear_ac_grad(dy, H, W, C=None, dy_coff=0, add=None, out=None):
    """Backward of resize_bilinear_ac (csrc/resample_grad.hip), float32: dy [B,Ho,Wo,Cs] is the gradient at the resize's
    output, read at channels dy_coff : dy_coff + C (the forward writes concat slices; C=None: all Cs) -> the gradient
    [B,H,W,C] at its input.  add / out: out = add + gradient, in place if they are the same tensor (the FPN top-down merge).
    A gather with a fixed summation order: two launches give the same bits; a 1x1 source takes a block reduction in fp64."""
    what = "resize_bilinear_ac_grad"
    _grad_tensor(what, "dy", dy)
    if dy.dim() != 4:
        raise ValueError(f"{what}: `dy` must be [B, Ho, Wo, C], got {tuple(dy.shape)}")
    B, Ho, Wo, Cs = dy.shape
    Cc = Cs - dy_coff if C is None else int(C)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or Cc < 1 or dy_coff < 0 or dy_coff + Cc > Cs:
        raise ValueError(f"{what}: channels {dy_coff} : {dy_coff + Cc} of {Cs} at {H} x {W} is no slice of dy")
    if Cs % 4 or dy_coff % 4:
        raise ValueError(f"{what}: dy's channel count ({Cs}) and the offset ({dy_coff}) must each be a multiple of 4 "
                         f"(16-byte accesses)")
    dx = _grad_out(what, (B, H, W, Cc), dy.device, add, out)
    _require_dev(dy, "dy")
    lib = _lib.load()
    ws_bytes = int(lib.ml_resize_bilinear_ac_grad_workspace_bytes(B, H, W, Cc, Ho, Wo))
    # (the slice sums of a 1x1 source, a few hundred KiB: from the caching allocator like the output, not a grow-only buffer)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dy.device) if ws_bytes else None
    with _Prof("resize_bilinear_grad", 0, 4 * (B * Ho * Wo * Cc + dx.numel() * (2 if add is not None else 1)),
               f"{Ho}x{Wo}->{H}x{W} C={Cc}"):
        _lib.check(lib.ml_resize_bilinear_ac_grad_f32(_ptr(dy), _ptr(add), _ptr(dx), B, H, W, Cc, Ho, Wo, Cs, dy_coff,
                                                      _ptr(ws), ws_bytes, _stream()), "ml_resize_bilinear_ac_grad_f32")
    return dx


def global_mean_grad(dpool, H, W, add=None, out=None):
    """Backward of global_mean: dpool [B,1,1,C] float32 -> dx[b,y,x,c] = dpool[b,0,0,c] / (H W) (+ add), one streaming launch."""
    what = "global_mean_grad"
    _grad_tensor(what, "dpool", dpool)
    if dpool.dim() != 4 or dpool.shape[1] != 1 or dpool.shape[2] != 1:
        raise ValueError(f"{what}: `dpool` must be [B, 1, 1, C], got {tuple(dpool.shape)}")
    B, Cc = dpool.shape[0], dpool.shape[3]
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"{what}: bad size {H} x {W}")
    dx = _grad_out(what, (B, H, W, Cc), dpool.device, add, out)
    _require_dev(dpool, "dpool")
    lib = _lib.load()
    with _Prof("global_mean_grad", 0, 4 * (dpool.numel() + dx.numel() * (2 if add is not None else 1)), f"{H}x{W} C={Cc}"):
        _lib.check(lib.ml_global_mean_grad_f32(_ptr(dpool), _ptr(add), _ptr(dx), B, H * W, Cc, _stream()),
                   "ml_global_mean_grad_f32")
    return dx


# ------------------------------------------------------------------ dense convolutions, backward (csrc/conv_grad.hip)
def _dense_only(what, p):
    """The packings the convolutions' backward takes: pack_dense.  The others are refused by name."""
    if p.group_cin_step:
        raise ValueError(f"{what}: grouped / depthwise convolutions are refused (dense convolutions only)")
    if p.cpp_shift != 30:
        raise ValueError(f"{what}: row-span (image input) convolutions are refused (dense convolutions only)")
    if p.shuffle2x2:
        raise ValueError(f"{what}: shuffle2x2 (Conv2DTranspose) convolutions are refused (dense convolutions only)")


def _dy_view(what, dy, dy_view, B, Ho, Wo, cout):
    """dy as a tensor [B,Ho,Wo,cout] or as the forward's out_view (tensor, element offset, channel stride, batch stride)
    -> (tensor, element offset, channel stride, batch stride or 0)"""
    if dy_view is None:
        _grad_tensor(what, "dy", dy, (B, Ho, Wo, cout))
        return dy, 0, cout, 0
    if dy is not None:
        raise ValueError(f"{what}: give `dy` or `dy_view`, not both")
    vt, elem_off, vcs, vbs = dy_view
    _grad_tensor(what, "dy_view", vt)
    elem_off, vcs, vbs = int(elem_off), int(vcs), int(vbs)
    if elem_off < 0 or vcs < cout or vbs < Ho * Wo * vcs or elem_off + (B - 1) * vbs + (Ho * Wo - 1) * vcs + cout > vt.numel():
        raise ValueError(f"{what}: dy_view (offset {elem_off}, channel stride {vcs}, batch stride {vbs}) is no view of "
                         f"[{B}, {Ho}, {Wo}, {cout}] inside a tensor of {vt.numel()} elements")
    return vt, elem_off, vcs, vbs


def conv2d_wgrad_geometry(x_shape, p, stride=1, padding="same", dilation=1, in_coff=0, dy_cstride=None, dy_bstride=0):
    """The ml_conv2d_wgrad_desc of a problem without its tensors: geometry only (what ml_conv2d_wgrad_plan reads).
    x_shape [B,H,W,Cbuf]; p: the forward's PackedConv."""
    what = "conv2d_wgrad"
    _dense_only(what, p)
    B, H, W, Cbuf = (int(v) for v in x_shape)
    if in_coff < 0 or in_coff + p.span > Cbuf:
        raise ValueError(f"{what}: x has {Cbuf} channels, the kernel needs [{in_coff}, {in_coff + p.span})")
    Ho, Wo, pt, pl = resolve_padding(H, W, p.kh_real, p.kw_real, stride, dilation, padding)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"{what}: the kernel does not fit the {H} x {W} input")
    g = _lib.ConvWgradDesc()
    d = g.conv
    d.B, d.H, d.W, d.in_cstride, d.in_coff = B, H, W, Cbuf, in_coff
    d.span, d.span_pad, d.cpp_shift = p.span, p.span_pad, p.cpp_shift
    d.Ho, d.Wo = Ho, Wo
    d.KH, d.KW, d.stride, d.dil, d.pad_t, d.pad_l = p.KH, p.KW, stride, dilation, pt, pl
    d.cout, d.n_pad = p.cout, p.n_pad
    d.out_cstride, d.out_coff, d.out_bstride = (p.cout if dy_cstride is None else int(dy_cstride)), 0, int(dy_bstride)
    d.group_cin_step, d.shuffle2x2, d.math = p.group_cin_step, p.shuffle2x2, _lib.MATH_F32
    return g


def conv2d_wgrad_plan(x_shape, p, **geometry):
    """-> (slices, pixels per slice, bytes of the partials) of one weight-gradient problem: ml_conv2d_wgrad_plan, host only.
    A function of the problem's geometry alone."""
    return _slice_plan("ml_conv2d_wgrad_plan", conv2d_wgrad_geometry(x_shape, p, **geometry))


def _wgrad_problem(x, dy, dc, stride=1, padding="same", dilation=1, in_coff=0, dy_view=None, want_bias=True, add=None,
                   out=None):
    """The checks of one weight-gradient problem (dtypes and shapes first: they need no device) -> (descriptor, (dkernel,
    dbias or None), (flops, bytes, shape))"""
    what = "conv2d_wgrad"
    _grad_tensor(what, "x", x)
    if x.dim() != 4:
        raise ValueError(f"{what}: `x` must be [B, H, W, C], got {tuple(x.shape)}")
    p = dc.p
    vcs, vbs = (None, 0) if dy_view is None else (int(dy_view[2]), int(dy_view[3]))
    g = conv2d_wgrad_geometry(x.shape, p, stride, padding, dilation, in_coff, vcs, vbs)
    d = g.conv
    vt, elem_off, vcs, vbs = _dy_view(what, dy, dy_view, d.B, d.Ho, d.Wo, p.cout)
    dk, db, add_k, add_b = _wgrad_outputs(what, x.device, (p.KH, p.KW, p.span, p.cout), (p.cout,), want_bias, add, out)
    _require_dev(x, "x")
    _require_dev(vt, "dy")
    d.in_, d.out = x.data_ptr(), vt.data_ptr() + 4 * elem_off
    g.dkernel, g.dbias = dk.data_ptr(), None if db is None else db.data_ptr()
    g.add_kernel = None if add_k is None else add_k.data_ptr()
    g.add_bias = None if add_b is None or db is None else add_b.data_ptr()
    M = d.B * d.Ho * d.Wo
    flops = 2.0 * M * p.KH * p.KW * p.span * p.cout
    nbytes = 4 * (d.B * d.H * d.W * p.span + M * p.cout + dk.numel() * (2 if add_k is not None else 1))
    shape = f"M={p.span} N={p.cout} K={M} k{p.KH}x{p.KW} s{stride} d{dilation} HxW={d.H}x{d.W}"
    return g, (dk, db), (flops, nbytes, shape)


def conv2d_wgrad(x, dy, dc, stride=1, padding="same", dilation=1, in_coff=0, dy_view=None, want_bias=True, add=None, out=None):
    """Weight and bias gradient of the dense conv `dc` (csrc/conv_grad.hip), float32: x [B,H,W,Cbuf] is the conv's input (read at
    channels in_coff : in_coff + cin), dy [B,Ho,Wo,cout] the gradient at its PRE-activation output -- or dy_view=(tensor,
    element offset, channel stride, batch stride), the forward's out_view (dy=None).  add / out: a kernel tensor or a (kernel,
    bias) pair; out = add + gradient with one float32 addition, in place if they are the same tensor.
    -> (dkernel [kh,kw,cin,cout], the Keras layout; dbias [cout], or None unless want_bias).  Exact fp32 products whatever
    set_conv_math says; a fixed summation order: two launches give the same bits, alone or in conv2d_wgrad_multi."""
    return conv2d_wgrad_multi([dict(x=x, dy=dy, dc=dc, stride=stride, padding=padding, dilation=dilation, in_coff=in_coff,
                                    dy_view=dy_view, want_bias=want_bias, add=add, out=out)])[0]


def conv2d_wgrad_multi(problems):
    """ml_conv2d_wgrad_multi_f32: several weight-gradient problems in one launch pair (the five un-shared pyramid levels of a
    tower depth).  problems: list of dicts with conv2d_wgrad's arguments -> list of (dkernel, dbias or None), the bits of the
    single calls."""
    if not problems:
        return []
    return _slice_sum_multi("conv_wgrad", [_wgrad_problem(**pr) for pr in problems], problems[0]["x"].device,
                            _lib.CONV_WGRAD_MAX_PROBLEMS, _lib.ConvWgradDesc, "ml_conv2d_wgrad_plan", "ml_conv2d_wgrad_multi_f32")


def _in_hw(what, in_hw, B_default):
    """in_hw = (H, W) of a conv's input, or its shape (B, H, W[, C]) -> (B, or B_default where in_hw has none, H, W)"""
    hw = tuple(int(v) for v in in_hw)
    if len(hw) not in (2, 3, 4):
        raise ValueError(f"{what}: in_hw is (H, W) or the input's shape (B, H, W[, C]), got {hw}")
    return (B_default, *hw) if len(hw) == 2 else hw[:3]


def _dgrad_problem(dy, dc, in_hw, stride=1, padding="same", dilation=1, dy_view=None, add=None, out=None):
    """One data-gradient problem -> the conv2d problem (a dict of conv2d's arguments) that computes it"""
    what = "conv2d_dgrad"
    p = dc.p
    _dense_only(what, p)
    B, H, W = _in_hw(what, in_hw, None)
    pads = dgrad_padding(H, W, p.kh_real, p.kw_real, stride, dilation, padding)        # refuses stride 2 by name
    Ho, Wo, _, _ = resolve_padding(H, W, p.kh_real, p.kw_real, stride, dilation, padding)
    vt0 = dy if dy_view is None else dy_view[0]
    if not isinstance(vt0, torch.Tensor):
        raise ValueError(f"{what}: `dy` must be a tensor")
    if B is None:
        B = int(vt0.shape[0])                                # (H, W) alone: dy, or the viewed tensor, is batch-major
    vt, elem_off, vcs, vbs = _dy_view(what, dy, dy_view, B, Ho, Wo, p.cout)
    shape = (B, H, W, p.span)
    for name, t in (("add", add), ("out", out)):
        if t is not None:
            _grad_tensor(what, name, t, shape)
    if out is not None and add is not None and (out is add or out.data_ptr() == add.data_ptr()):
        raise ValueError(f"{what}: `out` may not be `add` (a launch cut along K adds the residual after other blocks have "
                         f"written: aliasing is not safe to assume)")
    _require_dev(vt, "dy")
    if dy_view is not None or p.cout % 4:
        # the forward kernels read 16-byte rows: a contiguous copy with zero pad channels (the transposed weights have zero rows
        # there); from the caching allocator, every element written
        cp = -(-p.cout // 4) * 4
        dense = torch.empty((B, Ho, Wo, cp), dtype=torch.float32, device=vt.device)
        _lib.check(_lib.load().ml_conv2d_grad_gather_dy_f32(C.c_void_p(vt.data_ptr() + 4 * elem_off), _ptr(dense), B, Ho * Wo,
                                                            p.cout, vcs, vbs, _stream()), "ml_conv2d_grad_gather_dy_f32")
        vt = dense
    return dict(x=vt, dc=dc.dgrad, stride=1, padding=pads, dilation=dilation, act=_lib.ACT_NONE, residual=add, out=out)


def conv2d_dgrad(dy, dc, in_hw, stride=1, padding="same", dilation=1, dy_view=None, add=None, out=None):
    """Data gradient of the dense conv `dc` at stride 1, float32: the FORWARD kernels (generic, persistent 1x1, Winograd -- under
    whatever set_conv_math is set) on the transposed weights dc.dgrad: dx = conv(dy, kernel rotated by 180 degrees with cin /
    cout swapped) under the padding (K-1) d - pad.  dy [B,Ho,Wo,cout] at the conv's PRE-activation output, or dy_view as in
    conv2d_wgrad; in_hw = (H, W) of the conv's input, or its shape (B, H, W[, C]) -- needed where a viewed tensor's first
    axis is not the batch.  add: dx = add + gradient (the forward's residual); `out` may not be
    `add`.  -> dx [B,H,W,cin].  Stride 2 raises NotImplementedError."""
    pr = _dgrad_problem(dy, dc, in_hw, stride, padding, dilation, dy_view, add, out)
    return conv2d(pr.pop("x"), pr.pop("dc"), **pr)


def conv2d_dgrad_multi(problems):
    """Several data-gradient problems as ONE conv2d_multi launch.  problems: list of dicts with conv2d_dgrad's arguments."""
    return conv2d_multi([_dgrad_problem(**pr) for pr in problems])


def _dgrad_s2_desc(what, p, in_hw, padding="same", dilation=1, B_default=1):
    """The ml_conv2d_desc of a stride-2 data-gradient problem without its tensors: the FORWARD problem's geometry."""
    _dense_only(what, p)
    B, H, W = _in_hw(what, in_hw, B_default)
    Ho, Wo, pt, pl = resolve_padding(H, W, p.kh_real, p.kw_real, 2, dilation, padding)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"{what}: the kernel does not fit the {H} x {W} input")
    d = _lib.ConvDesc()
    d.B, d.H, d.W, d.in_cstride, d.in_coff = B, H, W, p.span, 0
    d.span, d.span_pad, d.cpp_shift = p.span, p.span_pad, p.cpp_shift
    d.Ho, d.Wo = Ho, Wo
    d.KH, d.KW, d.stride, d.dil, d.pad_t, d.pad_l = p.KH, p.KW, 2, dilation, pt, pl
    d.cout, d.n_pad = p.cout, p.n_pad
    d.out_cstride, d.out_coff, d.out_bstride = p.cout, 0, 0
    d.group_cin_step, d.shuffle2x2, d.math = p.group_cin_step, p.shuffle2x2, _lib.MATH_F32
    return d


def conv2d_dgrad_s2_classes(p, in_hw, padding="same", dilation=1):
    """The four parity classes of a stride-2 data-gradient problem (ml_conv2d_dgrad_s2_classes, host only).  p: the forward's
    PackedConv; in_hw = (H, W) (one image) or (B, H, W[, C]).  -> list over class c = 2 (iy & 1) + (ix & 1) of
    (pixels, [(ky, kx, off_y, off_x) per live tap, ascending]): input pixel (iy, ix) of the class reads dy at
    ((iy >> 1) + off_y, (ix >> 1) + off_x) for that tap."""
    d = _dgrad_s2_desc("conv2d_dgrad_s2", p, in_hw, padding, dilation)
    pixels, ntaps = (C.c_int64 * 4)(), (C.c_int32 * 4)()
    taps = (C.c_int32 * (4 * _lib.CONV_DGRAD_S2_MAX_TAPS * 4))()
    _lib.check(_lib.load().ml_conv2d_dgrad_s2_classes(C.byref(d), pixels, ntaps, taps), "ml_conv2d_dgrad_s2_classes")
    out = []
    for c in range(4):
        base = c * _lib.CONV_DGRAD_S2_MAX_TAPS * 4
        out.append((int(pixels[c]), [tuple(taps[base + 4 * t: base + 4 * t + 4]) for t in range(ntaps[c])]))
    return out


def conv2d_dgrad_s2(dy, dc, in_hw, padding="same", dilation=1, add=None, out=None):
    """Data gradient of the dense conv `dc` at STRIDE 2 (csrc/conv_grad.hip, ml_conv2d_dgrad_s2_f32), float32: dy [B,Ho,Wo,cout]
    dense, at the conv's PRE-activation output; in_hw = (H, W) of the conv's input or its shape (B, H, W[, C]).  Reads the
    Keras-layout kernel dc.keras_kernel (the bound master where there is one).  add / out: out = add + gradient with one
    float32 addition; `out` may be `add` (in place).  -> dx [B,H,W,cin]; every element written by the launch, pixels no tap
    reaches get add or +0.0.  Exact fp32 products whatever set_conv_math says; a fixed summation order (live taps ascending,
    cout ascending): two launches give the same bits."""
    what = "conv2d_dgrad_s2"
    p = dc.p
    _grad_tensor(what, "dy", dy)
    if dy.dim() != 4:
        raise ValueError(f"{what}: `dy` must be [B, Ho, Wo, cout], got {tuple(dy.shape)}")
    d = _dgrad_s2_desc(what, p, in_hw, padding, dilation, B_default=int(dy.shape[0]))
    _grad_tensor(what, "dy", dy, (d.B, d.Ho, d.Wo, p.cout))
    if not dy.is_contiguous():
        raise ValueError(f"{what}: `dy` must be contiguous (a dense tensor, not a view)")
    if p.span % 4 or p.cout % 4:
        raise ValueError(f"{what}: cin ({p.span}) and cout ({p.cout}) must each be a multiple of 4 (16-byte accesses)")
    dx = _grad_out(what, (d.B, d.H, d.W, p.span), dy.device, add, out)
    if not dx.is_contiguous() or (add is not None and not add.is_contiguous()):
        raise ValueError(f"{what}: `out` and `add` must be contiguous")
    _require_dev(dy, "dy")
    w = dc.keras_kernel
    d.out, d.wgt = dy.data_ptr(), w.data_ptr()
    M = d.B * d.Ho * d.Wo
    flops = 2.0 * M * p.KH * p.KW * p.span * p.cout
    nbytes = 4 * (dy.numel() + w.numel() + dx.numel() * (2 if add is not None else 1))
    with _Prof("conv_dgrad_s2", flops, nbytes, f"M={p.span} N={d.B * d.H * d.W} K={p.KH * p.KW * p.cout} k{p.KH}x{p.KW} s2 "
               f"d{dilation} HxW={d.H}x{d.W}"):
        _lib.check(_lib.load().ml_conv2d_dgrad_s2_f32(C.byref(d), _ptr(dx), _ptr(add), _stream()), "ml_conv2d_dgrad_s2_f32")
    return dx


# ------------------------------------------------------------------ depthwise 3x3, backward (csrc/dwconv_grad.hip)
def _dw_stride(what, stride, kernel_size=(3, 3)):
    if tuple(int(v) for v in kernel_size) != (3, 3):
        raise ValueError(f"{what}: kernel {tuple(kernel_size)}: 3 x 3 depthwise kernels only")
    if stride not in (1, 2):
        raise ValueError(f"{what}: stride {stride}: 1 or 2")


def _dw_slice(what, name, Cbuf, coff, C):
    if C < 1 or C % 4:
        raise ValueError(f"{what}: the channel count ({C}) must be a multiple of 4 (16-byte accesses)")
    if Cbuf % 4 or coff % 4:
        raise ValueError(f"{what}: {name}'s channel count ({Cbuf}) and the offset ({coff}) must each be a multiple of 4 "
                         f"(16-byte accesses)")
    if coff < 0 or coff + C > Cbuf:
        raise ValueError(f"{what}: {name} has {Cbuf} channels, the kernel needs [{coff}, {coff + C})")


def dwconv3x3_wgrad_geometry(x_shape, C=None, stride=1, padding="same", dilation=1, in_coff=0, dy_cstride=None, dy_coff=0,
                             kernel_size=(3, 3)):
    """The ml_dwconv3x3_grad_desc of a weight-gradient problem without its tensors: geometry only (what
    ml_dwconv3x3_wgrad_plan reads).  x_shape [B,H,W,Cbuf]; C=None: the channels of x from in_coff on."""
    what = "dwconv3x3_wgrad"
    _dw_stride(what, stride, kernel_size)
    B, H, W, Cbuf = (int(v) for v in x_shape)
    C = Cbuf - in_coff if C is None else int(C)
    dy_cs = C if dy_cstride is None else int(dy_cstride)
    _dw_slice(what, "x", Cbuf, in_coff, C)
    _dw_slice(what, "dy", dy_cs, dy_coff, C)
    Ho, Wo, pt, pl = resolve_padding(H, W, 3, 3, stride, dilation, padding)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"{what}: the kernel does not fit the {H} x {W} input")
    d = _lib.DwGradDesc()
    d.B, d.H, d.W, d.C, d.in_cstride, d.in_coff = B, H, W, C, Cbuf, in_coff
    d.Ho, d.Wo, d.dy_cstride, d.dy_coff = Ho, Wo, dy_cs, dy_coff
    d.stride, d.dil, d.pad_t, d.pad_l = stride, dilation, pt, pl
    return d


def dwconv3x3_wgrad_plan(x_shape, **geometry):
    """-> (slices, pixels per slice, bytes of the partials) of one depthwise weight-gradient problem:
    ml_dwconv3x3_wgrad_plan, host only.  A function of the problem's geometry alone."""
    return _slice_plan("ml_dwconv3x3_wgrad_plan", dwconv3x3_wgrad_geometry(x_shape, **geometry))


def _dw_wgrad_problem(x, dy, stride=1, padding="same", dilation=1, in_coff=0, dy_coff=0, want_bias=True, add=None, out=None,
                      C=None, kernel_size=(3, 3)):
    """The checks of one depthwise weight-gradient problem (dtypes and shapes first: they need no device)
    -> (descriptor, (dkernel, dbias or None), (flops, bytes, shape))"""
    what = "dwconv3x3_wgrad"
    _grad_tensor(what, "x", x)
    _grad_tensor(what, "dy", dy)
    if x.dim() != 4 or dy.dim() != 4:
        raise ValueError(f"{what}: `x` and `dy` must be [B, H, W, C], got {tuple(x.shape)} and {tuple(dy.shape)}")
    Cc = min(int(x.shape[3]) - in_coff, int(dy.shape[3]) - dy_coff) if C is None else int(C)
    d = dwconv3x3_wgrad_geometry(x.shape, Cc, stride, padding, dilation, in_coff, int(dy.shape[3]), dy_coff, kernel_size)
    if tuple(dy.shape[:3]) != (d.B, d.Ho, d.Wo):
        raise ValueError(f"{what}: `dy` is {tuple(dy.shape)}, expected {(d.B, d.Ho, d.Wo)} pixels")
    dk, db, add_k, add_b = _wgrad_outputs(what, x.device, (3, 3, Cc, 1), (Cc,), want_bias, add, out)
    _require_dev(x, "x")
    _require_dev(dy, "dy")
    d.x, d.dy = x.data_ptr(), dy.data_ptr()
    d.dkernel, d.dbias = dk.data_ptr(), None if db is None else db.data_ptr()
    d.add_kernel = None if add_k is None else add_k.data_ptr()
    d.add_bias = None if add_b is None or db is None else add_b.data_ptr()
    M = d.B * d.Ho * d.Wo
    nbytes = 4 * (d.B * d.H * d.W * Cc + M * Cc + 9 * Cc * (2 if add_k is not None else 1) +
                  (0 if db is None else Cc * (2 if add_b is not None else 1)))
    return d, (dk, db), (18.0 * M * Cc, nbytes, f"C={Cc} K={M} s{stride} d{dilation} HxW={d.H}x{d.W}")


def dwconv3x3_wgrad(x, dy, stride=1, padding="same", dilation=1, in_coff=0, dy_coff=0, want_bias=True, add=None, out=None,
                    C=None, workspace_bytes=None):
    """Weight and bias gradient of the depthwise 3x3 conv (csrc/dwconv_grad.hip), float32: x [B,H,W,Cbuf] is the conv's input,
    read at channels in_coff : in_coff + C; dy [B,Ho,Wo,Cdy] the gradient at its PRE-activation output, read at channels
    dy_coff : dy_coff + C (C=None: as many as both buffers hold from their offsets).  add / out: a kernel tensor or a
    (kernel, bias) pair; out = add + gradient with one float32 addition, in place if they are the same tensor.
    -> (dkernel [3,3,C,1], the Keras layout; dbias [C], or None unless want_bias).  A fixed summation order: two launches give
    the same bits, alone or in dwconv3x3_wgrad_multi.  workspace_bytes: None, or the size to give the launch (tests)."""
    return dwconv3x3_wgrad_multi([dict(x=x, dy=dy, stride=stride, padding=padding, dilation=dilation, in_coff=in_coff,
                                       dy_coff=dy_coff, want_bias=want_bias, add=add, out=out, C=C)],
                                 workspace_bytes=workspace_bytes)[0]


def dwconv3x3_wgrad_multi(problems, workspace_bytes=None):
    """ml_dwconv3x3_wgrad_multi_f32: up to 8 depthwise weight-gradient problems in one launch pair (the three dilations of
    the ASPP ride together; more go in several launches).  problems: list of dicts with dwconv3x3_wgrad's arguments
    -> list of (dkernel, dbias or None), the bits of the single calls."""
    if not problems:
        return []
    return _slice_sum_multi("dwconv3x3_wgrad", [_dw_wgrad_problem(**pr) for pr in problems], problems[0]["x"].device,
                            _lib.DWCONV_GRAD_MAX_PROBLEMS, _lib.DwGradDesc, "ml_dwconv3x3_wgrad_plan",
                            "ml_dwconv3x3_wgrad_multi_f32", (), workspace_bytes)


def _dw_dgrad_problem(dy, wgt, in_hw, stride=1, padding="same", dilation=1, dy_coff=0, C=None, add=None, out=None,
                      kernel_size=(3, 3)):
    what = "dwconv3x3_dgrad"
    _grad_tensor(what, "dy", dy)
    _grad_tensor(what, "wgt", wgt)
    _dw_stride(what, stride, kernel_size)
    if dy.dim() != 4:
        raise ValueError(f"{what}: `dy` must be [B, Ho, Wo, C], got {tuple(dy.shape)}")
    B, Cdy = int(dy.shape[0]), int(dy.shape[3])
    B_in, H, W = _in_hw(what, in_hw, B)
    Cc = Cdy - dy_coff if C is None else int(C)
    _dw_slice(what, "dy", Cdy, dy_coff, Cc)
    if wgt.dim() != 2 or tuple(wgt.shape) != (9, Cc):
        raise ValueError(f"{what}: `wgt` is {tuple(wgt.shape)}, expected {(9, Cc)} (packing.pack_depthwise of a 3 x 3 kernel)")
    Ho, Wo, pt, pl = resolve_padding(H, W, 3, 3, stride, dilation, padding)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"{what}: the kernel does not fit the {H} x {W} input")
    if tuple(dy.shape[:3]) != (B, Ho, Wo) or B_in != B:
        raise ValueError(f"{what}: `dy` is {tuple(dy.shape)}, expected {(B, Ho, Wo)} pixels for a {H} x {W} input")
    dx = _grad_out(what, (B, H, W, Cc), dy.device, add, out)
    _require_dev(dy, "dy")
    _require_dev(wgt, "wgt")
    d = _lib.DwGradDesc()
    d.B, d.H, d.W, d.C, d.in_cstride, d.in_coff = B, H, W, Cc, Cc, 0
    d.Ho, d.Wo, d.dy_cstride, d.dy_coff = Ho, Wo, Cdy, dy_coff
    d.stride, d.dil, d.pad_t, d.pad_l = stride, dilation, pt, pl
    d.dy, d.wgt, d.dx = dy.data_ptr(), wgt.data_ptr(), dx.data_ptr()
    d.add_x = None if add is None else add.data_ptr()
    nbytes = 4 * (B * Ho * Wo * Cc + 9 * Cc + dx.numel() * (2 if add is not None else 1))
    return d, dx, (18.0 * B * Ho * Wo * Cc, nbytes, f"C={Cc} s{stride} d{dilation} HxW={H}x{W}")


def dwconv3x3_dgrad(dy, wgt, in_hw, stride=1, padding="same", dilation=1, dy_coff=0, C=None, add=None, out=None):
    """Data gradient of the depthwise 3x3 conv (csrc/dwconv_grad.hip), float32, stride 1 or 2: dy [B,Ho,Wo,Cdy] at the conv's
    PRE-activation output, read at channels dy_coff : dy_coff + C (C=None: all from dy_coff); wgt: the forward's [9][C]
    (packing.pack_depthwise); in_hw = (H, W) of the conv's input, or its shape.  add / out: out = add + gradient with one
    float32 addition, in place if they are the same tensor.  -> dx [B,H,W,C]."""
    return dwconv3x3_dgrad_multi([dict(dy=dy, wgt=wgt, in_hw=in_hw, stride=stride, padding=padding, dilation=dilation,
                                       dy_coff=dy_coff, C=C, add=add, out=out)])[0]


def dwconv3x3_dgrad_multi(problems):
    """ml_dwconv3x3_dgrad_multi_f32: up to 8 data-gradient problems in one launch, each into a dx of its own (gradients that
    add into ONE tensor are chained through add= in separate launches).  -> list of dx, the bits of the single calls."""
    n = len(problems)
    if n == 0:
        return []
    if n > _lib.DWCONV_GRAD_MAX_PROBLEMS:
        return (dwconv3x3_dgrad_multi(problems[:_lib.DWCONV_GRAD_MAX_PROBLEMS]) +
                dwconv3x3_dgrad_multi(problems[_lib.DWCONV_GRAD_MAX_PROBLEMS:]))
    made = [_dw_dgrad_problem(**pr) for pr in problems]
    arr = (_lib.DwGradDesc * n)()
    flops, nbytes = 0.0, 0.0
    for i, (d, _, (f, nb, _)) in enumerate(made):
        arr[i] = d
        flops += f
        nbytes += nb
    with _Prof("dwconv3x3_dgrad", flops, nbytes, made[0][2][2] if n == 1 else "multi x%d" % n):
        _lib.check(_lib.load().ml_dwconv3x3_dgrad_multi_f32(arr, n, _stream()), "ml_dwconv3x3_dgrad_multi_f32")
    return [dx for _, dx, _ in made]


def gather_channels(src, coff, out):
    """ml_conv2d_grad_gather_dy_f32 on a channel slice: channels coff : coff + C of src [B,H,W,Cs] -> out [B,H,W,C], dense
    (C % 4 == 0), float32: a slice of a concat buffer's gradient in the form GroupNormalization's backward reads."""
    what = "gather_channels"
    _grad_tensor(what, "src", src)
    _grad_tensor(what, "out", out)
    if src.dim() != 4 or out.dim() != 4 or tuple(out.shape[:3]) != tuple(src.shape[:3]):
        raise ValueError(f"{what}: `src` {tuple(src.shape)} and `out` {tuple(out.shape)} must be [B, H, W, C] of the same pixels")
    B, H, W, Cs = src.shape
    Cc = int(out.shape[3])
    if Cc % 4 or coff < 0 or coff + Cc > Cs:
        raise ValueError(f"{what}: channels {coff} : {coff + Cc} of {Cs}: a slice of a multiple of 4 channels")
    _require_dev(src, "src")
    _require_dev(out, "out")
    with _Prof("gather_channels", 0, 8.0 * out.numel()):
        _lib.check(_lib.load().ml_conv2d_grad_gather_dy_f32(C.c_void_p(src.data_ptr() + 4 * coff), _ptr(out), B, H * W, Cc, Cs, 0,
                                                            _stream()), "ml_conv2d_grad_gather_dy_f32")
    return out


def relu_grad(y, dy, out=None):
    """ml_relu_grad_f32: the gradient in front of a ReLU whose OUTPUT is y, float32: dy where y > 0, else 0 (a conv + ReLU
    with no GroupNormalization behind it to carry the mask: the ASPP's pooled branch).  out: None, or dy (in place)."""
    what = "relu_grad"
    _grad_tensor(what, "y", y)
    _grad_tensor(what, "dy", dy, y.shape)
    if out is not None:
        _grad_tensor(what, "out", out, y.shape)
    for name, t in (("y", y), ("dy", dy), ("out", out)):
        if t is not None:
            _require_dev(t, name)
    out = torch.empty_like(dy) if out is None else out
    with _Prof("relu_grad", 0, 12.0 * y.numel()):
        _lib.check(_lib.load().ml_relu_grad_f32(_ptr(y), _ptr(dy), _ptr(out), y.numel(), _stream()), "ml_relu_grad_f32")
    return out


def scale_channels_(x, s):
    lib = _lib.load()
    if x.dtype != torch.float32 or s.dtype != torch.float32:
        raise NotImplementedError("scale_channels_: float32 tensors only (SqueezeExcite is not built for fp16 storage)")
    B, H, W, Cc = x.shape
    _lib.check(lib.ml_scale_channels_f32(_ptr(x), _ptr(s), B, H * W, Cc, _stream()), "ml_scale_channels_f32")
    return x


def squeeze_excite_multi(problems):
    """ml_squeeze_excite_f32 / _f16: whole SqueezeExcites (reference engine/layers/misc.py:24-54) of several problems in ONE
    launch pair.  problems: dicts x (contiguous NHWC fp32 or fp16, one dtype per call), w1 fp32 [C, Hd], w2 fp32 [Hd, C]
    (device), out=None (None: in place into x) and live=None ((device int32 [1], slots per image): a fixed-capacity
    RoI batch whose dead samples are neither read nor written).  -> list of outputs."""
    lib = _lib.load()
    n = len(problems)
    if n == 0:
        return []
    if n > _lib.SE_MAX_PROBLEMS:
        return squeeze_excite_multi(problems[:_lib.SE_MAX_PROBLEMS]) + squeeze_excite_multi(problems[_lib.SE_MAX_PROBLEMS:])
    arr = (_lib.SeDesc * n)()
    outs, nbytes, ws_bytes = [], 0.0, 0
    half = problems[0]["x"].dtype == torch.float16
    for i, pr in enumerate(problems):
        x, w1, w2 = pr["x"], pr["w1"], pr["w2"]
        _require_dev(x, "x")
        _require_dev(w1, "w1")
        _require_dev(w2, "w2")
        if x.dtype not in (torch.float32, torch.float16) or (x.dtype == torch.float16) != half:
            raise ValueError("squeeze_excite: x must be float32 or float16, one dtype per call")
        out = pr.get("out")
        if out is None:
            out = x
        else:
            _require_dev(out, "out")
            if out.shape != x.shape or out.dtype != x.dtype:
                raise ValueError("squeeze_excite: out must match x")
        B, Cc = int(x.shape[0]), int(x.shape[-1])
        HW = x.numel() // (B * Cc)
        if w1.dtype != torch.float32 or w2.dtype != torch.float32 or w1.dim() != 2 or w1.shape[0] != Cc or \
                tuple(w2.shape) != (w1.shape[1], Cc):
            raise ValueError("squeeze_excite: w1 must be fp32 [C, Hd] and w2 fp32 [Hd, C]")
        d = arr[i]
        d.x, d.out, d.w1, d.w2 = x.data_ptr(), out.data_ptr(), w1.data_ptr(), w2.data_ptr()
        d.B, d.HW, d.C, d.Hd = B, HW, Cc, int(w1.shape[1])
        if pr.get("live") is not None:
            lv, period = pr["live"]
            _require_dev(lv, "live")
            d.live, d.live_period = lv.data_ptr(), int(period)
        d.ws_offset = ws_bytes
        ws_bytes += (int(lib.ml_squeeze_excite_workspace_bytes(B, HW, Cc)) + 255) // 256 * 256
        nbytes += 3 * x.element_size() * x.numel()          # x read twice (pool, scale), out written once
        outs.append(out)
    ws = workspace(ws_bytes, problems[0]["x"].device, "se")
    fn = lib.ml_squeeze_excite_f16 if half else lib.ml_squeeze_excite_f32
    sfx = "_h" if half else ""
    # the two kernels are enqueued by ONE library call: the pool record's events bracket both, the scale record counts
    # the second launch (no time, no bytes of its own)
    with _Prof("squeeze_excite_pool" + sfx, 0, nbytes, f"multi x{n} (pool + scale timed together)") as prof:
        _lib.check(fn(arr, n, _ptr(ws), ws.numel(), _stream()), "ml_squeeze_excite")
    if prof.on:
        PROFILE.append({"kernel": "squeeze_excite_scale" + sfx, "flops": 0.0, "bytes": 0.0,
                        "shape": "timed with squeeze_excite_pool" + sfx, "start": prof.rec["end"], "end": prof.rec["end"]})
    return outs


def _se_res_check(t, name, like=None, op="se_residual"):
    _require_dev(t, name)
    if t.dtype != torch.float32:
        raise ValueError(f"{op}: `{name}` must be float32")
    if like is not None and tuple(t.shape) != tuple(like):
        raise ValueError(f"{op}: `{name}` has shape {tuple(t.shape)}, expected {tuple(like)}")


def se_residual(x, shortcut, w1, b1, w2, b2, scale, shift, want_y=False):
    """ml_se_residual_f32 (GATE): the tail of an SE-ResNet pre-activation basic block in one launch pair --
    g = sigmoid(w2^T relu(w1^T mean_hw(x) + b1) + b2), y = x * g + shortcut, act = relu(y * scale + shift).
    x / shortcut: fp32 NHWC [B,H,W,C]; w1 [C, Hd], b1 [Hd], w2 [Hd, C], b2 [C], scale / shift [C] (device fp32).
    -> (act, y if want_y else None).  Scratch from ops.workspace (graph-safe: grow-only, keyed by stream)."""
    lib = _lib.load()
    _se_res_check(x, "x")
    shape = tuple(x.shape)
    B, Cc = int(shape[0]), int(shape[-1])
    HW = x.numel() // max(1, B * Cc)
    _se_res_check(shortcut, "shortcut", shape)
    if w1.dim() != 2 or w1.shape[0] != Cc:
        raise ValueError("se_residual: w1 must be [C, Hd]")
    Hd = int(w1.shape[1])
    for t, name, want in ((w1, "w1", (Cc, Hd)), (b1, "b1", (Hd,)), (w2, "w2", (Hd, Cc)), (b2, "b2", (Cc,)),
                          (scale, "scale", (Cc,)), (shift, "shift", (Cc,))):
        _se_res_check(t, name, want)
    act = torch.empty_like(x)
    y = torch.empty_like(x) if want_y else None
    d = _lib.SeResidualDesc()
    d.x, d.shortcut, d.w1, d.b1, d.w2, d.b2 = (x.data_ptr(), shortcut.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                               w2.data_ptr(), b2.data_ptr())
    d.scale, d.shift, d.out_act = scale.data_ptr(), shift.data_ptr(), act.data_ptr()
    d.out_y = y.data_ptr() if y is not None else None
    d.B, d.HW, d.C, d.Hd, d.mode = B, HW, Cc, Hd, _lib.SE_RES_GATE
    ws = workspace(max(16, int(lib.ml_se_residual_workspace_bytes(B, HW, Cc))), x.device, "se_residual")
    nbytes = 4.0 * x.numel() * (4 + int(want_y))            # x read twice (pool, tail), shortcut once, act (+ y) written
    with _Prof("se_residual", 0, nbytes, f"B={B} HW={HW} C={Cc} Hd={Hd}{' +y' if want_y else ''}"):
        _lib.check(lib.ml_se_residual_f32(C.byref(d), _ptr(ws), ws.numel(), _stream()), "ml_se_residual_f32")
    return act, y


def se_bottleneck(c3, residual, w1, b1, w2, b2, out=None):
    """ml_se_bottleneck_f32 / _f16: the tail of an SE-ResNet-50 / SE-ResNeXt-50 bottleneck unit in three launches --
    g = sigmoid(w2^T relu(w1^T mean_hw(c3) + b1) + b2) once per sample, out = relu(c3 * g + residual).
    c3 / residual: contiguous NHWC [B,H,W,C], both float32 or both float16 (fp32 arithmetic, one rounding at the store);
    w1 [C, Hd], b1 [Hd], w2 [Hd, C], b2 [C] device fp32.  `out` (same shape and dtype) may be c3 itself; else allocated.
    Scratch from ops.workspace (graph-safe: grow-only, keyed by stream)."""
    lib = _lib.load()
    _require_dev(c3, "c3")
    _require_dev(residual, "residual")
    if c3.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"se_bottleneck: c3 must be float32 or float16, got {c3.dtype}")
    shape = tuple(c3.shape)
    if residual.dtype != c3.dtype or tuple(residual.shape) != shape:
        raise ValueError(f"se_bottleneck: residual {tuple(residual.shape)} / {residual.dtype} does not match c3 "
                         f"{shape} / {c3.dtype}")
    B, Cc = int(shape[0]), int(shape[-1])
    HW = c3.numel() // max(1, B * Cc)
    if w1.dim() != 2 or w1.shape[0] != Cc:
        raise ValueError("se_bottleneck: w1 must be [C, Hd]")
    Hd = int(w1.shape[1])
    for t, name, want in ((w1, "w1", (Cc, Hd)), (b1, "b1", (Hd,)), (w2, "w2", (Hd, Cc)), (b2, "b2", (Cc,))):
        _se_res_check(t, name, want, "se_bottleneck")
    if out is None:
        out = torch.empty_like(c3)
    else:
        _require_dev(out, "out")
        if out.dtype != c3.dtype or tuple(out.shape) != shape:
            raise ValueError("se_bottleneck: out must have c3's shape and dtype")
    d = _lib.SeBottleneckDesc()
    d.c3, d.residual, d.out = c3.data_ptr(), residual.data_ptr(), out.data_ptr()
    d.w1, d.b1, d.w2, d.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    d.B, d.HW, d.C, d.Hd = B, HW, Cc, Hd
    half = c3.dtype == torch.float16
    ws = workspace(max(16, int(lib.ml_se_bottleneck_workspace_bytes(B, HW, Cc))), c3.device, "se_bottleneck")
    nbytes = c3.element_size() * 4.0 * c3.numel()           # c3 read twice (pool, tail), residual once, out written once
    with _Prof("se_bottleneck_h" if half else "se_bottleneck", 0, nbytes, f"B={B} HW={HW} C={Cc} Hd={Hd}"):
        fn = lib.ml_se_bottleneck_f16 if half else lib.ml_se_bottleneck_f32
        _lib.check(fn(C.byref(d), _ptr(ws), ws.numel(), _stream()), "ml_se_bottleneck")
    return out


def bn_relu(x, scale, shift):
    """ml_se_residual_f32 (BN_RELU): relu(x * scale + shift) per channel, fp32 NHWC (a folded inference BatchNorm)."""
    lib = _lib.load()
    _se_res_check(x, "x")
    Cc = int(x.shape[-1])
    B = int(x.shape[0])
    _se_res_check(scale, "scale", (Cc,))
    _se_res_check(shift, "shift", (Cc,))
    out = torch.empty_like(x)
    d = _lib.SeResidualDesc()
    d.x, d.scale, d.shift, d.out_act = x.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr()
    d.B, d.HW, d.C, d.mode = B, x.numel() // max(1, B * Cc), Cc, _lib.SE_RES_BN_RELU
    with _Prof("bn_relu", 0, 8.0 * x.numel(), f"B={B} C={Cc}"):
        _lib.check(lib.ml_se_residual_f32(C.byref(d), None, 0, _stream()), "ml_se_residual_f32")
    return out


# How ResNet-50's four projection units (the first block of each stage) run: "on" = one GEMM over the concatenated K of the
# block's 3x3 output and its input (conv1x1_dual; conv maths "f32" and "f16s" only), "off" = the shortcut conv, then the
# 2c conv with the shortcut as its residual.  No other backbone reads it.  "on" is the default because the whole forward at
# 8 x 1024^2 measured faster with it by more than the spread in both maths (scripts/resnet50_timing.py).
PROJECTION_FUSION = "on"


def set_projection_fusion(mode):
    global PROJECTION_FUSION
    if mode not in ("on", "off"):
        raise ValueError(f"projection fusion must be 'on' or 'off', got {mode!r}")
    PROJECTION_FUSION = mode


def projection_fused():
    """True when a ResNet-50 projection unit launched now takes the one-GEMM kernel."""
    return PROJECTION_FUSION == "on" and CONV_MATH in ("f32", "f16s")


class DeviceDualConv:
    """The two 1x1 convs of a projection unit -- `dc_a` on the 3x3 output (its BN folded, no activation), `dc_x` the
    shortcut on the block input at `stride` -- and their one-GEMM operand: wgt [N][Ka + Kx] (row n = Wa[:, n] then
    Wx[:, n]) with bias = the sum of the two folded biases, made here once from the folded Keras kernels [1,1,K,N].
    `dc_a` / `dc_x`: the two convs' packings where the caller already holds them (a layer pair), else made here."""

    def __init__(self, ka, ba, kx, bx, device, dc_a=None, dc_x=None):
        from .packing import pack_dense
        ka, kx = np.asarray(ka, np.float32), np.asarray(kx, np.float32)
        if ka.shape[:2] != (1, 1) or kx.shape[:2] != (1, 1) or ka.shape[3] != kx.shape[3]:
            raise ValueError(f"DeviceDualConv: two 1x1 kernels of one output width expected, got {ka.shape} and {kx.shape}")
        self.Ka, self.Kx, self.N = int(ka.shape[2]), int(kx.shape[2]), int(ka.shape[3])
        zero = np.zeros(self.N, np.float64)
        ba = zero if ba is None else np.asarray(ba, np.float64)
        bx = zero if bx is None else np.asarray(bx, np.float64)
        self.dc_a = dc_a if dc_a is not None else DeviceConv(pack_dense(ka, ba.astype(np.float32)), device)
        self.dc_x = dc_x if dc_x is not None else DeviceConv(pack_dense(kx, bx.astype(np.float32)), device)
        w = np.ascontiguousarray(np.concatenate([ka[0, 0].T, kx[0, 0].T], axis=1))              # [N][Ka + Kx]
        self.wgt = torch.from_numpy(w).to(device)
        self.bias = torch.from_numpy((ba + bx).astype(np.float32)).to(device)
        self._wgt_h = None

    @property
    def wgt_h(self):
        """The operand rounded to IEEE half (what the two convs' own half packings hold); made on first use."""
        if self._wgt_h is None:
            self._wgt_h = self.wgt.cpu().to(torch.float16).to(self.wgt.device)
        return self._wgt_h


def conv1x1_dual(a, x, packed: DeviceDualConv, stride_b=1):
    """ml_conv1x1_dual_f32 / _f16: relu(a @ Wa + x[:, ::s, ::s] @ Wx + bias) in ONE launch -- a [B,Ho,Wo,Ka] and
    x [B,H,W,Kx] contiguous NHWC, both float32 (exact fp32 products) or both float16 (fp16 MFMA, fp32 accumulate, one
    rounding at the store); s = stride_b in {1, 2}, Ho = (H - 1) // s + 1.  x is read in place at its stride.  Shapes the
    kernel does not take (ML_E_BADARG: a K that is no multiple of its chunk, N % 128, a tensor of 2 GiB) run as the two
    launches the unit is made of: the shortcut conv, then the conv on `a` with the shortcut as residual and ReLU."""
    lib = _lib.load()
    _require_dev(a, "a")
    _require_dev(x, "x")
    if a.dtype not in (torch.float32, torch.float16) or x.dtype != a.dtype:
        raise ValueError(f"conv1x1_dual: a and x must both be float32 or both float16, got {a.dtype} and {x.dtype}")
    if stride_b not in (1, 2):
        raise ValueError(f"conv1x1_dual: stride_b must be 1 or 2, got {stride_b}")
    B, H, W, Kx = x.shape
    Ho, Wo = (H - 1) // stride_b + 1, (W - 1) // stride_b + 1
    if tuple(a.shape) != (B, Ho, Wo, packed.Ka) or Kx != packed.Kx:
        raise ValueError(f"conv1x1_dual: a {tuple(a.shape)} / x {tuple(x.shape)} do not match the packed unit "
                         f"(Ka={packed.Ka}, Kx={packed.Kx}, stride {stride_b})")
    half = a.dtype == torch.float16
    out = torch.empty((B, Ho, Wo, packed.N), dtype=a.dtype, device=a.device)
    M, es = B * Ho * Wo, a.element_size()
    fn, w = (lib.ml_conv1x1_dual_f16, packed.wgt_h) if half else (lib.ml_conv1x1_dual_f32, packed.wgt)
    with _Prof("conv1x1_dual_h" if half else "conv1x1_dual", 2.0 * M * packed.N * (packed.Ka + Kx),
               es * (M * (packed.Ka + Kx) + M * packed.N + w.numel()),
               f"M={M} N={packed.N} Ka={packed.Ka} Kx={Kx} s{stride_b} HxW={H}x{W}") as prof:
        status = fn(_ptr(a), _ptr(x), _ptr(w), _ptr(packed.bias), _ptr(out), B, H, W, packed.Ka, Kx, packed.N, stride_b,
                    _stream())
        if status == -1:                     # ML_E_BADARG: not a shape of this kernel, nothing was launched
            prof.on = False
        else:
            _lib.check(status, "ml_conv1x1_dual")
    if status == -1:
        sc = conv2d(x, packed.dc_x, stride=stride_b, padding="valid")
        return conv2d(a, packed.dc_a, padding="valid", act=_lib.ACT_RELU, residual=sc)
    return out


def restore_boxes(loc_pred, priors_i32):
    lib = _lib.load()
    _require_dev(loc_pred, "loc_pred")
    B, A, _ = loc_pred.shape
    boxes = torch.empty((B, A, 4), dtype=torch.float32, device=loc_pred.device)
    _lib.check(lib.ml_restore_boxes_f32(_ptr(loc_pred), _ptr(priors_i32), _ptr(boxes), B, A, _stream()),
               "ml_restore_boxes_f32")
    return boxes


def detection_proposal(cls_pred, boxes, min_confidence, nms_iou, post_iou, max_out, want_kept=False,
                       want_payload=False):
    """Fixed-capacity DetectionProposal: -> proposed [B,max_out,6] (-1 padded), counts [B] int32
    (device), kept [B,max_out,2] int32 or None[, payload [B,max_out*6+1] -- the all-gather record the
    kernel writes beside `proposed`, see parallel.all_gather_detections]."""
    lib = _lib.load()
    _require_dev(cls_pred, "cls_pred")
    _require_dev(boxes, "boxes")
    B, A, Cn = cls_pred.shape
    dev = cls_pred.device
    proposed = torch.empty((B, max_out, 6), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    kept = torch.empty((B, max_out, 2), dtype=torch.int32, device=dev) if want_kept else None
    payload = torch.empty((B, max_out * 6 + 1), dtype=torch.float32, device=dev) if want_payload else None
    ws = workspace(lib.ml_detection_workspace_bytes(B, A, Cn, max_out), dev, "det")
    with _Prof("detection_proposal", 0, 4 * (cls_pred.numel() + boxes.numel())):
        _lib.check(lib.ml_detection_proposal_f32(_ptr(cls_pred), _ptr(boxes), _ptr(proposed), _ptr(counts), _ptr(kept),
                                                 _ptr(payload), B, A, Cn, float(min_confidence), float(nms_iou),
                                                 float(post_iou), int(max_out), _ptr(ws), _stream()),
                   "ml_detection_proposal_f32")
    if want_payload:
        return proposed, counts, kept, payload
    return proposed, counts, kept


def mask_distribute(rows, max_k, base_size, has_k=False, want_k=False):
    """rows [B,cap,6] (has_k=False: k computed per MaskDistribute) or [B,cap,7] dist_boxes
    (has_k=True).  -> level_slots [B,L,cap] int32, level_counts [B,L] int32, level_max [L] int32 (max over
    the images: the one thing the host reads), kvals [B,cap] or None."""
    lib = _lib.load()
    _require_dev(rows, "rows")
    B, cap, rs = rows.shape
    L = max_k + 1
    slots = torch.empty((B, L, cap), dtype=torch.int32, device=rows.device)
    lcounts = torch.empty((B, L), dtype=torch.int32, device=rows.device)
    lmax = torch.empty((L,), dtype=torch.int32, device=rows.device)
    kvals = torch.empty((B, cap), dtype=torch.float32, device=rows.device) if want_k else None
    _lib.check(lib.ml_mask_distribute_i32(_ptr(rows), rs, int(has_k), _ptr(kvals), _ptr(slots), _ptr(lcounts), _ptr(lmax),
                                          B, cap, max_k, float(base_size), _stream()), "ml_mask_distribute_i32")
    return slots, lcounts, lmax, kvals


def roi_crop_resize(fmap, rows, slots, lcounts, level, n_l, crop_size, img_hw, roi_boxes, box_off, live=None, out=None):
    """rows [B,cap,6] (cx,cy,w,h,cls,conf) or [B,cap,7] dist_boxes (k first).  live: device int32 [1] = the level's
    RoI maximum when the launch runs at capacity (n_l = cap): slots past max(1, live) are not written.  out: the
    [B,n_l,ch,cw,C] tensor of fmap's dtype to write the crops into (None: allocated here)."""
    lib = _lib.load()
    _require_dev(fmap, "fmap")
    B, Hf, Wf, Cc = fmap.shape
    cap, rs = rows.shape[1], rows.shape[2]
    roff = rs - 6
    L = slots.shape[1]
    ch, cw = crop_size
    if out is None:
        out = torch.empty((B, n_l, ch, cw, Cc), dtype=fmap.dtype, device=fmap.device)
    else:
        _require_dev(out, "out")
        if tuple(out.shape) != (B, n_l, ch, cw, Cc) or out.dtype != fmap.dtype:
            raise ValueError(f"roi_crop_resize: out {tuple(out.shape)} / {out.dtype} does not match "
                             f"{(B, n_l, ch, cw, Cc)} / {fmap.dtype}")
    fn = lib.ml_roi_crop_resize_f16 if fmap.dtype == torch.float16 else lib.ml_roi_crop_resize_f32
    _lib.check(fn(_ptr(fmap), _ptr(rows), rs, roff, _ptr(slots), _ptr(lcounts), _ptr(out),
                  _ptr(roi_boxes), B, Hf, Wf, Cc, cap, L, level, n_l, ch, cw,
                  float(img_hw[0]), float(img_hw[1]), box_off, roi_boxes.shape[1], _ptr(live), _stream()), "ml_roi_crop_resize")
    return out


def roi_crop_resize_grad(dys, fmap_shapes, rows, slots, lcounts, crop_size, img_hw, add=None, out=None):
    """Backward of roi_crop_resize for every level in ONE launch (csrc/resample_grad.hip), float32.  dys[l]: the gradient
    [B,n_l,ch,cw,C] at level l's molded crops (n_l the host-sized value, or cap from a fixed-capacity forward: the same
    bits); fmap_shapes[l]: that level's (B,Hf,Wf,C); rows / slots / lcounts: what mask_distribute and the forward used.
    Rows j >= lcounts[b,l] are MoldBatch padding: their dy is never read.  The boxes carry no gradient (tf.stop_gradient
    behind DetectionProposal).  add[l] / out[l]: out = add + gradient, in place if they are the same tensor.
    -> one [B,Hf,Wf,C] gradient per level; a gather over slot j, then oy, then ox: two launches give the same bits."""
    what = "roi_crop_resize_grad"
    n = len(dys)
    if n == 0 or n != len(fmap_shapes) or n > _lib.RESAMPLE_MAX_LEVELS:
        raise ValueError(f"{what}: {n} gradients for {len(fmap_shapes)} feature maps (1..{_lib.RESAMPLE_MAX_LEVELS} levels)")
    for name, t, dt in (("rows", rows, torch.float32), ("slots", slots, torch.int32), ("lcounts", lcounts, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f"{what}: `{name}` must be a {dt} tensor")
    if rows.dim() != 3 or rows.shape[2] < 6 or slots.dim() != 3 or tuple(slots.shape[::2]) != tuple(rows.shape[:2]):
        raise ValueError(f"{what}: rows {tuple(rows.shape)} / slots {tuple(slots.shape)} are not [B,cap,>=6] / [B,L,cap]")
    B, cap, rs = rows.shape
    L = slots.shape[1]
    if tuple(lcounts.shape) != (B, L) or n > L:
        raise ValueError(f"{what}: lcounts {tuple(lcounts.shape)} must be [{B}, {L}] and cover the {n} levels")
    ch, cw = int(crop_size[0]), int(crop_size[1])
    adds = [None] * n if add is None else list(add)
    outs = [None] * n if out is None else list(out)
    if len(adds) != n or len(outs) != n:
        raise ValueError(f"{what}: add / out must have one entry per level")
    Cc = int(fmap_shapes[0][-1])
    arr = (_lib.RoiGradLevel * n)()
    dxs, nbytes = [], 0
    for l, (d, dy, shape) in enumerate(zip(arr, dys, fmap_shapes)):
        shape = tuple(int(v) for v in shape)
        _grad_tensor(what, f"dys[{l}]", dy)
        if len(shape) != 4 or shape[0] != B or shape[3] != Cc:
            raise ValueError(f"{what}: fmap_shapes[{l}] = {shape} is not [{B}, Hf, Wf, {Cc}]")
        if dy.dim() != 5 or tuple(dy.shape[0:1] + dy.shape[2:]) != (B, ch, cw, Cc) or not 1 <= dy.shape[1] <= cap:
            raise ValueError(f"{what}: dys[{l}] is {tuple(dy.shape)}, expected [{B}, n_l <= {cap}, {ch}, {cw}, {Cc}]")
        dx = _grad_out(what, shape, dy.device, adds[l], outs[l])
        _require_dev(dy, f"dys[{l}]")
        d.dy, d.dx, d.add = dy.data_ptr(), dx.data_ptr(), None if adds[l] is None else adds[l].data_ptr()
        d.Hf, d.Wf, d.n_l = shape[1], shape[2], dy.shape[1]
        nbytes += 4 * (dy.numel() + dx.numel() * (2 if adds[l] is not None else 1))
        dxs.append(dx)
    for name, t in (("rows", rows), ("slots", slots), ("lcounts", lcounts)):
        _require_dev(t, name)
    lib = _lib.load()
    with _Prof("roi_crop_resize_grad", 0, nbytes, f"levels={n} crop={ch}x{cw} C={Cc}"):
        _lib.check(lib.ml_roi_crop_resize_grad_f32(arr, n, _ptr(rows), rs, rs - 6, _ptr(slots), _ptr(lcounts), B, Cc, cap, L, ch,
                                                   cw, float(img_hw[0]), float(img_hw[1]), _stream()),
                   "ml_roi_crop_resize_grad_f32")
    return dxs


def mold_levels(src, n_l, cap):
    """ml_mold_levels_f32: src [B, L*cap, ...] (level l's RoIs at rows l*cap ..) -> [B, sum(n_l), ...] with the first n_l[l]
    rows of every level next to each other; n_l: host ints."""
    lib = _lib.load()
    _require_dev(src, "src")
    if src.dtype != torch.float32:
        raise RuntimeError("mold_levels: float32 tensor expected")
    B, L = src.shape[0], len(n_l)
    if src.shape[1] != L * cap:
        raise ValueError(f"mold_levels: {src.shape[1]} rows per image, expected {L} x {cap}")
    E = int(np.prod(src.shape[2:]))
    if E % 4:                                      # [B, L*cap, 6] boxes: tiny, plain slicing (data movement only)
        return torch.cat([src[:, l * cap:l * cap + n] for l, n in enumerate(n_l)], dim=1).contiguous()
    out = torch.empty((B, int(sum(n_l))) + tuple(src.shape[2:]), dtype=torch.float32, device=src.device)
    arr = (C.c_int32 * L)(*[int(n) for n in n_l])
    _lib.check(lib.ml_mold_levels_f32(_ptr(src), _ptr(out), B, L, int(cap), E, arr, _stream()), "ml_mold_levels_f32")
    return out


def mold_levels_dev(src, lmax, cap):
    """ml_mold_levels_dev_f32: the same concatenation with the level sizes read on the DEVICE (`lmax`: int32 [L], the
    per-level RoI maxima) -- part of the captured forward.  -> a capacity buffer shaped like `src` whose flat FRONT holds the
    [B, sum n_l, ...] tensor; `molded_front(buf, n_l)` takes it as a view once the host knows n_l."""
    lib = _lib.load()
    _require_dev(src, "src")
    _require_dev(lmax, "lmax")
    if src.dtype != torch.float32 or lmax.dtype != torch.int32:
        raise RuntimeError("mold_levels_dev: float32 tensor and int32 level maxima expected")
    B, L = src.shape[0], int(lmax.numel())
    if src.shape[1] != L * cap:
        raise ValueError(f"mold_levels_dev: {src.shape[1]} rows per image, expected {L} x {cap}")
    E = int(np.prod(src.shape[2:]))
    out = torch.empty_like(src)
    _lib.check(lib.ml_mold_levels_dev_f32(_ptr(src), _ptr(out), B, L, int(cap), E, _ptr(lmax), _stream()), "ml_mold_levels_dev_f32")
    return out


def molded_front(buf, n_l):
    """The [B, sum(n_l), ...] tensor at the front of a mold_levels_dev() buffer (a view: no launch)."""
    B, total = buf.shape[0], int(sum(n_l))
    E = int(np.prod(buf.shape[2:]))
    return buf.view(-1)[:B * total * E].view((B, total) + tuple(buf.shape[2:]))


def add_(x, y):
    """x += y (same shape)."""
    lib = _lib.load()
    _require_dev(x, "x")
    _require_dev(y, "y")
    if x.shape != y.shape:
        raise ValueError("add_: shape mismatch")
    if x.dtype == torch.float16 and y.dtype == torch.float16:
        with _Prof("add_h", 0, 6 * x.numel()):
            _lib.check(lib.ml_add_f16(_ptr(x), _ptr(y), x.numel(), _stream()), "ml_add_f16")
        return x
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise NotImplementedError("add_: float32 or float16 tensors (one dtype for both)")
    _lib.check(lib.ml_add_f32(_ptr(x), _ptr(y), x.numel(), _stream()), "ml_add_f32")
    return x


def fill_(x, v):
    lib = _lib.load()
    _lib.check(lib.ml_fill_f32(_ptr(x), float(v), x.numel(), _stream()), "ml_fill_f32")
    return x


# ----------------------------------------------------------------------------- deploy wrapper
def resize_image_ac(x, oh, ow, threshold=None):
    """ml_resize_image_ac: bilinear(align_corners=True) of a [B,H,W,C] uint8 / float32 tensor, any C.
    threshold=None -> float32 result; else int32 `value > threshold`."""
    lib = _lib.load()
    _require_dev(x, "x")
    if x.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"resize_image_ac: uint8 or float32 input, got {x.dtype}")
    B, H, W, Cc = x.shape
    out_f = out_i = None
    if threshold is None:
        out_f = torch.empty((B, oh, ow, Cc), dtype=torch.float32, device=x.device)
    else:
        out_i = torch.empty((B, oh, ow, Cc), dtype=torch.int32, device=x.device)
    with _Prof("resize_image", 0, x.numel() * x.element_size() + 4 * B * oh * ow * Cc):
        _lib.check(lib.ml_resize_image_ac(_ptr(x), int(x.dtype == torch.uint8), _ptr(out_f), _ptr(out_i),
                                          float(threshold if threshold is not None else 0.0), B, H, W, Cc, oh, ow,
                                          _stream()), "ml_resize_image_ac")
    return out_f if threshold is None else out_i


def trim_instances(roi_boxes, roi_masks):
    """ml_trim_instances_f32 -> (boxes [B,N,6], masks [B,N,mh,mw], counts [B] int32), fixed capacity."""
    lib = _lib.load()
    _require_dev(roi_boxes, "roi_boxes")
    _require_dev(roi_masks, "roi_masks")
    B, N, six = roi_boxes.shape
    if six != 6 or roi_masks.dim() != 5 or tuple(roi_masks.shape[:2]) != (B, N):
        raise ValueError(f"trim_instances: roi_boxes [B,N,6] / roi_masks [B,N,h,w,C] expected, got "
                         f"{tuple(roi_boxes.shape)} / {tuple(roi_masks.shape)}")
    _, _, mh, mw, Cc = roi_masks.shape
    out_b = torch.empty((B, N, 6), dtype=torch.float32, device=roi_boxes.device)
    out_m = torch.empty((B, N, mh, mw), dtype=torch.float32, device=roi_boxes.device)
    counts = torch.empty((B,), dtype=torch.int32, device=roi_boxes.device)
    with _Prof("trim_instances", 0, 4 * (roi_boxes.numel() * 2 + out_m.numel() * 2)):
        _lib.check(lib.ml_trim_instances_f32(_ptr(roi_boxes), _ptr(roi_masks), _ptr(out_b), _ptr(out_m), _ptr(counts),
                                             B, N, mh, mw, Cc, _stream()), "ml_trim_instances_f32")
    return out_b, out_m, counts


def upsample_boxes(rows, ratio0, ratio1):
    lib = _lib.load()
    _require_dev(rows, "rows")
    out = torch.empty(rows.shape, dtype=torch.int32, device=rows.device)
    _lib.check(lib.ml_upsample_boxes_i32(_ptr(rows), _ptr(out), rows.numel() // 6, float(ratio0), float(ratio1),
                                         _stream()), "ml_upsample_boxes_i32")
    return out


def threshold_i32(x, threshold=0.5):
    lib = _lib.load()
    _require_dev(x, "x")
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    _lib.check(lib.ml_threshold_i32(_ptr(x), _ptr(out), float(threshold), x.numel(), _stream()), "ml_threshold_i32")
    return out


def semantic_smoothing(x, kernel_sizes, weights):
    """ml_semantic_smoothing_f32: per-class grey opening (erosion -> dilation, flat k x k) times weight."""
    lib = _lib.load()
    _require_dev(x, "x")
    B, H, W, Cc = x.shape
    if len(kernel_sizes) != Cc or len(weights) != Cc:
        raise ValueError(f"semantic_smoothing: {Cc} classes need {Cc} kernel sizes and weights")
    ks = (C.c_int32 * Cc)(*[int(k) for k in kernel_sizes])
    ws = (C.c_float * Cc)(*[float(w) for w in weights])
    out = torch.empty_like(x)
    tmp = torch.empty_like(x)
    with _Prof("semantic_smoothing", 0, 4 * x.numel() * 8):
        _lib.check(lib.ml_semantic_smoothing_f32(_ptr(x), _ptr(out), _ptr(tmp), B, H, W, Cc, ks, ws, _stream()),
                   "ml_semantic_smoothing_f32")
    return out


# ----------------------------------------------------------------------------- serving post-processing
def instance_summary_rois(seg, det_outs, ins_outs, road_channel=1, default_road_size=3.25, ioi_threshold=0.1):
    """ml_instance_summary_rois_f32: crop_pad_mask + instance_summary without the [B,n,H,W] canvases (bit-identical).
    seg int32 [B,H,W,C], det_outs int32 [B,n,6], ins_outs int32 [B,n,mh,mw] -> [B,n,5]."""
    lib = _lib.load()
    for t, name in ((seg, "seg"), (det_outs, "det_outs"), (ins_outs, "ins_outs")):
        _require_dev(t, name)
        if t.dtype != torch.int32:
            raise RuntimeError("instance_summary_rois: int32 semantic map, detections and masks expected")
    B, H, W, Cc = seg.shape
    _, n, mh, mw = ins_outs.shape
    out = torch.empty((B, n, 5), dtype=torch.float32, device=seg.device)
    ws = workspace(int(lib.ml_instance_summary_workspace_bytes(B, H)), seg.device, "summary")
    with _Prof("instance_summary_rois", 0, 4 * (ins_outs.numel() + 2 * seg.numel())):
        _lib.check(lib.ml_instance_summary_rois_f32(_ptr(seg), Cc, int(road_channel), _ptr(det_outs), _ptr(ins_outs), _ptr(out),
                                                    B, n, mh, mw, H, W, float(default_road_size), float(ioi_threshold),
                                                    _ptr(ws), _stream()), "ml_instance_summary_rois_f32")
    return out


def crop_pad_mask(det_outs, ins_outs, height, width):
    """ml_crop_pad_mask_f32: det [B,n,6] int32, masks [B,n,mh,mw] int32 -> [B,n,H,W] float32."""
    lib = _lib.load()
    _require_dev(det_outs, "det_outs")
    _require_dev(ins_outs, "ins_outs")
    if det_outs.dtype != torch.int32 or ins_outs.dtype != torch.int32:
        raise RuntimeError("crop_pad_mask: int32 detections and masks expected (UpSampleOutput's outputs)")
    B, n, _ = det_outs.shape
    _, _, mh, mw = ins_outs.shape
    out = torch.empty((B, n, height, width), dtype=torch.float32, device=det_outs.device)
    thr = torch.empty((1,), dtype=torch.int32, device=det_outs.device)
    with _Prof("crop_pad_mask", 0, 4 * (out.numel() + ins_outs.numel())):
        _lib.check(lib.ml_crop_pad_mask_f32(_ptr(det_outs), _ptr(ins_outs), _ptr(out), _ptr(thr), B, n, mh, mw,
                                            int(height), int(width), _stream()), "ml_crop_pad_mask_f32")
    return out


def nonzero_bbox(seg, channel):
    """ml_nonzero_bbox_i32 -> int32 [5] = (ymin, xmin, ymax, xmax, any) over the whole batch."""
    lib = _lib.load()
    _require_dev(seg, "seg")
    B, H, W, Cc = seg.shape
    box = torch.tensor([2 ** 31 - 1, 2 ** 31 - 1, -1, -1, 0], dtype=torch.int32, device=seg.device)
    _lib.check(lib.ml_nonzero_bbox_i32(_ptr(seg), B, H, W, Cc, int(channel), _ptr(box), _stream()), "ml_nonzero_bbox_i32")
    return box


def instance_summary(seg, masks, road_channel=1, default_road_size=3.25, ioi_threshold=0.1):
    """ml_instance_summary_f32 -> [B,n,5] = (pixel sum, instance size, horizontal, vertical, include_my_road)."""
    lib = _lib.load()
    _require_dev(seg, "seg")
    _require_dev(masks, "masks")
    if seg.dtype != torch.int32 or masks.dtype != torch.float32:
        raise RuntimeError("instance_summary: int32 semantic map and float32 padded masks expected")
    B, H, W, Cc = seg.shape
    _, n, _, _ = masks.shape
    out = torch.empty((B, n, 5), dtype=torch.float32, device=seg.device)
    ws = workspace(int(lib.ml_instance_summary_workspace_bytes(B, H)), seg.device, "summary")
    with _Prof("instance_summary", 0, 4 * (2 * masks.numel() + 2 * seg.numel())):
        _lib.check(lib.ml_instance_summary_f32(_ptr(seg), Cc, int(road_channel), _ptr(masks), _ptr(out), B, n, H, W,
                                               float(default_road_size), float(ioi_threshold), _ptr(ws), _stream()),
                   "ml_instance_summary_f32")
    return out


# ----------------------------------------------------------------------------- serving 'visualize' output
def _palette(colors, what):
    """[K,3] colours -> (ctypes fp32 host array, K), 1 <= K <= ML_DRAW_MAX_CLASSES."""
    c = np.asarray(colors, dtype=np.float32)
    if c.ndim != 2 or c.shape[1] != 3 or not 1 <= c.shape[0] <= _lib.DRAW_MAX_CLASSES:
        raise ValueError(f"{what}: colours must be [K, 3] with 1 <= K <= {_lib.DRAW_MAX_CLASSES}, got {c.shape}")
    return (C.c_float * c.size)(*c.ravel().tolist()), int(c.shape[0])


def _frames(images, what):
    _require_dev(images, "images")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise RuntimeError(f"{what}: uint8 [B,H,W,3] frames expected, got {images.dtype} {tuple(images.shape)}")
    return tuple(int(v) for v in images.shape[:3])


def _detections(det_outs, B, what):
    _require_dev(det_outs, "det_outs")
    if det_outs.dtype != torch.int32 or det_outs.dim() != 3 or det_outs.shape[0] != B or det_outs.shape[2] != 6:
        raise RuntimeError(f"{what}: int32 detections [B={B},n,6] expected, got {det_outs.dtype} {tuple(det_outs.shape)}")
    return int(det_outs.shape[1])


def draw_boxes(images, det_outs, out=None):
    """ml_draw_boxes_u8 (DrawBoxes): white 1-pixel outlines of every detection row.  `out` may be `images`."""
    lib = _lib.load()
    B, H, W = _frames(images, "draw_boxes")
    n = _detections(det_outs, B, "draw_boxes")
    out = torch.empty_like(images) if out is None else out
    with _Prof("draw_boxes", 0, (images.numel() if out.data_ptr() != images.data_ptr() else 0) + out.numel() + 24 * B * n):
        _lib.check(lib.ml_draw_boxes_u8(_ptr(images), _ptr(det_outs), _ptr(out), B, n, H, W, _stream()), "ml_draw_boxes_u8")
    return out


def draw_instance(images, det_outs, masks, colors, alpha, out=None):
    """ml_draw_instance_u8 (DrawInstance) over CropAndPadMask's float32 [B,n,H,W] canvases."""
    lib = _lib.load()
    B, H, W = _frames(images, "draw_instance")
    n = _detections(det_outs, B, "draw_instance")
    _require_dev(masks, "masks")
    if masks.dtype != torch.float32 or tuple(masks.shape) != (B, n, H, W):
        raise RuntimeError(f"draw_instance: float32 masks [{B},{n},{H},{W}] expected, got {masks.dtype} {tuple(masks.shape)}")
    cols, K = _palette(colors, "draw_instance")
    out = torch.empty_like(images) if out is None else out
    with _Prof("draw_instance", 0, 2 * images.numel() + 4 * masks.numel() + 24 * B * n):
        _lib.check(lib.ml_draw_instance_u8(_ptr(images), _ptr(det_outs), _ptr(masks), _ptr(out), cols, K, float(alpha), B, n,
                                           H, W, _stream()), "ml_draw_instance_u8")
    return out


def draw_segmentation(images, maps, colors, alpha, out=None):
    """ml_draw_segmentation_u8 (DrawSegmentation): maps int32 or float32 [B,H,W,K]."""
    lib = _lib.load()
    B, H, W = _frames(images, "draw_segmentation")
    _require_dev(maps, "maps")
    cols, K = _palette(colors, "draw_segmentation")
    if maps.dtype not in (torch.int32, torch.float32) or tuple(maps.shape) != (B, H, W, K):
        raise RuntimeError(f"draw_segmentation: int32 / float32 maps [{B},{H},{W},{K}] expected, got "
                           f"{maps.dtype} {tuple(maps.shape)}")
    out = torch.empty_like(images) if out is None else out
    with _Prof("draw_segmentation", 0, 2 * images.numel() + 4 * maps.numel()):
        _lib.check(lib.ml_draw_segmentation_u8(_ptr(images), _ptr(maps), int(maps.dtype == torch.float32), _ptr(out), cols, K,
                                               float(alpha), B, H, W, _stream()), "ml_draw_segmentation_u8")
    return out


def serving_visualize(images, det_outs, ins_outs, seg_outs, instance_colors, instance_alpha, semantic_colors,
                      semantic_alpha, out=None):
    """ml_serving_visualize_u8: DrawBoxes -> CropAndPadMask + DrawInstance -> DrawSegmentation in one pass, the same bytes
    as the four layers without the [B,n,H,W] canvases.  images uint8 [B,H,W,3], det_outs int32 [B,n,6], ins_outs int32
    [B,n,mh,mw], seg_outs int32 [B,H,W,Ks] -> uint8 [B,H,W,3].  No host synchronisation (graph-capturable)."""
    lib = _lib.load()
    B, H, W = _frames(images, "serving_visualize")
    n = _detections(det_outs, B, "serving_visualize")
    for t, name in ((ins_outs, "ins_outs"), (seg_outs, "seg_outs")):
        _require_dev(t, name)
        if t.dtype != torch.int32:
            raise RuntimeError(f"serving_visualize: int32 `{name}` expected, got {t.dtype}")
    ci, Ki = _palette(instance_colors, "serving_visualize")
    cs, Ks = _palette(semantic_colors, "serving_visualize")
    if ins_outs.dim() != 4 or tuple(ins_outs.shape[:2]) != (B, n):
        raise RuntimeError(f"serving_visualize: instance masks [{B},{n},mh,mw] expected, got {tuple(ins_outs.shape)}")
    if tuple(seg_outs.shape) != (B, H, W, Ks):
        raise RuntimeError(f"serving_visualize: semantic map [{B},{H},{W},{Ks}] expected (one colour per class), got "
                           f"{tuple(seg_outs.shape)}")
    mh, mw = int(ins_outs.shape[2]), int(ins_outs.shape[3])
    out = torch.empty_like(images) if out is None else out
    thr = torch.empty((1,), dtype=torch.int32, device=images.device)
    with _Prof("serving_visualize", 0, 2 * images.numel() + 4 * seg_outs.numel() + 4 * ins_outs.numel() + 24 * B * n,
               f"B={B} {H}x{W} n={n}"):
        _lib.check(lib.ml_serving_visualize_u8(_ptr(images), _ptr(det_outs), _ptr(ins_outs), _ptr(seg_outs), _ptr(out),
                                               _ptr(thr), ci, Ki, float(instance_alpha), cs, Ks, float(semantic_alpha), B, n,
                                               mh, mw, H, W, _stream()), "ml_serving_visualize_u8")
    return out


# ----------------------------------------------------------------------------- serving 'visualize' content (JPEG)
_jpeg_capacity = {}


def jpeg_capacity(H, W):
    """ml_jpeg_encode_capacity: bytes no H x W frame's file can exceed at any quality."""
    cap = _jpeg_capacity.get((H, W))
    if cap is None:
        cap = int(_lib.load().ml_jpeg_encode_capacity(H, W))
        if cap < 0:
            _lib.check(cap, "ml_jpeg_encode_capacity")
        _jpeg_capacity[(H, W)] = cap
    return cap


def encode_jpeg(images, quality=95):
    """ml_jpeg_encode_u8 (EncodeImageContent, tf.io.encode_jpeg's defaults): uint8 [B,H,W,3] -> (buffer uint8
    [B,capacity], lengths int32 [B]); image b's file is buffer[b, :lengths[b]].  Both stay on the device and nothing is
    read back (graph-capturable); the bytes past a length are unspecified."""
    lib = _lib.load()
    B, H, W = _frames(images, "encode_jpeg")
    if not isinstance(quality, (int, np.integer)) or isinstance(quality, bool) or not 1 <= quality <= 100:
        raise ValueError(f"encode_jpeg: quality must be an integer in 1..100, got {quality!r}")
    cap = jpeg_capacity(H, W)
    nbytes = int(lib.ml_jpeg_encode_workspace_bytes(B, H, W))
    if nbytes < 0:
        _lib.check(nbytes, "ml_jpeg_encode_workspace_bytes")
    ws = workspace(nbytes, images.device, "jpeg")
    out = torch.empty((B, cap), dtype=torch.uint8, device=images.device)
    lengths = torch.empty((B,), dtype=torch.int32, device=images.device)
    with _Prof("jpeg_encode", 0, images.numel(), f"B={B} {H}x{W} q={quality}"):
        _lib.check(lib.ml_jpeg_encode_u8(_ptr(images), B, H, W, int(quality), _ptr(out), cap, _ptr(lengths), _ptr(ws),
                                         _stream()), "ml_jpeg_encode_u8")
    return out, lengths


def jpeg_contents(buffer, lengths):
    """The files of encode_jpeg as host `bytes`, one per image: the lengths are read first, then exactly that many
    bytes of each row are copied."""
    n = lengths.cpu().tolist()                                    # synchronises with the encoder's stream
    return [bytes(buffer[b, :k].cpu().numpy()) for b, k in enumerate(n)]


# ----------------------------------------------------------------------------- serving request content (JPEG)
class UnsupportedJpeg(Exception):
    """The stream is not one the device decoder takes (progressive, 4:2:2, not a JPEG ...): decode it elsewhere."""


class JpegDecodeError(ValueError):
    """A baseline stream the device decoder takes, but malformed (truncated, a code that is not in its table ...)."""


def _last_error():
    msg = _lib.load().ml_last_error()
    return msg.decode() if msg else "?"


def jpeg_info(content):
    """ml_jpeg_decode_info: (H, W, mode, blocks) of a stream the device path takes, else UnsupportedJpeg.  Host only."""
    info = (C.c_int32 * 4)()
    status = _lib.load().ml_jpeg_decode_info(content, len(content), info)
    if status == _lib.JPEG_UNSUPPORTED:
        raise UnsupportedJpeg(_last_error())
    _lib.check(status, "ml_jpeg_decode_info")
    return tuple(info)


class _Staging:
    """Two pinned host buffers used in turn; each remembers the event that closes its last upload, so the copy of call n
    is never overwritten by call n + 1 (call n + 2 waits for it).  One per device and host thread."""

    def __init__(self):
        self.slots = [[None, None], [None, None]]
        self.turn = 0

    def take(self, nbytes):
        slot = self.slots[self.turn]
        self.turn ^= 1
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=True)
        return slot


_jpeg_staging = threading.local()                                 # .by_device: {device: _Staging}, dies with its thread


JPEG_ENTROPY = ("host", "device")
JPEG_ENTROPY_DEFAULT = "host"                                     # what entropy=None means


def _jpeg_entropy(entropy, what):
    entropy = JPEG_ENTROPY_DEFAULT if entropy is None else entropy
    if entropy not in JPEG_ENTROPY:
        raise ValueError(f"{what}: entropy must be one of {JPEG_ENTROPY}, got {entropy!r}")
    return entropy


def decode_jpeg(contents, device, entropy=None):
    """Baseline JPEG `bytes` (or a list of at most 32 of them, all of one H x W and sampling mode) -> uint8 [B,H,W,3] on `device`, the
    bytes libjpeg-turbo's default decode gives.  entropy="host": the host Huffman-decodes into pinned staging memory
    (ml_jpeg_decode_entropy), one asynchronous copy uploads the packed coefficients, two launches reconstruct
    (ml_jpeg_decode_u8); nothing is read back.  entropy="device": the raw files and their plans go up, the Huffman
    decoding runs in kernels (ml_jpeg_entropy_device) in front of the same two launches, and the B status words are
    read back; if one of them is not 0 the call is decoded again by the host path, which also words every error.
    UnsupportedJpeg: a stream the device path does not take; JpegDecodeError: a malformed one; ValueError: mixed
    sizes or modes."""
    lib = _lib.load()
    entropy = _jpeg_entropy(entropy, "decode_jpeg")
    single = isinstance(contents, (bytes, bytearray, memoryview))
    items = [bytes(c) for c in ([contents] if single else contents)]
    if not 1 <= len(items) <= _lib.JPEG_DECODE_MAX_BATCH:
        raise ValueError(f"decode_jpeg: 1 .. {_lib.JPEG_DECODE_MAX_BATCH} streams a call, got {len(items)}")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"decode_jpeg: a CUDA/HIP device expected, got {device} (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    infos = [jpeg_info(c) for c in items]
    H, W = infos[0][:2]
    if any(i[:2] != (H, W) for i in infos):
        raise ValueError(f"decode_jpeg: the streams of a call must have one size, got {[i[:2] for i in infos]}")
    mode = infos[0][2]
    if any(i[2] != mode for i in infos):
        raise ValueError(f"decode_jpeg: the streams of a call must have one sampling mode, got {[i[2] for i in infos]}")
    out = torch.empty((len(items), H, W, 3), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        if entropy != "device" or not _decode_jpeg_group_device(lib, items, H, W, mode, device, out):
            _decode_jpeg_group(lib, items, H, W, mode, device, out)
    return out


def _decode_jpeg_group(lib, items, H, W, mode, device, out):
    B = len(items)
    bounds = []
    for c in items:
        n = int(lib.ml_jpeg_decode_packed_bytes(c, len(c)))
        if n < 0:
            _lib.check(n, "ml_jpeg_decode_packed_bytes")
        bounds.append(n)
    by_device = _jpeg_staging.__dict__.setdefault("by_device", {})
    slot = by_device.setdefault(str(device), _Staging()).take(sum(bounds))
    host = slot[0]
    offsets = (C.c_int64 * (B + 1))()
    at = 0
    for b, c in enumerate(items):
        offsets[b] = at
        n = int(lib.ml_jpeg_decode_entropy(c, len(c), C.c_void_p(host.data_ptr() + at), bounds[b]))
        if n < 0:
            raise JpegDecodeError(f"decode_jpeg: stream {b}: {_last_error()}")
        at += (n + 15) // 16 * 16
    offsets[B] = at
    nbytes = int(lib.ml_jpeg_decode_workspace_bytes(B, H, W, mode))
    if nbytes < 0:
        _lib.check(nbytes, "ml_jpeg_decode_workspace_bytes")
    packed = torch.empty(at, dtype=torch.uint8, device=device)
    packed.copy_(host[:at], non_blocking=True)
    slot[1] = torch.cuda.Event()
    slot[1].record()
    ws = workspace(nbytes, device, "jpeg_decode")
    with _Prof("jpeg_decode", 0, at + 2 * nbytes + out.numel(), f"B={B} {H}x{W} mode={mode}"):
        _lib.check(lib.ml_jpeg_decode_u8(_ptr(packed), offsets, B, H, W, mode, _ptr(out), _ptr(ws), _stream()),
                   "ml_jpeg_decode_u8")


def jpeg_entropy_geometry():
    """ml_jpeg_entropy_geometry: (bits per subsequence, subsequences per workgroup) of the device entropy decoder."""
    g = (C.c_int32 * 2)()
    _lib.check(_lib.load().ml_jpeg_entropy_geometry(g), "ml_jpeg_entropy_geometry")
    return tuple(g)


def _jpeg_entropy_launch(lib, items, device):
    """Upload the files and their plans and enqueue ml_jpeg_entropy_device -> (packed uint8 tensor, packed offsets
    c_int64 [B + 1], status int32 [B,4] tensor), all on the device and nothing read; None if a stream has no plan (the
    host decoder then says why)."""
    B = len(items)
    plan_bytes = int(lib.ml_jpeg_entropy_plan_bytes())
    file_offsets = (C.c_int64 * (B + 1))()
    packed_offsets = (C.c_int64 * (B + 1))()
    at, room = B * plan_bytes, 0
    for b, c in enumerate(items):
        n = int(lib.ml_jpeg_decode_packed_bytes(c, len(c)))
        if n < 0:
            _lib.check(n, "ml_jpeg_decode_packed_bytes")
        packed_offsets[b] = room
        room += (n + 15) // 16 * 16
        file_offsets[b] = at
        at += len(c)
    file_offsets[B], packed_offsets[B] = at, room
    by_device = _jpeg_staging.__dict__.setdefault("by_device", {})
    slot = by_device.setdefault(str(device), _Staging()).take(at)
    host = slot[0]
    for b, c in enumerate(items):
        if lib.ml_jpeg_entropy_plan(c, len(c), C.c_void_p(host.data_ptr() + b * plan_bytes)) != 0:
            return None
        C.memmove(host.data_ptr() + file_offsets[b], c, len(c))
    for b in range(B + 1):
        file_offsets[b] -= B * plan_bytes                         # relative to the first file
    nbytes = int(lib.ml_jpeg_entropy_workspace_bytes(file_offsets, B))
    if nbytes < 0:
        _lib.check(nbytes, "ml_jpeg_entropy_workspace_bytes")
    up = torch.empty(at, dtype=torch.uint8, device=device)
    up.copy_(host[:at], non_blocking=True)
    slot[1] = torch.cuda.Event()
    slot[1].record()
    packed = torch.empty(room, dtype=torch.uint8, device=device)
    status = torch.empty((B, 4), dtype=torch.int32, device=device)
    ws = workspace(nbytes, device, "jpeg_entropy")
    with _Prof("jpeg_entropy", 0, at + room, f"B={B}"):
        _lib.check(lib.ml_jpeg_entropy_device(C.c_void_p(up.data_ptr() + B * plan_bytes), file_offsets, _ptr(up), B,
                                              _ptr(packed), packed_offsets, _ptr(status), _ptr(ws), _stream()),
                   "ml_jpeg_entropy_device")
    return packed, packed_offsets, status


def _decode_jpeg_group_device(lib, items, H, W, mode, device, out):
    """The device entropy decoder in front of the two launches of ml_jpeg_decode_u8, on one stream; the statuses are the
    one host read.  False: a stream did not end with status 0 and `out` is to be decoded by the host path."""
    launched = _jpeg_entropy_launch(lib, items, device)
    if launched is None:
        return False
    packed, packed_offsets, status = launched
    B = len(items)
    nbytes = int(lib.ml_jpeg_decode_workspace_bytes(B, H, W, mode))
    if nbytes < 0:
        _lib.check(nbytes, "ml_jpeg_decode_workspace_bytes")
    ws = workspace(nbytes, device, "jpeg_decode")
    # (a stream that failed has had its words cleared by the entropy decoder's last launch: every block reads as empty)
    with _Prof("jpeg_decode", 0, packed.numel() + 2 * nbytes + out.numel(), f"B={B} {H}x{W} mode={mode}"):
        _lib.check(lib.ml_jpeg_decode_u8(_ptr(packed), packed_offsets, B, H, W, mode, _ptr(out), _ptr(ws), _stream()),
                   "ml_jpeg_decode_u8")
    return not bool(status[:, 0].any().item())


def jpeg_entropy_device(contents, device):
    """ml_jpeg_entropy_device alone, for tests: `bytes` or a list of them -> (packed uint8 tensor on `device`, offsets
    list [B + 1] -- stream b's packed form starts at offsets[b] --, status int32 [B,4] NumPy array: status, block,
    most rounds, last launch that moved a state across workgroups)."""
    lib = _lib.load()
    single = isinstance(contents, (bytes, bytearray, memoryview))
    items = [bytes(c) for c in ([contents] if single else contents)]
    if not 1 <= len(items) <= _lib.JPEG_DECODE_MAX_BATCH:
        raise ValueError(f"jpeg_entropy_device: 1 .. {_lib.JPEG_DECODE_MAX_BATCH} streams a call, got {len(items)}")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"jpeg_entropy_device: a CUDA/HIP device expected, got {device} (no CPU fallback)")
    for c in items:
        jpeg_info(c)
    with torch.cuda.device(device):
        launched = _jpeg_entropy_launch(lib, items, device)
        if launched is None:
            raise JpegDecodeError(f"jpeg_entropy_device: {_last_error()}")
        packed, offsets, status = launched
        return packed, list(offsets), status.cpu().numpy()


# ----------------------------------------------------------------------------- evaluation (csrc/evaluate.hip)
_EVAL_DTYPE = {torch.float32: _lib.EVAL_F32, torch.float16: _lib.EVAL_F16, torch.int32: _lib.EVAL_I32,
               torch.uint8: _lib.EVAL_U8}


def _require_bytes(gt, name):
    _require_dev(gt, name)
    if gt.dtype not in (torch.int8, torch.uint8) or gt.dim() != 4:
        raise RuntimeError(f"masklab_hip: `{name}` must be an int8 or uint8 [B,G,H,W] tensor, got {gt.dtype} {tuple(gt.shape)}")


def eval_mask_area(gt):
    """ml_eval_mask_area: gt [B,G,H,W] int8 / uint8 -> int64 [B,G], the non-zero pixels of every ground-truth mask."""
    _require_bytes(gt, "gt")
    B, G, H, W = gt.shape
    out = torch.empty((B, G), dtype=torch.int64, device=gt.device)
    with _Prof("eval_mask_area", 0, gt.numel()):
        _lib.check(_lib.load().ml_eval_mask_area(_ptr(gt), B, G, H, W, _ptr(out), _stream()), "ml_eval_mask_area")
    return out


def eval_mask_pairs(det, ins, gt, gt_area, pairs):
    """ml_eval_mask_pairs: det [B,n,6] int32, ins [B,n,h,w] int32, gt [B,G,H,W] int8 / uint8, gt_area int64 [B,G],
    pairs int32 [P,3] = (b, pr_i, gt_i) -> int64 [P,2] = (intersection, union); (-1, -1) for an index out of range."""
    _require_bytes(gt, "gt")
    for t, name, dt in ((det, "det", torch.int32), (ins, "ins", torch.int32), (gt_area, "gt_area", torch.int64),
                        (pairs, "pairs", torch.int32)):
        _require_dev(t, name)
        if t.dtype != dt:
            raise RuntimeError(f"eval_mask_pairs: `{name}` must be {dt}, got {t.dtype}")
    B, G, H, W = gt.shape
    if det.dim() != 3 or det.shape[0] != B or det.shape[2] != 6 or ins.dim() != 4 or tuple(ins.shape[:2]) != tuple(det.shape[:2]) \
            or tuple(gt_area.shape) != (B, G) or pairs.dim() != 2 or pairs.shape[1] != 3:
        raise ValueError(f"eval_mask_pairs: shapes det {tuple(det.shape)} ins {tuple(ins.shape)} gt {tuple(gt.shape)} "
                         f"gt_area {tuple(gt_area.shape)} pairs {tuple(pairs.shape)} do not fit")
    n, mh, mw = ins.shape[1:]
    P = int(pairs.shape[0])
    out = torch.empty((P, 2), dtype=torch.int64, device=gt.device)
    with _Prof("eval_mask_pairs", 0, 0):
        _lib.check(_lib.load().ml_eval_mask_pairs(_ptr(det), _ptr(ins), _ptr(gt), _ptr(gt_area), _ptr(pairs), P, B, n, mh, mw,
                                                  G, H, W, _ptr(out), _stream()), "ml_eval_mask_pairs")
    return out


def eval_semantic_counts(pr, gt):
    """ml_eval_semantic_counts: pr int32 [B,H,W,C], gt uint8 [B,H,W,C] -> int64 [B,C,2] = (intersection, union) of the
    pixels > 0.5."""
    _require_dev(pr, "pr")
    _require_dev(gt, "gt")
    if pr.dtype != torch.int32 or gt.dtype != torch.uint8 or pr.dim() != 4 or pr.shape != gt.shape:
        raise RuntimeError(f"eval_semantic_counts: int32 predictions and uint8 ground truth of one [B,H,W,C] shape expected, "
                           f"got {pr.dtype} {tuple(pr.shape)} and {gt.dtype} {tuple(gt.shape)}")
    B, H, W, Cc = pr.shape
    out = torch.empty((B, Cc, 2), dtype=torch.int64, device=pr.device)
    with _Prof("eval_semantic_counts", 0, 5 * pr.numel()):
        _lib.check(_lib.load().ml_eval_semantic_counts(_ptr(pr), _ptr(gt), B, H, W, Cc, _ptr(out), _stream()),
                   "ml_eval_semantic_counts")
    return out


def class_binary_iou(seg_true, seg_pred, threshold):
    """ml_eval_class_binary_iou: [B,H,W,C] maps -> (counts int64 [B,C,3] = true, pred, both; iou float32 [C,B])."""
    _require_dev(seg_true, "seg_true")
    _require_dev(seg_pred, "seg_pred")
    if seg_true.dtype not in _EVAL_DTYPE or seg_pred.dtype not in _EVAL_DTYPE:
        raise RuntimeError(f"class_binary_iou: float32, float16, int32 or uint8 maps expected, got {seg_true.dtype}, {seg_pred.dtype}")
    if seg_true.dim() != 4 or seg_true.shape != seg_pred.shape:
        raise ValueError(f"class_binary_iou: two [B,H,W,C] maps of one shape expected, got {tuple(seg_true.shape)}, {tuple(seg_pred.shape)}")
    B, H, W, Cc = seg_true.shape
    counts = torch.empty((B, Cc, 3), dtype=torch.int64, device=seg_true.device)
    iou = torch.empty((Cc, B), dtype=torch.float32, device=seg_true.device)
    with _Prof("class_binary_iou", 0, seg_true.numel() * (seg_true.element_size() + seg_pred.element_size())):
        _lib.check(_lib.load().ml_eval_class_binary_iou(_ptr(seg_true), _EVAL_DTYPE[seg_true.dtype], _ptr(seg_pred),
                                                        _EVAL_DTYPE[seg_pred.dtype], B, H * W, Cc, float(threshold), _ptr(counts),
                                                        _ptr(iou), _stream()), "ml_eval_class_binary_iou")
    return counts, iou


def detection_iou_metric(proposed, gt):
    """ml_eval_detection_metric_f32: proposed [B,n,6], gt [B,m,6] float32 -> float32 [3,B] = precision, recall, fmeasure."""
    for t, name in ((proposed, "proposed_boxes"), (gt, "gt_boxes")):
        _require_dev(t, name)
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 6:
            raise RuntimeError(f"detection_iou_metric: `{name}` must be float32 [B,n,6], got {t.dtype} {tuple(t.shape)}")
    if proposed.shape[0] != gt.shape[0]:
        raise ValueError("detection_iou_metric: the batch sizes differ")
    B = proposed.shape[0]
    out = torch.empty((3, B), dtype=torch.float32, device=proposed.device)
    with _Prof("detection_iou_metric", 0, 4 * (proposed.numel() + gt.numel())):
        _lib.check(_lib.load().ml_eval_detection_metric_f32(_ptr(proposed), _ptr(gt), B, proposed.shape[1], gt.shape[1], _ptr(out),
                                                            _stream()), "ml_eval_detection_metric_f32")
    return out


def confusion_matrix_metric(cls_true, cls_pred, mask, threshold):
    """ml_eval_confusion_f32: cls_true, cls_pred float32 [B,A,C], mask float32 [B,A] -> (counts int64 [4] = tp, fp, fn, tn;
    metrics float32 [4] = precision, recall, accuracy, fmeasure)."""
    for t, name in ((cls_true, "cls_true"), (cls_pred, "cls_pred"), (mask, "mask")):
        _require_dev(t, name)
        if t.dtype != torch.float32:
            raise RuntimeError(f"confusion_matrix_metric: `{name}` must be float32, got {t.dtype}")
    if cls_true.shape != cls_pred.shape or cls_true.dim() < 2 or mask.numel() * cls_true.shape[-1] != cls_true.numel():
        raise ValueError(f"confusion_matrix_metric: shapes {tuple(cls_true.shape)}, {tuple(cls_pred.shape)}, {tuple(mask.shape)} do not fit")
    counts = torch.empty((4,), dtype=torch.int64, device=cls_true.device)
    metrics = torch.empty((4,), dtype=torch.float32, device=cls_true.device)
    with _Prof("confusion_matrix_metric", 0, 4 * (2 * cls_true.numel() + mask.numel())):
        _lib.check(_lib.load().ml_eval_confusion_f32(_ptr(cls_true), _ptr(cls_pred), _ptr(mask), mask.numel(), cls_true.shape[-1],
                                                     float(threshold), _ptr(counts), _ptr(metrics), _stream()),
                   "ml_eval_confusion_f32")
    return counts, metrics


def eval_reference_host(det=None, ins=None, gt=None, pairs=None, pr_sem=None, gt_sem=None):
    """ml_eval_reference_host: the per-thread code of the three evaluation kernels in CPU loops over NumPy arrays (for
    tests without a device; not a product path).  -> (area int64 [B,G] | None, pairs int64 [P,2] | None, semantic int64
    [B,C,2] | None) for the sections whose inputs are given."""
    def arr(a, dtypes):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if a.dtype not in dtypes:
            raise TypeError(f"eval_reference_host: {a.dtype} where one of {dtypes} is expected")
        return a if a.ctypes.data % 16 == 0 else a.copy()          # a slice of a batch: a fresh buffer is aligned

    det, ins, pairs, pr_sem = (arr(a, (np.int32,)) for a in (det, ins, pairs, pr_sem))
    gt, gt_sem = arr(gt, (np.int8, np.uint8)), arr(gt_sem, (np.uint8,))
    B = n = mh = mw = G = H = W = Cc = 1
    area = out_pairs = out_sem = None
    if gt is not None:
        B, G, H, W = gt.shape
        area = np.zeros((B, G), np.int64)
    if pairs is not None:
        if gt is None or det is None or ins is None or det.shape[:2] != ins.shape[:2] or det.shape[0] != B or det.shape[2] != 6:
            raise ValueError("eval_reference_host: the pair section needs det [B,n,6], ins [B,n,h,w] and gt [B,G,H,W]")
        n, mh, mw = ins.shape[1:]
        pairs = pairs.reshape(-1, 3)
        out_pairs = np.zeros((pairs.shape[0], 2), np.int64)
    if pr_sem is not None or gt_sem is not None:
        if pr_sem is None or gt_sem is None or pr_sem.shape != gt_sem.shape or pr_sem.ndim != 4:
            raise ValueError("eval_reference_host: the semantic section needs pr_sem and gt_sem of one [B,H,W,C] shape")
        if gt is not None and pr_sem.shape[:3] != (B, H, W):
            raise ValueError("eval_reference_host: the masks and the semantic maps differ in B, H or W")
        B, H, W, Cc = pr_sem.shape
        out_sem = np.zeros((B, Cc, 2), np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)
    _lib.check(_lib.load().ml_eval_reference_host(p(det), p(ins), p(gt), p(pairs), 0 if pairs is None else pairs.shape[0],
                                                  p(pr_sem), p(gt_sem), B, n, mh, mw, G, H, W, Cc, p(area), p(out_pairs),
                                                  p(out_sem)), "ml_eval_reference_host")
    return area, out_pairs, out_sem


# ----------------------------------------------------------------------------- generator resizes (csrc/cv_resize.hip)
def _cv_planes(op, x):
    """x [B,H,W,C] (uint8: images, semantic maps) or [B,n,H,W] (int8: instance masks, planes of one channel)
    -> (planes, H, W, C, the output's shape but for its two sizes)."""
    if x.dtype not in (torch.uint8, torch.int8) or x.dim() != 4:
        raise RuntimeError(f"{op}: a uint8 [B,H,W,C] or int8 [B,n,H,W] tensor expected, got {x.dtype} {tuple(x.shape)}")
    if not x.is_contiguous():
        raise RuntimeError(f"{op}: `x` must be contiguous")
    if x.dtype == torch.int8:
        B, n, H, W = x.shape
        return B * n, H, W, 1, lambda oh, ow: (B, n, oh, ow)
    B, H, W, Cc = x.shape
    return B, H, W, Cc, lambda oh, ow: (B, oh, ow, Cc)


def _cv_out(op, out, shape, dtype, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(f"{op}: `out` must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return out


def cv_resize_linear(x, oh, ow, skip_minus_one=False, out=None):
    """ml_cv_resize_linear_u8: cv2.resize(plane, (ow, oh)) of every plane, OpenCV's fixed-point uint8 arithmetic restated
    (INTER_AREA at exactly 2x on both axes).  x: uint8 [B,H,W,C], or int8 [B,n,H,W] handled as its bytes (the reference's
    `mask.astype(np.uint8)` and the store back into int8).  skip_minus_one: a plane that starts with -1 is filled with -1
    unread.  OpenCV parity is unpinned (include/masklab_hip.h, "Generator resizes")."""
    _require_dev(x, "x")
    planes, H, W, Cc, shape = _cv_planes("cv_resize_linear", x)
    oh, ow = int(oh), int(ow)
    out = _cv_out("cv_resize_linear", out, shape(oh, ow), x.dtype, x.device)
    with _Prof("cv_resize_linear", 0, x.numel() + out.numel(), f"{planes}x{H}x{W}x{Cc}->{oh}x{ow}"):
        _lib.check(_lib.load().ml_cv_resize_linear_u8(_ptr(x), _ptr(out), planes, H, W, Cc, oh, ow, int(bool(skip_minus_one)),
                                                      _stream()), "ml_cv_resize_linear_u8")
    return out


def cv_resize_linear_round(x, oh, ow, dtype=torch.float32, out=None):
    """ml_cv_resize_linear_round_u8: np.round(cv2.resize(plane.astype(float64), (ow, oh))) of uint8 [B,H,W,C] planes, read
    as bytes and converted per tap -> float32 or uint8 [B,oh,ow,C] (the value is an integer in 0..255 either way)."""
    _require_dev(x, "x")
    if x.dtype != torch.uint8 or dtype not in (torch.float32, torch.uint8):
        raise RuntimeError(f"cv_resize_linear_round: uint8 input and a float32 or uint8 result expected, got {x.dtype} -> {dtype}")
    planes, H, W, Cc, shape = _cv_planes("cv_resize_linear_round", x)
    oh, ow = int(oh), int(ow)
    out = _cv_out("cv_resize_linear_round", out, shape(oh, ow), dtype, x.device)
    with _Prof("cv_resize_linear_round", 0, x.numel() + out.numel() * out.element_size(), f"{planes}x{H}x{W}x{Cc}->{oh}x{ow}"):
        _lib.check(_lib.load().ml_cv_resize_linear_round_u8(_ptr(x), _ptr(out), int(dtype == torch.float32), planes, H, W, Cc, oh, ow,
                                                            _stream()), "ml_cv_resize_linear_round_u8")
    return out


def cv_resize_reference_host(x, oh, ow, mode="u8", skip_minus_one=False):
    """ml_cv_resize_reference_host: the per-thread code of the resize kernels in CPU loops over a NumPy array (for tests
    without a device and the generator's device="cpu" path; not a product path).  mode "u8": cv_resize_linear;
    "round_f32" / "round_u8": cv_resize_linear_round."""
    modes = {"u8": (_lib.CV_RESIZE_U8, None), "round_u8": (_lib.CV_RESIZE_ROUND_U8, np.uint8),
             "round_f32": (_lib.CV_RESIZE_ROUND_F32, np.float32)}
    if mode not in modes:
        raise ValueError(f"cv_resize_reference_host: mode must be one of {sorted(modes)}, got {mode!r}")
    code, out_dtype = modes[mode]
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.uint8, np.int8) or x.ndim != 4 or (mode != "u8" and x.dtype != np.uint8):
        raise TypeError(f"cv_resize_reference_host: a uint8 [B,H,W,C] or (mode 'u8') int8 [B,n,H,W] array expected, got {x.dtype} "
                        f"{x.shape}")
    oh, ow = int(oh), int(ow)
    if x.dtype == np.int8:
        (B, n, H, W), Cc = x.shape, 1
        planes, shape = B * n, (B, n, oh, ow)
    else:
        B, H, W, Cc = x.shape
        planes, shape = B, (B, oh, ow, Cc)
    if oh < 1 or ow < 1:
        raise ValueError(f"cv_resize_reference_host: bad output size {oh} x {ow}")
    out = np.empty(shape, out_dtype or x.dtype)
    _lib.check(_lib.load().ml_cv_resize_reference_host(C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), code, planes, H, W, Cc,
                                                       oh, ow, int(bool(skip_minus_one))), "ml_cv_resize_reference_host")
    return out


# ----------------------------------------------------------------------------- dataset polygons (csrc/polygon.hip)
def _poly_host(op, a, name, dtype, cols=None):
    """A host array (NumPy or a CPU tensor) -> contiguous NumPy of `dtype`, 1-d or [rows, cols]."""
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise TypeError(f"{op}: `{name}` must be in host memory")
        a = a.numpy()
    a = np.asarray(a)
    if a.dtype != dtype:
        raise TypeError(f"{op}: `{name}` must be {np.dtype(dtype).name}, got {a.dtype}")
    if (a.ndim != 1) if cols is None else (a.ndim != 2 or a.shape[1] != cols):
        raise ValueError(f"{op}: `{name}` must be {'1-d' if cols is None else f'[rows, {cols}]'}, got shape {a.shape}")
    return np.ascontiguousarray(a)


def _poly_offsets(op, a, name, count, limit):
    """An offsets array in host memory: int32 [count + 1], from >= 0, never decreasing, to <= limit."""
    a = _poly_host(op, a, name, np.int32)
    if a.shape[0] != count + 1:
        raise ValueError(f"{op}: `{name}` must have {count + 1} entries, got {a.shape[0]}")
    if a[0] < 0 or a[-1] > limit or (np.diff(a) < 0).any():
        raise ValueError(f"{op}: `{name}` must start at >= 0, never decrease and end at <= {limit}")
    return a


def _poly_sizes(op, H, W, **counts):
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{op}: bad plane size {H} x {W} (H, W >= 1, H*W < 2^31)")
    for name, v in counts.items():
        if int(v) < 0:
            raise ValueError(f"{op}: `{name}` must be >= 0, got {v}")
    return (H, W) + tuple(int(v) for v in counts.values())


def _poly_dev(op, a, name, dtype, device, check):
    """A device tensor as it is (its offsets are trusted: the kernels clamp them), or a host array checked and uploaded."""
    if isinstance(a, torch.Tensor) and a.is_cuda:
        if a.dtype != dtype or not a.is_contiguous() or a.device != device:
            raise TypeError(f"{op}: `{name}` on the device must be a contiguous {dtype} tensor on {device}")
        return a
    return torch.from_numpy(check(a)).to(device)


def _poly_device(device, out):
    if out is not None:
        return out.device
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"masklab_hip: the polygon kernels run only on the device, got {device} (the host loops are "
                           f"polygon_reference_host)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def polygon_instance_masks(verts, plane_offsets, windows, B, n, H, W, device=None, out=None):
    """ml_polygon_instance_masks: polygons -> the int8 [B,n,H,W] instance planes of a batch in one launch.  verts float64
    [total,2] (x, y); plane_offsets int32 [B*n+1] into verts (an empty range: a padding plane of -1); windows int32 [B*n,4]
    = (x1, y1, x2, y2) inclusive: a plane is 1 inside its polygon (even-odd; include/masklab_hip.h, "Dataset polygons")
    and inside its window, 0 elsewhere.  Host arrays are checked and uploaded; device tensors are taken as they are.
    skimage parity is unpinned."""
    op = "polygon_instance_masks"
    H, W, B, n = _poly_sizes(op, H, W, B=B, n=n)
    device = _poly_device(device, out)
    out = _cv_out(op, out, (B, n, H, W), torch.int8, device)
    if B == 0 or n == 0:
        return out
    verts = _poly_dev(op, verts, "verts", torch.float64, device, lambda a: _poly_host(op, a, "verts", np.float64, 2))
    if verts.dim() != 2 or verts.shape[1] != 2:
        raise ValueError(f"{op}: `verts` must be [total, 2], got {tuple(verts.shape)}")
    total = int(verts.shape[0])
    plane_offsets = _poly_dev(op, plane_offsets, "plane_offsets", torch.int32, device,
                              lambda a: _poly_offsets(op, a, "plane_offsets", B * n, total))
    windows = _poly_dev(op, windows, "windows", torch.int32, device, lambda a: _poly_host(op, a, "windows", np.int32, 4))
    if plane_offsets.numel() != B * n + 1 or tuple(windows.shape) != (B * n, 4):
        raise ValueError(f"{op}: plane_offsets {tuple(plane_offsets.shape)} / windows {tuple(windows.shape)} do not fit B*n = {B * n}")
    with torch.cuda.device(device), _Prof(op, 0, out.numel() + verts.numel() * 8, f"{B}x{n}x{H}x{W}"):
        _lib.check(_lib.load().ml_polygon_instance_masks(_ptr(verts), total, _ptr(plane_offsets), _ptr(windows), B, n, H, W, _ptr(out),
                                                         _stream()), "ml_polygon_instance_masks")
    return out


def polygon_semantic_maps(verts, poly_offsets, group_offsets, B, S, H, W, device=None, out=None):
    """ml_polygon_semantic_maps: polygons -> the uint8 [B,H,W,S] semantic maps of a batch in one launch.  poly_offsets int32
    [P+1] into verts; group_offsets int32 [B*(S+1)+1] into the polygons: group (b, s) is label s of image b, group (b, S) the
    except group.  Channel s is 1 inside any polygon of its group and outside every except polygon.  S <= 16."""
    op = "polygon_semantic_maps"
    H, W, B, S = _poly_sizes(op, H, W, B=B, S=S)
    if S > _lib.EVAL_MAX_CLASSES:
        raise ValueError(f"{op}: {S} semantic labels, at most {_lib.EVAL_MAX_CLASSES}")
    device = _poly_device(device, out)
    out = _cv_out(op, out, (B, H, W, S), torch.uint8, device)
    if B == 0 or S == 0:
        return out
    verts = _poly_dev(op, verts, "verts", torch.float64, device, lambda a: _poly_host(op, a, "verts", np.float64, 2))
    if verts.dim() != 2 or verts.shape[1] != 2:
        raise ValueError(f"{op}: `verts` must be [total, 2], got {tuple(verts.shape)}")
    total = int(verts.shape[0])
    P = int(poly_offsets.shape[0]) - 1 if hasattr(poly_offsets, "shape") and len(poly_offsets.shape) == 1 else len(poly_offsets) - 1
    if P < 0:
        raise ValueError(f"{op}: `poly_offsets` must have at least one entry")
    poly_offsets = _poly_dev(op, poly_offsets, "poly_offsets", torch.int32, device, lambda a: _poly_offsets(op, a, "poly_offsets", P, total))
    group_offsets = _poly_dev(op, group_offsets, "group_offsets", torch.int32, device,
                              lambda a: _poly_offsets(op, a, "group_offsets", B * (S + 1), P))
    if poly_offsets.numel() != P + 1 or group_offsets.numel() != B * (S + 1) + 1:
        raise ValueError(f"{op}: poly_offsets {tuple(poly_offsets.shape)} / group_offsets {tuple(group_offsets.shape)} do not fit")
    with torch.cuda.device(device), _Prof(op, 0, out.numel() + verts.numel() * 8, f"{B}x{H}x{W}x{S}"):
        _lib.check(_lib.load().ml_polygon_semantic_maps(_ptr(verts), total, _ptr(poly_offsets), P, _ptr(group_offsets), B, S, H, W,
                                                        _ptr(out), _stream()), "ml_polygon_semantic_maps")
    return out


def polygon_reference_host(kind, verts, offsets, B, n_or_S, H, W, windows=None, group_offsets=None):
    """ml_polygon_reference_host: the polygon kernels' edge, scan and store code in CPU loops over NumPy arrays (for tests
    without a device and the dataset's device="cpu" path; not a product path).  kind "instance": offsets = plane_offsets,
    `windows`, n_or_S = n -> int8 [B,n,H,W]; kind "semantic": offsets = poly_offsets, `group_offsets`, n_or_S = S -> uint8
    [B,H,W,S]."""
    op = "polygon_reference_host"
    if kind not in ("instance", "semantic"):
        raise ValueError(f"{op}: kind must be 'instance' or 'semantic', got {kind!r}")
    H, W, B, k = _poly_sizes(op, H, W, B=B, n_or_S=n_or_S)
    verts = _poly_host(op, verts, "verts", np.float64, 2)
    total = verts.shape[0]
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else C.c_void_p(0)
    if kind == "instance":
        out = np.empty((B, k, H, W), np.int8)
        if B == 0 or k == 0:
            return out
        if windows is None:
            raise ValueError(f"{op}: kind 'instance' needs `windows`")
        offsets = _poly_offsets(op, offsets, "plane_offsets", B * k, total)
        windows = _poly_host(op, windows, "windows", np.int32, 4)
        if windows.shape[0] != B * k:
            raise ValueError(f"{op}: `windows` must be [{B * k}, 4], got {windows.shape}")
        _lib.check(_lib.load().ml_polygon_reference_host(_lib.POLYGON_INSTANCE, vp(verts), total, vp(offsets), 0, None, vp(windows), B, k,
                                                         H, W, vp(out)), "ml_polygon_reference_host")
        return out
    if k > _lib.EVAL_MAX_CLASSES:
        raise ValueError(f"{op}: {k} semantic labels, at most {_lib.EVAL_MAX_CLASSES}")
    out = np.empty((B, H, W, k), np.uint8)
    if B == 0 or k == 0:
        return out
    if group_offsets is None:
        raise ValueError(f"{op}: kind 'semantic' needs `group_offsets`")
    P = len(offsets) - 1
    if P < 0:
        raise ValueError(f"{op}: `poly_offsets` must have at least one entry")
    offsets = _poly_offsets(op, offsets, "poly_offsets", P, total)
    group_offsets = _poly_offsets(op, group_offsets, "group_offsets", B * (k + 1), P)
    _lib.check(_lib.load().ml_polygon_reference_host(_lib.POLYGON_SEMANTIC, vp(verts), total, vp(offsets), P, vp(group_offsets), None, B, k,
                                                     H, W, vp(out)), "ml_polygon_reference_host")
    return out


# ----------------------------------------------------------------------------- trainer: target assignment (csrc/train_targets.hip)
def _require_f32(op, *named):
    for t, name in named:
        _require_dev(t, name)
        if t.dtype != torch.float32:
            raise RuntimeError(f"{op}: `{name}` must be float32, got {t.dtype}")


def calculate_iou(aa_boxes, bb_boxes):
    """ml_train_calculate_iou_f32 (CalculateIOU.call): float32 [n, >=4] and [m, >=4] rows of (cx, cy, w, h, ...) -> float32 [n,m]."""
    _require_f32("calculate_iou", (aa_boxes, "aa_boxes"), (bb_boxes, "bb_boxes"))
    if aa_boxes.dim() != 2 or bb_boxes.dim() != 2 or aa_boxes.shape[1] < 4 or bb_boxes.shape[1] < 4:
        raise ValueError(f"calculate_iou: two [n, >=4] box tables expected, got {tuple(aa_boxes.shape)}, {tuple(bb_boxes.shape)}")
    n, m = aa_boxes.shape[0], bb_boxes.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=aa_boxes.device)
    if n and m:
        _lib.check(_lib.load().ml_train_calculate_iou_f32(_ptr(aa_boxes), aa_boxes.shape[1], n, _ptr(bb_boxes), bb_boxes.shape[1], m,
                                                          _ptr(out), _stream()), "ml_train_calculate_iou_f32")
    return out


def best_prior(gt_boxes, pr_boxes):
    """ml_train_best_prior_f32: gt_boxes float32 [B,G,6] (-1 padded), pr_boxes int32 [A,4] -> int32 [B,G], the first index of
    the maximum of every ground truth's IoU row (0 for a row of zeros)."""
    _require_f32("best_prior", (gt_boxes, "gt_boxes"))
    _require_dev(pr_boxes, "pr_boxes")
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 6 or pr_boxes.dtype != torch.int32 or pr_boxes.dim() != 2 or pr_boxes.shape[1] != 4:
        raise ValueError(f"best_prior: float32 [B,G,6] boxes and an int32 [A,4] prior table expected, got {tuple(gt_boxes.shape)} and "
                         f"{pr_boxes.dtype} {tuple(pr_boxes.shape)}")
    B, G, _ = gt_boxes.shape
    A = pr_boxes.shape[0]
    if G == 0 or A == 0:
        raise ValueError("best_prior: no ground-truth rows or no priors")
    keys = torch.empty((B, G), dtype=torch.int64, device=gt_boxes.device)
    best = torch.empty((B, G), dtype=torch.int32, device=gt_boxes.device)
    with _Prof("best_prior", 0, 4 * (gt_boxes.numel() + pr_boxes.numel())):
        _lib.check(_lib.load().ml_train_best_prior_f32(_ptr(gt_boxes), _ptr(pr_boxes), B, G, A, _ptr(keys), _ptr(best), _stream()),
                   "ml_train_best_prior_f32")
    return best


def assign_boxes(gt_boxes, pr_boxes, num_classes, best=None):
    """ml_train_assign_boxes_f32 (AssignBoxes.call) -> (cls_true [B,A,C], loc_true [B,A,4], assign_mask [B,A,1]) float32."""
    if best is None:
        best = best_prior(gt_boxes, pr_boxes)
    B, G, _ = gt_boxes.shape
    A, Cn = pr_boxes.shape[0], int(num_classes)
    dev = gt_boxes.device
    cls_true = torch.empty((B, A, Cn), dtype=torch.float32, device=dev)
    loc_true = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    mask = torch.empty((B, A, 1), dtype=torch.float32, device=dev)
    with _Prof("assign_boxes", 0, 4 * (gt_boxes.numel() + pr_boxes.numel() + cls_true.numel() + loc_true.numel() + mask.numel())):
        _lib.check(_lib.load().ml_train_assign_boxes_f32(_ptr(gt_boxes), _ptr(pr_boxes), _ptr(best), B, G, A, Cn, _ptr(cls_true),
                                                         _ptr(loc_true), _ptr(mask), _stream()), "ml_train_assign_boxes_f32")
    return cls_true, loc_true, mask


def assign_masks(roi_boxes, gt_boxes, gt_masks, crop_hw, num_classes, threshold=0.5):
    """ml_train_assign_masks (AssignMasks.call): roi_boxes [B,R,6], gt_boxes [B,G,6] float32, gt_masks [B,G,H,W] int8 / uint8
    -> int32 [B,R,h,w]."""
    _require_f32("assign_masks", (roi_boxes, "roi_boxes"), (gt_boxes, "gt_boxes"))
    _require_bytes(gt_masks, "gt_masks")
    B, G, H, W = gt_masks.shape
    if roi_boxes.dim() != 3 or roi_boxes.shape[2] != 6 or roi_boxes.shape[0] != B or tuple(gt_boxes.shape) != (B, G, 6):
        raise ValueError(f"assign_masks: shapes roi_boxes {tuple(roi_boxes.shape)} gt_boxes {tuple(gt_boxes.shape)} gt_masks "
                         f"{tuple(gt_masks.shape)} do not fit")
    R = roi_boxes.shape[1]
    mh, mw = int(crop_hw[0]), int(crop_hw[1])
    out = torch.empty((B, R, mh, mw), dtype=torch.int32, device=roi_boxes.device)
    dt = _lib.TRAIN_MASK_I8 if gt_masks.dtype == torch.int8 else _lib.TRAIN_MASK_U8
    with _Prof("assign_masks", 0, 4 * out.numel()):
        _lib.check(_lib.load().ml_train_assign_masks(_ptr(roi_boxes), _ptr(gt_boxes), _ptr(gt_masks), dt, B, R, G, H, W, mh, mw,
                                                     int(num_classes), float(threshold), _ptr(out), _stream()), "ml_train_assign_masks")
    return out


def assign_seg(gt_seg, out_hw):
    """ml_train_assign_seg (AssignSeg.call): gt_seg [B,H,W,C] float32 / uint8 -> float32 [B,oh,ow,C], rounded half to even."""
    _require_dev(gt_seg, "gt_seg")
    if gt_seg.dtype not in (torch.float32, torch.uint8) or gt_seg.dim() != 4:
        raise RuntimeError(f"assign_seg: a float32 or uint8 [B,H,W,C] map expected, got {gt_seg.dtype} {tuple(gt_seg.shape)}")
    B, H, W, Cn = gt_seg.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((B, oh, ow, Cn), dtype=torch.float32, device=gt_seg.device)
    with _Prof("assign_seg", 0, 4 * out.numel() + gt_seg.numel() * gt_seg.element_size()):
        _lib.check(_lib.load().ml_train_assign_seg(_ptr(gt_seg), _EVAL_DTYPE[gt_seg.dtype], B, H, W, Cn, oh, ow, _ptr(out), _stream()),
                   "ml_train_assign_seg")
    return out


# ----------------------------------------------------------------------------- trainer: the four losses (csrc/train_losses.hip)
# Each loss has one body, _x_loss(want_grad, ...): the checks, the allocations and the arguments of its forward op `x_loss`
# and of its fused op `x_loss_grad`, which adds d(sum_b upstream[b] * loss[b]) / d(prediction) from the same pass.
def _train_ws(B, Cc, device):
    """The per-block partial sums of one loss call: a few hundred KiB, written in full before they are read, so a fresh
    allocation per call (stream-ordered, like the outputs) rather than a cached workspace."""
    return torch.empty(int(_lib.load().ml_train_workspace_bytes(int(B), int(Cc))), dtype=torch.uint8, device=device)


def _upstream(op, upstream, B, device):
    """d(scalar) / d(loss[b]) as float32 [B] on the device; None = 1 / B, the K.mean the reference compiles per loss."""
    if upstream is None:
        return torch.full((B,), 1.0 / B, dtype=torch.float32, device=device)
    _require_f32(op, (upstream, "upstream"))
    if tuple(upstream.shape) != (B,):
        raise ValueError(f"{op}: `upstream` must be float32 [{B}], got {tuple(upstream.shape)}")
    return upstream


def _class_loss(want_grad, cls_true, cls_pred, assign_mask, cls_exists, weight, alpha, gamma, upstream=None, through_sigmoid=False):
    op = "class_loss_grad" if want_grad else "class_loss"
    _require_f32(op, (cls_true, "cls_true"), (cls_pred, "cls_pred"), (assign_mask, "assign_mask"), (cls_exists, "cls_exists"))
    if cls_true.dim() != 3 or cls_true.shape != cls_pred.shape or assign_mask.numel() * cls_true.shape[2] != cls_true.numel() or \
            tuple(cls_exists.shape) != (cls_true.shape[0], cls_true.shape[2]):
        raise ValueError(f"{op}: shapes {tuple(cls_true.shape)}, {tuple(cls_pred.shape)}, {tuple(assign_mask.shape)}, "
                         f"{tuple(cls_exists.shape)} do not fit")
    B, A, Cn = cls_true.shape
    dev = cls_true.device
    out = torch.empty((B,), dtype=torch.float32, device=dev)
    ws = _train_ws(B, Cn, dev)
    args = (_ptr(cls_true), _ptr(cls_pred), _ptr(assign_mask), _ptr(cls_exists), B, A, Cn, float(weight), float(alpha), float(gamma),
            _ptr(ws), _ptr(out))
    if not want_grad:
        with _Prof(op, 0, 4 * (2 * cls_true.numel() + assign_mask.numel())):
            _lib.check(_lib.load().ml_train_class_loss_f32(*args, _stream()), "ml_train_class_loss_f32")
        return out
    upstream = _upstream(op, upstream, B, dev)
    grad = torch.empty((B, A, Cn), dtype=torch.float32, device=dev)
    with _Prof(op, 0, 4 * (3 * cls_true.numel() + 2 * assign_mask.numel())):
        _lib.check(_lib.load().ml_train_class_loss_grad_f32(*args, _ptr(upstream), int(bool(through_sigmoid)), _ptr(grad), _stream()),
                   "ml_train_class_loss_grad_f32")
    return out, grad


def class_loss(cls_true, cls_pred, assign_mask, cls_exists, weight, alpha, gamma):
    """ml_train_class_loss_f32 (ClassLoss.call): [B,A,C], [B,A,C], [B,A(,1)], [B,C] float32 -> float32 [B]."""
    return _class_loss(False, cls_true, cls_pred, assign_mask, cls_exists, weight, alpha, gamma)


def class_loss_grad(cls_true, cls_pred, assign_mask, cls_exists, weight, alpha, gamma, upstream=None, through_sigmoid=False):
    """ml_train_class_loss_grad_f32: class_loss plus d(sum_b upstream[b] * loss[b]) / d(cls_pred) -> (loss [B], grad [B,A,C]).
    through_sigmoid: times cls_pred * (1 - cls_pred), the gradient at the output conv's pre-activation."""
    return _class_loss(True, cls_true, cls_pred, assign_mask, cls_exists, weight, alpha, gamma, upstream, through_sigmoid)


def _box_loss(want_grad, loc_true, loc_pred, assign_mask, weight, momentum, beta, use_adjust, state, upstream=None):
    op = "box_loss_grad" if want_grad else "box_loss"
    _require_f32(op, (loc_true, "loc_true"), (loc_pred, "loc_pred"), (assign_mask, "assign_mask"))
    if loc_true.dim() != 3 or loc_true.shape[2] != 4 or loc_true.shape != loc_pred.shape or assign_mask.numel() * 4 != loc_true.numel():
        raise ValueError(f"{op}: shapes {tuple(loc_true.shape)}, {tuple(loc_pred.shape)}, {tuple(assign_mask.shape)} do not fit")
    if use_adjust:
        _require_f32(op, (state, "state"))
        if state.numel() != 8:
            raise ValueError(f"{op}: `state` must hold moving_mean[4] and moving_var[4]")
    B, A, _ = loc_true.shape
    dev = loc_true.device
    out = torch.empty((B,), dtype=torch.float32, device=dev)
    ws = _train_ws(B, 4, dev)
    nbytes = 4 * (3 if use_adjust else 1) * (2 * loc_true.numel() + assign_mask.numel())           # with use_adjust, three passes
    args = (_ptr(loc_true), _ptr(loc_pred), _ptr(assign_mask), B, A, float(weight), float(momentum), float(1 - momentum), float(beta),
            int(bool(use_adjust)), _ptr(state if use_adjust else None), _ptr(ws), _ptr(out))
    if not want_grad:
        with _Prof(op, 0, nbytes):
            _lib.check(_lib.load().ml_train_box_loss_f32(*args, _stream()), "ml_train_box_loss_f32")
        return out
    upstream = _upstream(op, upstream, B, dev)
    grad = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    with _Prof(op, 0, nbytes + 4 * (assign_mask.numel() + loc_true.numel())):
        _lib.check(_lib.load().ml_train_box_loss_grad_f32(*args, _ptr(upstream), _ptr(grad), _stream()),
                   "ml_train_box_loss_grad_f32")
    return out, grad


def box_loss(loc_true, loc_pred, assign_mask, weight, momentum, beta, use_adjust, state=None):
    """ml_train_box_loss_f32 (BoxLoss.call): [B,A,4], [B,A,4], [B,A(,1)] float32 -> float32 [B].  state: float32 [8] on the
    device = moving_mean, moving_var, updated in place when use_adjust."""
    return _box_loss(False, loc_true, loc_pred, assign_mask, weight, momentum, beta, use_adjust, state)


def box_loss_grad(loc_true, loc_pred, assign_mask, weight, momentum, beta, use_adjust, state=None, upstream=None):
    """ml_train_box_loss_grad_f32: box_loss plus d(sum_b upstream[b] * loss[b]) / d(loc_pred) -> (loss [B], grad [B,A,4]).
    `state` moves once, as by one box_loss call; beta is a constant of the gradient."""
    return _box_loss(True, loc_true, loc_pred, assign_mask, weight, momentum, beta, use_adjust, state, upstream)


def _mask_loss(want_grad, mask_true, mask_pred, weight, label_smoothing, upstream=None, through_sigmoid=False):
    op = "mask_loss_grad" if want_grad else "mask_loss"
    _require_dev(mask_true, "mask_true")
    _require_f32(op, (mask_pred, "mask_pred"))
    if mask_true.dtype != torch.int32 or mask_pred.dim() != 5 or tuple(mask_true.shape) != tuple(mask_pred.shape[:4]):
        raise ValueError(f"{op}: int32 [B,R,h,w] targets and float32 [B,R,h,w,C] predictions expected, got {mask_true.dtype} "
                         f"{tuple(mask_true.shape)} and {tuple(mask_pred.shape)}")
    B, R, mh, mw, Cn = mask_pred.shape
    dev = mask_pred.device
    roi_loss = torch.empty((B, R), dtype=torch.float32, device=dev)
    out = torch.empty((B,), dtype=torch.float32, device=dev)
    args = (_ptr(mask_true), _ptr(mask_pred), B, R, mh, mw, Cn, float(weight), float(1 - label_smoothing), float(label_smoothing / 2.),
            _ptr(roi_loss), _ptr(out))
    if not want_grad:
        with _Prof(op, 0, 8 * mask_true.numel()):
            _lib.check(_lib.load().ml_train_mask_loss_f32(*args, _stream()), "ml_train_mask_loss_f32")
        return out
    upstream = _upstream(op, upstream, B, dev)
    grad = torch.empty((B, R, mh, mw, Cn), dtype=torch.float32, device=dev)
    with _Prof(op, 0, 4 * (4 * mask_true.numel() + mask_pred.numel())):
        _lib.check(_lib.load().ml_train_mask_loss_grad_f32(*args, _ptr(upstream), int(bool(through_sigmoid)), _ptr(grad), _stream()),
                   "ml_train_mask_loss_grad_f32")
    return out, grad


def mask_loss(mask_true, mask_pred, weight, label_smoothing):
    """ml_train_mask_loss_f32 (MaskLoss.call): mask_true int32 [B,R,h,w], mask_pred float32 [B,R,h,w,C] -> float32 [B]."""
    return _mask_loss(False, mask_true, mask_pred, weight, label_smoothing)


def mask_loss_grad(mask_true, mask_pred, weight, label_smoothing, upstream=None, through_sigmoid=False):
    """ml_train_mask_loss_grad_f32: mask_loss plus d(sum_b upstream[b] * loss[b]) / d(mask_pred) -> (loss [B], grad
    [B,R,h,w,C]): non-zero only in the class channel of the selected RoIs."""
    return _mask_loss(True, mask_true, mask_pred, weight, label_smoothing, upstream, through_sigmoid)


def _seg_loss(want_grad, seg_true, seg_pred, seg_exist, weight, label_smoothing, upstream=None, through_sigmoid=False):
    op = "seg_loss_grad" if want_grad else "seg_loss"
    _require_f32(op, (seg_true, "seg_true"), (seg_pred, "seg_pred"), (seg_exist, "seg_exist"))
    if seg_true.dim() != 4 or seg_true.shape != seg_pred.shape or tuple(seg_exist.shape) != (seg_true.shape[0], seg_true.shape[3]):
        raise ValueError(f"{op}: shapes {tuple(seg_true.shape)}, {tuple(seg_pred.shape)}, {tuple(seg_exist.shape)} do not fit")
    B, H, W, Cn = seg_true.shape
    dev = seg_true.device
    out = torch.empty((B,), dtype=torch.float32, device=dev)
    ws = _train_ws(B, Cn, dev)
    args = (_ptr(seg_true), _ptr(seg_pred), _ptr(seg_exist), B, H * W, Cn, float(weight), float(1 - label_smoothing),
            float(label_smoothing / 2.), _ptr(ws), _ptr(out))
    if not want_grad:
        with _Prof(op, 0, 8 * seg_true.numel()):
            _lib.check(_lib.load().ml_train_seg_loss_f32(*args, _stream()), "ml_train_seg_loss_f32")
        return out
    upstream = _upstream(op, upstream, B, dev)
    grad = torch.empty((B, H, W, Cn), dtype=torch.float32, device=dev)
    with _Prof(op, 0, 12 * seg_true.numel()):
        _lib.check(_lib.load().ml_train_seg_loss_grad_f32(*args, _ptr(upstream), int(bool(through_sigmoid)), _ptr(grad), _stream()),
                   "ml_train_seg_loss_grad_f32")
    return out, grad


def seg_loss(seg_true, seg_pred, seg_exist, weight, label_smoothing):
    """ml_train_seg_loss_f32 (SegLoss.call): seg_true, seg_pred [B,H,W,C], seg_exist [B,C] float32 -> float32 [B]."""
    return _seg_loss(False, seg_true, seg_pred, seg_exist, weight, label_smoothing)


def seg_loss_grad(seg_true, seg_pred, seg_exist, weight, label_smoothing, upstream=None, through_sigmoid=False):
    """ml_train_seg_loss_grad_f32: seg_loss plus d(sum_b upstream[b] * loss[b]) / d(seg_pred) -> (loss [B], grad [B,H,W,C])."""
    return _seg_loss(True, seg_true, seg_pred, seg_exist, weight, label_smoothing, upstream, through_sigmoid)


# ----------------------------------------------------------------------------- optimizers (csrc/optimizer.hip)
OPTIMIZER_KINDS = {"RectifiedAdam": _lib.OPT_RADAM, "AdamW": _lib.OPT_ADAMW}
_OPT_ROLES = ("p", "g", "m", "v")


def _optimizer_refuse(i, quad):
    """Words the TypeError / ValueError of tensor i, whose quick checks failed."""
    if len(quad) != 4:
        raise ValueError(f"optimizer_step: tensor {i} must be a (p, g, m, v) tuple")
    for role, t in zip(_OPT_ROLES, quad):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"optimizer_step: `{role}` of tensor {i} is a {type(t).__name__}, not a torch tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"optimizer_step: `{role}` of tensor {i} is {t.dtype}; the step is float32 only")
    n = quad[0].numel()
    for role, t in zip(_OPT_ROLES, quad):
        if not t.is_contiguous():
            raise ValueError(f"optimizer_step: `{role}` of tensor {i} must be contiguous")
        if t.numel() != n:
            raise ValueError(f"optimizer_step: `{role}` of tensor {i} has {t.numel()} elements, `p` has {n}")
    ptrs = [t.data_ptr() for t in quad]
    order = sorted(range(4), key=ptrs.__getitem__)
    for a, b in zip(order, order[1:]):
        if ptrs[b] - ptrs[a] < 4 * n:
            raise ValueError(f"optimizer_step: `{_OPT_ROLES[a]}` and `{_OPT_ROLES[b]}` of tensor {i} overlap")
    raise AssertionError("optimizer_step: a tensor was refused for no reason")


def optimizer_check(tensors):
    """The argument checks of a step, all on the host: float32 (TypeError); contiguous, equal numel, the four buffers of a
    tensor apart from each other (ValueError); and only when all of that holds: all on one device, none on the host
    (RuntimeError).  tensors: list of (p, g, m, v).  -> the table's key: a tuple of (p, g, m, v addresses, numel) per tensor.
    Runs every step over every tensor (an address may change under the same object), so the passing path is kept short."""
    f32, key, device, misplaced = torch.float32, [], None, None
    for i, quad in enumerate(tensors):
        try:
            p, g, m, v = quad
            fine = (p.dtype is f32 and g.dtype is f32 and m.dtype is f32 and v.dtype is f32 and
                    p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous())
            n = p.numel()
            fine = fine and g.numel() == n and m.numel() == n and v.numel() == n
        except (AttributeError, TypeError, ValueError):
            fine = False
        if not fine:
            _optimizer_refuse(i, quad)
        a, b, c, d = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        if n:
            w, x, y, z = sorted((a, b, c, d))
            if x - w < 4 * n or y - x < 4 * n or z - y < 4 * n:
                _optimizer_refuse(i, quad)
        key.append((a, b, c, d, n))
        if misplaced is None:
            at = p.get_device()                              # -1: the host
            if device is None and at >= 0:
                device = at
            if not (at == device and g.get_device() == at and m.get_device() == at and v.get_device() == at):
                role, t = next((r, t) for r, t in zip(_OPT_ROLES, quad) if t.get_device() != device)
                misplaced = (role, i, t.device)
    if misplaced is not None:
        role, i, where = misplaced
        if where.type != "cuda":
            raise RuntimeError(f"optimizer_step: `{role}` of tensor {i} is on {where}: the step runs only on the MI355X kernels "
                               f"(no CPU fallback)")
        raise RuntimeError(f"optimizer_step: `{role}` of tensor {i} is on {where}, the tensors before it on cuda:{device}")
    return tuple(key)


class OptimizerTable:
    """The device table of a step (`ml_opt_tensor` per tensor) and its pinned staging memory.  update() uploads the table
    only when an address or a size in it differs from the last upload: a stream-ordered copy from pinned memory on the current
    stream, never a device synchronise.  A captured step holds the table's address, so the table cannot change during a
    capture: take one eager step with the same tensors first."""

    def __init__(self):
        self.key = None
        self.table = None
        self.n = 0
        self.chunks = 0
        self.uploads = 0            # how many times the table went up (tests, timing)
        self._staging = _Staging()
        self._retired = []          # outgrown tables: a graph captured earlier may replay with their address

    def update(self, key, device):
        """key: what optimizer_check returned for the step's tensors."""
        if key == self.key and (self.table is None or self.table.device == device):
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("optimizer_step: the tensors differ from the last eager step's, and the device table cannot be "
                               "uploaded while a graph is captured: take one eager step with these tensors first")
        lib = _lib.load()
        n = len(key)
        nbytes = n * C.sizeof(_lib.OptTensor)
        chunks = 0
        if n:
            slot = self._staging.take(nbytes)
            host = slot[0]
            arr = (_lib.OptTensor * n).from_address(host.data_ptr())
            for e, (p, g, m, v, numel) in zip(arr, key):
                e.p, e.g, e.m, e.v, e.n, e.first_chunk = p, g, m, v, numel, 0
            chunks = int(lib.ml_optimizer_plan(arr, n))
            if chunks < 0:
                _lib.check(chunks, "ml_optimizer_plan")
            if self.table is None or self.table.numel() < nbytes or self.table.device != device:
                if self.table is not None:
                    self._retired.append(self.table)
                self.table = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.table[:nbytes].copy_(host[:nbytes], non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
            self.uploads += 1
        self.key, self.n, self.chunks = key, n, chunks


def optimizer_state(device, iterations=0, lr=0.001):
    """`ml_opt_state` on the device: int64 iterations, float32 lr (and 4 bytes of padding), as an int64 [2] tensor."""
    host = np.zeros(1, dtype=np.dtype([("iterations", "<i8"), ("lr", "<f4"), ("reserved", "<i4")]))
    host["iterations"], host["lr"] = int(iterations), float(lr)
    return torch.from_numpy(host.view(np.int64).copy()).to(device)


def optimizer_state_lr(state):
    """The float32 [1] view of a state's lr: fill_() sets it in stream order, .item() reads it."""
    return state.view(torch.float32)[2:3]


def optimizer_scalars_buffer(device):
    """`ml_opt_scalars` on the device, zeroed: what the scalars launch of a step writes and its apply launch reads."""
    return torch.zeros(C.sizeof(_lib.OptScalars), dtype=torch.uint8, device=device)


def optimizer_scalars_read(scalars):
    """A host copy of the device's `ml_opt_scalars` (a device-to-host read: for tests and logging, not part of a step)."""
    return _lib.OptScalars.from_buffer_copy(scalars.cpu().numpy().tobytes())


def optimizer_step(kind, tensors, table, state, scalars, beta_1, beta_2, epsilon, decay=0., weight_decay=0., init_lr=1.):
    """One step of the reference's RectifiedAdam / AdamW (kind: a key of OPTIMIZER_KINDS) over every (p, g, m, v) of `tensors`
    in two launches on the current stream: ml_optimizer_scalars reads `state` (optimizer_state: iterations and lr stay on the
    device), writes `scalars` (optimizer_scalars_buffer) and adds 1 to the iterations; ml_optimizer_apply_f32 updates p, m, v
    of every tensor in place.  table: the OptimizerTable of this parameter set.  Nothing is read on the host, so a step can be
    captured into a graph (after one eager step, which uploads the table).  An empty `tensors` still counts a step."""
    if kind not in OPTIMIZER_KINDS:
        raise ValueError(f"optimizer_step: kind must be one of {sorted(OPTIMIZER_KINDS)}, got {kind!r}")
    key = optimizer_check(tensors)
    for name, t in (("state", state), ("scalars", scalars)):
        _require_dev(t, name)
    if state.dtype != torch.int64 or state.numel() != 2 or scalars.dtype != torch.uint8 or scalars.numel() != C.sizeof(_lib.OptScalars):
        raise ValueError("optimizer_step: `state` must come from optimizer_state() and `scalars` from optimizer_scalars_buffer()")
    if key and tensors[0][0].device != state.device:
        raise RuntimeError(f"optimizer_step: the tensors are on {tensors[0][0].device}, the optimizer's state on {state.device}")
    lib = _lib.load()
    code = OPTIMIZER_KINDS[kind]
    with torch.cuda.device(state.device):
        table.update(key, state.device)
        nelem = sum(k[4] for k in key)
        with _Prof("optimizer_step", 12 * nelem, 28 * nelem, f"{kind} x{len(key)}"):
            dev_scalars = _ptr_as(scalars, _lib.OptScalars)
            _lib.check(lib.ml_optimizer_scalars(code, _ptr_as(state, _lib.OptState), dev_scalars, float(beta_1), float(beta_2),
                                                float(epsilon), float(decay), float(weight_decay), float(init_lr), _stream()),
                       "ml_optimizer_scalars")
            _lib.check(lib.ml_optimizer_apply_f32(code, _ptr_as(table.table, _lib.OptTensor), table.n, table.chunks, dev_scalars,
                                                  _stream()), "ml_optimizer_apply_f32")


# ----------------------------------------------------------------------------- re-packing stepped weights (csrc/repack.hip)
_REPACK_FORMS = (("wgt", torch.float32), ("x3", torch.float32), ("h", torch.float16), ("wino", torch.float32))


def _repack_tensor(on_gpu, what, name, t, dtype, numel, device):
    """-> (address, device) of destination or master `t`, checked against what the job's geometry says it holds; on_gpu: a
    launch follows, so the tensor must be on a device (a plan alone takes tensors from anywhere)."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous():
        raise TypeError(f"{what}: `{name}` must be a contiguous {dtype} torch tensor")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{what}: `{name}` has {t.numel()} elements, the job's geometry asks for {numel}")
    if on_gpu and not t.is_cuda:
        raise RuntimeError(f"{what}: `{name}` is on {t.device}: the re-pack runs only on the MI355X kernels (no CPU fallback)")
    if device is not None and t.device != device:
        raise RuntimeError(f"{what}: `{name}` is on {t.device}, the tensors before it on {device}")
    return t.data_ptr(), t.device


def _repack_fill(e, i, job, device, on_gpu=True):
    """Job dict `job` (DeviceConv.repack_jobs, repack_table_job) -> entry `e` of the host table.  -> (device, bytes moved)"""
    what = f"repack_weights: job {i}"
    kind = job.get("kind", "conv")
    if kind not in ("conv", "table"):
        raise ValueError(f"{what}: kind must be 'conv' or 'table', got {kind!r}")
    N, Cc, KH, KW = (int(job[k]) for k in ("N", "C", "KH", "KW"))
    taps = KH * KW
    s_n, s_c, s_tap, offset = (int(job[k]) for k in ("s_n", "s_c", "s_tap", "offset"))
    src = job["src"]
    extent = offset + (taps - 1) * s_tap + (Cc - 1) * s_c + (N - 1) * s_n + 1
    ptr, device = _repack_tensor(on_gpu, what, "kernel", src, torch.float32, None, device)
    if min(N, Cc, KH, KW, s_n, s_c) < 1 or s_tap < 0 or offset < 0 or extent > src.numel():
        raise ValueError(f"{what}: the view (N {N}, C {Cc}, {KH}x{KW}, strides {s_n}, {s_c}, {s_tap}, offset {offset}) does not lie "
                         f"inside the master's {src.numel()} elements")
    e.src, e.s_n, e.s_c, e.s_tap = ptr + 4 * offset, s_n, s_c, s_tap
    e.kind, e.N, e.C, e.KH, e.KW = (_lib.REPACK_TABLE if kind == "table" else _lib.REPACK_CONV), N, Cc, KH, KW
    e.cpp_shift, e.group_cin_step = int(job.get("cpp_shift", NO_PIX_SPAN)), int(job.get("group_cin_step", 0))
    e.bias_reps = int(job.get("bias_reps", 1))
    nbytes = 4 * N * Cc * taps
    if job.get("src_bias") is not None:
        e.src_bias = _repack_tensor(on_gpu, what, "bias", job["src_bias"], torch.float32, N if kind == "table" else None, device)[0]
        e.bias_n = job["src_bias"].numel()
    if kind == "table":
        cp = int(job["cp"])
        e.cp = cp
        e.table = _repack_tensor(on_gpu, what, "table", job["table"], torch.float32, Cc * cp, device)[0]
        if job.get("table_bias") is not None:
            e.table_bias = _repack_tensor(on_gpu, what, "table_bias", job["table_bias"], torch.float32, cp, device)[0]
        return device, nbytes + 4 * (Cc + 1) * cp
    if job.get("bias") is not None:
        if job.get("src_bias") is None:
            raise ValueError(f"{what}: a bias form needs a master bias")
        e.bias = _repack_tensor(on_gpu, what, "bias form", job["bias"], torch.float32, e.bias_n * e.bias_reps, device)[0]
        nbytes += 4 * e.bias_n * e.bias_reps
    for side, prefix in (("fwd", "fwd_"), ("tr", "tr_")):
        d = job.get(side)
        if not d:
            continue
        n_pad, span_pad, span_pad_h = int(d["n_pad"]), int(d["span_pad"]), int(d.get("span_pad_h", 0))
        setattr(e, prefix + "n_pad", n_pad), setattr(e, prefix + "span_pad", span_pad), setattr(e, prefix + "span_pad_h", span_pad_h)
        sizes = {"wgt": n_pad * taps * span_pad, "x3": n_pad * taps * span_pad, "h": n_pad * taps * span_pad_h,
                 "wino": max(n_pad, 128) * span_pad * 16}
        for form, dtype in _REPACK_FORMS:
            if d.get(form) is not None:
                addr = _repack_tensor(on_gpu, what, f"{side} {form}", d[form], dtype, sizes[form], device)[0]
                setattr(e, prefix + form, addr)
                nbytes += sizes[form] * (2 if form == "h" else 4)
    return device, nbytes


def repack_table_job(kernel, bias, table, table_bias):
    """The job of the fused mask tail's lane table (packing.pack_out1x1_table): kernel [1,1,C_mid,ncls] and bias [ncls] or None
    on the device -> `table` [C_mid / 32, 16, 2, cp] and `table_bias` [cp]."""
    if not isinstance(kernel, torch.Tensor) or kernel.dim() != 4 or tuple(kernel.shape[:2]) != (1, 1):
        raise ValueError("repack_table_job: `kernel` must be a [1,1,C_mid,ncls] tensor")
    cmid, ncls = int(kernel.shape[2]), int(kernel.shape[3])
    cp = 1
    while cp < ncls:
        cp *= 2
    return dict(kind="table", src=kernel, src_bias=bias, N=ncls, C=cmid, KH=1, KW=1, s_n=1, s_c=ncls, s_tap=0, offset=0,
                table=table, table_bias=table_bias, cp=cp)


class RepackTable:
    """The device table of a re-pack (`ml_repack_job` per job) and its pinned staging memory, kept by whoever re-packs the
    same layers every step: update() plans and uploads only when a job differs from the last upload's (a stream-ordered copy
    from pinned memory, never a device synchronise).  A captured re-pack holds the table's address: take one eager call with
    the same jobs first."""

    def __init__(self):
        self.raw = None
        self.table = None
        self.n = 0
        self.units = 0
        self.nbytes = 0
        self.uploads = 0
        self._staging = _Staging()
        self._retired = []          # outgrown tables, kept for good: a graph captured earlier may replay with their address
        self._seen = None           # (job dicts, their tensors, the tensors' addresses, device) of the last update

    @staticmethod
    def _job_tensors(jobs):
        out = []
        for j in jobs:
            out += [j.get(k) for k in ("src", "src_bias", "bias", "table", "table_bias")]
            for side in ("fwd", "tr"):
                out += [v for v in (j.get(side) or {}).values() if isinstance(v, torch.Tensor)]
        return [t for t in out if isinstance(t, torch.Tensor)]

    def update(self, jobs):
        """-> the jobs' device (None for no jobs).  The SAME job dicts as the last call (by identity) whose tensors sit where
        they sat are not checked again: a caller that keeps its job list pays for the checks once.  Job dicts are immutable
        once handed over: a caller that wants another tensor in a job builds a new dict (a dict changed in place would go
        unseen here)."""
        n = len(jobs)
        if self._seen is not None and len(self._seen[0]) == n and all(a is b for a, b in zip(self._seen[0], jobs)) and \
                [t.data_ptr() for t in self._seen[1]] == self._seen[2]:
            return self._seen[3]
        self._seen = None
        device = self._update(jobs)
        tensors = self._job_tensors(jobs)
        self._seen = (list(jobs), tensors, [t.data_ptr() for t in tensors], device)
        return device

    def _update(self, jobs):
        n = len(jobs)
        arr = (_lib.RepackJob * max(n, 1))()
        device, moved = None, 0
        for i, job in enumerate(jobs):
            device, b = _repack_fill(arr[i], i, job, device)
            moved += b
        raw = bytes(arr) if n else b""
        if raw == self.raw and (self.table is None or self.table.device == device):
            return device
        if n and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("repack_weights: the jobs differ from the last eager call's, and the device table cannot be "
                               "uploaded while a graph is captured: take one eager call with these jobs first")
        units = 0
        if n:
            units = int(_lib.load().ml_repack_plan(arr, n))
            if units < 0:
                _lib.check(units, "ml_repack_plan")
            nbytes = n * C.sizeof(_lib.RepackJob)
            slot = self._staging.take(nbytes)
            host = slot[0]
            C.memmove(host.data_ptr(), arr, nbytes)
            if self.table is None or self.table.numel() < nbytes or self.table.device != device:
                if self.table is not None:
                    self._retired.append(self.table)
                self.table = torch.empty(nbytes, dtype=torch.uint8, device=device)
            with torch.cuda.device(device):
                self.table[:nbytes].copy_(host[:nbytes], non_blocking=True)
                slot[1] = torch.cuda.Event()
                slot[1].record()
            self.uploads += 1
        self.raw, self.n, self.units, self.nbytes = raw, n, units, moved
        return device


def repack_plan(jobs):
    """Host only: validates `jobs` as ml_repack_plan does and -> (work units, [(nb, cb, first_unit) per job]).  Nothing is
    launched, so the tensors may live anywhere (a packing on the CPU plans like one on the device)."""
    n = len(jobs)
    arr = (_lib.RepackJob * max(n, 1))()
    device = None
    for i, job in enumerate(jobs):
        device, _ = _repack_fill(arr[i], i, job, device, on_gpu=False)
    units = int(_lib.load().ml_repack_plan(arr, n)) if n else 0
    if units < 0:
        _lib.check(units, "ml_repack_plan")
    return units, [(arr[i].nb, arr[i].cb, arr[i].first_unit) for i in range(n)]


def repack_weights(jobs, table=None):
    """Brings packed forms up to their master weights on the device, in place, every job in ONE launch on the current stream
    (ml_repack_f32): what a training step runs after the optimizer's step.  jobs: DeviceConv.repack_jobs() lists and
    repack_table_job() dicts, concatenated.  Every element of every destination is written (pads and zero blocks included),
    no address changes, nothing is read on the host.  table: the caller's RepackTable (a step that re-packs the same layers
    every time uploads its table once); None makes one for this call."""
    jobs = list(jobs)
    if not jobs:
        return
    table = RepackTable() if table is None else table
    device = table.update(jobs)
    with torch.cuda.device(device):
        with _Prof("repack_weights", 0, table.nbytes, f"x{table.n} ({table.units} units)"):
            _lib.check(_lib.load().ml_repack_f32(_ptr_as(table.table, _lib.RepackJob), table.n, table.units, _stream()),
                       "ml_repack_f32")
