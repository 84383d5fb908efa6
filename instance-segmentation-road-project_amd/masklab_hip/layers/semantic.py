"""Semantic-segmentation layers -- drop-ins for reference engine/layers/semantic.py:
AtrousSeparableConv2D :32-90, ASPPNetwork :93-168, SegmentationSubNet :178-246.
Every ReLU is fused into the GroupNormalization apply pass (or conv epilogue) and every
tf.concat is fused away: producers write their channel slice of the concat buffer directly."""
import numpy as np
import torch

from .. import ops
from ..keras_like import Conv2D, DepthwiseConv2D, Layer, check_incoming_grad, pair_grads
from ..normalization import GroupNormalization
from .detection import _TowerMixin


class AtrousSeparableConv2D(Layer):
    """depthwise 3x3 (dilated, 'same', no bias) -> GN -> ReLU -> 1x1 (no bias) -> GN -> ReLU
    (reference :32-90)."""

    def __init__(self, filters, dilation_rate=3, groups=16, **kwargs):
        prefix = kwargs.get('name', 'AtrousSeparableConv2d')
        super().__init__(**kwargs)
        self.groups = groups
        self.filters = filters
        self.dilation_rate = dilation_rate
        self.depth_conv2d = DepthwiseConv2D((3, 3), dilation_rate=dilation_rate, padding='same', use_bias=False,
                                            name=prefix + '_depthwise')
        self.point_conv2d = Conv2D(self.filters, (1, 1), use_bias=False, name=prefix + '_pointwise')
        self.depth_norm = GroupNormalization(groups=self.groups, name=prefix + '_depthwise_GN')
        self.point_norm = GroupNormalization(groups=self.groups, name=prefix + '_pointwise_GN')

    def build(self, input_shape):
        s = self.depth_conv2d.build(input_shape)
        s = self.depth_norm.build(s)
        s = self.point_conv2d.build(s)
        s = self.point_norm.build(s)
        self.built = True
        return s

    def children(self):
        return [self.depth_conv2d, self.depth_norm, self.point_conv2d, self.point_norm]

    def weight_specs(self):
        out = {}
        for ch in self.children():          # children carry the reference's explicit names
            out.update(ch.weight_specs())
        return out

    def _forward(self, inputs, out=None, out_coff=0, tape=None):
        """The one forward of `call` (tape None: the norms normalise in place) and `call_with_tape` (tape: a dict that
        receives each conv's input and each norm's input; the norms then write tensors of their own)."""
        d = self.depth_conv2d(inputs)
        dn = self.depth_norm(d, fuse_relu=True, inplace=tape is None)
        p = self.point_conv2d(dn)
        if tape is not None:
            tape.update(inputs=inputs, depth_out=d, point_in=dn, point_out=p)
        if out is None:
            return self.point_norm(p, fuse_relu=True, inplace=tape is None)
        return ops.groupnorm_chunk(p, self.point_norm.gamma, self.point_norm.beta, self.groups,
                                   self.point_norm.epsilon, relu=True, out=out, out_coff=out_coff)

    def call(self, inputs, out=None, out_coff=0, **kwargs):
        return self._forward(inputs, out, out_coff)

    def call_with_tape(self, inputs, out=None, out_coff=0, **kwargs):
        """`call` that keeps what `backward` needs.  -> (output, tape): the output is `call`'s bit for bit; the tape holds each
        conv's input and each norm's input.  The depthwise GroupNormalization writes a tensor of its own here where `call`
        normalises in place."""
        tape = {}
        return self._forward(inputs, out, out_coff, tape), tape

    def backward(self, tape, dy, need_dx=True, add=None):
        """Backward of `call_with_tape`: dy [B,H,W,filters] float32 (dense) is the gradient at the branch's output; it is
        overwritten.  point GN grad -> 1x1 wgrad / dgrad -> depth GN grad -> depthwise wgrad / dgrad.  add: dx = add +
        gradient (in place on `add`).  -> (dx or None unless need_dx, {full weight name: gradient})."""
        return _branches_backward([self], [tape], [dy], need_dx, add)

    def get_config(self):
        config = super().get_config()
        config.update({'filters': self.filters, 'dilation_rate': self.dilation_rate, 'groups': self.groups})
        return config


def _branches_backward(branches, tapes, dys, need_dx=True, add=None, lead=None):
    """The backward of several AtrousSeparableConv2D branches of ONE input, stage by stage in multi launches: the point
    norms (with `lead`, the ASPP's 1x1 branch as (conv, norm, conv input, norm input, dy), riding in the same launches:
    it is a point stage without a depthwise one), the 1x1 convs' weight and data gradients, the depth norms, the depthwise
    weight gradients (one launch for every dilation), and the input's gradient chained through add= in the order lead,
    then the branches as given.  -> (dx or None, {full weight name: gradient})"""
    grads = {}
    convs = [br.point_conv2d for br in branches]
    norms = [br.point_norm for br in branches]
    conv_in = [t["point_in"] for t in tapes]
    norm_in = [t["point_out"] for t in tapes]
    dys = list(dys)
    if lead is not None:
        convs, norms = [lead[0]] + convs, [lead[1]] + norms
        conv_in, norm_in, dys = [lead[2]] + conv_in, [lead[3]] + norm_in, [lead[4]] + dys
    for c in convs:
        c._check_backward()
    for br in branches:
        br.depth_conv2d._check_backward()
    back = GroupNormalization.backward_multi(norms, norm_in, dys, fuse_relu=True, inplace=True)
    for g, (_, gg) in zip(norms, back):
        g.name_grads(gg, grads)
    dzs = [dz for dz, _ in back]                             # at the 1x1 convs' output
    pairs = ops.conv2d_wgrad_multi([dict(x=x, dy=dz, want_bias=c.use_bias, **c._grad_args())
                                    for c, x, dz in zip(convs, conv_in, dzs)])
    for c, pair in zip(convs, pairs):
        c.name_grads(pair_grads(c, pair), grads)
    k = 0 if lead is None else 1
    dx = add
    if lead is not None and need_dx:
        dx = ops.conv2d_dgrad(dzs[0], in_hw=(conv_in[0].shape[1], conv_in[0].shape[2]), add=add, **convs[0]._grad_args())
    ddn = ops.conv2d_dgrad_multi([dict(dy=dz, in_hw=(x.shape[1], x.shape[2]), **c._grad_args())
                                  for c, x, dz in zip(convs[k:], conv_in[k:], dzs[k:])])
    dnorms = [br.depth_norm for br in branches]
    back = GroupNormalization.backward_multi(dnorms, [t["depth_out"] for t in tapes], ddn, fuse_relu=True, inplace=True)
    for g, (_, gg) in zip(dnorms, back):
        g.name_grads(gg, grads)
    dds = [dd for dd, _ in back]                             # at the depthwise convs' output
    dws = [br.depth_conv2d for br in branches]
    pairs = ops.dwconv3x3_wgrad_multi([dict(x=t["inputs"], dy=dd, want_bias=c.use_bias, C=c.C, **c._grad_args())
                                       for c, t, dd in zip(dws, tapes, dds)])
    for c, pair in zip(dws, pairs):
        c.name_grads(pair_grads(c, pair), grads)
    if not need_dx:
        return None, grads
    for c, t, dd in zip(dws, tapes, dds):
        x = t["inputs"]
        dx = ops.dwconv3x3_dgrad(dd, c.wgt, (x.shape[1], x.shape[2]), C=c.C, add=dx, out=dx, **c._grad_args())
    return dx, grads


class ASPPNetwork(Layer):
    """Atrous Spatial Pyramid Pooling (reference :93-168): 1x1 branch, three atrous separable
    branches, image-pooling branch (ReLU, NO GroupNorm), concat (5*nf) -> 1x1 -> GN -> ReLU."""

    def __init__(self, num_features=256, atrous_rate=(6, 12, 18), groups=16, **kwargs):
        self.num_features = num_features
        self.atrous_rate = atrous_rate
        self.groups = groups
        super().__init__(**kwargs)
        self.aspp_1x1 = Conv2D(num_features, (1, 1), use_bias=False, name='aspp_1x1')
        self.aspp_1x1_gn = GroupNormalization(groups=groups, name='aspp_1x1_GN')
        self.aspp_branches = [AtrousSeparableConv2D(num_features, dilation_rate=rate, groups=groups,
                                                    name=f'aspp_{rate}') for rate in atrous_rate]
        self.aspp_pool_conv = Conv2D(num_features, (1, 1), activation='relu', use_bias=False, name='aspp_pool')
        self.concat_conv = Conv2D(num_features, (1, 1), use_bias=False, name='concat_projection')
        self.concat_gn = GroupNormalization(groups=groups, name='concat_projection_GN')

    def build(self, input_shape):
        s = self.aspp_1x1.build(input_shape)
        self.aspp_1x1_gn.build(s)
        for br in self.aspp_branches:
            br.build(input_shape)
        self.aspp_pool_conv.build((input_shape[0], 1, 1, input_shape[-1]))
        n_cat = self.num_features * (2 + len(self.aspp_branches))
        s = self.concat_conv.build(tuple(input_shape[:3]) + (n_cat,))
        self.built = True
        return self.concat_gn.build(s)

    def children(self):
        return [self.aspp_1x1, self.aspp_1x1_gn, *self.aspp_branches, self.aspp_pool_conv,
                self.concat_conv, self.concat_gn]

    def weight_specs(self):
        out = {}
        for ch in self.children():
            out.update(ch.weight_specs())
        return out

    def _forward(self, inputs, tape=None):
        """The one forward of `call` (tape None: the norms normalise in place) and `call_with_tape` (tape: a dict that
        receives each conv's input, each norm's input and the pool conv's post-ReLU output, the branches' tapes under
        "branches"; the norms then write tensors of their own)."""
        B, H, W, _ = inputs.shape
        nf = self.num_features
        n_br = len(self.aspp_branches)
        cat = torch.empty((B, H, W, nf * (2 + n_br)), dtype=inputs.dtype, device=inputs.device)
        x1 = self.aspp_1x1(inputs)
        ops.groupnorm_chunk(x1, self.aspp_1x1_gn.gamma, self.aspp_1x1_gn.beta, self.groups,
                            self.aspp_1x1_gn.epsilon, relu=True, out=cat, out_coff=0)
        branch_tapes = [None if tape is None else {} for _ in self.aspp_branches]
        for i, (br, br_tape) in enumerate(zip(self.aspp_branches, branch_tapes)):
            br._forward(inputs, out=cat, out_coff=nf * (1 + i), tape=br_tape)
        pool_in = ops.global_mean(inputs)                    # tf.reduce_mean(axis=(1,2)) (:149)
        pool_out = self.aspp_pool_conv(pool_in)              # 1x1 + ReLU, no GN (:126-129)
        ops.resize_bilinear_ac(pool_out, H, W, out=cat, out_coff=nf * (1 + n_br))  # :152
        concat_out = self.concat_conv(cat)
        if tape is not None:
            tape.update(inputs=inputs, aspp_1x1_out=x1, branches=branch_tapes, pool_in=pool_in, pool_out=pool_out, cat=cat,
                        concat_out=concat_out)
        return self.concat_gn(concat_out, fuse_relu=True, inplace=tape is None)

    def call(self, inputs, **kwargs):
        return self._forward(inputs)

    def call_with_tape(self, inputs, **kwargs):
        """`call` that keeps what `backward` needs.  -> (output, tape): the output is `call`'s bit for bit; it differs from
        `call` only in that GroupNormalization writes a tensor of its own where `call` normalises in place.  The tape holds
        each conv's input, each norm's input and the pool conv's post-ReLU output."""
        tape = {}
        return self._forward(inputs, tape), tape

    def _concat_slices(self):
        """concat_projection cut along its input channels into the concat's 2 + len(rates) slices, each a dense 1x1 conv of
        its own: the data gradient of slice i is one problem on ITS transposed packing, so every slice's gradient arrives
        dense, which is what GroupNormalization's backward reads.  Made once per loaded weights."""
        dev = self.concat_conv.dev
        if getattr(self, "_slices_of", None) is not dev:
            from .. import packing
            k = packing.unpack_dense(dev.p)
            nf = self.num_features
            self._slices = [ops.DeviceConv(packing.pack_dense(np.ascontiguousarray(k[:, :, i * nf:(i + 1) * nf, :])),
                                           dev.wgt.device) for i in range(k.shape[2] // nf)]
            self._slices_of = dev
        return self._slices

    def device_params(self):
        """The concat slices are cut from the concat conv's host weights BEFORE that conv binds (afterwards it holds none),
        then follow the conv's master, each as its cin slice."""
        conv = self.concat_conv
        fresh = conv.dev is not None and getattr(conv, "_params_of", None) is not conv.dev
        slices = self._concat_slices() if fresh else None
        out = super().device_params()
        if fresh:
            nf = self.num_features
            for i, dc in enumerate(slices):
                dc.bind_master(conv._params["kernel"], cin_slice=(i * nf, (i + 1) * nf))
        return out

    def _own_repack_jobs(self):
        if getattr(self, "_slices_of", None) is not self.concat_conv.dev or not self.concat_conv.dev.follows_master:
            return []
        return [j for dc in self._slices if dc.follows_master for j in dc.repack_jobs()]

    def backward(self, tape, dy, need_dx=True):
        """Backward of `call_with_tape`: dy [B,H,W,num_features] float32 is the gradient at the output (left unchanged).
        concat_gn (relu) -> concat_conv's weight gradient and, as one multi launch of five problems on cin-sliced transposed
        packings, its data gradient into five dense slices; the 1x1 branch and the atrous branches stage by stage in
        multi launches (_branches_backward); the pool branch: resize_bilinear_ac_grad to 1x1 -> ReLU mask -> aspp_pool's
        weight / data gradient -> global_mean_grad.  The input's gradient is chained through add= in the fixed order
        aspp_1x1, the atrous branches in the order of `atrous_rate`, the pool branch.
        -> (dx [B,H,W,C] or None unless need_dx, {full weight name: gradient} with the names of init_weights())."""
        check_incoming_grad("ASPPNetwork.backward: dy", dy)
        x = tape["inputs"]
        B, H, W, _ = x.shape
        for c in (self.aspp_1x1, self.aspp_pool_conv, self.concat_conv):
            c._check_backward()
        grads = {}
        dz, gg = self.concat_gn.backward(tape["concat_out"], dy, fuse_relu=True)
        self.concat_gn.name_grads(gg, grads)
        cc = self.concat_conv
        cc.name_grads(pair_grads(cc, ops.conv2d_wgrad(tape["cat"], dz, want_bias=cc.use_bias, **cc._grad_args())), grads)
        dcat = ops.conv2d_dgrad_multi([dict(dy=dz, dc=dc, in_hw=(H, W), stride=1, padding="same", dilation=1)
                                       for dc in self._concat_slices()])
        # the pool branch first (it is small); its part of dx comes last in the chain
        d_pool = ops.resize_bilinear_ac_grad(dcat[-1], 1, 1)
        d_pool = ops.relu_grad(tape["pool_out"], d_pool, out=d_pool)
        d_mean, gp = self.aspp_pool_conv.backward(tape["pool_in"], d_pool, need_dx=need_dx)
        self.aspp_pool_conv.name_grads(gp, grads)
        dx, gb = _branches_backward(self.aspp_branches, tape["branches"], dcat[1:-1], need_dx,
                                    lead=(self.aspp_1x1, self.aspp_1x1_gn, x, tape["aspp_1x1_out"], dcat[0]))
        grads.update(gb)
        if need_dx:
            dx = ops.global_mean_grad(d_mean, H, W, add=dx, out=dx)
        return dx, grads

    def get_config(self):
        config = super().get_config()
        config.update({"num_features": self.num_features, "atrous_rate": self.atrous_rate, "groups": self.groups})
        return config


class SegmentationSubNet(Layer, _TowerMixin):
    """DeepLab V3+ decoder (reference :178-246): skip 1x1 -> GN -> ReLU ; upsample ASPP output
    (align_corners) ; concat ; depth x [Conv3x3+ReLU ; GN] ; Conv1x1 + sigmoid."""

    def __init__(self, num_depth=2, num_features=256, num_skip_features=48, num_classes=3,
                 use_separable_conv=False, expand_ratio=4., use_squeeze_excite=False, squeeze_ratio=16.,
                 groups=16, **kwargs):
        self.num_depth = num_depth
        self.num_features = num_features
        self.num_skip_features = num_skip_features
        self.num_classes = num_classes
        self.use_separable_conv = use_separable_conv
        self.expand_ratio = expand_ratio
        self.use_squeeze_excite = use_squeeze_excite
        self.squeeze_ratio = squeeze_ratio
        self.groups = groups
        super().__init__(**kwargs)
        self.skip_conv = Conv2D(self.num_skip_features, (1, 1), use_bias=False, name='skip_projection')
        self.skip_gn = GroupNormalization(groups=groups, name='skip_projection_GN')
        self.block = self._make_tower(self.name, num_depth, num_features, groups, use_separable_conv,
                                      expand_ratio, use_squeeze_excite, squeeze_ratio)
        self.output_layer = Conv2D(num_classes, (1, 1), activation='sigmoid', name=f'{self.name}/output')

    def build(self, input_shapes):
        dec_shape, skip_shape = input_shapes
        s = self.skip_conv.build(skip_shape)
        self.skip_gn.build(s)
        s = tuple(skip_shape[:3]) + (dec_shape[-1] + self.num_skip_features,)
        s = self._build_chain(self.block, s)
        self.built = True
        return self.output_layer.build(s)

    def children(self):
        return [self.skip_conv, self.skip_gn, *self.block, self.output_layer]

    def weight_specs(self):
        out = {}
        for ch in self.children():
            out.update(ch.weight_specs())
        return out

    def _forward(self, inputs, tape=None):
        """The one forward of `call` (tape None) and `call_with_tape` (tape: a dict that receives the skip conv's input and
        output, the tower's tape and the output conv's input; the tower's GroupNormalization then writes tensors of its
        own instead of normalising in place: _run_tower)."""
        dec_input, skip_dec_input = inputs[0], inputs[1]
        B, H, W, _ = skip_dec_input.shape
        c_dec = dec_input.shape[-1]
        cat = torch.empty((B, H, W, c_dec + self.num_skip_features), dtype=dec_input.dtype,
                          device=dec_input.device)
        s = self.skip_conv(skip_dec_input)
        ops.groupnorm_chunk(s, self.skip_gn.gamma, self.skip_gn.beta, self.groups, self.skip_gn.epsilon,
                            relu=True, out=cat, out_coff=c_dec)
        ops.resize_bilinear_ac(dec_input, H, W, out=cat, out_coff=0)      # ResizeLike (:226) into the concat (:227)
        if tape is not None:
            tape.update(inputs=[dec_input, skip_dec_input], skip_out=s)
        x = self._run_tower(self.block, cat, tape=tape)
        if tape is not None:
            tape["out_in"] = x
        return self.output_layer(x)

    def call(self, inputs, **kwargs):
        return self._forward(inputs)

    def call_with_tape(self, inputs, **kwargs):
        """`call` that keeps what `backward` needs.  -> (seg_pred, tape): seg_pred is `call`'s bit for bit; the tape holds the
        skip conv's input and output, the concat, every tower unit's conv input and post-ReLU output, and the output conv's
        input.  GroupNormalization writes a tensor of its own here where `call` normalises in place.  Towers with
        SqueezeExcite or separable units raise NotImplementedError."""
        self._check_tape_units([self._units(self.block)])      # before any launch
        tape = {}
        return self._forward(inputs, tape), tape

    def backward(self, tape, d_seg, need_dx=(True, True)):
        """Backward of `call_with_tape`: d_seg [B,H,W,num_classes] float32 is the gradient at the PRE-activation of the output
        conv's sigmoid (seg_loss_grad(through_sigmoid=True) / loss_and_gradients(wrt="pre_activation")).  The output 1x1
        conv (any cout: the data gradient pads dy through the gather), the tower units deepest first (the loop of the
        detection towers), then the concat splits: the decoder slice through resize_bilinear_ac_grad(dy_coff=0, C=c_dec) to
        the ASPP output's gradient, the skip slice through skip_gn's backward (relu) and skip_conv's weight gradient, and
        its data gradient if the skip input's gradient is wanted.
        -> ((d_aspp_out or None, d_skip_in or None) as need_dx says, {full weight name: gradient} with the names of
        init_weights(): what RectifiedAdam.apply_gradients takes)."""
        units = [self._units(self.block)]
        self._check_tape_units(units)
        dec_input, skip_in = tape["inputs"]
        B, H, W, _ = skip_in.shape
        check_incoming_grad("SegmentationSubNet.backward: d_seg", d_seg, (B, H, W, self.num_classes))
        need_dec, need_skip = need_dx
        grads = {}
        out = self.output_layer
        dx, go = out.backward(tape["out_in"], d_seg)
        out.name_grads(go, grads)
        d_cat = self._towers_backward(units, tape, [dx], grads)[0]
        c_dec = int(dec_input.shape[-1])
        d_dec = ops.resize_bilinear_ac_grad(d_cat, dec_input.shape[1], dec_input.shape[2], C=c_dec, dy_coff=0) if need_dec else None
        # the skip slice, dense: GroupNormalization's backward reads a dense dy
        d_s = torch.empty((B, H, W, self.num_skip_features), dtype=torch.float32, device=d_cat.device)
        ops.gather_channels(d_cat, c_dec, d_s)
        d_s, gg = self.skip_gn.backward(tape["skip_out"], d_s, fuse_relu=True, inplace=True)
        self.skip_gn.name_grads(gg, grads)
        d_skip, gs = self.skip_conv.backward(skip_in, d_s, need_dx=bool(need_skip))
        self.skip_conv.name_grads(gs, grads)
        return (d_dec, d_skip), grads

    def get_config(self):
        config = super().get_config()
        config.update({
            "num_depth": self.num_depth, "num_features": self.num_features,
            "num_skip_features": self.num_skip_features, "num_classes": self.num_classes,
            "use_separable_conv": self.use_separable_conv, "expand_ratio": self.expand_ratio,
            "use_squeeze_excite": self.use_squeeze_excite, "squeeze_ratio": self.squeeze_ratio,
            "groups": self.groups})
        return config


class SemanticSmoothing(Layer):
    """Label-map post-processing (reference semantic.py:258-292): grey opening -- tf.nn.erosion2d then
    tf.nn.dilation2d with an all-zero kernel_size x kernel_size element, SAME -- times `weight`;
    kernel_size <= 0 only applies the weight.  One instance handles every channel of its input with the
    same (kernel_size, weight), like the reference's per-class tf.split; `smooth_classes` below runs the
    whole split -> smooth -> concat of retinamasklab.py:619-627 in one call."""

    def __init__(self, kernel_size=10, weight=1., **kwargs):
        self.kernel_size = kernel_size
        self.weight = weight
        super().__init__(**kwargs)

    def call(self, inputs, **kwargs):
        n_classes = int(inputs.shape[-1])
        return ops.semantic_smoothing(inputs, [self.kernel_size] * n_classes, [self.weight] * n_classes)

    @staticmethod
    def smooth_classes(seg_pred, kernel_sizes, weights):
        """tf.split(seg_pred, n) -> SemanticSmoothing(kernel, weight) per class -> tf.concat."""
        return ops.semantic_smoothing(seg_pred, list(kernel_sizes), list(weights))

    def get_config(self):
        config = super().get_config()
        config.update({"kernel_size": self.kernel_size, "weight": self.weight})
        return config


class AssignSeg(Layer):
    """The semantic truth at the prediction's size (reference :304-311): inputs = [seg_true [B,H,W,C] float32 / uint8,
    seg_pred [B,h,w,C]] -> float32 [B,h,w,C] = tf.round (half to even) of ResizeLike's align_corners bilinear resize."""

    def call(self, inputs, **kwargs):
        seg_true, seg_pred = inputs[0], inputs[1]
        return ops.assign_seg(seg_true.contiguous(), (int(seg_pred.shape[1]), int(seg_pred.shape[2])))
