"""Detection layers -- drop-ins for reference engine/layers/detection.py:
FeaturePyramid :30-74, BoxRegressionSubNet :89-155, ClassificationSubNet :158-228,
PriorLayer :236-306, RestoreBoxes :309-344, NormalizeBoxes :347-375, DetectionProposal :435-578.
Same class names / constructor kwargs / get_config(); `call` runs the HIP kernels."""
import numpy as np
import torch

from .. import ops
from ..keras_like import Conv2D, Layer, check_incoming_grad, pair_grads
from ..normalization import GroupNormalization
from ..prior import PriorBoxes
from .misc import MobileSeparableConv2D, SqueezeExcite


class FeaturePyramid(Layer):
    """Build Feature Pyramid Network (reference :30-74).  Top-down pass: lateral 1x1, bilinear
    (align_corners) upsample of the previous PRE-3x3 sum fused with the add, then the 3x3 'P{k}'."""

    def __init__(self, strides, num_features=256, **kwargs):
        self.strides = strides
        self.num_features = num_features
        super().__init__(**kwargs)
        self.blocks = []
        for layer_stride in sorted(self.strides, reverse=True):
            p_num = int(np.round(np.log2(layer_stride)))
            lateral = Conv2D(num_features, (1, 1), padding='same', name=f'{self.name}/C{p_num}_lateral')
            out = Conv2D(num_features, (3, 3), padding='same', name=f'{self.name}/P{p_num}')
            self.blocks.append([lateral, out])

    def build(self, input_shapes):
        outs = []
        for block, shape in zip(self.blocks, list(input_shapes)[::-1]):
            s = block[0].build(shape)
            outs.append(block[1].build(s))
        self.built = True
        return outs[::-1]

    def children(self):
        return [l for b in self.blocks for l in b]

    def call(self, inputs, **kwargs):
        return self._forward(inputs, kwargs.get("fork_stream"))

    def call_with_tape(self, inputs):
        """`call` without fork_stream (the same launches on one stream: the same bits) and what `backward` needs.
        -> (outputs, tape): tape["inputs"] the C taps and tape["merged"] the merged maps the 3x3 convs read, finest first."""
        tape = {"inputs": list(inputs)}
        return self._forward(inputs, None, tape), tape

    def _forward(self, inputs, fork, tape=None):
        # The top-down chain (lateral -> resize + add -> next lateral ...) is serial, but the 3x3 output conv of a
        # coarse level only reads its own merged map and is a 64- / 256-tile launch: with `fork_stream` those run on an
        # auxiliary stream beside the chain; the finest level's conv (1024 tiles) closes the chain on the main stream.
        aux = fork("_fpn_stream") if fork is not None and len(inputs) > 1 else None
        main = torch.cuda.current_stream() if aux is not None else None
        prev = None
        pyramid_outputs = []
        last = len(inputs) - 1
        for idx, head in enumerate(inputs[::-1]):
            block = self.blocks[idx]
            lateral = block[0](head)
            if prev is not None:
                # ResizeLike(prev -> lateral size) + Add, in place into `lateral` (reference :58-60)
                ops.resize_bilinear_ac(prev, lateral.shape[1], lateral.shape[2], add=lateral, out=lateral)
            prev = lateral
            if tape is not None:
                tape.setdefault("merged", []).insert(0, lateral)
            if aux is not None and idx != last:
                aux.wait_stream(main)
                lateral.record_stream(aux)
                with torch.cuda.stream(aux):
                    pyramid_outputs.append(block[1](lateral))
            else:
                pyramid_outputs.append(block[1](lateral))
        if aux is not None:
            main.wait_stream(aux)
            for t in pyramid_outputs[:-1]:
                t.record_stream(main)
        return pyramid_outputs[::-1]

    def backward_top_down(self, d_merged):
        """Backward of the top-down chain of `call`.  d_merged: the gradients at the merged maps, finest first (what the 3x3
        output convs' data gradient delivers).  merged[l] = lateral[l] + resize(merged[l+1]), so the gradient at
        merged[l+1] also receives resize^T of the full gradient at merged[l]: d_merged[l+1] += resize^T(d_merged[l]), finest
        to coarsest, IN PLACE.  -> the same tensors, now the gradients at the lateral convs' outputs."""
        for fine, coarse in zip(d_merged[:-1], d_merged[1:]):
            ops.resize_bilinear_ac_grad(fine, coarse.shape[1], coarse.shape[2], add=coarse, out=coarse)
        return list(d_merged)

    def backward(self, tape, d_outputs, need_dx=False):
        """The layer's backward.  tape: call_with_tape's; d_outputs: the gradients at the outputs, finest first, float32
        [B,h,w,num_features] each (the 3x3 `P{k}` convs are linear: these are their pre-activation gradients).
        In this order: one conv2d_wgrad_multi and one conv2d_dgrad_multi over the 3x3 convs; backward_top_down in place on
        the result; one conv2d_wgrad_multi over the laterals; with need_dx their conv2d_dgrad_multi.
        -> (the gradients at the C taps, finest first, or None unless need_dx; {full weight name: gradient})"""
        n = len(tape["inputs"])
        if len(d_outputs) != n or len(tape["merged"]) != n:
            raise ValueError(f"FeaturePyramid.backward: {len(d_outputs)} gradients for {n} levels")
        blocks = self.blocks[:n][::-1]                           # finest first, like the tensors
        for l, (dy, m) in enumerate(zip(d_outputs, tape["merged"])):
            check_incoming_grad(f"FeaturePyramid.backward: d_outputs[{l}]", dy, m.shape)
        grads = {}

        def weight_grads(convs, xs, dys):
            for c in convs:
                c._check_backward()
            pairs = ops.conv2d_wgrad_multi([dict(x=x, dy=dy, want_bias=c.use_bias, **c._grad_args())
                                            for c, x, dy in zip(convs, xs, dys)])
            for c, pair in zip(convs, pairs):
                c.name_grads(pair_grads(c, pair), grads)

        def data_grads(convs, xs, dys):
            return ops.conv2d_dgrad_multi([dict(dy=dy, in_hw=(x.shape[1], x.shape[2]), **c._grad_args())
                                           for c, x, dy in zip(convs, xs, dys)])

        outs = [b[1] for b in blocks]
        weight_grads(outs, tape["merged"], d_outputs)
        d_lateral = self.backward_top_down(data_grads(outs, tape["merged"], d_outputs))
        laterals = [b[0] for b in blocks]
        weight_grads(laterals, tape["inputs"], d_lateral)
        d_inputs = data_grads(laterals, tape["inputs"], d_lateral) if need_dx else None
        return d_inputs, grads

    def get_config(self):
        config = super().get_config()
        config.update({"strides": self.strides, "num_features": self.num_features})
        return config


class _TowerMixin:
    """depth x [optional SqueezeExcite ; Conv3x3+ReLU ; GroupNormalization] shared by every head."""

    def _make_tower(self, prefix, num_depth, num_features, groups, use_separable_conv, expand_ratio,
                    use_squeeze_excite, squeeze_ratio):
        block = []
        for i in range(num_depth):
            if use_squeeze_excite:
                block.append(SqueezeExcite(squeeze_ratio, name=f'{prefix}/se{i}'))
            if use_separable_conv:
                block.append(MobileSeparableConv2D(num_features, (3, 3), expand_ratio=expand_ratio,
                                                   name=f'{prefix}/sep{i}'))
            else:
                block.append(Conv2D(num_features, (3, 3), activation='relu', padding='same',
                                    kernel_initializer='normal', kernel_stddev=0.01, name=f'{prefix}/conv{i}'))
            block.append(GroupNormalization(groups, name=f'{prefix}/gn{i}'))
        return block

    @staticmethod
    def _conv_tiles(c, x):
        """128 x 128 tiles of conv `c` on input `x` (the library's split-K / narrow-tile decisions look at this count)."""
        from ..packing import resolve_padding
        Ho, Wo, _, _ = resolve_padding(int(x.shape[1]), int(x.shape[2]), c.kernel_size[0], c.kernel_size[1], c.strides[0],
                                       c.dilation_rate[0], c.padding)
        return -(-int(x.shape[0]) * Ho * Wo // 128) * (c.dev.p.n_pad // 128 if c.dev.p.n_pad >= 128 else 1), (int(x.shape[0]), Ho, Wo)

    @staticmethod
    def _run_tower(block, x, tape=None):
        """tape: None, or a dict that receives what the backward needs, in _run_towers_multi's form for ONE tower -- per depth
        [conv input] ("conv_in") and [post-ReLU conv output] ("conv_out"); GroupNormalization then writes a tensor of its
        own instead of normalising the conv output in place (the same bits).  [Conv2D, GroupNormalization] units only."""
        if tape is not None:
            _TowerMixin._check_tape_units([_TowerMixin._units(block)])
            tape["conv_in"], tape["conv_out"] = [], []
        block_input = x                          # never modified in place (it is a caller's tensor)
        i = 0
        while i < len(block):
            layer = block[i]
            nxt = block[i + 1] if i + 1 < len(block) else None
            if tape is not None and isinstance(layer, Conv2D):
                tape["conv_in"].append([x])
            if isinstance(layer, Conv2D) and isinstance(nxt, GroupNormalization) and layer.dev is not None:
                # conv -> (ReLU) -> GroupNormalization: the conv's epilogue sums its tiles, no statistics pass (fp32, big maps)
                tiles, oshape = _TowerMixin._conv_tiles(layer, x)
                tpc = ops.gn_fusable(oshape, layer.filters, nxt.groups, layer.dev, tiles, x.dtype)
                if tpc:
                    part = torch.empty((tiles, 4, 2), dtype=torch.float64, device=x.device)
                    x = layer(x, gn_partials=part)
                    if tape is not None:
                        tape["conv_out"].append([x])
                    x = GroupNormalization.call_multi([nxt], [x], inplace=tape is None, partials=[(part, tpc)])[0]
                    i += 2
                    continue
            i += 1
            if isinstance(layer, GroupNormalization):
                x = layer(x, inplace=tape is None)      # conv output is a fresh tensor: normalise in place
            elif isinstance(layer, SqueezeExcite):
                x = layer(x, keep_input=(x is block_input))
            else:
                x = layer(x)
                if tape is not None:
                    tape["conv_out"].append([x])
        return x

    @staticmethod
    def _units(block):
        """The depth units [SqueezeExcite?, Conv2D | MobileSeparableConv2D, GroupNormalization] of a tower block, as
        (se or None, conv, norm) triples; None when the block is made of anything else."""
        units, i = [], 0
        while i < len(block):
            se = block[i] if isinstance(block[i], SqueezeExcite) else None
            i += se is not None
            if i + 1 >= len(block) or not isinstance(block[i], (Conv2D, MobileSeparableConv2D)) or \
                    not isinstance(block[i + 1], GroupNormalization):
                return None
            units.append((se, block[i], block[i + 1]))
            i += 2
        return units

    @staticmethod
    def _run_towers_multi(blocks, xs, lives=None, tape=None):
        """Depth-major execution of several un-shared towers (one per pyramid level / RoI level):
        the SqueezeExcites of depth i run for ALL towers in one launch pair and their convs in one multi-problem launch,
        so the few-tile problems of the coarse levels ride along with the fine level instead of each being a
        latency-bound launch of its own.  Separable units (MobileSeparableConv2D) run level by level within their depth.
        Falls back to tower-major order when the towers are not made of the same depth units.
        tape: None, or a dict that receives what the backward needs -- per depth, every level's conv input ("conv_in") and
        post-ReLU conv output ("conv_out"); GroupNormalization then writes a tensor of its own instead of normalising the
        conv output in place (the same bits).  Towers of [Conv2D, GroupNormalization] units only."""
        units = [_TowerMixin._units(b) for b in blocks]
        if tape is not None:
            _TowerMixin._check_tape_units(units, lives)
            tape["conv_in"], tape["conv_out"] = [], []
        same = (all(u is not None for u in units) and len({len(u) for u in units}) == 1 and
                all(len({(se is None, type(c)) for se, c, _ in (u[d] for u in units)}) == 1 for d in range(len(units[0]))))
        if not same:
            if lives is not None:
                raise NotImplementedError("fixed-capacity RoI batches: towers of [SqueezeExcite?, Conv2D | "
                                          "MobileSeparableConv2D, GroupNormalization] units only")
            return [_TowerMixin._run_tower(b, x) for b, x in zip(blocks, xs)]
        inputs = list(xs)                  # the caller's tensors: never modified in place
        xs = list(xs)
        lives = lives if lives is not None else [None] * len(xs)
        no_lives = all(lv is None for lv in lives)
        for d in range(len(units[0])):
            ses = [u[d][0] for u in units]
            convs = [u[d][1] for u in units]
            norms = [u[d][2] for u in units]
            if ses[0] is not None:
                xs = SqueezeExcite.call_multi(ses, xs, lives=None if no_lives else lives,
                                              keep_input=[x is x0 for x, x0 in zip(xs, inputs)])
            if isinstance(convs[0], MobileSeparableConv2D):
                xs = [c(x, live=lv) for c, x, lv in zip(convs, xs, lives)]
                xs = GroupNormalization.call_multi(norms, xs, inplace=True, lives=None if no_lives else lives)
                continue
            # levels whose GroupNorm chunks are whole conv tiles take their statistics from the conv's epilogue
            parts = [None] * len(xs)
            if no_lives:
                geo = [_TowerMixin._conv_tiles(c, x) for c, x in zip(convs, xs)]
                launch_tiles = sum(t for t, _ in geo)
                for k, (c, g, x, (t, oshape)) in enumerate(zip(convs, norms, xs, geo)):
                    tpc = ops.gn_fusable(oshape, c.filters, g.groups, c.dev, launch_tiles, x.dtype)
                    if tpc:
                        parts[k] = (torch.empty((t, 4, 2), dtype=torch.float64, device=x.device), tpc)
            if tape is not None:
                tape["conv_in"].append(list(xs))
            xs = ops.conv2d_multi([dict(x=x, dc=c.dev, stride=c.strides[0], padding=c.padding,
                                        dilation=c.dilation_rate[0], act=ops._lib.ACT_BY_NAME[c.activation], live=lv,
                                        gn_partials=None if pt is None else pt[0])
                                   for c, x, lv, pt in zip(convs, xs, lives, parts)])
            if tape is not None:
                tape["conv_out"].append(list(xs))
            xs = GroupNormalization.call_multi(norms, xs, inplace=tape is None, lives=None if no_lives else lives,
                                               partials=None if all(pt is None for pt in parts) else parts)
        return xs

    @staticmethod
    def _check_tape_units(units, lives=None):
        """What the towers' backward is built for: [Conv2D(3x3, relu), GroupNormalization] units, the same depth everywhere"""
        if any(u is None for u in units) or len({len(u) for u in units}) != 1 or lives is not None:
            raise NotImplementedError("tower backward: towers of [Conv2D, GroupNormalization] depth units only")
        for u in units:
            for se, conv, _ in u:
                if se is not None:
                    raise NotImplementedError(f"tower backward: SqueezeExcite ('{se.name}') has no backward")
                if isinstance(conv, MobileSeparableConv2D):
                    raise NotImplementedError(f"tower backward: MobileSeparableConv2D ('{conv.name}') has no backward")
                if conv.activation != 'relu':
                    raise NotImplementedError(f"tower backward: '{conv.name}' must end in a ReLU (the mask comes from the "
                                              f"GroupNormalization behind it)")

    @staticmethod
    def _towers_backward(units, tape, dxs, grads, need_dx=True):
        """The depth units of several towers, deepest depth first: GroupNormalization.backward_multi(input_relu=True, in place
        on `dxs`, the gradients at the towers' outputs) -> conv2d_wgrad_multi -> conv2d_dgrad_multi.  tape: "conv_in" /
        "conv_out" per depth and level, as _run_towers_multi / _run_tower record them.  Fills `grads` with the units' weights.
        -> the gradients at the towers' inputs (None with need_dx=False: the first depth's data gradient is not run)."""
        for depth in range(len(units[0]) - 1, -1, -1):
            convs = [u[depth][1] for u in units]
            norms = [u[depth][2] for u in units]
            for c in convs:
                c._check_backward()
            back = GroupNormalization.backward_multi(norms, tape["conv_out"][depth], dxs, input_relu=True, inplace=True)
            for g, (_, gg) in zip(norms, back):
                g.name_grads(gg, grads)
            dys = [dx for dx, _ in back]                     # at the convs' pre-activation
            xs = tape["conv_in"][depth]
            pairs = ops.conv2d_wgrad_multi([dict(x=x, dy=dy, want_bias=c.use_bias, **c._grad_args())
                                            for c, x, dy in zip(convs, xs, dys)])
            for c, pair in zip(convs, pairs):
                c.name_grads(pair_grads(c, pair), grads)
            if depth == 0 and not need_dx:
                return None
            dxs = ops.conv2d_dgrad_multi([dict(dy=dy, in_hw=(x.shape[1], x.shape[2]), **c._grad_args())
                                          for c, x, dy in zip(convs, xs, dys)])
        return dxs

    @staticmethod
    def _build_chain(block, shape):
        for layer in block:
            shape = layer.build(shape)
        return shape


class BoxRegressionSubNet(Layer, _TowerMixin):
    """Box Regression Module in RetinaMask (reference :89-155); one un-shared block per level."""

    def __init__(self, num_blocks, num_depth=4, num_features=256, num_priors=9, use_separable_conv=False,
                 expand_ratio=4., use_squeeze_excite=False, squeeze_ratio=16., groups=16, **kwargs):
        self.num_blocks = num_blocks
        self.num_depth = num_depth
        self.num_features = num_features
        self.num_priors = num_priors
        self.use_separable_conv = use_separable_conv
        self.expand_ratio = expand_ratio
        self.use_squeeze_excite = use_squeeze_excite
        self.squeeze_ratio = squeeze_ratio
        self.groups = groups
        super().__init__(**kwargs)
        self.out_dim = 4
        self.blocks = []
        for idx in range(self.num_blocks):
            prefix = f'{self.name}/block{idx}'
            block = self._make_tower(prefix, num_depth, num_features, groups, use_separable_conv, expand_ratio,
                                     use_squeeze_excite, squeeze_ratio)
            block.append(self._output_conv(prefix))
            self.blocks.append(block)

    def _output_conv(self, prefix):
        return Conv2D(self.num_priors * 4, (3, 3), padding='same', kernel_initializer='normal',
                      kernel_stddev=0.01, name=f'{prefix}/output')

    def build(self, input_shapes):
        for block, shape in zip(self.blocks, input_shapes):
            self._build_chain(block, shape)
        self.built = True
        return (input_shapes[0][0], None, self.out_dim)

    def children(self):
        return [l for b in self.blocks for l in b]

    def call(self, inputs, **kwargs):
        return self._forward(inputs)

    def _pred_views(self, shapes):
        """Every level's row range of the [B, A, d] prediction as (element offset, channel stride, batch stride)"""
        d = self.out_dim
        per_level = [int(s[1]) * int(s[2]) * self.num_priors for s in shapes]
        total = sum(per_level)
        views, off = [], 0
        for n in per_level:
            views.append((off * d, self.num_priors * d, total * d))
            off += n
        return views, total

    def _forward(self, inputs, tape=None):
        """The one forward of `call` (tape None) and `call_with_tape` (tape: a dict that receives what `backward` needs;
        GroupNormalization then writes a tensor of its own instead of normalising in place: _run_towers_multi)."""
        # Reshape((-1, d)) + Concatenate(axis=1) (reference :138-140) are fused: every level's
        # output conv writes straight into its row range of the [B, A, d] prediction.
        views, total = self._pred_views([x.shape for x in inputs])      # the towers keep every level's height and width
        pred = torch.empty((inputs[0].shape[0], total, self.out_dim), dtype=torch.float32, device=inputs[0].device)
        blocks = self.blocks[:len(inputs)]
        if tape is not None:
            tape["inputs"] = list(inputs)
        xs = self._run_towers_multi([b[:-1] for b in blocks], inputs, tape=tape)
        if tape is not None:
            tape["out_in"] = list(xs)
        ops.conv2d_multi([dict(x=x, dc=b[-1].dev, stride=1, padding='same', act=ops._lib.ACT_BY_NAME[b[-1].activation],
                               out_view=(pred,) + view) for b, x, view in zip(blocks, xs, views)])
        return pred

    def call_with_tape(self, inputs, **kwargs):
        """`call` that keeps what `backward` needs.  -> (pred, tape): pred is `call`'s bit for bit; the tape holds every depth's
        conv input and post-ReLU conv output per level, and the output convs' inputs.  GroupNormalization writes a tensor
        of its own here (inplace=False) where `call` normalises in place; the epilogue-statistics path is kept where `call`
        uses it.  Towers with SqueezeExcite or separable units raise NotImplementedError."""
        tape = {}
        return self._forward(inputs, tape), tape

    def backward(self, tape, d_pred):
        """Backward of `call_with_tape`: d_pred [B, A, d] float32 is the gradient at the PRE-activation of the prediction (the
        box head is linear; the class head's sigmoid is the loss's: loss_and_gradients(wrt="pre_activation")).
        The output convs read it as views (one weight-gradient launch, one data-gradient launch); then, deepest depth
        first: GroupNormalization.backward_multi(input_relu=True, in place) -> conv2d_wgrad_multi -> conv2d_dgrad_multi.
        -> (the gradients at `inputs`, one per level; {full weight name: gradient} with the names of init_weights():
        .../conv{i}/kernel, /bias, .../gn{i}/gamma, /beta, .../output/kernel, /bias -- what apply_gradients takes)."""
        n = len(tape["inputs"])
        blocks = self.blocks[:n]
        units = [self._units(b[:-1]) for b in blocks]
        self._check_tape_units(units)
        views, total = self._pred_views([x.shape for x in tape["out_in"]])
        check_incoming_grad(f"{type(self).__name__}.backward: d_pred", d_pred,
                            (int(tape["inputs"][0].shape[0]), total, self.out_dim))
        grads = {}
        outs = [b[-1] for b in blocks]
        for c in outs:
            c._check_backward()
        pairs = ops.conv2d_wgrad_multi([dict(x=x, dy=None, dy_view=(d_pred,) + v, want_bias=c.use_bias, **c._grad_args())
                                        for c, x, v in zip(outs, tape["out_in"], views)])
        for c, pair in zip(outs, pairs):
            c.name_grads(pair_grads(c, pair), grads)
        dxs = ops.conv2d_dgrad_multi([dict(dy=None, dy_view=(d_pred,) + v, in_hw=(x.shape[1], x.shape[2]), **c._grad_args())
                                      for c, x, v in zip(outs, tape["out_in"], views)])
        return self._towers_backward(units, tape, dxs, grads), grads

    def get_config(self):
        config = super().get_config()
        config.update({
            "num_blocks": self.num_blocks, "num_depth": self.num_depth, "num_features": self.num_features,
            "num_priors": self.num_priors, "use_separable_conv": self.use_separable_conv,
            "expand_ratio": self.expand_ratio, "use_squeeze_excite": self.use_squeeze_excite,
            "squeeze_ratio": self.squeeze_ratio, 'groups': self.groups})
        return config


class ClassificationSubNet(BoxRegressionSubNet):
    """Classifcation Module in RetinaMask (reference :158-228): sigmoid outputs, bias -log(99)."""

    def __init__(self, num_blocks, num_classes, num_depth=4, num_features=256, num_priors=9,
                 use_separable_conv=False, expand_ratio=4., use_squeeze_excite=False, squeeze_ratio=16.,
                 groups=16, **kwargs):
        self.num_classes = num_classes
        super().__init__(num_blocks, num_depth=num_depth, num_features=num_features, num_priors=num_priors,
                         use_separable_conv=use_separable_conv, expand_ratio=expand_ratio,
                         use_squeeze_excite=use_squeeze_excite, squeeze_ratio=squeeze_ratio, groups=groups, **kwargs)
        self.out_dim = num_classes

    def _output_conv(self, prefix):
        return Conv2D(self.num_priors * self.num_classes, (3, 3), padding='same', activation='sigmoid',
                      kernel_initializer='normal', kernel_stddev=0.01,
                      bias_value=float(-np.log((1 - 0.01) / 0.01)), name=f'{prefix}/output')

    def get_config(self):
        config = super().get_config()
        config.update({"num_classes": self.num_classes})
        return config


class PriorLayer(Layer):
    """Prior boxes for the image size (reference :236-306).  The table depends only on (H, W), so it
    is built once on the host (PriorBoxes.anchors) and cached on the device as int32 [A,4]."""

    def __init__(self, prior, padding='same', **kwargs):
        if isinstance(prior, dict):
            self.prior = PriorBoxes(**prior)
        elif isinstance(prior, PriorBoxes):
            self.prior = prior
        else:
            raise ValueError('prior must be an instance of the PriorBoxes class.')
        self.padding = padding
        kwargs.update({"trainable": False})
        super().__init__(**kwargs)
        self._cache = {}

    def anchors(self, height, width, device):
        key = (int(height), int(width), str(device))
        if key not in self._cache:
            self._cache[key] = torch.from_numpy(self.prior.anchors(height, width, self.padding)).to(device)
        return self._cache[key]

    def call(self, inputs, **kwargs):
        B, H, W = inputs.shape[0], inputs.shape[1], inputs.shape[2]
        a = self.anchors(H, W, inputs.device)
        return a.unsqueeze(0).expand(B, -1, -1)     # K.repeat + transpose (reference :296-297) as a view

    def get_config(self):
        config = super().get_config()
        config.update({"prior": self.prior.config, 'padding': self.padding})
        return config


class RestoreBoxes(Layer):
    """(loc_pred, pr_boxes) -> (cx,cy,w,h) (reference :309-344)."""

    def call(self, inputs, **kwargs):
        loc_pred, pr_boxes = inputs[0], inputs[1]
        priors = pr_boxes[0] if pr_boxes.dim() == 3 else pr_boxes   # shared by the batch
        return ops.restore_boxes(loc_pred.contiguous(), priors.contiguous().to(torch.int32))


class NormalizeBoxes(Layer):
    """(cx,cy,w,h) -> normalised (y1,x1,y2,x2) (reference :347-375).  On the hot path this is
    fused into the NMS / RoI kernels; the standalone layer is tiny index arithmetic on <= B*N
    boxes and is evaluated with torch elementwise ops."""

    def call(self, inputs, **kwargs):
        shape = kwargs.get('shape', (1.0, 1.0))
        ih, iw = float(shape[0]), float(shape[1])
        cx, cy, w, h = inputs[..., 0], inputs[..., 1], inputs[..., 2], inputs[..., 3]
        return torch.stack([(cy - h / 2) / ih, (cx - w / 2) / iw, (cy + h / 2) / ih, (cx + w / 2) / iw], dim=-1)


class DetectionProposal(Layer):
    """Threshold -> per-(image,class) NMS -> per-image cross-class NMS -> [B,N,6] rows
    (cx,cy,w,h,class id,confidence), -1 padded (reference :435-578).  The device path is fixed
    capacity (N = nms_max_output_size); `call` trims to the reference's dynamic N = max(1, max count)
    with ONE tiny device->host read of the per-image counts."""

    def __init__(self, min_confidence=0.05, nms_iou_threshold=0.4, post_iou_threshold=0.65,
                 nms_max_output_size=1000, max_batch_size=64, **kwargs):
        self.min_confidence = min_confidence
        self.nms_iou_threshold = nms_iou_threshold
        self.post_iou_threshold = post_iou_threshold
        self.nms_max_output_size = nms_max_output_size
        self.max_batch_size = max_batch_size
        super().__init__(**kwargs)

    def propose_fixed(self, cls_pred, boxes, want_kept=False, want_payload=False):
        """-> proposed [B,cap,6] (-1 padded), counts [B] int32 (device), kept [B,cap,2] or None
        [, payload [B,cap*6+1]: the all-gather record, see parallel.all_gather_detections]."""
        if cls_pred.shape[0] > 32 and self.max_batch_size is not None:
            raise ValueError("DetectionProposal: MoldBatch supports at most 32 images per call "
                             "(reference misc.py:275); shard larger batches")
        return ops.detection_proposal(cls_pred.contiguous(), boxes.contiguous(), self.min_confidence,
                                      self.nms_iou_threshold, self.post_iou_threshold,
                                      self.nms_max_output_size, want_kept=want_kept, want_payload=want_payload)

    def call(self, inputs, **kwargs):
        cls_pred, boxes = inputs[0], inputs[1]
        proposed, counts, _ = self.propose_fixed(cls_pred, boxes)
        n = max(1, max(counts.tolist()))          # the dynamic N of the reference (MoldBatch): B ints read by the host
        return proposed[:, :n].contiguous()

    def get_config(self):
        config = super().get_config()
        config.update({
            "min_confidence": self.min_confidence, "nms_iou_threshold": self.nms_iou_threshold,
            "post_iou_threshold": self.post_iou_threshold, "nms_max_output_size": self.nms_max_output_size,
            "max_batch_size": self.max_batch_size})
        return config


class CalculateIOU(Layer):
    """IoU of every pair of two (cx,cy,w,h) box tables (reference :378-422): inputs = [aa_boxes [n, >=4], bb_boxes [m, >=4]]
    -> float32 [n,m], with the reference's + 1e-5 in the denominator.  AssignBoxes, AssignMasks and DetectionIOUMetric
    evaluate the same arithmetic inside their own kernels and never build the matrix."""

    def call(self, inputs, **kwargs):
        aa_boxes, bb_boxes = inputs[0], inputs[1]
        return ops.calculate_iou(aa_boxes.to(torch.float32).contiguous(), bb_boxes.to(torch.float32).contiguous())


class AssignBoxes(Layer):
    """Ground-truth boxes -> per-prior targets (reference :589-697): inputs = [gt_boxes [B,G,6] (-1 padded), pr_boxes
    [B,A,4]] -> (cls_true [B,A,C], loc_true [B,A,4], assign_mask [B,A,1]) float32.  The reference's rule, restated per prior
    (include/masklab_hip.h, "Trainer forward"); pr_boxes[0] serves the whole batch, as in the reference."""

    def __init__(self, num_classes, **kwargs):
        self.num_classes = num_classes
        super().__init__(**kwargs)

    def call(self, inputs, **kwargs):
        gt_boxes, pr_boxes = inputs[0], inputs[1]
        priors = pr_boxes[0] if pr_boxes.dim() == 3 else pr_boxes
        priors = priors.contiguous().to(torch.int32)
        gt_boxes = gt_boxes.to(torch.float32).contiguous()
        self.last_best = ops.best_prior(gt_boxes, priors)
        return ops.assign_boxes(gt_boxes, priors, self.num_classes, best=self.last_best)

    def get_config(self):
        config = super().get_config()
        config.update({"num_classes": self.num_classes})
        return config
