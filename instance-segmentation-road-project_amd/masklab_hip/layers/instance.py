"""Instance-segmentation layers -- drop-ins for reference engine/layers/instance.py:
MaskDistribute :32-74, PyramidRoiAlign :77-147, MaskSubNet :158-240."""
import torch

from .. import ops
from ..keras_like import Conv2D, Conv2DTranspose, Layer, check_incoming_grad, pair_grads
from .detection import _TowerMixin


class MaskDistribute(Layer):
    """Pick the pyramid level of every box from its size (reference :32-74):
    k = clip(floor(log2((sqrt(w*h)+eps)/(base+eps))), 0, max_k); k = -1 for padded rows."""

    def __init__(self, max_k=2, base_size=64, **kwargs):
        self.max_k = max_k
        self.base_size = base_size
        super().__init__(**kwargs)

    def call(self, inputs, **kwargs):
        inputs = inputs.contiguous()
        _, _, _, kvals = ops.mask_distribute(inputs, self.max_k, self.base_size, has_k=False, want_k=True)
        # Concatenate([k, boxes], axis=-1) (:66): data movement of a [B,N,7] table, off the fused hot path
        # (InferenceModel consumes the level slots directly and never builds dist_boxes)
        return torch.cat([kvals[..., None], inputs], dim=-1)

    def get_config(self):
        config = super().get_config()
        config.update({"max_k": self.max_k, "base_size": self.base_size})
        return config


class PyramidRoiAlign(Layer):
    """Per level: crop_and_resize the boxes assigned to it and mold by image with -1 padding
    (reference :77-147).  NOTE: one bilinear sample per output cell (tf.image.crop_and_resize),
    boxes normalised by the IMAGE (H, W)."""

    def __init__(self, crop_size=(14, 14), max_batch_size=64, **kwargs):
        self.crop_size = crop_size
        self.max_batch_size = max_batch_size
        super().__init__(**kwargs)

    def distribute(self, n_levels, rows, has_k, base_size=1.0):
        """Enqueue the level assignment + per-level slot lists (no host read)."""
        if rows.shape[0] > 32 and self.max_batch_size is not None:
            raise ValueError("PyramidRoiAlign: MoldBatch supports at most 32 images per call")
        slots, lcounts, lmax, _ = ops.mask_distribute(rows, n_levels - 1, base_size, has_k=has_k)
        return slots, lcounts, lmax

    def crop_distributed(self, fmap_outputs, rows, image_hw, slots, lcounts, lmax):
        """One device->host read (`lmax`: the per-level maxima the distribute kernel wrote, L ints) sizes the
        molded outputs like the reference's dynamic shapes; callers enqueue independent work (the semantic
        head) before calling this."""
        B = rows.shape[0]
        n_l = [max(1, int(v)) for v in lmax.tolist()]     # the single sync
        total = sum(n_l)
        roi_boxes = torch.empty((B, total, 6), dtype=torch.float32, device=rows.device)
        roi_fmaps, off = [], 0
        for level, fmap in enumerate(fmap_outputs):
            roi_fmaps.append(ops.roi_crop_resize(fmap, rows, slots, lcounts, level, n_l[level],
                                                 tuple(self.crop_size), image_hw, roi_boxes, off))
            off += n_l[level]
        return roi_fmaps, roi_boxes

    def crop_capacity(self, fmap_outputs, rows, image_hw, slots, lcounts, lmax):
        """The same crops with NO host read: every level is launched at capacity (n_l = cap RoI slots per image) and the
        kernels skip the slots past the level's maximum, which they read from `lmax` on the device.
        -> (roi_fmaps per level [B,cap,ch,cw,C], roi_boxes_cap [B,L*cap,6], lives = [(lmax[l:l+1], cap)])."""
        B, cap = rows.shape[0], rows.shape[1]
        L = len(fmap_outputs)
        roi_boxes = torch.empty((B, L * cap, 6), dtype=torch.float32, device=rows.device)
        roi_fmaps, lives = [], []
        for level, fmap in enumerate(fmap_outputs):
            live = lmax[level:level + 1]
            roi_fmaps.append(ops.roi_crop_resize(fmap, rows, slots, lcounts, level, cap, tuple(self.crop_size), image_hw,
                                                 roi_boxes, level * cap, live=live))
            lives.append((live, cap))
        return roi_fmaps, roi_boxes, lives

    def crop_levels(self, fmap_outputs, rows, image_hw, has_k, base_size=1.0):
        """rows: [B,cap,6] proposals (has_k=False) or [B,cap,7] dist_boxes (has_k=True)."""
        slots, lcounts, lmax = self.distribute(len(fmap_outputs), rows, has_k, base_size)
        return self.crop_distributed(fmap_outputs, rows, image_hw, slots, lcounts, lmax)

    def backward(self, grad_roi_fmaps, fmap_shapes, rows, image_hw, slots, lcounts, add=None, out=None):
        """The gradient at the pyramid levels from the gradients at the molded crops of crop_distributed (sized) or
        crop_capacity ([B,cap,...]): one launch for all levels (ops.roi_crop_resize_grad).  rows / slots / lcounts: what
        the forward used; the boxes carry no gradient.  add / out: per level, out = add + gradient (a level also
        receives the gradients of the two towers)."""
        return ops.roi_crop_resize_grad(grad_roi_fmaps, fmap_shapes, rows, slots, lcounts, tuple(self.crop_size), image_hw,
                                        add=add, out=out)

    def call(self, inputs, **kwargs):
        fmap_outputs, dist_boxes, images = inputs[0], inputs[1], inputs[2]
        image_hw = (int(images.shape[1]), int(images.shape[2]))
        roi_fmaps, roi_boxes = self.crop_levels(fmap_outputs, dist_boxes.contiguous(), image_hw, has_k=True)
        return [roi_fmaps, roi_boxes]

    def get_config(self):
        config = super().get_config()
        config.update({"crop_size": self.crop_size, "max_batch_size": self.max_batch_size})
        return config


class MaskSubNet(Layer, _TowerMixin):
    """Mask Prediction Module In RetinaMask (reference :158-240): per level (own weights)
    depth x [Conv3x3+ReLU ; GN] ; Conv2DTranspose 2x2 s2 + ReLU ; Conv1x1 + sigmoid."""

    def __init__(self, num_blocks, num_classes, num_depth=4, num_features=256, use_separable_conv=False,
                 expand_ratio=4., use_squeeze_excite=False, squeeze_ratio=16., groups=16, **kwargs):
        self.num_blocks = num_blocks
        self.num_classes = num_classes
        self.num_depth = num_depth
        self.num_features = num_features
        self.use_separable_conv = use_separable_conv
        self.expand_ratio = expand_ratio
        self.use_squeeze_excite = use_squeeze_excite
        self.squeeze_ratio = squeeze_ratio
        self.groups = groups
        super().__init__(**kwargs)
        self.blocks = []
        for idx in range(self.num_blocks):
            prefix = f'{self.name}/block{idx}'
            block = self._make_tower(prefix, num_depth, num_features, groups, use_separable_conv, expand_ratio,
                                     use_squeeze_excite, squeeze_ratio)
            block.append(Conv2DTranspose(num_features, (2, 2), (2, 2), padding='same', activation='relu',
                                         kernel_stddev=0.01, name=f'{prefix}/deconv'))
            block.append(Conv2D(num_classes, (1, 1), padding='same', activation='sigmoid',
                                kernel_initializer='normal', kernel_stddev=0.01, name=f'{prefix}/output'))
            self.blocks.append(block)

    def build(self, input_shapes):
        if not isinstance(input_shapes, list):
            input_shapes = [input_shapes]
        out = None
        for block, shape in zip(self.blocks, input_shapes):
            s = (None,) + tuple(shape[2:]) if len(shape) == 5 else tuple(shape)
            out = self._build_chain(block, s)
        self.built = True
        return (input_shapes[0][0], None) + tuple(out[1:])

    def children(self):
        return [l for b in self.blocks for l in b]

    def load_weights(self, weights, device):
        super().load_weights(weights, device)
        # the 1x1 output kernels once more, in the lane order of the fused tail kernel (csrc/deconv_out.hip)
        from .. import packing
        self._tail_tables, self._tail_wo = [], []
        for block in self.blocks:
            deconv, out = block[-2], block[-1]
            p = deconv.dev.p
            ok = (p.span == p.span_pad and p.n_pad == p.cout and p.cout // 4 in (128, 256) and self.num_classes <= 32
                  and out.kernel_size == (1, 1) and out.strides == (1, 1))
            if not ok:
                self._tail_tables = None
                break
            k, b = out.folded(weights)
            table, bo, _ = packing.pack_out1x1_table(k, b)
            self._tail_tables.append((torch.from_numpy(table).to(device), torch.from_numpy(bo).to(device)))
            self._tail_wo.append(torch.from_numpy(k.copy()).to(device))       # [1,1,C_mid,ncls] as it is: the backward's operand

    def device_params(self):
        """The output convs' kernels are the very tensors the tail's backward reads (`_tail_wo`): they become those convs'
        masters, so one step moves the conv packing, the lane table and the backward's operand together."""
        if getattr(self, "_tail_tables", None) is not None:
            for block, wo in zip(self.blocks, self._tail_wo):
                block[-1].bind_params(kernel=wo)
        return super().device_params()

    def _own_repack_jobs(self):
        if getattr(self, "_tail_tables", None) is None:
            return []
        jobs = []
        for block, wo, (table, bo) in zip(self.blocks, self._tail_wo, self._tail_tables):
            out = block[-1]
            if out.dev is not None and out.dev.follows_master and getattr(out, "_params_of", None) is out.dev:
                jobs.append(ops.repack_table_job(out._params["kernel"], out._params.get("bias"), table, bo))
        return jobs

    def _fused_tail(self, blocks, xs, shapes, roi_masks, per_roi, lives=None, tape=None):
        """Conv2DTranspose + ReLU -> Conv2D 1x1 + sigmoid of every level in one launch, written straight into
        `roi_masks` (csrc/deconv_out.hip); False when the configuration is outside that kernel's shapes."""
        from .. import _lib
        if getattr(self, "_tail_tables", None) is None or ops.CONV_MATH == "f16":
            return False
        if any(x.shape[0] * x.shape[1] * x.shape[2] >= 1 << 24 for x in xs):
            return False
        if xs[0].dtype == torch.float16 and any(x.shape[-1] % 64 for x in xs):
            return False
        problems, off = [], 0
        for i, ((_, n), b, x) in enumerate(zip(shapes, blocks, xs)):
            table, bo = self._tail_tables[i]
            problems.append(dict(x=x.contiguous(), dc=b[-2].dev, wo_table=table, bo=bo, out=roi_masks,
                                 out_base=off * per_roi, rois_per_image=n,
                                 live=None if lives is None else lives[i][0]))
            off += n
        ops.deconv2x2_out1x1_multi(problems, self.num_classes, _lib.ACT_BY_NAME[blocks[0][-2].activation],
                                   _lib.ACT_BY_NAME[blocks[0][-1].activation], tape=tape)
        return True

    def capacity_supported(self, crop_size):
        """True when the whole head runs in the fixed-capacity form (towers of [SqueezeExcite?, Conv2D |
        MobileSeparableConv2D, GroupNormalization] units + the fused tail kernel)."""
        towers = all(len(b) >= 2 and self._units(b[:-2]) is not None for b in self.blocks)
        return towers and getattr(self, "_tail_tables", None) is not None and crop_size[0] * crop_size[1] >= 2

    def call(self, inputs, lives=None, **kwargs):
        """lives (fixed-capacity form, PyramidRoiAlign.crop_capacity): per level (device int32 [1], cap) -- RoI slots past
        max(1, live) of an image do not exist; the result is then [B, L*cap, 2h, 2w, classes] with level l's RoIs at
        rows l*cap .. (molded by ops.mold_levels once the host knows the maxima)."""
        return self._forward(inputs, lives)

    def _forward(self, inputs, lives=None, tape=None):
        """The one forward of `call` (tape None) and `call_with_tape` (tape: a dict that receives what `backward` needs; the
        towers' GroupNormalization then writes tensors of its own instead of normalising in place, the fused tail stores
        T, and what keeps no tape is refused before anything runs)."""
        if not isinstance(inputs, list):
            inputs = [inputs]
        if tape is not None:
            if lives is not None:
                raise NotImplementedError("MaskSubNet.call_with_tape: the fixed-capacity form (`lives`) keeps no tape")
            self._check_train("call_with_tape", inputs)
            if any(h.shape[1] < 1 for h in inputs):
                raise ValueError("MaskSubNet.call_with_tape: every level needs at least one RoI per image")
            if any(h.shape[0] * h.shape[1] * h.shape[2] * h.shape[3] >= 1 << 24 for h in inputs):
                raise NotImplementedError("MaskSubNet.call_with_tape: 2^24 or more input pixels in a level are outside the fused tail")
        from .. import _lib
        blocks = self.blocks[:len(inputs)]
        shapes = [(int(h.shape[0]), int(h.shape[1])) for h in inputs]
        # fold rois into the batch (:211-213); all levels advance together (multi-problem launches)
        xs = [h.reshape((h.shape[0] * h.shape[1],) + tuple(h.shape[2:])) for h in inputs]
        if tape is not None:
            tape.update(inputs=list(inputs), shapes=shapes)
        xs = self._run_towers_multi([b[:-2] for b in blocks], xs, lives=lives, tape=tape)
        if tape is not None:
            tape.update(tail_in=list(xs), T=[])
        if all(n > 0 for _, n in shapes):
            B = shapes[0][0]
            oh, ow, ncls = 2 * int(xs[0].shape[1]), 2 * int(xs[0].shape[2]), self.num_classes
            total = sum(n for _, n in shapes)
            roi_masks = torch.empty((B, total, oh, ow, ncls), dtype=torch.float32, device=xs[0].device)
            if self._fused_tail(blocks, xs, shapes, roi_masks, oh * ow * ncls, lives=lives,
                                tape=None if tape is None else tape["T"]):
                return roi_masks
        if tape is not None:
            raise NotImplementedError("MaskSubNet.call_with_tape: this configuration is outside the fused tail kernel")
        if lives is not None:
            raise NotImplementedError("MaskSubNet: the fixed-capacity form needs the fused tail kernel")
        if xs[0].dtype == torch.float16:          # (the pixel-shuffle epilogue of the unfused pair is fp32 only)
            xs = [ops.cast_h2f(x) for x in xs]
        xs = ops.conv2d_multi([dict(x=x, dc=b[-2].dev, act=_lib.ACT_BY_NAME[b[-2].activation])
                               for b, x in zip(blocks, xs)])                    # Conv2DTranspose + ReLU
        # unfold + Concatenate(axis=1) (:222-225) fused into the output convs: level l's [B*n_l, h, w, classes] maps
        # land at rows [off_l, off_l + n_l) of every image of roi_masks through a per-image strided view.  The
        # view's "image" is one RoI-level block: problem (b, level) would need B problems per level, so instead the
        # conv's batch axis is the IMAGE (n_l RoIs of one image are n_l*h rows of a [B, n_l*h, w, classes] map).
        B = shapes[0][0]
        oh, ow = int(xs[0].shape[1]), int(xs[0].shape[2])
        ncls = self.num_classes
        total = sum(n for _, n in shapes)
        roi_masks = torch.empty((B, total, oh, ow, ncls), dtype=torch.float32, device=xs[0].device)
        per_roi = oh * ow * ncls
        problems, off = [], 0
        for (_, n), b, x in zip(shapes, blocks, xs):
            xv = x.reshape(B, n * oh, ow, x.shape[3])          # a view: RoIs of one image stacked along H (1x1 conv)
            problems.append(dict(x=xv, dc=b[-1].dev, stride=1, padding=b[-1].padding,
                                 act=_lib.ACT_BY_NAME[b[-1].activation],
                                 out_view=(roi_masks, off * per_roi, ncls, total * per_roi)))
            off += n
        ops.conv2d_multi(problems)
        return roi_masks

    def _check_train(self, what, xs):
        """What call_with_tape / backward are built for: float32 tensors under exact or f32x3 products on the fused tail"""
        if ops.CONV_MATH == "f16" or any(x.dtype != torch.float32 for x in xs):
            raise NotImplementedError(f"MaskSubNet.{what}: float32 tensors only (no half tensors, no set_conv_math('f16'))")
        if getattr(self, "_tail_tables", None) is None:
            raise NotImplementedError(f"MaskSubNet.{what}: this configuration is outside the fused tail kernel (transposed-conv "
                                      f"filters 128 or 256 on an input width that is a multiple of 32, at most 32 classes)")
        for b in self.blocks:
            if b[-2].activation != 'relu' or b[-1].activation != 'sigmoid':
                raise NotImplementedError(f"MaskSubNet.{what}: the tail must be Conv2DTranspose + ReLU -> Conv2D 1x1 + sigmoid")

    def call_with_tape(self, inputs, lives=None, **kwargs):
        """`call` that keeps what `backward` needs.  -> (roi_masks, tape): roi_masks is `call`'s bit for bit; the tape holds
        the towers' tape of _run_towers_multi(tape=) (every depth's conv input and post-ReLU conv output per level), the
        towers' outputs ("tail_in") and, per level, T = the transposed conv's post-ReLU output [R h w, 4, C_mid] float32
        in GEMM layout, which the fused tail's tape launch stores.  Refused by name: the
        fixed-capacity form, half tensors / set_conv_math('f16'), configurations outside the fused tail, towers with
        SqueezeExcite or separable units."""
        tape = {}
        return self._forward(inputs, lives, tape), tape

    def backward(self, tape, d_masks, need_dx=True, consume_tape=False):
        """Backward of `call_with_tape`: d_masks [B, total, 2h, 2w, classes] float32 is the gradient at the PRE-activation of
        roi_masks (the sigmoid is the loss's: MaskLoss.call_with_grad(through_sigmoid=True)).  Order of work: the tail of
        every level in one launch (ops.deconv2x2_out1x1_grad_multi: dT, and the 1x1 output conv's gradients, in one pass over
        T); the transposed conv as the 1x1 conv [1,1,cin,4 C_mid] it is on dT in GEMM layout -- one conv2d_wgrad_multi, one
        conv2d_dgrad_multi, the weight gradient brought back to [2,2,C_mid,cin] / [C_mid]; then _towers_backward.
        consume_tape: dT overwrites T (no T-sized allocation; the tape cannot be used again).
        -> (the gradients at `inputs`, one [B,n_l,h,w,C] per level, or None with need_dx=False: the first depth's data
        gradient is not run and the weight gradients are the same bits; {full weight name: gradient} with the names of
        init_weights(): .../conv{i}/kernel, /bias, .../gn{i}/gamma, /beta, .../deconv/kernel, /bias, .../output/kernel, /bias
        -- what apply_gradients takes)."""
        n = len(tape["inputs"])
        blocks = self.blocks[:n]
        units = [self._units(b[:-2]) for b in blocks]
        self._check_tape_units(units)
        check_incoming_grad("MaskSubNet.backward: d_masks", d_masks)      # its shape once the tape itself is known good
        if tape.get("T") is None or len(tape["T"]) != n:
            raise ValueError("MaskSubNet.backward: the tape holds no T (consumed by an earlier backward?)")
        self._check_train("backward", tape["T"])
        xs, shapes = tape["tail_in"], tape["shapes"]
        B, total = shapes[0][0], sum(s[1] for s in shapes)
        h, w = int(xs[0].shape[1]), int(xs[0].shape[2])
        ncls = self.num_classes
        check_incoming_grad("MaskSubNet.backward: d_masks", d_masks, (B, total, 2 * h, 2 * w, ncls))
        deconvs, outs = [b[-2] for b in blocks], [b[-1] for b in blocks]
        for c in outs:
            c._check_backward()
        for c in deconvs:
            if getattr(c, "dev1x1", None) is None:
                raise RuntimeError(f"layer '{c.name}' has no weights loaded")
        grads = {}
        per_roi = 4 * h * w * ncls
        problems, off = [], 0
        for i, (_, n_l) in enumerate(shapes):
            problems.append(dict(dy=d_masks, T=tape["T"][i], wo=self._tail_wo[i], hw=(h, w), rois_per_image=n_l,
                                 dy_base=off * per_roi, out=tape["T"][i] if consume_tape else None))
            off += n_l
        tails = ops.deconv2x2_out1x1_grad_multi(problems)
        if consume_tape:
            tape["T"] = None
        for c, tail in zip(outs, tails):
            c.name_grads(pair_grads(c, tail[1:]), grads)
        # the transposed conv = a 1x1 conv with 4 C_mid outputs on the GEMM layout
        dys = [dT.view(x.shape[0], h, w, dT.shape[1] * dT.shape[2]) for x, (dT, _, _) in zip(xs, tails)]
        args = dict(stride=1, padding="same", dilation=1)
        pairs = ops.conv2d_wgrad_multi([dict(x=x, dy=dy, dc=c.dev1x1, want_bias=True, **args) for c, x, dy in zip(deconvs, xs, dys)])
        for c, (dk1, db4) in zip(deconvs, pairs):
            grads[f"{c.name}/kernel"], grads[f"{c.name}/bias"] = ops.deconv2x2_grad_relayout(dk1, db4)
        if not need_dx and not units[0]:
            return None, grads
        dxs = ops.conv2d_dgrad_multi([dict(dy=dy, dc=c.dev1x1, in_hw=(h, w), **args) for c, dy in zip(deconvs, dys)])
        dxs = self._towers_backward(units, tape, dxs, grads, need_dx=need_dx)
        if dxs is None:
            return None, grads
        return [dx.reshape(tuple(t.shape)) for dx, t in zip(dxs, tape["inputs"])], grads

    def get_config(self):
        config = super().get_config()
        config.update({
            "num_blocks": self.num_blocks, "num_classes": self.num_classes, "num_depth": self.num_depth,
            "num_features": self.num_features, "use_separable_conv": self.use_separable_conv,
            "expand_ratio": self.expand_ratio, "use_squeeze_excite": self.use_squeeze_excite,
            "squeeze_ratio": self.squeeze_ratio, "groups": self.groups})
        return config


class TrimInstances(Layer):
    """Drop the -1 padded RoIs and keep each RoI's own class channel (reference instance.py:258-286):
    rows with class != -1, in tf.where (row-major) order; mask = roi_masks[b, r, :, :, class];
    mold=True re-groups per image with -1 padding (MoldBatch) -> ([B,n,6], [B,n,h,w]), n = the
    largest per-image count; mold=False returns the flat rows ([R,6], [R,h,w])."""

    def __init__(self, mold=True, max_batch_size=64, **kwargs):
        self.mold = mold
        self.max_batch_size = max_batch_size
        super().__init__(**kwargs)
        self.last_counts = None

    def call(self, inputs, **kwargs):
        roi_boxes, roi_masks = inputs[0], inputs[1]
        boxes, masks, counts = ops.trim_instances(roi_boxes, roi_masks)
        self.last_counts = counts
        host_counts = counts.cpu()                       # the dynamic output shape needs the count on the host
        if self.mold:
            n = max(1, int(host_counts.max())) if host_counts.numel() else 1
            return boxes[:, :n].contiguous(), masks[:, :n].contiguous()
        keep = torch.arange(boxes.shape[1], device=boxes.device)[None, :] < counts[:, None]
        return boxes[keep], masks[keep]

    def get_config(self):
        config = super().get_config()
        config.update({"mold": self.mold, "max_batch_size": self.max_batch_size})
        return config


class AssignMasks(Layer):
    """Ground-truth masks -> per-RoI targets (reference :296-386): inputs = [roi_boxes [B,R,6], roi_masks [B,R,h,w,C],
    gt_boxes [B,G,6], gt_masks [B,G,H,W] int8 / uint8] -> int32 [B,R,h,w]: an RoI is matched to the first ground truth of
    its class with the highest IoU if that is >= match_iou_threshold; its target is the matched class where the bilinear
    crop of that ground truth's mask is > 0.5 and num_classes elsewhere; unmatched and padded RoIs are num_classes."""

    def __init__(self, match_iou_threshold=0.5, **kwargs):
        self.match_iou_threshold = match_iou_threshold
        kwargs.update({"trainable": False})
        super().__init__(**kwargs)

    def call(self, inputs, **kwargs):
        roi_boxes, roi_masks, gt_boxes, gt_masks = inputs[0], inputs[1], inputs[2], inputs[3]
        return ops.assign_masks(roi_boxes.contiguous(), gt_boxes.to(torch.float32).contiguous(), gt_masks.contiguous(),
                                (int(roi_masks.shape[2]), int(roi_masks.shape[3])), int(roi_masks.shape[-1]),
                                self.match_iou_threshold)

    def get_config(self):
        config = super().get_config()
        config.update({"match_iou_threshold": self.match_iou_threshold})
        return config
