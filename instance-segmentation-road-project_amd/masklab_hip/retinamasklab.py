"""Model build API -- drop-in for the inference half of reference engine/retinamasklab.py:
build_backbone_network :19-37, build_detection_network :40-112, build_instance_network :115-157,
build_semantic_network :160-198, construct_inference_network :420-495, find_layer_name :646-649,
and the deploy wrapper of load_masklab_inference_model_from_h5 :598-643 (DeployModel below).
Same function names, argument meaning and return structure; the returned model runs eagerly on
the MI355X kernels.  construct_trainer_network :223-395 is restated forward (TrainerModel: target assignment, the four
losses and the metrics of a batch with ground truth) plus the losses' gradients at the head outputs
(TrainerModel.loss_and_gradients); construct_masklabdataset :398-417 builds the file-reading datasets
(masklab_hip/utils/dataset).  GroupNormalization has its backward as a layer method (normalization.py), not yet wired in: the
conv, resize and RoI-align backward of the heads and the backbone's backward stay out of scope; the optimizers
(masklab_hip/optimizers.py) wait for their gradients.
"""
import numpy as np
import torch

from . import backbone
from . import keras_like as K
from . import ops
from .config import ModelConfiguration
from .layers import (ASPPNetwork, AssignBoxes, AssignMasks, AssignSeg, BoxRegressionSubNet, ClassificationSubNet, CropAndPadMask,
                     DetectionProposal,
                     DownSampleInput, DrawBoxes, DrawInstance, DrawSegmentation, EncodeImageContent, SummaryOutput,
                     FeaturePyramid, MaskDistribute, MaskSubNet, PriorLayer, PyramidRoiAlign, ResizeLike,
                     RestoreBoxes, SegmentationSubNet, SemanticSmoothing, TrimInstances, UpSampleOutput)
from .prior import PriorBoxes

VERBOSE = False


def _say(*lines):
    if VERBOSE:
        print("\n".join(lines))


def construct_masklabdataset(configuration: ModelConfiguration, device="cuda"):
    """reference :398-417: (trainset, validset) from `configuration.dataset`; `except_semantic_labels` goes along, since
    the masks are drawn per batch and not read from a `processed/` tree."""
    from .utils import MaskLabDataset
    d_config = configuration.dataset
    trainset, validset = (MaskLabDataset(cases, min_area=d_config.min_area, data_dir=d_config.data_dir,
                                         instance_labels=d_config.instance_labels, semantic_labels=d_config.semantic_labels,
                                         except_semantic_labels=d_config.except_semantic_labels, device=device)
                          for cases in (d_config.train_cases, d_config.valid_cases))
    _say("Dataset Summary", "-------------------------------", f"* Num of Train Images : {len(d_config.train_cases)}",
         f"* Num of Valid Images : {len(d_config.valid_cases)}",
         f"* Num of Images : {len(d_config.train_cases) + len(d_config.valid_cases)}", "-------------------------------\n")
    return trainset, validset


def build_backbone_network(configuration: ModelConfiguration):
    config = configuration.backbone
    model = backbone.load_backbone(config.backbone_type, config.backbone_outputs, config.num_features)
    _say("Backbone Network Summary", "------------------------",
         f"* Backbone Type : {config.backbone_type}", f"* Backbone outputs : {config.backbone_outputs}",
         f"* Num features of Backbone Additional Layers: {config.num_features}", "------------------------\n")
    return model


def build_detection_network(configuration: ModelConfiguration):
    config = configuration.detection
    num_backbone_outputs = len(configuration.backbone.backbone_outputs)
    num_classes = len(configuration.dataset.instance_labels)
    # the output block's name encodes its stride (= number of stride-2 layers), reference :46-48
    prior_strides = [2 ** int(output_name[-1]) for output_name in configuration.backbone.backbone_outputs]
    prior_sizes = [4 * stride for stride in prior_strides]
    prior = PriorBoxes(strides=prior_strides, sizes=prior_sizes, pr_scales=config.pr_scales,
                       pr_ratios=config.pr_ratios)
    prior_subnet = PriorLayer(prior)
    assert len(set(config.feature_pyramid_inputs) - {'C1', 'C2', 'C3', 'C4', 'C5', 'P6', 'P7'}) == 0, \
        "feature pyramid inputs must be drawn from C1~C5, P6, P7"
    feature_pyramid_strides = [2 ** int(name[1]) for name in config.feature_pyramid_inputs]
    fpn_subnet = FeaturePyramid(strides=feature_pyramid_strides, num_features=config.num_features)
    cls_subnet = ClassificationSubNet(num_blocks=num_backbone_outputs, num_classes=num_classes,
                                      num_depth=config.num_depth, num_features=config.num_features,
                                      num_priors=len(prior), use_separable_conv=config.use_separable_conv,
                                      expand_ratio=config.expand_ratio,
                                      use_squeeze_excite=config.use_squeeze_excite,
                                      squeeze_ratio=config.squeeze_ratio, groups=config.groups)
    # NB reference quirk kept (:95): the box tower's squeeze-excite flag is `use_separable_conv`
    loc_subnet = BoxRegressionSubNet(num_blocks=num_backbone_outputs, num_depth=config.num_depth,
                                     num_features=config.num_features, num_priors=len(prior),
                                     use_separable_conv=config.use_separable_conv,
                                     expand_ratio=config.expand_ratio,
                                     use_squeeze_excite=config.use_separable_conv,
                                     squeeze_ratio=config.squeeze_ratio, groups=config.groups)
    return prior_subnet, fpn_subnet, cls_subnet, loc_subnet


def build_instance_network(configuration: ModelConfiguration):
    num_classes = len(configuration.dataset.instance_labels)
    config = configuration.instance
    restore_subnet = RestoreBoxes()
    distribute_subnet = MaskDistribute(max_k=config.max_k, base_size=config.base_size)
    pyramid_roi_align = PyramidRoiAlign(crop_size=config.crop_size)
    # NB reference quirk kept (:139): expand_ratio receives `use_separable_conv`
    mask_subnet = MaskSubNet(num_blocks=config.max_k + 1, num_classes=num_classes, num_depth=config.num_depth,
                             num_features=config.num_features, use_separable_conv=config.use_separable_conv,
                             expand_ratio=config.use_separable_conv, use_squeeze_excite=config.use_squeeze_excite,
                             squeeze_ratio=config.squeeze_ratio, groups=config.groups)
    return restore_subnet, distribute_subnet, pyramid_roi_align, mask_subnet


def build_semantic_network(configuration: ModelConfiguration):
    config = configuration.semantic
    num_classes = len(configuration.dataset.semantic_labels)
    aspp_subnet = ASPPNetwork(num_features=config.num_aspp_features, atrous_rate=config.atrous_rate,
                              groups=config.atrous_groups)
    # NB reference quirk kept (:179): expand_ratio receives `use_separable_conv`
    seg_subnet = SegmentationSubNet(num_depth=config.num_depth, num_features=config.num_features,
                                    num_skip_features=config.num_skip_features, num_classes=num_classes,
                                    use_separable_conv=config.use_separable_conv,
                                    expand_ratio=config.use_separable_conv,
                                    use_squeeze_excite=config.use_squeeze_excite,
                                    squeeze_ratio=config.squeeze_ratio, groups=config.groups)
    return aspp_subnet, seg_subnet


def build_network_shapes(configuration, backbone_network, detection_networks, instance_networks, semantic_networks):
    """Propagate the symbolic shapes through the backbone and the head groups so that every weight spec exists (no GPU
    involved).  The inference and the trainer model share the layer objects; building them again changes nothing."""
    bb = backbone_network
    shapes = bb.output_shapes if bb.built else bb.build((None, None, None, 3))
    by_name = dict(zip(bb.output_names, shapes))
    if detection_networks is not None:
        det_config = configuration.detection
        _, fpn, cls, loc = detection_networks
        fpn_in = [by_name[n] for n in bb.output_names if n in det_config.feature_pyramid_inputs]
        rest = [by_name[n] for n in bb.output_names if n not in det_config.feature_pyramid_inputs]
        feats = fpn.build(fpn_in) + rest
        cls.build(feats)
        loc.build(feats)
        if instance_networks is not None:
            ins = configuration.instance
            mask = instance_networks[3]
            ch, cw = ins.crop_size
            mask.build([(None, None, ch, cw, f[-1]) for f in feats[:ins.max_k + 1]])
    if semantic_networks is not None:
        seg_config = configuration.semantic
        aspp, seg = semantic_networks
        a = aspp.build(by_name[seg_config.aspp_input_name])
        seg.build([a, by_name[seg_config.skip_input_name]])


class InferenceModel(K.Layer):
    """The Keras functional `Model(images -> [cls_pred, loc_pred, roi_boxes, roi_masks, seg_pred])`
    of reference :420-495, executed eagerly.  Output list shrinks like the reference when a head
    group is None."""

    def __init__(self, configuration, backbone_network, detection_networks=None, semantic_networks=None,
                 instance_networks=None, name='inference'):
        super().__init__(name=name)
        self.configuration = configuration
        self.backbone_network = backbone_network
        self.detection_networks = detection_networks
        self.semantic_networks = semantic_networks
        self.instance_networks = instance_networks if detection_networks is not None else None
        self.detection_proposal = None
        self.output_names = []
        if detection_networks is not None:
            self.output_names += ['cls_pred', 'loc_pred']
            if self.instance_networks is not None:
                det_config = configuration.detection
                # re-instantiated from config.detection.* every time (reference :459-466)
                self.detection_proposal = DetectionProposal(
                    min_confidence=det_config.min_confidence, nms_iou_threshold=det_config.nms_iou_threshold,
                    post_iou_threshold=det_config.post_iou_threshold,
                    nms_max_output_size=det_config.nms_max_output_size,
                    max_batch_size=configuration.train.inference_batch_size)
                self.output_names += ['roi_boxes', 'roi_masks']
        if semantic_networks is not None:
            self.output_names.append('seg_pred')
        self.layers = self._flat_layers()
        self.device = None
        self.last_detections = None
        self._use_graphs = False
        self._graphs = {}
        # Auxiliary HIP streams (semantic head, box tower, P6/P7, coarse FPN convs beside the main chain): True / False /
        # "auto" = on unless the forward is so small that it is bound by the host's launch rate, where the extra
        # stream hand-overs cost more than the overlap gives (1 x 512 x 512: 2.78 ms with, 2.45 ms without); under
        # hipGraph capture they are always worth it (the branches replay without host work: 1.94 ms).
        self.use_side_stream = "auto"
        self._side_stream = None
        # Stage 2 without a host read ("dynamic shapes without host sync"): RoI crops + mask head launched at
        # capacity, the kernels reading the per-level RoI maxima from device memory; the molded shapes are produced when
        # the outputs are handed over (ONE read, after the whole forward is enqueued).  True / False / "auto" = with
        # hipGraph replay (the whole forward is then ONE graph), where nothing but that read remains for the host.
        self.device_counts = "auto"
        self._capacity_held = 0          # bytes of capacity tensors already captured in this model's graphs (they count as free)
        self._build_shapes()

    # ---- structure
    def _flat_layers(self):
        layers = [self.backbone_network]
        for grp in (self.detection_networks, self.instance_networks, self.semantic_networks):
            if grp is not None:
                layers += list(grp)
        if self.detection_proposal is not None:
            layers.append(self.detection_proposal)
        return layers

    def get_layer(self, name):
        for l in self.layers:
            if l.name == name:
                return l
        raise ValueError(f"No such layer: {name}")

    def children(self):
        return self.layers

    def weight_specs(self):
        out = {}
        for l in self.layers:
            out.update(l.weight_specs())
        return out

    def _build_shapes(self):
        build_network_shapes(self.configuration, self.backbone_network, self.detection_networks, self.instance_networks,
                             self.semantic_networks)
        self.built = True

    # ---- weights
    def init_weights(self, seed=0):
        """Random weights from each layer's initializer (what a fresh Keras model has), keyed and
        seeded by weight name so the result is independent of construction order."""
        return K.init_weights(self.weight_specs(), seed)

    def _drop_graphs(self):
        """Forget the captured graphs (their private memory pools go with them) and let ops release the scratch buffers
        that only those captures kept alive."""
        from . import ops
        self._graphs = {}
        self._capacity_held = 0
        ops.graph_owner_released(self)

    def load_weights(self, weights, device="cuda"):
        self.device = torch.device(device)
        self._drop_graphs()                  # captured graphs hold the addresses of the tensors being replaced
        for l in self.layers:
            l.load_weights(weights, self.device)
        return self

    def reload_class_outputs(self, weights):
        """Re-pack and upload only the class towers' output convs (parity fixtures rescale those kernels to
        move the score distribution; everything else keeps its device copy)."""
        if self.detection_networks is None:
            raise RuntimeError("no detection networks")
        self._drop_graphs()
        for block in self.detection_networks[2].blocks:
            block[-1].load_weights(weights, self.device)

    # ---- forward (reference :431-491)
    # Stage 1 = everything up to the one host read (backbone, FPN, towers, box decode, DetectionProposal,
    # level assignment, semantic head); stage 2 = RoI crops + mask head, whose molded shapes depend on the
    # RoI counts the host reads in between (the reference's dynamic shapes).
    def _stage1(self, images, want_kept=False):
        cfg = self.configuration
        bb = self.backbone_network
        aux = self._aux_streams_wanted(images)
        fork_ok = aux and self.detection_networks is not None and hasattr(bb, "join_extra_levels")
        feats = bb(images, fork_stream=self._fork_stream) if fork_ok else bb(images)
        by_name = dict(zip(bb.output_names, feats))
        st = {"image_hw": (int(images.shape[1]), int(images.shape[2]))}

        def semantic_head():
            seg_config = cfg.semantic
            aspp_subnet, seg_subnet = self.semantic_networks
            aspp_outputs = aspp_subnet(by_name[seg_config.aspp_input_name])
            return seg_subnet([aspp_outputs, by_name[seg_config.skip_input_name]])

        # The semantic head only needs backbone taps.  With `use_side_stream` it goes to a second HIP stream, enqueued
        # once the towers are queued: it then runs beside the detection post-processing (40 + 8 blocks), through
        # the host's read of the RoI counts and its preparation of stage 2 (~0.2 ms during which the main stream is
        # empty), and beside the first mask-head launches.  Joined at the end of stage 2 (of stage 1 under capture).
        side = None

        def launch_semantic_on_side():
            from . import ops as _ops
            if self.semantic_networks is None or not aux or _ops.PROFILE is not None:
                return None
            main = torch.cuda.current_stream()
            if self._side_stream is None:
                self._side_stream = torch.cuda.Stream(device=self.device)
            self._side_stream.wait_stream(main)
            with torch.cuda.stream(self._side_stream):
                st["seg_pred"] = semantic_head()
            return self._side_stream

        if self.detection_networks is None:
            side = launch_semantic_on_side()
        if self.detection_networks is not None:
            det_config = cfg.detection
            prior_subnet, fpn_subnet, cls_subnet, loc_subnet = self.detection_networks
            pr_boxes = prior_subnet(images)
            fpn_inputs = [by_name[n] for n in bb.output_names if n in det_config.feature_pyramid_inputs]
            without_fpn = [by_name[n] for n in bb.output_names if n not in det_config.feature_pyramid_inputs]
            feature_outputs = (fpn_subnet(fpn_inputs, fork_stream=self._fork_stream) if fork_ok
                               else fpn_subnet(fpn_inputs)) + without_fpn
            if fork_ok:
                bb.join_extra_levels(feats)                    # P6 / P7 ran beside the FPN chain
            # The class and the box tower are independent chains of the same shape (5 levels x 4 convs, 1365 tiles per
            # launch = 2.67 rounds of the chip's 512 resident blocks): on two streams the last, partly filled round of
            # one launch is topped up by the other tower's blocks.  Same kernels, same inputs: bit-identical outputs.
            tower_stream = self._fork_stream("_tower_stream") if aux else None
            if tower_stream is not None:
                with torch.cuda.stream(tower_stream):
                    st["loc_pred"] = loc_subnet(feature_outputs)
                st["cls_pred"] = cls_subnet(feature_outputs)
                torch.cuda.current_stream().wait_stream(tower_stream)
                st["loc_pred"].record_stream(torch.cuda.current_stream())
            else:
                st["cls_pred"] = cls_subnet(feature_outputs)
                st["loc_pred"] = loc_subnet(feature_outputs)
            side = launch_semantic_on_side()
            if self.instance_networks is not None:
                restore_subnet, distribute_subnet, pyramid_roi_align, _ = self.instance_networks
                restored_boxes = restore_subnet([st["loc_pred"], pr_boxes])
                # fused DetectionProposal -> MaskDistribute -> PyramidRoiAlign in fixed capacity:
                # the only host read is the per-level RoI count that sizes the molded outputs.
                proposed, counts, kept, payload = self.detection_proposal.propose_fixed(
                    st["cls_pred"], restored_boxes, want_kept=want_kept, want_payload=True)
                n_levels = cfg.instance.max_k + 1
                if distribute_subnet.max_k + 1 != n_levels:
                    raise ValueError("MaskDistribute.max_k does not match config.instance.max_k")
                slots, lcounts, lmax = pyramid_roi_align.distribute(n_levels, proposed, has_k=False,
                                                                    base_size=distribute_subnet.base_size)
                st.update(proposed=proposed, counts=counts, kept=kept, payload=payload, boxes=restored_boxes,
                          slots=slots, lcounts=lcounts, lmax=lmax, roi_features=feature_outputs[:n_levels])
        if side is not None:
            st["side"] = side
            st["keepalive"] = by_name            # backbone taps the side stream still reads
            if torch.cuda.is_current_stream_capturing() and not getattr(self, "_capturing_whole", False):
                self._join_side(st)              # a captured stage 1 must be self-contained
        elif self.semantic_networks is not None:
            # independent of the instance branch and enqueued BEFORE the host reads the RoI counts, so the
            # GPU stays busy while the host waits (same stream, same results)
            st["seg_pred"] = semantic_head()
        return st

    def _aux_streams_wanted(self, images):
        mode = getattr(self, "use_side_stream", False)
        if mode != "auto":
            return bool(mode)
        if torch.cuda.is_current_stream_capturing():
            return True
        return int(images.shape[0]) * int(images.shape[1]) * int(images.shape[2]) > 512 * 512

    def _fork_stream(self, attr):
        """A lazily created auxiliary stream that starts behind everything enqueued on the current one (None under the
        per-launch profiling hook, whose event pairs assume one stream)."""
        from . import ops as _ops
        if _ops.PROFILE is not None:
            return None
        s = getattr(self, attr, None)
        if s is None:
            s = torch.cuda.Stream(device=self.device)
            setattr(self, attr, s)
        s.wait_stream(torch.cuda.current_stream())
        return s

    def _join_side(self, st):
        side = st.pop("side", None)
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
            st["seg_pred"].record_stream(torch.cuda.current_stream())
            st.pop("keepalive", None)

    def _stage2(self, st):
        outputs = []
        if self.detection_networks is not None:
            outputs += [st["cls_pred"], st["loc_pred"]]
            if self.instance_networks is not None:
                _, _, pyramid_roi_align, mask_subnet = self.instance_networks
                roi_fmaps, roi_boxes = pyramid_roi_align.crop_distributed(
                    st["roi_features"], st["proposed"], st["image_hw"], st["slots"], st["lcounts"], st["lmax"])
                roi_masks = mask_subnet(roi_fmaps)
                outputs += [roi_boxes, roi_masks]
                self.last_detections = dict(proposed=st["proposed"], counts=st["counts"], kept=st["kept"],
                                            boxes=st["boxes"], payload=st["payload"],
                                            level_counts=st["lcounts"], level_max=st["lmax"])
        self._join_side(st)
        if self.semantic_networks is not None:
            outputs.append(st["seg_pred"])
        return outputs

    # ---- stage 2 at capacity: no host read inside the forward
    # The capacity form trades memory for the missing host read: every RoI level is sized for B x nms_max_output_size slots.
    # It is used while its tensors stay below CAPACITY_BYTES_LIMIT and a quarter of the device's free memory (each input
    # shape captured under hipGraph keeps its own set: graph-private pools are not shared), and never past
    # MAX_CAPACITY_ROIS slots per level.
    MAX_CAPACITY_ROIS = 8192
    CAPACITY_BYTES_LIMIT = 16 << 30

    def capacity_bytes(self, batch):
        """Estimate of what ONE fixed-capacity stage 2 holds: per RoI level the crops and every tower / deconv
        intermediate ([B*cap, ch, cw, C] each: under graph capture none of them is recycled), plus masks_cap
        [B, L*cap, 2ch, 2cw, classes] fp32 twice (at capacity, and the buffer its molded form is the front of) and the
        split-K workspace (per stream).  A SqueezeExcite tower adds the out-of-place SqueezeExcite output at the tower input
        and its pooled-sum workspace; a separable tower the expanded (expand_ratio x C) maps of every depth."""
        from . import ops
        ins = self.configuration.instance
        pra, mask = self.instance_networks[2], self.instance_networks[3]
        cap = int(self.detection_proposal.nms_max_output_size)
        L = ins.max_k + 1
        ch, cw = pra.crop_size
        es = 2 if ops.half_storage() else 4
        slots = int(batch) * cap
        maps = 2 + mask.num_depth                         # crops, tower outputs, deconv output (per level)
        extra = 0
        if mask.use_squeeze_excite:
            maps += 1
            extra = L * ((int(ops._lib.load().ml_squeeze_excite_workspace_bytes(slots, ch * cw, mask.num_features)) + 255)
                         // 256 * 256)
        if mask.use_separable_conv:                       # expand conv output + depthwise output of every depth
            maps += mask.num_depth * 2 * int(mask.expand_ratio * mask.num_features) / mask.num_features
        per_level = int(slots * ch * cw * mask.num_features * es * maps)
        masks = slots * L * 4 * ch * cw * mask.num_classes * 4
        return L * per_level + 2 * masks + extra + 2 * int(ops._lib.load().ml_conv2d_workspace_bytes())   # (masks: at capacity + molded)

    def _capacity_wanted(self, images):
        mode = getattr(self, "device_counts", "auto")
        on = self._use_graphs if mode == "auto" else bool(mode)
        if not on or self.instance_networks is None:
            return False
        pra, mask = self.instance_networks[2], self.instance_networks[3]
        cap = int(self.detection_proposal.nms_max_output_size)
        if not (mask.capacity_supported(tuple(pra.crop_size)) and int(images.shape[0]) * cap <= self.MAX_CAPACITY_ROIS
                and cap * pra.crop_size[0] * pra.crop_size[1] >= 128):
            return False
        need = self.capacity_bytes(int(images.shape[0]))
        limit = self.CAPACITY_BYTES_LIMIT
        if self.device is not None and self.device.type == "cuda":
            limit = min(limit, torch.cuda.mem_get_info(self.device)[0] // 4 + self._capacity_held)
        return need <= limit

    def _stage2_capacity(self, st):
        """RoI crops + mask head with every level at capacity (reference engine/layers/instance.py:115-134,211-233 +
        MoldBatch misc.py:231-286): kernels skip the RoI slots past the level maxima they read on the device.
        -> the forward's RAW result: fixed-shape tensors + `lmax` (what `_mold` needs the host to read)."""
        from . import ops
        _, _, pyramid_roi_align, mask_subnet = self.instance_networks
        roi_fmaps, boxes_cap, lives = pyramid_roi_align.crop_capacity(
            st["roi_features"], st["proposed"], st["image_hw"], st["slots"], st["lcounts"], st["lmax"])
        masks_cap = mask_subnet(roi_fmaps, lives=lives)
        self.last_detections = dict(proposed=st["proposed"], counts=st["counts"], kept=st["kept"], boxes=st["boxes"],
                                    payload=st["payload"], level_counts=st["lcounts"], level_max=st["lmax"])
        self._join_side(st)
        # MoldBatch + Concatenate(axis=1) at the front of two capacity buffers, sized on the device from `lmax`: part of the
        # captured forward, so that nothing is launched after it (round 4: the two molding launches behind the host's read
        # left the GPU idle for their launch latencies -- 0.25 ms of gaps per forward under a kernel trace at 1 x 512^2)
        cap = int(st["proposed"].shape[1])
        return dict(cls_pred=st["cls_pred"], loc_pred=st["loc_pred"], boxes_cap=boxes_cap, masks_cap=masks_cap,
                    boxes_molded=ops.mold_levels_dev(boxes_cap, st["lmax"], cap),
                    masks_molded=ops.mold_levels_dev(masks_cap, st["lmax"], cap),
                    lmax=st["lmax"], cap=cap, seg_pred=st.get("seg_pred"))

    def _mold(self, raw):
        """The ONE host read of the forward (the per-level RoI maxima, L ints) and the molded outputs it sizes."""
        from . import ops
        n_l = [min(max(1, int(v)), raw["cap"]) for v in raw["lmax"].tolist()]
        outputs = [raw["cls_pred"], raw["loc_pred"], ops.molded_front(raw["boxes_molded"], n_l),
                   ops.molded_front(raw["masks_molded"], n_l)]
        if self.semantic_networks is not None:
            outputs.append(raw["seg_pred"])
        return outputs

    # ---- hipGraph replay (launch-bound small batches: serving one image at a time)
    def enable_graphs(self, enabled=True):
        """Capture the forward (~300 kernel launches) into a hipGraph per input shape and replay it: one launch instead
        of hundreds, which is what a batch-1 forward is bound by.  With the fixed-capacity stage 2 (`device_counts`) the
        WHOLE forward is one graph; otherwise stage 1 is (stage 2's shapes then depend on a host read).  The tensors
        the graph returns are graph-owned buffers, valid until the next call (`outputs_graph_owned`).
        Memory: every captured input shape (x conv math x thresholds) keeps its own activations, capacity tensors
        (`capacity_bytes`) and split-K workspace for as long as the graph lives; `enable_graphs(False)`, `load_weights`
        and `reload_class_outputs` drop them all.  A server that sees many input shapes should bucket them."""
        self._use_graphs = bool(enabled)
        if not enabled:
            self._drop_graphs()
        return self

    @property
    def outputs_graph_owned(self):
        return bool(self._use_graphs)

    def _stage1_graphed(self, images, whole=False):
        from . import ops
        # kernel arguments are baked into a capture: everything they are computed from is part of the key
        dp = self.detection_proposal
        key = (tuple(images.shape), images.dtype, ops.CONV_MATH, bool(whole)) + (
            () if dp is None else (float(dp.min_confidence), float(dp.nms_iou_threshold), float(dp.post_iou_threshold),
                                   int(dp.nms_max_output_size)))
        entry = self._graphs.get(key)
        if entry is None:
            if ops.PROFILE is not None:
                raise RuntimeError("graph capture cannot run under the per-launch profiling hook")
            # warm-up: fills the anchor / workspace caches, sets kernel attributes
            if whole:
                self._stage2_capacity(self._stage1(images))
            else:
                self._join_side(self._stage1(images))
            torch.cuda.synchronize(self.device)
            static_in = images.clone()
            graph = torch.cuda.CUDAGraph()
            self._capturing_whole = bool(whole)          # (the side stream then joins at the end of stage 2)
            try:
                with torch.cuda.graph(graph):
                    st = self._stage1(static_in)
                    if whole:
                        st = self._stage2_capacity(st)
            finally:
                self._capturing_whole = False
            entry = self._graphs[key] = (graph, static_in, st)
            ops.graph_owner_registered(self)
            if whole:
                self._capacity_held += self.capacity_bytes(int(images.shape[0]))
        graph, static_in, st = entry
        static_in.copy_(images)
        graph.replay()
        return st

    def call(self, images, **kwargs):
        if not isinstance(images, torch.Tensor):
            images = torch.as_tensor(np.asarray(images))
        if self.device is None:
            raise RuntimeError("InferenceModel: call load_weights(weights, device) first")
        images = images.to(self.device).contiguous()
        want_kept = kwargs.get("want_kept", False)
        from . import ops
        graphs = getattr(self, "_use_graphs", False) and not want_kept and ops.PROFILE is None
        if not want_kept and self._capacity_wanted(images):
            # no host read inside the forward; with graphs the whole of it is one replay
            raw = self._stage1_graphed(images, whole=True) if graphs else self._stage2_capacity(self._stage1(images))
            if kwargs.get("defer", False):
                return DeferredOutputs(self, raw)
            return self._mold(raw)
        if graphs:
            st = self._stage1_graphed(images)
        else:
            st = self._stage1(images, want_kept=want_kept)
        return self._stage2(st)

    def predict(self, images, **kwargs):
        """Keras `Model.predict`: numpy in, list of numpy out."""
        outs = self.call(images, **kwargs)
        if isinstance(outs, DeferredOutputs):
            outs = outs.materialize()
        torch.cuda.synchronize(self.device)
        return [o.cpu().numpy() for o in outs]


class DeferredOutputs:
    """What `InferenceModel(images, defer=True)` returns on the fixed-capacity path: the forward is fully enqueued and
    NOTHING has been read by the host yet, so a caller that pipelines forwards (bench.py) never stalls; `materialize()`
    does the one read (per-level RoI maxima) and returns the molded output list, shaped exactly like the reference's
    (roi_boxes / roi_masks with N = sum of the level maxima, engine/layers/misc.py:231-286)."""

    def __init__(self, model, raw):
        self.model, self.raw = model, raw

    def materialize(self):
        return self.model._mold(self.raw)


def construct_inference_network(configuration: ModelConfiguration, backbone_network, detection_networks=None,
                                semantic_networks=None, instance_networks=None):
    """Same signature as reference :420-424."""
    return InferenceModel(configuration, backbone_network, detection_networks=detection_networks,
                          semantic_networks=semantic_networks, instance_networks=instance_networks)


class TrainerModel(K.Layer):
    """The Keras functional `Model([images, gt_boxes, gt_boxes_exist, gt_masks, gt_seg, gt_seg_exist] -> losses and metrics)`
    of reference :223-395, executed eagerly (no hipGraph, no fixed-capacity stage 2): what
    `fit_generator(validation_data=...)` evaluates to report a checkpoint's validation losses.  `loss_and_gradients` adds the
    gradients of the compiled scalar at the four head outputs; `train_on_batch` carries them through the head groups' `backward`s into an optimizer's step and one re-pack (the FPN and the backbone are frozen; trainable="head_tune" also trains the FPN and the two extra levels behind C5).  The backbone and head layers
    are the OBJECTS the inference model holds, as in the reference; the assignment, loss and metric layers are the model's
    own.  Every output is float32 [B]; the lists shrink like the reference's when a head group is None.
    `last_forward` keeps the intermediate tensors of the last call."""

    METRIC_NAMES = ['other_road_iou_metric', 'my_road_metric', 'crack_iou_metric']

    def __init__(self, configuration, backbone_network, detection_networks=None, semantic_networks=None,
                 instance_networks=None, name='trainer'):
        super().__init__(name=name)
        from .losses import BoxLoss, ClassLoss, MaskLoss, SegLoss
        from .metrics import ClassBinaryIOU, DetectionIOUMetric
        config = configuration.loss
        self.configuration = configuration
        self.backbone_network = backbone_network
        self.detection_networks = detection_networks
        self.semantic_networks = semantic_networks
        self.instance_networks = instance_networks if detection_networks is not None else None
        self.input_names = ['images']
        self.output_names = []
        own = []
        if detection_networks is not None:
            det_config = configuration.detection
            num_classes = len(configuration.dataset.instance_labels)
            self.input_names += ['gt_boxes', 'gt_boxes_exist']
            self.assign_boxes = AssignBoxes(num_classes=num_classes)
            self.class_loss = ClassLoss(weight=config.cls_loss_weight, alpha=config.cls_loss_alpha,
                                        gamma=config.cls_loss_gamma, name='class_loss')
            self.box_loss = BoxLoss(weight=config.box_loss_weight, momentum=config.box_loss_momentum,
                                    beta=config.box_loss_beta, use_adjust=config.box_loss_use_adjust, name='box_loss')
            self.metric_restore = RestoreBoxes()
            self.metric_proposal = DetectionProposal(                                  # config.detection.* (:295-300)
                min_confidence=det_config.min_confidence, nms_iou_threshold=det_config.nms_iou_threshold,
                post_iou_threshold=det_config.post_iou_threshold, nms_max_output_size=det_config.nms_max_output_size,
                max_batch_size=configuration.train.max_batch_size)
            self.detection_metric = DetectionIOUMetric()
            self.output_names += ['class_loss', 'box_loss', 'detection_precision_metric', 'detection_recall_metric',
                                  'detection_fmeasure_metric']
            own += [self.assign_boxes, self.class_loss, self.box_loss, self.metric_restore, self.metric_proposal,
                    self.detection_metric]
            if self.instance_networks is not None:
                self.input_names.append('gt_masks')
                self.loss_proposal = DetectionProposal(                                # config.loss.* (:314-319)
                    min_confidence=config.min_confidence, nms_iou_threshold=config.nms_iou_threshold,
                    post_iou_threshold=config.post_iou_threshold, nms_max_output_size=config.nms_max_output_size,
                    max_batch_size=configuration.train.max_batch_size)
                self.assign_masks = AssignMasks()
                self.mask_loss = MaskLoss(weight=config.mask_loss_weight,
                                          label_smoothing=config.mask_loss_label_smoothing, name='mask_loss')
                self.output_names.append('mask_loss')
                own += [self.loss_proposal, self.assign_masks, self.mask_loss]
        if semantic_networks is not None:
            if len(configuration.dataset.semantic_labels) != len(self.METRIC_NAMES):
                raise ValueError("the trainer network unpacks ClassBinaryIOU into three metrics (reference :385-391): it needs "
                                 "three semantic labels")
            self.input_names += ['gt_seg', 'gt_seg_exist']
            self.assign_seg = AssignSeg()
            self.seg_loss = SegLoss(weight=config.seg_loss_weight, label_smoothing=config.seg_loss_label_smoothing,
                                    name='seg_loss')
            self.class_iou = ClassBinaryIOU(0.5, name='class_iou_metric')
            self.output_names += ['seg_loss'] + self.METRIC_NAMES
            own += [self.assign_seg, self.seg_loss, self.class_iou]
        self.layers = [backbone_network]
        for grp in (self.detection_networks, self.instance_networks, self.semantic_networks):
            if grp is not None:
                self.layers += list(grp)
        self.layers += own
        self.device = None
        self.last_forward = None
        build_network_shapes(configuration, backbone_network, self.detection_networks, self.instance_networks,
                             self.semantic_networks)
        self.built = True

    # ---- structure and weights (the surface of InferenceModel)
    def get_layer(self, name):
        for l in self.layers:
            if l.name == name:
                return l
        raise ValueError(f"No such layer: {name}")

    def children(self):
        return self.layers

    def weight_specs(self):
        out = {}
        for l in self.layers:
            out.update(l.weight_specs())
        return out

    def init_weights(self, seed=0):
        return K.init_weights(self.weight_specs(), seed)

    def load_weights(self, weights, device="cuda"):
        """Load every layer, the shared ones included.  An inference model built beside this one has its own
        `load_weights` (it also drops its captured graphs); `box_loss/moving_mean` and `box_loss/moving_var` are optional."""
        self.device = torch.device(device)
        for l in self.layers:
            l.load_weights(weights, self.device)
        return self

    # ---- the head groups' weights as device tensors ("Re-pack")
    def head_groups(self):
        """The head groups whose backward exists, those present: class, box, mask, ASPP, segmentation sub-networks."""
        out = []
        if self.detection_networks is not None:
            out += list(self.detection_networks[2:4])
            if self.instance_networks is not None:
                out.append(self.instance_networks[3])
        if self.semantic_networks is not None:
            out += list(self.semantic_networks)
        return out

    STAGES = ("heads", "head_tune")

    def _stage_layers(self, what, stage):
        """The layers a stage trains.  "heads": the head groups present.  "head_tune" (the reference's train_head_tune,
        freeze_depth="C5"): those, the FeaturePyramid and the backbone's extra levels (P6_conv, P6_norm, P7_conv)."""
        if stage not in self.STAGES:
            raise ValueError(f"TrainerModel.{what}: stage must be one of {self.STAGES}, got {stage!r}")
        layers = self.head_groups()
        if stage == "head_tune":
            if self.detection_networks is None:
                raise ValueError(f"TrainerModel.{what}: the 'head_tune' stage trains the FeaturePyramid: it needs the detection "
                                 f"networks")
            layers = layers + [self.detection_networks[1]] + self.backbone_network.extra_level_layers()
        return layers

    def device_params(self, stage="heads"):
        """{full weight name: float32 device tensor} of every layer the stage trains (Layer.device_params): what an
        optimizer's apply_gradients steps.  "heads": the head groups present; the FPN and the backbone are not in it, and
        nothing of them is bound or uploaded.  "head_tune": also the FPN's and the extra levels' (P6_conv, P6_norm, P7_conv)
        parameters.  The backbone's body is in neither: its BatchNormalization is folded into its weights."""
        if self.device is None:
            raise RuntimeError("TrainerModel: call load_weights(weights, device) first")
        out = {}
        for g in self._stage_layers("device_params", stage):
            out.update(g.device_params())
        return out

    def _repack_job_source(self):
        """repack() after the head parameters stepped: every packing under the head groups, not the frozen layers'."""
        return [j for g in self.head_groups() for j in g.repack_jobs()]

    def repack(self, stage="heads"):
        """Layer.repack over the stage's layers: one launch.  "head_tune" keeps a job list and a table of its own, so a
        "heads" step's stay what they were."""
        layers = self._stage_layers("repack", stage)
        if stage == "heads":
            return super().repack()
        if getattr(self, "_tune_repack", None) is None:
            self._tune_repack = [ops.RepackTable(), (None, None)]
        if self._tune_repack[1][0] != ops.forms_epoch():
            self._tune_repack[1] = (ops.forms_epoch(), [j for g in layers for j in g.repack_jobs()])
        ops.repack_weights(self._tune_repack[1][1], self._tune_repack[0])

    # ---- forward (reference :233-391)
    def _named_inputs(self, inputs):
        if isinstance(inputs, dict):
            missing = [n for n in self.input_names if n not in inputs]
            if missing:
                raise ValueError(f"TrainerModel: inputs {missing} are missing")
            return {n: inputs[n] for n in self.input_names}
        inputs = list(inputs)
        if len(inputs) != len(self.input_names):
            raise ValueError(f"TrainerModel: {len(self.input_names)} inputs expected ({self.input_names}), got {len(inputs)}")
        return dict(zip(self.input_names, inputs))

    def _dev(self, t, dtype=None):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.ascontiguousarray(t))
        t = t.to(self.device)
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t.contiguous()

    GRAD_OF = {"class_loss": "cls_pred", "box_loss": "loc_pred", "mask_loss": "roi_masks", "seg_loss": "seg_pred"}

    def call(self, inputs, **kwargs):
        return self._forward(inputs, None)

    def _check_upstream(self, what, upstream):
        unknown = sorted(set(upstream or {}) - set(self.GRAD_OF))
        if unknown:
            raise ValueError(f"TrainerModel.{what}: upstream names {unknown} are not losses ({sorted(self.GRAD_OF)})")

    def loss_and_gradients(self, inputs, upstream=None, wrt="predictions"):
        """The forward of `call`, metrics included, with every loss layer run as `call_with_grad` -> (outputs, grads):
        the outputs of `call` bit for bit, and grads = {"cls_pred", "loc_pred", "roi_masks", "seg_pred"} (those whose head
        group is present), each shaped like that tensor of `last_forward`: the gradient of sum over the losses of
        sum_b upstream[loss][b] * loss[b].  upstream None is 1 / B everywhere -- the scalar engine/train.py compiles,
        add_loss(K.mean(loss)) per loss; a dict {loss name: float32 [B]} overrides single losses.  wrt="pre_activation"
        gives the class, mask and seg gradients at the pre-activation of their output convs' fused sigmoid (loc_pred is
        linear).  train_on_batch carries them on: through the heads' `backward`s into an optimizer's step and `repack()`.  Also kept in last_forward["grads"]."""
        if wrt not in ("predictions", "pre_activation"):
            raise ValueError(f"TrainerModel.loss_and_gradients: wrt must be 'predictions' or 'pre_activation', got {wrt!r}")
        self._check_upstream("loss_and_gradients", upstream)
        grads = {}
        outputs = self._forward(inputs, dict(upstream=dict(upstream or {}), through_sigmoid=wrt == "pre_activation", grads=grads))
        self.last_forward["grads"] = grads
        return outputs, grads

    def _loss(self, layer, inputs, want):
        """One loss layer: its forward, or with `want` its fused loss + gradient, the gradient filed under the prediction's name."""
        if want is None:
            return layer(inputs)
        up = want["upstream"].get(layer.name)
        if up is not None:
            up = self._dev(up, torch.float32)
        sig = want["through_sigmoid"] and layer.name != "box_loss"
        loss, want["grads"][self.GRAD_OF[layer.name]] = layer.call_with_grad(inputs, upstream=up, through_sigmoid=sig)
        return loss

    @staticmethod
    def _head(layer, inputs, want):
        """A head group's forward: `call`, or with want["tapes"] its `call_with_tape` (the same bits), the tape kept by name."""
        if want is None or want.get("tapes") is None:
            return layer(inputs)
        out, want["tapes"][layer.name] = layer.call_with_tape(inputs)
        return out

    # ---- one training step ("The step")
    def _trainable_names(self, trainable, params):
        """The names of `params` a step updates.  "heads": all of them; a set of names or a predicate narrows it.  A name under
        the FPN or the backbone raises NotImplementedError, any other unknown name ValueError."""
        if isinstance(trainable, str):
            if trainable not in self.STAGES:
                raise ValueError(f"TrainerModel.train_on_batch: trainable must be 'heads', 'head_tune', a set of weight names or "
                                 f"a predicate, got {trainable!r}")
            return set(params)
        frozen_specs = dict(self.backbone_network.weight_specs())
        if self.detection_networks is not None:
            frozen_specs.update(self.detection_networks[1].weight_specs())
        if callable(trainable):
            frozen = [n for n in frozen_specs if trainable(n)]
            names = {n for n in params if trainable(n)}
        else:
            names = set(trainable)
            unknown = sorted(names - set(params) - set(frozen_specs))
            if unknown:
                raise ValueError(f"TrainerModel.train_on_batch: {unknown[:5]} are not trainable weights of this model")
            frozen = sorted(names & set(frozen_specs))
        if frozen:
            raise NotImplementedError(f"TrainerModel.train_on_batch: {list(frozen)[:5]} lie under the FPN or the backbone, which a "
                                      f"set of names or a predicate cannot select: trainable=\"head_tune\" trains the FPN and the "
                                      f"P6 / P7 levels (the whole stage), and the backbone's body cannot be trained yet -- its "
                                      f"BatchNormalization is folded into its weights")
        return names

    def train_on_batch(self, inputs, optimizer, trainable="heads", upstream=None):
        """One eager training step with Keras's semantics -> the outputs of `call` for this batch as they were BEFORE the
        update, bit for bit (the head groups run as call_with_tape, documented bit-equal to call).
        The gradients are those of loss_and_gradients(wrt="pre_activation", upstream=upstream), routed through
        cls_subnet.backward, loc_subnet.backward, mask_subnet.backward(need_dx=False) and seg_subnet.backward ->
        aspp.backward(need_dx=False); the gradients at the head inputs are dropped: the FPN and the backbone are frozen.
        The merged {name: gradient} dict (kept as last_forward["weight_grads"]) goes to
        optimizer.apply_gradients(device_params(), grads, trainable=names), then ONE repack_weights brings every packing of
        the head groups up to its master.  trainable: "heads" (every weight of the head groups present), a set of names or a
        predicate; a name under the FPN or the backbone raises NotImplementedError, a name the model does not have
        ValueError.  trainable="head_tune" is the reference's first training stage (train_head_tune: everything behind the C5
        tap): the backbone and the FPN run as call_with_tape (the same bits), MaskSubNet.backward(need_dx=True), and per
        pyramid level the class tower's, the box tower's and PyramidRoiAlign.backward's gradients are summed in that order
        (_head_tune_backward), then BackboneModel.backward_extra_levels and FeaturePyramid.backward; the merged dict goes to
        ONE apply_gradients over device_params("head_tune") and one re-pack launch.  The semantic head's input gradients are
        still dropped (its inputs are backbone taps), and the backbone's body stays frozen.  Head groups with SqueezeExcite or separable towers, half tensors and set_conv_math("f16") raise
        NotImplementedError before anything runs; a refused step changes no weight."""
        tune = isinstance(trainable, str) and trainable == "head_tune"
        params = self.device_params("head_tune" if tune else "heads")     # raises by name for what cannot be trained
        names = self._trainable_names(trainable, params)
        self._check_upstream("train_on_batch", upstream)
        grads, tapes = {}, {}
        outputs = self._forward(inputs, dict(upstream=dict(upstream or {}), through_sigmoid=True, grads=grads, tapes=tapes,
                                             head_tune=tune))
        wg = {}
        if self.detection_networks is not None and tune:
            self._head_tune_backward(tapes, grads, wg)
        elif self.detection_networks is not None:
            _, _, cls_subnet, loc_subnet = self.detection_networks
            wg.update(cls_subnet.backward(tapes[cls_subnet.name], grads["cls_pred"])[1])
            wg.update(loc_subnet.backward(tapes[loc_subnet.name], grads["loc_pred"])[1])
            if self.instance_networks is not None:
                mask_subnet = self.instance_networks[3]
                wg.update(mask_subnet.backward(tapes[mask_subnet.name], grads["roi_masks"], need_dx=False)[1])
        if self.semantic_networks is not None:
            aspp_subnet, seg_subnet = self.semantic_networks
            (d_aspp, _), g = seg_subnet.backward(tapes[seg_subnet.name], grads["seg_pred"], need_dx=(True, False))
            wg.update(g)
            wg.update(aspp_subnet.backward(tapes[aspp_subnet.name], d_aspp, need_dx=False)[1])
        self.last_forward["grads"] = grads
        self.last_forward["weight_grads"] = wg
        optimizer.apply_gradients(params, wg, trainable=names)
        self.repack("head_tune" if tune else "heads")
        return outputs

    def _head_tune_backward(self, tapes, grads, wg):
        """The detection side of a "head_tune" step: the towers' and the mask head's backward with their input gradients kept,
        summed per pyramid level in the fixed order class tower, box tower, RoI align (in place on the class tower's
        tensors), then the extra levels' and the FPN's backward.  Fills `wg`."""
        _, fpn_subnet, cls_subnet, loc_subnet = self.detection_networks
        bb = self.backbone_network
        d_feat, g = cls_subnet.backward(tapes[cls_subnet.name], grads["cls_pred"])
        wg.update(g)
        d_loc, g = loc_subnet.backward(tapes[loc_subnet.name], grads["loc_pred"])
        wg.update(g)
        d_feat = [ops.add_(a, b) for a, b in zip(d_feat, d_loc)]
        if self.instance_networks is not None:
            pyramid_roi_align, mask_subnet = self.instance_networks[2:4]
            d_rois, g = mask_subnet.backward(tapes[mask_subnet.name], grads["roi_masks"], need_dx=True)
            wg.update(g)
            t = tapes[pyramid_roi_align.name]
            n = len(t["fmap_shapes"])
            pyramid_roi_align.backward(d_rois, t["fmap_shapes"], t["rows"], t["image_hw"], t["slots"], t["lcounts"],
                                       add=d_feat[:n], out=d_feat[:n])
        n_fpn = len(tapes[fpn_subnet.name]["inputs"])
        extra = dict(zip(tapes["feature_names"][n_fpn:], d_feat[n_fpn:]))       # gradients at other backbone taps are dropped
        wg.update(bb.backward_extra_levels(tapes[bb.name], extra.get("P6"), extra.get("P7"), need_dx=False)[1])
        wg.update(fpn_subnet.backward(tapes[fpn_subnet.name], d_feat[:n_fpn], need_dx=False)[1])

    def _forward(self, inputs, want):
        if self.device is None:
            raise RuntimeError("TrainerModel: call load_weights(weights, device) first")
        cfg = self.configuration
        x = self._named_inputs(inputs)
        images = self._dev(x['images'])
        bb = self.backbone_network
        tune = want is not None and want.get("head_tune")
        if tune:
            feats, want["tapes"][bb.name] = bb.call_with_tape(images)
        else:
            feats = bb(images)
        by_name = dict(zip(bb.output_names, feats))
        fw, outputs = {}, []
        if self.detection_networks is not None:
            det_config = cfg.detection
            prior_subnet, fpn_subnet, cls_subnet, loc_subnet = self.detection_networks
            pr_boxes = prior_subnet(images)
            fpn_inputs = [by_name[n] for n in bb.output_names if n in det_config.feature_pyramid_inputs]
            without_fpn = [by_name[n] for n in bb.output_names if n not in det_config.feature_pyramid_inputs]
            if tune:
                fpn_outputs, want["tapes"][fpn_subnet.name] = fpn_subnet.call_with_tape(fpn_inputs)
                want["tapes"]["feature_names"] = [n for n in bb.output_names if n in det_config.feature_pyramid_inputs] + \
                    [n for n in bb.output_names if n not in det_config.feature_pyramid_inputs]
            else:
                fpn_outputs = fpn_subnet(fpn_inputs)
            feature_outputs = fpn_outputs + without_fpn
            cls_pred = self._head(cls_subnet, feature_outputs, want)
            loc_pred = self._head(loc_subnet, feature_outputs, want)
            gt_boxes = self._dev(x['gt_boxes'], torch.float32)
            gt_boxes_exist = self._dev(x['gt_boxes_exist'], torch.float32)
            cls_true, loc_true, assign_mask = self.assign_boxes([gt_boxes, pr_boxes])
            outputs += [self._loss(self.class_loss, [cls_true, cls_pred, assign_mask, gt_boxes_exist], want),
                        self._loss(self.box_loss, [loc_true, loc_pred, assign_mask], want)]
            # The metric's proposals stay at capacity (-1 padded): DetectionIOUMetric counts rows, so the reference's
            # trimmed tensor gives the same numbers, and nothing is read by the host.
            restored_boxes = self.metric_restore([loc_pred, pr_boxes])
            proposed, _, _ = self.metric_proposal.propose_fixed(cls_pred, restored_boxes)
            outputs += list(self.detection_metric([proposed, gt_boxes]))
            fw.update(cls_pred=cls_pred, loc_pred=loc_pred, pr_boxes=pr_boxes, proposed=proposed, cls_true=cls_true,
                      loc_true=loc_true, assign_mask=assign_mask, best_prior=self.assign_boxes.last_best)
            if self.instance_networks is not None:
                restore_layer, distribute_layer, pyramid_roi_align, mask_subnet = self.instance_networks
                restored_boxes = restore_layer([loc_pred, pr_boxes])
                proposed_loss, _, _ = self.loss_proposal.propose_fixed(cls_pred, restored_boxes)
                # gt_boxes' -1 rows sit in the MIDDLE of this list: the distribute kernel drops every row with cx == -1
                # wherever it is (csrc/detect.hip), and the crops are taken from the per-level slot lists it writes
                chosen_boxes = torch.cat([gt_boxes, proposed_loss], dim=1)              # Concatenate(axis=1)
                dist_boxes = distribute_layer(chosen_boxes)
                if tune:
                    # PyramidRoiAlign.call taken apart, so that its backward gets the tables this forward used
                    fmaps, rows = feature_outputs[:cfg.instance.max_k + 1], dist_boxes.contiguous()
                    image_hw = (int(images.shape[1]), int(images.shape[2]))
                    slots, lcounts, lmax = pyramid_roi_align.distribute(len(fmaps), rows, True)
                    roi_fmaps, roi_boxes = pyramid_roi_align.crop_distributed(fmaps, rows, image_hw, slots, lcounts, lmax)
                    want["tapes"][pyramid_roi_align.name] = dict(rows=rows, slots=slots, lcounts=lcounts, image_hw=image_hw,
                                                                 fmap_shapes=[tuple(f.shape) for f in fmaps])
                else:
                    roi_fmaps, roi_boxes = pyramid_roi_align([feature_outputs[:cfg.instance.max_k + 1], dist_boxes, images])
                roi_masks = self._head(mask_subnet, roi_fmaps, want)
                gt_masks = self._dev(x['gt_masks'])
                match_gt_masks = self.assign_masks([roi_boxes, roi_masks, gt_boxes, gt_masks])
                outputs.append(self._loss(self.mask_loss, [match_gt_masks, roi_masks], want))
                fw.update(proposed_loss=proposed_loss, roi_boxes=roi_boxes, roi_masks=roi_masks, match_gt_masks=match_gt_masks)
        if self.semantic_networks is not None:
            sem_config = cfg.semantic
            aspp_subnet, seg_subnet = self.semantic_networks
            aspp_out = self._head(aspp_subnet, by_name[sem_config.aspp_input_name], want)
            seg_pred = self._head(seg_subnet, [aspp_out, by_name[sem_config.skip_input_name]], want)
            gt_seg = self._dev(x['gt_seg'])
            gt_seg_exist = self._dev(x['gt_seg_exist'], torch.float32)
            seg_assigned = self.assign_seg([gt_seg, seg_pred])
            outputs.append(self._loss(self.seg_loss, [seg_assigned, seg_pred, gt_seg_exist], want))
            outputs += list(self.class_iou([seg_assigned, seg_pred]))
            fw.update(seg_pred=seg_pred, seg_assigned=seg_assigned)
        self.last_forward = fw
        return outputs

    def predict(self, inputs, **kwargs):
        """Keras `Model.predict` with named outputs: {output name: float32 [B] ndarray}."""
        outs = self.call(inputs, **kwargs)
        torch.cuda.synchronize(self.device)
        return {n: o.cpu().numpy() for n, o in zip(self.output_names, outs)}


def construct_trainer_network(configuration: ModelConfiguration, backbone_network, detection_networks=None,
                              semantic_networks=None, instance_networks=None):
    """Same signature as reference :223-227; the returned model trains its head groups (train_on_batch) and, as the "head_tune" stage, the FPN and P6 / P7; the backbone's body is frozen."""
    return TrainerModel(configuration, backbone_network, detection_networks=detection_networks,
                        semantic_networks=semantic_networks, instance_networks=instance_networks)


def construct_masklab_networks(config: ModelConfiguration, with_trainer=False):
    """Reference :201-220 returns (trainer, inference).  The trainer network (losses and metrics of a batch with
    ground truth, gradients at the head outputs) is built on request; by default the first element is None."""
    K.clear_session()
    backbone_network = build_backbone_network(config)
    detection_networks = build_detection_network(config)
    instance_networks = build_instance_network(config)
    semantic_networks = build_semantic_network(config)
    inference = construct_inference_network(configuration=config, backbone_network=backbone_network,
                                            detection_networks=detection_networks,
                                            semantic_networks=semantic_networks,
                                            instance_networks=instance_networks)
    trainer = None
    if with_trainer:                      # after the inference model, whose automatic layer names stay what they were
        trainer = construct_trainer_network(configuration=config, backbone_network=backbone_network,
                                            detection_networks=detection_networks,
                                            semantic_networks=semantic_networks,
                                            instance_networks=instance_networks)
    return trainer, inference


class DeployModel(K.Layer):
    """The non-serving `Model(images -> (detection, instance, semantic))` that reference
    load_masklab_inference_model_from_h5 assembles around the inference network (:598-643):
    DownSampleInput(config.postprocess.resolution) -> inference model -> TrimInstances(mold=True),
    per-class SemanticSmoothing + ResizeLike(target=downsampled) -> UpSampleOutput(target=images).
    All three outputs are int32: detection [B,n,6] (cx,cy,w,h,label,conf*100 at input resolution),
    instance [B,n,h,w] (0/1), semantic [B,H,W,classes] (0/1)."""

    def __init__(self, configuration, inference_model, name='inference'):
        super().__init__(name=name)
        if inference_model.output_names != ['cls_pred', 'loc_pred', 'roi_boxes', 'roi_masks', 'seg_pred']:
            raise ValueError("the deploy wrapper unpacks five outputs (reference :608): it needs the detection, "
                             "instance and semantic heads")
        post = configuration.postprocess
        if len(post.smoothing_kernel_sizes) != len(post.smoothing_weights):
            raise ValueError("postprocess.smoothing_kernel_sizes and smoothing_weights differ in length")
        self.configuration = configuration
        self.model = inference_model
        self.down_sample = DownSampleInput(post.resolution)
        self.trim = TrimInstances(mold=True)
        self.smoothing = [SemanticSmoothing(kernel_size=k, weight=w)
                          for k, w in zip(post.smoothing_kernel_sizes, post.smoothing_weights)]
        self.resize_like = ResizeLike()
        self.up_sample = UpSampleOutput()
        self.output_names = ['detection', 'instance', 'semantic']
        self.built = True

    def call(self, images, **kwargs):
        if not isinstance(images, torch.Tensor):
            images = torch.as_tensor(np.asarray(images))
        if self.model.device is None:
            raise RuntimeError("DeployModel: load weights into the inference model first")
        images = images.to(self.model.device).contiguous()
        downsampled = self.down_sample(images)                                     # :607
        _, _, box_pred, mask_pred, seg_pred = self.model(downsampled)              # :608
        detection_pred, instance_pred = self.trim([box_pred, mask_pred])           # :614-615
        n_split = len(self.smoothing)
        n_cls = int(seg_pred.shape[-1])
        if n_cls % n_split:
            raise ValueError(f"tf.split: {n_cls} semantic classes do not split into {n_split} parts (:619)")
        rep = n_cls // n_split
        post_semantics = SemanticSmoothing.smooth_classes(                         # :619-627 in one launch group
            seg_pred, [l.kernel_size for l in self.smoothing for _ in range(rep)],
            [l.weight for l in self.smoothing for _ in range(rep)])
        semantic_pred = self.resize_like(post_semantics, target=downsampled)       # :628
        return self.up_sample([detection_pred, instance_pred, semantic_pred], target=images)   # :634-635

    def predict(self, images, **kwargs):
        outs = self.call(images, **kwargs)
        torch.cuda.synchronize(self.model.device)
        return [o.cpu().numpy() for o in outs]


def construct_deploy_network(configuration: ModelConfiguration, inference_model):
    """Wrap an inference model like reference :598-643 (serving=False)."""
    return DeployModel(configuration, inference_model)


class ServingModel(K.Layer):
    """The arithmetic of reference road_project/setup/serving.py:16-52 (`load_serving_model_from_h5`):
    deploy model -> CropAndPadMask -> SummaryOutput, the 'summarize' tensor float32 [B,n',11]
    (class, cx, cy, w, h, conf, pixel count, instance size, horizontal size, vertical size, include_my_road).
    visualize=True adds the 'visualize' output in front, the reference's order: the frame uint8 [B,H,W,3] after
    DrawBoxes -> DrawInstance(instance colours) -> DrawSegmentation(semantic colours) (:32-40), colours and alphas from
    configuration.postprocess.  encode=True (with visualize=True) finishes it like the reference (:41): the first output
    is EncodeImageContent's JPEG content, encoded on the device (ops.encode_jpeg) -- `call` returns (buffer uint8
    [B,capacity], lengths int32 [B]) in its place, both on the device, and `predict` one `bytes` per image.  The frames
    come in decoded; masklab_hip.serving puts DecodeImageContent in front."""

    def __init__(self, configuration, deploy_model, name='serving', visualize=False, encode=False):
        super().__init__(name=name)
        if encode and not visualize:
            raise ValueError("ServingModel(encode=True) encodes the 'visualize' output: it needs visualize=True")
        post = configuration.postprocess
        self.deploy_model = deploy_model
        self.crop_and_pad = CropAndPadMask()
        self.summary = SummaryOutput(default_road_size=post.default_road_size)
        self.visualize = bool(visualize)
        if self.visualize:
            self.draw_boxes = DrawBoxes()
            self.draw_instance = DrawInstance(post.instance_colors, post.instance_alpha)
            self.draw_segmentation = DrawSegmentation(post.semantic_colors, post.semantic_alpha)
        self.encode = bool(encode)
        if self.encode:
            self.encode_content = EncodeImageContent()
        self.output_names = ['visualize', 'summarize'] if self.visualize else ['summarize']
        self.built = True

    def _content(self, vis):
        from . import ops
        return ops.encode_jpeg(vis, self.encode_content.quality) if self.encode else vis

    def call(self, images, **kwargs):
        if not isinstance(images, torch.Tensor):
            images = torch.as_tensor(np.asarray(images))
        images = images.to(self.deploy_model.model.device).contiguous()
        if self.visualize and images.dtype != torch.uint8:
            raise ValueError(f"ServingModel(visualize=True) draws into uint8 frames, got {images.dtype}")
        det_outs, ins_outs, seg_outs = self.deploy_model(images)                            # :27-29
        if kwargs.get("materialise_masks", False):                                          # the reference's literal wiring
            crop_and_pad_masks = self.crop_and_pad([images, det_outs, ins_outs, seg_outs])  # :30
            summary = self.summary([det_outs, seg_outs, crop_and_pad_masks])                # :47-48
            if not self.visualize:
                return summary
            vis = self.draw_boxes([images, det_outs])                                       # :34
            vis = self.draw_instance([vis, det_outs, crop_and_pad_masks])                   # :35-37
            vis = self.draw_segmentation([vis, seg_outs])                                   # :38-40
            return [self._content(vis), summary]                                            # :41
        # CropAndPadMask folded into SummaryOutput: same numbers bit for bit, no [B,n,H,W] tensor
        summary = self.summary([det_outs, seg_outs, ins_outs], from_rois=True)
        if not self.visualize:
            return summary
        # the three Draw* layers over CropAndPadMask in one kernel: same bytes, no [B,n,H,W] tensor
        from . import ops
        di, ds = self.draw_instance, self.draw_segmentation
        vis = ops.serving_visualize(images, det_outs.contiguous(), ins_outs.contiguous(), seg_outs.contiguous(), di.colors,
                                    di.alpha, ds.colors, ds.alpha)
        return [self._content(vis), summary]

    def predict(self, images, **kwargs):
        out = self.call(images, **kwargs)
        torch.cuda.synchronize(self.deploy_model.model.device)
        if self.encode:
            from . import ops
            return [ops.jpeg_contents(*out[0]), out[1].cpu().numpy()]
        if self.visualize:
            return [o.cpu().numpy() for o in out]
        return out.cpu().numpy()


def construct_serving_network(configuration: ModelConfiguration, deploy_model, visualize=False, encode=False):
    return ServingModel(configuration, deploy_model, visualize=visualize, encode=encode)


def load_masklab_inference_model_from_weights(weights, config: ModelConfiguration, device="cuda"):
    """Counterpart of reference load_masklab_inference_model_from_h5 (:498-643) for a name-keyed
    weight dict / .npz (see tools/convert_keras_h5.py for the h5 -> npz step): builds the networks
    from `config`, loads the weights and returns the deploy model."""
    if isinstance(weights, str):
        with np.load(weights) as z:
            weights = {k: z[k] for k in z.files}
    _, inference = construct_masklab_networks(config)
    inference.load_weights(weights, device)
    return construct_deploy_network(config, inference)


def load_masklab_inference_model_from_h5(save_path, config: ModelConfiguration, serving=False, device="cuda"):
    """Same name and arguments as reference engine/retinamasklab.py:498-643: the checkpoint at `save_path` -> the deploy
    model `images uint8 [B,H,W,3] -> (detection, instance, semantic)` (DownSampleInput -> inference network ->
    TrimInstances / SemanticSmoothing / ResizeLike -> UpSampleOutput).  `save_path`: a Keras .h5 as the reference
    writes it (needs `h5py`, imported lazily; the layer-name re-wiring of :515-586 becomes masklab_hip/checkpoint.py's
    name mapping) or the .npz tools/convert_keras_h5.py makes of it.  The networks are built from `config` (the
    reference rebuilds them from the loaded Keras model; `config.json` saved beside the weights, engine/train.py:31-32,
    is that configuration).  serving=True puts DecodeImageContent (JPEG bytes in, misc.py:328-337) in front: here that
    wiring lives in masklab_hip.serving.load_serving_model_from_h5 (content bytes in, [JPEG content, summary] out),
    built on the serving=False model; this function keeps refusing it."""
    if serving:
        raise NotImplementedError("load_masklab_inference_model_from_h5(serving=True) wraps the model in "
                                  "DecodeImageContent (JPEG byte strings in): image decoding is outside the accelerated "
                                  "path -- decode on the host and use the serving=False model (or construct_serving_network "
                                  "for the summary outputs)")
    _, inference = construct_masklab_networks(config)
    path = str(save_path)
    if path.lower().endswith(".npz"):
        with np.load(path) as z:
            weights = {k: z[k] for k in z.files}
    else:
        from . import checkpoint
        specs = {k: tuple(v.shape) for k, v in inference.weight_specs().items()}
        weights = checkpoint.load_keras_h5(path, specs)
    inference.load_weights(weights, device)
    return construct_deploy_network(config, inference)


def find_layer_name(re_format, model):
    return sorted([layer.name for layer in model.layers if re_format.match(layer.name)])
