"""Backbone loader + preprocess -- drop-in for reference engine/backbone/base.py
(BackBonePreProcess :22-84, BACKBONE_LAYERS :104-182, load_backbone :185-316).

Backbones on the hot path: 'resnet50' (the reference's default: tf.keras.applications.ResNet50, the legacy
Keras-Applications model, restated in backbone/resnet50.py), 'resnext50' (in-tree in the reference), 'seresnet34' (the
reference project's own model, vendored thirdparty/classification_models), 'seresnet50' and 'seresnext50' (the same
vendored model zoo, senet.py), 'resnext101' (a build-side extension: the model zoo's resnext.py, which the reference
never wires in) and 'mobilenet' (tf.keras.applications.MobileNet v1); BACKBONES pairs each with its body class, preprocess
and extra-level padding, and the six residual bodies share backbone/body.py.  Everything else raises NotImplementedError
like the reference does for unknown types.  BatchNormalization is folded into the conv weights at load time; the
3-channel stems read a channel-padded NHWC4 image written by the preprocess kernel.
"""
from .. import ops
from ..keras_like import Conv2D, DepthwiseConv2D, GroupedConv2D, Layer
from ..layers.misc import Identity
from ..normalization import GroupNormalization
from .body import input_affine
from .mobilenet import MobileNetV1
from .resnet50 import ResNet50
from .resnext import ResNeXt50
from .resnext101 import ResNeXt101
from .senet import SEResNet50, SEResNeXt50
from .seresnet34 import SEResNet34

BACKBONE_LAYERS = {
    # the reference's default (reference :105-111): Keras auto-named Activations of the legacy Keras-Applications ResNet50
    "resnet50": {"C1": 'activation', "C2": 'activation_9', "C3": "activation_21", "C4": "activation_39",
                 "C5": "activation_48"},
    "resnext50": {"C1": 'conv1_relu', "C2": 'conv2_block3_out', "C3": "conv3_block4_out",
                  "C4": "conv4_block6_out", "C5": "conv5_block3_out"},
    # build-side extension: architecture from the vendored thirdparty model zoo
    "resnext101": {"C1": "relu0", "C2": "stage1_unit3_relu", "C3": "stage2_unit4_relu",
                   "C4": "stage3_unit23_relu", "C5": "stage4_unit3_relu"},
    # the reference project's own backbone (road_project/train.py:36-37; taps reference :126-132)
    "seresnet34": {"C1": "relu0", "C2": "stage2_unit1_relu1", "C3": "stage3_unit1_relu1", "C4": "stage4_unit1_relu1",
                   "C5": "relu1"},
    # vendored thirdparty senet.py (reference :133-146): Keras auto-named Activations, see backbone/senet.py
    "seresnet50": {"C1": "activation", "C2": "activation_15", "C3": "activation_35", "C4": "activation_65",
                   "C5": "activation_80"},
    "seresnext50": {"C1": "activation", "C2": "activation_16", "C3": "activation_36", "C4": "activation_66",
                    "C5": "activation_80"},
    "mobilenet": {"C1": "conv_pw_1_relu", "C2": "conv_pw_3_relu", "C3": "conv_pw_5_relu",
                  "C4": "conv_pw_11_relu", "C5": "conv_pw_13_relu"},
}

# backbone_type -> (body class, BackBonePreProcess arguments, padding of the extra-level convs); reference :190-279, and
# :292-314 for the padding: mobilenet pads ((0, 1), (0, 1)) + valid, the others 'same'
BACKBONES = {
    "resnet50": (ResNet50, dict(rgb=False, mean_shift=True, normalize=0), 'same'),                    # :190-193
    "resnext50": (ResNeXt50, dict(rgb=True, mean_shift=True, normalize=2), 'same'),                   # :215-217
    "resnext101": (ResNeXt101, dict(rgb=True, mean_shift=False, normalize=0), 'same'),                # then bn_data
    "seresnet34": (SEResNet34, dict(rgb=True, mean_shift=False, normalize=0), 'same'),                # :232-234, then bn_data
    "seresnet50": (SEResNet50, dict(rgb=True, mean_shift=True, normalize=3), 'same'),                 # :220-223
    "seresnext50": (SEResNeXt50, dict(rgb=True, mean_shift=True, normalize=3), 'same'),               # :238-241
    "mobilenet": (MobileNetV1, dict(rgb=False, mean_shift=False, normalize=2), ((0, 1), (0, 1))),     # :254-256
}


class BackBonePreProcess(Layer):
    """Image preprocess (reference :22-84): optional BGR flip, mean shift, normalisation mode
    0 none / 1 [0,1] / 2 [-1,1] / 3 standardisation.  Output is NHWC4 (4th channel zero) so the
    MFMA stem can read 16-byte pixels; `out_channels=3` gives the plain tensor."""

    def __init__(self, rgb=True, mean_shift=False, normalize=0, out_channels=4, **kwargs):
        self.rgb = rgb
        self.mean_shift = mean_shift
        self.normalize = normalize
        self.out_channels = out_channels
        super().__init__(**kwargs)
        self.mean = [123.68, 116.779, 103.939] if rgb else [103.939, 116.779, 123.68]
        self.std = [0.225, 0.224, 0.229] if rgb else [0.229, 0.224, 0.225]
        self.extra_affine = None      # (mean, divisor, shift) of a model-owned input BatchNorm (ResNeXt-101 bn_data)

    def build(self, input_shape):
        self.built = True
        return tuple(input_shape[:3]) + (self.out_channels,)

    def call(self, inputs, **kwargs):
        mean = self.mean if self.mean_shift else [0.0, 0.0, 0.0]
        if self.normalize == 1:
            div, shift = 255.0, 0.0
        elif self.normalize == 2:
            div, shift = 127.5, (0.0 if self.mean_shift else -1.0)
        elif self.normalize == 3:
            div, shift = [255.0 * s for s in self.std], 0.0          # x / 255 / std (:71-73)
        else:
            div, shift = 1.0, 0.0
        if self.extra_affine is not None:
            if self.normalize != 0 or self.mean_shift:
                raise NotImplementedError("an input BatchNorm is only combined with the raw (normalize=0) mode")
            mean, div, shift = self.extra_affine
        return ops.preprocess(inputs, flip=not self.rgb, mean=mean, divisor=div, shift=shift,
                              out_channels=self.out_channels)

    def get_config(self):
        config = super().get_config()
        config.update({"rgb": self.rgb, "mean_shift": self.mean_shift, "normalize": self.normalize})
        return config


class BackboneModel(Layer):
    """What `load_backbone` returns: callable images -> [features], with Keras-Model-like
    `.output_names` (C-taps ascending, then P6, P7 -- reference :287-314)."""

    def __init__(self, backbone_type, backbone_outputs, num_features, **kwargs):
        super().__init__(name=backbone_type, **kwargs)
        bt = backbone_type.lower()
        if bt not in BACKBONES:
            raise NotImplementedError(
                f"backbone_type must be one of {list(BACKBONES)} on the MI355X path (got '{backbone_type}')")
        body, preprocess, pad = BACKBONES[bt]
        self.backbone_type = bt
        self.backbone_outputs = tuple(backbone_outputs)
        self.num_features = num_features
        self.preprocess = BackBonePreProcess(**preprocess)
        self.body = body()
        self.taps = [k for k in ("C1", "C2", "C3", "C4", "C5") if k in self.backbone_outputs]
        if not self.taps:
            raise ValueError("backbone_outputs must name at least one C-level")
        self.identities = {k: Identity(name=k) for k in self.taps}
        self.p6_conv = Conv2D(num_features, (3, 3), strides=(2, 2), padding=pad, activation='relu', name='P6_conv')
        self.p6_norm = GroupNormalization(name='P6_norm')          # default groups=32 (Appendix B.2)
        self.p7_conv = Conv2D(num_features, (3, 3), strides=(2, 2), padding=pad, activation='relu', name='P7_conv')
        self.output_names = list(self.taps)
        if 'P6' in self.backbone_outputs:
            self.output_names.append('P6')
        if 'P7' in self.backbone_outputs:
            self.output_names.append('P7')
        self.input_names = ['images']

    def build(self, input_shape=(None, None, None, 3)):
        s = self.preprocess.build(input_shape)
        tap_shapes = self.body.build(s)
        shapes = [tap_shapes[k] for k in self.taps]
        s6 = self.p6_conv.build(shapes[-1])
        self.p6_norm.build(s6)
        s7 = self.p7_conv.build(s6)
        if 'P6' in self.backbone_outputs:
            shapes.append(s6)
        if 'P7' in self.backbone_outputs:
            shapes.append(s7)
        self.built = True
        self.output_shapes = shapes
        return shapes

    def children(self):
        return [self.body, self.p6_conv, self.p6_norm, self.p7_conv]

    def weight_specs(self):
        out = {}
        for ch in self.children():
            out.update(ch.weight_specs())
        return out

    def load_weights(self, weights, device):
        super().load_weights(weights, device)
        eps = getattr(self.body, "INPUT_BN_EPS", None)
        if eps is not None:
            self.preprocess.extra_affine = input_affine(weights, eps)

    def call(self, images, **kwargs):
        return self._forward(images, kwargs.get("fork_stream"))

    def call_with_tape(self, images):
        """`call` without fork_stream (the same launches on one stream: the same bits; the body as in `call`, frozen and
        folded) and what backward_extra_levels needs.  -> (feats, tape): tape = {"c5": the last C tap, "p6": P6_conv's
        post-ReLU output, "g6": P6_norm's output, "p7": P7_conv's post-ReLU output}."""
        tape = {}
        return self._forward(images, None, tape), tape

    def extra_level_layers(self):
        """The layers behind the last C tap: what a head-tune step trains of the backbone, asked for their device_params()
        one by one (BackboneModel.device_params() keeps raising for the folded body)."""
        return [self.p6_conv, self.p6_norm, self.p7_conv]

    def backward_extra_levels(self, tape, d_p6, d_p7, need_dx=False):
        """Backward of the two extra levels.  tape: call_with_tape's; d_p6 / d_p7: the gradients at the exported P6 (PRE-norm,
        post-ReLU) and P7, float32, or None for a level nobody reads.  In this order: relu_grad at p7; P7_conv's weight
        gradient and its stride-2 data gradient (ops.conv2d_dgrad_s2); P6_norm.backward; its result plus d_p6, through p6's
        ReLU; P6_conv's weight gradient and, with need_dx, its stride-2 data gradient.
        -> (the gradient at the last C tap or None unless need_dx, {full weight name: gradient}).  d_p7 None leaves P7_conv
        and P6_norm without a gradient; both None returns (None, {})."""
        from ..keras_like import check_incoming_grad
        grads = {}
        p6, g6, p7 = tape["p6"], tape["g6"], tape["p7"]
        total = None
        if d_p7 is not None:
            check_incoming_grad("BackboneModel.backward_extra_levels: d_p7", d_p7, p7.shape)
            dz7 = ops.relu_grad(p7, d_p7)
            d_g6, g = self.p7_conv.backward(g6, dz7, strided_dx=True)
            self.p7_conv.name_grads(g, grads)
            total, g = self.p6_norm.backward(p6, d_g6, inplace=True)
            self.p6_norm.name_grads(g, grads)
        if d_p6 is not None:
            check_incoming_grad("BackboneModel.backward_extra_levels: d_p6", d_p6, p6.shape)
            total = ops.add_(total, d_p6) if total is not None else d_p6
        if total is None:
            return None, grads
        dz6 = ops.relu_grad(p6, total, out=total if d_p7 is not None else None)      # never over the caller's d_p6
        d_c5, g = self.p6_conv.backward(tape["c5"], dz6, need_dx=need_dx, strided_dx=True)
        self.p6_conv.name_grads(g, grads)
        return d_c5, grads

    def _forward(self, images, fork, tape=None):
        x = self.preprocess(images)
        taps = self.body(x, wanted=self.taps)
        feats = [self.identities[k](taps[k]) for k in self.taps]
        # The extra levels are three small launches (16- and 4-tile convs, a 64-block GroupNorm: ~0.14 ms during which
        # most of the chip idles).  A caller that has other work for the main stream (the FPN chain) passes
        # `fork_stream` and joins `self.pending_stream` before it consumes P6 / P7.
        aux = fork("_extra_level_stream") if fork is not None else None
        self.pending_stream = aux
        import contextlib
        import torch
        with (torch.cuda.stream(aux) if aux is not None else contextlib.nullcontext()):
            p6 = self.p6_conv(feats[-1])
            g6 = self.p6_norm(p6)                              # new tensor: P6 itself stays intact
            p7 = self.p7_conv(g6)
        if tape is not None:
            tape.update(c5=feats[-1], p6=p6, g6=g6, p7=p7)
        if 'P6' in self.backbone_outputs:
            feats.append(p6)                                   # exported P6 is PRE-norm (:308-309)
        if 'P7' in self.backbone_outputs:
            feats.append(p7)
        return feats

    def join_extra_levels(self, feats):
        """Make the current stream wait for the P6 / P7 chain started by call(fork_stream=...)."""
        import torch
        aux = getattr(self, "pending_stream", None)
        if aux is None:
            return
        cur = torch.cuda.current_stream()
        cur.wait_stream(aux)
        for name, t in zip(self.output_names, feats):
            if name in ("P6", "P7"):
                t.record_stream(cur)
        self.pending_stream = None


def load_backbone(backbone_type="resnet50", backbone_outputs=('C3', 'C4', 'C5', 'P6', 'P7'), num_features=256):
    """Same signature as reference engine/backbone/base.py:185-187."""
    if backbone_type.lower() not in BACKBONE_LAYERS:
        raise NotImplementedError(
            f"backbone_type must be one of {list(BACKBONE_LAYERS.keys())} (got '{backbone_type}'); the other "
            f"reference backbones build on code the reference does not vendor (keras_applications, "
            f"tf.keras.applications, efficientnet) and are outside the accelerated hot path")
    model = BackboneModel(backbone_type, backbone_outputs, num_features)
    model.build((None, None, None, 3))
    return model
