"""ResNet-50 body -- the reference's DEFAULT backbone (engine/config.py:51, load_backbone's default argument,
engine/backbone/base.py:185-195, taps :105-111).  The reference does not vendor the architecture: base.py imports
tensorflow.keras.applications.ResNet50 (TF 1.x), and its tap names (`activation`, `activation_9`, `activation_21`,
`activation_39`, `activation_48`) are Keras auto-names, which only the legacy Keras-Applications 1.0.x resnet50.py
produces (49 Activations = 1 + 3 (3 + 4 + 6 + 3); the later resnet_common variant names its outputs `conv2_block3_out`).
That published model, restated:
    conv1_pad ZeroPadding 3, conv1 64 x 7x7 / 2 valid WITH bias, bn_conv1, ReLU (= activation, tap C1),
    pool1_pad ZeroPadding 1, max-pool 3x3 / 2 valid;
    stages 2..5 with blocks a..c / a..d / a..f / a..c and filters (64, 64, 256) .. (512, 512, 2048); block `a` is a
    conv_block whose shortcut res{s}a_branch1 (1x1) + bn{s}a_branch1 and branch2a both carry the stride (1 in stage 2,
    2 in stages 3-5), the others are identity_blocks;
    block: res{s}{b}_branch2a 1x1 + bn + ReLU, branch2b 3x3 'same' + bn + ReLU, branch2c 1x1 + bn, Add, ReLU; every conv
    has a bias; every BatchNormalization the Keras default epsilon 1e-3, with scale and centre.
Taps activation_9 / _21 / _39 / _48 are the outputs of the last block of stages 2..5.  53 convs + 53 BNs, 23 587 712
parameters (53 120 of them BN moving statistics).  Preprocess BackBonePreProcess(rgb=False, mean_shift=True, normalize=0):
BGR flip, subtract [103.939, 116.779, 123.68].  Layers keep their Keras names, so a Keras checkpoint loads by name.

Every BatchNorm is folded into its conv (the conv's bias included); ReLU and the identity blocks' Add are conv epilogues.
The first block of a stage, relu(bn(conv_2c(y)) + bn(conv_1(x))), is two GEMMs that end in the same output tile: with
ops.set_projection_fusion("on") it runs as ONE GEMM over the concatenated K of y and x (csrc/conv1x1_dual.hip; conv maths
"f32" and "f16s"), x read in place at the block's stride and the shortcut tensor never written; "off", and in "f32x3" /
"f16", it is the shortcut conv followed by the 2c conv with the shortcut as residual."""
from .. import ops
from ..keras_like import Conv2D
from .body import ResidualBody

BN_EPS = 1e-3
STAGES = ((2, "abc", (64, 64, 256), 1), (3, "abcd", (128, 128, 512), 2), (4, "abcdef", (256, 256, 1024), 2),
          (5, "abc", (512, 512, 2048), 2))


class _DualPack:
    """The one-GEMM operand of a projection unit, made when the unit's weights are loaded (after its two convs)."""

    def __init__(self, conv_a, conv_x):
        self.conv_a, self.conv_x, self.dev = conv_a, conv_x, None

    def weight_specs(self):
        return {}

    def load_weights(self, weights, device):
        ka, ba = self.conv_a.folded(weights)
        kx, bx = self.conv_x.folded(weights)
        self.dev = ops.DeviceDualConv(ka, ba, kx, bx, device, dc_a=self.conv_a.dev, dc_x=self.conv_x.dev)


class _Block:
    """conv_block (`shortcut`) or identity_block of stage `s`, block letter `b`."""

    def __init__(self, filters, stage, block, stride, shortcut):
        conv, bnn = f"res{stage}{block}_branch", f"bn{stage}{block}_branch"
        # synthetic-init gamma ranges: the residual branch's last BN starts small so that random weights keep the taps O(1)
        # through 16 residual additions, as resnext.py does; biases are drawn too, so that the bias fold is exercised
        # (real checkpoints override both)
        rng = {"1": (0.5, 1.0), "2a": (0.5, 1.5), "2b": (0.5, 1.5), "2c": (0.1, 0.3)}
        kw = lambda s: dict(fold_bn=(bnn + s, BN_EPS, True, rng[s]), name=conv + s, kernel_initializer="he_normal",
                            bias_initializer="normal")
        f1, f2, f3 = filters
        self.stride = stride
        self.conv2a = Conv2D(f1, 1, strides=stride, activation='relu', **kw("2a"))
        self.conv2b = Conv2D(f2, 3, padding='same', activation='relu', **kw("2b"))
        self.conv2c = Conv2D(f3, 1, activation='relu', **kw("2c"))              # + Add + ReLU in its epilogue
        self.shortcut = Conv2D(f3, 1, strides=stride, **kw("1")) if shortcut else None
        self.dual = _DualPack(self.conv2c, self.shortcut) if shortcut else None

    def layers(self):
        """In the published model's creation order: 2a, 2b, 2c, [shortcut]; then the unit's one-GEMM packing."""
        return [l for l in (self.conv2a, self.conv2b, self.conv2c, self.shortcut, self.dual) if l is not None]

    def build(self, shape):
        s = self.conv2c.build(self.conv2b.build(self.conv2a.build(shape)))
        if self.shortcut is not None:
            sc = self.shortcut.build(shape)
            assert tuple(s[1:]) == tuple(sc[1:]) or None in s, (s, sc)
        return s

    def __call__(self, x):
        y = self.conv2b(self.conv2a(x))
        if self.shortcut is None:
            return self.conv2c(y, residual=x)
        if ops.projection_fused():
            return ops.conv1x1_dual(y, x, self.dual.dev, self.stride)
        return self.conv2c(y, residual=self.shortcut(x))


class ResNet50(ResidualBody):
    def __init__(self, **kwargs):
        super().__init__(name=kwargs.pop("name", "resnet50_body"), **kwargs)
        # synthetic init: the stem reads raw mean-shifted pixels (rms ~ 74), so bn_conv1's gamma starts at ~ 1 / 100
        self.stem = Conv2D(64, 7, strides=2, padding=((3, 3), (3, 3)),
                           fold_bn=("bn_conv1", BN_EPS, True, (0.005, 0.015)), activation='relu', image_input=True,
                           kernel_initializer="he_normal", bias_initializer="normal", name="conv1")
        self.stages = [[_Block(filters, stage, b, stride if b == "a" else 1, b == "a") for b in blocks]
                       for stage, blocks, filters, stride in STAGES]
