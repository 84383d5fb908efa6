"""SE-ResNet-34 body -- the backbone the reference project trains and serves (road_project/train.py:36-37; load_backbone
engine/backbone/base.py:229-237, taps :126-132).  Architecture from the vendored thirdparty/classification_models:
resnet.py ResNet :173-283 with MODELS_PARAMS['seresnet34'] :297 (repetitions (3, 4, 6, 3), filters 64 * 2^stage),
residual_conv_block :60-109 (pre-activation basic block), ChannelSE _common_blocks.py:88-119 (reduction 16), BatchNorm
eps 2e-5 (get_bn_params).  Preprocess: raw RGB 0..255 into the model's own `bn_data` (scale=False), applied in the
preprocess kernel like ResNeXt-101's.

Per unit `stage{s}_unit{u}_`, with x the unit's input and a = relu(bn1(x)):
    shortcut = sc(a) (1x1, stride, no BN, no bias) in the first unit of a stage, x itself in the others
    c2 = conv2(relu(bn2(conv1(a))))     conv1 3x3 (stride 2 in the first unit of stages 2-4) with bn2 + relu folded in
    y = c2 * ChannelSE(c2) + shortcut   no ReLU after the add
The gate, the add and the NEXT unit's bn1 + relu (the final `bn1` / `relu1` after the last unit) are one launch pair
(csrc/se_residual.hip): it writes relu(bn(y)) and, when the next unit takes y as its identity shortcut, y.  Taps: C1 relu0,
C2..C4 = stage{2..4}_unit1_relu1 (the BN + ReLU'd input of the next stage), C5 relu1.  ChannelSE's two 1x1 convs are
auto-named `conv2d_N` in Keras; here `stage{s}_unit{u}_se/conv{1,2}/{kernel,bias}` (checkpoint.py maps them)."""
import numpy as np

from .. import ops
from ..keras_like import Conv2D
from .body import STAGE_TAPS, BatchNorm, ChannelSE, ResidualBody

BN_EPS = 2e-5
REPETITIONS = (3, 4, 6, 3)


class _Unit:
    def __init__(self, filters, stage, block, stride, first):
        base = f"stage{stage + 1}_unit{block + 1}_"
        self.first = first
        he = dict(kernel_initializer="he_normal")
        self.bn1 = BatchNorm(filters if not first or stage == 0 else filters // 2, BN_EPS, gamma_range=(0.5, 1.0),
                             name=base + "bn1")
        self.sc = Conv2D(filters, 1, strides=stride, use_bias=False, name=base + "sc", **he) if first else None
        self.conv1 = Conv2D(filters, 3, strides=stride, padding=((1, 1), (1, 1)), use_bias=False,
                            fold_bn=(base + "bn2", BN_EPS, True, (0.5, 1.5)), activation='relu', name=base + "conv1", **he)
        # the residual branch starts small (a quarter of he_normal) so that random weights keep the taps O(1) through the
        # identity additions of a stage (real checkpoints override)
        self.conv2 = Conv2D(filters, 3, padding=((1, 1), (1, 1)), use_bias=False, kernel_initializer="normal",
                            kernel_stddev=0.25 * float(np.sqrt(2.0 / (9 * filters))), name=base + "conv2")
        self.se = ChannelSE(filters, name=base + "se")

    def layers(self):
        return [l for l in (self.bn1, self.sc, self.conv1, self.conv2, self.se) if l is not None]

    def build(self, shape):
        s = self.conv2.build(self.conv1.build(shape))
        if self.sc is not None:
            self.sc.build(shape)
        return s

    def __call__(self, a, x, next_bn, want_y):
        """a = relu(bn1(x)) (written by the previous tail), x = the unit's raw input (None in a stage's first unit)
        -> (relu(next_bn(y)), y or None)."""
        shortcut = self.sc(a) if self.first else x
        c2 = self.conv2(self.conv1(a))
        se = self.se
        return ops.se_residual(c2, shortcut, se.w1, se.b1, se.w2, se.b2, next_bn.scale, next_bn.shift, want_y=want_y)


class SEResNet34(ResidualBody):
    INPUT_BN_EPS = BN_EPS

    def __init__(self, repetitions=REPETITIONS, **kwargs):
        super().__init__(name=kwargs.pop("name", "seresnet34_body"), **kwargs)
        self.stem = Conv2D(64, 7, strides=2, padding=((3, 3), (3, 3)), use_bias=False,
                           fold_bn=("bn0", BN_EPS, True), activation='relu', image_input=True,
                           kernel_initializer="he_normal", name="conv0")           # + bn0 + relu0, then pooling0
        self.stages = []
        for stage, rep in enumerate(repetitions):
            filters = 64 * 2 ** stage
            self.stages.append([_Unit(filters, stage, block, 1 if (stage == 0 or block > 0) else 2, block == 0)
                                for block in range(rep)])
        # after the last unit
        self.bn1 = BatchNorm(64 * 2 ** (len(repetitions) - 1), BN_EPS, gamma_range=(0.5, 1.0), name="bn1")
        self.trailing = [self.bn1]

    def call(self, x, wanted=("C3", "C4", "C5"), **kwargs):
        if ops.half_storage():
            raise NotImplementedError("the 'f16s' conv math (fp16 storage) is not built for the seresnet34 backbone: its "
                                      "SE block tail is fp32-only -- use 'f32', 'f32x3' or 'f16'")
        return super().call(x, wanted=wanted, **kwargs)

    def run_stages(self, x, taps, last):
        """Thread (a, y) through the units: a stage's tap is the BN + ReLU'd input of the next stage (C5: relu1)."""
        units = self.units()
        a, y = ops.bn_relu(x, units[0].bn1.scale, units[0].bn1.shift), None     # stage1_unit1_bn1 / relu1
        ends = {}
        k = 0
        for tap, st in zip(STAGE_TAPS, self.stages):
            k += len(st)
            ends[k - 1] = tap
        for k, u in enumerate(units):
            nxt = units[k + 1] if k + 1 < len(units) else None
            a, y = u(a, y, nxt.bn1 if nxt is not None else self.bn1, want_y=nxt is not None and not nxt.first)
            if k in ends:
                taps[ends[k]] = a
                if int(ends[k][1]) >= last:
                    break
