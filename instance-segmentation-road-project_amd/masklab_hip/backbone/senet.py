"""SE-ResNeXt-50 and SE-ResNet-50 bodies -- the two SENet backbones of the reference's load_backbone
(engine/backbone/base.py:220-246, taps :133-146).  Architecture from the vendored thirdparty/classification_models:
senet.py SENet :198-324 with MODELS_PARAMS :331-355 (repetitions (3, 4, 6, 3), outputs 256 .. 2048, stride 2 in the first
unit of stages 2-4), SEResNetBottleneck :46-88, SEResNeXtBottleneck :91-134, ChannelSE _common_blocks.py:88-119
(reduction 16), GroupConv2D :13-76 (32 slices -> 32 Conv2D -> concat).  BatchNorm eps 9.999999747378752e-06 (float32
1e-5, get_bn_params).  Preprocess BackBonePreProcess(rgb=True, mean_shift=True, normalize=3): (x - mean) / 255 / std.

Per unit `stage{s}_unit{u}_`, with x the unit's input:
    y1  = relu(bn1(conv1(x)))       1x1, width out/2 (SE-ResNeXt) or out/4 with the stride on it (SE-ResNet)
    y2  = relu(bn2(conv2(y1)))      pad 1 + 3x3: 32 groups with the stride (SE-ResNeXt), dense at stride 1 (SE-ResNet)
    c3  = bn3(conv3(y2))            1x1 to the unit's output width, no activation
    residual = sc_bn(sc(x)) (1x1, stride) in the first unit of a stage, x in the others
    out = relu(c3 * ChannelSE(c3) + residual)   one launch triple (csrc/se_bottleneck.hip), written over c3
Every BatchNorm is folded into its conv.  Taps are the reference's Keras auto-named Activations: C1 the stem ReLU; C2..C4
the stage outputs for SE-ResNet-50, and for SE-ResNeXt-50 the conv1 ReLU of the NEXT stage's first unit (a reference
quirk, kept: it is a conv epilogue); C5 the last unit's output.  The reference leaves every backbone layer to Keras'
automatic names (`conv2d_N`, `batch_normalization_N`); here they are hierarchical (checkpoint.py pairs them by creation
order): conv0 / bn0, stage{s}_unit{u}_{conv1, bn1, conv2, bn2, conv3, bn3, sc, sc_bn, se/conv1, se/conv2}; SE-ResNeXt's
3x3 as the reference stores it, `..._conv2/group{g}/kernel` [3,3,c,c] x 32."""
import numpy as np

from .. import ops
from ..keras_like import Conv2D, GroupedConv2D
from .body import ChannelSE, ResidualBody

BN_EPS = 9.999999747378752e-06
REPETITIONS = (3, 4, 6, 3)
GROUPS = 32


class GroupConv2D(GroupedConv2D):
    """thirdparty GroupConv2D (pad 1 + 32 x [slice -> Conv2D 3x3 (stride), no bias] -> concat): its 32 kernels
    `group{g}/kernel` [3,3,c,c] are concatenated at load into GroupedConv2D's layout, kernel[.., g*c+i, m] = K_g[.., i, m]."""

    def build(self, input_shape):
        assert int(input_shape[-1]) == self.filters
        self.cin = self.filters
        c = self.filters // self.groups
        for g in range(self.groups):
            self.add_weight(f"group{g}/kernel", (3, 3, c, c), "normal", stddev=float(np.sqrt(2.0 / (9 * c))))
        self.built = True
        H, W = input_shape[1], input_shape[2]
        if H is None or W is None:
            return (input_shape[0], None, None, self.filters)
        return (input_shape[0], (H - 1) // self.strides[0] + 1, (W - 1) // self.strides[0] + 1, self.filters)

    def kernel(self, weights):
        return np.concatenate([self._get(weights, f"group{g}/kernel") for g in range(self.groups)], axis=2)


class _Unit:
    """One bottleneck unit of either model (grouped: SE-ResNeXt's, else SE-ResNet's)."""

    def __init__(self, filters, stage, block, stride, grouped):
        base = f"stage{stage + 1}_unit{block + 1}_"
        # synthetic-init gamma ranges: bn3 starts small so that random weights keep the taps O(1) through the identity
        # additions of a stage, as resnext.py does (real checkpoints override)
        rng = {1: (0.5, 1.5), 2: (0.5, 1.5), 3: (0.1, 0.3)}
        bn = lambda s: (f"{base}bn{s}", BN_EPS, True, rng[s])
        he = dict(kernel_initializer="he_normal")
        width = filters // 2 if grouped else filters // 4
        self.conv1 = Conv2D(width, 1, strides=1 if grouped else stride, use_bias=False, fold_bn=bn(1), activation='relu',
                            name=base + "conv1", **he)
        if grouped:
            self.conv2 = GroupConv2D(width, GROUPS, strides=stride, fold_bn=bn(2), activation='relu', name=base + "conv2")
        else:
            self.conv2 = Conv2D(width, 3, padding=((1, 1), (1, 1)), use_bias=False, fold_bn=bn(2), activation='relu',
                                name=base + "conv2", **he)
        self.conv3 = Conv2D(filters, 1, use_bias=False, fold_bn=bn(3), name=base + "conv3", **he)
        self.sc = None
        if block == 0:
            self.sc = Conv2D(filters, 1, strides=stride, use_bias=False, fold_bn=(base + "sc_bn", BN_EPS, True, (0.5, 1.0)),
                             name=base + "sc", **he)
        self.se = ChannelSE(filters, name=base + "se")

    def layers(self):
        """In the reference's creation order: conv1, conv2, conv3, [sc], ChannelSE."""
        return [l for l in (self.conv1, self.conv2, self.conv3, self.sc, self.se) if l is not None]

    def build(self, shape):
        s = self.conv3.build(self.conv2.build(self.conv1.build(shape)))
        if self.sc is not None:
            assert tuple(self.sc.build(shape)[1:]) == tuple(s[1:]) or None in s, (shape, s)
        return s

    def __call__(self, x):
        return self.tail(x, self.conv1(x))

    def tail(self, x, y1):
        """y1 = conv1(x) -> the unit's output; c3 is overwritten by it."""
        residual = self.sc(x) if self.sc is not None else x
        c3 = self.conv3(self.conv2(y1))
        se = self.se
        return ops.se_bottleneck(c3, residual, se.w1, se.b1, se.w2, se.b2, out=c3)


class _SENet50(ResidualBody):
    GROUPED = None

    def __init__(self, repetitions=REPETITIONS, **kwargs):
        super().__init__(**kwargs)
        self.stem = Conv2D(64, 7, strides=2, padding=((3, 3), (3, 3)), use_bias=False, fold_bn=("bn0", BN_EPS, True),
                           activation='relu', image_input=True, kernel_initializer="he_normal", name="conv0")
        self.stages = []
        for stage, rep in enumerate(repetitions):
            filters = 256 * 2 ** stage
            self.stages.append([_Unit(filters, stage, block, 2 if (block == 0 and stage > 0) else 1, self.GROUPED)
                                for block in range(rep)])


class SEResNet50(_SENet50):
    GROUPED = False

    def __init__(self, **kwargs):
        super().__init__(name=kwargs.pop("name", "seresnet50_body"), **kwargs)


class SEResNeXt50(_SENet50):
    """Its C2..C4 are the conv1 ReLU of the NEXT stage's first unit, not the stage outputs."""
    GROUPED = True

    def __init__(self, **kwargs):
        super().__init__(name=kwargs.pop("name", "seresnext50_body"), **kwargs)

    def stage_shapes(self, s):
        taps = {}
        for si, units in enumerate(self.stages):
            for bi, u in enumerate(units):
                if bi == 0 and si > 0:
                    taps[f"C{si + 1}"] = u.conv1.build(s)
                s = u.build(s)
        taps["C5"] = s
        return taps

    def run_stages(self, x, taps, last):
        for si, units in enumerate(self.stages):
            for bi, u in enumerate(units):
                y1 = u.conv1(x)
                if bi == 0 and si > 0:
                    taps[f"C{si + 1}"] = y1              # the next stage's conv1 ReLU is the previous stage's tap
                    if si + 1 >= last:
                        return
                x = u.tail(x, y1)
        taps["C5"] = x
