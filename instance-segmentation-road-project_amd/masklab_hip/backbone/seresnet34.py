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
from ..keras_like import Conv2D, Layer, WeightSpec

BN_EPS = 2e-5
REPETITIONS = (3, 4, 6, 3)
SE_REDUCTION = 16


class BatchNorm(Layer):
    """An inference BatchNormalization that is not folded into a conv: its (scale, shift) are applied by the SE tail
    kernel.  `gamma` ~ U(gamma_range) in the synthetic init."""

    def __init__(self, channels, eps=BN_EPS, gamma_range=(0.5, 1.5), **kwargs):
        super().__init__(**kwargs)
        self.channels, self.eps = int(channels), eps
        self.add_weight("gamma", (self.channels,), "uniform", low=gamma_range[0], high=gamma_range[1])
        self.add_weight("beta", (self.channels,), "normal", stddev=0.1)
        self.add_weight("moving_mean", (self.channels,), "normal", stddev=0.1)
        self.add_weight("moving_variance", (self.channels,), "uniform", low=0.5, high=1.5)
        self.built = True
        self.scale = self.shift = None

    def folded(self, weights):
        """(scale, shift) in fp64, rounded once: y * scale + shift == (y - mean) / sqrt(var + eps) * gamma + beta."""
        g = self._get(weights, "gamma").astype(np.float64)
        sc = g / np.sqrt(self._get(weights, "moving_variance").astype(np.float64) + self.eps)
        sh = self._get(weights, "beta").astype(np.float64) - self._get(weights, "moving_mean").astype(np.float64) * sc
        return sc.astype(np.float32), sh.astype(np.float32)

    def _load_own(self, weights, device):
        import torch
        sc, sh = self.folded(weights)
        self.scale = torch.from_numpy(sc).to(device)
        self.shift = torch.from_numpy(sh).to(device)


class ChannelSE(Layer):
    """_common_blocks.py ChannelSE: GlobalAveragePooling2D -> Conv2D(C/16, 1x1, bias) -> relu -> Conv2D(C, 1x1, bias)
    -> sigmoid -> Multiply.  Weights only: the arithmetic is in the SE tail kernel."""

    def __init__(self, channels, reduction=SE_REDUCTION, **kwargs):
        super().__init__(**kwargs)
        self.channels = int(channels)
        self.hidden = self.channels // reduction
        self.add_weight("conv1/kernel", (1, 1, self.channels, self.hidden), "he_normal")
        self.add_weight("conv1/bias", (self.hidden,), "normal", stddev=0.1)
        self.add_weight("conv2/kernel", (1, 1, self.hidden, self.channels), "he_normal")
        self.add_weight("conv2/bias", (self.channels,), "normal", stddev=0.1)
        self.built = True
        self.w1 = None

    def _load_own(self, weights, device):
        import torch
        C, Hd = self.channels, self.hidden
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
        self.w1 = up(self._get(weights, "conv1/kernel").reshape(C, Hd))
        self.b1 = up(self._get(weights, "conv1/bias"))
        self.w2 = up(self._get(weights, "conv2/kernel").reshape(Hd, C))
        self.b2 = up(self._get(weights, "conv2/bias"))


class _Unit:
    def __init__(self, filters, stage, block, stride, first):
        base = f"stage{stage + 1}_unit{block + 1}_"
        self.first = first
        he = dict(kernel_initializer="he_normal")
        self.bn1 = BatchNorm(filters if not first or stage == 0 else filters // 2, gamma_range=(0.5, 1.0),
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


class SEResNet34(Layer):
    def __init__(self, repetitions=REPETITIONS, **kwargs):
        super().__init__(name=kwargs.pop("name", "seresnet34_body"), **kwargs)
        self.conv0 = Conv2D(64, 7, strides=2, padding=((3, 3), (3, 3)), use_bias=False,
                            fold_bn=("bn0", BN_EPS, True), activation='relu', image_input=True,
                            kernel_initializer="he_normal", name="conv0")
        self.stages = []
        for stage, rep in enumerate(repetitions):
            filters = 64 * 2 ** stage
            self.stages.append([_Unit(filters, stage, block, 1 if (stage == 0 or block > 0) else 2, block == 0)
                                for block in range(rep)])
        self.bn1 = BatchNorm(64 * 2 ** (len(repetitions) - 1), gamma_range=(0.5, 1.0), name="bn1")   # after the last unit
        self._bn_data = {
            "bn_data/beta": WeightSpec((3,), "normal", stddev=0.1),
            "bn_data/moving_mean": WeightSpec((3,), "uniform", low=100.0, high=130.0),
            "bn_data/moving_variance": WeightSpec((3,), "uniform", low=3000.0, high=5000.0),
        }

    def units(self):
        return [u for st in self.stages for u in st]

    def build(self, input_shape):
        s = self.conv0.build(input_shape)
        taps = {"C1": s}
        H, W = s[1], s[2]
        s = (s[0], None if H is None else (H + 2 - 3) // 2 + 1, None if W is None else (W + 2 - 3) // 2 + 1, s[3])
        for tap, units in zip(("C2", "C3", "C4", "C5"), self.stages):
            for u in units:
                s = u.build(s)
            taps[tap] = s
        self.built = True
        return taps

    def children(self):
        return [self.conv0] + [l for u in self.units() for l in u.layers()] + [self.bn1]

    def weight_specs(self):
        out = dict(self._bn_data)
        for ch in self.children():
            out.update(ch.weight_specs())
        return out

    def input_affine(self, weights):
        """(mean, divisor, shift) realising bn_data (scale=False) inside the preprocess kernel."""
        mean = np.asarray(weights["bn_data/moving_mean"], np.float64)
        div = np.sqrt(np.asarray(weights["bn_data/moving_variance"], np.float64) + BN_EPS)
        return mean.astype(np.float32), div.astype(np.float32), np.asarray(weights["bn_data/beta"], np.float32)

    def call(self, x, wanted=("C3", "C4", "C5"), **kwargs):
        if ops.half_storage():
            raise NotImplementedError("the 'f16s' conv math (fp16 storage) is not built for the seresnet34 backbone: its "
                                      "SE block tail is fp32-only -- use 'f32', 'f32x3' or 'f16'")
        taps = {}
        if "C1" not in wanted and self.conv0.dev is not None and ops.has_fused_stem():
            x = ops.stem_pool(x, self.conv0.dev)            # stem + bn0 + relu0 + pooling0 in one pass
        else:
            x = self.conv0(x)
            taps["C1"] = x
            x = ops.maxpool3x3s2(x, pad=1)
        last = max(int(t[1]) for t in wanted)
        units = self.units()
        a, y = ops.bn_relu(x, units[0].bn1.scale, units[0].bn1.shift), None     # stage1_unit1_bn1 / relu1
        ends = {}
        k = 0
        for tap, st in zip(("C2", "C3", "C4", "C5"), self.stages):
            k += len(st)
            ends[k - 1] = tap
        for k, u in enumerate(units):
            nxt = units[k + 1] if k + 1 < len(units) else None
            a, y = u(a, y, nxt.bn1 if nxt is not None else self.bn1, want_y=nxt is not None and not nxt.first)
            if k in ends:
                taps[ends[k]] = a
                if int(ends[k][1]) >= last:
                    break
        return taps
