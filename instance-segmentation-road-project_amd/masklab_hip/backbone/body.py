"""What the residual backbones share: the body skeleton (7x7/2 stem, 3x3/2 max-pool, four stages of units, taps C1..C5),
the model-owned input BatchNorm `bn_data` of the vendored thirdparty/classification_models ResNets, and the two weight-only
layers whose arithmetic runs in the SE tail kernels.  The unit classes stay in their model's file."""
import numpy as np

from .. import ops
from ..keras_like import Layer, WeightSpec

STAGE_TAPS = ("C2", "C3", "C4", "C5")


def bn_data_specs():
    """The input BatchNorm, scale=False: beta / moving statistics over raw 0..255 RGB."""
    return {
        "bn_data/beta": WeightSpec((3,), "normal", stddev=0.1),
        "bn_data/moving_mean": WeightSpec((3,), "uniform", low=100.0, high=130.0),
        "bn_data/moving_variance": WeightSpec((3,), "uniform", low=3000.0, high=5000.0),
    }


def input_affine(weights, eps):
    """(mean, divisor, shift) realising bn_data (scale=False) inside the preprocess kernel."""
    mean = np.asarray(weights["bn_data/moving_mean"], np.float64)
    div = np.sqrt(np.asarray(weights["bn_data/moving_variance"], np.float64) + eps)
    return mean.astype(np.float32), div.astype(np.float32), np.asarray(weights["bn_data/beta"], np.float32)


class BatchNorm(Layer):
    """An inference BatchNormalization that is not folded into a conv: its (scale, shift) are applied by the SE tail
    kernel.  `gamma` ~ U(gamma_range) in the synthetic init."""

    def __init__(self, channels, eps, gamma_range=(0.5, 1.5), **kwargs):
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

    def __init__(self, channels, reduction=16, **kwargs):
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


class ResidualBody(Layer):
    """A subclass constructs `self.stem` (a Conv2D(..., image_input=True) with the model's names) and `self.stages` (four
    lists of unit objects with layers(), build(shape) and __call__(x)), and may set `self.trailing` (layers created after
    the units) and INPUT_BN_EPS (the epsilon of its `bn_data`).  A model whose taps are not the stage outputs overrides
    stage_shapes() and run_stages()."""
    INPUT_BN_EPS = None
    trailing = ()

    def units(self):
        return [u for st in self.stages for u in st]

    def build(self, input_shape):
        s = self.stem.build(input_shape)
        taps = {"C1": s}
        H, W = s[1], s[2]
        s = (s[0], None if H is None else (H + 2 - 3) // 2 + 1, None if W is None else (W + 2 - 3) // 2 + 1, s[3])
        taps.update(self.stage_shapes(s))
        self.built = True
        return taps

    def stage_shapes(self, s):
        """Build every unit from the pooled shape `s`; -> the shapes of C2..C5."""
        taps = {}
        for tap, stage in zip(STAGE_TAPS, self.stages):
            for u in stage:
                s = u.build(s)
            taps[tap] = s
        return taps

    def children(self):
        """Creation order (checkpoint.py pairs Keras auto-names by it): the stem, the units, the trailing layers."""
        return [self.stem] + [l for u in self.units() for l in u.layers()] + list(self.trailing)

    def weight_specs(self):
        out = bn_data_specs() if self.INPUT_BN_EPS is not None else {}
        out.update(super().weight_specs())
        return out

    def call(self, x, wanted=("C3", "C4", "C5"), **kwargs):
        import torch
        half = ops.half_storage()            # fp16-storage mode: the body's tensors AND its taps are IEEE half
        taps = {}
        if "C1" not in wanted and self.stem.dev is not None and ops.has_fused_stem():
            x = ops.stem_pool(x, self.stem.dev)     # stem + pool in one pass (csrc/stem.hip): same bits as the pair below
        else:
            x = self.stem(x, out_dtype=torch.float16 if half else None)
            taps["C1"] = x
            x = ops.maxpool3x3s2(x, pad=1)
        last = max(int(t[1]) for t in wanted)
        if last >= 2:
            self.run_stages(x, taps, last)
        return taps

    def run_stages(self, x, taps, last):
        """Fill `taps` with C2..C`last` from the pooled stem output `x`; nothing beyond tap `last` is launched."""
        for tap, stage in zip(STAGE_TAPS, self.stages):
            if int(tap[1]) > last:
                break
            for u in stage:
                x = u(x)
            taps[tap] = x
