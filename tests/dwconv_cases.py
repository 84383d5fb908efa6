"""Depthwise 3x3 cases that the older tables of tests/test_gpu_ops.py::test_dwconv3x3 and of its half twin in
tests/test_gpu_f16_heads.py leave out: ReLU6 on data that spans both clamps, no bias with no activation, stride 2 together
with dilation 2, a dilation larger than the map, the smallest channel counts.  Own generators, seeded by the case's name: the
modules' shared streams stay what they were.  Importable without a GPU."""
import zlib

import numpy as np

from oracle import tfops as T

ACT = {None: lambda v: v, "relu": T.relu, "relu6": T.relu6}

# name: (stride, padding, dilation, C, (H, W), act, bias)       bias: "n01" | "spread" (evenly over [-1.5, 7.5]) | None
# C is the fp32 kernel's; the half kernel moves 8 channels per lane and runs the same case on 2 C channels.
CASES = {
    "relu6_clamps": (1, "same", 1, 64, (9, 11), "relu6", "spread"),
    "linear_no_bias": (1, "same", 1, 32, (7, 9), None, None),
    "stride2_dil2": (2, "same", 2, 32, (15, 18), "relu6", "spread"),
    "stride2_dil2_explicit": (2, ((2, 2), (2, 2)), 2, 32, (15, 18), None, "n01"),
    "dil12_on_5x7": (1, "same", 12, 32, (5, 7), None, "n01"),            # only the centre tap is inside the image
    "smallest_c": (1, "same", 1, 4, (5, 6), "relu", "n01"),              # one vector per pixel
    "smallest_c_stride2": (2, ((0, 1), (0, 1)), 1, 4, (6, 8), "relu6", "spread"),
}


def case(name, C, half=False):
    """-> x [2, H, W, C] (fp32 or half), k [3, 3, C, 1] fp32, b [C] fp32 or None, and the pre-activation in float64 on the
    operands as the kernel holds them (the weights and the bias stay fp32 in both kernels).  Asserts on that reference alone
    what the case is for: at least 5 % of a ReLU6 case above 6 and 5 % below 0; the centre tap alone under dilation 12."""
    stride, padding, dil, _, hw, act, bias = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.normal(size=(2, hw[0], hw[1], C)).astype(np.float16 if half else np.float32)
    k = (rng.normal(size=(3, 3, C, 1)) * 0.3).astype(np.float32)
    b = {None: None, "n01": rng.normal(size=C), "spread": rng.permutation(np.linspace(-1.5, 7.5, C))}[bias]
    pre = T.depthwise_conv2d(x.astype(np.float64), k.astype(np.float64), stride, padding, dil)
    if b is not None:
        b = b.astype(np.float32)
        pre = pre + b.astype(np.float64)
    if act == "relu6":
        assert (pre > 6).mean() >= 0.05 and (pre < 0).mean() >= 0.05, name
    if name == "dil12_on_5x7":                       # 'same' pads 12 each side: every other tap reads padding
        assert np.array_equal(pre, x.astype(np.float64) * k[1, 1, :, 0].astype(np.float64) + b.astype(np.float64))
    return x, k, b, pre
