"""References for the backward of the depthwise 3x3 convolution (test infrastructure, not collected: no `test_` prefix).

1.  `dwconv` / `grads`: torch.nn.functional.conv2d(groups=C) in float64 on the CPU under autograd -- NHWC tensors, the Keras
    kernel [3,3,C,1], the padding resolve_padding gives applied explicitly (asymmetric; a trailing pad that is negative
    crops the rows a strided window never reaches) -> dw [3,3,C,1], db [C], dx [B,H,W,C].
2.  `magnitudes`: the uncancelled magnitude of every gradient element, which the bar is relative to -- S_w = sum |x| |dy|,
    S_b = sum |dy|, S_x = sum |w| |dy| -- from the same conv on absolute values.
3.  `check`: tests/resample_grad_ref.py's: |got - want| <= 1e-5 * S, exact zeros where S == 0.
4.  `direct_loops`: the formulas of include/masklab_hip.h as plain loops.
5.  `slice_pixels`: csrc/dwconv_grad.hip's slice rule restated.
6.  The case table; inputs are seeded by case name."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from conv_grad_ref import pads_of
from resample_grad_ref import BAR, check     # noqa: F401  (the bar and its check)

F32, F64 = np.float32, np.float64
SLICE_MIN, SLICE_MAX, SLICE_ROUND, PARTIAL_ROWS = 64, 1024, 16, 10      # csrc/dwconv_grad.hip's DW_SLICE_* / DW_ROUND / DW_ROWS


def slice_pixels(pixels):
    """The slice length csrc/dwconv_grad.hip plans for a problem of `pixels` output pixels: 1 / 64 of them, rounded up to a
    multiple of 16, clamped"""
    return min(max(-(-(-(-pixels // 64)) // SLICE_ROUND) * SLICE_ROUND, SLICE_MIN), SLICE_MAX)


def dwconv(x, w, b, stride, dilation, pads):
    """x [B,H,W,C], w [3,3,C,1], b [C] or None: torch tensors of one dtype -> [B,Ho,Wo,C]"""
    pt, pb, pl, pr = pads
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, w.permute(2, 3, 0, 1), b, stride=stride, dilation=dilation, groups=x.shape[3]).permute(0, 2, 3, 1)


def grads(x, w, dy, stride=1, padding="same", dilation=1):
    """float64 (dw [3,3,C,1], db [C], dx [B,H,W,C]) of sum(dwconv(x, w) * dy) by autograd"""
    leaf = lambda a: torch.from_numpy(np.asarray(a, F64)).requires_grad_(True)
    xt, wt = leaf(x), leaf(w)
    bt = torch.zeros(w.shape[2], dtype=torch.float64, requires_grad=True)
    _, _, pads = pads_of(x.shape[1], x.shape[2], 3, 3, stride, dilation, padding)
    (dwconv(xt, wt, bt, stride, dilation, pads) * torch.from_numpy(np.asarray(dy, F64))).sum().backward()
    return wt.grad.numpy(), bt.grad.numpy(), xt.grad.numpy()


def magnitudes(x, w, dy, stride=1, padding="same", dilation=1):
    """float64 (S_w, S_b, S_x): the gradients of the same conv on |x|, |w|, |dy|"""
    return grads(np.abs(x), np.abs(w), np.abs(dy), stride, padding, dilation)


def direct_loops(x, w, dy, stride, dilation, pt, pl):
    """dw, db, dx by the formulas of include/masklab_hip.h, plain loops in float64 (tiny cases only)"""
    x, w, dy = (np.asarray(a, F64) for a in (x, w, dy))
    B, H, W, _ = x.shape
    _, Ho, Wo, _ = dy.shape
    dw, dx = np.zeros_like(w), np.zeros_like(x)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for i in range(3):
                    for j in range(3):
                        iy, ix = oy * stride + i * dilation - pt, ox * stride + j * dilation - pl
                        if 0 <= iy < H and 0 <= ix < W:
                            dw[i, j, :, 0] += x[b, iy, ix] * dy[b, oy, ox]
                            dx[b, iy, ix] += w[i, j, :, 0] * dy[b, oy, ox]
    return dw, dy.sum(axis=(0, 1, 2)), dx


# ------------------------------------------------------------------ the cases
# name -> x shape [B,H,W,Cbuf] and the options that differ from (stride 1, 'same', dilation 1, the whole buffers, a bias)
CASES = {
    "same_d1": dict(x=(2, 7, 9, 32)),
    "dil6": dict(x=(2, 9, 11, 64), dilation=6),
    "dil12_on_5x7": dict(x=(2, 5, 7, 32), dilation=12),           # only the centre tap ever lands inside the image
    "valid": dict(x=(2, 7, 9, 32), padding="valid"),
    "stride2": dict(x=(2, 15, 18, 32), stride=2),                  # 18 -> 9 columns: the pad is on the right only
    "stride2_dil2": dict(x=(2, 15, 18, 32), stride=2, dilation=2),  # 3 columns of pad: 1 left, 2 right
    "smallest_c": dict(x=(2, 5, 6, 4)),
    "one_pixel": dict(x=(2, 1, 1, 32)),
    "in_slice": dict(x=(2, 7, 9, 96), in_coff=32, C=32, dy_c=160, dy_coff=64),
    "no_bias": dict(x=(2, 7, 9, 32), want_bias=False),
    "slices": dict(x=(2, 9, 13, 32)),                              # 234 pixels = 3 x 64 + 42; pixel 64 is (row 4, column 12)
    "multi_d1": dict(x=(2, 8, 8, 64), dilation=1, x_seed="multi"),
    "multi_d2": dict(x=(2, 8, 8, 64), dilation=2, x_seed="multi"),
    "multi_d6": dict(x=(2, 8, 8, 64), dilation=6, x_seed="multi"),
}
MULTI_NAMES = ["multi_d1", "multi_d2", "multi_d6"]


def geometry(name):
    """-> dict(x_shape, C, stride, padding, dilation, in_coff, dy_c, dy_coff, want_bias, Ho, Wo, pad_t, pad_l)"""
    c = CASES[name]
    g = dict(x_shape=c["x"], stride=c.get("stride", 1), padding=c.get("padding", "same"), dilation=c.get("dilation", 1),
             in_coff=c.get("in_coff", 0), dy_coff=c.get("dy_coff", 0), want_bias=c.get("want_bias", True))
    g["C"] = c.get("C", c["x"][3])
    g["dy_c"] = c.get("dy_c", g["C"])
    g["Ho"], g["Wo"], pads = pads_of(c["x"][1], c["x"][2], 3, 3, g["stride"], g["dilation"], g["padding"])
    g["pad_t"], g["pad_l"] = pads[0], pads[2]
    return g


def _rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def inputs(name):
    """N(0,1) inputs seeded by the case's name -> (g, x [B,H,W,C] float32, w [3,3,C,1] float32, dy [B,Ho,Wo,C] float32): the
    slices themselves; `in_buffer` lays them out in the case's wider buffers"""
    g = geometry(name)
    B, H, W, _ = g["x_shape"]
    x = _rng(CASES[name].get("x_seed", name) + "/x").normal(0, 1, (B, H, W, g["C"])).astype(F32)
    r = _rng(name)
    w = r.normal(0, 1, (3, 3, g["C"], 1)).astype(F32)
    dy = r.normal(0, 1, (B, g["Ho"], g["Wo"], g["C"])).astype(F32)
    return g, x, w, dy


def in_buffer(a, channels, coff, fill=np.nan):
    """a [B,H,W,C] as channels coff : coff + C of a [B,H,W,channels] buffer; `fill` (never to be read) in the others"""
    if channels == a.shape[3] and coff == 0:
        return a
    buf = np.full(a.shape[:3] + (channels,), fill, F32)
    buf[..., coff:coff + a.shape[3]] = a
    return buf
