"""The cases of the stride-2 data gradient (test infrastructure, not collected: no `test_` prefix), shared by
tests/test_conv_dgrad_s2_cpu.py and tests/test_gpu_conv_dgrad_s2.py, and the NumPy restatement of its parity rule.

A case is the FORWARD problem: x shape [B,H,W,cin], cout, kernel, and what differs from ('same', dilation 1).  Each is the
smallest problem at which one arm of csrc/conv_grad.hip's stride-2 kernel can go wrong."""
import numpy as np

F32 = np.float32

CASES = {
    "same_even": dict(x=(2, 8, 8, 64), cout=64, k=3),                    # TF 'same' on an even map: pads (0, 1)
    # odd map, pads (1, 1); cin = 32 + 4: a second 32-column block with a tail; cout = 20: a K chunk of 20 of 32
    "odd_tails": dict(x=(2, 7, 9, 36), cout=20, k=3),
    "valid": dict(x=(1, 8, 8, 32), cout=32, k=3, padding="valid"),       # 3 x 3 outputs: the last row and column are never read
    "k1_even": dict(x=(1, 8, 8, 32), cout=48, k=1),                      # three classes without a tap
    "k1_odd": dict(x=(1, 7, 7, 32), cout=48, k=1),
    "p6_to_p7": dict(x=(2, 1, 2, 32), cout=32, k=3),                     # 1 x 2 -> 1 x 1: classes without a pixel
    "c5_to_p6": dict(x=(2, 2, 3, 32), cout=32, k=3),                     # 2 x 3 -> 1 x 2
    "dil2": dict(x=(1, 9, 9, 32), cout=32, k=3, dilation=2),             # per axis every tap lives in ONE parity
    "k5": dict(x=(1, 10, 10, 8), cout=12, k=5),
    # classes of 3 x 10 x 10 = 300 pixels: three 128-pixel tiles, the last of 44, tiles that cross images; cin 132 = two N tiles
    "class300": dict(x=(3, 20, 20, 132), cout=64, k=3),
    "cin96": dict(x=(1, 4, 6, 96), cout=8, k=3),                         # three 32-column blocks: the instantiation none above runs
}


def geometry(name):
    """-> dict(x_shape, cin, cout, k, padding, dilation, Ho, Wo, pad_t, pad_l)"""
    from masklab_hip.packing import resolve_padding
    c = CASES[name]
    g = dict(x_shape=c["x"], cin=c["x"][3], cout=c["cout"], k=c["k"], padding=c.get("padding", "same"),
             dilation=c.get("dilation", 1))
    g["Ho"], g["Wo"], g["pad_t"], g["pad_l"] = resolve_padding(c["x"][1], c["x"][2], c["k"], c["k"], 2, g["dilation"], g["padding"])
    return g


def inputs(name):
    """N(0,1) -> (g, w [k,k,cin,cout] float32, dy [B,Ho,Wo,cout] float32)"""
    g = geometry(name)
    r = np.random.default_rng(700 + list(CASES).index(name))
    w = r.normal(0, 1, (g["k"], g["k"], g["cin"], g["cout"])).astype(F32)
    dy = r.normal(0, 1, (g["x_shape"][0], g["Ho"], g["Wo"], g["cout"])).astype(F32)
    return g, w, dy


def parity_classes(g):
    """The parity rule restated: list over class c = 2 (iy & 1) + (ix & 1) of (pixels, [(ky, kx, off_y, off_x)]): tap (ky, kx)
    is live for the class iff py + pad_t - ky d and px + pad_l - kx d are even, and then oy = (iy >> 1) + off_y."""
    B, H, W, _ = g["x_shape"]
    k, d = g["k"], g["dilation"]
    out = []
    for py in (0, 1):
        for px in (0, 1):
            taps = []
            for ky in range(k):
                for kx in range(k):
                    ty, tx = py + g["pad_t"] - ky * d, px + g["pad_l"] - kx * d
                    if ty % 2 == 0 and tx % 2 == 0:
                        taps.append((ky, kx, ty // 2, tx // 2))
            out.append((B * len(range(py, H, 2)) * len(range(px, W, 2)), taps))
    return out


def live_pairs_of_classes(g, classes):
    """(tap, input pixel) pairs the classes' tap lists reach inside dy"""
    B, H, W, _ = g["x_shape"]
    n = 0
    for c, (_, taps) in enumerate(classes):
        py, px = c >> 1, c & 1
        for _, _, oy, ox in taps:
            ys = sum(0 <= (iy >> 1) + oy < g["Ho"] for iy in range(py, H, 2))
            xs = sum(0 <= (ix >> 1) + ox < g["Wo"] for ix in range(px, W, 2))
            n += B * ys * xs
    return n


def live_pairs_of_forward(g):
    """(tap, input pixel) pairs of the forward: windows positions that fall inside the map"""
    B, H, W, _ = g["x_shape"]
    k, d = g["k"], g["dilation"]
    n = 0
    for t in range(k):
        ys = sum(0 <= 2 * oy + t * d - g["pad_t"] < H for oy in range(g["Ho"]))
        for u in range(k):
            n += B * ys * sum(0 <= 2 * ox + u * d - g["pad_l"] < W for ox in range(g["Wo"]))
    return n
