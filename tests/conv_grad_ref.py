"""References for the backward of the dense convolutions (test infrastructure, not collected: no `test_` prefix).

1.  `conv` / `grads`: torch.nn.functional.conv2d in float64 on the CPU under autograd -- NHWC tensors, the Keras kernel
    [kh,kw,cin,cout], the padding resolve_padding gives applied explicitly (a trailing pad that is negative crops the rows a
    strided window never reaches) -> dW, db, dx.
2.  `magnitudes`: the uncancelled magnitude of every gradient element, which the bar is relative to -- S_w = sum |x| |dy|,
    S_b = sum |dy|, S_x = sum |w| |dy| -- from the same conv on absolute values.
3.  `check`: tests/resample_grad_ref.py's: |got - want| <= 1e-5 * S, exact zeros where S == 0.
4.  The case table of the weight gradient, the cases of the data gradient, and the float64 / float32 restatement of a head
    tower (conv, ReLU, the chunk-wise GroupNormalization of tests/groupnorm_grad_ref.py)."""
import numpy as np
import torch
import torch.nn.functional as F

import groupnorm_grad_ref as GR
from resample_grad_ref import BAR, check     # noqa: F401  (the bar and its check)

F32, F64 = np.float32, np.float64
SLICE_MIN, SLICE_MAX = 512, 1024      # csrc/conv_grad.hip's WG_SLICE_MIN / WG_SLICE_MAX


def slice_pixels(pixels):
    """The slice length csrc/conv_grad.hip plans for a problem of `pixels` output pixels whose partials fit its share of the
    workspace: 1 / 128 of them, rounded up to a multiple of 32, clamped; test_conv_grad_cpu.py asserts it from the plan"""
    return min(max(-(-(-(-pixels // 128)) // 32) * 32, SLICE_MIN), SLICE_MAX)


def pads_of(H, W, kh, kw, stride, dilation, padding):
    """-> (Ho, Wo, (top, bottom, left, right)): bottom / right are what makes the padded input end where the last window ends
    (negative: rows no window reaches)"""
    from masklab_hip.packing import resolve_padding
    Ho, Wo, pt, pl = resolve_padding(H, W, kh, kw, stride, dilation, padding)
    pb = (Ho - 1) * stride + (kh - 1) * dilation + 1 - H - pt
    pr = (Wo - 1) * stride + (kw - 1) * dilation + 1 - W - pl
    return Ho, Wo, (pt, pb, pl, pr)


def conv(x, w, b, stride, dilation, pads):
    """x [B,H,W,cin], w [kh,kw,cin,cout], b [cout] or None: torch tensors of one dtype -> [B,Ho,Wo,cout]"""
    pt, pb, pl, pr = pads
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, w.permute(3, 2, 0, 1), b, stride=stride, dilation=dilation).permute(0, 2, 3, 1)


def grads(x, w, dy, stride=1, padding="same", dilation=1):
    """float64 (dW [kh,kw,cin,cout], db [cout], dx [B,H,W,cin]) of sum(conv(x, w) * dy) by autograd"""
    leaf = lambda a: torch.from_numpy(np.asarray(a, F64)).requires_grad_(True)
    xt, wt = leaf(x), leaf(w)
    bt = torch.zeros(w.shape[3], dtype=torch.float64, requires_grad=True)
    _, _, pads = pads_of(x.shape[1], x.shape[2], w.shape[0], w.shape[1], stride, dilation, padding)
    (conv(xt, wt, bt, stride, dilation, pads) * torch.from_numpy(np.asarray(dy, F64))).sum().backward()
    return wt.grad.numpy(), bt.grad.numpy(), xt.grad.numpy()


def magnitudes(x, w, dy, stride=1, padding="same", dilation=1):
    """float64 (S_w, S_b, S_x): the gradients of the same conv on |x|, |w|, |dy|"""
    return grads(np.abs(x), np.abs(w), np.abs(dy), stride, padding, dilation)


def direct_loops(x, w, dy, stride, dilation, pt, pl):
    """dW, db, dx by the formulas of include/masklab_hip.h, plain loops in float64 (tiny cases only)"""
    x, w, dy = (np.asarray(a, F64) for a in (x, w, dy))
    B, H, W, _ = x.shape
    kh, kw, _, _ = w.shape
    _, Ho, Wo, _ = dy.shape
    dW, dx = np.zeros_like(w), np.zeros_like(x)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for i in range(kh):
                    for j in range(kw):
                        iy, ix = oy * stride + i * dilation - pt, ox * stride + j * dilation - pl
                        if 0 <= iy < H and 0 <= ix < W:
                            dW[i, j] += np.outer(x[b, iy, ix], dy[b, oy, ox])
                            dx[b, iy, ix] += w[i, j] @ dy[b, oy, ox]
    return dW, dy.sum(axis=(0, 1, 2)), dx


# ------------------------------------------------------------------ the weight gradient's cases
# name -> x shape [B,H,W,Cbuf], cout, kernel, and the options that differ from (stride 1, 'same', dilation 1, the whole buffer)
WGRAD_CASES = {
    "tower": dict(x=(2, 8, 8, 32), cout=32, k=3),
    "cout75_view": dict(x=(2, 13, 11, 32), cout=75, k=3, view=True),     # 286 pixels; image 1 starts inside a 32-pixel chunk
    "cin_tail": dict(x=(1, 9, 10, 136), cout=12, k=1, padding="valid"),  # 136 = 4 x 32 + 8: a cin tile of 8
    "two_tiles": dict(x=(1, 6, 6, 160), cout=160, k=3),                  # two cout tiles; 45 units = 5 unit groups
    "stride2": dict(x=(2, 13, 11, 32), cout=32, k=3, stride=2, padding=((0, 1), (0, 1))),
    "k1s2": dict(x=(2, 13, 11, 64), cout=32, k=1, stride=2),
    "dil3": dict(x=(1, 12, 12, 32), cout=32, k=3, dilation=3),
    "dead_taps": dict(x=(1, 2, 2, 32), cout=32, k=3, dilation=3),        # every tap but the centre only meets padding
    "one_pixel": dict(x=(2, 1, 1, 32), cout=32, k=3),
    "k5": dict(x=(1, 9, 10, 32), cout=32, k=5),                          # 25 units = 3 unit groups
    "in_slice": dict(x=(2, 8, 8, 40), cout=32, k=3, in_coff=4, cin=32),
    "no_bias": dict(x=(2, 8, 8, 32), cout=32, k=3, want_bias=False),
    "slices": dict(x=(1, 47, 49, 32), cout=32, k=3),                     # 2303 pixels = 4 x 512 + 255
    "long_slices": dict(x=(1, 362, 362, 4), cout=8, k=3),                # 131 044 pixels = 127 x 1024 + 996: the longest slices
}
LEVELS = [(2, 16, 16, 32), (2, 8, 8, 32), (2, 4, 4, 32), (2, 2, 2, 32), (2, 1, 1, 32)]
for _i, _s in enumerate(LEVELS):
    WGRAD_CASES[f"levels{_i}"] = dict(x=_s, cout=32, k=3)
LEVEL_NAMES = [f"levels{i}" for i in range(len(LEVELS))]
# 9 216 pixels = 18 slices of 512: one pass of the finish kernel's sixteen-wide loop, then two remainders (the table's last
# row: the cases before it keep their seeds)
WGRAD_CASES["slices18"] = dict(x=(1, 96, 96, 4), cout=8, k=3)
VIEW_GAP, VIEW_OFF = 152, 30          # floats between the images of a dy view beyond their own, and before the first


def geometry(name):
    """-> dict(x_shape, cin, cout, k, stride, padding, dilation, in_coff, want_bias, view, Ho, Wo)"""
    c = WGRAD_CASES[name]
    g = dict(x_shape=c["x"], cout=c["cout"], k=c["k"], stride=c.get("stride", 1), padding=c.get("padding", "same"),
             dilation=c.get("dilation", 1), in_coff=c.get("in_coff", 0), want_bias=c.get("want_bias", True),
             view=c.get("view", False))
    g["cin"] = c.get("cin", c["x"][3])
    g["Ho"], g["Wo"], _ = pads_of(c["x"][1], c["x"][2], c["k"], c["k"], g["stride"], g["dilation"], g["padding"])
    return g


def view_layout(g):
    """(element offset, channel stride, batch stride, elements of the tensor) of a case's dy view"""
    cs = g["cout"]
    bs = g["Ho"] * g["Wo"] * cs + VIEW_GAP
    return VIEW_OFF, cs, bs, VIEW_OFF + g["x_shape"][0] * bs


def wgrad_inputs(name):
    """N(0,1) inputs -> (g, x [B,H,W,Cbuf] float32, w [k,k,cin,cout] float32, dy [B,Ho,Wo,cout] float32)"""
    g = geometry(name)
    r = np.random.default_rng(300 + list(WGRAD_CASES).index(name))
    x = r.normal(0, 1, g["x_shape"]).astype(F32)
    w = r.normal(0, 1, (g["k"], g["k"], g["cin"], g["cout"])).astype(F32)
    dy = r.normal(0, 1, (g["x_shape"][0], g["Ho"], g["Wo"], g["cout"])).astype(F32)
    return g, x, w, dy


def in_view(g, dy, fill=np.nan):
    """dy laid out as the case's view inside a flat float32 array; `fill` everywhere else (never read)"""
    off, cs, bs, n = view_layout(g)
    flat = np.full(n, fill, F32)
    for b in range(dy.shape[0]):
        flat[off + b * bs: off + b * bs + dy[b].size] = dy[b].reshape(-1)
    return flat


# ------------------------------------------------------------------ the data gradient's cases (stride 1)
DGRAD_CASES = {
    "tower": dict(x=(2, 8, 8, 32), cout=32, k=3),
    "cout75_view": dict(x=(2, 13, 11, 32), cout=75, k=3, view=True),
    "dil3": dict(x=(1, 12, 12, 32), cout=32, k=3, dilation=3),
    "k1": dict(x=(2, 9, 10, 64), cout=32, k=1),
    "valid": dict(x=(2, 9, 10, 32), cout=32, k=3, padding="valid"),
    "wino128": dict(x=(2, 8, 8, 128), cout=128, k=3),                    # the transposed problem is Winograd-eligible under "f32"
}


def dgrad_inputs(name):
    c = DGRAD_CASES[name]
    g = dict(x_shape=c["x"], cin=c["x"][3], cout=c["cout"], k=c["k"], stride=1, padding=c.get("padding", "same"),
             dilation=c.get("dilation", 1), view=c.get("view", False))
    g["Ho"], g["Wo"], _ = pads_of(c["x"][1], c["x"][2], c["k"], c["k"], 1, g["dilation"], g["padding"])
    r = np.random.default_rng(500 + list(DGRAD_CASES).index(name))
    w = r.normal(0, 1, (g["k"], g["k"], g["cin"], g["cout"])).astype(F32)
    dy = r.normal(0, 1, (c["x"][0], g["Ho"], g["Wo"], g["cout"])).astype(F32)
    return g, w, dy


# ------------------------------------------------------------------ a head tower, restated
def tower_forward(inputs, weights, prefix, depth, groups, num_levels):
    """The towers of BoxRegressionSubNet / ClassificationSubNet up to the output convs' PRE-activation, in the dtype of
    `inputs` (torch tensors; `weights`: {name: torch tensor}).  -> (pred [B, A, d], every conv's pre-activation)"""
    preds, pre = [], []
    for l in range(num_levels):
        x = inputs[l]
        for i in range(depth):
            w, b = weights[f"{prefix}/block{l}/conv{i}/kernel"], weights[f"{prefix}/block{l}/conv{i}/bias"]
            z = conv(x, w, b, 1, 1, (1, 1, 1, 1))
            pre.append(z)
            x = GR.restatement(torch.relu(z), weights[f"{prefix}/block{l}/gn{i}/gamma"], weights[f"{prefix}/block{l}/gn{i}/beta"],
                               groups)
        w, b = weights[f"{prefix}/block{l}/output/kernel"], weights[f"{prefix}/block{l}/output/bias"]
        z = conv(x, w, b, 1, 1, (1, 1, 1, 1))
        preds.append(z)
    return preds, pre


def tower_autograd(inputs, weights, d_pred, prefix, depth, groups, out_dim, dtype):
    """-> (d_inputs per level, {name: gradient}, the smallest |pre-activation| of the ReLU convs, pred), NumPy in `dtype`, of
    sum(pred * d_pred) with pred = the levels' outputs reshaped to [B, -1, out_dim] and concatenated along axis 1"""
    tdt = torch.float64 if dtype == F64 else torch.float32
    xs = [torch.from_numpy(np.asarray(a, dtype)).requires_grad_(True) for a in inputs]
    ws = {k: torch.from_numpy(np.asarray(v, dtype)).requires_grad_(True) for k, v in weights.items() if k.startswith(prefix + "/")}
    preds, pre = tower_forward(xs, ws, prefix, depth, groups, len(inputs))
    pred = torch.cat([p.reshape(p.shape[0], -1, out_dim) for p in preds], dim=1)
    assert pred.dtype == tdt
    (pred * torch.from_numpy(np.asarray(d_pred, dtype))).sum().backward()
    kink = min(float(z.detach().abs().min()) for z in pre)
    return [x.grad.numpy() for x in xs], {k: v.grad.numpy() for k, v in ws.items() if v.grad is not None}, kink, pred.detach().numpy()
