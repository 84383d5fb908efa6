"""References for BatchNormalization's training forward and backward (test infrastructure, not collected: no `test_` prefix).

1.  `restatement`: the rule of include/masklab_hip.h ("BatchNormalization, training") in float64 torch tensor ops, residual
    and ReLU included.  `autograd` differentiates it.
2.  `closed_form`: the backward formulas of the header in NumPy float64.
3.  `moving_update`: the moving-statistics rule in float32 NumPy, exactly as written: three operations, each rounded.
4.  `scale_forward` / `scale_backward`: the uncancelled magnitude S of every output, which the bar is relative to; `check`
    holds |got - want| <= BAR * S.
5.  The cases of the GPU test and their inputs."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
EPS = 1e-3
MOMENTUM = 0.99
# y is one fused multiply-add on float32 coefficients rounded once from fp64; a gradient term is a handful of float32
# operations on fp64-summed means: about 1e-6 of S.  The project's bar.
BAR = 1e-5
# Where |y| < GUARD * (|x*scale| + |shift| + |residual|) in float64 a float32 rounding of y may flip the ReLU's mask: dy is
# set to exactly 0 there.  At most GUARD_CAP of a case's elements may be zeroed so.
GUARD = 1e-4
GUARD_CAP = 0.005

# (B, H, W, C).  A-F are the issue's; G and H sit one pixel below and one above the only boundary the slice plan of
# csrc/batchnorm.hip adds (slices are 64 pixels at least: 64 pixels are one slice, 65 are two, the second of one pixel).
CASES = {
    "A": (1, 2, 3, 4),           # 6 pixels: one lane
    "B": (2, 5, 7, 64),          # 70 pixels
    "C": (3, 17, 19, 12),        # 969 pixels: C no multiple of a wave's channel span
    "D": (2, 33, 31, 32),        # 2046 pixels: several slices, ragged last
    "E": (1, 40, 41, 68),        # 1640 pixels, C = 68: a partial channel tile
    "F": (2, 16, 16, 32),        # 512 pixels: channel means at up to 30 standard deviations
    "G": (1, 8, 8, 8),           # 64 pixels: the last size that is one slice
    "H": (1, 5, 13, 8),          # 65 pixels: two slices, the second holds one pixel
}
# name -> (relu, residual, scale, center)
COMBOS = {"plain": (False, False, True, True), "relu": (True, False, True, True), "residual": (False, True, True, True),
          "residual_relu": (True, True, True, True), "no_scale": (True, False, False, True),
          "no_center": (False, True, True, False)}


def batch_stats(x):
    """float64 (mean_b, var_b, var_u) per channel"""
    xf = np.asarray(x, F64).reshape(-1, x.shape[-1])
    n = xf.shape[0]
    mean = xf.mean(axis=0)
    var = ((xf - mean) ** 2).mean(axis=0)
    return mean, var, var * n / (n - 1)


def coefficients(x, gamma, beta, eps=EPS):
    """float64 (mean_b, r, scale, shift); a missing gamma counts as ones, a missing beta as zeros"""
    mean, var, _ = batch_stats(x)
    r = 1 / np.sqrt(var + eps)
    scale = (np.ones_like(r) if gamma is None else np.asarray(gamma, F64)) * r
    shift = (np.zeros_like(r) if beta is None else np.asarray(beta, F64)) - mean * scale
    return mean, r, scale, shift


def forward(x, gamma, beta, residual=None, relu=False, eps=EPS):
    """float64 y in NumPy (the forward is continuous: no guard needed)"""
    _, _, scale, shift = coefficients(x, gamma, beta, eps)
    y = np.asarray(x, F64) * scale + shift
    if residual is not None:
        y = y + np.asarray(residual, F64)
    return np.maximum(y, 0) if relu else y


def scale_forward(x, gamma, beta, residual=None, eps=EPS):
    """S of y: |x*scale| + |shift| + |residual|"""
    _, _, scale, shift = coefficients(x, gamma, beta, eps)
    S = np.abs(np.asarray(x, F64) * scale) + np.abs(shift)
    return S + np.abs(np.asarray(residual, F64)) if residual is not None else S


def inputs(name, combo="plain", seed=0):
    """The issue's recipe.  -> dict(x, gamma, beta, residual, dy, zeroed): gamma / beta / residual are None where the
    combination has none (they are drawn all the same: the draws do not depend on the combination); zeroed: the fraction
    of dy the mask guard set to 0 (asserted <= GUARD_CAP)."""
    relu, has_res, has_scale, has_center = COMBOS[combo]
    shape = CASES[name]
    C = shape[-1]
    rng = np.random.default_rng(100 * list(CASES).index(name) + seed)
    off = rng.normal(0, 1, C) * (8 if name == "F" else 1)
    sd = rng.uniform(0.5, 2, C)
    x = (off + sd * rng.normal(0, 1, shape)).astype(F32)
    gamma = rng.uniform(0.5, 1.5, C).astype(F32)
    beta = rng.normal(0, 0.1, C).astype(F32)
    residual = rng.normal(0, 1, shape).astype(F32)
    dy = rng.normal(0, 1, shape).astype(F32)
    gamma, beta, residual = (gamma if has_scale else None), (beta if has_center else None), (residual if has_res else None)
    zeroed = 0.0
    if relu:
        y = forward(x, gamma, beta, residual)
        close = np.abs(y) < GUARD * scale_forward(x, gamma, beta, residual)
        dy = np.where(close, F32(0), dy)
        zeroed = float(close.mean())
        assert zeroed <= GUARD_CAP, (name, combo, seed, zeroed)
    return dict(x=x, gamma=gamma, beta=beta, residual=residual, dy=dy, zeroed=zeroed)


def moving_inputs(name, seed=0):
    """moving_mean ~ N(0, 0.1), moving_variance ~ U(0.5, 1.5), from a generator of their own"""
    C = CASES[name][-1]
    rng = np.random.default_rng(7919 + 100 * list(CASES).index(name) + seed)
    return rng.normal(0, 0.1, C).astype(F32), rng.uniform(0.5, 1.5, C).astype(F32)


def restatement(x, gamma, beta, residual=None, relu=False, eps=EPS):
    """The rule on float64 torch tensors [B,H,W,C]; gamma / beta: [C] or None.  -> (y, mean_b, var_b)"""
    mean = x.mean(dim=(0, 1, 2))
    var = ((x - mean) ** 2).mean(dim=(0, 1, 2))
    scale = 1 / torch.sqrt(var + eps)
    if gamma is not None:
        scale = gamma * scale
    shift = -mean * scale
    if beta is not None:
        shift = beta + shift
    y = x * scale + shift
    if residual is not None:
        y = y + residual
    return (torch.relu(y) if relu else y), mean, var


def autograd(x, dy, gamma, beta, residual=None, relu=False, eps=EPS):
    """-> float64 (dx, d_residual, dgamma, dbeta) of sum(restatement * dy); None for an input that is None.  torch's ReLU has
    gradient 0 at 0, as tf.nn.relu's."""
    leaf = lambda a: None if a is None else torch.from_numpy(np.asarray(a, F64)).requires_grad_(True)
    xl, gl, bl, rl = leaf(x), leaf(gamma), leaf(beta), leaf(residual)
    (restatement(xl, gl, bl, rl, relu, eps)[0] * torch.from_numpy(np.asarray(dy, F64))).sum().backward()
    return tuple(None if t is None else t.grad.numpy() for t in (xl, rl, gl, bl))


def _backward_terms(x, dy, gamma, beta, residual, relu, eps):
    mean, r, scale, _ = coefficients(x, gamma, beta, eps)
    g = np.asarray(dy, F64)
    if relu:
        g = g * (forward(x, gamma, beta, residual, eps=eps) > 0)
    return np.asarray(x, F64), g, mean, r, scale


def closed_form(x, dy, gamma, beta, residual=None, relu=False, eps=EPS):
    """-> float64 (dx, d_residual, dgamma, dbeta): the header's formulas"""
    xf, g, mean, r, scale = _backward_terms(x, dy, gamma, beta, residual, relu, eps)
    n = xf.size // xf.shape[-1]
    xhat = (xf - mean) * r
    dbeta = g.reshape(-1, xf.shape[-1]).sum(axis=0)
    dgamma = (g * xhat).reshape(-1, xf.shape[-1]).sum(axis=0)
    dx = scale * (g - dbeta / n - xhat * dgamma / n)
    return dx, g, dgamma, dbeta


def scale_backward(x, dy, gamma, beta, residual=None, relu=False, eps=EPS):
    """S of (dx, d_residual, dgamma, dbeta): every term of the closed form with its absolute value, (|x| + |mean_b|) * r in
    place of |xhat| (a large channel offset is priced in)."""
    xf, g, mean, r, scale = _backward_terms(x, dy, gamma, beta, residual, relu, eps)
    n = xf.size // xf.shape[-1]
    g = np.abs(g)
    xa = (np.abs(xf) + np.abs(mean)) * r
    sbeta = g.reshape(-1, xf.shape[-1]).sum(axis=0)
    sgamma = (g * xa).reshape(-1, xf.shape[-1]).sum(axis=0)
    sdx = np.abs(scale) * (g + sbeta / n + xa * sgamma / n)
    return sdx, g, sgamma, sbeta


def moving_update(moving, stat, momentum=MOMENTUM):
    """moving - (moving - f32(stat)) * np.float32(1.0 - momentum): float32 arrays, one rounding per operation"""
    moving = np.asarray(moving, F32)
    diff = moving - np.asarray(stat).astype(F32)
    step = diff * F32(1.0 - momentum)
    out = moving - step
    assert diff.dtype == step.dtype == out.dtype == F32
    return out


def check(got, want, S, what, names=("dx", "d_residual", "dgamma", "dbeta"), bar=BAR):
    """|got - want| <= bar * S per output, skipping outputs that are None on both sides; prints the largest ratio so that the
    margin is on record.  -> that ratio"""
    worst = 0.0
    for name, g, w, s in zip(names, got, want, S):
        if g is None and w is None:
            continue
        assert g is not None and w is not None, (what, name)
        g, w = np.asarray(g, F64), np.asarray(w, F64)
        assert g.shape == w.shape and np.isfinite(g).all(), (what, name, g.shape, w.shape)
        ratio = np.abs(g - w) / np.maximum(s, np.finfo(F64).tiny)
        ratio = np.where((s == 0) & (g == w), 0.0, ratio)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= bar, f"{what}: {name} off by {ratio.max():.3g} * S at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    print(f"{what}: max |got - want| / S = {worst:.3g} (bar {bar:g})")
    return worst
