"""References for GroupNormalization's backward (test infrastructure, not collected: no `test_` prefix).

1.  `restatement`: the reference layer (engine/normalization.py:116-160) in float64 torch tensor ops -- reshape
    [N,H,W,C] to [N,G,H,W,C/G], mean and variance over the last three axes, gamma / beta reshaped to [1,G,1,1,C/G] and
    broadcast -- with the optional ReLU in front of the layer and the optional ReLU behind it.  `autograd` differentiates it.
2.  `closed_form`: the formulas of include/masklab_hip.h ("GroupNormalization, backward") in NumPy float64.
3.  `scale`: the uncancelled magnitude S of every output, which the bar is relative to; `check` holds |got - want| <= BAR * S.
4.  The cases of the GPU test and their inputs."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
EPS = 1e-5
# A term is about a dozen float32 operations on fp64-summed means, each within an ulp or two: about 1e-6 of S.
BAR = 1e-5
# No float32 rounding of y moves it across 0 if |y| >= GUARD * (|xhat * gamma| + |beta|): y's float32 error is a few ulp of
# the larger addend.
GUARD = 1e-5

# (N, H, W, C, G): the smallest shapes at which each path of csrc/groupnorm_grad.hip can go wrong
CASES = {
    "A": (2, 3, 5, 6, 3),        # L = 30: scalar accesses (C % 4), chunk shorter than a wave, C/G = 2
    "B": (2, 5, 5, 32, 4),       # L = 200: one-pass, 16-byte accesses, chunk starts mid-row (200 mod 32 = 8), C/G = 8
    "C": (3, 4, 4, 24, 4),       # L = 96: C/G = 6, residues no power of two on the 16-byte path; N = 3 in the parameter fold
    "D": (2, 24, 20, 32, 2),     # L = 7680: sliced, several slices, ragged last slice, C/G = 16 (the towers' value)
    "E": (1, 33, 41, 16, 2),     # L = 10824: sliced, chunk 1 starts mid-row (10824 mod 16 = 8), L no multiple of 1024
    "F": (1, 35, 41, 6, 2),      # L = 4305: sliced, scalar accesses (L odd), just above the one-pass limit, C/G = 3
}


def inputs(name, seed=0):
    """x = max(N(0.3, 1), 0): about 38 % exact zeros, a ReLU'd conv output; gamma ~ U(0.5, 1.5); beta ~ N(0, 0.1); then dy ~ N(0, 1)"""
    N, H, W, C, G = CASES[name]
    r = np.random.default_rng(100 * list(CASES).index(name) + seed)
    x = np.maximum(r.normal(0.3, 1, (N, H, W, C)), 0).astype(F32)
    gamma = r.uniform(0.5, 1.5, C).astype(F32)
    beta = r.normal(0, 0.1, C).astype(F32)
    dy = r.normal(0, 1, (N, H, W, C)).astype(F32)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, groups=G)


def restatement(z, gamma, beta, groups, relu=False, input_relu=False, eps=EPS):
    """The reference's call() on float64 torch tensors; z: the layer's input, or with input_relu what the ReLU in front
    of the layer is applied to.  gamma / beta: [C] or None."""
    x = torch.relu(z) if input_relu else z
    N, H, W, C = x.shape
    grouped = x.reshape(N, groups, H, W, C // groups)
    mean = grouped.mean(dim=(2, 3, 4), keepdim=True)
    var = ((grouped - mean) ** 2).mean(dim=(2, 3, 4), keepdim=True)
    out = (grouped - mean) / torch.sqrt(var + eps)
    if gamma is not None:
        out = out * gamma.reshape(1, groups, 1, 1, C // groups)
    if beta is not None:
        out = out + beta.reshape(1, groups, 1, 1, C // groups)
    out = out.reshape(N, H, W, C)
    return torch.relu(out) if relu else out


def autograd(x, dy, gamma, beta, groups, relu=False, input_relu=False, eps=EPS):
    """-> float64 (dx, dgamma, dbeta) of sum(restatement * dy); None for a weight that is None.  torch's ReLU has gradient 0
    at 0, as tf.nn.relu's."""
    leaf = lambda a: None if a is None else torch.from_numpy(np.asarray(a, F64)).requires_grad_(True)
    z, g, b = leaf(x), leaf(gamma), leaf(beta)
    (restatement(z, g, b, groups, relu, input_relu, eps) * torch.from_numpy(np.asarray(dy, F64))).sum().backward()
    return tuple(None if t is None else t.grad.numpy() for t in (z, g, b))


def _chunks(x, dy, gamma, beta, groups, eps):
    """float64 per-chunk views [N, G, L], the index j [G, L] by the rule j = g*(C/G) + (c mod C/G), c = (g*L + i) mod C"""
    N, C = x.shape[0], x.shape[-1]
    cg = C // groups
    xf, df = np.asarray(x, F64).reshape(N, groups, -1), np.asarray(dy, F64).reshape(N, groups, -1)
    L = xf.shape[2]
    c = (np.arange(groups * L) % C).reshape(groups, L)
    j = np.arange(groups)[:, None] * cg + c % cg
    gam = np.ones(C) if gamma is None else np.asarray(gamma, F64)
    bet = np.zeros(C) if beta is None else np.asarray(beta, F64)
    mean = xf.mean(axis=2, keepdims=True)
    r = 1 / np.sqrt(xf.var(axis=2, keepdims=True) + eps)
    xhat = (xf - mean) * r
    return xf, df, xhat, r, j, gam[j][None], bet[j][None]


def _terms(x, dy, gamma, beta, groups, relu, eps):
    xf, df, xhat, r, j, gam, bet = _chunks(x, dy, gamma, beta, groups, eps)
    d = df * ((xhat * gam + bet) > 0) if relu else df
    return xf, d, xhat, r, j, gam


def closed_form(x, dy, gamma, beta, groups, relu=False, input_relu=False, eps=EPS):
    """-> float64 (dx, dgamma, dbeta), the last two for all C indices (a missing gamma counts as ones)"""
    xf, d, xhat, r, j, gam = _terms(x, dy, gamma, beta, groups, relu, eps)
    g = d * gam
    dx = r * (g - g.mean(axis=2, keepdims=True) - xhat * (g * xhat).mean(axis=2, keepdims=True))
    if input_relu:
        dx = dx * (xf > 0)
    C = x.shape[-1]
    jj = np.broadcast_to(j[None], d.shape).reshape(-1)
    dbeta = np.bincount(jj, weights=d.reshape(-1), minlength=C)
    dgamma = np.bincount(jj, weights=(d * xhat).reshape(-1), minlength=C)
    return dx.reshape(x.shape), dgamma, dbeta


def scale(x, dy, gamma, beta, groups, relu=False, input_relu=False, eps=EPS):
    """The uncancelled magnitude of (dx, dgamma, dbeta): every term of the closed form with its absolute value."""
    xf, d, xhat, r, j, gam = _terms(x, dy, gamma, beta, groups, relu, eps)
    g = np.abs(d * gam)
    sdx = r * (g + g.mean(axis=2, keepdims=True) + np.abs(xhat) * (g * np.abs(xhat)).mean(axis=2, keepdims=True))
    C = x.shape[-1]
    jj = np.broadcast_to(j[None], d.shape).reshape(-1)
    sbeta = np.bincount(jj, weights=np.abs(d).reshape(-1), minlength=C)
    sgamma = np.bincount(jj, weights=np.abs(d * xhat).reshape(-1), minlength=C)
    return sdx.reshape(x.shape), sgamma, sbeta


def mask_margin(x, gamma, beta, groups, eps=EPS):
    """min over the elements of |y| / (|xhat * gamma| + |beta|) in float64: at GUARD or above, the float32 y of the kernels
    and the float64 y of the references have the same sign everywhere, so both mask the same elements."""
    xf, _, xhat, _, _, gam, bet = _chunks(x, x, gamma, beta, groups, eps)
    a = xhat * gam
    return float((np.abs(a + bet) / (np.abs(a) + np.abs(bet))).min())


def check(got, want, S, what, bar=BAR):
    """|got - want| <= bar * S per output of (dx, dgamma, dbeta), skipping outputs that are None on both sides; prints the
    largest ratio so that the margin is on record.  -> that ratio"""
    worst = 0.0
    for name, g, w, s in zip(("dx", "dgamma", "dbeta"), got, want, S):
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
