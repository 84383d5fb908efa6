"""References for the backward of the mask head's fused tail (test infrastructure, not collected: no `test_` prefix).

The tail is Conv2DTranspose(C_mid, 2x2, stride 2) + ReLU followed by Conv2D(ncls, 1x1) (+ sigmoid, which is the loss's):
    x [R,h,w,cin], wd [2,2,C_mid,cin], bd [C_mid], wo [1,1,C_mid,ncls], bo [ncls]
    T[r, 2i+a, 2j+b, o] = relu(sum_c x[r,i,j,c] wd[a,b,o,c] + bd[o]),   z = T . wo + bo    ([R,2h,2w,ncls], the pre-sigmoid output)

1.  `tail_forward`: torch.nn.functional.conv_transpose2d, ReLU, a matmul -- any dtype, under autograd.
2.  `tail_forward_gemm`: the same as four 1x1 GEMMs (one per output position q = 2a + b) on the pixels as rows, i.e. the GEMM
    layout T [M, 4, C_mid] of the device (M = R h w), then the pixel shuffle `gemm_to_map`.
3.  `tail_loops`: plain loops in float64 (tiny cases).
4.  The op-level reference: T is an INPUT there (any sign: the mask is T > 0, the 1x1 kernel's gradient uses T as it is), so
    `op_reference` is closed-form float64 with the uncancelled magnitudes S the bar is relative to (`check`: |got - want| <=
    1e-5 S, exact zeros where S == 0 -- tests/test_gpu_conv_grad.py's bar and definition):
        dT  = [T > 0] sum_k dy wo          S = [T > 0] sum_k |dy| |wo|
        dWo = sum T dy                     S = sum |T| |dy|
        dbo = sum dy                       S = sum |dy|
    and, for the transposed conv run as the 1x1 conv [1,1,cin,4 C_mid] on dT, with the magnitude carried through the chain
    (S_dT in the place of |dT|: the terms that were added to make each dT do not cancel for free):
        dWd = sum x dT                     S = sum |x| S_dT
        dbd = sum dT                       S = sum S_dT
        dx  = sum_n dT wd                  S = sum_n S_dT |wd|
5.  `slice_pixels`: csrc/deconv_out_grad.hip's slice rule, restated.
6.  The case table."""
import numpy as np
import torch
import torch.nn.functional as F

from resample_grad_ref import BAR, check     # noqa: F401  (the bar and its check)

F32, F64 = np.float32, np.float64
SLICE_MIN, SLICE_ROUND, SLICE_DIV = 128, 32, 512      # TG_SLICE_MIN / TG_ROUND / TG_SLICE_DIV


def slice_pixels(M):
    """Pixels per slice of a problem of M input pixels: ceil(M / 512) rounded up to a multiple of 32, at least 128"""
    return max(-(-(-(-M // SLICE_DIV)) // SLICE_ROUND) * SLICE_ROUND, SLICE_MIN)


def slices(M):
    return -(-M // slice_pixels(M))


def partial_bytes(M, c_mid, ncls):
    """Bytes of a problem's partials: per slice [ncls][C_mid] floats + [ncls] doubles (rounded up to 4 floats), the sum rounded
    up to 256"""
    n = slices(M) * (ncls * c_mid + (2 * ncls + 3) // 4 * 4) * 4
    return (n + 255) // 256 * 256


# ------------------------------------------------------------------ layouts
def gemm_to_map(Tg, R, h, w):
    """[R h w, 4, C] (q = 2a + b) -> [R, 2h, 2w, C]; numpy or torch"""
    C = Tg.shape[-1]
    t = Tg.reshape(R, h, w, 2, 2, C)
    t = t.permute(0, 1, 3, 2, 4, 5) if isinstance(t, torch.Tensor) else t.transpose(0, 1, 3, 2, 4, 5)
    return t.reshape(R, 2 * h, 2 * w, C)


def map_to_gemm(Tm):
    """[R, 2h, 2w, C] -> [R h w, 4, C]: the inverse of gemm_to_map"""
    R, H2, W2, C = Tm.shape
    t = Tm.reshape(R, H2 // 2, 2, W2 // 2, 2, C)
    t = t.permute(0, 1, 3, 2, 4, 5) if isinstance(t, torch.Tensor) else t.transpose(0, 1, 3, 2, 4, 5)
    return t.reshape(R * (H2 // 2) * (W2 // 2), 4, C)


def kernel_as_1x1(wd):
    """[2,2,C,cin] -> [cin, 4C], column q C + o: restated here (packing.transpose2x2_as_1x1 is what is tested against it)"""
    C, cin = wd.shape[2], wd.shape[3]
    out = np.zeros((cin, 4 * C), wd.dtype)
    for a in range(2):
        for b in range(2):
            out[:, (2 * a + b) * C:(2 * a + b + 1) * C] = wd[a, b].T
    return out


def kernel_from_1x1(k):
    """[cin, 4C] -> [2,2,C,cin]"""
    cin, C = k.shape[0], k.shape[1] // 4
    out = np.zeros((2, 2, C, cin), k.dtype)
    for a in range(2):
        for b in range(2):
            out[a, b] = k[:, (2 * a + b) * C:(2 * a + b + 1) * C].T
    return out


# ------------------------------------------------------------------ the tail, three times
def tail_forward(x, wd, bd, wo, bo):
    """torch tensors of one dtype -> (z [R,2h,2w,ncls], the transposed conv's pre-ReLU output [R,2h,2w,C])"""
    pre = F.conv_transpose2d(x.permute(0, 3, 1, 2), wd.permute(3, 2, 0, 1), bd, stride=2).permute(0, 2, 3, 1)
    return torch.relu(pre) @ wo[0, 0] + bo, pre


def tail_forward_gemm(x, wd, bd, wo, bo):
    """The same through the GEMM layout -> (z, pre-ReLU [M,4,C])"""
    R, h, w, cin = x.shape
    rows = x.reshape(R * h * w, cin)
    pre = torch.stack([rows @ wd[q // 2, q % 2].T + bd for q in range(4)], dim=1)
    return gemm_to_map(torch.relu(pre) @ wo[0, 0] + bo, R, h, w), pre


def tail_loops(x, wd, bd, wo, bo):
    x, wd, bd, wo, bo = (np.asarray(a, F64) for a in (x, wd, bd, wo, bo))
    R, h, w, _ = x.shape
    z = np.zeros((R, 2 * h, 2 * w, wo.shape[3]))
    for r in range(R):
        for i in range(h):
            for j in range(w):
                for a in range(2):
                    for b in range(2):
                        t = np.maximum(wd[a, b] @ x[r, i, j] + bd, 0.0)
                        z[r, 2 * i + a, 2 * j + b] = t @ wo[0, 0] + bo
    return z


def tail_autograd(x, wd, bd, wo, bo, dz, dtype=F64, forward=tail_forward):
    """-> ({x, wd, bd, wo, bo: gradient of sum(z dz)}, z, pre-ReLU values) as NumPy in `dtype`"""
    leaf = lambda a: torch.from_numpy(np.asarray(a, dtype)).requires_grad_(True)
    ts = {k: leaf(v) for k, v in dict(x=x, wd=wd, bd=bd, wo=wo, bo=bo).items()}
    z, pre = forward(ts["x"], ts["wd"], ts["bd"], ts["wo"], ts["bo"])
    (z * torch.from_numpy(np.asarray(dz, dtype))).sum().backward()
    return {k: v.grad.numpy() for k, v in ts.items()}, z.detach().numpy(), pre.detach().numpy()


# ------------------------------------------------------------------ the op-level reference
def level_dy(dy, off, n_l):
    """The RoIs [off, off + n_l) of every image of dy [B,total,2h,2w,ncls] -> [B n_l h w, 4, ncls] (the GEMM layout)"""
    B, _, H2, W2, ncls = dy.shape
    return map_to_gemm(np.ascontiguousarray(dy[:, off:off + n_l]).reshape(B * n_l, H2, W2, ncls))


def op_reference(T, dyg, wo, x=None, wd=None):
    """T [M,4,C], dyg [M,4,ncls] (level_dy), wo [1,1,C,ncls]; x [R,h,w,cin] / wd [2,2,C,cin] for the transposed conv's part.
    -> dict name -> (want, S), float64"""
    T, dyg, w = np.asarray(T, F64), np.asarray(dyg, F64), np.asarray(wo, F64)[0, 0]
    mask = T > 0
    dT, S_dT = mask * (dyg @ w.T), mask * (np.abs(dyg) @ np.abs(w).T)
    out = {"dT": (dT, S_dT),
           "dWo": (np.einsum("mqc,mqk->ck", T, dyg)[None, None], np.einsum("mqc,mqk->ck", np.abs(T), np.abs(dyg))[None, None]),
           "dbo": (dyg.sum(axis=(0, 1)), np.abs(dyg).sum(axis=(0, 1)))}
    if x is not None:
        M, _, C = T.shape
        rows = np.asarray(x, F64).reshape(M, -1)
        k = kernel_as_1x1(np.asarray(wd, F64))
        out["dWd"] = (kernel_from_1x1(rows.T @ dT.reshape(M, 4 * C)), kernel_from_1x1(np.abs(rows).T @ S_dT.reshape(M, 4 * C)))
        out["dbd"] = (dT.sum(axis=(0, 1)), S_dT.sum(axis=(0, 1)))
        out["dx"] = ((dT.reshape(M, 4 * C) @ k.T).reshape(x.shape), (S_dT.reshape(M, 4 * C) @ np.abs(k).T).reshape(x.shape))
    return out


# ------------------------------------------------------------------ the cases (B = 2 images)
B = 2
# name -> C_mid, ncls, cin, levels [(RoIs per image, h, w)], the loss's sparsity or a dense dy
CASES = {
    "m36_c128_n1": dict(C=128, ncls=1, cin=32, levels=[(1, 3, 6)], sparse=False),           # less than one forward tile
    "m128_c256_n3": dict(C=256, ncls=3, cin=64, levels=[(1, 8, 8)], sparse=True),           # exactly one tile, one slice
    "m150_c128_n5": dict(C=128, ncls=5, cin=32, levels=[(3, 5, 5)], sparse=False),          # a ragged second tile / slice
    "slices_c256_n3": dict(C=256, ncls=3, cin=32, levels=[(3, 7, 7)], sparse=False),        # 294 pixels = 128 + 128 + 38
    "slices_c128_sparse": dict(C=128, ncls=3, cin=32, levels=[(3, 7, 7)], sparse=True),
    "n32_c128": dict(C=128, ncls=32, cin=32, levels=[(3, 5, 5)], sparse=False),
    "n32_c256": dict(C=256, ncls=32, cin=32, levels=[(1, 3, 6)], sparse=True),
    "two_levels": dict(C=256, ncls=3, cin=32, levels=[(3, 7, 7), (1, 7, 7)], sparse=True),
    "four_levels": dict(C=128, ncls=5, cin=32, levels=[(2, 5, 5), (1, 5, 5), (3, 5, 5), (1, 5, 5)], sparse=False),
}


def pixels(level):
    n_l, h, w = level
    return B * n_l * h * w


def inputs(name):
    """-> dict: dy [B,total,2h,2w,ncls]; per level T [M,4,C] (every element exactly 0 or |value| >= 0.05, either sign: no case
    depends on which side of the kink a rounding falls), x [R,h,w,cin], wd, bd, wo, bo -- float32"""
    c = CASES[name]
    r = np.random.default_rng(900 + list(CASES).index(name))
    C, ncls, cin = c["C"], c["ncls"], c["cin"]
    total = sum(n for n, _, _ in c["levels"])
    _, h, w = c["levels"][0]
    dy = r.normal(0, 1, (B, total, 2 * h, 2 * w, ncls)).astype(F32)
    if c["sparse"]:                   # one class channel of about half the RoIs, as mask_loss's gradient
        keep = np.zeros_like(dy)
        for b in range(B):
            for j in range(total):
                if r.random() < 0.5 or (b, j) == (0, 0):
                    k = int(r.integers(ncls))
                    keep[b, j, :, :, k] = 1
        dy *= keep
    levels = []
    for n_l, lh, lw in c["levels"]:
        M = B * n_l * lh * lw
        mag = r.uniform(0.05, 1.0, (M, 4, C))
        sign = np.where(r.random((M, 4, C)) < 0.3, -1.0, 1.0)
        T = (mag * sign * (r.random((M, 4, C)) >= 0.3)).astype(F32)
        levels.append(dict(T=T, x=r.normal(0, 1, (B * n_l, lh, lw, cin)).astype(F32),
                           wd=r.normal(0, 0.3, (2, 2, C, cin)).astype(F32), bd=r.normal(0, 0.3, C).astype(F32),
                           wo=r.normal(0, 0.3, (1, 1, C, ncls)).astype(F32), bo=r.normal(0, 0.3, ncls).astype(F32)))
    return dict(dy=dy, levels=levels)
