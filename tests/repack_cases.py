"""Cases, weights and host expectations of the re-pack tests (test infrastructure, not collected: no `test_` prefix).

A case is the smallest kernel at which an arm of csrc/repack.hip can go wrong.  The expectation of every form is the host
function that defines it: packing.pack_dense / pack_winograd / pack_dense_transposed / pack_transpose2x2 / pack_out1x1_table
and the lazy properties of an ops.DeviceConv that lives on the CPU (wgt_x3, wgt_h)."""
import numpy as np
import torch

from masklab_hip import ops, packing

# name -> (kh, kw, cin, cout, bias)
CONV_CASES = {
    "tiny": (3, 3, 8, 4, True),       # n_pad 32; 24 pad channels; Winograd padded to four blocks; transposed cp = 4
    "ragged": (3, 3, 40, 36, True),   # span_pad 64 with a partial chunk; n_pad 64; the transposed side ragged too
    "priors": (3, 3, 64, 27, True),   # cout % 4 != 0: transposed cp = 28 with a zero channel
    "wide": (3, 3, 32, 130, True),    # two 128-wide tiles; no Winograd form; Winograd on the transposed side (132 -> 160)
    "skip": (1, 1, 64, 48, False),    # 1x1; no bias
    "k5": (5, 5, 4, 4, True),         # 25 taps: three runs of the nine-tap stage
}
SLICES = (5, 32, 32)                  # a 1x1 kernel of 5 * 32 -> 32 channels cut into five cin slices
DECONV = (128, 32)                    # Conv2DTranspose kernel [2,2,cout = 128,cin = 32] + bias
TABLES = ((128, 3), (128, 1))         # fused mask tail: C_mid -> ncls, cp = 4 and 1


def exact_weights(rng, shape):
    """Integers times 2^-20 with |w| < 8, signs mixed, some exact zeros and -0.0: every fp64 partial sum of G g G^T is exact."""
    w = (rng.integers(-(1 << 23) + 1, 1 << 23, size=shape).astype(np.float64) * 2.0 ** -20).astype(np.float32)
    flat = w.reshape(-1)
    pick = rng.permutation(flat.size)
    flat[pick[:max(1, flat.size // 16)]] = 0.0
    flat[pick[max(1, flat.size // 16):max(2, flat.size // 8)]] = -0.0
    return w


def wide_range_weights(rng, shape):
    """Magnitudes 2^-30 ... 2^10, full 24-bit significands, signs mixed: the fp64 sums of G g G^T are inexact for many elements."""
    w = rng.uniform(1.0, 2.0, size=shape) * 2.0 ** rng.integers(-30, 10, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    return w.astype(np.float32)


def small_weights(rng, shape):
    """|w| in [1e-8, 1e-4]: hi(w) and 2^11 (w - hi(w)) land among the subnormal halves."""
    w = np.exp(rng.uniform(np.log(1e-8), np.log(1e-4), size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    return w.astype(np.float32)


def wino_ok(p):
    return (p.KH, p.KW) == (3, 3) and p.n_pad <= 128 and not p.shuffle2x2


def side_forms(packed, prefix=""):
    """Every form of one packing as the host makes it: {prefix + name: array}."""
    dc = ops.DeviceConv(packed, "cpu")
    out = {prefix + "wgt": np.ascontiguousarray(packed.wgt), prefix + "x3": dc.wgt_x3.numpy(), prefix + "h": dc.wgt_h.numpy()}
    if packed.bias is not None:
        out[prefix + "bias"] = packed.bias
    if wino_ok(packed):
        out[prefix + "wino"] = packing.pack_winograd(packed)
    return out


def host_forms(kernel, bias=None):
    """A dense conv's forms, forward and transposed, from the Keras kernel."""
    out = side_forms(packing.pack_dense(kernel, bias))
    out.update(side_forms(packing.pack_dense_transposed(kernel), "tr."))
    return out


def materialise(dc, dgrad=True):
    """Touches every lazy form `dc` can have (and of its dgrad), so that a re-pack has them all to write."""
    for d in (dc, dc.dgrad) if dgrad else (dc,):
        d.wgt_x3, d.wgt_h
        if wino_ok(d.p):
            d.wgt_wino
    return dc


def device_tensors(dc):
    """{name: tensor} of every form `dc` has materialised, named as host_forms names them."""
    out = {}
    for prefix, d in (("", dc), ("tr.", dc._dgrad)):
        if d is None:
            continue
        for name, t in (("wgt", d.wgt), ("x3", d._wgt_x3), ("h", d._wgt_h), ("wino", d._wgt_wino), ("bias", d.bias)):
            if t is not None:
                out[prefix + name] = t
    return out


def to_host(tensors):
    return {k: v.detach().cpu().numpy() for k, v in tensors.items()}


def conv_case(name, rng, weights=exact_weights):
    kh, kw, cin, cout, has_bias = CONV_CASES[name]
    return weights(rng, (kh, kw, cin, cout)), (weights(rng, (cout,)) if has_bias else None)


def bound_conv(kernel0, bias0, device, dgrad=True):
    """A DeviceConv packed on the host from (kernel0, bias0), every form materialised, bound to device masters that hold the
    same weights.  -> (dc, master kernel, master bias or None)"""
    dc = materialise(ops.DeviceConv(packing.pack_dense(kernel0, bias0), device), dgrad)
    mk = torch.from_numpy(kernel0.copy()).to(device)                     # copies: on the CPU from_numpy would share memory
    mb = None if bias0 is None else torch.from_numpy(bias0.copy()).to(device)
    dc.bind_master(mk, mb)
    return dc, mk, mb
