"""GPU tests of the exact view extents in csrc/conv_grad.hip (csrc/ranges.h: ml_view_elems): an output may begin at the first
byte after a strided view's last element, which lies inside the last pixel's channel stride.  Every range of a case lives in
ONE flat allocation, so the placement is the test's and not the caching allocator's.  The results are compared bit for bit with
the same call into separately allocated tensors: the kernels are unchanged, only the refusal was wrong."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import conv_grad_ref as R
from test_gpu_conv_grad import _dc


def _u32(t):
    return host(t).reshape(-1).view(np.uint32)


# [2,9,9,24] -> 162 x 8 floats: more than one block of the gather
@pytest.mark.parametrize("shape,coff,C", [((2, 3, 3, 12), 4, 4), ((2, 3, 3, 12), 8, 4), ((2, 9, 9, 24), 16, 8)])
def test_gather_channels_into_the_bytes_right_behind_src(shape, coff, C):
    """Accept: out begins at the first byte after src (the view reaches Cs - coff - C channels less far than its last pixel's
    stride; the over-counted extent reached `coff` channels past src).  Refuse: out begins 16 bytes before the view's real
    end, which for coff + C == Cs is 16 bytes before the end of src."""
    from masklab_hip import ops
    B, H, W, Cs = shape
    n_src, n_out = B * H * W * Cs, B * H * W * C
    r = np.random.default_rng(71)
    flat = torch.full((n_src + n_out,), float("nan"), dtype=torch.float32, device="cuda")
    src = flat[:n_src].view(shape)
    src.copy_(dev(r.normal(0, 1, shape).astype(np.float32)))
    want = src[..., coff:coff + C].contiguous()
    apart = ops.gather_channels(src, coff, torch.full((B, H, W, C), float("nan"), dtype=torch.float32, device="cuda"))
    behind = flat[n_src:].view(B, H, W, C)
    assert behind.data_ptr() == src.data_ptr() + 4 * n_src
    got = ops.gather_channels(src, coff, behind)
    np.testing.assert_array_equal(_u32(got), _u32(want))
    np.testing.assert_array_equal(_u32(got), _u32(apart))
    np.testing.assert_array_equal(_u32(src[..., coff:coff + C].contiguous()), _u32(want))       # src is as it was
    end = n_src - (Cs - coff - C)                                                                # the view's last element + 1
    inside = flat[end - 4:end - 4 + n_out].view(B, H, W, C)
    with pytest.raises(RuntimeError, match="out may not overlap dy"):
        ops.gather_channels(src, coff, inside)


def test_conv2d_wgrad_into_the_bytes_right_behind_a_dy_view():
    """cout75_view's problem with its dy at element offset 30, channel stride 80 > cout 75 and a batch stride with a gap;
    dkernel begins at the view's real last element + 1 (5 floats before the end of the last pixel's stride), dbias behind it"""
    from masklab_hip import ops
    g, x, w, dy = R.wgrad_inputs("cout75_view")
    B, Ho, Wo, cout = dy.shape
    off, cs = R.VIEW_OFF, 80
    bs = Ho * Wo * cs + R.VIEW_GAP
    end = off + (B - 1) * bs + (Ho * Wo - 1) * cs + cout
    assert off > 0 and cs > cout and end < off + (B - 1) * bs + Ho * Wo * cs
    flat = torch.full((end + w.size + cout,), float("nan"), dtype=torch.float32, device="cuda")
    for b in range(B):
        flat[off + b * bs:off + b * bs + Ho * Wo * cs].view(Ho * Wo, cs)[:, :cout].copy_(dev(dy[b].reshape(Ho * Wo, cout)))
    args = dict(x=dev(x), dy=None, dc=_dc(w), stride=g["stride"], padding=g["padding"], dilation=g["dilation"],
                in_coff=g["in_coff"], dy_view=(flat, off, cs, bs))
    apart = ops.conv2d_wgrad(**args)
    dk, db = flat[end:end + w.size].view(w.shape), flat[end + w.size:]
    assert dk.data_ptr() == flat.data_ptr() + 4 * end
    got = ops.conv2d_wgrad(**args, out=(dk, db))
    assert got[0].data_ptr() == dk.data_ptr() and got[1].data_ptr() == db.data_ptr()
    for a, b, what in zip(got, apart, ("dkernel", "dbias")):
        np.testing.assert_array_equal(_u32(a), _u32(b), err_msg=what)
    with pytest.raises(RuntimeError, match="dkernel may not overlap x or dy"):
        ops.conv2d_wgrad(**args, out=(flat[end - 1:end - 1 + w.size].view(w.shape), db))
