"""GPU tests of the stride-2 data gradient ops.conv2d_dgrad_s2 (csrc/conv_grad.hip, ml_conv2d_dgrad_s2_f32) and of
Conv2D.backward(strided_dx=True), against torch.nn.functional.conv2d autograd in float64 on the CPU (tests/conv_grad_ref.py).
The bar is the project's gradient bar: |got - want| <= 1e-5 * S with S = sum |dy| |w| over the element's live taps, exact
zeros where S == 0 (R.check).  An element's fp32 chain has at most 25 x cout terms: off by at most L * 2^-24 * S, about
sqrt(L) * 2^-24 * S on random data -- for the longest chain here (9 taps x 64) 1.4e-6 * S at worst.

Every case runs without add, with add out of place, with `out is add`, on a 0xFF-filled `out` between 0xFF-filled sentinels,
and twice for equal bits; pixels no tap reaches must be +0.0, or add bit for bit.  -m gpu."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import conv_dgrad_s2_cases as S
import conv_grad_ref as R
import dirty_memory as DM

GUARD = 256                                          # floats of sentinel on each side of `out` (16-byte multiples)


def _dc(w, bias=None):
    from masklab_hip import ops, packing
    return ops.DeviceConv(packing.pack_dense(w, bias), torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (g, w, dy, dx float64, S_x float64): computed once per case, shared and left unchanged"""
    g, w, dy = S.inputs(name)
    x0 = np.zeros(g["x_shape"])
    dx = R.grads(x0, w, dy, 2, g["padding"], g["dilation"])[2]
    S_x = R.magnitudes(x0, w, dy, 2, g["padding"], g["dilation"])[2]
    return g, w, dy, dx, S_x


def _bits_of(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", list(S.CASES))
def test_conv2d_dgrad_s2(name):
    from masklab_hip import ops
    g, w, dy, dx, S_x = reference(name)
    dc, dyd = _dc(w), dev(dy)
    args = dict(dy=dyd, dc=dc, in_hw=g["x_shape"], padding=g["padding"], dilation=g["dilation"])
    n = int(np.prod(g["x_shape"]))

    # on stale memory, into the middle of a poisoned buffer: every element written, nothing beside them
    flat = DM.fill_bytes(torch.empty(n + 2 * GUARD, dtype=torch.float32, device="cuda"), DM.POISON)
    out = flat[GUARD:GUARD + n].view(g["x_shape"])
    with DM.poisoned():
        ret = ops.conv2d_dgrad_s2(**args, out=out)
    assert ret.data_ptr() == out.data_ptr()
    got = host(ret).copy()
    whole = host(flat)
    assert DM.holds(whole[:GUARD], DM.POISON) and DM.holds(whole[GUARD + n:], DM.POISON), f"{name}: wrote beside dx"
    assert got.dtype == np.float32 and got.shape == tuple(g["x_shape"])
    assert not DM.poison_elements(got).any(), f"{name}: elements left unwritten"
    err = np.abs(got - dx)
    print(f"{name}: largest |got - want| / S = {float((err[S_x > 0] / S_x[S_x > 0]).max()):.2e}, "
          f"{int((S_x == 0).sum())} of {n} elements unreached")
    R.check(got, dx, S_x, f"{name} dx")
    unreached = S_x == 0
    assert not _bits_of(got)[unreached].any(), f"{name}: an unreached pixel is not +0.0"

    # twice, into fresh memory of another content: the same bits
    with DM.zeroed():
        DM.assert_same_bits(DM.snapshot(ops.conv2d_dgrad_s2(**args)), got, f"{name}: second launch")

    # add out of place: one float32 addition on the same sums, so the very bits; unreached pixels are add itself
    add_h = np.random.default_rng(37).normal(0, 1, g["x_shape"]).astype(np.float32)
    add_h.reshape(-1)[::7] = -0.0                      # a sign an added +0.0 would lose
    add = dev(add_h)
    with DM.poisoned():
        with_add = DM.snapshot(ops.conv2d_dgrad_s2(**args, add=add))
    want_add = add_h + got
    want_add[got == 0] = add_h[got == 0]
    DM.assert_same_bits(with_add, want_add, f"{name}: add out of place")
    assert np.array_equal(_bits_of(with_add)[unreached], _bits_of(add_h)[unreached]), f"{name}: unreached pixels are not add's bits"
    R.check(with_add, add_h.astype(np.float64) + dx, S_x + np.abs(add_h), f"{name} add + dx")
    np.testing.assert_array_equal(host(add), add_h)

    # in place
    ret = ops.conv2d_dgrad_s2(**args, add=add, out=add)
    assert ret.data_ptr() == add.data_ptr()
    DM.assert_same_bits(DM.snapshot(ret), with_add, f"{name}: out is add")

    # the inputs are left unchanged
    np.testing.assert_array_equal(host(dyd), dy)
    np.testing.assert_array_equal(host(dc.keras_kernel), w)


def test_the_kernel_reads_the_bound_master_as_it_stands():
    """Unbound, the op reads an uploaded copy of the Keras kernel; bound (DeviceConv.bind_master), the master itself: a
    stepped weight is seen by the next launch without a re-pack."""
    from masklab_hip import ops
    g, w, dy, dx, S_x = reference("same_even")
    dyd = dev(dy)
    args = dict(dy=dyd, in_hw=g["x_shape"], padding=g["padding"])
    free = DM.snapshot(ops.conv2d_dgrad_s2(dc=_dc(w), **args))
    dc = _dc(w)
    master = dev(w)
    dc.bind_master(master)
    assert dc.keras_kernel is master
    DM.assert_same_bits(DM.snapshot(ops.conv2d_dgrad_s2(dc=dc, **args)), free, "bound against unbound")
    master.mul_(2.0)                                   # exact in float32: every product and sum doubles
    DM.assert_same_bits(DM.snapshot(ops.conv2d_dgrad_s2(dc=dc, **args)), free * np.float32(2), "a stepped master, no re-pack")


def test_conv2d_layer_backward_strided_dx_is_the_op():
    from masklab_hip import keras_like as K, ops
    g, w, dy, dx, S_x = reference("odd_tails")
    bias = np.random.default_rng(41).normal(0, 1, g["cout"]).astype(np.float32)
    layer = K.Conv2D(g["cout"], (3, 3), strides=(2, 2), padding="same", activation="relu", name="unit/s2")
    layer.build(g["x_shape"])
    layer.load_weights({"unit/s2/kernel": w, "unit/s2/bias": bias}, torch.device("cuda:0"))
    x = np.random.default_rng(43).normal(0, 1, g["x_shape"]).astype(np.float32)
    xd, dyd = dev(x), dev(dy)
    got, grads = layer.backward(xd, dyd, strided_dx=True)
    assert list(grads) == ["kernel", "bias"]
    want = DM.snapshot(ops.conv2d_dgrad_s2(dyd, layer.dev, g["x_shape"], "same", 1))
    DM.assert_same_bits(DM.snapshot(got), want, "Conv2D.backward(strided_dx=True)")
    R.check(want, dx, S_x, "Conv2D.backward dx")
    DM.assert_same_bits(DM.snapshot(grads["kernel"]), DM.snapshot(ops.conv2d_wgrad(xd, dyd, layer.dev, 2, "same", 1)[0]),
                        "Conv2D.backward(strided_dx=True): the weight gradient")
    add_h = np.random.default_rng(44).normal(0, 1, g["x_shape"]).astype(np.float32)
    add = dev(add_h)
    ret, _ = layer.backward(xd, dyd, add=add, strided_dx=True)
    DM.assert_same_bits(DM.snapshot(ret), DM.snapshot(ops.conv2d_dgrad_s2(dyd, layer.dev, g["x_shape"], add=dev(add_h))),
                        "Conv2D.backward(strided_dx=True, add=)")
    assert layer.backward(xd, dyd, need_dx=False, strided_dx=True)[0] is None
    # the default keeps today's refusal, and a stride-1 layer is untouched by the flag
    with pytest.raises(NotImplementedError, match="stride 2"):
        layer.backward(xd, dyd)
    with pytest.raises(ValueError, match="not a dy_view"):
        layer.backward(xd, None, dy_view=(dyd, 0, g["cout"], dyd[0].numel()), strided_dx=True)
    plain = K.Conv2D(g["cout"], (3, 3), padding="same", name="unit/s1")
    plain.build(g["x_shape"])
    plain.load_weights({"unit/s1/kernel": w, "unit/s1/bias": bias}, torch.device("cuda:0"))
    dy1 = dev(np.random.default_rng(45).normal(0, 1, g["x_shape"][:3] + (g["cout"],)).astype(np.float32))
    DM.assert_same_bits(DM.snapshot(plain.backward(xd, dy1, strided_dx=True)[0]), DM.snapshot(plain.backward(xd, dy1)[0]),
                        "a stride-1 layer under strided_dx=True")
