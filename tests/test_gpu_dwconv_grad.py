"""GPU tests of the depthwise 3x3 convolution's backward: ops.dwconv3x3_wgrad / _wgrad_multi, ops.dwconv3x3_dgrad / _dgrad_multi
(csrc/dwconv_grad.hip) and DepthwiseConv2D.backward, against torch autograd in float64 over the restatement of
tests/dwconv_grad_ref.py.  The bar is the project's gradient bar, |got - want| <= 1e-5 * S with S the uncancelled magnitude of
the element (sum |x| |dy|, sum |dy|, sum |w| |dy|), exact zeros where S == 0.  A slice's fp32 sum of L terms is off by at
most L * 2^-24 * S (L <= 1 024; the cases' slices hold 64 pixels), the slices add in fp64; the data gradient is nine fp32
terms.  Every op also holds: two launches give the same bits; the bits do not depend on what outputs, partials and
workspace held; the inputs are left unchanged; nothing outside the outputs is written and no channel beside the slices
read is read (NaN neighbours, sentinel guards).  -m gpu.

Largest |got - want| / S measured on the MI355X, per case (the bar is 1e-5):
    dw / db   same_d1 3.3e-08 / 1.3e-08   dil6 6.5e-08 / 2.5e-08   dil12_on_5x7 3.7e-08 / 2.7e-08   valid 6.1e-08 / 1.7e-08
              stride2 3.5e-08 / 1.5e-08   stride2_dil2 3.3e-08 / 1.7e-08   smallest_c 4.3e-08 / 1.6e-08
              one_pixel 6.5e-08 / 5.1e-08   in_slice 3.2e-08 / 2.7e-08   no_bias 4.2e-08 / -   slices 3.0e-08 / 1.3e-08
              multi_d1 4.1e-08 / 2.5e-08   multi_d2 3.9e-08 / 1.9e-08   multi_d6 9.9e-08 / 2.9e-08
    dx        same_d1 1.2e-07   dil6 1.2e-07   dil12_on_5x7 5.9e-08   valid 1.2e-07   stride2 1.1e-07   stride2_dil2 1.3e-07
              smallest_c 9.9e-08   one_pixel 5.7e-08   in_slice 1.2e-07   no_bias 1.5e-07   slices 1.6e-07
              multi_d1 1.7e-07   multi_d2 1.6e-07   multi_d6 1.2e-07"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import dirty_memory as DM
import dwconv_grad_ref as R
from sentinel_dest import SENT
from test_gpu_resample_grad import _bits, _everything


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (g, x, w, dy, dw, db, dx, S_w, S_b, S_x): computed once per case, shared and left unchanged"""
    g, x, w, dy = R.inputs(name)
    dw, db, dx = R.grads(x, w, dy, g["stride"], g["padding"], g["dilation"])
    S_w, S_b, S_x = R.magnitudes(x, w, dy, g["stride"], g["padding"], g["dilation"])
    return g, x, w, dy, dw, db, dx, S_w, S_b, S_x


def _buffers(name):
    """The case's x and dy in their (wider) buffers, NaN in every channel that must not be read -> (xb, dyb) host arrays"""
    g, x, _, dy = reference(name)[:4]
    return R.in_buffer(x, g["x_shape"][3], g["in_coff"]), R.in_buffer(dy, g["dy_c"], g["dy_coff"])


def _wgrad_problem(name):
    """-> (the arguments of ops.dwconv3x3_wgrad for the case, its (device tensor, host array) inputs)"""
    g = reference(name)[0]
    xb, dyb = _buffers(name)
    xd, dyd = dev(xb), dev(dyb)
    args = dict(x=xd, dy=dyd, stride=g["stride"], padding=g["padding"], dilation=g["dilation"], in_coff=g["in_coff"],
                dy_coff=g["dy_coff"], want_bias=g["want_bias"], C=g["C"])
    return args, [(xd, xb), (dyd, dyb)]


def _dgrad_problem(name):
    from masklab_hip import packing
    g, x, w = reference(name)[:3]
    _, dyb = _buffers(name)
    dyd, wd = dev(dyb), dev(packing.pack_depthwise(w))
    args = dict(dy=dyd, wgt=wd, in_hw=x.shape, stride=g["stride"], padding=g["padding"], dilation=g["dilation"],
                dy_coff=g["dy_coff"], C=g["C"])
    return args, [(dyd, dyb), (wd, packing.pack_depthwise(w))]


def _guarded(shape, head=8, tail=8):
    """A tensor of `shape` inside a sentinel-filled flat buffer -> (buffer, the tensor: a view)"""
    n = int(np.prod(shape))
    buf = torch.full((head + n + tail,), SENT, device="cuda", dtype=torch.float32)
    return buf, buf[head:head + n].view(*shape)


def _guards_hold(buf, n, head=8, what=""):
    flat = host(buf)
    assert (flat[:head] == SENT).all() and (flat[head + n:] == SENT).all(), f"{what}: written outside the output"


# ------------------------------------------------------------------ the weight and bias gradient
@pytest.mark.parametrize("name", list(R.CASES))
def test_dwconv3x3_wgrad(name):
    from masklab_hip import ops
    g, x, w, dy, dw, db, dx, S_w, S_b, S_x = reference(name)
    args, inputs = _wgrad_problem(name)
    got = _everything(lambda **kw: ops.dwconv3x3_wgrad(**args, **kw), inputs, name)
    assert isinstance(got, tuple) and got[0].dtype == np.float32 and got[0].shape == w.shape
    R.check(got[0], dw, S_w, f"{name} dw")
    if g["want_bias"]:
        R.check(got[1], db, S_b, f"{name} db")
    else:
        assert got[1] is None
    if name == "dil12_on_5x7":
        dead = S_w.reshape(9, -1).max(axis=1) == 0
        assert dead.sum() == 8 and not dead[4] and not got[0].reshape(9, -1)[dead].any()    # exact zeros, written
    # sentinel guards around the outputs: the same bits, nothing written beside them
    C = g["C"]
    kbuf, kout = _guarded((3, 3, C, 1))
    bbuf, bout = _guarded((C,))
    ret = ops.dwconv3x3_wgrad(**args, out=(kout, bout) if g["want_bias"] else kout)
    _bits([ret[0], ret[1]] if g["want_bias"] else [ret[0]], list(got) if g["want_bias"] else [got[0]], f"{name}: guarded outputs")
    _guards_hold(kbuf, 9 * C, what=f"{name} dkernel")
    _guards_hold(bbuf, C if g["want_bias"] else 0, what=f"{name} dbias")
    # add= in place is add + the gradient computed separately: one float32 addition, so the very bits
    r = np.random.default_rng(31)
    add_k, add_b = r.normal(0, 1, w.shape).astype(np.float32), r.normal(0, 1, C).astype(np.float32)
    bk, bb = dev(add_k), dev(add_b)
    pair = (bk, bb) if g["want_bias"] else bk
    ret = ops.dwconv3x3_wgrad(**args, add=pair, out=pair)
    assert ret[0].data_ptr() == bk.data_ptr() and (ret[1] is None or ret[1].data_ptr() == bb.data_ptr())
    np.testing.assert_array_equal(host(ret[0]), add_k + got[0], err_msg=f"{name}: add in place, kernel")
    if g["want_bias"]:
        np.testing.assert_array_equal(host(ret[1]), add_b + got[1], err_msg=f"{name}: add in place, bias")
    fresh = (dev(add_k), dev(add_b)) if g["want_bias"] else dev(add_k)
    _bits(ops.dwconv3x3_wgrad(**args, add=fresh), ret, f"{name}: add out of place")


def test_a_workspace_that_is_too_small_is_refused():
    from masklab_hip import ops
    args, _ = _wgrad_problem("slices")
    need = ops.dwconv3x3_wgrad_plan(R.geometry("slices")["x_shape"])[2]
    with pytest.raises(RuntimeError, match="workspace is too small"):
        ops.dwconv3x3_wgrad(**args, workspace_bytes=need - 256)


def test_wgrad_multi_is_its_single_launches():
    from masklab_hip import ops
    problems = [_wgrad_problem(name) for name in R.MULTI_NAMES]
    shared = problems[0][0]["x"]
    for args, _ in problems:                                  # the three dilations read ONE input
        args["x"] = shared
    singles = [DM.snapshot(ops.dwconv3x3_wgrad(**args)) for args, _ in problems]
    inputs = [problems[0][1][0]] + [ins[1] for _, ins in problems]
    got = _everything(lambda: ops.dwconv3x3_wgrad_multi([args for args, _ in problems]), inputs, "multi")
    DM.assert_same_bits(got, singles, "one multi launch against three single launches")
    for name, one in zip(R.MULTI_NAMES, got):
        ref = reference(name)
        R.check(one[0], ref[4], ref[7], f"{name} dw in a multi launch")
    # and beside problems of other shapes: the slices of a problem do not depend on the launch it rides in
    mixed = ["slices", "multi_d2", "smallest_c", "in_slice", "stride2_dil2", "one_pixel", "no_bias", "dil6"]
    others = [_wgrad_problem(name) for name in mixed]
    both = DM.snapshot(ops.dwconv3x3_wgrad_multi([args for args, _ in others]))
    for name, b, (args, _) in zip(mixed, both, others):
        _bits(ops.dwconv3x3_wgrad(**args), b, f"{name}: alone against a mixed launch")


# ------------------------------------------------------------------ the data gradient
@pytest.mark.parametrize("name", list(R.CASES))
def test_dwconv3x3_dgrad(name):
    from masklab_hip import ops
    g, x, w, dy, dw, db, dx, S_w, S_b, S_x = reference(name)
    args, inputs = _dgrad_problem(name)
    got = _everything(lambda **kw: ops.dwconv3x3_dgrad(**args, **kw), inputs, name)
    assert got.dtype == np.float32 and got.shape == x.shape
    R.check(got, dx, S_x, f"{name} dx")
    buf, out = _guarded(x.shape)
    _bits(ops.dwconv3x3_dgrad(**args, out=out), got, f"{name}: a guarded output")
    _guards_hold(buf, x.size, what=f"{name} dx")
    # add= in place is add + the gradient: one float32 addition, so the very bits
    add_h = np.random.default_rng(37).normal(0, 1, x.shape).astype(np.float32)
    add = dev(add_h)
    ret = ops.dwconv3x3_dgrad(**args, add=add, out=add)
    assert ret.data_ptr() == add.data_ptr()
    np.testing.assert_array_equal(host(ret), add_h + got, err_msg=f"{name}: add in place")
    fresh = dev(add_h)
    _bits(ops.dwconv3x3_dgrad(**args, add=fresh), ret, f"{name}: add out of place")
    np.testing.assert_array_equal(host(fresh), add_h)


def test_dgrad_multi_is_its_single_launches():
    from masklab_hip import ops
    mixed = R.MULTI_NAMES + ["stride2", "smallest_c", "in_slice", "one_pixel", "valid"]
    problems = [_dgrad_problem(name) for name in mixed]
    singles = [DM.snapshot(ops.dwconv3x3_dgrad(**args)) for args, _ in problems]
    inputs = [pair for _, ins in problems for pair in ins]
    got = _everything(lambda: ops.dwconv3x3_dgrad_multi([args for args, _ in problems]), inputs, "dgrad multi")
    DM.assert_same_bits(got, singles, "one multi launch against its single launches")
    alone = DM.snapshot(ops.dwconv3x3_dgrad_multi([args for args, _ in problems[:3]]))
    DM.assert_same_bits(alone, singles[:3], "the three dilations alone")
    args = problems[0][0]
    with pytest.raises(RuntimeError, match="write the same dx"):
        out = torch.empty(reference(mixed[0])[1].shape, dtype=torch.float32, device="cuda")
        ops.dwconv3x3_dgrad_multi([dict(args, out=out), dict(args, out=out)])


# ------------------------------------------------------------------ the layer
@pytest.mark.parametrize("name", ["dil6", "stride2", "no_bias"])
def test_depthwise_layer_backward_is_the_ops(name):
    from masklab_hip import keras_like as K, ops
    g, x, w, dy, dw, db, dx, S_w, S_b, S_x = reference(name)
    layer = K.DepthwiseConv2D((3, 3), strides=(g["stride"],) * 2, padding=g["padding"], dilation_rate=(g["dilation"],) * 2,
                              use_bias=g["want_bias"], name="unit/dw")
    layer.build(x.shape)
    weights = {"unit/dw/depthwise_kernel": w}
    if g["want_bias"]:
        weights["unit/dw/bias"] = np.random.default_rng(41).normal(0, 1, g["C"]).astype(np.float32)
    layer.load_weights(weights, torch.device("cuda:0"))
    xd, dyd = dev(x), dev(dy)
    got_dx, grads = layer.backward(xd, dyd)
    assert list(grads) == (["depthwise_kernel", "bias"] if g["want_bias"] else ["depthwise_kernel"])
    want = ops.dwconv3x3_wgrad(xd, dyd, g["stride"], g["padding"], g["dilation"], want_bias=g["want_bias"])
    _bits([grads["depthwise_kernel"], grads.get("bias")], list(want), "DepthwiseConv2D.backward: the weight gradient")
    _bits(got_dx, ops.dwconv3x3_dgrad(dyd, layer.wgt, x.shape, g["stride"], g["padding"], g["dilation"]),
          "DepthwiseConv2D.backward: the data gradient")
    R.check(host(grads["depthwise_kernel"]), dw, S_w, "DepthwiseConv2D.backward dw")
    R.check(host(got_dx), dx, S_x, "DepthwiseConv2D.backward dx")
    none_dx, again = layer.backward(xd, dyd, need_dx=False)
    assert none_dx is None
    _bits(again, grads, "need_dx=False: the same weight bits")
    add_h = np.random.default_rng(43).normal(0, 1, x.shape).astype(np.float32)
    np.testing.assert_array_equal(host(layer.backward(xd, dyd, add=dev(add_h))[0]), add_h + host(got_dx))
