"""GPU tests of the dense convolutions' backward: ops.conv2d_wgrad / conv2d_wgrad_multi (csrc/conv_grad.hip), ops.conv2d_dgrad /
conv2d_dgrad_multi (the forward kernels on transposed weights), Conv2D.backward and the backward of one head tower, against
torch autograd in float64 over the restatements of tests/conv_grad_ref.py.  The bar is the project's gradient bar,
|got - want| <= 1e-5 * S with S the uncancelled magnitude of the element (sum |x| |dy|, sum |dy|, sum |w| |dy|), exact zeros
where S == 0.  A slice's fp32 chain of L terms is off by at most L * 2^-24 * S and behaves like sqrt(L) * 2^-24 * S on random
data; the slices add in fp64.  Every op also holds: two launches give the same bits; the bits do not depend on what outputs
and workspace held; the inputs are left unchanged.  -m gpu.

Largest |got - want| / S measured on the MI355X, per case (the bar is 1e-5):
    dW / db   tower 1.8e-07 / 8.0e-09   cout75_view 2.8e-07 / 6.3e-09   cin_tail 1.4e-07 / 5.8e-09   two_tiles 2.5e-07 / 1.5e-08
              stride2 2.4e-07 / 1.1e-08   k1s2 1.4e-07 / 1.1e-08   dil3 2.1e-07 / 1.6e-08   dead_taps 1.1e-07 / 2.6e-08
              one_pixel 8.6e-08 / 5.4e-08   k5 2.3e-07 / 1.3e-08   in_slice 2.3e-07 / 7.9e-09   no_bias 2.1e-07 / -
              slices 5.9e-08 / 1.7e-09   long_slices (1 024-pixel slices) 7.6e-09 / 1.6e-10   slices18 2.9e-08 / 7.4e-10
              levels0..4 1.9e-07, 2.3e-07, 1.5e-07, 1.6e-07, 9.2e-08 / 7.0e-09 .. 4.7e-08
    dx        tower 1.8e-07   cout75_view 1.0e-07   dil3 1.7e-07   k1 2.0e-07   valid 2.0e-07   wino128 (Winograd) 1.3e-07
              tower under "f32x3" 8.3e-08; with add= the same figures to within 2e-08
    towers    largest error relative to max |want| over every tensor: float32 CPU restatement 7.4e-07 (loc), 6.9e-07 (cls);
              device 7.1e-07 (loc), 6.3e-07 (cls); the tensor closest to its 4 x bound: loc/block0/gn1/beta, 2.7e-07 against
              4 x 1.1e-07"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import conv_grad_ref as R
import dirty_memory as DM
import optimizer_ref as OR
from test_gpu_resample_grad import _bits, _everything, _kernels


def _dc(w, bias=None):
    from masklab_hip import ops, packing
    return ops.DeviceConv(packing.pack_dense(w, bias), torch.device("cuda:0"))


# ------------------------------------------------------------------ the weight and bias gradient
@functools.lru_cache(maxsize=None)
def wgrad_reference(name):
    """-> (g, x, w, dy, dW, db, S_w, S_b): computed once per case, shared and left unchanged"""
    g, x, w, dy = R.wgrad_inputs(name)
    xs = x[..., g["in_coff"]:g["in_coff"] + g["cin"]]
    dW, db, _ = R.grads(xs, w, dy, g["stride"], g["padding"], g["dilation"])
    S_w, S_b, _ = R.magnitudes(xs, w, dy, g["stride"], g["padding"], g["dilation"])
    return g, x, w, dy, dW, db, S_w, S_b


def _wgrad_problem(name):
    """-> (the arguments of ops.conv2d_wgrad for the case, its (device tensor, host array) inputs)"""
    g, x, w, dy = wgrad_reference(name)[:4]
    xd = dev(x)
    args = dict(x=xd, dc=_dc(w), stride=g["stride"], padding=g["padding"], dilation=g["dilation"], in_coff=g["in_coff"],
                want_bias=g["want_bias"])
    if g["view"]:
        flat = R.in_view(g, dy)
        fd = dev(flat)
        off, cs, bs, _ = R.view_layout(g)
        args.update(dy=None, dy_view=(fd, off, cs, bs))
        return args, [(xd, x), (fd, flat)]
    dyd = dev(dy)
    args.update(dy=dyd)
    return args, [(xd, x), (dyd, dy)]


@pytest.mark.parametrize("name", list(R.WGRAD_CASES))
def test_conv2d_wgrad(name):
    from masklab_hip import ops
    g, x, w, dy, dW, db, S_w, S_b = wgrad_reference(name)
    args, inputs = _wgrad_problem(name)
    got = _everything(lambda **kw: ops.conv2d_wgrad(**args, **kw), inputs, name)
    assert isinstance(got, tuple) and got[0].dtype == np.float32 and got[0].shape == w.shape
    R.check(got[0], dW, S_w, f"{name} dW")
    if g["want_bias"]:
        R.check(got[1], db, S_b, f"{name} db")
    else:
        assert got[1] is None
    if name == "dead_taps":
        dead = S_w.reshape(9, -1).max(axis=1) == 0
        assert dead.sum() == 8 and not got[0].reshape(9, -1)[dead].any()            # exact zeros, written (the battery poisons)
    # add= in place is add + the gradient computed separately: one float32 addition, so the very bits
    r = np.random.default_rng(31)
    add_k, add_b = r.normal(0, 1, w.shape).astype(np.float32), r.normal(0, 1, w.shape[3]).astype(np.float32)
    bk, bb = dev(add_k), dev(add_b)
    pair = (bk, bb) if g["want_bias"] else bk
    ret = ops.conv2d_wgrad(**args, add=pair, out=pair)
    assert ret[0].data_ptr() == bk.data_ptr() and (ret[1] is None or ret[1].data_ptr() == bb.data_ptr())
    np.testing.assert_array_equal(host(ret[0]), add_k + got[0], err_msg=f"{name}: add in place, kernel")
    if g["want_bias"]:
        np.testing.assert_array_equal(host(ret[1]), add_b + got[1], err_msg=f"{name}: add in place, bias")
    fresh = (dev(add_k), dev(add_b)) if g["want_bias"] else dev(add_k)
    _bits(ops.conv2d_wgrad(**args, add=fresh), ret, f"{name}: add out of place")


def test_conv2d_wgrad_levels_in_one_launch_are_their_single_launches():
    from masklab_hip import ops
    problems = [_wgrad_problem(name) for name in R.LEVEL_NAMES]
    singles = [DM.snapshot(ops.conv2d_wgrad(**args)) for args, _ in problems]
    inputs = [pair for _, ins in problems for pair in ins]
    got = _everything(lambda: ops.conv2d_wgrad_multi([args for args, _ in problems]), inputs, "levels")
    DM.assert_same_bits(got, singles, "levels: one multi launch against five single launches")
    # and beside problems of other shapes: the slices of a problem do not depend on the launch it rides in
    mixed = ["slices", "levels1", "cout75_view", "levels3", "two_tiles"]
    others = [_wgrad_problem(name) for name in mixed]
    both = DM.snapshot(ops.conv2d_wgrad_multi([args for args, _ in others]))
    for name, b, (args, _) in zip(mixed, both, others):
        _bits(ops.conv2d_wgrad(**args), b, f"{name}: alone against a mixed launch")


def test_conv2d_wgrad_is_the_ascending_fp64_fold_of_its_partials():
    """The finish kernel's sum (csrc/slice_sum.h), restated on the host from the partials the launch left in the conv
    workspace: 18 slices, so the sixteen-wide loop runs once and the remainder loop twice.  part [18][T cin cout] fp32 at
    offset 0, bpart [18][cout] at the next multiple of 256 bytes; added in ascending slice order in float64 and rounded once,
    these are the very additions the kernel makes: bit equality, no tolerance."""
    from masklab_hip import ops
    g, x, w = wgrad_reference("slices18")[:3]
    args, _ = _wgrad_problem("slices18")
    slices, _, nbytes = ops.conv2d_wgrad_plan(g["x_shape"], args["dc"].p)
    assert slices == 18
    dk, db = ops.conv2d_wgrad(**args)
    torch.cuda.synchronize()
    tcc, cout = w.size, g["cout"]
    boff = (slices * tcc * 4 + 255) // 256 * 256
    assert nbytes == boff + (slices * cout * 4 + 255) // 256 * 256
    ws = host(ops.workspace(0, args["x"].device, "conv")[:nbytes])
    part = ws[:slices * tcc * 4].view(np.float32).reshape(slices, tcc)
    bpart = ws[boff:boff + slices * cout * 4].view(np.float32).reshape(slices, cout)
    for got, p, what in ((dk, part, "dkernel"), (db, bpart, "dbias")):
        t = np.zeros(p.shape[1], np.float64)
        for s in range(slices):
            t = t + p[s].astype(np.float64)
        np.testing.assert_array_equal(host(got).reshape(-1).view(np.uint32), t.astype(np.float32).view(np.uint32),
                                      err_msg=f"slices18: {what} against the host fold of its partials")


# ------------------------------------------------------------------ the data gradient
DGRAD_RUNS = [(name, "f32") for name in R.DGRAD_CASES] + [("tower", "f32x3")]


@functools.lru_cache(maxsize=None)
def dgrad_reference(name):
    g, w, dy = R.dgrad_inputs(name)
    zeros = np.zeros(g["x_shape"])
    dx = R.grads(zeros, w, dy, 1, g["padding"], g["dilation"])[2]
    S_x = R.magnitudes(zeros, w, dy, 1, g["padding"], g["dilation"])[2]
    return g, w, dy, dx, S_x


@pytest.mark.parametrize("name,math", DGRAD_RUNS)
def test_conv2d_dgrad(name, math):
    from masklab_hip import ops, packing
    g, w, dy, dx, S_x = dgrad_reference(name)
    dc = _dc(w)
    H, W = g["x_shape"][1:3]
    args = dict(dc=dc, in_hw=g["x_shape"], stride=1, padding=g["padding"], dilation=g["dilation"])
    if g["view"]:
        flat = R.in_view(g, dy)
        fd = dev(flat)
        off, cs, bs, _ = R.view_layout(g)
        args.update(dy=None, dy_view=(fd, off, cs, bs))
        inputs = [(fd, flat)]
    else:
        dyd = dev(dy)
        args.update(dy=dyd)
        inputs = [(dyd, dy)]
    ops.set_conv_math(math)
    try:
        got = _everything(lambda **kw: ops.conv2d_dgrad(**args, **kw), inputs, f"{name} {math}")
        assert got.dtype == np.float32 and got.shape == tuple(g["x_shape"])
        R.check(got, dx, S_x, f"{name} {math} dx")
        if name == "wino128":                               # the transposed tower problem runs on the Winograd kernel
            ops.PROFILE = []
            try:
                ops.conv2d_dgrad(**args)
                assert [rec["kernel"] for rec in ops.PROFILE] == ["conv_wino_f32"]
            finally:
                ops.PROFILE = None
        # add= is the forward's residual: the bits of that launch, and add + gradient within the bar
        add_h = np.random.default_rng(37).normal(0, 1, g["x_shape"]).astype(np.float32)
        add = dev(add_h)
        with_add = DM.snapshot(ops.conv2d_dgrad(**args, add=add))
        cp = -(-g["cout"] // 4) * 4
        dense = np.zeros(dy.shape[:3] + (cp,), np.float32)
        dense[..., :g["cout"]] = dy
        pads = packing.dgrad_padding(H, W, g["k"], g["k"], 1, g["dilation"], g["padding"])
        _bits(ops.conv2d(dev(dense), dc.dgrad, stride=1, padding=pads, dilation=g["dilation"], residual=add), with_add,
              f"{name} {math}: add= against the residual form")
        R.check(with_add, add_h.astype(np.float64) + dx, S_x + np.abs(add_h), f"{name} {math} add + dx")
        np.testing.assert_array_equal(host(add), add_h)
    finally:
        ops.set_conv_math("f32")


def test_conv2d_dgrad_multi_is_its_single_launches():
    from masklab_hip import ops
    problems = []
    for name in ("tower", "dil3"):
        g, w, dy, _, _ = dgrad_reference(name)
        problems.append(dict(dy=dev(dy), dc=_dc(w), in_hw=g["x_shape"][1:3], stride=1, padding=g["padding"], dilation=g["dilation"]))
    multi = DM.snapshot(ops.conv2d_dgrad_multi(problems))
    for pr, m, name in zip(problems, multi, ("tower", "dil3")):
        g, _, _, dx, S_x = dgrad_reference(name)
        R.check(m, dx, S_x, f"{name} in a multi launch")


# ------------------------------------------------------------------ the layer
def test_conv2d_layer_backward_is_the_ops():
    from masklab_hip import keras_like as K, ops
    g, x, w, dy, dW, db, S_w, S_b = wgrad_reference("tower")
    bias = np.random.default_rng(41).normal(0, 1, g["cout"]).astype(np.float32)
    layer = K.Conv2D(g["cout"], (3, 3), padding="same", activation="relu", name="unit/conv")
    layer.build(g["x_shape"])
    layer.load_weights({"unit/conv/kernel": w, "unit/conv/bias": bias}, torch.device("cuda:0"))
    xd, dyd = dev(x), dev(dy)
    dx, grads = layer.backward(xd, dyd)
    assert list(grads) == ["kernel", "bias"]
    want = ops.conv2d_wgrad(xd, dyd, layer.dev, 1, "same", 1)
    _bits([grads["kernel"], grads["bias"]], list(want), "Conv2D.backward: the weight gradient")
    _bits(dx, ops.conv2d_dgrad(dyd, layer.dev, (8, 8), 1, "same", 1), "Conv2D.backward: the data gradient")
    R.check(host(grads["kernel"]), dW, S_w, "Conv2D.backward dW")
    assert layer.backward(xd, dyd, need_dx=False)[0] is None
    nobias = K.Conv2D(g["cout"], (3, 3), padding="same", use_bias=False, name="unit/nobias")
    nobias.build(g["x_shape"])
    nobias.load_weights({"unit/nobias/kernel": w}, torch.device("cuda:0"))
    assert list(nobias.backward(xd, dyd, need_dx=False)[1]) == ["kernel"]
    strided = K.Conv2D(g["cout"], (3, 3), strides=(2, 2), padding="same", name="unit/s2")
    strided.build(g["x_shape"])
    strided.load_weights({"unit/s2/kernel": w, "unit/s2/bias": bias}, torch.device("cuda:0"))
    dy2 = dev(np.zeros((2, 4, 4, 32), np.float32))
    assert strided.backward(xd, dy2, need_dx=False)[1]["kernel"].shape == (3, 3, 32, 32)      # stride 2 has its weight gradient
    with pytest.raises(NotImplementedError, match="stride 2"):
        strided.backward(xd, dy2)


# ------------------------------------------------------------------ one head tower
TOWER = dict(num_depth=2, num_features=32, num_priors=3, groups=4)
TOWER_INPUTS = [(2, 8, 8, 32), (2, 4, 4, 32)]
KINK = 1e-4
TOWER_SEED = 0


def _tower_weights(net, seed):
    """N(0, 0.2) kernels (pre-activations of a few units: none near the ReLU's kink), N(0, 0.1) biases, gamma ~ U(0.5, 1.5)"""
    r = np.random.default_rng(seed)
    out = {}
    for name, spec in net.weight_specs().items():
        if name.endswith("/kernel"):
            out[name] = r.normal(0, 0.2, spec.shape).astype(np.float32)
        elif name.endswith("/gamma"):
            out[name] = r.uniform(0.5, 1.5, spec.shape).astype(np.float32)
        else:
            out[name] = r.normal(0, 0.1, spec.shape).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def tower_reference(kind):
    from masklab_hip.layers.detection import BoxRegressionSubNet, ClassificationSubNet
    if kind == "loc":
        net = BoxRegressionSubNet(2, name="loc", **TOWER)
    else:
        net = ClassificationSubNet(2, 5, name="cls", **TOWER)
    net.build(TOWER_INPUTS)
    weights = _tower_weights(net, TOWER_SEED + (kind == "cls"))
    r = np.random.default_rng(43)
    inputs = [r.normal(0, 1, s).astype(np.float32) for s in TOWER_INPUTS]
    A = sum(s[1] * s[2] * TOWER["num_priors"] for s in TOWER_INPUTS)
    d_pred = r.normal(0, 1, (2, A, net.out_dim)).astype(np.float32)
    want = R.tower_autograd(inputs, weights, d_pred, kind, TOWER["num_depth"], TOWER["groups"], net.out_dim, np.float64)
    f32 = R.tower_autograd(inputs, weights, d_pred, kind, TOWER["num_depth"], TOWER["groups"], net.out_dim, np.float32)
    return net, weights, inputs, d_pred, want, f32


def _rel(got, want):
    """the largest error relative to the tensor's largest magnitude"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("kind", ["loc", "cls"])
def test_tower_backward(kind):
    """Largest error relative to max |want| over every tensor, float32 CPU restatement / device (the device is held to 4 x the
    restatement's figure per tensor): the module docstring's `towers` line."""
    from masklab_hip import optimizers
    net, weights, inputs, d_pred, want, f32 = tower_reference(kind)
    assert want[2] >= KINK, f"a pre-activation lies {want[2]:.3g} from the ReLU's kink: choose another seed"
    net.load_weights(weights, torch.device("cuda:0"))
    xs = [dev(a) for a in inputs]
    (pred, tape), taped = _kernels(lambda: net.call_with_tape(xs))
    call, called = _kernels(lambda: net.call(xs))
    _bits(pred, call, f"{kind}: call_with_tape's prediction against call's")
    assert called and taped == called, f"{kind}: call_with_tape's launches are not call's"
    # the prediction's PRE-activation is what the restatement computes: the sigmoid of the class head is the loss's
    pre = host(pred) if kind == "loc" else None
    if pre is not None:
        assert _rel(pre, want[3]) <= 1e-5
    d_inputs, grads = net.backward(tape, dev(d_pred))
    assert sorted(grads) == sorted(weights) and len(d_inputs) == len(inputs)
    worst_dev = worst_f32 = 0.0
    for name, g, w64, w32 in ([(f"d_inputs[{l}]", d_inputs[l], want[0][l], f32[0][l]) for l in range(len(inputs))] +
                              [(n, grads[n], want[1][n], f32[1][n]) for n in sorted(grads)]):
        assert tuple(g.shape) == w64.shape and g.dtype == torch.float32, name
        e32, edev = _rel(w32, w64), _rel(host(g), w64)
        worst_dev, worst_f32 = max(worst_dev, edev), max(worst_f32, e32)
        print(f"{kind} {name}: float32 restatement {e32:.3g}, device {edev:.3g}")
        assert edev <= 4 * e32, f"{kind} {name}: device {edev:.3g} against 4 x {e32:.3g}"
    print(f"{kind}: largest relative error  float32 restatement {worst_f32:.3g}  device {worst_dev:.3g}")
    # two backward passes give the same bits, the tape is left as it was
    pred2, tape2 = net.call_with_tape(xs)
    again = net.backward(tape2, dev(d_pred))
    _bits([again[0], again[1]], [d_inputs, grads], f"{kind}: two backward passes")
    for x, a in zip(xs, inputs):
        np.testing.assert_array_equal(host(x), a)
    # the gradients go to the optimizer as they are: one RectifiedAdam step is the float32 evaluation, bit for bit
    params = {n: dev(weights[n]) for n in weights}
    g_h = {n: host(grads[n]) for n in grads}
    opt = optimizers.RectifiedAdam(1e-3)
    opt.apply_gradients(params, grads)
    sc = opt.scalars
    different = 0
    for n in weights:
        p, g = weights[n].reshape(-1), g_h[n].reshape(-1)
        zero = np.zeros_like(p)
        new = OR.element32("RectifiedAdam", sc, p, g, zero, zero)[0]
        different += int((host(params[n]).reshape(-1).view(np.uint32) != new.view(np.uint32)).sum())
    assert different == 0, f"{different} stepped weights differ from the float32 evaluation"


def test_tower_backward_refusals():
    from masklab_hip.layers.detection import BoxRegressionSubNet
    net, weights, inputs, d_pred, _, _ = tower_reference("loc")
    net.load_weights(weights, torch.device("cuda:0"))
    pred, tape = net.call_with_tape([dev(a) for a in inputs])
    with pytest.raises(TypeError, match="float32 only"):
        net.backward(tape, dev(d_pred).half())
    with pytest.raises(ValueError, match="expected a contiguous"):
        net.backward(tape, dev(d_pred[:, :-1]))
    se = BoxRegressionSubNet(2, use_squeeze_excite=True, name="loc_se", **TOWER)
    with pytest.raises(NotImplementedError, match="SqueezeExcite"):
        se.call_with_tape([dev(a) for a in inputs])
