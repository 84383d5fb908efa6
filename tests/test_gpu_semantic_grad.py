"""GPU tests of the semantic head's backward: ASPPNetwork / SegmentationSubNet call_with_tape and backward (layers/semantic.py),
against torch autograd in float64 over a restatement of the head (this file's `head_forward`: the convs of
tests/conv_grad_ref.py and tests/dwconv_grad_ref.py, the chunk-wise GroupNormalization of tests/groupnorm_grad_ref.py, the
align_corners resize of tests/resample_grad_ref.py).  The head is ASPPNetwork (32 features, 8 groups, rates (1, 2, 6)) on a
[2, 6, 7, 64] input -- rate 6 leaves only the centre row of taps, and of the outer columns one pixel pair each -- feeding
SegmentationSubNet (depth 2, 32 features, 16 skip features, 3 classes) with a [2, 11, 13, 32] skip input.

GroupNormalization's cancellation makes a fixed bar meaningless here, so -- as for the detection towers -- every gradient
tensor is held to 4 x the error of the SAME restatement evaluated in float32 on the CPU, both relative to the tensor's
largest magnitude.  The ReLUs' kinks: the float64 reference's pre-ReLU values all lie at least KINK from 0 (asserted; the
seed is chosen for it), far beyond any float32 error of those values, so no evaluation takes another side of a kink.
-m gpu.

Measured on the MI355X (largest error relative to max |want| over every tensor):
    float32 CPU restatement 1.16e-06, device 6.7e-07 (both at concat_projection_GN/gamma); the depthwise kernels' gradients:
    rate 1 2.6e-07 / 4.1e-07, rate 2 5.8e-07 / 5.6e-07 (restatement / device); the tensor closest to its 4 x bound:
    skip_projection_GN/beta, 2.3e-07 against 4 x 1.1e-07 (2.1 x)"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import conv_grad_ref as CR
import dwconv_grad_ref as DR
import groupnorm_grad_ref as GR
import optimizer_ref as OR
import resample_grad_ref as RR
from test_gpu_resample_grad import _bits, _everything, _kernels

NF, GROUPS, RATES, SKIP, CLASSES, DEPTH = 32, 8, (1, 2, 6), 16, 3, 2
ASPP_IN, SKIP_IN = (2, 6, 7, 64), (2, 11, 13, 32)
KINK = 5e-5            # pre-ReLU values are O(1) and their float32 error a few 1e-7: 100 x beyond it
SEED = 14              # the first weight seed whose float64 reference keeps every pre-ReLU value KINK from 0


def make_nets():
    from masklab_hip.layers.semantic import ASPPNetwork, SegmentationSubNet
    aspp = ASPPNetwork(num_features=NF, atrous_rate=RATES, groups=GROUPS, name="aspp")
    seg = SegmentationSubNet(num_depth=DEPTH, num_features=NF, num_skip_features=SKIP, num_classes=CLASSES, groups=GROUPS,
                             name="seg")
    dec_shape = aspp.build(ASPP_IN)
    seg.build([dec_shape, SKIP_IN])
    return aspp, seg


def make_weights(specs, seed):
    """N(0, 0.2) dense kernels, N(0, 0.5) depthwise kernels, N(0, 0.1) biases and betas, gamma ~ U(0.5, 1.5)"""
    r = np.random.default_rng(seed)
    out = {}
    for name, spec in specs.items():
        if name.endswith("/depthwise_kernel"):
            out[name] = r.normal(0, 0.5, spec.shape).astype(np.float32)
        elif name.endswith("/kernel"):
            out[name] = r.normal(0, 0.2, spec.shape).astype(np.float32)
        elif name.endswith("/gamma"):
            out[name] = r.uniform(0.5, 1.5, spec.shape).astype(np.float32)
        else:
            out[name] = r.normal(0, 0.1, spec.shape).astype(np.float32)
    return out


def _resize(x, oh, ow):
    My = torch.from_numpy(RR.resize_axis_matrix(x.shape[1], oh)).to(x.dtype)
    Mx = torch.from_numpy(RR.resize_axis_matrix(x.shape[2], ow)).to(x.dtype)
    return torch.einsum("ph,qw,bhwc->bpqc", My, Mx, x)


def head_forward(x, skip, w):
    """The head in the dtype of its tensors -> (the output conv's PRE-activation, the ASPP's output, every pre-ReLU value)"""
    pre = []

    def gn_relu(z, name):
        y = GR.restatement(z, w[f"{name}/gamma"], w[f"{name}/beta"], GROUPS)
        pre.append(y)
        return torch.relu(y)

    def c1(z, name):
        return CR.conv(z, w[f"{name}/kernel"], w.get(f"{name}/bias"), 1, 1, (0, 0, 0, 0))

    B, H, W, _ = x.shape
    parts = [gn_relu(c1(x, "aspp_1x1"), "aspp_1x1_GN")]
    for r in RATES:
        _, _, pads = CR.pads_of(H, W, 3, 3, 1, r, "same")
        d = DR.dwconv(x, w[f"aspp_{r}_depthwise/depthwise_kernel"], None, 1, r, pads)
        d = gn_relu(d, f"aspp_{r}_depthwise_GN")
        parts.append(gn_relu(c1(d, f"aspp_{r}_pointwise"), f"aspp_{r}_pointwise_GN"))
    pool = c1(x.mean(dim=(1, 2), keepdim=True), "aspp_pool")
    pre.append(pool)
    parts.append(torch.relu(pool).expand(B, H, W, NF))          # the align_corners resize of a 1 x 1 map
    aspp_out = gn_relu(c1(torch.cat(parts, dim=3), "concat_projection"), "concat_projection_GN")
    s = gn_relu(c1(skip, "skip_projection"), "skip_projection_GN")
    z = torch.cat([_resize(aspp_out, skip.shape[1], skip.shape[2]), s], dim=3)
    for i in range(DEPTH):
        t = CR.conv(z, w[f"seg/conv{i}/kernel"], w[f"seg/conv{i}/bias"], 1, 1, (1, 1, 1, 1))
        pre.append(t)
        z = GR.restatement(torch.relu(t), w[f"seg/gn{i}/gamma"], w[f"seg/gn{i}/beta"], GROUPS)
    return c1(z, "seg/output"), aspp_out, pre


def head_autograd(x, skip, weights, d_seg, dtype):
    """-> (dx, dskip, {name: gradient}, the smallest |pre-ReLU value|, seg pre-activation, aspp_out): NumPy in `dtype`"""
    leaf = lambda a: torch.from_numpy(np.asarray(a, dtype)).requires_grad_(True)
    xt, st = leaf(x), leaf(skip)
    ws = {k: leaf(v) for k, v in weights.items()}
    out, aspp_out, pre = head_forward(xt, st, ws)
    assert out.dtype == (torch.float64 if dtype == np.float64 else torch.float32)
    (out * torch.from_numpy(np.asarray(d_seg, dtype))).sum().backward()
    kink = min(float(z.detach().abs().min()) for z in pre)
    return (xt.grad.numpy(), st.grad.numpy(), {k: v.grad.numpy() for k, v in ws.items()}, kink, out.detach().numpy(),
            aspp_out.detach().numpy())


@functools.lru_cache(maxsize=None)
def head_reference():
    aspp, seg = make_nets()
    specs = dict(aspp.weight_specs())
    specs.update(seg.weight_specs())
    weights = make_weights(specs, SEED)
    r = np.random.default_rng(47)
    x, skip = r.normal(0, 1, ASPP_IN).astype(np.float32), r.normal(0, 1, SKIP_IN).astype(np.float32)
    d_seg = r.normal(0, 1, SKIP_IN[:3] + (CLASSES,)).astype(np.float32)
    want = head_autograd(x, skip, weights, d_seg, np.float64)
    f32 = head_autograd(x, skip, weights, d_seg, np.float32)
    return weights, x, skip, d_seg, want, f32


def _loaded():
    aspp, seg = make_nets()
    weights = head_reference()[0]
    aspp.load_weights(weights, torch.device("cuda:0"))
    seg.load_weights(weights, torch.device("cuda:0"))
    return aspp, seg


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def _head_backward(aspp, seg, xd, sd, dd, need_dx=(True, True), need_x=True):
    """call_with_tape and backward of the whole head -> (seg pre-sigmoid prediction's tensor, (dx, dskip), grads)"""
    a_out, a_tape = aspp.call_with_tape(xd)
    pred, s_tape = seg.call_with_tape([a_out, sd])
    (d_aspp, d_skip), grads = seg.backward(s_tape, dd, need_dx=need_dx)
    dx = None
    if d_aspp is not None:
        dx, ga = aspp.backward(a_tape, d_aspp, need_dx=need_x)
        grads = dict(grads, **ga)
    return pred, a_out, (dx, d_skip), grads


def test_call_with_tape_is_call():
    aspp, seg = _loaded()
    weights, x, skip, d_seg, want, f32 = head_reference()
    xd, sd = dev(x), dev(skip)
    (a_out, a_tape), a_taped = _kernels(lambda: aspp.call_with_tape(xd))
    a_call, a_called = _kernels(lambda: aspp.call(xd))
    _bits(a_out, a_call, "ASPPNetwork.call_with_tape's output against call's")
    assert a_called and a_taped == a_called, "ASPPNetwork: call_with_tape's launches are not call's"
    (pred, s_tape), s_taped = _kernels(lambda: seg.call_with_tape([a_out, sd]))
    s_call, s_called = _kernels(lambda: seg.call([a_out, sd]))
    _bits(pred, s_call, "SegmentationSubNet.call_with_tape's output against call's")
    assert s_called and s_taped == s_called, "SegmentationSubNet: call_with_tape's launches are not call's"
    np.testing.assert_array_equal(host(xd), x)
    assert _rel(host(a_out), want[5]) <= 1e-5
    sig = 1.0 / (1.0 + np.exp(-want[4]))
    assert np.abs(host(pred) - sig).max() <= 1e-5
    for key in ("inputs", "aspp_1x1_out", "branches", "pool_in", "pool_out", "cat", "concat_out"):
        assert key in a_tape
    assert a_tape["pool_out"].shape == (2, 1, 1, NF) and float(a_tape["pool_out"].min()) >= 0.0       # post-ReLU
    assert len(s_tape["conv_in"]) == len(s_tape["conv_out"]) == DEPTH


def test_head_backward():
    """Every gradient tensor and both input gradients against float64 autograd, each held to 4 x the float32 CPU
    restatement's error (the module docstring's figures)."""
    from masklab_hip import optimizers
    aspp, seg = _loaded()
    weights, x, skip, d_seg, want, f32 = head_reference()
    assert want[3] >= KINK, f"a pre-ReLU value lies {want[3]:.3g} from the kink: choose another seed"
    xd, sd, dd = dev(x), dev(skip), dev(d_seg)
    run = lambda: _head_backward(aspp, seg, xd, sd, dd)[2:]
    (dx, d_skip), grads = run()
    assert sorted(grads) == sorted(weights)
    worst_dev = worst_f32 = 0.0
    closest = (0.0, "")
    for name, g, w64, w32 in ([("dx", dx, want[0], f32[0]), ("dskip", d_skip, want[1], f32[1])] +
                              [(n, grads[n], want[2][n], f32[2][n]) for n in sorted(grads)]):
        assert tuple(g.shape) == w64.shape and g.dtype == torch.float32, name
        e32, edev = _rel(w32, w64), _rel(host(g), w64)
        worst_dev, worst_f32 = max(worst_dev, edev), max(worst_f32, e32)
        closest = max(closest, (edev / max(e32, 1e-300), name))
        print(f"{name}: float32 restatement {e32:.3g}, device {edev:.3g}")
        assert edev <= 4 * e32, f"{name}: device {edev:.3g} against 4 x {e32:.3g}"
    print(f"largest relative error  float32 restatement {worst_f32:.3g}  device {worst_dev:.3g}; closest to its bound: "
          f"{closest[1]} at {closest[0]:.3g} x")
    # the dead taps of rate 6 on a 6 x 7 map: exact zeros
    dead = want[2]["aspp_6_depthwise/depthwise_kernel"].reshape(9, -1)
    got6 = host(grads["aspp_6_depthwise/depthwise_kernel"]).reshape(9, -1)
    rows = [t for t in range(9) if not dead[t].any()]
    assert rows == [0, 1, 2, 6, 7, 8] and not got6[rows].any()
    # the battery on the whole backward: the same bits from two passes, from stale and from zeroed memory; inputs unchanged
    got = _everything(run, [(xd, x), (sd, skip), (dd, d_seg)], "head backward")
    _bits([(dx, d_skip), grads], list(got), "head backward: the battery's first pass")
    # need_dx=False arms return None and the same weight bits
    _, _, (ndx, nskip), ngrads = _head_backward(aspp, seg, xd, sd, dd, need_dx=(True, False), need_x=False)
    assert ndx is None and nskip is None
    _bits(ngrads, grads, "need_dx=False: the same weight bits")
    a_out, _ = aspp.call_with_tape(xd)
    _, s_tape = seg.call_with_tape([a_out, sd])
    (nd, ns), sgrads = seg.backward(s_tape, dd, need_dx=(False, True))
    assert nd is None
    _bits(ns, d_skip, "need_dx=(False, True): the skip input's gradient")
    _bits(sgrads, {k: v for k, v in grads.items() if k in sgrads}, "need_dx=(False, True): the same weight bits")
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


def test_atrous_branch_backward_alone_is_the_aspp_s():
    """AtrousSeparableConv2D.backward on its own gives the bits the branch has inside the ASPP's multi launches"""
    aspp, seg = _loaded()
    weights, x, skip, d_seg, want, f32 = head_reference()
    xd = dev(x)
    br = aspp.aspp_branches[2]
    (out, tape), taped = _kernels(lambda: br.call_with_tape(xd))
    call, called = _kernels(lambda: br.call(xd))
    _bits(out, call, "AtrousSeparableConv2D.call_with_tape's output against call's")
    assert called and taped == called, "AtrousSeparableConv2D: call_with_tape's launches are not call's"
    dy_h = np.random.default_rng(53).normal(0, 1, tuple(out.shape)).astype(np.float32)
    dx, grads = br.backward(tape, dev(dy_h))
    assert sorted(grads) == sorted(n for n in weights if n.startswith("aspp_6_"))
    none_dx, again = br.backward(br.call_with_tape(xd)[1], dev(dy_h), need_dx=False)
    assert none_dx is None
    _bits(again, grads, "need_dx=False: the same weight bits")
    add_h = np.random.default_rng(59).normal(0, 1, x.shape).astype(np.float32)
    with_add = br.backward(br.call_with_tape(xd)[1], dev(dy_h), add=dev(add_h))[0]
    np.testing.assert_array_equal(host(with_add), add_h + host(dx))


def test_refusals():
    from masklab_hip.layers.semantic import SegmentationSubNet
    aspp, seg = _loaded()
    weights, x, skip, d_seg, want, f32 = head_reference()
    xd, sd = dev(x), dev(skip)
    a_out, a_tape = aspp.call_with_tape(xd)
    pred, s_tape = seg.call_with_tape([a_out, sd])
    with pytest.raises(TypeError, match="float32 only"):
        seg.backward(s_tape, dev(d_seg).half())
    with pytest.raises(ValueError, match="expected a contiguous"):
        seg.backward(s_tape, dev(d_seg[:, :-1]))
    with pytest.raises(TypeError, match="float32 only"):
        aspp.backward(a_tape, a_out.half())
    for kw, message in ((dict(use_squeeze_excite=True), "SqueezeExcite"), (dict(use_separable_conv=True), "MobileSeparableConv2D")):
        net = SegmentationSubNet(num_depth=DEPTH, num_features=NF, num_skip_features=SKIP, num_classes=CLASSES, groups=GROUPS,
                                 name="seg_v", **kw)
        with pytest.raises(NotImplementedError, match=message):
            net.call_with_tape([a_out, sd])
        with pytest.raises(NotImplementedError, match=message):
            net.backward(s_tape, dev(d_seg))
