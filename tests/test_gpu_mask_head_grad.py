"""GPU tests of the mask head's backward: MaskSubNet.call_with_tape and MaskSubNet.backward (layers/instance.py), against torch
autograd in float64 over a restatement of the head (this file's `head_forward`: the convs of tests/conv_grad_ref.py, the
chunk-wise GroupNormalization of tests/groupnorm_grad_ref.py, the tail of tests/mask_tail_grad_ref.py).  The head is
MaskSubNet(num_blocks=2, num_classes=3, num_depth=1, num_features=128, groups=16) on two levels of [2, n_l, 2, 3, 128] crops
with n_l = (2, 1).

GroupNormalization's cancellation makes a fixed bar meaningless here, so -- as for the detection towers and the semantic
head -- every gradient tensor is held to 4 x the error of the SAME restatement evaluated in float32 on the CPU, both relative
to the tensor's largest magnitude.  The ReLUs' kinks: the float64 reference's pre-ReLU values, the towers' and the transposed
convs', all lie at least KINK from 0 (asserted; the seed is chosen for it, on the CPU), far beyond any float32 error of those
values, so no evaluation takes another side of a kink.  -m gpu.

Measured on the MI355X (largest error relative to max |want| over every tensor):
    float32 CPU restatement 8.38e-07 (block1/gn0/gamma), device 8.04e-07 (d_inputs[0]); the tail's tensors, restatement / device:
    deconv/kernel 4.0e-07 / 4.6e-07 and 7.1e-07 / 6.8e-07, deconv/bias 1.1e-07 / 7.8e-08 and 2.8e-07 / 1.5e-07, output/kernel
    6.2e-07 / 5.3e-07 and 6.1e-07 / 4.4e-07, output/bias 6.7e-08 / 2.3e-08 and 3.5e-08 / 3.5e-08 (the dy sums are fp64 on the
    device: the rounded exact sum); the tensor closest to its 4 x bound: d_inputs[0], 8.0e-07 against 4 x 5.5e-07 (1.5 x)"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import conv_grad_ref as CR
import groupnorm_grad_ref as GR
import mask_tail_grad_ref as TR
import optimizer_ref as OR
from test_gpu_resample_grad import _bits, _everything, _kernels

NB, CLASSES, DEPTH, NF, GROUPS = 2, 3, 1, 128, 16
N_L, CROP = (2, 1), (2, 3)
INPUTS = [(2, n, CROP[0], CROP[1], NF) for n in N_L]
KINK = 5e-5            # pre-ReLU values are O(1) and their float32 error a few 1e-7: 100 x beyond it
SEED = 0               # the first weight seed whose float64 reference keeps every pre-ReLU value KINK from 0 (found on the CPU)


def make_net(name="mask", **kw):
    from masklab_hip.layers.instance import MaskSubNet
    net = MaskSubNet(num_blocks=NB, num_classes=CLASSES, num_depth=DEPTH, num_features=NF, groups=GROUPS, name=name, **kw)
    net.build(INPUTS)
    return net


def make_weights(specs, seed):
    """N(0, 0.2) kernels, N(0, 0.1) biases and betas, gamma ~ U(0.5, 1.5)"""
    r = np.random.default_rng(seed)
    out = {}
    for name, spec in specs.items():
        if name.endswith("/kernel"):
            out[name] = r.normal(0, 0.2, spec.shape).astype(np.float32)
        elif name.endswith("/gamma"):
            out[name] = r.uniform(0.5, 1.5, spec.shape).astype(np.float32)
        else:
            out[name] = r.normal(0, 0.1, spec.shape).astype(np.float32)
    return out


def head_forward(inputs, w, name="mask"):
    """The head in the dtype of its tensors -> (the output convs' PRE-activation [B, total, 2h, 2w, classes], every pre-ReLU value)"""
    outs, pre = [], []
    for l, x5 in enumerate(inputs):
        B, n_l = x5.shape[:2]
        x = x5.reshape((B * n_l,) + tuple(x5.shape[2:]))
        p = f"{name}/block{l}"
        for i in range(DEPTH):
            z = CR.conv(x, w[f"{p}/conv{i}/kernel"], w[f"{p}/conv{i}/bias"], 1, 1, (1, 1, 1, 1))
            pre.append(z)
            x = GR.restatement(torch.relu(z), w[f"{p}/gn{i}/gamma"], w[f"{p}/gn{i}/beta"], GROUPS)
        z, t = TR.tail_forward(x, w[f"{p}/deconv/kernel"], w[f"{p}/deconv/bias"], w[f"{p}/output/kernel"], w[f"{p}/output/bias"])
        pre.append(t)
        outs.append(z.reshape((B, n_l) + tuple(z.shape[1:])))
    return torch.cat(outs, dim=1), pre


def head_autograd(inputs, weights, d_masks, dtype):
    """-> (d inputs per level, {name: gradient}, the smallest |pre-ReLU value|, the pre-sigmoid output): NumPy in `dtype`"""
    leaf = lambda a: torch.from_numpy(np.asarray(a, dtype)).requires_grad_(True)
    xs = [leaf(a) for a in inputs]
    ws = {k: leaf(v) for k, v in weights.items()}
    out, pre = head_forward(xs, ws)
    assert out.dtype == (torch.float64 if dtype == np.float64 else torch.float32)
    (out * torch.from_numpy(np.asarray(d_masks, dtype))).sum().backward()
    kink = min(float(z.detach().abs().min()) for z in pre)
    return [x.grad.numpy() for x in xs], {k: v.grad.numpy() for k, v in ws.items()}, kink, out.detach().numpy()


def case(seed):
    weights = make_weights(make_net().weight_specs(), seed)
    r = np.random.default_rng(61)
    inputs = [r.normal(0, 1, s).astype(np.float32) for s in INPUTS]
    d_masks = r.normal(0, 1, (2, sum(N_L), 2 * CROP[0], 2 * CROP[1], CLASSES)).astype(np.float32)
    return weights, inputs, d_masks


@functools.lru_cache(maxsize=None)
def head_reference():
    weights, inputs, d_masks = case(SEED)
    want = head_autograd(inputs, weights, d_masks, np.float64)
    f32 = head_autograd(inputs, weights, d_masks, np.float32)
    return weights, inputs, d_masks, want, f32


def _loaded():
    net = make_net()
    net.load_weights(head_reference()[0], torch.device("cuda:0"))
    return net


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def test_call_with_tape_is_call():
    net = _loaded()
    weights, inputs, d_masks, want, f32 = head_reference()
    xs = [dev(a) for a in inputs]
    (masks, tape), taped = _kernels(lambda: net.call_with_tape(xs))
    call, called = _kernels(lambda: net.call(xs))
    _bits(masks, call, "MaskSubNet.call_with_tape's roi_masks against call's")
    # the same launches but the tail's, which also stores T
    assert called.count("deconv2x2_out1x1") == 1 and "deconv2x2_out1x1_tape" not in called
    assert taped == ["deconv2x2_out1x1_tape" if k == "deconv2x2_out1x1" else k for k in called]
    for x, a in zip(xs, inputs):
        np.testing.assert_array_equal(host(x), a)
    assert np.abs(host(masks) - 1.0 / (1.0 + np.exp(-want[3]))).max() <= 1e-5
    assert len(tape["conv_in"]) == len(tape["conv_out"]) == DEPTH and len(tape["tail_in"]) == len(tape["T"]) == NB
    for T, n in zip(tape["T"], N_L):
        assert tuple(T.shape) == (2 * n * CROP[0] * CROP[1], 4, NF) and T.dtype == torch.float32 and float(T.min()) >= 0.0


def test_head_backward():
    """Every gradient tensor and the input gradients against float64 autograd, each held to 4 x the float32 CPU
    restatement's error"""
    from masklab_hip import optimizers
    net = _loaded()
    weights, inputs, d_masks, want, f32 = head_reference()
    assert want[2] >= KINK, f"a pre-ReLU value lies {want[2]:.3g} from the kink: choose another seed"
    xs, dd = [dev(a) for a in inputs], dev(d_masks)

    def run(**kw):
        _, tape = net.call_with_tape(xs)
        return net.backward(tape, dd, **kw)

    dxs, grads = run()
    assert sorted(grads) == sorted(weights) and len(dxs) == NB
    worst_dev = worst_f32 = 0.0
    closest = (0.0, "")
    for name, g, w64, w32 in ([(f"d_inputs[{l}]", dxs[l], want[0][l], f32[0][l]) for l in range(NB)] +
                              [(n, grads[n], want[1][n], f32[1][n]) for n in sorted(grads)]):
        assert tuple(g.shape) == w64.shape and g.dtype == torch.float32, name
        e32, edev = _rel(w32, w64), _rel(host(g), w64)
        worst_dev, worst_f32 = max(worst_dev, edev), max(worst_f32, e32)
        closest = max(closest, (edev / max(e32, 1e-300), name))
        print(f"{name}: float32 restatement {e32:.3g}, device {edev:.3g}")
        assert edev <= 4 * e32, f"{name}: device {edev:.3g} against 4 x {e32:.3g}"
    print(f"largest relative error  float32 restatement {worst_f32:.3g}  device {worst_dev:.3g}; closest to its bound: "
          f"{closest[1]} at {closest[0]:.3g} x")
    # the battery on the whole backward: the same bits from two passes, from stale and from zeroed memory; inputs unchanged
    got = _everything(run, [(x, a) for x, a in zip(xs, inputs)] + [(dd, d_masks)], "head backward")
    _bits([dxs, grads], list(got), "head backward: the battery's first pass")
    # need_dx=False returns None and the same weight bits; so does the backward that writes dT over the tape
    ndx, ngrads = run(need_dx=False)
    assert ndx is None
    _bits(ngrads, grads, "need_dx=False: the same weight bits")
    _, tape = net.call_with_tape(xs)
    cdx, cgrads = net.backward(tape, dd, consume_tape=True)
    _bits([cdx, cgrads], [dxs, grads], "consume_tape=True: the same bits")
    assert tape["T"] is None
    with pytest.raises(ValueError, match="holds no T"):
        net.backward(tape, dd)
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


def test_refusals():
    from masklab_hip import ops
    net = _loaded()
    weights, inputs, d_masks, want, f32 = head_reference()
    xs = [dev(a) for a in inputs]
    masks, tape = net.call_with_tape(xs)
    with pytest.raises(TypeError, match="float32 only"):
        net.backward(tape, dev(d_masks).half())
    with pytest.raises(ValueError, match="expected a contiguous"):
        net.backward(tape, dev(d_masks[:, :-1]))
    with pytest.raises(NotImplementedError, match="fixed-capacity form"):
        net.call_with_tape(xs, lives=[(torch.ones(1, dtype=torch.int32, device="cuda"), n) for n in N_L])
    with pytest.raises(NotImplementedError, match="float32 tensors only"):
        net.call_with_tape([x.half() for x in xs])
    old = ops.CONV_MATH
    try:
        ops.CONV_MATH = "f16"
        with pytest.raises(NotImplementedError, match="set_conv_math"):
            net.call_with_tape(xs)
        with pytest.raises(NotImplementedError, match="set_conv_math"):
            net.backward(tape, dev(d_masks))
    finally:
        ops.CONV_MATH = old
    tables, net._tail_tables = net._tail_tables, None
    try:
        with pytest.raises(NotImplementedError, match="outside the fused tail"):
            net.call_with_tape(xs)
        with pytest.raises(NotImplementedError, match="outside the fused tail"):
            net.backward(tape, dev(d_masks))
    finally:
        net._tail_tables = tables
    for kw, message in ((dict(use_squeeze_excite=True), "SqueezeExcite"), (dict(use_separable_conv=True), "MobileSeparableConv2D")):
        v = make_net("mask_v", **kw)
        v._tail_tables = net._tail_tables
        with pytest.raises(NotImplementedError, match=message):
            v.call_with_tape(xs)
        with pytest.raises(NotImplementedError, match=message):
            v.backward(tape, dev(d_masks))
    with pytest.raises(NotImplementedError, match="Conv2DTranspose.backward"):
        net.blocks[0][-2].backward(xs[0], None)


def test_loss_to_pyramid_chain():
    """MaskLoss.call_with_grad(through_sigmoid=True) -> MaskSubNet.backward -> PyramidRoiAlign.backward: finite gradients of
    the pyramid levels' shapes, and every head weight receives one that steps under RectifiedAdam bit for bit"""
    from masklab_hip import optimizers
    from masklab_hip.layers.instance import PyramidRoiAlign
    from masklab_hip.losses import MaskLoss
    net = _loaded()
    weights = head_reference()[0]
    r = np.random.default_rng(67)
    shapes = [(2, 16, 16, NF), (2, 8, 8, NF)]
    fmaps = [dev(r.normal(0, 1, s).astype(np.float32)) for s in shapes]
    pad = (-1,) * 7
    rows = np.array([[(0, 20.3, 18.7, 17.9, 13.3, 0, 0.5), (0, 41.0, 30.0, 12.0, 22.0, 2, 0.5), (1, 32.0, 32.0, 40.0, 36.0, 1, 0.5), pad],
                     [(1, 22.0, 40.0, 30.0, 28.0, 2, 0.5), (0, 12.0, 12.0, 9.0, 14.0, 1, 0.5), pad, pad]], np.float32)
    align = PyramidRoiAlign(crop_size=CROP, name="align")
    rows_d = dev(rows)
    slots, lcounts, lmax = align.distribute(2, rows_d, has_k=True)
    roi_fmaps, roi_boxes = align.crop_distributed(fmaps, rows_d, (64, 64), slots, lcounts, lmax)
    assert [tuple(t.shape) for t in roi_fmaps] == INPUTS
    masks, tape = net.call_with_tape(roi_fmaps)
    mask_true = r.integers(0, CLASSES + 1, (2, sum(N_L), 2 * CROP[0], 2 * CROP[1])).astype(np.int32)
    mask_true[0, 0, 0, 0], mask_true[1, 0, 0, 0] = 0, 2                        # at least one selected RoI per image
    loss, d_masks = MaskLoss().call_with_grad([dev(mask_true), masks], through_sigmoid=True)
    assert tuple(d_masks.shape) == tuple(masks.shape) and np.isfinite(host(loss)).all()
    d_rois, grads = net.backward(tape, d_masks)
    d_fmaps = align.backward(d_rois, shapes, rows_d, (64, 64), slots, lcounts)
    assert [tuple(t.shape) for t in d_fmaps] == shapes
    for t in d_fmaps:
        a = host(t)
        assert np.isfinite(a).all() and a.any()
    assert sorted(grads) == sorted(weights)
    for n, g in grads.items():
        a = host(g)
        assert a.shape == weights[n].shape and np.isfinite(a).all() and a.any(), n
    params = {n: dev(weights[n]) for n in weights}
    g_h = {n: host(grads[n]) for n in grads}
    opt = optimizers.RectifiedAdam(1e-3)
    opt.apply_gradients(params, grads)
    different = 0
    for n in weights:
        p, g = weights[n].reshape(-1), g_h[n].reshape(-1)
        zero = np.zeros_like(p)
        new = OR.element32("RectifiedAdam", opt.scalars, p, g, zero, zero)[0]
        different += int((host(params[n]).reshape(-1).view(np.uint32) != new.view(np.uint32)).sum())
    assert different == 0, f"{different} stepped weights differ from the float32 evaluation"
