"""GPU tests of FeaturePyramid.call_with_tape / backward and BackboneModel.backward_extra_levels against float64 autograd on
the CPU over restatements of the layers (tests/conv_grad_ref.py's conv, tests/resample_grad_ref.py's align-corners resize,
tests/groupnorm_grad_ref.py's chunk-wise GroupNormalization).  The bar is the project's: |got - want| <= 1e-5 * S, S the
uncancelled magnitude of the element.  S is carried along the backward chain: a stage's S is that stage's closed form on
the absolute values of its operands, with the S of the gradient it receives in place of that gradient (the resize's weights
are non-negative; GroupNormalization: groupnorm_grad_ref.scale), and a forward value that the device formed by cancellation
enters at its own uncancelled magnitude (_gn_forward_magnitude).  -m gpu."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import conv_grad_ref as R
import dirty_memory as DM
import groupnorm_grad_ref as GR
import resample_grad_ref as RR

F32, F64 = np.float32, np.float64
DEVICE = "cuda:0"
KINK = 1e-4                                           # no ReLU pre-activation of the float64 restatement is nearer to 0


def _weights(specs, seed):
    """N(0, 0.2) kernels, N(0, 0.1) biases and betas, gamma ~ U(0.5, 1.5)"""
    r = np.random.default_rng(seed)
    out = {}
    for name, spec in specs.items():
        if name.endswith("/kernel"):
            out[name] = r.normal(0, 0.2, spec.shape).astype(F32)
        elif name.endswith("/gamma"):
            out[name] = r.uniform(0.5, 1.5, spec.shape).astype(F32)
        else:
            out[name] = r.normal(0, 0.1, spec.shape).astype(F32)
    return out


def _t(a):
    return torch.from_numpy(np.asarray(a, F64))


# ------------------------------------------------------------------ FeaturePyramid
FPN_SHAPES = [(2, 8, 12, 32), (2, 4, 6, 32), (2, 2, 3, 32)]          # C3 - C5 of a 64 x 96 image
FPN_FEATURES = 32


def _fpn():
    from masklab_hip.layers.detection import FeaturePyramid
    fpn = FeaturePyramid([8, 16, 32], num_features=FPN_FEATURES, name="fpn")
    fpn.build(FPN_SHAPES)
    return fpn


@functools.lru_cache(maxsize=None)
def fpn_reference():
    """-> (weights, inputs, d_outputs, want grads {name: float64}, S {name: float64}, want d_inputs, S d_inputs)"""
    fpn = _fpn()
    weights = _weights(fpn.weight_specs(), 11)
    r = np.random.default_rng(12)
    xs = [r.normal(0, 1, s).astype(F32) for s in FPN_SHAPES]
    dys = [r.normal(0, 1, s[:3] + (FPN_FEATURES,)).astype(F32) for s in FPN_SHAPES]
    names = [(f"fpn/C{p}_lateral", f"fpn/P{p}") for p in (3, 4, 5)]               # finest first
    leaf = lambda a: _t(a).requires_grad_(True)
    xt = [leaf(x) for x in xs]
    wt = {k: leaf(v) for k, v in weights.items()}
    merged, prev, total = [None] * 3, None, 0
    for l in (2, 1, 0):                                                           # the top-down chain, coarsest first
        lat, out = names[l]
        m = R.conv(xt[l], wt[f"{lat}/kernel"], wt[f"{lat}/bias"], 1, 1, (0, 0, 0, 0))
        if prev is not None:
            m = m + RR.resize(prev, m.shape[1], m.shape[2])
        merged[l] = prev = m
        total = total + (R.conv(m, wt[f"{out}/kernel"], wt[f"{out}/bias"], 1, 1, (1, 1, 1, 1)) * _t(dys[l])).sum()
    total.backward()
    want = {k: v.grad.numpy() for k, v in wt.items()}
    want_dx = [x.grad.numpy() for x in xt]
    # S along the chain: the 3x3 convs on the real merged maps, then the top-down transposes, then the laterals
    S, S_lat = {}, [None] * 3
    for l in range(3):
        lat, out = names[l]
        S[f"{out}/kernel"], S[f"{out}/bias"], S_lat[l] = R.magnitudes(merged[l].detach().numpy(), weights[f"{out}/kernel"], dys[l])
    for l in (0, 1):
        S_lat[l + 1] = S_lat[l + 1] + RR.resize_grad(S_lat[l], FPN_SHAPES[l + 1][1], FPN_SHAPES[l + 1][2])[1]
    S_dx = []
    for l in range(3):
        lat = names[l][0]
        S[f"{lat}/kernel"], S[f"{lat}/bias"], s = R.magnitudes(xs[l], weights[f"{lat}/kernel"], S_lat[l])
        S_dx.append(s)
    return weights, xs, dys, want, S, want_dx, S_dx


def test_feature_pyramid_call_with_tape_is_call():
    weights, xs = fpn_reference()[:2]
    fpn = _fpn()
    fpn.load_weights(weights, torch.device(DEVICE))
    xd = [dev(x) for x in xs]
    want = DM.snapshot(fpn(xd))
    outs, tape = fpn.call_with_tape(xd)
    DM.assert_same_bits(DM.snapshot(outs), want, "FeaturePyramid.call_with_tape against call")
    assert [t.data_ptr() for t in tape["inputs"]] == [x.data_ptr() for x in xd]
    assert [tuple(m.shape) for m in tape["merged"]] == [s[:3] + (FPN_FEATURES,) for s in FPN_SHAPES]
    for x, h in zip(xd, xs):
        np.testing.assert_array_equal(host(x), h)


def test_feature_pyramid_backward():
    weights, xs, dys, want, S, want_dx, S_dx = fpn_reference()
    fpn = _fpn()
    fpn.load_weights(weights, torch.device(DEVICE))
    xd, dyd = [dev(x) for x in xs], [dev(d) for d in dys]
    _, tape = fpn.call_with_tape(xd)
    d_inputs, grads = fpn.backward(tape, dyd, need_dx=True)
    assert set(grads) == set(weights) == set(fpn.weight_specs())
    for k in sorted(want):
        R.check(host(grads[k]), want[k], S[k], k)
    for l, (g, w, s) in enumerate(zip(d_inputs, want_dx, S_dx)):
        assert tuple(g.shape) == FPN_SHAPES[l]
        R.check(host(g), w, s, f"d_inputs[{l}]")
    for d, h in zip(dyd, dys):                                    # the caller's gradients are left as they were
        np.testing.assert_array_equal(host(d), h)
    # without the input gradients: the same weight gradients, and twice the same bits
    first = DM.snapshot(grads)
    none, again = fpn.backward(tape, dyd)
    assert none is None
    DM.assert_same_bits(DM.snapshot(again), first, "FeaturePyramid.backward twice")
    with pytest.raises(ValueError, match="2 gradients for 3 levels"):
        fpn.backward(tape, dyd[:2])


# ------------------------------------------------------------------ the extra levels
EXTRA_FEATURES, EXTRA_CIN = 64, 32
EXTRA_MAPS = {"c5_2x3": (2, 2, 3, EXTRA_CIN), "map_5x7": (2, 5, 7, EXTRA_CIN)}    # 2x3 -> 1x2 -> 1x1; 5x7 -> 3x4 -> 2x2


def _backbone():
    """A BackboneModel whose three extra-level layers are built for an EXTRA_CIN-channel tap; its body is never run"""
    from masklab_hip import backbone as BB
    bb = BB.load_backbone("resnet50", ("C3", "C4", "C5", "P6", "P7"), EXTRA_FEATURES)
    s6 = bb.p6_conv.build((None, None, None, EXTRA_CIN))
    bb.p6_norm.build(s6)
    bb.p7_conv.build(s6)
    return bb


def _extra_specs(bb):
    specs = {}
    for l in bb.extra_level_layers():
        specs.update(l.weight_specs())
    return specs


@functools.lru_cache(maxsize=None)
def extra_reference(name):
    from masklab_hip.packing import resolve_padding
    shape = EXTRA_MAPS[name]
    bb = _backbone()
    weights = _weights(_extra_specs(bb), 21)
    r = np.random.default_rng(22 + list(EXTRA_MAPS).index(name))
    c5 = r.normal(0, 1, shape).astype(F32)
    pad = bb.p6_conv.padding
    h6, w6, _, _ = resolve_padding(shape[1], shape[2], 3, 3, 2, 1, pad)
    h7, w7, _, _ = resolve_padding(h6, w6, 3, 3, 2, 1, pad)
    d_p6 = r.normal(0, 1, (shape[0], h6, w6, EXTRA_FEATURES)).astype(F32)
    d_p7 = r.normal(0, 1, (shape[0], h7, w7, EXTRA_FEATURES)).astype(F32)
    pads6, pads7 = R.pads_of(shape[1], shape[2], 3, 3, 2, 1, pad)[2], R.pads_of(h6, w6, 3, 3, 2, 1, pad)[2]
    groups = bb.p6_norm.groups
    leaf = lambda a: _t(a).requires_grad_(True)
    wt = {k: leaf(v) for k, v in weights.items()}

    def run(d6, d7):
        for v in wt.values():
            v.grad = None
        x = leaf(c5)
        z6 = R.conv(x, wt["P6_conv/kernel"], wt["P6_conv/bias"], 2, 1, pads6)
        p6 = torch.relu(z6)
        g6 = GR.restatement(p6, wt["P6_norm/gamma"], wt["P6_norm/beta"], groups)
        z7 = R.conv(g6, wt["P7_conv/kernel"], wt["P7_conv/bias"], 2, 1, pads7)
        p7 = torch.relu(z7)
        total = 0
        if d6 is not None:
            total = total + (p6 * _t(d6)).sum()
        if d7 is not None:
            total = total + (p7 * _t(d7)).sum()
        total.backward()
        kink = min(float(z6.detach().abs().min()), float(z7.detach().abs().min()))
        return ({k: v.grad.numpy().copy() for k, v in wt.items() if v.grad is not None}, x.grad.numpy(),
                [t.detach().numpy() for t in (p6, g6, p7)], kink)

    want, want_dx, (p6, g6, p7), kink = run(d_p6, d_p7)
    assert kink >= KINK, (name, kink)
    # S along the chain, on the real forward values
    S = {}
    dz7 = np.abs(d_p7) * (p7 > 0)
    _, S["P7_conv/bias"], S_g6 = R.magnitudes(g6, weights["P7_conv/kernel"], dz7, 2, pad, 1)
    g6_mag = _gn_forward_magnitude(p6, weights["P6_norm/gamma"], weights["P6_norm/beta"], groups)
    S["P7_conv/kernel"] = R.magnitudes(g6_mag, weights["P7_conv/kernel"], dz7, 2, pad, 1)[0]
    s_dx, S["P6_norm/gamma"], S["P6_norm/beta"] = GR.scale(p6, S_g6, weights["P6_norm/gamma"], weights["P6_norm/beta"], groups)
    dz6 = (s_dx + np.abs(d_p6)) * (p6 > 0)
    S["P6_conv/kernel"], S["P6_conv/bias"], S_dx = R.magnitudes(c5, weights["P6_conv/kernel"], dz6, 2, pad, 1)
    only6 = run(d_p6, None)
    return dict(weights=weights, c5=c5, d_p6=d_p6, d_p7=d_p7, want=want, want_dx=want_dx, S=S, S_dx=S_dx,
                want6=only6[0], want6_dx=only6[1], p6=p6)


def _gn_forward_magnitude(x, gamma, beta, groups):
    """The uncancelled magnitude of GroupNormalization's OUTPUT, (|x| + |mean|) r |gamma| + |beta|.  P7_conv's weight
    gradient is sum g6 * dz7 over the tape's g6, which the device formed in float32: where xhat gamma + beta cancels, g6 is
    off by ulps of its addends, not of itself, so that sum's S takes g6 at this magnitude."""
    xf, _, _, r, _, gam, bet = GR._chunks(x, x, gamma, beta, groups, GR.EPS)
    return ((np.abs(xf) + np.abs(xf.mean(axis=2, keepdims=True))) * r * np.abs(gam) + np.abs(bet)).reshape(x.shape)


def _loaded_backbone(weights):
    bb = _backbone()
    for l in bb.extra_level_layers():
        l.load_weights(weights, torch.device(DEVICE))
    return bb


def _tape(bb, c5):
    """What BackboneModel.call_with_tape keeps, made by the same three calls"""
    p6 = bb.p6_conv(c5)
    g6 = bb.p6_norm(p6)
    return dict(c5=c5, p6=p6, g6=g6, p7=bb.p7_conv(g6))


@pytest.mark.parametrize("name", list(EXTRA_MAPS))
def test_backward_extra_levels(name):
    ref = extra_reference(name)
    bb = _loaded_backbone(ref["weights"])
    assert [l.name for l in bb.extra_level_layers()] == ["P6_conv", "P6_norm", "P7_conv"]
    tape = _tape(bb, dev(ref["c5"]))
    kept = DM.snapshot(tape)
    d6, d7 = dev(ref["d_p6"]), dev(ref["d_p7"])
    d_c5, grads = bb.backward_extra_levels(tape, d6, d7, need_dx=True)
    assert set(grads) == set(ref["weights"])
    for k in sorted(ref["want"]):
        R.check(host(grads[k]), ref["want"][k], ref["S"][k], f"{name} {k}")
    R.check(host(d_c5), ref["want_dx"], ref["S_dx"], f"{name} d_c5")
    np.testing.assert_array_equal(host(d6), ref["d_p6"])          # the caller's gradients and the tape are left as they were
    np.testing.assert_array_equal(host(d7), ref["d_p7"])
    DM.assert_same_bits(DM.snapshot(tape), kept, f"{name}: the tape")
    first = DM.snapshot(grads)
    none, again = bb.backward_extra_levels(tape, d6, d7)
    assert none is None
    DM.assert_same_bits(DM.snapshot(again), first, f"{name}: twice")
    # a backbone without P7: only P6_conv has a gradient
    d_c5, grads = bb.backward_extra_levels(tape, d6, None, need_dx=True)
    assert set(grads) == {"P6_conv/kernel", "P6_conv/bias"}
    dz6 = np.abs(ref["d_p6"]) * (ref["p6"] > 0)
    S_k, S_b, S_x = R.magnitudes(ref["c5"], ref["weights"]["P6_conv/kernel"], dz6, 2, bb.p6_conv.padding, 1)
    R.check(host(grads["P6_conv/kernel"]), ref["want6"]["P6_conv/kernel"], S_k, f"{name} P6_conv/kernel, no P7")
    R.check(host(d_c5), ref["want6_dx"], S_x, f"{name} d_c5, no P7")
    np.testing.assert_array_equal(host(d6), ref["d_p6"])
    assert bb.backward_extra_levels(tape, None, None) == (None, {})


def test_the_extra_levels_keep_their_refusals():
    """BackboneModel.device_params() still raises for the folded body; the stride-2 layers' default backward still refuses"""
    ref = extra_reference("c5_2x3")
    bb = _loaded_backbone(ref["weights"])
    tape = _tape(bb, dev(ref["c5"]))
    with pytest.raises(NotImplementedError, match="stride 2"):
        bb.p7_conv.backward(tape["g6"], dev(ref["d_p7"]))
    params = {}
    for l in bb.extra_level_layers():
        params.update(l.device_params())
    assert set(params) == set(ref["weights"])
    assert bb.p7_conv.dev.keras_kernel is params["P7_conv/kernel"]
