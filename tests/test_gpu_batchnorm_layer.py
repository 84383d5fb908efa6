"""GPU tests of masklab_hip.normalization.BatchNormalization: the layer's call / call_with_tape / backward are the ops' bits;
two training calls move the statistics twice; a forward + backward captured in one graph replays with the bits of eager
steps, moving statistics included; and a ResNet basic unit built from existing parts (Conv2D -> BN + ReLU -> Conv2D -> BN +
input + ReLU) has every gradient within 4 x the error of a float32 CPU restatement against float64 (the project's bar for
composites) and trains: the loss is lower after 10 AdamW steps.  -m gpu.

Largest error relative to max |want| per tensor of the basic unit, measured on the MI355X, float32 restatement / device:
    dx 3.0e-07 / 2.9e-07   bn1/gamma 6.0e-07 / 4.8e-07   bn1/beta 5.4e-07 / 5.6e-07   bn2/gamma 1.5e-07 / 1.3e-07
    bn2/beta 1.6e-07 / 1.1e-07   conv1/kernel 3.6e-07 / 6.1e-07   conv2/kernel 3.9e-07 / 4.3e-07
    loss 7040.67 -> 5776.31 after 10 AdamW(1e-3) steps"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import batchnorm_ref as R
import dirty_memory as DM


def _bits(a, b, what):
    DM.assert_same_bits(DM.snapshot(a), DM.snapshot(b), what)


def _layer(name, combo, layer_name="bn"):
    """a loaded layer for the case's channel count, the combination's scale / center -> (layer, inputs, its weights)"""
    from masklab_hip.normalization import BatchNormalization
    _, _, has_scale, has_center = R.COMBOS[combo]
    inp = R.inputs(name, combo)
    C = inp["x"].shape[-1]
    mm0, mv0 = R.moving_inputs(name)
    layer = BatchNormalization(momentum=R.MOMENTUM, epsilon=R.EPS, center=has_center, scale=has_scale, name=layer_name)
    layer.build((None, None, None, C))
    weights = {f"{layer_name}/moving_mean": mm0, f"{layer_name}/moving_variance": mv0}
    if has_scale:
        weights[f"{layer_name}/gamma"] = inp["gamma"]
    if has_center:
        weights[f"{layer_name}/beta"] = inp["beta"]
    layer.load_weights(weights, torch.device("cuda:0"))
    return layer, inp, weights


@pytest.mark.parametrize("name,combo", [("B", "plain"), ("D", "residual_relu"), ("E", "no_scale"), ("C", "no_center")])
def test_layer_equals_the_ops(name, combo):
    from masklab_hip import ops
    relu, has_res, has_scale, has_center = R.COMBOS[combo]
    layer, inp, weights = _layer(name, combo)
    mm0, mv0 = weights["bn/moving_mean"], weights["bn/moving_variance"]
    x, dy = dev(inp["x"]), dev(inp["dy"])
    gamma, beta = (None if inp[k] is None else dev(inp[k]) for k in ("gamma", "beta"))
    residual = dev(inp["residual"]) if has_res else None
    mm, mv = dev(mm0), dev(mv0)
    y_w, saved, bm, bv = ops.batchnorm_train(x, gamma, beta, mm, mv, R.MOMENTUM, R.EPS, relu=relu, residual=residual)
    want_g = DM.snapshot(ops.batchnorm_grad(x, dy, saved, gamma, y=y_w if relu else None, relu=relu, want_residual_grad=has_res))
    y, tape = layer.call_with_tape(x, fuse_relu=relu, residual=residual)
    _bits(y, y_w, f"{name} {combo}: call_with_tape")
    _bits(tuple(layer.state().values()), (mm, mv), f"{name} {combo}: the layer's moving statistics after one step")
    assert list(layer.state()) == ["bn/moving_mean", "bn/moving_variance"]
    dx, dres, grads = layer.backward(tape, dy)
    assert list(grads) == [k for k, has in (("gamma", has_scale), ("beta", has_center)) if has]
    assert (dres is not None) == has_res
    _bits((dx, dres), want_g[:2], f"{name} {combo}: backward")
    for k, w in (("gamma", want_g[2]), ("beta", want_g[3])):
        if k in grads:
            _bits(grads[k], w, f"{name} {combo}: d{k}")
    # the weights the kernels read are the optimizer's: device_params() hands out the layer's own tensors
    params = layer.device_params()
    assert list(params) == [f"bn/{k}" for k in grads]
    assert all(params[f"bn/{k}"].data_ptr() == getattr(layer, k).data_ptr() for k in grads)
    into = {}
    layer.name_grads(grads, into)
    assert list(into) == list(params)
    # in place over the gradient; need_residual_grad asked for without a residual in the forward
    dyc = dy.clone()
    dx2, _, _ = layer.backward(tape, dyc, inplace=True, need_residual_grad=False)
    assert dx2.data_ptr() == dyc.data_ptr()
    _bits(dx2, want_g[0], f"{name} {combo}: backward in place")
    # call(training=True) is call_with_tape's forward: the same bits from the same moving statistics
    layer.load_weights(weights, torch.device("cuda:0"))
    _bits(layer(x, training=True, fuse_relu=relu, residual=residual), y_w, f"{name} {combo}: call(training=True)")
    _bits(tuple(layer.state().values()), (mm, mv), f"{name} {combo}: moving statistics after call(training=True)")
    # inference reads the moving statistics where they are
    want_i = ops.batchnorm_infer(x, gamma, beta, mm, mv, R.EPS, relu=relu, residual=residual)
    _bits(layer(x, fuse_relu=relu, residual=residual), want_i, f"{name} {combo}: call(training=False)")
    xc = x.clone()
    assert layer(xc, fuse_relu=relu, residual=residual, inplace=True).data_ptr() == xc.data_ptr()
    _bits(xc, want_i, f"{name} {combo}: call(training=False, inplace=True)")
    got = layer.get_weights_host()
    assert list(got) == list(layer.weight_specs())
    DM.assert_same_bits((got["bn/moving_mean"], got["bn/moving_variance"]), DM.snapshot((mm, mv)), "get_weights_host")


def test_two_training_calls_move_the_statistics_twice():
    layer, inp, weights = _layer("D", "plain")
    x = dev(inp["x"])
    mean_b, _, var_u = R.batch_stats(inp["x"])
    mm, mv = weights["bn/moving_mean"], weights["bn/moving_variance"]
    for step in (1, 2):
        y, tape = layer.call_with_tape(x)
        mm, mv = R.moving_update(mm, host(tape["batch_mean"])), R.moving_update(mv, host(tape["batch_var"]))
        got = layer.get_weights_host()
        DM.assert_same_bits((got["bn/moving_mean"], got["bn/moving_variance"]), (mm, mv), f"step {step}")
    # two steps of the rule in float64, from the float64 statistics
    f = 1.0 - R.MOMENTUM
    want = weights["bn/moving_mean"].astype(np.float64)
    for _ in range(2):
        want = want - (want - mean_b) * f
    np.testing.assert_allclose(mm, want, atol=1e-6)
    assert np.abs(mm - weights["bn/moving_mean"]).max() > 1e-3
    # inference now normalises with the moved statistics
    y = host(layer(x))
    scale = inp["gamma"].astype(np.float64) / np.sqrt(mv.astype(np.float64) + R.EPS)
    np.testing.assert_allclose(y, (inp["x"].astype(np.float64) - mm) * scale + inp["beta"], atol=1e-4)


def test_captured_forward_and_backward_replay_with_the_bits_of_eager_steps():
    layer, inp, weights = _layer("D", "residual_relu")
    x, residual, dy = dev(inp["x"]), dev(inp["residual"]), dev(inp["dy"])
    mm0, mv0 = dev(weights["bn/moving_mean"]), dev(weights["bn/moving_variance"])

    def reset():
        layer.moving_mean.copy_(mm0)
        layer.moving_variance.copy_(mv0)
        torch.cuda.synchronize()

    def step():
        y, tape = layer.call_with_tape(x, fuse_relu=True, residual=residual)
        dx, dres, grads = layer.backward(tape, dy)
        return y, dx, dres, grads["gamma"], grads["beta"], tape["batch_mean"], tape["batch_var"]

    state = lambda: (layer.moving_mean, layer.moving_variance)
    reset()
    eager = [DM.snapshot((step(), state())) for _ in range(2)]
    assert not np.array_equal(eager[0][1][0], eager[1][1][0])
    reset()
    step()                                                    # warm-up: the workspace exists before the capture
    reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        DM.assert_same_bits(DM.snapshot((outs, state())), eager[k], f"replay {k + 1}")


# ---------------------------------------------------------------- a ResNet basic unit from existing parts
UNIT_SHAPE = (2, 12, 10, 16)
KINK = 1e-4                        # no pre-activation nearer to the ReLUs' kinks: float32 and float64 mask the same elements


def _unit_layers():
    from masklab_hip import keras_like as K
    from masklab_hip.normalization import BatchNormalization
    K.clear_session()
    layers = [K.Conv2D(16, 3, padding="same", use_bias=False, name="unit/conv1"),
              BatchNormalization(momentum=R.MOMENTUM, epsilon=R.EPS, name="unit/bn1"),
              K.Conv2D(16, 3, padding="same", use_bias=False, name="unit/conv2"),
              BatchNormalization(momentum=R.MOMENTUM, epsilon=R.EPS, name="unit/bn2")]
    specs = {}
    for layer in layers:
        layer.build(UNIT_SHAPE)
        specs.update(layer.weight_specs())
    return layers, specs


def _unit_restatement(x, target, w, dtype):
    """The unit in torch on the CPU in `dtype`: -> (loss, {name: gradient}, dx, the smallest |pre-activation|)"""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
    names = [n for n in w if not n.split("/")[-1].startswith("moving")]
    leaves = {n: t(w[n]) for n in names}
    xl = t(x)
    conv = lambda a, k: torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    z1 = R.restatement(conv(xl, leaves["unit/conv1/kernel"]), leaves["unit/bn1/gamma"], leaves["unit/bn1/beta"])[0]
    z2 = R.restatement(conv(torch.relu(z1), leaves["unit/conv2/kernel"]), leaves["unit/bn2/gamma"], leaves["unit/bn2/beta"], xl)[0]
    loss = ((torch.relu(z2) - torch.from_numpy(target).to(dtype)) ** 2).sum()
    loss.backward()
    kink = min(float(z1.detach().abs().min()), float(z2.detach().abs().min()))
    return float(loss.detach()), {n: leaves[n].grad.numpy() for n in names}, xl.grad.numpy(), kink


@functools.lru_cache(maxsize=None)
def unit_reference():
    from masklab_hip import keras_like as K
    _, specs = _unit_layers()
    weights = K.init_weights(specs, 2)
    rng = np.random.default_rng(12)                       # (the seed: see KINK)
    x = rng.normal(0, 1, UNIT_SHAPE).astype(np.float32)
    target = rng.normal(0.5, 1, UNIT_SHAPE).astype(np.float32)
    return weights, x, target, _unit_restatement(x, target, weights, torch.float64), _unit_restatement(x, target, weights, torch.float32)


def _unit_step(layers, x, target):
    """forward with tapes, the loss, backward -> (loss tensor, {full name: gradient}, dx)"""
    conv1, bn1, conv2, bn2 = layers
    c1 = conv1(x)
    a1, tape1 = bn1.call_with_tape(c1, fuse_relu=True)
    c2 = conv2(a1)
    out, tape2 = bn2.call_with_tape(c2, fuse_relu=True, residual=x)
    diff = out - target
    loss = (diff * diff).sum()
    grads = {}
    dc2, dres, g = bn2.backward(tape2, 2 * diff, inplace=True)
    bn2.name_grads(g, grads)
    da1, g = conv2.backward(a1, dc2)
    conv2.name_grads(g, grads)
    dc1, _, g = bn1.backward(tape1, da1, inplace=True)
    bn1.name_grads(g, grads)
    dx, g = conv1.backward(x, dc1, add=dres)
    conv1.name_grads(g, grads)
    return loss, grads, dx


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def test_resnet_basic_unit_gradients_and_training():
    from masklab_hip import optimizers
    weights, x_h, target_h, want, f32 = unit_reference()
    assert min(want[3], f32[3]) >= KINK, f"a pre-activation lies {min(want[3], f32[3]):.3g} from a ReLU's kink: choose another seed"
    layers, _ = _unit_layers()
    for layer in layers:
        layer.load_weights(weights, torch.device("cuda:0"))
    x, target = dev(x_h), dev(target_h)
    loss, grads, dx = _unit_step(layers, x, target)
    assert abs(float(loss) - want[0]) <= 1e-5 * want[0]
    assert sorted(grads) == sorted(want[1])
    for name, g, w64, w32 in [("dx", dx, want[2], f32[2])] + [(n, grads[n], want[1][n], f32[1][n]) for n in sorted(grads)]:
        assert tuple(g.shape) == w64.shape and g.dtype == torch.float32, name
        e32, edev = _rel(w32, w64), _rel(host(g), w64)
        print(f"{name}: float32 restatement {e32:.3g}, device {edev:.3g}")
        assert edev <= 4 * e32, f"{name}: device {edev:.3g} against 4 x {e32:.3g}"
    np.testing.assert_array_equal(host(x), x_h)
    # 10 AdamW steps through apply_gradients on the layers' own tensors: the loss falls
    for layer in layers:
        layer.load_weights(weights, torch.device("cuda:0"))
    params = {}
    for layer in layers:
        params.update(layer.device_params())
    assert sorted(params) == sorted(grads)
    opt = optimizers.AdamW(1e-3)
    first = float(_unit_step(layers, x, target)[0])
    for _ in range(10):
        _, grads, _ = _unit_step(layers, x, target)
        opt.apply_gradients(params, grads)
        for layer in (layers[0], layers[2]):
            layer.repack()
    last = float(_unit_step(layers, x, target)[0])
    print(f"basic unit: loss {first:.6g} -> {last:.6g} after 10 AdamW(1e-3) steps")
    assert last < first
