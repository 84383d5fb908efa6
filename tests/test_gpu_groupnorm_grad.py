"""GPU tests of GroupNormalization's backward (csrc/groupnorm_grad.hip): ops.groupnorm_chunk_grad / _multi / _stats and the
layer's backward / backward_multi against torch autograd over the float64 restatement of tests/groupnorm_grad_ref.py.
The bar is |got - want| <= 1e-5 * S, S the uncancelled magnitude (groupnorm_grad_ref.scale): a term is about a dozen float32
operations on fp64-summed means, about 1e-6 of S.  Every case and flag combination also holds: two launches give the same
bits; the bits do not depend on what outputs and workspace held; exact zeros where input_relu meets x == 0; in place on dy,
with `stats=` and without the parameter gradients the same bits.  -m gpu.

Largest |got - want| / S measured on the MI355X, per case over its four flag combinations (the bar is 1e-5):
    A 8.9e-08   B 1.1e-07   C 1.1e-07   D 1.3e-07   E 1.4e-07   F 1.2e-07"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import dirty_memory as DM
import groupnorm_grad_ref as R

# (relu, input_relu), gamma given?
COMBOS = {"plain": (False, False, True), "input_relu": (False, True, True), "relu": (True, False, True),
          "no_gamma": (True, True, False)}


@functools.lru_cache(maxsize=None)
def reference(name, combo):
    """-> (inputs, want, S): computed once per (case, combination), shared and left unchanged"""
    relu, input_relu, has_gamma = COMBOS[combo]
    inp = R.inputs(name)
    gamma = inp["gamma"] if has_gamma else None
    args = (inp["x"], inp["dy"], gamma, inp["beta"], inp["groups"], relu, input_relu)
    # (autograd needs a gamma leaf to return dgamma: ones are what gamma=None means)
    want = R.autograd(inp["x"], inp["dy"], inp["gamma"] if has_gamma else np.ones_like(inp["gamma"]), *args[3:])
    return dict(inp, gamma=gamma), want, R.scale(*args)


def _bits(a, b, what):
    DM.assert_same_bits(DM.snapshot(a), DM.snapshot(b), what)


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("name", list(R.CASES))
def test_groupnorm_chunk_grad(name, combo):
    from masklab_hip import ops
    relu, input_relu, has_gamma = COMBOS[combo]
    inp, want, S = reference(name, combo)
    G = inp["groups"]
    if relu:          # before anything runs on the device: no float32 rounding of y can flip a mask bit -- cap on exceptions: 0
        assert R.mask_margin(inp["x"], inp["gamma"], inp["beta"], G) >= R.GUARD
    x, gamma, beta = dev(inp["x"]), (dev(inp["gamma"]) if has_gamma else None), dev(inp["beta"])

    def run(dy=None, **kw):
        return ops.groupnorm_chunk_grad(x, dev(inp["dy"]) if dy is None else dy, gamma, beta, G, R.EPS, relu=relu,
                                        input_relu=input_relu, **kw)

    got = DM.snapshot(run())
    R.check(got, want, S, f"{name} {combo}")                                                     # 1
    assert all(g.dtype == np.float32 for g in got) and got[0].shape == inp["x"].shape
    _bits(run(), got, f"{name} {combo}: two launches")                                           # 2
    with DM.zeroed():                                                                            # 3
        clean = DM.snapshot(run())
    with DM.poisoned():
        dirty = DM.snapshot(run())
    DM.assert_same_bits(dirty, clean, f"{name} {combo}: stale outputs and workspace")
    DM.assert_same_bits(clean, got, f"{name} {combo}: zeroed outputs and workspace")
    assert not any(DM.poison_elements(d).any() for d in dirty)
    if input_relu:                                                                               # 4
        assert (inp["x"] == 0).any() and not got[0][inp["x"] == 0].any()
    dy = dev(inp["dy"])                                                                          # 5
    inplace = run(dy=dy, out=dy)
    assert inplace[0].data_ptr() == dy.data_ptr()
    _bits(inplace, got, f"{name} {combo}: in place on dy")
    stats = ops.groupnorm_chunk_stats(x, G)                                                      # 6
    chunks = inp["x"].astype(np.float64).reshape(inp["x"].shape[0] * G, -1)
    np.testing.assert_allclose(host(stats), np.stack([chunks.sum(1), (chunks ** 2).sum(1)], 1), rtol=1e-6)
    _bits(run(stats=stats), got, f"{name} {combo}: with stats=")
    dx_only = run(want_param_grads=False)                                                        # 7
    assert dx_only[1] is None and dx_only[2] is None
    _bits(dx_only[0], got[0], f"{name} {combo}: without the parameter gradients")
    np.testing.assert_array_equal(host(x), inp["x"])                                             # the input is left alone


def _problem(name, combo="plain", **kw):
    relu, input_relu, has_gamma = COMBOS[combo]
    inp = reference(name, combo)[0]
    return dict(x=dev(inp["x"]), dy=dev(inp["dy"]), gamma=dev(inp["gamma"]) if has_gamma else None, beta=dev(inp["beta"]),
                groups=inp["groups"], eps=R.EPS, relu=relu, input_relu=input_relu, **kw)


def test_groupnorm_chunk_grad_multi_equals_single_launches():
    """B (one-pass) and D (sliced; with relu: its statistics pass rides along) in one launch set.  With A in the list, which
    has no 16-byte accesses, it is still one launch set (scalar accesses beside the others): the same triples either way."""
    from masklab_hip import ops
    picks = [("B", "input_relu"), ("D", "relu"), ("D", "plain"), ("B", "no_gamma")]
    singles = [DM.snapshot(ops.groupnorm_chunk_grad(**_problem(*p))) for p in picks]
    with DM.poisoned():
        multi = ops.groupnorm_chunk_grad_multi([_problem(*p) for p in picks])
    for p, m, s in zip(picks, multi, singles):
        _bits(tuple(m), s, f"multi {p}")
    inplace = [_problem(*p) for p in picks]
    for pr in inplace:
        pr.update(out=pr["dy"], want_param_grads=False)
    for p, pr, m, s in zip(picks, inplace, ops.groupnorm_chunk_grad_multi(inplace), singles):
        assert m[0].data_ptr() == pr["dy"].data_ptr() and m[1] is None and m[2] is None
        _bits(m[0], s[0], f"multi in place {p}")
    picks = [("B", "plain"), ("D", "plain"), ("A", "plain")]
    singles = [DM.snapshot(ops.groupnorm_chunk_grad(**_problem(*p))) for p in picks]
    for p, m, s in zip(picks, ops.groupnorm_chunk_grad_multi([_problem(*p) for p in picks]), singles):
        _bits(tuple(m), s, f"multi with a scalar problem {p}")


def _layers(names, center=True):
    from masklab_hip.normalization import GroupNormalization
    layers, weights = [], {}
    for k, name in enumerate(names):
        inp = reference(name, "plain")[0]
        layer = GroupNormalization(inp["groups"], center=center, name=f"g/gn{k}")
        layer.build((None, None, None, inp["x"].shape[-1]))
        weights.update({f"g/gn{k}/gamma": inp["gamma"], f"g/gn{k}/beta": inp["beta"]})
        layer.load_weights(weights, torch.device("cuda:0"))
        layers.append(layer)
    return layers


@pytest.mark.parametrize("name", ["B", "E"])
def test_layer_backward_equals_the_op(name):
    from masklab_hip import ops
    inp = reference(name, "relu")[0]
    x, dy = dev(inp["x"]), dev(inp["dy"])
    (layer,) = _layers([name])
    want = DM.snapshot(ops.groupnorm_chunk_grad(x, dy, dev(inp["gamma"]), dev(inp["beta"]), inp["groups"], R.EPS, relu=True,
                                                input_relu=True))
    dx, grads = layer.backward(x, dy, fuse_relu=True, input_relu=True)
    assert list(grads) == ["gamma", "beta"]
    _bits((dx, grads["gamma"], grads["beta"]), want, f"{name}: layer.backward")
    dx, grads = layer.backward(x, dy, fuse_relu=True, input_relu=True, inplace=True)
    assert dx.data_ptr() == dy.data_ptr()
    _bits(dx, want[0], f"{name}: layer.backward in place")
    # center=False: no beta in the forward, none returned
    (bare,) = _layers([name], center=False)
    dy = dev(inp["dy"])
    want = DM.snapshot(ops.groupnorm_chunk_grad(x, dy, dev(inp["gamma"]), None, inp["groups"], R.EPS, relu=True))
    dx, grads = bare.backward(x, dy, fuse_relu=True)
    assert list(grads) == ["gamma"]
    _bits((dx, grads["gamma"]), want[:2], f"{name}: layer.backward without beta")


def test_backward_multi_equals_backward_per_layer():
    """[B, D, E] in one launch set; [B, A]: A has no 16-byte accesses and runs scalar ones in the same launch set -- the same results either way"""
    from masklab_hip.normalization import GroupNormalization
    for names in (["B", "D", "E"], ["B", "A"]):
        layers = _layers(names)
        xs = [dev(reference(n, "plain")[0]["x"]) for n in names]
        dys = lambda: [dev(reference(n, "plain")[0]["dy"]) for n in names]
        singles = [DM.snapshot(l.backward(x, dy, input_relu=True)) for l, x, dy in zip(layers, xs, dys())]
        multi = GroupNormalization.backward_multi(layers, xs, dys(), input_relu=True)
        _bits([tuple(m) for m in multi], singles, f"backward_multi {names}")
        grads = dys()
        multi = GroupNormalization.backward_multi(layers, xs, grads, input_relu=True, inplace=True)
        assert all(m[0].data_ptr() == g.data_ptr() for m, g in zip(multi, grads))
        _bits([tuple(m) for m in multi], singles, f"backward_multi in place {names}")


def test_tower_unit_chain_forward_then_backward():
    """What a tower unit needs (Conv3x3 + ReLU -> GroupNormalization): the forward out of place, so that x survives, then
    backward(x, dy, input_relu=True) is the gradient at the conv's pre-activation z, x = relu(z).  Case B."""
    inp = reference("B", "plain")[0]
    z = np.where(inp["x"] > 0, inp["x"], np.float32(-1))            # a pre-activation whose ReLU is x
    x = dev(np.maximum(z, 0))
    np.testing.assert_array_equal(host(x), inp["x"])
    (layer,) = _layers(["B"])
    y = layer(x, inplace=False)
    assert y.data_ptr() != x.data_ptr()
    np.testing.assert_array_equal(host(x), inp["x"])                # the forward left its input alone
    fwd = R.restatement(*(torch.from_numpy(a.astype(np.float64)) for a in (z, inp["gamma"], inp["beta"])), inp["groups"],
                        input_relu=True).numpy()
    np.testing.assert_allclose(host(y), fwd, atol=1e-5)
    dz, grads = layer.backward(x, dev(inp["dy"]), input_relu=True)
    want = R.autograd(z, inp["dy"], inp["gamma"], inp["beta"], inp["groups"], input_relu=True)
    S = R.scale(inp["x"], inp["dy"], inp["gamma"], inp["beta"], inp["groups"], input_relu=True)
    R.check((host(dz), host(grads["gamma"]), host(grads["beta"])), want, S, "chain B")
    assert not host(dz)[z < 0].any()
