"""CPU tests of BatchNormalization's training kernels (csrc/batchnorm.hip): the references of tests/batchnorm_ref.py against
torch's own batch norm and autograd, the mask guard's cap, every refusal of the C entry points (fake pointers: a refusal
comes before any launch) and of the ops (host tensors), the slice plan, and the layer's names."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import batchnorm_ref as R

# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("combo", list(R.COMBOS))
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_is_torch_batch_norm_in_training_mode(name, combo):
    relu, has_res, _, _ = R.COMBOS[combo]
    inp = R.inputs(name, combo)
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))
    x = t(inp["x"])
    y, mean, var = R.restatement(x, t(inp["gamma"]), t(inp["beta"]), t(inp["residual"]), relu)
    mm0, mv0 = R.moving_inputs(name)
    rm, rv = t(mm0).clone(), t(mv0).clone()
    want = torch.nn.functional.batch_norm(x.permute(0, 3, 1, 2), rm, rv, t(inp["gamma"]), t(inp["beta"]), training=True,
                                          momentum=1.0 - R.MOMENTUM, eps=R.EPS).permute(0, 2, 3, 1)
    if has_res:
        want = want + t(inp["residual"])
    if relu:
        want = torch.relu(want)
    assert float((y - want).abs().max()) <= 1e-12
    np.testing.assert_allclose(R.forward(inp["x"], inp["gamma"], inp["beta"], inp["residual"], relu), want.numpy(), atol=1e-12)
    # the running statistics: torch's momentum is 1 - momentum, and its running variance is Bessel-corrected too
    mean_b, var_b, var_u = R.batch_stats(inp["x"])
    np.testing.assert_allclose(mean.numpy(), mean_b, atol=1e-12)
    np.testing.assert_allclose(var.numpy(), var_b, rtol=1e-12)
    rule = lambda moving, stat: moving - (moving - stat) * (1.0 - R.MOMENTUM)          # the rule in float64
    np.testing.assert_allclose(rm.numpy(), rule(mm0.astype(np.float64), mean_b), atol=1e-12)
    np.testing.assert_allclose(rv.numpy(), rule(mv0.astype(np.float64), var_u), atol=1e-12)
    # and the float32 rule is that, rounded: within a few float32 ulp of the float64 value
    for moving, stat in ((mm0, mean_b), (mv0, var_u)):
        got = R.moving_update(moving, stat)
        assert got.dtype == np.float32
        np.testing.assert_allclose(got, rule(moving.astype(np.float64), stat), atol=4 * 2.0 ** -24 * (np.abs(moving).max() + 1))


@pytest.mark.parametrize("combo", list(R.COMBOS))
@pytest.mark.parametrize("name", list(R.CASES))
def test_closed_form_equals_autograd_over_the_restatement(name, combo):
    relu = R.COMBOS[combo][0]
    inp = R.inputs(name, combo)
    C = inp["x"].shape[-1]
    args = (inp["x"], inp["dy"], inp["gamma"], inp["beta"], inp["residual"], relu)
    # (autograd needs leaves to return dgamma / dbeta / d_residual: ones, zeros and zeros are what None means)
    want = R.autograd(inp["x"], inp["dy"], np.ones(C) if inp["gamma"] is None else inp["gamma"],
                      np.zeros(C) if inp["beta"] is None else inp["beta"],
                      np.zeros_like(inp["x"]) if inp["residual"] is None else inp["residual"], relu)
    R.check(R.closed_form(*args), want, R.scale_backward(*args), f"{name} {combo}", bar=1e-10)


def test_mask_guard_zeroes_at_most_half_a_percent():
    worst = 0.0
    for name in R.CASES:
        for combo in R.COMBOS:
            for seed in range(2):
                inp = R.inputs(name, combo, seed)                       # (asserts the cap itself)
                assert inp["zeroed"] <= R.GUARD_CAP and (R.COMBOS[combo][0] or inp["zeroed"] == 0)
                worst = max(worst, inp["zeroed"])
    print(f"mask guard: at most {100 * worst:.3f} % of a case's dy zeroed")
    # case F is what it says: channel means far out, where float32 E[x^2] - mean^2 fails
    x = R.inputs("F")["x"]
    mean, var, _ = R.batch_stats(x)
    assert (np.abs(mean) / np.sqrt(var)).max() > 10
    x2 = x.reshape(-1, x.shape[-1])
    naive = (x2 * x2).mean(axis=0, dtype=np.float32) - x2.mean(axis=0, dtype=np.float32) ** 2
    assert (np.abs(naive - var) / var).max() > 1e-4


# ---------------------------------------------------------------- the plan
def test_plan_is_a_function_of_the_geometry_alone():
    from masklab_hip import _lib, ops
    lib = _lib.load()
    for name, (B, H, W, C) in R.CASES.items():
        n = B * H * W
        plan = ops.batchnorm_plan(n, C)
        assert plan == ops.batchnorm_plan(n, C), name
        assert plan["slices"] >= 1 and plan["pixels_per_slice"] >= 1
        assert (plan["slices"] - 1) * plan["pixels_per_slice"] < n <= plan["slices"] * plan["pixels_per_slice"], (name, plan)
        assert plan["bytes"] == lib.ml_batchnorm_workspace_bytes(n, C) > 0
    # the boundary the plan adds, and the cases around it
    assert ops.batchnorm_plan(64, 8)["slices"] == 1 and ops.batchnorm_plan(65, 8)["slices"] == 2
    assert ops.batchnorm_plan(2046, 32)["slices"] > 2                    # case D: several slices, ragged last
    assert 2046 % ops.batchnorm_plan(2046, 32)["pixels_per_slice"] != 0
    # ResNet-50's largest map at 8 x 1024^2
    big = ops.batchnorm_plan(8 * 512 * 512, 64)
    assert big["slices"] * big["pixels_per_slice"] >= 8 * 512 * 512 and big["bytes"] < (8 << 20)
    with pytest.raises(ValueError, match="C "):
        ops.batchnorm_plan(100, 6)
    assert lib.ml_batchnorm_workspace_bytes(100, 6) == -1


# ---------------------------------------------------------------- refusals: the C entry points
N, C = 8, 8
BYTES = N * C * 4
p = lambda k: ctypes.c_void_p(1 << 20 | 4096 * k)                        # aligned, apart, never dereferenced


def _train(lib, **kw):
    a = dict(x=p(1), residual=None, y=p(2), gamma=p(3), beta=p(4), moving_mean=p(5), moving_var=p(6), saved=p(7),
             batch_mean=p(8), batch_var=p(9), N=N, C=C, eps=1e-3, momentum=0.99, relu=0, workspace=p(20), workspace_bytes=1 << 16,
             stream=None)
    a.update(kw)
    return lib.ml_batchnorm_train_f32(*a.values())


def _infer(lib, **kw):
    a = dict(x=p(1), residual=None, y=p(2), gamma=p(3), beta=p(4), moving_mean=p(5), moving_var=p(6), N=N, C=C, eps=1e-3, relu=0,
             workspace=p(20), workspace_bytes=1 << 16, stream=None)
    a.update(kw)
    return lib.ml_batchnorm_infer_f32(*a.values())


def _grad(lib, **kw):
    a = dict(x=p(1), dy=p(2), y=p(3), saved=p(4), gamma=p(5), dx=p(6), d_residual=None, dgamma=p(8), dbeta=p(9), N=N, C=C, relu=0,
             workspace=p(20), workspace_bytes=1 << 16, stream=None)
    a.update(kw)
    return lib.ml_batchnorm_grad_f32(*a.values())


off = lambda k, b: ctypes.c_void_p(p(k).value + b)
REFUSALS = [
    (_train, dict(C=6), b"C (6)"), (_infer, dict(C=6), b"C (6)"), (_grad, dict(C=6), b"C (6)"),
    (_train, dict(N=1), b"N (1"), (_grad, dict(N=1), b"N (1"), (_infer, dict(N=0), b"N (0"),
    (_train, dict(x=None), b"x must"), (_train, dict(x=off(1, 4)), b"x must"), (_train, dict(y=off(2, 8)), b"y must"),
    (_train, dict(residual=off(10, 4)), b"residual must"), (_train, dict(saved=None), b"saved"),
    (_train, dict(batch_mean=None), b"batch_mean"), (_train, dict(batch_var=None), b"batch_var"),
    (_train, dict(moving_var=None), b"moving_mean and moving_var"),
    (_train, dict(y=off(1, 16)), b"y may be x itself"), (_train, dict(residual=p(2)), b"y may not alias residual"),
    (_train, dict(saved=p(1)), b"overlaps an input"), (_train, dict(workspace=p(3)), b"overlaps an input"),
    (_train, dict(batch_var=p(8)), b"two outputs"), (_train, dict(moving_mean=p(2)), b"two outputs"),
    (_train, dict(workspace_bytes=64), b"workspace too small"), (_train, dict(workspace=None), b"workspace must"),
    (_train, dict(momentum=1.5), b"momentum"),
    (_infer, dict(moving_mean=None), b"moving_mean"), (_infer, dict(y=off(1, 16)), b"y may be x itself"),
    (_infer, dict(residual=p(2)), b"y may not alias residual"), (_infer, dict(workspace_bytes=64), b"workspace too small"),
    (_infer, dict(workspace=p(1)), b"overlaps"),
    (_grad, dict(dy=None), b"dy must"), (_grad, dict(dx=off(6, 4)), b"dx must"), (_grad, dict(saved=None), b"saved"),
    (_grad, dict(relu=1, y=None), b"y (the forward's output"), (_grad, dict(d_residual=off(7, 4)), b"d_residual must"),
    (_grad, dict(dx=p(1)), b"overlaps x, y, saved or gamma"), (_grad, dict(relu=1, dx=p(3)), b"overlaps x, y, saved or gamma"),
    (_grad, dict(dx=off(2, 16)), b"dx may be dy itself"), (_grad, dict(d_residual=off(2, 16)), b"d_residual may be dy itself"),
    (_grad, dict(dx=p(2), d_residual=p(2)), b"dx and d_residual may not alias"),
    (_grad, dict(d_residual=p(1)), b"overlaps x, y, saved or gamma"), (_grad, dict(dgamma=p(2)), b"dgamma, dbeta and workspace"),
    (_grad, dict(dbeta=p(8)), b"dgamma, dbeta and workspace"), (_grad, dict(workspace_bytes=64), b"workspace too small"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_c_entry_points_refuse_by_name(k):
    from masklab_hip import _lib
    lib = _lib.load()
    call, kw, text = REFUSALS[k]
    assert call(lib, **kw) != 0, (call.__name__, kw)
    assert text in lib.ml_last_error(), (call.__name__, kw, lib.ml_last_error())


# ---------------------------------------------------------------- refusals: the ops
def test_ops_check_their_arguments_before_any_device_work():
    from masklab_hip import ops
    x, dy = torch.zeros(2, 3, 5, 8), torch.zeros(2, 3, 5, 8)
    v = lambda n=8: torch.ones(n)
    saved = torch.zeros(8, 2, dtype=torch.float64)
    train = dict(x=x, gamma=v(), beta=v(), moving_mean=v(), moving_var=v(), momentum=0.99, eps=1e-3)
    infer = dict(x=x, gamma=v(), beta=v(), moving_mean=v(), moving_var=v(), eps=1e-3)
    grad = dict(x=x, dy=dy, saved=saved, gamma=v())
    half = x.half()
    for fn, ok, bads in (
        (ops.batchnorm_train, train, [
            (dict(x=half), TypeError), (dict(residual=half), TypeError), (dict(x=torch.zeros(2, 3, 5, 6)), ValueError),
            (dict(x=torch.zeros(1, 1, 1, 8)), ValueError), (dict(residual=torch.zeros(2, 3, 5, 4)), ValueError),
            (dict(gamma=v(4)), ValueError), (dict(beta=v().double()), ValueError), (dict(moving_mean=v(4)), ValueError),
            (dict(moving_var=None), ValueError), (dict(out=torch.zeros(2, 3, 5, 4)), ValueError), (dict(momentum=2.0), ValueError),
            (dict(x=3), ValueError), (dict(), RuntimeError)]),
        (ops.batchnorm_infer, infer, [
            (dict(x=half), TypeError), (dict(x=torch.zeros(2, 3, 5, 6)), ValueError), (dict(moving_mean=None), ValueError),
            (dict(moving_var=v(4)), ValueError), (dict(out=half), ValueError), (dict(), RuntimeError)]),
        (ops.batchnorm_grad, grad, [
            (dict(dy=dy.half()), TypeError), (dict(x=half), TypeError), (dict(dy=torch.zeros(2, 3, 5, 4)), ValueError),
            (dict(x=torch.zeros(1, 1, 1, 8), dy=torch.zeros(1, 1, 1, 8)), ValueError), (dict(saved=torch.zeros(8, 2)), ValueError),
            (dict(saved=torch.zeros(4, 2, dtype=torch.float64)), ValueError), (dict(gamma=v(4)), ValueError),
            (dict(relu=True), ValueError), (dict(relu=True, y=half), TypeError), (dict(out=torch.zeros(2, 3, 5, 4)), ValueError),
            (dict(), RuntimeError)])):
        for bad, err in bads:
            with pytest.raises(err):
                fn(**{**ok, **bad})
    with pytest.raises(ValueError, match="N \\(1 pixels"):
        ops.batchnorm_train(**{**train, "x": torch.zeros(1, 1, 1, 8)})
    with pytest.raises(ValueError, match="C \\(6\\)"):
        ops.batchnorm_train(**{**train, "x": torch.zeros(2, 3, 5, 6)})
    ops.batchnorm_plan(30, 8)                                            # host only: no device needed


# ---------------------------------------------------------------- the layer's names
def test_layer_has_keras_names_defaults_and_config_keys():
    from masklab_hip import ops
    from masklab_hip.normalization import BatchNormalization
    layer = BatchNormalization(name="stage/bn")
    assert (layer.axis, layer.momentum, layer.epsilon, layer.center, layer.scale) == (-1, 0.99, 1e-3, True, True)
    layer.build((None, None, None, 16))
    assert list(layer.weight_specs()) == [f"stage/bn/{k}" for k in ("gamma", "beta", "moving_mean", "moving_variance")]
    assert all(s.shape == (16,) for s in layer.weight_specs().values())
    keras_keys = {"name", "trainable", "axis", "momentum", "epsilon", "center", "scale", "beta_initializer", "gamma_initializer",
                  "moving_mean_initializer", "moving_variance_initializer", "beta_regularizer", "gamma_regularizer",
                  "beta_constraint", "gamma_constraint"}
    assert set(layer.get_config()) == keras_keys
    again = BatchNormalization.from_config(layer.get_config())
    assert again.get_config() == layer.get_config()
    bare = BatchNormalization(center=False, scale=False, name="bare")
    bare.build((None, None, None, 8))
    assert list(bare.weight_specs()) == ["bare/moving_mean", "bare/moving_variance"]
    for axis in (1, 0, 2):
        with pytest.raises(NotImplementedError):
            BatchNormalization(axis=axis)
    BatchNormalization(axis=3)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        layer.device_params()
    with pytest.raises(RuntimeError, match="no weights loaded"):
        layer.state()
    # loaded on the host device the keys are there (the kernels never run here)
    from masklab_hip.keras_like import init_weights
    weights = init_weights(layer.weight_specs(), 1)
    layer.load_weights(weights, torch.device("cpu"))
    assert list(layer.device_params()) == ["stage/bn/gamma", "stage/bn/beta"]
    assert list(layer.state()) == ["stage/bn/moving_mean", "stage/bn/moving_variance"]
    host = layer.get_weights_host()
    assert list(host) == list(layer.weight_specs()) and all(np.array_equal(host[k], weights[k]) for k in weights)
    bare.load_weights(init_weights(bare.weight_specs(), 1), torch.device("cpu"))
    assert bare.device_params() == {} and list(bare.state()) == ["bare/moving_mean", "bare/moving_variance"]
    with pytest.raises(RuntimeError):                                   # host tensors: no CPU fallback
        layer(torch.zeros(2, 3, 5, 16))
    for math in ("f16", "f16s"):
        ops.set_conv_math(math)
        try:
            with pytest.raises(NotImplementedError, match="float32 only"):
                layer.device_params()
            with pytest.raises(NotImplementedError, match="float32 only"):
                layer(torch.zeros(2, 3, 5, 16), training=True)
            with pytest.raises(NotImplementedError, match="float32 only"):
                layer.call_with_tape(torch.zeros(2, 3, 5, 16))
        finally:
            ops.set_conv_math("f32")
