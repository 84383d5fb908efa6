"""CPU tests of the optimizers: the float64 restatement (tests/optimizer_ref.py) against torch's own optimizers as
independent witnesses, the step at which RectifiedAdam starts to rectify, CyclicLR against hand-computed values, the
argument checks of the ops on host tensors, and the host half of the C entry points."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import optimizer_ref as R

N, STEPS = 1000, 12


def _witness(make, kind, **over):
    """12 steps from zero state in float64: torch's optimizer `make(param)` against the restatement. -> max |difference|"""
    p0 = R.case([N], 3)[0].astype(np.float64)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = make(tp)
    ref = R.Trajectory(kind, [p0], **over)
    worst = 0.
    for step in range(STEPS):
        g = R.gradients([N], 3, step)[0].astype(np.float64)
        tp.grad = torch.tensor(g)
        opt.step()
        ref.step([g])
        worst = max(worst, float(np.abs(ref.p[0] - tp.detach().numpy()).max()))
    return worst


def test_rectified_adam_restatement_equals_torch_radam():
    worst = _witness(lambda p: torch.optim.RAdam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-7), "RectifiedAdam")
    assert worst <= 1e-12, worst


def test_rectified_adam_weight_decay_equals_torch_decoupled_radam():
    worst = _witness(lambda p: torch.optim.RAdam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-7, weight_decay=0.01,
                                                 decoupled_weight_decay=True), "RectifiedAdam", weight_decay=0.01)
    assert worst <= 1e-12, worst


def test_adamw_without_decay_and_epsilon_equals_torch_adam():
    # (torch's AdamW is no witness of the decay: it decays the weight before it steps, the reference after)
    worst = _witness(lambda p: torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=0.), "AdamW", weight_decay=0., epsilon=0.)
    assert worst <= 1e-12, worst


def test_rectification_starts_at_the_sixth_step():
    h = R.hyper("RectifiedAdam")
    s = [R.scalars64("RectifiedAdam", it, 1e-3, h) for it in range(8)]
    assert abs(s[4]["n_sma"] - 4.996) < 1e-3 and abs(s[5]["n_sma"] - 5.994) < 1e-3            # t = 5 and t = 6
    assert [x["rectified"] for x in s] == [0, 0, 0, 0, 0, 1, 1, 1]
    assert all(x["step"] == 1e-3 / (1 - 0.9 ** (it + 1)) for it, x in enumerate(s[:5]))


def test_float32_evaluation_stays_within_the_fp64_bar():
    """What the GPU test's bar rests on: the float32 NumPy evaluation against float64 from the same float32 state, in units of S."""
    sizes = [5000]
    for kind in R.KINDS:
        for wd in (0., 0.01):
            h = R.hyper(kind, weight_decay=wd)
            p = R.case(sizes, 1)[0]
            m, v = np.zeros_like(p), np.zeros_like(p)
            for it in range(12):
                g = R.gradients(sizes, 1, it)[0]
                s = R.scalars64(kind, it, float(np.float32(h["lr"])), h)
                assert R.no_subnormals(R.intermediates32(kind, s, p, g, m, v))
                got, want, S = R.element32(kind, s, p, g, m, v), R.step64(kind, s, p, g, m, v), R.magnitudes(kind, s, p, g, m, v)
                for a, b, mag in zip(got, want, S):
                    assert np.all(np.abs(a - b) <= 1e-6 * mag)
                p, m, v = got


class _Model:
    """Anything with `.optimizer.lr`."""

    def __init__(self):
        self.optimizer = type("Optimizer", (), {"lr": None})()


def _run(clr, n):
    """on_train_begin, then n batches -> the lr in force for batch 0 .. n (n + 1 values)"""
    model = _Model()
    clr.set_model(model)
    clr.on_train_begin()
    lrs = [model.optimizer.lr]
    for _ in range(n):
        clr.on_batch_end(0)
        lrs.append(model.optimizer.lr)
    return lrs


def test_cyclic_lr_modes_against_hand_computed_values():
    from masklab_hip.callbacks import CyclicLR
    base, top, half = 0.001, 0.006, 4
    amp = top - base
    # two full cycles = 4 * step_size iterations; checked at 0, step_size/2, step_size, 2 step_size, 3 step_size (and the end)
    at = [0, 2, 4, 8, 12, 16]
    want = {"triangular": [base, base + amp / 2, top, base, top, base],
            "triangular2": [base, base + amp / 2, top, base, base + amp / 2, base],
            "exp_range": [base, base + amp / 2 * 0.9 ** 2, base + amp * 0.9 ** 4, base, base + amp * 0.9 ** 12, base]}
    for mode, values in want.items():
        lrs = _run(CyclicLR(base, top, step_size=half, mode=mode, gamma=0.9), 16)
        assert len(lrs) == 17
        for i, w in zip(at, values):
            assert math.isclose(lrs[i], w, rel_tol=1e-12), (mode, i, lrs[i], w)
    # halfway down the second cycle of triangular2: half of half the amplitude
    assert math.isclose(_run(CyclicLR(base, top, step_size=half, mode="triangular2"), 14)[14], base + amp / 4, rel_tol=1e-12)
    with pytest.raises(ValueError):
        CyclicLR(mode="sawtooth")


def test_cyclic_lr_custom_scale_fn_in_each_scale_mode():
    from masklab_hip.callbacks import CyclicLR
    base, top, half = 0.01, 0.05, 5
    amp = top - base
    per_cycle = _run(CyclicLR(base, top, step_size=half, scale_fn=lambda c: 1. / c, scale_mode="cycle", mode="ignored"), 15)
    assert math.isclose(per_cycle[5], top, rel_tol=1e-12) and math.isclose(per_cycle[15], base + amp / 2, rel_tol=1e-12)
    assert math.isclose(per_cycle[13], base + amp * 0.6 / 2, rel_tol=1e-12)                  # cycle 2, x = 0.4
    per_iteration = _run(CyclicLR(base, top, step_size=half, scale_fn=lambda i: 1. / (1. + i), scale_mode="iterations"), 15)
    assert math.isclose(per_iteration[5], base + amp / 6, rel_tol=1e-12)
    assert math.isclose(per_iteration[13], base + amp * 0.6 / 14, rel_tol=1e-12)


def test_cyclic_lr_history_and_resume():
    from masklab_hip.callbacks import CyclicLR
    clr = CyclicLR(0.001, 0.006, step_size=4)
    lrs = _run(clr, 6)
    assert clr.history["lr"] == lrs[:6] and clr.history["iterations"] == [1., 2., 3., 4., 5., 6.]
    clr.on_batch_end(0, {"loss": 0.5})
    assert clr.history["loss"] == [0.5] and len(clr.history["lr"]) == 7
    clr.on_train_begin()                                  # a second fit() goes on where the cycle stands
    assert clr.model.optimizer.lr == clr.clr() != clr.base_lr
    clr._reset(new_base_lr=0.002)
    clr.on_train_begin()
    assert clr.model.optimizer.lr == 0.002


def test_optimizer_classes_have_the_reference_arguments_and_config():
    import inspect
    import masklab_hip as M
    from masklab_hip import optimizers as O
    assert O.__all__ == ["AdamW", "RectifiedAdam"]
    assert M.get_custom_objects()["RectifiedAdam"] is O.RectifiedAdam and M.get_custom_objects()["AdamW"] is O.AdamW
    sig = {n: p.default for n, p in inspect.signature(O.RectifiedAdam.__init__).parameters.items() if n not in ("self", "kwargs")}
    assert sig == dict(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0., weight_decay=0.)
    sig = {n: p.default for n, p in inspect.signature(O.AdamW.__init__).parameters.items() if n not in ("self", "kwargs")}
    assert list(sig.items()) == list(dict(lr=0.001, beta_1=0.9, beta_2=0.999, weight_decay=1e-4, epsilon=1e-8, decay=0.).items())
    cfg = O.RectifiedAdam(1e-4).get_config()
    assert set(cfg) == {"lr", "beta_1", "beta_2", "decay", "epsilon", "weight_decay"} and cfg["epsilon"] == 1e-7
    assert cfg["lr"] == float(np.float32(1e-4))
    assert O.AdamW().get_config()["weight_decay"] == 1e-4 and O.AdamW().epsilon == 1e-8
    opt = O.RectifiedAdam()
    opt.lr = 0.5                                          # before any step: held on the host, read back as the float32 it will be
    assert opt.lr == 0.5 and opt.iterations == 0 and opt.get_weights()[0] == 0 and len(opt.get_weights()) == 1


def test_argument_checks_raise_on_the_host():
    from masklab_hip import ops
    from masklab_hip.optimizers import RectifiedAdam
    t = lambda n=8: torch.zeros(n)
    for bad, err in (((t().half(), t(), t(), t()), TypeError), ((t(), t().double(), t(), t()), TypeError),
                     ((t(), t(), t(), t().int()), TypeError), ((t(), None, t(), t()), TypeError),
                     ((t(16)[::2], t(), t(), t()), ValueError), ((t(), t(4), t(), t()), ValueError),
                     ((t(), t(), t(), t(9)), ValueError), ((t(), t(), t()), ValueError)):
        with pytest.raises(err):
            ops.optimizer_check([(t(), t(), t(), t()), bad])
    buf = torch.zeros(32)
    for quad in ((buf[:8], t(), buf[:8], t()), (buf[:8], t(), t(), buf[4:12]), (t(), buf[0:8], buf[7:15], t())):
        with pytest.raises(ValueError, match="overlap"):
            ops.optimizer_check([quad])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                    # all right, but host tensors
        ops.optimizer_check([(buf[0:8], buf[8:16], buf[16:24], buf[24:32]), (t(0), t(0), t(0), t(0))])
    with pytest.raises(ValueError):
        ops.optimizer_step("SGD", [], None, None, None, 0.9, 0.999, 1e-7)
    # through the class: the same exceptions, a missing gradient, and no moments left behind by a refused step
    opt = RectifiedAdam()
    params = {"a": t(), "b": t(4)}
    with pytest.raises(ValueError, match="no gradient"):
        opt.apply_gradients(params, {"a": t()})
    with pytest.raises(ValueError, match="no gradient"):
        opt.apply_gradients(params, {"a": t(), "b": None})
    with pytest.raises(RuntimeError):
        opt.apply_gradients(params, {"a": t(), "b": t(4)})
    with pytest.raises(RuntimeError):
        opt.apply_gradients(params, {"a": t()}, trainable={"a"})
    with pytest.raises(TypeError):
        opt.apply_gradients({"a": t().half()}, {"a": t()})
    with pytest.raises(ValueError):
        opt.apply_gradients(params, {"a": t(), "b": t(5)}, trainable=lambda n: n == "b")
    assert opt.get_weights()[1:] == [] and opt.iterations == 0


def test_scalars_fields_are_the_restatements_and_the_plan_is_a_chunk_prefix_sum():
    from masklab_hip import _lib
    lib = _lib.load()
    assert set(R.FLOAT_FIELDS) | {"rectified", "decays"} == {f[0] for f in _lib.OptScalars._fields_}
    # the host half of the ABI: the chunk prefix sum, tensors without elements included
    sizes = [0, 1, _lib.OPT_CHUNK, _lib.OPT_CHUNK + 1, 0, 3 * _lib.OPT_CHUNK + 7, 0]
    table = (_lib.OptTensor * len(sizes))()
    for e, n in zip(table, sizes):
        e.p = e.g = e.m = e.v = 64 if n else None
        e.n = n
    assert lib.ml_optimizer_plan(table, len(sizes)) == 8 and [e.first_chunk for e in table] == [0, 0, 1, 2, 4, 4, 8]
    assert lib.ml_optimizer_plan(None, 0) == 0
    table[1].n = -1
    assert lib.ml_optimizer_plan(table, len(sizes)) < 0
    table[1].n, table[1].g = 1, None
    assert lib.ml_optimizer_plan(table, len(sizes)) < 0
