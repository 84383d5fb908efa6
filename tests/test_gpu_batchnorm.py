"""GPU tests of BatchNormalization's training forward and backward (csrc/batchnorm.hip): ops.batchnorm_train / _infer / _grad
against the float64 references of tests/batchnorm_ref.py.  The bar is |got - want| <= 1e-5 * S, S the uncancelled magnitude
(batchnorm_ref.scale_forward / scale_backward).  Every case and flag combination also holds: batch_mean / batch_var within
1e-6 of fp64; the moving vectors BIT-equal to the float32 rule applied to the kernel's own batch statistics, and untouched
with update_moving=False; two launches give the same bits; the bits do not depend on what outputs and workspace held; in
place over dy and without the parameter gradients the same bits; the inputs are left alone; inference on the moving
statistics; and sentinels around every output of the three entry points.  -m gpu.

Largest |got - want| / S measured on the MI355X, per case over its six flag combinations, forward and backward (the bar is 1e-5):
    A 6.8e-08   B 1.5e-07   C 1.1e-07   D 1.2e-07   E 1.3e-07   F 1.1e-07   G 8.4e-08   H 1.0e-07
    (inference, all cases: at most 1.5e-07)"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import batchnorm_ref as R
import dirty_memory as DM
from sentinel_dest import SENT, Dest


@functools.lru_cache(maxsize=None)
def reference(name, combo):
    """-> (inputs, float64 y, S of y, float64 gradients, their S): computed once per (case, combination), shared, left unchanged"""
    relu = R.COMBOS[combo][0]
    inp = R.inputs(name, combo)
    C = inp["x"].shape[-1]
    fwd = (inp["x"], inp["gamma"], inp["beta"], inp["residual"])
    bwd = (inp["x"], inp["dy"], inp["gamma"], inp["beta"], inp["residual"], relu)
    # (autograd needs leaves to return dgamma / dbeta: ones and zeros are what None means)
    grads = R.autograd(inp["x"], inp["dy"], np.ones(C) if inp["gamma"] is None else inp["gamma"],
                       np.zeros(C) if inp["beta"] is None else inp["beta"], inp["residual"], relu)
    return inp, R.forward(*fwd, relu=relu), R.scale_forward(*fwd), grads, R.scale_backward(*bwd)


def _bits(a, b, what):
    DM.assert_same_bits(DM.snapshot(a), DM.snapshot(b), what)


def _opt(a):
    return None if a is None else dev(a)


@pytest.mark.parametrize("combo", list(R.COMBOS))
@pytest.mark.parametrize("name", list(R.CASES))
def test_batchnorm_train_and_grad(name, combo):
    from masklab_hip import ops
    relu, has_res, _, _ = R.COMBOS[combo]
    inp, y_want, y_S, g_want, g_S = reference(name, combo)
    mm0, mv0 = R.moving_inputs(name)
    x, gamma, beta, residual = dev(inp["x"]), _opt(inp["gamma"]), _opt(inp["beta"]), _opt(inp["residual"])

    def forward(update=True):
        mm, mv = dev(mm0), dev(mv0)
        out = ops.batchnorm_train(x, gamma, beta, mm, mv, R.MOMENTUM, R.EPS, relu=relu, residual=residual, update_moving=update)
        return out + (mm, mv)

    y, saved, bm, bv, mm, mv = fwd = forward()
    got = DM.snapshot(fwd)
    worst = R.check(got[:1], (y_want,), (y_S,), f"{name} {combo} forward", names=("y",))          # 1
    mean_b, var_b, var_u = R.batch_stats(inp["x"])
    np.testing.assert_allclose(got[2], mean_b, rtol=1e-6)                                          # 2
    np.testing.assert_allclose(got[3], var_u, rtol=1e-6)
    np.testing.assert_allclose(got[1][:, 0], mean_b, rtol=1e-12, atol=1e-13)                       #    saved: fp64
    np.testing.assert_allclose(got[1][:, 1], 1 / np.sqrt(var_b + R.EPS), rtol=1e-9)
    assert got[2].dtype == got[3].dtype == np.float32 and got[1].dtype == np.float64
    DM.assert_same_bits(got[4], R.moving_update(mm0, got[2]), f"{name} {combo}: moving_mean")      # 3
    DM.assert_same_bits(got[5], R.moving_update(mv0, got[3]), f"{name} {combo}: moving_variance")
    still = DM.snapshot(forward(update=False))
    DM.assert_same_bits(still[4:], (mm0, mv0), f"{name} {combo}: update_moving=False")
    DM.assert_same_bits(still[:4], got[:4], f"{name} {combo}: update_moving=False, the rest")

    def backward(dy=None, **kw):
        return ops.batchnorm_grad(x, dev(inp["dy"]) if dy is None else dy, saved, gamma, y=y if relu else None, relu=relu,
                                  want_residual_grad=has_res, **kw)

    grads = DM.snapshot(backward())
    want = (g_want[0], g_want[1] if has_res else None, g_want[2], g_want[3])
    worst = max(worst, R.check(grads, want, g_S, f"{name} {combo} backward"))                      # 4
    print(f"{name} {combo}: max |got - want| / S = {worst:.3g}")
    assert all(g is None or g.dtype == np.float32 for g in grads) and grads[0].shape == inp["x"].shape
    _bits(forward(), got, f"{name} {combo}: two forward launches")                                 # 5
    _bits(backward(), grads, f"{name} {combo}: two backward launches")
    with DM.zeroed():                                                                              # 6
        clean = DM.snapshot((forward(), backward()))
    with DM.poisoned():
        dirty = DM.snapshot((forward(), backward()))
    DM.assert_same_bits(dirty, clean, f"{name} {combo}: stale outputs and workspace")
    DM.assert_same_bits(clean, (got, grads), f"{name} {combo}: zeroed outputs and workspace")
    assert not any(DM.poison_elements(d).any() for part in dirty for d in part if d is not None)
    dy = dev(inp["dy"])                                                                            # 7
    inplace = backward(dy=dy, out=dy)
    assert inplace[0].data_ptr() == dy.data_ptr()
    _bits(inplace, grads, f"{name} {combo}: in place over dy")
    dx_only = backward(want_param_grads=False)
    assert dx_only[2] is None and dx_only[3] is None
    _bits(dx_only[:2], grads[:2], f"{name} {combo}: without the parameter gradients")
    for t, a in ((x, inp["x"]), (gamma, inp["gamma"]), (beta, inp["beta"]), (residual, inp["residual"])):    # 8
        if t is not None:
            np.testing.assert_array_equal(host(t), a)
    # in place over x: the same y
    xc = x.clone()
    y2 = ops.batchnorm_train(xc, gamma, beta, dev(mm0), dev(mv0), R.MOMENTUM, R.EPS, relu=relu, residual=residual, out=xc)[0]
    assert y2.data_ptr() == xc.data_ptr()
    _bits(y2, got[0], f"{name} {combo}: y in place over x")


@pytest.mark.parametrize("combo", list(R.COMBOS))
@pytest.mark.parametrize("name", list(R.CASES))
def test_batchnorm_infer(name, combo):                                                             # 9
    from masklab_hip import ops
    relu, has_res, _, _ = R.COMBOS[combo]
    inp = reference(name, combo)[0]
    mm0, mv0 = R.moving_inputs(name)
    x, gamma, beta, residual = dev(inp["x"]), _opt(inp["gamma"]), _opt(inp["beta"]), _opt(inp["residual"])
    mm, mv = dev(mm0), dev(mv0)
    run = lambda **kw: ops.batchnorm_infer(x, gamma, beta, mm, mv, R.EPS, relu=relu, residual=residual, **kw)
    got = DM.snapshot(run())
    C = inp["x"].shape[-1]
    gam = np.ones(C) if inp["gamma"] is None else inp["gamma"].astype(np.float64)
    bet = np.zeros(C) if inp["beta"] is None else inp["beta"].astype(np.float64)
    scale = gam / np.sqrt(mv0.astype(np.float64) + R.EPS)
    xf = inp["x"].astype(np.float64)
    want = (xf - mm0) / np.sqrt(mv0.astype(np.float64) + R.EPS) * gam + bet
    S = np.abs(xf * scale) + np.abs(bet - mm0 * scale)
    if has_res:
        want, S = want + inp["residual"], S + np.abs(inp["residual"])
    if relu:
        want = np.maximum(want, 0)
    R.check((got,), (want,), (S,), f"{name} {combo} inference", names=("y",))
    with DM.poisoned():
        _bits(run(), got, f"{name} {combo}: inference on stale memory")
    DM.assert_same_bits(DM.snapshot((mm, mv)), (mm0, mv0), f"{name} {combo}: inference leaves the moving statistics alone")
    xc = x.clone()
    ops.batchnorm_infer(xc, gamma, beta, mm, mv, R.EPS, relu=relu, residual=residual, out=xc)
    _bits(xc, got, f"{name} {combo}: inference in place")


def _vec(C, dtype=torch.float32, cols=1):
    return Dest((1, 1, 1), C * cols, C * cols, head=4, tail=8, dtype=dtype)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t)


def _inside(d):
    """the address of a Dest's region"""
    return d.buf.data_ptr() + d.head * d.buf.element_size()


@pytest.mark.parametrize("name", ["A", "D", "E", "H"])
def test_sentinels_around_every_output(name):                                                      # 10
    """The three entry points write into sentinel-filled buffers (y, saved, batch_mean, batch_var; y of inference; dx,
    d_residual, dgamma, dbeta): the bits of the ops, and not an element outside."""
    from masklab_hip import _lib, ops
    lib = _lib.load()
    combo = "residual_relu"
    inp = reference(name, combo)[0]
    B, H, W, C = inp["x"].shape
    n = B * H * W
    mm0, mv0 = R.moving_inputs(name)
    x, gamma, beta, residual, dy = (dev(inp[k]) for k in ("x", "gamma", "beta", "residual", "dy"))
    mm, mv = dev(mm0), dev(mv0)
    y_w, saved_w, bm_w, bv_w = DM.snapshot(ops.batchnorm_train(x, gamma, beta, mm, mv, R.MOMENTUM, R.EPS, relu=True, residual=residual))
    want_moving = DM.snapshot((mm, mv))
    ws = torch.empty(int(lib.ml_batchnorm_workspace_bytes(n, C)), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    maps = lambda: Dest((B, H, W), C, C, head=8, tail=8)
    y_d, saved_d, bm_d, bv_d, mm_d, mv_d = maps(), _vec(C, torch.float64, 2), _vec(C), _vec(C), _vec(C), _vec(C)
    mm_d.buf[mm_d.head:mm_d.head + C] = dev(mm0)
    mv_d.buf[mv_d.head:mv_d.head + C] = dev(mv0)
    _lib.check(lib.ml_batchnorm_train_f32(_p(x), _p(residual), _p(_inside(y_d)), _p(gamma), _p(beta), _p(_inside(mm_d)),
                                          _p(_inside(mv_d)), _p(_inside(saved_d)), _p(_inside(bm_d)), _p(_inside(bv_d)), n, C,
                                          R.EPS, R.MOMENTUM, 1, _p(ws), ws.numel(), stream), "train")
    y = y_d.read()
    DM.assert_same_bits(y, y_w, "y")
    DM.assert_same_bits(saved_d.read().reshape(C, 2), saved_w, "saved")
    DM.assert_same_bits((bm_d.read().reshape(C), bv_d.read().reshape(C)), (bm_w, bv_w), "batch statistics")
    DM.assert_same_bits((mm_d.read().reshape(C), mv_d.read().reshape(C)), want_moving, "moving statistics")
    i_d = maps()
    _lib.check(lib.ml_batchnorm_infer_f32(_p(x), _p(residual), _p(_inside(i_d)), _p(gamma), _p(beta), _p(mm), _p(mv), n, C, R.EPS,
                                          1, _p(ws), ws.numel(), stream), "infer")
    DM.assert_same_bits(i_d.read(), DM.snapshot(ops.batchnorm_infer(x, gamma, beta, mm, mv, R.EPS, relu=True, residual=residual)),
                        "inference")
    yt, saved = dev(y_w), dev(saved_w)
    want = DM.snapshot(ops.batchnorm_grad(x, dy, saved, gamma, y=yt, relu=True, want_residual_grad=True))
    dx_d, dr_d, dg_d, db_d = maps(), maps(), _vec(C), _vec(C)
    _lib.check(lib.ml_batchnorm_grad_f32(_p(x), _p(dy), _p(yt), _p(saved), _p(gamma), _p(_inside(dx_d)), _p(_inside(dr_d)),
                                         _p(_inside(dg_d)), _p(_inside(db_d)), n, C, 1, _p(ws), ws.numel(), stream), "grad")
    DM.assert_same_bits((dx_d.read(), dr_d.read(), dg_d.read().reshape(C), db_d.read().reshape(C)), want, "gradients")
    assert SENT not in y and SENT not in want[0]


def test_d_residual_may_be_dy_when_dx_is_not():
    """The one aliasing of the C entry point that ops.batchnorm_grad does not offer: d_residual written over dy."""
    from masklab_hip import _lib, ops
    lib = _lib.load()
    inp = reference("D", "residual_relu")[0]
    B, H, W, C = inp["x"].shape
    n = B * H * W
    x, gamma, beta, residual = (dev(inp[k]) for k in ("x", "gamma", "beta", "residual"))
    y, saved, _, _ = ops.batchnorm_train(x, gamma, beta, None, None, R.MOMENTUM, R.EPS, relu=True, residual=residual,
                                         update_moving=False)
    want = DM.snapshot(ops.batchnorm_grad(x, dev(inp["dy"]), saved, gamma, y=y, relu=True, want_residual_grad=True))
    dy, dx = dev(inp["dy"]), torch.empty_like(x)
    dgamma, dbeta = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ws = torch.empty(int(lib.ml_batchnorm_workspace_bytes(n, C)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.ml_batchnorm_grad_f32(_p(x), _p(dy), _p(y), _p(saved), _p(gamma), _p(dx), _p(dy), _p(dgamma), _p(dbeta), n, C, 1,
                                         _p(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "grad")
    _bits((dx, dy, dgamma, dbeta), want, "d_residual over dy")
