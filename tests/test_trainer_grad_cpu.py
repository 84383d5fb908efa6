"""CPU tests that pin the oracle of the loss gradients (tests/trainer_grad_ref.py) before any GPU run: the float64 torch
restatement's forward equals tests/trainer_ref.py, the float32 closed forms equal its autograd under the bar the GPU tests
use, a five-point central difference in float64 agrees with autograd (which guards the restatement itself), and the new
ops refuse what their forward twins refuse.  No GPU involved."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import trainer_cases as CASES
import trainer_grad_ref as G
import trainer_ref as REF

F32, F64 = np.float32, np.float64
C = CASES.NUM_CLASSES


def _upstream(B, seed):
    up = np.random.default_rng(seed).uniform(0.2, 2.0, B).astype(F32)
    up[B // 2] = 0
    return up


def _forward_equal(got, want, name):
    print(f"{name}: restatement {got} trainer_ref {want}")
    np.testing.assert_allclose(got, np.asarray(want, F64), rtol=1e-6, atol=0, err_msg=name)


def _difference_agrees(fn, pred, upstream, grad, eligible, name, n=50, seed=0):
    """`n` sampled elements among `eligible` (non-zero gradient, five-point stencil clear of every kink) to 1e-6 relative"""
    where = np.flatnonzero(eligible & (grad != 0))
    assert len(where) >= n, (name, len(where))
    where = np.random.default_rng(seed).choice(where, n, replace=False)
    fd = G.central_difference(fn, pred, upstream, where)
    rel = np.abs(fd - grad.reshape(-1)[where]) / np.abs(grad.reshape(-1)[where])
    print(f"{name}: five-point difference against autograd on {n} elements, max rel {rel.max():.3g}")
    assert rel.max() <= 1e-6, name


@pytest.fixture(scope="module")
def boxes():
    gt, pr = CASES.boxes_small()
    _, cls_true, loc_true, mask = REF.assign_boxes(gt, pr, C)
    cls_pred, _, exist = CASES.predictions(gt, len(pr), 3)
    _, loc_pred, _ = CASES.predictions(gt, len(pr), G.BOX_SEED)
    return cls_true, loc_true, mask, cls_pred, loc_pred, exist


# ----------------------------------------------------------------------------- ClassLoss
@pytest.mark.parametrize("weight,alpha,gamma", [(300., .25, 2.), (1., .5, 1.5)])
def test_class_loss_restatement_closed_form_and_difference(boxes, weight, alpha, gamma):
    cls_true, _, mask, cls_pred, _, exist = boxes
    fn = lambda x: G.class_loss(cls_true, x, mask, exist, weight, alpha, gamma)
    loss, _ = G.autograd(fn, cls_pred)
    _forward_equal(loss, REF.class_loss(cls_true, cls_pred, mask, exist, weight, alpha, gamma), "class_loss")
    for up in (G.default_upstream(3), _upstream(3, 1)):
        _, want = G.autograd(fn, cls_pred, up)
        assert not want[0, :3].reshape(-1)[[0, 1, 3, 4]].any() and want[0, 0, 2] != 0          # outside the clip: 0, 1, 1e-9, 1 - 1e-9
        assert np.isfinite(want).all() and not want[mask.reshape(3, -1) == -1].any() and not want[0, :, 1].any()
        G.check(G.class_loss_grad(cls_true, cls_pred, mask, exist, weight, alpha, gamma, up), want, name="class closed form")
        sig = G.class_loss_grad(cls_true, cls_pred, mask, exist, weight, alpha, gamma, up, through_sigmoid=True)
        G.check(sig, want * (cls_pred.astype(F64) * (1 - cls_pred.astype(F64))), name="class closed form through sigmoid")
    _difference_agrees(fn, cls_pred, up, want, (cls_pred > 0.1) & (cls_pred < 0.9), "class_loss")


def test_clip_passes_at_equality_and_stops_outside():
    eps, hi = F32(1e-7), F32(1) - F32(1e-7)
    pred = np.array([[[eps, hi, np.nextafter(eps, F32(0)), np.nextafter(hi, F32(1)), F32(.25)]]], F32)
    true, mask, exist = np.array([[[1, 0, 1, 0, 1]]], F32), np.zeros((1, 1, 1), F32), np.ones((1, 5), F32)
    _, want = G.autograd(lambda x: G.class_loss(true, x, mask, exist, 1., .25, 2.), pred)
    assert want[0, 0, 0] != 0 and want[0, 0, 1] != 0 and want[0, 0, 2] == 0 and want[0, 0, 3] == 0
    G.check(G.class_loss_grad(true, pred, mask, exist, 1., .25, 2., G.default_upstream(1)), want, name="clip")


# ----------------------------------------------------------------------------- BoxLoss
def box_guard(loc_true, loc_pred, mask, betas):
    """No positive coordinate within 1e-4 of the branch |d| = 1.5 beta, in float64, for every beta in use."""
    pos = np.asarray(mask).reshape(mask.shape[0], -1) == 0
    d = np.abs(np.asarray(loc_true, F64) - np.asarray(loc_pred, F64))[pos]
    for beta in betas:
        near = np.abs(d - 1.5 * np.broadcast_to(np.asarray(beta, F64), (4,)))
        assert near.min() > CASES.GUARD, (beta, float(near.min()))


def test_box_loss_restatement_closed_form_and_difference(boxes):
    _, loc_true, mask, _, loc_pred, _ = boxes
    assert (mask[2] == 1).all() and (mask == 0).sum() > 50
    ref, mine = REF.BoxLoss(2., .9, .11, True), G.BoxLoss(2., .9, .11, True)
    up = _upstream(3, 2)
    betas = []
    for call in range(3):
        want_loss = ref(loc_true, loc_pred, mask)
        beta = np.clip(ref.moving_mean - ref.moving_var, F32(1e-3), F32(.11))
        betas.append(beta)
        loss, want = G.autograd(lambda x: mine(loc_true, x, mask), loc_pred, up)
        _forward_equal(loss, want_loss, f"box_loss call {call}")
        np.testing.assert_allclose(mine.last_beta.numpy(), beta, rtol=1e-6)
        np.testing.assert_allclose(mine.moving_mean.numpy(), ref.moving_mean, rtol=1e-6)
        _, fixed = G.autograd(lambda x: G.box_loss(loc_true, x, mask, 2., beta), loc_pred, up)  # beta is a constant: the same
        np.testing.assert_allclose(want, fixed, rtol=1e-6, atol=0)
        assert not want[2].any() and not want[mask.reshape(3, -1) != 0].any()
        G.check(G.box_loss_grad(loc_true, loc_pred, mask, 2., beta, up), fixed, name=f"box closed form call {call}")
    assert np.all(betas[0] != betas[2])
    box_guard(loc_true, loc_pred, mask, betas + [.11])
    fn = lambda x: G.box_loss(loc_true, x, mask, 1., .11)
    loss, want = G.autograd(fn, loc_pred)
    _forward_equal(loss, REF.BoxLoss(1., .9, .11, False)(loc_true, loc_pred, mask), "box_loss fixed beta")
    G.check(G.box_loss_grad(loc_true, loc_pred, mask, 1., .11, G.default_upstream(3)), want, name="box closed form fixed beta")
    d = np.abs(loc_true.astype(F64) - loc_pred)
    clear = (np.abs(d - .165) > .01) & (d > .01)                    # the stencil reaches 2e-3 to either side
    _difference_agrees(fn, loc_pred, G.default_upstream(3), want, clear, "box_loss", n=40)
    assert ((d < .165) & (want != 0)).sum() >= 5                     # the quadratic branch is among the positives


# ----------------------------------------------------------------------------- MaskLoss
@pytest.mark.parametrize("smoothing", [0., .1])
def test_mask_loss_restatement_closed_form_and_difference(smoothing):
    roi, gt, masks = CASES.masks_int8()
    target, _, matched = REF.assign_masks(roi, gt, masks, (28, 28), C)
    assert not matched.all()
    pred = CASES.mask_predictions(roi, 5)
    fn = lambda x: G.mask_loss(target, x, 1., smoothing)
    loss, _ = G.autograd(fn, pred)
    _forward_equal(loss, REF.mask_loss(target, pred, 1., smoothing), "mask_loss")
    for up in (G.default_upstream(2), np.array([1.5, 0], F32)):
        _, want = G.autograd(fn, pred, up)
        got, S = G.mask_loss_grad(target, pred, 1., smoothing, up, with_scale=True)
        assert (want != 0).reshape(2, 6, -1).any(axis=2).tolist() == (matched & (up != 0)[:, None]).tolist()
        G.check(got, want, S, name="mask closed form")
        sig, S = G.mask_loss_grad(target, pred, 1., smoothing, up, through_sigmoid=True, with_scale=True)
        G.check(sig, want * (pred.astype(F64) * (1 - pred.astype(F64))), S, name="mask closed form through sigmoid")
    _difference_agrees(fn, pred, G.default_upstream(2), G.autograd(fn, pred)[1], (pred > 0.1) & (pred < 0.9), "mask_loss")


# ----------------------------------------------------------------------------- SegLoss
@pytest.mark.parametrize("smoothing", [0., .1])
def test_seg_loss_restatement_closed_form_and_difference(smoothing):
    gt, exist, _ = CASES.seg_case((37, 53), (8, 12), "uint8")
    true, _ = REF.assign_seg(gt, (8, 12))
    pred = CASES.seg_predictions((8, 12), 9)
    fn = lambda x: G.seg_loss(true, x, exist, .5, smoothing)
    loss, _ = G.autograd(fn, pred)
    _forward_equal(loss, REF.seg_loss(true, pred, exist, .5, smoothing), "seg_loss")
    for up in (G.default_upstream(2), np.array([0, .7], F32)):
        _, want = G.autograd(fn, pred, up)
        got, S = G.seg_loss_grad(true, pred, exist, .5, smoothing, up, with_scale=True)
        assert not want[1, :, :, 0].any()
        G.check(got, want, S, name="seg closed form")
        sig, S = G.seg_loss_grad(true, pred, exist, .5, smoothing, up, through_sigmoid=True, with_scale=True)
        G.check(sig, want * (pred.astype(F64) * (1 - pred.astype(F64))), S, name="seg closed form through sigmoid")
    _difference_agrees(fn, pred, up, want, (pred > 0.1) & (pred < 0.9), "seg_loss")


# ----------------------------------------------------------------------------- the ops' checks
def test_grad_ops_refuse_what_their_forward_twins_refuse():
    from masklab_hip import ops
    f = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    cases = [
        (ops.class_loss, ops.class_loss_grad, [(f(2, 7, 5), f(2, 7, 5), f(2, 7, 1), f(2, 5), 1., .25, 2.),        # host tensors
                                               (f(2, 7, 5), f(2, 7, 5, dtype=torch.float64), f(2, 7, 1), f(2, 5), 1., .25, 2.),
                                               (f(2, 7, 5), f(2, 6, 5), f(2, 7, 1), f(2, 5), 1., .25, 2.),
                                               (None, f(2, 7, 5), f(2, 7, 1), f(2, 5), 1., .25, 2.)]),
        (ops.box_loss, ops.box_loss_grad, [(f(2, 7, 4), f(2, 7, 4), f(2, 7, 1), 1., .9, .11, False),
                                           (f(2, 7, 4), f(2, 7, 4, dtype=torch.float16), f(2, 7, 1), 1., .9, .11, True, f(8)),
                                           (f(2, 7, 3), f(2, 7, 3), f(2, 7, 1), 1., .9, .11, False)]),
        (ops.mask_loss, ops.mask_loss_grad, [(i32(2, 3, 4, 4), f(2, 3, 4, 4, 5), 1., 0.),
                                             (f(2, 3, 4, 4), f(2, 3, 4, 4, 5), 1., 0.),
                                             (i32(2, 3, 4, 4), f(2, 3, 4, 5), 1., 0.)]),
        (ops.seg_loss, ops.seg_loss_grad, [(f(2, 4, 4, 3), f(2, 4, 4, 3), f(2, 3), 1., 0.),
                                           (f(2, 4, 4, 3), f(2, 4, 4, 3), f(2, 3, dtype=torch.float64), 1., 0.),
                                           (f(2, 4, 4, 3), f(2, 4, 5, 3), f(2, 3), 1., 0.)]),
    ]
    for forward, grad, arg_sets in cases:
        for args in arg_sets:
            want, got = G.raised(forward, *args), G.raised(grad, *args)
            assert want[0] is not None and got == want, (forward.__name__, got, want)
