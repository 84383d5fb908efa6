"""GPU tests of the losses' backward (csrc/train_losses.hip): the four fused "loss + gradient" ops, the layers'
call_with_grad and TrainerModel.loss_and_gradients against torch autograd over the float64 restatement of
tests/trainer_grad_ref.py.  The bar is |got - want| <= 1e-5 * S, S the uncancelled magnitude (trainer_grad_ref.check): a term
is about a dozen float32 operations plus logf / powf, each within a couple of ulp, about 1e-6 of S.  Every case also holds:
two launches give the same bits; the loss has the forward-only call's bits; exact zeros where the gradient is exactly zero;
through_sigmoid is the plain gradient times pred * (1 - pred) within 2 float32 ulp; the bits do not depend on what the
outputs and partials held; `upstream` scales per image and a zero gives exact zeros.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import backbone_cases as MODEL_CASES
import dirty_memory as DM
import trainer_cases as CASES
import trainer_grad_ref as G
import trainer_ref as REF

F32, F64 = np.float32, np.float64
C = CASES.NUM_CLASSES


def _bits(a, b, what):
    DM.assert_same_bits(DM.snapshot(a), DM.snapshot(b), what)


def _ulps(a, b):
    """distance in float32 steps, signed zeros alike"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def _upstreams(B, seed):
    """random positives with one 0; a single image gets a positive and a 0 in turn"""
    if B == 1:
        return [np.array([0.7], F32), np.zeros(1, F32)]
    up = np.random.default_rng(seed).uniform(0.2, 2.0, B).astype(F32)
    up[B // 2] = 0
    return [up]


def check_case(name, fused, forward, pred, want_fn, scale_fn=None, sigmoid=True):
    """fused(upstream or None, through_sigmoid) -> (loss, grad) on the device, from equal starting states each time;
    forward() -> the forward-only loss; want_fn(upstream) -> autograd's float64 gradient; scale_fn(upstream, through_sigmoid)
    -> S (None: |want|).  Runs the seven checks of the module's docstring."""
    B = pred.shape[0]
    loss, grad = (host(t) for t in fused(None, False))
    _bits(fused(None, False), (loss, grad), f"{name}: two launches")                              # 1
    _bits(forward(), loss, f"{name}: the forward-only loss")                                      # 2
    assert grad.dtype == F32 and grad.shape == pred.shape
    want = want_fn(G.default_upstream(B))
    G.check(grad, want, None if scale_fn is None else scale_fn(G.default_upstream(B), False), name)          # 3, 4
    if sigmoid:                                                                                   # 5
        s_loss, s_grad = (host(t) for t in fused(None, True))
        _bits(s_loss, loss, f"{name}: loss through sigmoid")
        times = (grad.astype(F64) * (pred.astype(F64) * (1 - pred.astype(F64)))).astype(F32)
        ulps = _ulps(s_grad, times)
        print(f"{name}: through_sigmoid against grad * pred * (1 - pred): max {ulps.max()} ulp")
        assert ulps.max() <= 2 and not s_grad[grad == 0].any()
    with DM.zeroed():                                                                             # 6
        clean = DM.snapshot(fused(None, sigmoid))
    with DM.poisoned():
        dirty = DM.snapshot(fused(None, sigmoid))
    DM.assert_same_bits(dirty, clean, f"{name}: stale outputs and partials")
    assert not DM.poison_elements(dirty[1]).any()
    for k, up in enumerate(_upstreams(B, len(name))):                                             # 7
        u_loss, u_grad = (host(t) for t in fused(dev(up), False))
        _bits(u_loss, loss, f"{name}: the loss does not depend on upstream")
        G.check(u_grad, want_fn(up), None if scale_fn is None else scale_fn(up, False), f"{name} upstream {up}")
        assert not u_grad[up == 0].any()


# ----------------------------------------------------------------------------- the class and box cases
def _small():
    gt, pr = CASES.boxes_small()
    _, cls_true, loc_true, mask = REF.assign_boxes(gt, pr, C)
    cls_pred, _, exist = CASES.predictions(gt, len(pr), 3)
    _, loc_pred, _ = CASES.predictions(gt, len(pr), G.BOX_SEED)
    assert (mask[2] == 1).all() and len(pr) % 256 and (exist == 0).any()
    return dict(cls_true=cls_true, loc_true=loc_true, mask=mask, cls_pred=cls_pred, loc_pred=loc_pred, exist=exist)


def adjusted_betas(loc_true, loc_pred, mask, calls=3):
    ref, betas = REF.BoxLoss(1., .9, .11, True), []
    for _ in range(calls):
        ref(loc_true, loc_pred, mask)
        betas.append(np.clip(ref.moving_mean - ref.moving_var, F32(1e-3), F32(.11)))
    return betas


def branch_distance(loc_true, loc_pred, mask, betas):
    """float64 | |d| - 1.5 beta |, the minimum over `betas`, +inf off the positive anchors: [B,A,4]"""
    d = np.abs(loc_true.astype(F64) - loc_pred.astype(F64))
    near = np.min([np.abs(d - 1.5 * np.broadcast_to(np.asarray(b, F64), (4,))) for b in betas], axis=0)
    return np.where((mask.reshape(mask.shape[0], -1) == 0)[..., None], near, np.inf)


def _strided():
    """B = 1, A = ML_TRAIN_MAX_BLOCKS * 256 + 77: the grid-stride loop wraps once; masks from {-1, 0, 1}; class predictions
    include the clip's two ends EXACTLY (they pass) and their outer neighbours (zero gradient).  With ~44 000 positives some
    N(0, 1) box coordinate always lands within GUARD of a branch point, so those predictions are moved by 0.01 until the
    float64 check below holds for 0.11 and the three adjusted betas (which move by ~1e-7 with them)."""
    from masklab_hip import _lib
    A = _lib.TRAIN_MAX_BLOCKS * 256 + 77
    rng = np.random.default_rng(A)
    mask = rng.integers(-1, 2, (1, A, 1)).astype(F32)
    cls_true = (rng.integers(0, C + 1, (1, A, 1)) == np.arange(C)).astype(F32)
    cls_pred = rng.uniform(0, 1, (1, A, C)).astype(F32)
    eps, hi = F32(1e-7), F32(1) - F32(1e-7)
    cls_pred[0, -2] = [eps, hi, np.nextafter(eps, F32(0)), np.nextafter(hi, F32(1)), 0.5]
    cls_pred[0, -1] = [hi, eps, 0, 1, 0.25]
    mask[0, -2:] = [[0], [1]]
    exist = np.array([[1, 1, 0, 1, 1]], F32)
    loc_true = (rng.normal(size=(1, A, 4)) * (mask == 0)).astype(F32)
    loc_pred = rng.normal(size=(1, A, 4)).astype(F32)
    for _ in range(10):
        betas = adjusted_betas(loc_true, loc_pred, mask) + [.11]
        close = branch_distance(loc_true, loc_pred, mask, betas) < 3 * CASES.GUARD
        if not close.any():
            break
        loc_pred[close] += F32(0.01)
    return dict(cls_true=cls_true, loc_true=loc_true, mask=mask, cls_pred=cls_pred, loc_pred=loc_pred, exist=exist)


@pytest.fixture(scope="module", params=["small", "strided"])
def boxes(request):
    host_side = _small() if request.param == "small" else _strided()
    return request.param, host_side, {k: dev(v) for k, v in host_side.items()}


@pytest.mark.parametrize("weight,alpha,gamma", [(300., .25, 2.), (1., .5, 1.5)])
def test_class_loss_grad(boxes, weight, alpha, gamma):
    from masklab_hip.losses import ClassLoss
    name, h, d = boxes
    layer = ClassLoss(weight=weight, alpha=alpha, gamma=gamma)
    inputs = [d["cls_true"], d["cls_pred"], d["mask"], d["exist"]]
    fn = lambda x: G.class_loss(h["cls_true"], x, h["mask"], h["exist"], weight, alpha, gamma)
    check_case(f"class_loss[{name} {weight:g} {alpha} {gamma}]", lambda up, sig: layer.call_with_grad(inputs, up, sig),
               lambda: layer(inputs), h["cls_pred"], lambda up: G.autograd(fn, h["cls_pred"], up)[1])
    grad = host(layer.call_with_grad(inputs)[1])
    if name == "small":
        assert np.isfinite(grad[2]).all() and grad[2].any() and not grad[0, :3].reshape(-1)[[0, 1, 3, 4]].any()
    else:
        assert grad[0, -2, 0] != 0 and grad[0, -2, 1] != 0 and not grad[0, -2, 2:4].any()       # at the clip's ends / beyond
        assert grad[0, -1, 0] != 0 and grad[0, -1, 1] != 0 and not grad[0, -1, 2:4].any()


def test_box_loss_grad_fixed_beta(boxes):
    from masklab_hip.losses import BoxLoss
    name, h, d = boxes
    assert branch_distance(h["loc_true"], h["loc_pred"], h["mask"], [.11]).min() > CASES.GUARD
    layer = BoxLoss(weight=1., beta=.11, use_adjust=False)
    inputs = [d["loc_true"], d["loc_pred"], d["mask"]]
    fn = lambda x: G.box_loss(h["loc_true"], x, h["mask"], 1., .11)
    check_case(f"box_loss[{name} fixed beta]", lambda up, sig: layer.call_with_grad(inputs, up), lambda: layer(inputs), h["loc_pred"],
               lambda up: G.autograd(fn, h["loc_pred"], up)[1], sigmoid=False)
    np.testing.assert_array_equal(host(layer.moving_mean), np.full(4, .11, F32))                 # untouched without use_adjust
    if name == "small":
        assert not host(layer.call_with_grad(inputs)[1])[2].any()                               # no positive anchor: exact zeros
    with pytest.raises(ValueError, match="through_sigmoid"):
        layer.call_with_grad(inputs, through_sigmoid=True)


def test_box_loss_grad_adjusted_over_three_calls(boxes):
    from masklab_hip import ops
    from masklab_hip.losses import BoxLoss
    name, h, d = boxes
    betas = adjusted_betas(h["loc_true"], h["loc_pred"], h["mask"])
    near = branch_distance(h["loc_true"], h["loc_pred"], h["mask"], betas).min()
    print(f"[{name}] positives {(h['mask'] == 0).sum()}, nearest coordinate to a branch point {near:.3g}")
    assert near > CASES.GUARD
    inputs = [d["loc_true"], d["loc_pred"], d["mask"]]
    fused, forward = BoxLoss(weight=2., momentum=.9, beta=.11, use_adjust=True), BoxLoss(weight=2., momentum=.9, beta=.11, use_adjust=True)
    up = _upstreams(h["mask"].shape[0], 5)[0]
    for call, beta in enumerate(betas):
        loss, grad = fused.call_with_grad(inputs, upstream=dev(up))
        _bits(loss, forward(inputs), f"box_loss[{name}] call {call}: the forward-only loss")
        _bits(fused.state, forward.state, f"box_loss[{name}] call {call}: the moving statistics")
        fn = lambda x: G.box_loss(h["loc_true"], x, h["mask"], 2., beta)
        G.check(host(grad), G.autograd(fn, h["loc_pred"], up)[1], name=f"box_loss[{name} adjusted] call {call}")
    assert np.all(host(fused.moving_mean) != F32(.11))

    def fresh(upstream, sig):                                        # the first call again, from the initial state every time
        state = dev(np.array([.11] * 4 + [0.] * 4, F32))
        return ops.box_loss_grad(*inputs, 2., .9, .11, True, state, upstream=upstream) + (state,)

    def fresh_forward():
        return ops.box_loss(*inputs, 2., .9, .11, True, dev(np.array([.11] * 4 + [0.] * 4, F32)))

    fn = lambda x: G.box_loss(h["loc_true"], x, h["mask"], 2., betas[0])
    check_case(f"box_loss[{name} adjusted, first call]", lambda u, s: fresh(u, s)[:2], fresh_forward, h["loc_pred"],
               lambda u: G.autograd(fn, h["loc_pred"], u)[1], sigmoid=False)
    with DM.zeroed():
        clean = DM.snapshot(fresh(None, False))
    with DM.poisoned():
        DM.assert_same_bits(DM.snapshot(fresh(None, False)), clean, f"box_loss[{name}]: the state on stale memory")


# ----------------------------------------------------------------------------- the mask cases
@pytest.mark.parametrize("smoothing", [0., .1])
@pytest.mark.parametrize("case", ["int8", "int8_one_image_unselected"])
def test_mask_loss_grad(case, smoothing):
    from masklab_hip.losses import MaskLoss
    roi, gt, masks = CASES.masks_int8()
    target, _, matched = REF.assign_masks(roi, gt, masks, (28, 28), C)
    assert target.shape[2] * target.shape[3] == 784 and not matched.all() and matched.any(axis=1).all()
    if case == "int8_one_image_unselected":
        target = target.copy()
        target[1] = C                                                # no RoI of image 1 is selected: nz = 0, the divisor is 1
    pred = CASES.mask_predictions(roi, 5)
    d_target, d_pred = dev(target), dev(pred)
    layer = MaskLoss(weight=1., label_smoothing=smoothing)
    fn = lambda x: G.mask_loss(target, x, 1., smoothing)
    check_case(f"mask_loss[{case} smoothing {smoothing}]", lambda up, sig: layer.call_with_grad([d_target, d_pred], up, sig),
               lambda: layer([d_target, d_pred]), pred, lambda up: G.autograd(fn, pred, up)[1],
               lambda up, sig: G.mask_loss_grad(target, pred, 1., smoothing, up, sig, with_scale=True)[1])
    loss, grad = (host(t) for t in layer.call_with_grad([d_target, d_pred]))
    selected = grad.reshape(2, 6, -1).any(axis=2)
    if case == "int8":
        assert selected.tolist() == matched.tolist()
    else:
        assert loss[1] == 0 and not grad[1].any() and selected[0].tolist() == matched[0].tolist()
    assert (np.count_nonzero(grad.reshape(2, 6, 784, C), axis=(2, 3)) == 784 * selected).all()   # one channel of a selected RoI


# ----------------------------------------------------------------------------- the seg cases
@pytest.mark.parametrize("smoothing", [0., .1])
@pytest.mark.parametrize("case", ["small", "strided"])
def test_seg_loss_grad(case, smoothing):
    from masklab_hip.losses import SegLoss
    if case == "small":
        gt, exist, _ = CASES.seg_case((37, 53), (8, 12), "uint8")
        true, _ = REF.assign_seg(gt, (8, 12))
        true, pred = true.astype(F32), CASES.seg_predictions((8, 12), 9)
    else:                                                            # 363 x 362 pixels > ML_TRAIN_MAX_BLOCKS * 256: the loop wraps
        rng = np.random.default_rng(363)
        true = (rng.random((1, 363, 362, 3)) < 0.5).astype(F32)
        pred = rng.uniform(0, 1, true.shape).astype(F32)
        exist = np.array([[1, 0, 1]], F32)
        from masklab_hip import _lib
        assert 363 * 362 > _lib.TRAIN_MAX_BLOCKS * 256
    assert (exist == 0).any() and pred.shape[3] == 3
    d_true, d_pred, d_exist = dev(true), dev(pred), dev(exist)
    layer = SegLoss(weight=.5, label_smoothing=smoothing)
    fn = lambda x: G.seg_loss(true, x, exist, .5, smoothing)
    check_case(f"seg_loss[{case} smoothing {smoothing}]", lambda up, sig: layer.call_with_grad([d_true, d_pred, d_exist], up, sig),
               lambda: layer([d_true, d_pred, d_exist]), pred, lambda up: G.autograd(fn, pred, up)[1],
               lambda up, sig: G.seg_loss_grad(true, pred, exist, .5, smoothing, up, sig, with_scale=True)[1])
    grad = host(layer.call_with_grad([d_true, d_pred, d_exist])[1])
    assert not grad[..., exist[-1] == 0][-1].any() and grad[..., exist[-1] != 0].all()


# ----------------------------------------------------------------------------- the ops' checks on device tensors
def test_grad_ops_refuse_what_their_forward_twins_refuse_on_the_device():
    from masklab_hip import ops
    f = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    cases = [(ops.class_loss, ops.class_loss_grad, (f(2, 7, 5), f(2, 6, 5), f(2, 7, 1), f(2, 5), 1., .25, 2.), ValueError),
             (ops.class_loss, ops.class_loss_grad, (f(2, 7, 5), f(2, 7, 5, dtype=torch.float16), f(2, 7, 1), f(2, 5), 1., .25, 2.), RuntimeError),
             (ops.box_loss, ops.box_loss_grad, (f(2, 7, 4), f(2, 7, 4), f(2, 6, 1), 1., .9, .11, False), ValueError),
             (ops.box_loss, ops.box_loss_grad, (f(2, 7, 4), f(2, 7, 4), f(2, 7, 1), 1., .9, .11, True, f(7)), ValueError),
             (ops.mask_loss, ops.mask_loss_grad, (f(2, 3, 4, 4), f(2, 3, 4, 4, 5), 1., 0.), ValueError),
             (ops.seg_loss, ops.seg_loss_grad, (f(2, 4, 4, 3), f(2, 4, 4, 3), f(2, 2), 1., 0.), ValueError)]
    for forward, grad, args, kind in cases:
        want, got = G.raised(forward, *args), G.raised(grad, *args)
        assert want[0] is kind and got == want, (forward.__name__, got, want)
    with pytest.raises(ValueError, match="upstream"):
        ops.seg_loss_grad(f(2, 4, 4, 3), f(2, 4, 4, 3), f(2, 3), 1., 0., upstream=f(3))
    big = torch.zeros((33, 1, 2, 2, 5), device="cuda")
    with pytest.raises(RuntimeError, match="B <= 32"):
        ops.mask_loss_grad(torch.zeros((33, 1, 2, 2), dtype=torch.int32, device="cuda"), big, 1., 0.)


# ----------------------------------------------------------------------------- the model
SHAPE = (2, 64, 96, 3)


@pytest.fixture(scope="module")
def trainers():
    """The smallest trainer configuration tests/test_gpu_trainer.py builds (ResNeXt-50, shipped heads, 2 x 64 x 96), twice
    from the same weights -- BoxLoss's state advances per call -> (cfg, weights, trainer, its twin, inputs).  The RoIs hold
    the ground-truth rows, so selected RoIs exist whatever the proposals are."""
    from masklab_hip import retinamasklab as R
    cfg = MODEL_CASES.shipped_se_config("resnext50", ('C3', 'C4', 'C5', 'P6', 'P7'))
    first, _ = R.construct_masklab_networks(cfg, with_trainer=True)
    twin, _ = R.construct_masklab_networks(cfg, with_trainer=True)
    w = first.init_weights(seed=2)
    first.load_weights(w, "cuda:0")
    twin.load_weights(w, "cuda:0")
    rng = np.random.default_rng(7)
    gt_boxes = np.full((2, 4, 6), -1, F32)
    gt_boxes[0, 0] = (40, 28, 40, 34, 1, 1)
    gt_boxes[0, 2] = (70, 40, 30, 22, 3, 1)
    gt_boxes[1, 1] = (20, 30, 24, 36, 0, 1)
    gt_masks = np.full((2, 4, 64, 96), -1, np.int8)
    for b, g in ((0, 0), (0, 2), (1, 1)):
        gt_masks[b, g] = CASES._ellipse(64, 96, gt_boxes[b, g])
    inputs = dict(images=rng.integers(0, 256, SHAPE, dtype=np.uint8), gt_boxes=gt_boxes,
                  gt_boxes_exist=np.array([[1, 1, 0, 1, 1], [1, 1, 1, 1, 1]], F32), gt_masks=gt_masks,
                  gt_seg=(rng.random(SHAPE) < 0.5).astype(np.uint8), gt_seg_exist=np.array([[1, 1, 1], [1, 0, 1]], F32))
    return cfg, w, first, twin, inputs


def _ops_on(trainer, fw, inputs, state, through_sigmoid):
    """the four ops on the tensors of a forward, upstream 1 / B -> {prediction name: (loss, grad)}"""
    from masklab_hip import ops
    c, out = trainer.configuration.loss, {}
    if "cls_pred" in fw:
        out["cls_pred"] = ops.class_loss_grad(fw["cls_true"], fw["cls_pred"], fw["assign_mask"], dev(inputs["gt_boxes_exist"]),
                                              c.cls_loss_weight, c.cls_loss_alpha, c.cls_loss_gamma, through_sigmoid=through_sigmoid)
        out["loc_pred"] = ops.box_loss_grad(fw["loc_true"], fw["loc_pred"], fw["assign_mask"], c.box_loss_weight, c.box_loss_momentum,
                                            c.box_loss_beta, c.box_loss_use_adjust, state)
    if "roi_masks" in fw:
        out["roi_masks"] = ops.mask_loss_grad(fw["match_gt_masks"], fw["roi_masks"], c.mask_loss_weight, c.mask_loss_label_smoothing,
                                              through_sigmoid=through_sigmoid)
    if "seg_pred" in fw:
        out["seg_pred"] = ops.seg_loss_grad(fw["seg_assigned"], fw["seg_pred"], dev(inputs["gt_seg_exist"]), c.seg_loss_weight,
                                            c.seg_loss_label_smoothing, through_sigmoid=through_sigmoid)
    return out


@pytest.mark.parametrize("wrt", ["predictions", "pre_activation"])
def test_loss_and_gradients_is_the_forward_plus_the_four_ops(trainers, wrt):
    cfg, _, trainer, twin, inputs = trainers
    _bits(trainer.box_loss.state, twin.box_loss.state, "the two trainers start from equal BoxLoss states")
    state = trainer.box_loss.state.clone()
    want_outputs = twin(inputs)
    outputs, grads = trainer.loss_and_gradients(inputs, wrt=wrt)
    _bits(outputs, want_outputs, "loss_and_gradients' outputs against call's")
    _bits(trainer.box_loss.state, twin.box_loss.state, "BoxLoss moved once")
    fw = trainer.last_forward
    assert list(grads) == ["cls_pred", "loc_pred", "roi_masks", "seg_pred"] and fw["grads"] is grads
    by_name = dict(zip(trainer.output_names, outputs))
    for pred_name, (loss, grad) in _ops_on(trainer, fw, inputs, state, wrt == "pre_activation").items():
        assert grads[pred_name].shape == fw[pred_name].shape and grads[pred_name].dtype == torch.float32
        _bits(grads[pred_name], grad, f"grads[{pred_name}] ({wrt})")
        _bits(by_name[{v: k for k, v in trainer.GRAD_OF.items()}[pred_name]], loss, f"the loss beside grads[{pred_name}]")
        assert host(grad).any(), pred_name
    assert (host(fw["match_gt_masks"]).min(axis=(2, 3)) < C).any()


def test_loss_and_gradients_upstream_by_name_and_bad_arguments(trainers):
    _, _, trainer, twin, inputs = trainers
    up = np.array([0, 2.5], F32)
    _, base = twin.loss_and_gradients(inputs)
    _, grads = trainer.loss_and_gradients(inputs, upstream={"seg_loss": up, "mask_loss": dev(up)})
    _bits(grads["cls_pred"], base["cls_pred"], "an upstream for other losses leaves cls_pred's gradient alone")
    for name in ("seg_pred", "roi_masks"):
        g, b = host(grads[name]), host(base[name])
        assert not g[0].any() and g[1].any()
        np.testing.assert_allclose(g[1], b[1] * 5, rtol=1e-6)       # 2.5 against 1 / 2
    with pytest.raises(ValueError, match="wrt"):
        trainer.loss_and_gradients(inputs, wrt="logits")
    with pytest.raises(ValueError, match="not losses"):
        trainer.loss_and_gradients(inputs, upstream={"cls_pred": up})


def test_gradients_shrink_with_the_head_groups(trainers):
    from masklab_hip import retinamasklab as R
    cfg, w, trainer, _, inputs = trainers
    bb, det, ins, sem = trainer.backbone_network, trainer.detection_networks, trainer.instance_networks, trainer.semantic_networks
    no_ins = R.construct_trainer_network(cfg, bb, detection_networks=det, semantic_networks=sem).load_weights(w, "cuda:0")
    no_sem = R.construct_trainer_network(cfg, bb, detection_networks=det, instance_networks=ins).load_weights(w, "cuda:0")
    only_sem = R.construct_trainer_network(cfg, bb, semantic_networks=sem).load_weights(w, "cuda:0")
    for model, names in ((no_ins, ["cls_pred", "loc_pred", "seg_pred"]), (no_sem, ["cls_pred", "loc_pred", "roi_masks"]),
                         (only_sem, ["seg_pred"])):
        outputs, grads = model.loss_and_gradients({n: inputs[n] for n in model.input_names})
        assert list(grads) == names and len(outputs) == len(model.output_names)
        for n in names:
            assert grads[n].shape == model.last_forward[n].shape and torch.isfinite(grads[n]).all()
