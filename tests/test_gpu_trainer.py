"""GPU tests of the trainer forward: the assignment and loss kernels (csrc/train_targets.hip, csrc/train_losses.hip), their layers and the trainer
model against the NumPy restatement tests/trainer_ref.py.  Assigned targets are compared for exact equality (the log columns
of loc_true within 4 float32 ulp), losses to rtol 1e-5 / atol 1e-6 * weight: with FP contraction off every term is the
restatement's up to the few-ulp difference of log / pow (2^-24 each) and the sums are float64 on both sides, which leaves
the bars about 10x of room.  Every op is launched twice and must give the same bits.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import backbone_cases as MODEL_CASES
import trainer_cases as CASES
import trainer_ref as REF

F32 = np.float32
C = CASES.NUM_CLASSES


def _twice(fn):
    """-> the host copies of fn()'s tensors; a second launch must give the same bits."""
    first, second = [host(t) for t in fn()], [host(t) for t in fn()]
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg="two launches differ")
    return first


def _close(got, want, weight, name):
    got, want = np.asarray(got), np.asarray(want)
    print(f"{name}: got {got} want {want} max rel {np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-30)):.3g}")
    assert got.dtype == F32 and got.shape == want.shape, name
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * weight, err_msg=name)


def _ulps(a, b):
    """distance in float32 steps between two arrays of finite values of one sign pattern"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


# ----------------------------------------------------------------------------- AssignBoxes, ClassLoss, BoxLoss
@pytest.fixture(scope="module", params=["small", "large"])
def assigned(request):
    """-> (gt, priors, the restatement's targets, the device's targets as device tensors)"""
    from masklab_hip.layers import AssignBoxes
    gt, pr = CASES.boxes_small() if request.param == "small" else CASES.boxes_large()
    want = REF.assign_boxes(gt, pr, C)
    layer = AssignBoxes(num_classes=C)
    d_gt, d_pr = dev(gt), dev(pr)[None].expand(gt.shape[0], -1, -1)
    got = _twice(lambda: (*layer([d_gt, d_pr]), layer.last_best))
    return request.param, gt, pr, want, got, layer([d_gt, d_pr])


def test_assign_boxes_equals_the_restatement(assigned):
    name, gt, pr, (best, cls_true, loc_true, mask), (g_cls, g_loc, g_mask, g_best), _ = assigned
    assert g_best.dtype == np.int32 and g_cls.dtype == g_loc.dtype == g_mask.dtype == F32
    np.testing.assert_array_equal(g_best, best)
    np.testing.assert_array_equal(g_cls, cls_true)
    np.testing.assert_array_equal(g_mask, mask)
    np.testing.assert_array_equal(g_loc[..., :2], loc_true[..., :2])
    ulps = _ulps(g_loc[..., 2:], loc_true[..., 2:])
    print(f"[{name}] A={len(pr)} positives={(mask == 0).sum()} ignored={(mask == -1).sum()} log columns: max {ulps.max()} ulp, "
          f"{(ulps > 0).sum()} of {(loc_true[..., 2:] != 0).sum()} non-zero entries differ")
    assert ulps.max() <= 4
    assert (mask == 0).sum() > 50 and (mask == -1).sum() > 50
    if name == "small":
        assert np.all(g_mask[2] == 1) and not g_loc[2].any() and g_best[0].tolist() == [602, 617, 15, 547, 0, 627, 0]


def test_calculate_iou_layer_has_the_oracle_bits():
    from masklab_hip.layers import CalculateIOU
    from oracle.metrics import calculate_iou
    gt, pr = CASES.boxes_small()
    d_gt, d_pr = dev(gt[0]), dev(pr)
    got, = _twice(lambda: (CalculateIOU()([d_gt, d_pr]),))
    np.testing.assert_array_equal(got.view(np.uint32), calculate_iou(gt[0], pr).view(np.uint32))


def test_class_loss(assigned):
    from masklab_hip.losses import ClassLoss
    name, gt, pr, (_, cls_true, _, mask), _, (d_cls, _, d_mask) = assigned
    cls_pred, _, exist = CASES.predictions(gt, len(pr), 3)
    d_pred, d_exist = dev(cls_pred), dev(exist)
    for weight, alpha, gamma in ((300., .25, 2.), (1., .5, 1.5)):
        layer = ClassLoss(weight=weight, alpha=alpha, gamma=gamma)
        got, = _twice(lambda: (layer([d_cls, d_pred, d_mask, d_exist]),))
        _close(got, REF.class_loss(cls_true, cls_pred, mask, exist, weight, alpha, gamma), weight, f"class_loss[{name}]")
    if name == "small":
        assert (mask[2] == 1).all()                                  # no positive: the focal terms of the negatives over #neg


def test_box_loss_three_calls_and_fixed_beta(assigned):
    from masklab_hip.losses import BoxLoss
    name, gt, pr, (_, _, loc_true, mask), _, (_, d_loc, d_mask) = assigned
    _, loc_pred, _ = CASES.predictions(gt, len(pr), 4)
    d_pred = dev(loc_pred)
    layer, ref = BoxLoss(weight=2., momentum=.9, beta=.11, use_adjust=True), REF.BoxLoss(2., .9, .11, True)
    for call in range(3):
        got = host(layer([d_loc, d_pred, d_mask]))
        want = ref(loc_true, loc_pred, mask)
        _close(got, want, 2., f"box_loss[{name}] call {call}")
        mm, mv = host(layer.moving_mean), host(layer.moving_var)
        print(f"  moving_mean {mm} moving_var {mv}")
        np.testing.assert_allclose(mm, ref.moving_mean, rtol=1e-5)
        np.testing.assert_allclose(mv, ref.moving_var, rtol=1e-5)
    assert np.all(ref.moving_mean != F32(.11)) and np.all(ref.moving_var > 0)
    again = BoxLoss(weight=2., momentum=.9, beta=.11, use_adjust=True)       # a fresh layer: the same bits as the first call
    first = BoxLoss(weight=2., momentum=.9, beta=.11, use_adjust=True)
    np.testing.assert_array_equal(host(again([d_loc, d_pred, d_mask])), host(first([d_loc, d_pred, d_mask])))
    np.testing.assert_array_equal(host(again.state), host(first.state))
    fixed = BoxLoss(weight=1., beta=.11, use_adjust=False)
    got, = _twice(lambda: (fixed([d_loc, d_pred, d_mask]),))
    _close(got, REF.BoxLoss(1., .9, .11, False)(loc_true, loc_pred, mask), 1., f"box_loss[{name}] fixed beta")
    np.testing.assert_array_equal(host(fixed.moving_mean), np.full(4, .11, F32))           # untouched without use_adjust
    if name == "small":
        assert got[2] == 0                                           # no positive anchor: 0 / (0 + eps)


# ----------------------------------------------------------------------------- AssignMasks, MaskLoss
@pytest.mark.parametrize("case", ["int8", "uint8", "int8_one_image_unmatched"])
def test_assign_masks_and_mask_loss(case):
    from masklab_hip.layers import AssignMasks
    from masklab_hip.losses import MaskLoss
    roi, gt, masks = CASES.masks_uint8() if case == "uint8" else CASES.masks_int8()
    if case == "int8_one_image_unmatched":
        roi = roi.copy()
        roi[1, :, 4] = (roi[1, :, 4] + 1) % C                        # every RoI of image 1 has the wrong class
        roi[1, 2] = -1
    pred = CASES.mask_predictions(roi, 5)
    want, _, matched = REF.assign_masks(roi, gt, masks, (28, 28), C)
    d_roi, d_gt, d_masks, d_pred = dev(roi), dev(gt), dev(masks), dev(pred)
    layer = AssignMasks()
    got, = _twice(lambda: (layer([d_roi, d_pred, d_gt, d_masks]),))
    assert got.dtype == np.int32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert ((want != C).reshape(want.shape[0], want.shape[1], -1).any(axis=2) == matched).all()
    d_target = dev(got)
    for weight, smoothing in ((1e-2, 0.), (1., .1)):
        loss = MaskLoss(weight=weight, label_smoothing=smoothing)
        g, = _twice(lambda: (loss([d_target, d_pred]),))
        _close(g, REF.mask_loss(want, pred, weight, smoothing), weight, f"mask_loss[{case}]")
        if case == "int8_one_image_unmatched":
            assert g[1] == 0 and g[0] > 0                            # an image with no selected RoI


# ----------------------------------------------------------------------------- AssignSeg, SegLoss
@pytest.mark.parametrize("in_hw,out_hw,dtype", [((5, 5), (9, 9), "uint8"), ((5, 5), (9, 9), "float32"), ((37, 53), (8, 12), "uint8"),
                                                ((37, 53), (8, 12), "float32")])
def test_assign_seg_and_seg_loss(in_hw, out_hw, dtype):
    from masklab_hip.layers import AssignSeg
    from masklab_hip.losses import SegLoss
    if in_hw == (5, 5) and dtype == "float32":
        gt, exist, halves = CASES.seg_case(in_hw, out_hw, "uint8")
        gt = gt.astype(F32)                                          # the same exact halves, float32 truth
    else:
        gt, exist, halves = CASES.seg_case(in_hw, out_hw, dtype)
    assert (halves > 0) == (in_hw == (5, 5))
    pred = CASES.seg_predictions(out_hw, 9)
    want, _ = REF.assign_seg(gt, out_hw)
    d_gt, d_pred, d_exist = dev(gt), dev(pred), dev(exist)
    got, = _twice(lambda: (AssignSeg()([d_gt, d_pred]),))
    assert got.dtype == F32
    np.testing.assert_array_equal(got, want)
    d_true = dev(got)
    for weight, smoothing in ((.5, 0.), (1., .2)):
        layer = SegLoss(weight=weight, label_smoothing=smoothing)
        g, = _twice(lambda: (layer([d_true, d_pred, d_exist]),))
        _close(g, REF.seg_loss(want, pred, exist, weight, smoothing), weight, f"seg_loss[{in_hw}->{out_hw} {dtype}]")


# ----------------------------------------------------------------------------- stale output and scratch memory
def test_no_trainer_op_depends_on_what_its_outputs_and_partials_held():
    """Every output, key table and partial-sum buffer is a torch.empty: the same bits on 0xFF bytes as on zeroes."""
    import dirty_memory as DM
    from masklab_hip import ops
    gt, pr = CASES.boxes_small()
    cls_pred, loc_pred, exist = CASES.predictions(gt, len(pr), 3)
    roi, gt_m, masks = CASES.masks_int8()
    seg, seg_exist, _ = CASES.seg_case((37, 53), (8, 12), "uint8")
    d = {k: dev(v) for k, v in dict(gt=gt, pr=pr, cls_pred=cls_pred, loc_pred=loc_pred, exist=exist, roi=roi, gt_m=gt_m, masks=masks,
                                    mask_pred=CASES.mask_predictions(roi, 5), seg=seg, seg_exist=seg_exist,
                                    seg_pred=CASES.seg_predictions((8, 12), 9)).items()}

    def run():
        state = dev(np.array([.11] * 4 + [0.] * 4, F32))
        best = ops.best_prior(d["gt"], d["pr"])
        cls_true, loc_true, mask = ops.assign_boxes(d["gt"], d["pr"], C, best=best)
        target = ops.assign_masks(d["roi"], d["gt_m"], d["masks"], (28, 28), C)
        seg_true = ops.assign_seg(d["seg"], (8, 12))
        return dict(best=best, cls_true=cls_true, loc_true=loc_true, mask=mask, target=target, seg_true=seg_true,
                    iou=ops.calculate_iou(d["gt"][0], d["roi"][0]),
                    class_loss=ops.class_loss(cls_true, d["cls_pred"], mask, d["exist"], 300., .25, 2.),
                    box_loss=ops.box_loss(loc_true, d["loc_pred"], mask, 1., .9, .11, True, state), state=state,
                    box_loss_fixed=ops.box_loss(loc_true, d["loc_pred"], mask, 1., .9, .11, False),
                    mask_loss=ops.mask_loss(target, d["mask_pred"], 1., .1),
                    seg_loss=ops.seg_loss(seg_true, d["seg_pred"], d["seg_exist"], .5, 0.))

    with DM.zeroed():
        clean = DM.snapshot(run())
    with DM.poisoned():
        dirty = DM.snapshot(run())
    DM.assert_same_bits(dirty, clean, "trainer ops")


# ----------------------------------------------------------------------------- the model
SHAPE = (2, 64, 96, 3)


@pytest.fixture(scope="module")
def models():
    """ResNeXt-50 under the shipped head configuration at 2 x 64 x 96 (five levels down to 1 x 1; MobileNet's explicit
    stride-2 padding does not reach 1 x 1 there and the oracle cannot run it), synthetic weights whose class logits are scaled so
    that proposals exist -> (cfg, trainer, inference, inputs).  One ground-truth row is a proposal the oracle expects, so
    that the detection metrics are not all zero."""
    from masklab_hip import retinamasklab as R
    from oracle import fixtures as FX
    from oracle import masklab as O
    cfg = MODEL_CASES.shipped_se_config("resnext50", ('C3', 'C4', 'C5', 'P6', 'P7'))
    trainer, inference = R.construct_masklab_networks(cfg, with_trainer=True)
    w = trainer.init_weights(seed=2)
    images = np.random.default_rng(64 + 96).integers(0, 256, SHAPE, dtype=np.uint8)
    c1, l1 = O.inference_forward(cfg, w, images, literal_groups=False, with_instance=False, with_semantic=False)
    scale, thr = FX.choose_logit_scale(cfg, c1, l1, SHAPE[1], SHAPE[2])
    assert scale is not None, "no order-stable logit scale on the grid"
    for proposal in (trainer.metric_proposal, inference.detection_proposal):
        proposal.min_confidence = thr
    bias = -np.log(99.0)
    scaled = (1.0 / (1.0 + np.exp(-(scale * (np.log(c1.astype(np.float64) / (1.0 - c1)) - bias) + bias)))).astype(F32)
    det = cfg.detection
    expected, _ = O.detection_proposal(scaled, FX.boxes_from(cfg, l1, SHAPE[1], SHAPE[2]), thr, det.nms_iou_threshold,
                                       det.post_iou_threshold, det.nms_max_output_size)
    assert expected[1, 0, 0] != -1, "fixture: image 1 has no proposal"
    w = FX.scale_cls_logits(w, scale)
    trainer.load_weights(w, "cuda:0")
    inference.load_weights(w, "cuda:0")
    rng = np.random.default_rng(7)
    gt_boxes = np.full((2, 4, 6), -1, np.float32)
    gt_boxes[0, 0] = (40, 28, 40, 34, 1, 1)
    gt_boxes[0, 2] = (70, 40, 30, 22, 3, 1)                          # a -1 row between valid rows
    gt_boxes[1, 1] = (20, 30, 24, 36, 0, 1)
    gt_boxes[1, 3] = (*np.round(expected[1, 0, :4], 1), expected[1, 0, 4], 1)
    gt_masks = np.full((2, 4, 64, 96), -1, np.int8)
    for b, g in ((0, 0), (0, 2), (1, 1), (1, 3)):
        gt_masks[b, g] = CASES._ellipse(64, 96, gt_boxes[b, g])
    inputs = dict(images=images, gt_boxes=gt_boxes, gt_boxes_exist=np.array([[1, 1, 0, 1, 1], [1, 1, 1, 1, 1]], F32),
                  gt_masks=gt_masks, gt_seg=(rng.random(SHAPE) < 0.5).astype(np.uint8), gt_seg_exist=np.array([[1, 1, 1], [1, 0, 1]], F32))
    return cfg, trainer, inference, inputs


def test_trainer_model_equals_the_restatement_on_its_own_predictions(models):
    cfg, trainer, inference, inputs = models
    before = inference.predict(inputs["images"])
    ref_loss = REF.BoxLoss(cfg.loss.box_loss_weight, cfg.loss.box_loss_momentum, cfg.loss.box_loss_beta, cfg.loss.box_loss_use_adjust)
    ref_loss.moving_mean, ref_loss.moving_var = host(trainer.box_loss.moving_mean).copy(), host(trainer.box_loss.moving_var).copy()
    outs = trainer([inputs[n] for n in trainer.input_names])
    assert len(outs) == 10 and all(o.dtype == torch.float32 and tuple(o.shape) == (2,) for o in outs)
    fw = {k: host(v) for k, v in trainer.last_forward.items()}
    assert set(fw) >= {"cls_pred", "loc_pred", "pr_boxes", "proposed", "proposed_loss", "roi_boxes", "roi_masks", "seg_pred", "cls_true",
                       "loc_true", "assign_mask", "match_gt_masks", "seg_assigned"}
    fw["pr_boxes"] = fw["pr_boxes"][0]
    got = dict(zip(trainer.output_names, (host(o) for o in outs)))
    want, targets = REF.trainer_tail(cfg, inputs, fw, ref_loss)
    for name in ("best_prior", "cls_true", "assign_mask", "seg_assigned"):
        np.testing.assert_array_equal(fw[name], targets[name], err_msg=name)
    np.testing.assert_array_equal(fw["loc_true"][..., :2], targets["loc_true"][..., :2])
    assert _ulps(fw["loc_true"][..., 2:], targets["loc_true"][..., 2:]).max() <= 4
    flips = fw["match_gt_masks"] != targets["match_gt_masks"]        # RoIs come from the network: no 0.5 guard on their crops
    print(f"match_gt_masks: {flips.sum()} of {flips.size} cells differ; selected RoIs {(targets['match_gt_masks'].min(axis=(2, 3)) < C).sum()}")
    assert not flips.any()
    weights = dict(class_loss=cfg.loss.cls_loss_weight, box_loss=cfg.loss.box_loss_weight, mask_loss=cfg.loss.mask_loss_weight,
                   seg_loss=cfg.loss.seg_loss_weight)
    for name in trainer.output_names:
        if name in weights:
            _close(got[name], want[name], weights[name], name)
        else:                                                        # the six metrics, as tests/test_gpu_evaluate.py holds them
            print(f"{name}: {got[name]}")
            np.testing.assert_array_equal(got[name].view(np.uint32), np.asarray(want[name], F32).view(np.uint32), err_msg=name)
    assert (targets["match_gt_masks"].min(axis=(2, 3)) < C).any(axis=1).all() and got["mask_loss"].min() > 0
    assert got["detection_recall_metric"][1] > 0 and got["detection_precision_metric"][0] == 0
    assert (fw["proposed"][..., 0] != -1).sum() > 0 and (fw["proposed_loss"][..., 0] != -1).sum() > (fw["proposed"][..., 0] != -1).sum()
    named = trainer.predict(inputs)                                  # the reference's dict in, {name: ndarray} out
    assert list(named) == trainer.output_names and all(v.shape == (2,) and v.dtype == F32 for v in named.values())
    for name in ("class_loss", "mask_loss", "seg_loss", "my_road_metric"):      # (box_loss moved its statistics in between)
        np.testing.assert_array_equal(named[name], got[name], err_msg=name)
    after = inference.predict(inputs["images"])
    for name, a, b in zip(inference.output_names, before, after):    # the layers are shared: nothing of theirs may change
        np.testing.assert_array_equal(a, b, err_msg=name)


def test_trainer_rois_are_the_ground_truth_rows_plus_the_loss_proposals(models):
    from masklab_hip import ops
    from oracle import masklab as O
    cfg, trainer, _, inputs = models
    trainer(inputs)
    fw = trainer.last_forward
    boxes = ops.restore_boxes(fw["loc_pred"], fw["pr_boxes"][0].contiguous())
    c = cfg.loss
    ref, _ = O.detection_proposal(host(fw["cls_pred"]), host(boxes), c.min_confidence, c.nms_iou_threshold, c.post_iou_threshold,
                                  c.nms_max_output_size)
    proposed, roi_boxes = host(fw["proposed_loss"]), host(fw["roi_boxes"])
    np.testing.assert_array_equal(proposed[:, :ref.shape[1]], ref)   # rows incl. -1 padding, bit exact
    assert np.all(proposed[:, ref.shape[1]:] == -1)
    for b in range(SHAPE[0]):
        gt = inputs["gt_boxes"][b]
        want = np.concatenate([gt[gt[:, 0] != -1], ref[b][ref[b][:, 0] != -1]])
        rows = roi_boxes[b][roi_boxes[b][:, 0] != -1]
        assert len(rows) == len(want) > (gt[:, 0] != -1).sum()
        key = lambda r: r[np.lexsort(r.T[::-1])]
        np.testing.assert_array_equal(key(rows), key(want))
