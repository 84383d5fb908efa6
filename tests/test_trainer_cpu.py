"""CPU tests of the trainer forward: the NumPy restatement (tests/trainer_ref.py) of AssignBoxes against a second, per-anchor
formulation (the rule the kernels follow), of AssignMasks and AssignSeg against scalar loops, the fixtures' promised events,
the trainer model's structure and the drop-in surface of the new layers.  No GPU involved."""
import inspect
import math

import numpy as np
import pytest

import trainer_cases as CASES
import trainer_ref as REF

F32 = np.float32


# ----------------------------------------------------------------------------- AssignBoxes
def per_anchor_assign(gt, pr, num_classes):
    """The rule of include/masklab_hip.h ("Trainer forward"), every anchor on its own: match entries = every g with
    IoU >= 0.5 in ascending g, then every g with conf > 0 whose best prior this is; label = the last entry's class, loc_true
    = the sum over entries in that order; -1 if any IoU lies in [0.4, 0.5)."""
    iou = REF.iou_matrix(gt, pr)
    B, G, A = iou.shape
    prf = pr.astype(F32)
    best = np.stack([[int(np.flatnonzero(iou[b, g] == iou[b, g].max())[0]) for g in range(G)] for b in range(B)])
    label = np.full((B, A), -1, F32)
    loc = np.zeros((B, A, 4), F32)
    ignore = np.zeros((B, A), bool)
    anchors = np.arange(A)
    for b in range(B):
        for second in (False, True):
            for g in range(G):
                row = gt[b, g]
                entry = (anchors == best[b, g]) & bool(row[5] > 0) if second else iou[b, g] >= F32(0.5)
                if not second:
                    ignore[b] |= (iou[b, g] >= F32(0.4)) & (iou[b, g] < F32(0.5))
                if not entry.any():
                    continue
                hat = np.stack([(row[0] - prf[:, 0]) / prf[:, 2], (row[1] - prf[:, 1]) / prf[:, 3],
                                np.log(row[2] / prf[:, 2]), np.log(row[3] / prf[:, 3])], axis=1).astype(F32)
                label[b, entry] = row[4]
                loc[b, entry] = loc[b, entry] + hat[entry]
    li = np.where(label != -1, label, num_classes).astype(np.int32)
    cls_true = (li[..., None] == np.arange(num_classes)).astype(F32)
    mask = np.where(ignore, -1, np.where(li == num_classes, 1, 0)).astype(F32)
    return best, cls_true, loc, mask[..., None]


@pytest.mark.parametrize("case", ["small", "large"])
def test_literal_assign_boxes_equals_the_per_anchor_rule(case):
    gt, pr = CASES.boxes_small() if case == "small" else CASES.boxes_large()
    with np.errstate(invalid="ignore", divide="ignore"):             # log of a padded row's -1, never selected
        want = per_anchor_assign(gt, pr, CASES.NUM_CLASSES)
    got = REF.assign_boxes(gt, pr, CASES.NUM_CLASSES)
    for name, g, w in zip(("best", "cls_true", "loc_true", "assign_mask"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert got[1].dtype == got[2].dtype == got[3].dtype == F32 and got[3].shape == gt.shape[:1] + (len(pr), 1)


def test_the_small_box_table_contains_every_event_of_the_rule():
    gt, pr = CASES.boxes_small()
    iou = REF.iou_matrix(gt, pr)
    best, cls_true, loc_true, mask = REF.assign_boxes(gt, pr, CASES.NUM_CLASSES)
    ties = [int((iou[0, g] == iou[0, g].max()).sum()) for g in range(6)]
    assert ties[0] == 2 and ties[3] == 4 and ties[2] == 20 and ties[4] == len(pr)            # the first index must win
    assert best[0].tolist() == [602, 617, 15, 547, 0, 627, 0] and best[2].tolist() == [0] * 7
    both = (iou[0, 0] >= 0.5) & (iou[0, 1] >= 0.5)
    last = both & (iou[0, 5] < 0.5) & (np.arange(len(pr)) != 602)                              # rows 0 and 1 and nothing after them
    assert both.sum() == 25 and last.sum() > 0 and np.all(cls_true[0, last, 1] == 1)           # the higher row's label wins
    a = 602                                                                                    # row 0's best prior: entered twice
    p = pr[a].astype(F32)
    once = (gt[0, 0, 0] - p[0]) / p[2]
    other = (gt[0, 1, 0] - p[0]) / p[2] if iou[0, 1, a] >= 0.5 else F32(0)
    assert loc_true[0, a, 0] == (F32(0) + once + other) + once
    assert 0 < iou[0, 2].max() < 0.03 and mask[0, 15, 0] == 0 and cls_true[0, 15, 2] == 1     # a forced positive
    assert iou[0, 4].max() == 0 and cls_true[0, 0, 4] == 1 and loc_true[0, 0, 2] == np.log(F32(10) / F32(pr[0, 2]))
    band = (iou[0, 0] >= 0.5) & (iou[0, 5] >= 0.4) & (iou[0, 5] < 0.5)
    assert band.sum() == 2 and np.all(mask[0, band, 0] == -1) and np.all(cls_true[0, band].sum(axis=1) == 1)
    assert np.all(mask[2] == 1) and not cls_true[2].any() and not loc_true[2].any()          # no valid row at all
    assert gt[1, 1, 0] == -1 and gt[1, 2, 0] != -1 and (mask[1] == 0).sum() > 0


# ----------------------------------------------------------------------------- AssignMasks
def scalar_crop_sample(img, box, i, j, ch, cw):
    """tf.image.crop_and_resize for ONE output cell, float32 scalars (extrapolation value 0)."""
    H, W = img.shape
    y1, x1, y2, x2 = (F32(v) for v in box)
    in_y = y1 * F32(H - 1) + F32(i) * ((y2 - y1) * F32(H - 1) / F32(ch - 1))
    in_x = x1 * F32(W - 1) + F32(j) * ((x2 - x1) * F32(W - 1) / F32(cw - 1))
    if in_y < 0 or in_y > H - 1 or in_x < 0 or in_x > W - 1:
        return F32(0)
    t, b, l, r = math.floor(in_y), math.ceil(in_y), math.floor(in_x), math.ceil(in_x)
    fy, fx = in_y - F32(t), in_x - F32(l)
    top = F32(img[t, l]) + (F32(img[t, r]) - F32(img[t, l])) * fx
    bot = F32(img[b, l]) + (F32(img[b, r]) - F32(img[b, l])) * fx
    return top + (bot - top) * fy


@pytest.mark.parametrize("case", [CASES.masks_int8, CASES.masks_uint8])
def test_assign_masks_equals_scalar_loops(case):
    roi, gt, masks = case()
    got, _, matched = REF.assign_masks(roi, gt, masks, (28, 28), CASES.NUM_CLASSES)
    B, R = roi.shape[:2]
    H, W = masks.shape[2:]
    for b in range(B):
        for r in range(R):
            best, g_best = F32(-1), 0
            for g in range(gt.shape[1]):
                v = REF.calculate_iou(gt[b, g:g + 1, :4], roi[b, r:r + 1, :4])[0, 0]
                v = v * F32(gt[b, g, 5] != -1 and roi[b, r, 5] != -1) * F32(gt[b, g, 4] == roi[b, r, 4])
                if v > best:
                    best, g_best = v, g
            assert bool(best >= 0.5) == bool(matched[b, r])
            if not matched[b, r]:
                assert np.all(got[b, r] == CASES.NUM_CLASSES)
                continue
            box = REF.normalize_boxes(roi[b, r:r + 1], H, W)[0]
            want = np.array([[int(gt[b, g_best, 4]) if scalar_crop_sample(masks[b, g_best], box, i, j, 28, 28) > 0.5
                              else CASES.NUM_CLASSES for j in range(28)] for i in range(28)], np.int32)
            np.testing.assert_array_equal(got[b, r], want)
            assert (want != CASES.NUM_CLASSES).sum() > 20
    if masks.dtype == np.int8:
        tie = REF.assign_masks(roi, gt, masks[:, [1, 0, 2]], (28, 28), CASES.NUM_CLASSES)[0]      # the first of two equal IoUs wins
        assert (tie[0, 0] != got[0, 0]).any() and (got[1, 1, -1] == CASES.NUM_CLASSES).all()      # ... and the extrapolated rows are empty


# ----------------------------------------------------------------------------- AssignSeg
@pytest.mark.parametrize("in_hw,out_hw,dtype", [((5, 5), (9, 9), "uint8"), ((37, 53), (8, 12), "uint8"), ((37, 53), (8, 12), "float32")])
def test_assign_seg_equals_scalar_loops(in_hw, out_hw, dtype):
    gt, _, halves = CASES.seg_case(in_hw, out_hw, dtype)
    got, _ = REF.assign_seg(gt, out_hw)
    assert got.dtype == F32 and (halves > 0) == (in_hw == (5, 5))
    H, W = in_hw
    sy, sx = F32((H - 1) / float(out_hw[0] - 1)), F32((W - 1) / float(out_hw[1] - 1))
    x = gt.astype(F32)
    for b in range(2):
        for i in range(out_hw[0]):
            for j in range(out_hw[1]):
                fy, fx = F32(i) * sy, F32(j) * sx
                t, l = math.floor(fy), math.floor(fx)
                bo, r = min(math.ceil(fy), H - 1), min(math.ceil(fx), W - 1)
                ty, tx = fy - F32(t), fx - F32(l)
                top = x[b, t, l] + (x[b, t, r] - x[b, t, l]) * tx
                bot = x[b, bo, l] + (x[b, bo, r] - x[b, bo, l]) * tx
                v = top + (bot - top) * ty
                want = np.array([round(float(c)) for c in v], F32)              # Python's round: half to even
                np.testing.assert_array_equal(got[b, i, j], want)
    if halves:
        assert set(np.unique(got)) == {0.0, 1.0}                                 # 0.5 -> 0, never 0.5 -> 1 by rounding up


# ----------------------------------------------------------------------------- the losses on inputs counted by hand
def test_restated_losses_on_hand_counted_inputs():
    cls_true = np.array([[[1, 0], [0, 0], [0, 2]]], F32)
    cls_pred = np.array([[[.5, .5], [.5, .5], [.5, .5]]], F32)
    mask = np.array([[[0], [1], [-1]]], F32)
    term = F32(.25) * (-np.power(F32(.5), F32(2)) * np.log(F32(.5)))
    got = REF.class_loss(cls_true, cls_pred, mask, np.array([[1, 0]], F32), weight=2.)
    assert got.shape == (1,) and got[0] == F32(2) * F32(np.float64(term) * 2 / (2 + np.float64(REF.EPS)))
    loc_true = np.zeros((1, 2, 4), F32)
    loc_pred = np.array([[[.1, .16, .17, 1.], [9, 9, 9, 9]]], F32)              # |d| - beta/2 < beta  <=>  |d| < 1.5 beta = 0.165
    layer = REF.BoxLoss(beta=.11)
    terms = [F32(.5) * (F32(.1) * F32(.1)) / F32(.11), F32(.5) * (F32(.16) * F32(.16)) / F32(.11), F32(.17) - F32(.5) * F32(.11),
             F32(1) - F32(.5) * F32(.11)]
    want = (((terms[0] + terms[1]) + terms[2]) + terms[3]) / F32(4)
    assert layer(loc_true, loc_pred, np.array([[[0], [1]]], F32))[0] == F32(np.float64(want) / (1 + np.float64(REF.EPS)))
    adj = REF.BoxLoss(beta=.11, use_adjust=True)
    adj(loc_true, loc_pred, np.array([[[0], [1]]], F32))
    assert adj.moving_mean[0] == F32(.11) * F32(.9) + F32(.05) * F32(1 - .9) and adj.moving_var[0] > 0
    target = np.full((2, 2, 2, 2), 3, np.int32)
    target[0, 1, 0] = 1
    pred = np.full((2, 2, 2, 2, 3), .5, F32)
    got = REF.mask_loss(target, pred, weight=1.)
    assert got[1] == 0 and got[0] == F32(np.float64(-np.log(F32(.5) + REF.EPS)) / 2)      # one selected RoI: its mean over (1 + 1)
    seg = REF.seg_loss(np.ones((1, 2, 2, 2), F32), np.full((1, 2, 2, 2), .5, F32), np.array([[1, 0]]), weight=.5)
    assert seg[0] == F32(.5) * F32(np.float64(-np.log(F32(.5) + REF.EPS)) / 2)


# ----------------------------------------------------------------------------- the model and the layers' surface
def _small_config():
    from masklab_hip import ModelConfiguration
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = "mobilenet"
    return cfg


def test_trainer_network_has_the_reference_outputs_and_shares_the_layers():
    from masklab_hip import retinamasklab as R
    cfg = _small_config()
    trainer, inference = R.construct_masklab_networks(cfg, with_trainer=True)
    assert trainer.input_names == ["images", "gt_boxes", "gt_boxes_exist", "gt_masks", "gt_seg", "gt_seg_exist"]
    assert trainer.output_names == ["class_loss", "box_loss", "detection_precision_metric", "detection_recall_metric",
                                    "detection_fmeasure_metric", "mask_loss", "seg_loss", "other_road_iou_metric", "my_road_metric",
                                    "crack_iou_metric"]
    assert trainer.backbone_network is inference.backbone_network
    for mine, theirs in zip((trainer.detection_networks, trainer.instance_networks, trainer.semantic_networks),
                            (inference.detection_networks, inference.instance_networks, inference.semantic_networks)):
        assert len(mine) == len(theirs) and all(a is b for a, b in zip(mine, theirs))
    d, l = cfg.detection, cfg.loss
    assert trainer.metric_proposal.get_config()["min_confidence"] == d.min_confidence != l.min_confidence
    assert (trainer.loss_proposal.min_confidence, trainer.loss_proposal.nms_iou_threshold, trainer.loss_proposal.post_iou_threshold,
            trainer.loss_proposal.nms_max_output_size) == (l.min_confidence, l.nms_iou_threshold, l.post_iou_threshold,
                                                           l.nms_max_output_size)
    assert trainer.metric_proposal.max_batch_size == trainer.loss_proposal.max_batch_size == cfg.train.max_batch_size
    specs = trainer.weight_specs()
    assert set(specs) - set(inference.weight_specs()) == {"box_loss/moving_mean", "box_loss/moving_var"}
    w = trainer.init_weights(0)
    assert np.all(w["box_loss/moving_mean"] == F32(l.box_loss_beta)) and not w["box_loss/moving_var"].any()
    assert [trainer.get_layer(n).name for n in ("class_loss", "box_loss", "mask_loss", "seg_loss", "class_iou_metric")]
    with pytest.raises(RuntimeError, match="load_weights"):
        trainer([np.zeros((1, 64, 96, 3), np.uint8)] * 6)
    assert R.construct_masklab_networks(cfg)[0] is None                           # the default is unchanged


def test_trainer_outputs_shrink_with_the_head_groups():
    from masklab_hip import retinamasklab as R
    cfg = _small_config()
    bb, det, ins, sem = (R.build_backbone_network(cfg), R.build_detection_network(cfg), R.build_instance_network(cfg),
                         R.build_semantic_network(cfg))
    no_ins = R.construct_trainer_network(cfg, bb, detection_networks=det, semantic_networks=sem)
    assert "mask_loss" not in no_ins.output_names and "gt_masks" not in no_ins.input_names and len(no_ins.output_names) == 9
    only_sem = R.construct_trainer_network(cfg, bb, semantic_networks=sem, instance_networks=ins)
    assert only_sem.output_names == ["seg_loss", "other_road_iou_metric", "my_road_metric", "crack_iou_metric"]
    assert only_sem.input_names == ["images", "gt_seg", "gt_seg_exist"]
    assert list(inspect.signature(R.construct_trainer_network).parameters) == [
        "configuration", "backbone_network", "detection_networks", "semantic_networks", "instance_networks"]


def test_new_layers_mirror_the_reference_surface():
    import masklab_hip as M
    from masklab_hip import layers as L
    from masklab_hip import losses
    assert losses.__all__ == ["ClassLoss", "BoxLoss", "MaskLoss", "SegLoss"]
    reg = M.get_custom_objects()
    for name in losses.__all__:
        assert reg[name] is getattr(losses, name)
    for name in ("CalculateIOU", "AssignBoxes", "AssignMasks", "AssignSeg"):
        assert reg[name] is getattr(L, name)
    base = {"name": "x", "trainable": True}
    assert losses.ClassLoss(name="x").get_config() == {**base, "weight": 1., "alpha": .25, "gamma": 2.}
    assert losses.BoxLoss(name="x").get_config() == {**base, "momentum": .9, "weight": 1., "beta": .11, "use_adjust": False}
    assert losses.MaskLoss(name="x").get_config() == {**base, "weight": 1., "label_smoothing": 0, "max_batch_size": 64}
    assert losses.SegLoss(name="x").get_config() == {**base, "weight": 1., "label_smoothing": 0.}
    assert L.AssignBoxes(num_classes=5, name="x").get_config() == {**base, "num_classes": 5}
    assert L.AssignMasks(name="x").get_config() == {"name": "x", "trainable": False, "match_iou_threshold": 0.5}
    for cls in (losses.ClassLoss, losses.BoxLoss, losses.MaskLoss, losses.SegLoss):
        assert cls.from_config(cls(weight=3., name="y").get_config()).weight == 3.
    assert list(inspect.signature(losses.BoxLoss.__init__).parameters) == ["self", "weight", "momentum", "beta", "use_adjust", "kwargs"]
    assert "__init__" not in vars(L.AssignSeg) and "__init__" not in vars(L.CalculateIOU)      # the reference defines none
    box = losses.BoxLoss(beta=.2, name="box_loss")
    assert {k: v.shape for k, v in box.weight_specs().items()} == {"box_loss/moving_mean": (4,), "box_loss/moving_var": (4,)}


def test_new_layers_refuse_cpu_tensors():
    import torch
    from masklab_hip import layers as L
    from masklab_hip import losses
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.AssignBoxes(num_classes=5)([z(1, 2, 6), z(1, 8, 4, dtype=torch.int32)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.CalculateIOU()([z(2, 4), z(3, 4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.AssignMasks()([z(1, 2, 6), z(1, 2, 4, 4, 5), z(1, 2, 6), z(1, 2, 8, 8, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.AssignSeg()([z(1, 5, 5, 3), z(1, 9, 9, 3)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.ClassLoss()([z(1, 2, 5), z(1, 2, 5), z(1, 2, 1), z(1, 5)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.SegLoss()([z(1, 2, 2, 3), z(1, 2, 2, 3), z(1, 3)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.MaskLoss()([z(1, 2, 4, 4, dtype=torch.int32), z(1, 2, 4, 4, 5)])


def test_trainer_workspace_size_and_refusals_without_a_device():
    from masklab_hip import _lib
    lib = _lib.load()
    assert lib.ml_train_workspace_bytes(8, 5) >= 8 * 8 * 5 * 2 and lib.ml_train_workspace_bytes(0, 5) == 0
    # argument checks run before anything is launched: refused without a device
    assert lib.ml_train_best_prior_f32(None, None, 1, 1, 1, None, None, None) != 0 and b"null pointer" in lib.ml_last_error()
