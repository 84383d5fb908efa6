"""Setup of the training-step tests (test infrastructure, not collected): the reference's default configuration -- plain
towers, no SqueezeExcite, ResNet-50 -- with every head one unit deep, at 2 x 64 x 96, and the batch of
tests/test_gpu_trainer.py's `models` fixture (its fourth ground-truth row fixed instead of taken from the oracle)."""
import numpy as np

from masklab_hip import ModelConfiguration, keras_like as K, retinamasklab as R

SHAPE = (2, 64, 96, 3)
F32 = np.float32
LOSSES = ("class_loss", "box_loss", "mask_loss", "seg_loss")


def config(**detection):
    cfg = ModelConfiguration()
    cfg.detection.num_depth = cfg.instance.num_depth = cfg.semantic.num_depth = 1
    for k, v in detection.items():
        setattr(cfg.detection, k, v)
    return cfg


def build(cfg=None):
    """-> (trainer, inference) sharing their layers"""
    K.clear_session()
    return R.construct_masklab_networks(cfg or config(), with_trainer=True)


def _ellipse(H, W, box, squeeze=0.8):
    cx, cy, w, h = box[:4]
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((xx - cx) / (squeeze * w / 2)) ** 2 + ((yy - cy) / (squeeze * h / 2)) ** 2) <= 1).astype(np.int8)


def inputs():
    rng = np.random.default_rng(7)
    images = np.random.default_rng(64 + 96).integers(0, 256, SHAPE, dtype=np.uint8)
    gt_boxes = np.full((2, 4, 6), -1, F32)
    gt_boxes[0, 0] = (40, 28, 40, 34, 1, 1)
    gt_boxes[0, 2] = (70, 40, 30, 22, 3, 1)                          # a -1 row between valid rows
    gt_boxes[1, 1] = (20, 30, 24, 36, 0, 1)
    gt_boxes[1, 3] = (60, 30, 20, 20, 2, 1)
    gt_masks = np.full((2, 4, 64, 96), -1, np.int8)
    for b, g in ((0, 0), (0, 2), (1, 1), (1, 3)):
        gt_masks[b, g] = _ellipse(64, 96, gt_boxes[b, g])
    return dict(images=images, gt_boxes=gt_boxes, gt_boxes_exist=np.array([[1, 1, 0, 1, 1], [1, 1, 1, 1, 1]], F32),
                gt_masks=gt_masks, gt_seg=(rng.random(SHAPE) < 0.5).astype(np.uint8),
                gt_seg_exist=np.array([[1, 1, 1], [1, 0, 1]], F32))


def loss_sum(trainer, outputs, names=LOSSES):
    """The sum over `names` of the batch means of the losses among a call's outputs, float64 on the host."""
    by = dict(zip(trainer.output_names, outputs))
    return float(sum(np.mean(by[n].detach().cpu().numpy().astype(np.float64)) for n in names))


def hand_weight_grads(trainer, batch, upstream=None):
    """The composition train_on_batch is held to: the forward with tapes, loss_and_gradients' gradients at the pre-activations,
    the five backwards called by hand.  -> (outputs, {name: gradient})"""
    grads, tapes = {}, {}
    outs = trainer._forward(batch, dict(upstream=dict(upstream or {}), through_sigmoid=True, grads=grads, tapes=tapes))
    _, _, cls, loc = trainer.detection_networks
    mask = trainer.instance_networks[3]
    aspp, seg = trainer.semantic_networks
    wg = {}
    wg.update(cls.backward(tapes[cls.name], grads["cls_pred"])[1])
    wg.update(loc.backward(tapes[loc.name], grads["loc_pred"])[1])
    wg.update(mask.backward(tapes[mask.name], grads["roi_masks"], need_dx=False)[1])
    (d_aspp, _), g = seg.backward(tapes[seg.name], grads["seg_pred"], need_dx=(True, False))
    wg.update(g)
    wg.update(aspp.backward(tapes[aspp.name], d_aspp, need_dx=False)[1])
    return outs, wg
