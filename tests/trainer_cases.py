"""Fixtures of the trainer-forward tests (test infrastructure, not collected), shared by the CPU and the GPU tests: prior
tables, ground-truth box tables that contain every event of the AssignBoxes rule, RoI / mask tables for AssignMasks and the
semantic maps of AssignSeg.  Every generator checks in float64 what it promises (no crop or resize sample within 1e-4 of
0.5 other than exact halves), so exact equality of the assigned targets is a fair demand."""
import functools

import numpy as np

import trainer_ref as REF

NUM_CLASSES = 5
GUARD = 1e-4
# (cx, cy, w, h) on the 64 x 96 prior table: maxima tied over 2 / 4 / 20 priors (rows 0, 3, 2), 25 priors with IoU >= 0.5 to
# rows 0 AND 1, a forced positive at IoU 0.025 (row 2), IoU 0 everywhere (row 4 -> prior 0), 2 priors positive for row 0 inside
# row 5's ignore band
SIX_BOXES = [(40, 28, 40, 34), (41, 29, 40, 34), (16, 16, 5, 5), (8, 32, 32, 32), (500, 500, 10, 10), (48, 32, 64, 64)]


@functools.lru_cache(maxsize=None)
def priors(H, W):
    """The default configuration's prior table at H x W, int32 [A,4]."""
    from masklab_hip import ModelConfiguration, retinamasklab as R
    return R.build_detection_network(ModelConfiguration())[0].prior.anchors(H, W, 'same')


def _rows(boxes, classes):
    return np.array([(*b, c, 1.0) for b, c in zip(boxes, classes)], np.float32)


@functools.lru_cache(maxsize=None)
def boxes_small():
    """-> (gt_boxes [3,7,6], priors [1935,4]).  Image 1 has a -1 row BETWEEN valid rows, image 2 no valid row."""
    gt = np.full((3, 7, 6), -1, np.float32)
    gt[0, :6] = _rows(SIX_BOXES, [0, 1, 2, 3, 4, 0])
    gt[1, 0] = _rows([SIX_BOXES[0]], [2])[0]
    gt[1, 2] = _rows([SIX_BOXES[3]], [4])[0]
    gt[1, 5] = _rows([(70, 40, 30, 22)], [1])[0]
    pr = priors(64, 96)
    assert pr.shape == (1935, 4)
    return gt, pr


@functools.lru_cache(maxsize=None)
def boxes_large():
    """-> (gt_boxes [2,70,6], priors [25590,4]) at 256 x 320: G = 70 crosses the kernels' tile of 64 ground truths; image 0 is
    full, image 1 has -1 rows in the middle and at the end; two rows are copies of priors (IoU 1), one pair is a duplicate."""
    rng = np.random.default_rng(70)
    pr = priors(256, 320)
    assert pr.shape == (25590, 4)
    gt = np.full((2, 70, 6), -1, np.float32)
    for b, n in ((0, 70), (1, 41)):
        size = np.exp(rng.uniform(np.log(6), np.log(180), (n, 2)))
        rows = np.concatenate([rng.uniform(0, 320, (n, 1)), rng.uniform(0, 256, (n, 1)), size, rng.integers(0, NUM_CLASSES, (n, 1)),
                               np.ones((n, 1))], axis=1).astype(np.float32)
        where = np.arange(70) if n == 70 else np.sort(rng.choice(70, n, replace=False))
        gt[b, where] = rows
    gt[0, 66, :4] = pr[20000]
    gt[0, 3, :4] = pr[77]
    gt[0, 69, :4] = gt[0, 10, :4]                                   # the same box twice, classes as drawn
    return gt, pr


def predictions(gt, A, seed):
    """-> (cls_pred in (0, 1), loc_pred ~ N(0, 1), gt_boxes_exist with zeros) for a box table."""
    rng = np.random.default_rng(seed)
    B = gt.shape[0]
    cls_pred = rng.uniform(0, 1, (B, A, NUM_CLASSES)).astype(np.float32)
    cls_pred[0, :3] = [0, 1, 0.5, 1e-9, 1 - 1e-9]                   # the clip's two ends
    loc_pred = rng.normal(size=(B, A, 4)).astype(np.float32)
    exist = np.ones((B, NUM_CLASSES), np.float32)
    exist[0, 1] = 0
    exist[B - 1, 3] = 0
    return cls_pred, loc_pred, exist


# ----------------------------------------------------------------------------- AssignMasks
def _ellipse(H, W, box, squeeze=0.8):
    y, x = np.mgrid[:H, :W]
    return (((x - box[0]) / (squeeze * box[2] / 2)) ** 2 + ((y - box[1]) / (squeeze * box[3] / 2)) ** 2 <= 1)


def _shifted(box, iou):
    """`box` moved along x so that its IoU with itself is `iou`: (w - d) / (w + d) = iou."""
    d = box[2] * (1 - iou) / (1 + iou)
    return (box[0] + d, box[1], box[2], box[3])


def _guarded(roi, gt, masks, name):
    target, samples, matched = REF.assign_masks(roi, gt, masks, (28, 28), NUM_CLASSES, dtype=np.float64)
    near = np.abs(samples - 0.5)[matched]
    assert near.size and near.min() > GUARD, (name, float(near.min()))
    return matched


@functools.lru_cache(maxsize=None)
def masks_int8():
    """-> (roi_boxes [2,6,6], gt_boxes [2,3,6], gt_masks int8 [2,3,37,53]); image 0's last instance is padding (-1)."""
    H, W = 37, 53
    a, b0, b1, b2 = (18.3, 14.2, 21.4, 16.6), (30.5, 20.25, 30.2, 22.7), (10.1, 9.2, 13.7, 12.3), (40.0, 30.0, 20.3, 11.1)
    gt = np.full((2, 3, 6), -1, np.float32)
    gt[0, :2] = _rows([a, a], [1, 1])                               # two ground truths of equal IoU: the first wins
    gt[1] = _rows([b0, b1, b2], [3, 0, 2])
    masks = np.zeros((2, 3, H, W), np.int8)
    masks[0, 0] = _ellipse(H, W, a)
    masks[0, 1] = _ellipse(H, W, a, 0.5)
    masks[0, 2] = -1
    for g, box in enumerate((b0, b1, b2)):
        masks[1, g] = _ellipse(H, W, box, 0.9)
    roi = np.full((2, 6, 6), -1, np.float32)
    roi[0, 0] = (*a, 1, 0.9)                                        # equal to a ground truth
    roi[0, 1] = (*_shifted(a, 0.51), 1, 0.8)                        # IoU just above 0.5
    roi[0, 2] = (*_shifted(a, 0.49), 1, 0.7)                        # ... and just below
    roi[0, 4] = (*a, 2, 0.6)                                        # class mismatch at IoU 1   (row 3: a -1 row in the middle)
    roi[0, 5] = (25.0, 20.0, 30.0, 20.0, 1, 0.5)                    # an IoU well below the threshold
    roi[1, 0] = (*b0, 3, 0.9)
    roi[1, 1] = (43.0, 32.0, 26.0, 14.0, 2, 0.8)                    # reaches outside the mask: extrapolation
    roi[1, 3] = (*b1, 0, 0.7)
    roi[1, 4] = (5.0, 30.0, 6.0, 6.0, 4, 0.6)                       # nothing there
    matched = _guarded(roi, gt, masks, "masks_int8")
    assert matched.tolist() == [[True, True, False, False, False, False], [True, True, False, True, False, False]]
    return roi, gt, masks


@functools.lru_cache(maxsize=None)
def masks_uint8():
    """-> (roi_boxes [1,4,6], gt_boxes [1,2,6], gt_masks uint8 [1,2,64,96])."""
    H, W = 64, 96
    a, b = (40.3, 30.1, 50.7, 37.9), (70.2, 45.6, 30.3, 28.4)
    gt = _rows([a, b], [4, 2])[None]
    masks = np.stack([_ellipse(H, W, a), _ellipse(H, W, b, 0.7)])[None].astype(np.uint8)
    roi = np.full((1, 4, 6), -1, np.float32)
    roi[0, 0] = (*_shifted(a, 0.8), 4, 0.9)
    roi[0, 1] = (76.0, 49.0, 40.0, 32.0, 2, 0.8)                    # over the right and the bottom border
    roi[0, 2] = (*b, 2, 0.7)
    matched = _guarded(roi, gt, masks, "masks_uint8")
    assert matched.tolist() == [[True, True, True, False]]
    return roi, gt, masks


def mask_predictions(roi, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, roi.shape[:2] + (28, 28, NUM_CLASSES)).astype(np.float32)


# ----------------------------------------------------------------------------- AssignSeg
@functools.lru_cache(maxsize=None)
def seg_case(in_hw, out_hw, dtype):
    """-> (gt_seg [2,H,W,3] of `dtype`, gt_seg_exist [2,3] with a zero).  uint8 truth is 0 / 1; float32 truth is soft."""
    rng = np.random.default_rng(in_hw[0] * 100 + out_hw[0])
    shape = (2,) + tuple(in_hw) + (3,)
    gt = (rng.random(shape) < 0.5).astype(np.uint8) if dtype == "uint8" else rng.random(shape).astype(np.float32)
    _, resized = REF.assign_seg(gt, out_hw, dtype=np.float64)
    frac = resized - np.floor(resized)
    near = np.abs(frac - 0.5)
    assert near[near != 0].min() > GUARD, float(near[near != 0].min())
    exist = np.ones((2, 3), np.float32)
    exist[1, 0] = 0
    return gt, exist, int((near == 0).sum())


def seg_predictions(out_hw, seed):
    return np.random.default_rng(seed).uniform(0, 1, (2,) + tuple(out_hw) + (3,)).astype(np.float32)
