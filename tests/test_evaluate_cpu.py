"""CPU tests of the evaluation loop and the metric layers' host side: ml_eval_reference_host -- the per-thread code of the
mask-area, mask-pair and semantic kernels in CPU loops -- against the NumPy restatement (tests/evaluate_ref.py), the host
box matching, the result table of a toy dataset, and the drop-in surface of masklab_hip.metrics.  Every comparison is
exact equality."""
import inspect

import numpy as np
import pytest

import evaluate_cases as CASES
import evaluate_ref as REF


@pytest.fixture(scope="module")
def truth():
    return CASES.ground_truth()


@pytest.mark.parametrize("size", [28, 14])
def test_areas_and_pair_statistics_match_the_restatement(size, truth):
    from masklab_hip import ops
    det, ins = CASES.predictions(size)
    _, gt_ins, _ = truth
    pairs = CASES.all_pairs(2, det.shape[1], gt_ins.shape[1])
    area, got, _ = ops.eval_reference_host(det=det, ins=ins, gt=gt_ins, pairs=pairs)
    np.testing.assert_array_equal(area, REF.mask_areas(gt_ins))
    assert area[0, 0] > 0 and area[0, 1] == 0 and area[0, 2] == CASES.H * CASES.W      # int8 -1 pixels count as set
    want = REF.pair_stats(det, ins, gt_ins, pairs)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[-5:], -1)                                           # an index out of range
    pred_area = {i: int(got[i * 3 + 1, 1]) for i in range(len(CASES.BOXES))}              # against the empty mask: union = area
    assert pred_area[5] > 0 and pred_area[9] == 0 and pred_area[10] == 1 and pred_area[11] == 0
    assert all(0 < pred_area[i] < CASES.BOXES[i][2] * CASES.BOXES[i][3] for i in (0, 1, 2, 3, 4, 6, 8))
    if size == 28:
        assert pred_area[CASES.HALF_ROW] == 0             # every sample is exactly 0.5: none counts
    else:
        assert pred_area[CASES.HALF_ROW] == 14 * 7        # 14 x 14 from 14 x 14 is the identity: the stripes themselves


def test_unaligned_mask_rows_take_the_scalar_head_and_tail():
    """H*W = 97*131 is odd, so every second mask starts off a 16-byte boundary; a view shifted by one byte moves them all."""
    from masklab_hip import ops
    rng = np.random.default_rng(3)
    buf = (rng.random(1 + 5 * 33 * 7) < 0.5).astype(np.uint8) * rng.integers(1, 256, 1 + 5 * 33 * 7).astype(np.uint8)
    for lo in (0, 1):
        gt = buf[lo:lo + 5 * 33 * 7].reshape(1, 5, 33, 7)
        np.testing.assert_array_equal(ops.eval_reference_host(gt=gt)[0], REF.mask_areas(gt))
    tiny = np.ones((1, 2, 1, 3), np.uint8)                # masks shorter than 16 bytes
    np.testing.assert_array_equal(ops.eval_reference_host(gt=tiny)[0], [[3, 3]])


@pytest.mark.parametrize("shape", [(2, CASES.H, CASES.W, 3), (2, 37, 53, 3), (3, 5, 7, 5), (1, 1, 1, 1), (2, 1, 2, 16)])
def test_semantic_counts_match_the_restatement(shape):
    from masklab_hip import ops
    rng = np.random.default_rng(shape[1])
    pr = CASES.semantic_prediction(shape)
    pr[0, 0, 0, :] = -3                                                                   # not above 0.5
    gt = (rng.random(shape) < 0.4).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    got = ops.eval_reference_host(pr_sem=pr, gt_sem=gt)[2]
    np.testing.assert_array_equal(got, REF.semantic_counts(pr, gt))
    assert got.shape == (shape[0], shape[3], 2)


def test_reference_host_refuses_bad_arguments():
    from masklab_hip import ops
    with pytest.raises(RuntimeError, match="C <= 16"):
        ops.eval_reference_host(pr_sem=np.zeros((1, 2, 2, 17), np.int32), gt_sem=np.zeros((1, 2, 2, 17), np.uint8))
    with pytest.raises(RuntimeError, match="LDS"):                    # 128 x 128 = 16384 > ML_EVAL_MAX_MASK
        ops.eval_reference_host(det=np.zeros((1, 1, 6), np.int32), ins=np.zeros((1, 1, 128, 128), np.int32),
                                gt=np.zeros((1, 1, 4, 4), np.uint8), pairs=np.zeros((1, 3), np.int32))


@pytest.mark.parametrize("name", sorted(CASES.MATCHING))
def test_box_matching(name):
    from masklab_hip.evaluate import match_boxes
    pr, gt, want = CASES.MATCHING[name]
    pr, gt = np.asarray(pr, np.int32), np.asarray(gt, np.float32)
    got = list(zip(*match_boxes(pr, gt)))
    assert got == want == REF.match(pr, gt)


def _toy(truth, size=28):
    det, ins = CASES.predictions(size)
    ins[0, 3] = 0                        # matched to the empty ground-truth mask: an empty union
    gt_det, gt_ins, gt_sem = truth
    sem = CASES.semantic_prediction(gt_sem.shape)
    return det, ins, sem, gt_det, gt_ins, gt_sem


def test_result_table_of_a_two_image_dataset(truth):
    from evaluate_cases import HostReferenceEvaluator
    batch = _toy(truth)
    want = REF.evaluate_ref(CASES.INSTANCE_LABELS, CASES.SEMANTIC_LABELS, [batch])
    whole = HostReferenceEvaluator(CASES.INSTANCE_LABELS, CASES.SEMANTIC_LABELS)
    whole.update(*batch)
    by_image = HostReferenceEvaluator(CASES.INSTANCE_LABELS, CASES.SEMANTIC_LABELS)
    for b in range(2):
        by_image.update(*(a[b:b + 1] for a in batch))
    assert whole.result() == by_image.result() == want
    assert list(want) == CASES.INSTANCE_LABELS + CASES.SEMANTIC_LABELS
    assert want['car']['counts'] == 1 and 0 < want['car']['iou'] < 1          # the 56 x 56 box on the 0 / 255 mask
    assert want['manhole'] == {"iou": 0.0, "counts": 1.0, "miou": 0.0}       # the empty union counts with IoU 0
    assert want['my_road']['counts'] == 2 and want['crack']['counts'] == 1    # image 1 has no instance labels: no crack row
    assert want['other_road']['miou'] == want['other_road']['iou'] / (2 + 1e-7)


def test_image_without_detections(truth):
    """the deploy model returns a single -1 row for it"""
    from evaluate_cases import HostReferenceEvaluator
    _, _, sem, gt_det, gt_ins, gt_sem = _toy(truth)
    batch = (np.full((1, 1, 6), -1, np.int32), np.zeros((1, 1, 28, 28), np.int32), sem[:1], gt_det[:1], gt_ins[:1], gt_sem[:1])
    ev = HostReferenceEvaluator(CASES.INSTANCE_LABELS, CASES.SEMANTIC_LABELS)
    ev.update(*batch)
    assert ev.result() == REF.evaluate_ref(CASES.INSTANCE_LABELS, CASES.SEMANTIC_LABELS, [batch])
    assert all(ev.result()[k]['counts'] == 0 for k in CASES.INSTANCE_LABELS) and ev.result()['crack']['counts'] == 1


def test_evaluator_refuses_what_it_cannot_count():
    from masklab_hip.evaluate import Evaluator
    with pytest.raises(ValueError, match="duplicates"):
        Evaluator(['crack'], ['road', 'crack'], device="cpu")
    assert Evaluator._pairs(np.zeros((0, 1, 6), np.int32), np.zeros((0, 1, 6))).shape == (0, 3)      # an empty batch


def test_metric_layers_mirror_the_reference_surface():
    import masklab_hip as M
    from masklab_hip import metrics
    assert metrics.__all__ == ["ConfusionMatrixMetric", "ClassBinaryIOU", "DetectionIOUMetric"]
    reg = M.get_custom_objects()
    for name in metrics.__all__:
        assert reg[name] is getattr(metrics, name)
    for cls, default in ((metrics.ConfusionMatrixMetric, 0.3), (metrics.ClassBinaryIOU, 0.5)):
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters) == ["self", "threshold", "kwargs"] and sig.parameters["threshold"].default == default
        assert cls().get_config()["threshold"] == default and cls(threshold=0.7, name="m").get_config() == \
            {"name": "m", "trainable": True, "threshold": 0.7}
        assert cls.from_config(cls(0.2).get_config()).threshold == 0.2
    assert "__init__" not in vars(metrics.DetectionIOUMetric)                 # the reference defines none
    assert set(metrics.DetectionIOUMetric(name="d").get_config()) == {"name", "trainable"}


def test_metric_layers_refuse_cpu_tensors():
    import torch
    from masklab_hip import metrics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.ClassBinaryIOU()([torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.DetectionIOUMetric()([torch.zeros(1, 2, 6), torch.zeros(1, 2, 6)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.ConfusionMatrixMetric()([torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), torch.zeros(1, 2)])


def test_restated_metric_layers_on_hand_counted_inputs():
    """the NumPy restatements the GPU tests compare against, on inputs small enough to count by hand"""
    t = np.zeros((1, 2, 2, 2), np.float32)
    p = np.zeros((1, 2, 2, 2), np.float32)
    t[0, :, :, 0] = [[1, 1], [0, 0]]
    p[0, :, :, 0] = [[1, 0], [1, 0]]
    iou = REF.class_binary_iou(t, p)
    assert iou[0][0] == np.float32(1) / np.float32(3) and iou[1][0] == 1                 # the empty class reads 1
    cls_true = np.array([[[1, 0], [0, 1], [0, 1], [1, 0], [1, 0]]], np.float32)
    cls_pred = np.array([[[.9, .1], [.2, .8], [.5, .5], [.1, .2], [.9, 0]]], np.float32)
    mask = np.array([[0, 0, 0, 1, -1]], np.float32)
    (_, _, accuracy, _), counts = REF.confusion_matrix_metric(cls_true, cls_pred, mask)
    assert counts == [2, 1, 0, 1]            # tie -> class 0 != 1: fp; background below the threshold: tn; the last is ignored
    assert accuracy == np.float32(3) / (np.float32(4) + np.float32(1e-7))
