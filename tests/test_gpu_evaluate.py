"""GPU tests of the evaluation kernels (csrc/evaluate.hip), the metric layers (masklab_hip/metrics.py) and the evaluation
loop (masklab_hip/evaluate.py) against the NumPy restatement tests/evaluate_ref.py and oracle/metrics.py.  Every
comparison is exact equality; the kernels are launched twice and must give the same bits.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import backbone_cases as MODEL_CASES
from backbone_refs import SERESNET34 as BACKBONE_REF
import evaluate_cases as CASES
import evaluate_ref as REF


def _twice(fn):
    first, second = host(fn()), host(fn())
    np.testing.assert_array_equal(first, second, err_msg="two launches differ")
    return first


# ----------------------------------------------------------------------------- the three evaluation kernels
@pytest.mark.parametrize("size", [28, 14])
def test_mask_area_and_pair_kernels(size):
    from masklab_hip import ops
    det, ins = CASES.predictions(size)
    _, gt_ins, _ = CASES.ground_truth()
    pairs = CASES.all_pairs(2, det.shape[1], gt_ins.shape[1])
    d_gt = dev(gt_ins)
    area = _twice(lambda: ops.eval_mask_area(d_gt))
    np.testing.assert_array_equal(area, REF.mask_areas(gt_ins))
    d_det, d_ins, d_area, d_pairs = dev(det), dev(ins), dev(area), dev(pairs)
    got = _twice(lambda: ops.eval_mask_pairs(d_det, d_ins, d_gt, d_area, d_pairs))
    np.testing.assert_array_equal(got, REF.pair_stats(det, ins, gt_ins, pairs))
    np.testing.assert_array_equal(got[-5:], -1)
    np.testing.assert_array_equal(got, ops.eval_reference_host(det=det, ins=ins, gt=gt_ins, pairs=pairs)[1])


def test_mask_area_off_a_16_byte_boundary_and_uint8():
    from masklab_hip import ops
    rng = np.random.default_rng(3)
    n = 5 * 33 * 7
    buf = dev((rng.random(16 + n) < 0.5).astype(np.uint8) * rng.integers(1, 256, 16 + n).astype(np.uint8))
    for lo in (0, 1, 15):
        gt = buf[lo:lo + n].view(1, 5, 33, 7)
        np.testing.assert_array_equal(_twice(lambda: ops.eval_mask_area(gt)), REF.mask_areas(host(gt)))


def test_pairs_walk_a_full_hd_box_in_many_blocks():
    """1080 x 1920, one box over the whole frame and one clipped at two borders: 128 blocks per pair."""
    from masklab_hip import ops
    rng = np.random.default_rng(7)
    Hh, Ww = 1080, 1920
    det = np.array([[[960, 540, 1920, 1080, 0, 90], [1800, 1000, 400, 300, 1, 80]]], np.int32)
    ins = np.kron(rng.integers(0, 2, (1, 2, 7, 7)), np.ones((4, 4), np.int64)).astype(np.int32)
    gt = (rng.random((1, 2, Hh, Ww)) < 0.5).astype(np.uint8)
    pairs = np.array([[0, 0, 0], [0, 1, 1], [0, 1, 0]], np.int32)
    d_gt = dev(gt)
    area = ops.eval_mask_area(d_gt)
    np.testing.assert_array_equal(host(area), REF.mask_areas(gt))
    d_det, d_ins, d_pairs = dev(det), dev(ins), dev(pairs)
    got = _twice(lambda: ops.eval_mask_pairs(d_det, d_ins, d_gt, area, d_pairs))
    np.testing.assert_array_equal(got, REF.pair_stats(det, ins, gt, pairs))
    assert got[0, 1] > 1 << 20


@pytest.mark.parametrize("shape", [(2, CASES.H, CASES.W, 3), (2, 37, 53, 3), (1, 1080, 1920, 3), (3, 5, 7, 5), (1, 1, 1, 1)])
def test_semantic_counts_kernel(shape):
    from masklab_hip import ops
    rng = np.random.default_rng(shape[1])
    pr = CASES.semantic_prediction(shape)
    pr[0, 0, 0, :] = -3
    gt = (rng.random(shape) < 0.4).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    d_pr, d_gt = dev(pr), dev(gt)
    got = _twice(lambda: ops.eval_semantic_counts(d_pr, d_gt))
    np.testing.assert_array_equal(got, REF.semantic_counts(pr, gt))
    if shape[1] == 1080:
        assert got.min() > 1 << 16                          # counts beyond 16 bits, from many blocks


# ----------------------------------------------------------------------------- the three metric layers
def test_detection_iou_metric_has_the_oracle_bits():
    from masklab_hip.metrics import DetectionIOUMetric
    from oracle.metrics import detection_iou_metric
    rng = np.random.default_rng(11)
    gt = np.full((3, 4, 6), -1, np.float32)
    gt[0, :3] = np.concatenate([rng.uniform(20, 80, (3, 2)), rng.uniform(5, 40, (3, 2)), rng.integers(0, 5, (3, 1)), np.ones((3, 1))], 1)
    gt[1, :4] = np.concatenate([rng.uniform(20, 80, (4, 2)), rng.uniform(5, 40, (4, 2)), rng.integers(0, 5, (4, 1)), np.ones((4, 1))], 1)
    prop = np.full((3, 7, 6), -1, np.float32)                 # image 2 has no ground truth at all
    for b, k in ((0, 5), (1, 7), (2, 3)):
        prop[b, :k] = np.concatenate([rng.uniform(20, 80, (k, 2)), rng.uniform(5, 40, (k, 2)), rng.integers(0, 5, (k, 1)),
                                      rng.uniform(0.1, 1, (k, 1))], 1)
    prop[0, :3, :4] = gt[0, :3, :4] + rng.uniform(-1.5, 1.5, (3, 4)).astype(np.float32)      # hits, near hits
    prop[1, :4, :4] = gt[1, :4, :4] * np.float32(1.21)                                        # IoUs around the 0.5 line
    layer = DetectionIOUMetric()
    d_prop, d_gt = dev(prop), dev(gt)
    got = [_twice(lambda i=i: layer([d_prop, d_gt])[i]) for i in range(3)]
    want = detection_iou_metric(prop, gt)
    for name, g, w in zip(("precision", "recall", "fmeasure"), got, want):
        assert g.dtype == np.float32 and g.shape == (3,)
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=name)
    assert 0 < want[0][0] < 1 or 0 < want[0][1] < 1, "fixture: every proposal hits or none does"
    assert want[1][2] == 0 and want[2][2] == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.int32, np.uint8])
def test_class_binary_iou(dtype):
    from masklab_hip.metrics import ClassBinaryIOU
    rng = np.random.default_rng(13)
    shape = (2, 37, 53, 3)
    if np.issubdtype(dtype, np.floating):
        t, p = rng.random(shape).astype(dtype), rng.random(shape).astype(dtype)
        t[0, 0, :8, 0] = p[0, 0, :8, 0] = 0.5                  # exactly the threshold: not above it
    else:
        t, p = rng.integers(0, 2, shape).astype(dtype), rng.integers(0, 2, shape).astype(dtype)
    t[1, :, :, 2] = p[1, :, :, 2] = 0                          # an all-empty class
    layer = ClassBinaryIOU()
    d_t, d_p = dev(t), dev(p)
    want = REF.class_binary_iou(t, p)
    assert len(want) == 3 and want[2][1] == 1 and 0 < want[0][0] < 1
    for c in range(3):
        got = _twice(lambda: layer([d_t, d_p])[c])
        assert got.dtype == np.float32 and got.shape == (2,)
        np.testing.assert_array_equal(got.view(np.uint32), want[c].view(np.uint32))
    from masklab_hip import ops
    counts = host(ops.class_binary_iou(d_t, d_p, 0.5)[0])
    np.testing.assert_array_equal(counts[..., 0], (t.astype(np.float64) > 0.5).sum(axis=(1, 2)))
    uneven = ClassBinaryIOU(threshold=0.25)([d_t[:, :5, :3].contiguous(), d_p[:, :5, :3].contiguous()])      # 45 elements per image
    for c, w in enumerate(REF.class_binary_iou(t[:, :5, :3], p[:, :5, :3], 0.25)):
        np.testing.assert_array_equal(host(uneven[c]).view(np.uint32), w.view(np.uint32))


def test_confusion_matrix_metric():
    from masklab_hip.metrics import ConfusionMatrixMetric
    rng = np.random.default_rng(17)
    B, A, C = 2, 1003, 5
    cls_true = np.eye(C, dtype=np.float32)[rng.integers(0, C, (B, A))]
    cls_pred = rng.random((B, A, C)).astype(np.float32) * np.float32(0.6)
    agree = rng.random((B, A)) < 0.5
    cls_pred[agree] += cls_true[agree] * np.float32(0.5)
    cls_pred[:, ::7] = np.float32(0.25)                        # every class ties (below the threshold)
    cls_pred[:, 1::7] = np.float32(0.1)
    cls_pred[:, 1::7, 1:3] = np.float32(0.9)                   # classes 1 and 2 tie for the maximum: class 1 wins
    cls_pred[:, 2::7] *= np.float32(0.3)                       # rows below the threshold
    cls_true[:, 3::50] = 0                                     # an all-zero truth row: argmax 0
    mask = rng.choice(np.array([0, 1, -1], np.float32), (B, A), p=[0.5, 0.3, 0.2])
    layer = ConfusionMatrixMetric()
    d = [dev(cls_true), dev(cls_pred), dev(mask)]
    got = [_twice(lambda i=i: layer(d)[i]) for i in range(4)]
    want, counts = REF.confusion_matrix_metric(cls_true, cls_pred, mask)
    from masklab_hip import ops
    np.testing.assert_array_equal(host(ops.confusion_matrix_metric(*d, 0.3)[0]), counts)
    assert min(counts) > 0 and sum(counts) == int((mask != -1).sum())
    for name, g, w in zip(("precision", "recall", "accuracy", "fmeasure"), got, want):
        assert g.dtype == np.float32 and g.shape == ()
        assert g.view(np.uint32) == np.float32(w).view(np.uint32), name


# ----------------------------------------------------------------------------- the loop, end to end
FRAMES = (2, 200, 328, 3)
SHIFT = 3


@pytest.fixture(scope="module")
def shipped():
    """The shipped SE-ResNet-34 configuration with order-stable weights, so that detections exist -> (deploy model,
    dataset whose ground truth is made of the model's own fp32 predictions)."""
    from masklab_hip import retinamasklab as R
    with pytest.MonkeyPatch.context() as patch:
        BACKBONE_REF.patch(patch)
        cfg = MODEL_CASES.shipped_se_config("seresnet34", ('C3', 'C4', 'C5', 'P6'))
        cfg.postprocess.resolution = FRAMES[1:3]                 # the frames are already at the working size
        model, w, images = MODEL_CASES.order_stable_fixture(cfg, FRAMES, seed=5)
        model.load_weights(w, "cuda:0")
        deploy = R.construct_deploy_network(cfg, model)
        predictions = [deploy.predict(images[b:b + 1]) for b in range(FRAMES[0])]
        G = max(p[0].shape[1] for p in predictions) + 1
        gt_det = np.full((FRAMES[0], G, 6), -1.0, np.float32)
        gt_ins = np.full((FRAMES[0], G, FRAMES[1], FRAMES[2]), -1, np.int8)
        gt_sem = np.zeros(FRAMES, np.uint8)
        for b, (det, ins, sem) in enumerate(predictions):
            valid = np.flatnonzero(det[0, :, -1] >= 0)
            assert b > 0 or len(valid) >= 3, "fixture produced too few detections"
            for slot, j in enumerate(valid):
                gt_det[b, slot] = det[0, j]
                canvas = REF.pasted_mask(det[0, j], ins[0, j], FRAMES[1], FRAMES[2])
                gt_ins[b, slot] = 0
                gt_ins[b, slot, :, SHIFT:] = canvas[:, :-SHIFT]
            gt_sem[b, :, SHIFT:] = sem[0, :, :-SHIFT]
        gt_det[0, 0], gt_ins[0, 0] = -1, -1                      # one dropped
        gt_det[0, 1, 4] = (gt_det[0, 1, 4] + 1) % len(CASES.INSTANCE_LABELS)          # one relabelled
        gt_ins[1] = -1                                           # image 1 has no instance labels: its crack row is not counted
        gt_det[1] = -1
        yield deploy, CASES.ToyDataset(images, gt_det, gt_ins, gt_sem), predictions


def test_evaluate_equals_the_restated_loop(shipped):
    from masklab_hip.evaluate import evaluate
    deploy, dataset, predictions = shipped
    got = evaluate(deploy, dataset)
    batches = [(*predictions[b], *(dataset[b:b + 1][k] for k in ("detection", "instance", "semantic"))) for b in range(len(dataset))]
    want = REF.evaluate_ref(CASES.INSTANCE_LABELS, CASES.SEMANTIC_LABELS, batches)
    print({k: v for k, v in got.items() if v["counts"]})
    assert list(got) == list(want) == CASES.INSTANCE_LABELS + CASES.SEMANTIC_LABELS
    for key in want:
        assert got[key] == want[key], key
    assert any(got[k]["counts"] > 0 and 0 < got[k]["miou"] < 1 for k in CASES.INSTANCE_LABELS)
    assert got["my_road"]["counts"] == 2 and got["crack"]["counts"] == 1


def test_evaluate_runs_under_the_split_operand_conv_math(shipped):
    from masklab_hip import ops
    from masklab_hip.evaluate import evaluate
    deploy, dataset, _ = shipped
    exact = evaluate(deploy, dataset)
    ops.set_conv_math("f32x3")
    try:
        got = evaluate(deploy, dataset)
    finally:
        ops.set_conv_math("f32")
    assert list(got) == list(exact)
    for key in got:                                              # what the mode costs, in the reference's own numbers: printed, not gated
        print(f"{key:12s} f32 miou {exact[key]['miou']:.6f} ({exact[key]['counts']:.0f})   f32x3 miou {got[key]['miou']:.6f} "
              f"({got[key]['counts']:.0f})")
