"""Drop-in for the reference's engine/metrics.py: ConfusionMatrixMetric, ClassBinaryIOU and DetectionIOUMetric with the
same constructor arguments and get_config keys.  Inputs are device tensors; every comparison and count runs in the integer
counting kernels of csrc/evaluate.hip (through masklab_hip.ops) and the closing formulas in float32 on the device as
well, so with counts below 2^24 each result is exact.  There is no CPU fallback."""
from . import keras_like as K


class ConfusionMatrixMetric(K.Layer):
    """engine/metrics.py:11-67.  inputs = [cls_true [B,A,C], cls_pred [B,A,C], mask [B,A]], float32 -> float32 scalars
    (precision, recall, accuracy, fmeasure).  Per anchor the argmax (first maximum, as tf.argmax); the prediction is
    background unless its row maximum > threshold, the truth unless mask == 0; anchors with mask == -1 are dropped."""

    def __init__(self, threshold=0.3, **kwargs):
        super().__init__(**kwargs)
        self.threshold = threshold

    def call(self, inputs, **kwargs):
        from . import ops
        cls_true, cls_pred, mask = inputs
        _, metrics = ops.confusion_matrix_metric(cls_true, cls_pred, mask, self.threshold)
        return tuple(metrics.unbind(0))

    def get_config(self):
        return {**super().get_config(), "threshold": self.threshold}


class ClassBinaryIOU(K.Layer):
    """engine/metrics.py:70-106.  inputs = [seg_true, seg_pred], both [B,H,W,C] float32, float16, int32 or uint8 -> a list
    of C float32 [B] tensors: intersection / union of the pixels > threshold per (image, class), 1 for an empty union."""

    def __init__(self, threshold=0.5, **kwargs):
        super().__init__(**kwargs)
        self.threshold = threshold

    def call(self, inputs, **kwargs):
        from . import ops
        seg_true, seg_pred = inputs
        _, iou = ops.class_binary_iou(seg_true, seg_pred, self.threshold)
        return list(iou.unbind(0))

    def get_config(self):
        return {**super().get_config(), "threshold": self.threshold}


class DetectionIOUMetric(K.Layer):
    """engine/metrics.py:109-165.  inputs = [proposed_boxes [B,n,6], gt_boxes [B,m,6]] (cx, cy, w, h, class id, confidence;
    rows padded with -1), float32 -> float32 [B] (precision, recall, fmeasure) at IoU > 0.5, bit for bit the arithmetic of
    oracle/metrics.py::detection_iou_metric."""

    def call(self, inputs, **kwargs):
        from . import ops
        proposed_boxes, gt_boxes = inputs
        return tuple(ops.detection_iou_metric(proposed_boxes, gt_boxes).unbind(0))


__all__ = ["ConfusionMatrixMetric", "ClassBinaryIOU", "DetectionIOUMetric"]
