"""Drop-in for the reference's engine/losses.py: ClassLoss, BoxLoss, MaskLoss and SegLoss with the same constructor
arguments and get_config keys.  Inputs are float32 device tensors; every term and every sum runs in the kernels of
csrc/train_losses.hip (through masklab_hip.ops): float32 terms as the reference writes them, float64 sums in a fixed
order, so two calls give the same bits.  `call` is the forward.  `call_with_grad(inputs, upstream=None,
through_sigmoid=False)` returns (loss [B], grad): the same loss bit for bit and, from the same pass of the same kernel,
the gradient of sum_b upstream[b] * loss[b] with respect to the layer's prediction -- upstream None is 1 / B, the K.mean the
reference compiles; through_sigmoid gives the gradient at the output conv's pre-activation.  These layers stop there: the head
groups' own `backward`s take the gradients on (the FPN and the backbone have none yet).  No CPU fallback."""
import numpy as np
import torch

from . import keras_like as K
from . import ops


class ClassLoss(K.Layer):
    """engine/losses.py:12-50, focal loss.  inputs = [cls_true [B,A,C], cls_pred [B,A,C], assign_mask [B,A,1], cls_exists
    [B,C]] -> float32 [B]: the focal terms (predictions clipped to [eps, 1 - eps], truth binarised by != 0) times cls_exists,
    summed over the anchors that are not ignored, over (#positive + #negative + eps), times weight."""

    def __init__(self, weight=1., alpha=.25, gamma=2., **kwargs):
        self.weight = weight
        self.alpha = alpha
        self.gamma = gamma
        super().__init__(**kwargs)

    def _op_args(self, inputs):
        cls_true, cls_pred, mask, cls_exists = inputs
        return cls_true, cls_pred, mask, cls_exists.to(torch.float32), self.weight, self.alpha, self.gamma

    def call(self, inputs, **kwargs):
        return ops.class_loss(*self._op_args(inputs))

    def call_with_grad(self, inputs, upstream=None, through_sigmoid=False):
        """-> (loss [B], d / d cls_pred [B,A,C]); ignored anchors and classes that do not exist get zeros."""
        return ops.class_loss_grad(*self._op_args(inputs), upstream=upstream, through_sigmoid=through_sigmoid)

    def get_config(self):
        return {**super().get_config(), "weight": self.weight, "alpha": self.alpha, "gamma": self.gamma}


class BoxLoss(K.Layer):
    """engine/losses.py:53-114, (adjusted) smooth L1.  inputs = [loc_true [B,A,4], loc_pred [B,A,4], assign_mask [B,A,1]] ->
    float32 [B].  With use_adjust the layer owns two device vectors, `moving_mean` (initialised to beta) and `moving_var`
    (zeros), and updates them with `momentum` on EVERY call, as the reference does -- validation included.  They are
    weights `<name>/moving_mean` and `<name>/moving_var`, optional in a weight dict: an inference checkpoint has neither
    and the initialisers apply."""

    def __init__(self, weight=1., momentum=0.9, beta=.11, use_adjust=False, **kwargs):
        self.momentum = momentum
        self.weight = weight
        self.beta = beta
        self.use_adjust = use_adjust
        super().__init__(**kwargs)
        self.state = None                   # float32 [8] on the device: moving_mean, moving_var
        self.build(None)

    def build(self, input_shape):
        self.add_weight("moving_mean", (4,), "constant", value=self.beta)
        self.add_weight("moving_var", (4,), "constant", value=0.)
        self.built = True
        return input_shape

    def _load_own(self, weights, device):
        vals = []
        for key in ("moving_mean", "moving_var"):
            vals.append(self._get(weights, key) if f"{self.name}/{key}" in weights else self._specs[key].make(None))
        self.state = torch.from_numpy(np.concatenate(vals).astype(np.float32)).to(device)

    @property
    def moving_mean(self):
        return None if self.state is None else self.state[:4]

    @property
    def moving_var(self):
        return None if self.state is None else self.state[4:]

    def _op_args(self, inputs):
        loc_true, loc_pred, mask = inputs
        if self.state is None or self.state.device != loc_true.device:
            self._load_own({}, loc_true.device)
        return loc_true, loc_pred, mask, self.weight, self.momentum, self.beta, self.use_adjust, self.state

    def call(self, inputs, **kwargs):
        return ops.box_loss(*self._op_args(inputs))

    def call_with_grad(self, inputs, upstream=None, through_sigmoid=False):
        """-> (loss [B], d / d loc_pred [B,A,4]), zeros off the positive anchors.  The moving statistics move once, as by
        `call`; beta is a constant of the gradient.  loc_pred is a linear output: through_sigmoid must stay False."""
        if through_sigmoid:
            raise ValueError("BoxLoss: loc_pred is not a sigmoid output, there is no through_sigmoid gradient")
        return ops.box_loss_grad(*self._op_args(inputs), upstream=upstream)

    def get_config(self):
        return {**super().get_config(), "momentum": self.momentum, "weight": self.weight, "beta": self.beta,
                "use_adjust": self.use_adjust}


class MaskLoss(K.Layer):
    """engine/losses.py:117-168.  inputs = [mask_true int32 [B,R,h,w] (AssignMasks), mask_pred [B,R,h,w,C]] -> float32 [B]:
    an RoI's class is the minimum of its target; for the RoIs with a class < C the mean binary cross entropy of that class
    channel; per image their sum over (the number with a non-zero loss + 1), times weight.  B <= 32 (MoldBatch)."""

    def __init__(self, weight=1., label_smoothing=0, max_batch_size=64, **kwargs):
        self.weight = weight
        self.label_smoothing = label_smoothing
        self.max_batch_size = max_batch_size
        super().__init__(**kwargs)

    def _op_args(self, inputs):
        mask_true, mask_pred = inputs
        if mask_pred.shape[0] > 32:
            raise ValueError("MaskLoss: MoldBatch supports at most 32 images per call (reference misc.py:275)")
        return mask_true, mask_pred, self.weight, self.label_smoothing

    def call(self, inputs, **kwargs):
        return ops.mask_loss(*self._op_args(inputs))

    def call_with_grad(self, inputs, upstream=None, through_sigmoid=False):
        """-> (loss [B], d / d mask_pred [B,R,h,w,C]): non-zero in the class channel of the selected RoIs only."""
        return ops.mask_loss_grad(*self._op_args(inputs), upstream=upstream, through_sigmoid=through_sigmoid)

    def get_config(self):
        return {**super().get_config(), "weight": self.weight, "label_smoothing": self.label_smoothing,
                "max_batch_size": self.max_batch_size}


class SegLoss(K.Layer):
    """engine/losses.py:171-201.  inputs = [mask_true [B,H,W,C], mask_pred [B,H,W,C], mask_exists [B,C]] -> float32 [B]: the
    binary cross entropy's mean over (H, W) per class, times mask_exists, mean over the classes, times weight."""

    def __init__(self, weight=1., label_smoothing=0., **kwargs):
        self.weight = weight
        self.label_smoothing = label_smoothing
        super().__init__(**kwargs)

    def _op_args(self, inputs):
        mask_true, mask_pred, mask_exists = inputs
        return mask_true, mask_pred, mask_exists.to(torch.float32), self.weight, self.label_smoothing

    def call(self, inputs, **kwargs):
        return ops.seg_loss(*self._op_args(inputs))

    def call_with_grad(self, inputs, upstream=None, through_sigmoid=False):
        """-> (loss [B], d / d mask_pred [B,H,W,C])."""
        return ops.seg_loss_grad(*self._op_args(inputs), upstream=upstream, through_sigmoid=through_sigmoid)

    def get_config(self):
        return {**super().get_config(), "weight": self.weight, "label_smoothing": self.label_smoothing}


__all__ = ["ClassLoss", "BoxLoss", "MaskLoss", "SegLoss"]
