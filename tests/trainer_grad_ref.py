"""The oracle of the loss gradients (test infrastructure, not collected), in two parts that owe each other nothing.

1.  A float64 torch restatement of the four loss layers, line by line from the reference's engine/losses.py (the tf.* call
    named beside each line), which torch autograd differentiates: the INDEPENDENT differentiator.  Python constants enter as
    the float32 values TensorFlow converts them to; tensors enter as given.  A count, a comparison and the read of an
    assigned variable carry no gradient in TensorFlow, and none here: tf.where / torch.where select, sums of masks do not
    depend on the prediction, and BoxLoss's beta is detached.
2.  The closed forms of include/masklab_hip.h ("Trainer backward: the losses") in float32 NumPy, the way the kernels of
    csrc/train_losses.hip evaluate them, and in float64 the magnitude S every comparison is scaled by: the same expression
    with the two cross-entropy terms ADDED in absolute value (for the focal and the smooth-L1 gradient nothing cancels and S
    is |gradient|).

`autograd(fn, pred, upstream)` returns (loss [B], d sum_b upstream[b] * loss[b] / d pred) of a restatement."""
import re

import numpy as np
import torch

F32 = np.float32
F64 = np.float64


def _c(v):
    """a Python constant as TensorFlow holds it in a float32 graph"""
    return float(F32(v))


EPS = _c(1e-7)                          # K.epsilon()
# trainer_cases.predictions(gt, A, BOX_SEED) gives the loc_pred of the boxes_small gradient cases: the smooth-L1 branch is
# discontinuous in the derivative, so no positive coordinate may sit within trainer_cases.GUARD of |d| = 1.5 beta for any beta in
# use (0.11 and three adjusted ones).  Seed 7 keeps 8.7e-4; the CPU test asserts it, seeds 4, 5, 9 and 15 fail it.
BOX_SEED = 7
ONE_MINUS_EPS = float(F32(1) - F32(1e-7))


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, F64))


# ----------------------------------------------------------------------------- 1. the restatement (torch, float64)
def split_neg_pos_mask(mask):                                                    # losses.py:251-269
    neg_mask = torch.where(mask == 1., torch.ones_like(mask), torch.zeros_like(mask))
    pos_mask = torch.where(mask == 0., torch.ones_like(mask), torch.zeros_like(mask))
    ignore_mask = torch.where(mask == -1., torch.zeros_like(mask), torch.ones_like(mask))
    return neg_mask, pos_mask, ignore_mask


def focal_loss(y_true, y_pred, gamma=2., alpha=.25):                              # losses.py:204-218
    y_pred = torch.clamp(y_pred, EPS, ONE_MINUS_EPS)                             # tf.clip_by_value: equality passes
    pt = torch.where(y_true == 1., y_pred, 1. - y_pred)
    loss = -torch.pow(1. - pt, _c(gamma)) * torch.log(pt)
    return _c(alpha) * loss


def smooth_l1(y_true, y_pred, beta=0.11):                                        # losses.py:221-234
    l1_loss = torch.abs(y_true - y_pred) - 0.5 * beta
    l2_loss = 0.5 * (y_true - y_pred) ** 2 / beta
    loss = torch.where(l1_loss < beta, l2_loss, l1_loss)
    return loss.mean(dim=-1)


def binary_cross_entropy(y_true, y_pred, label_smoothing=0.1):                   # losses.py:237-248
    y_true = _c(1 - label_smoothing) * y_true + _c(label_smoothing / 2.)
    return -(y_true * torch.log(y_pred + EPS) + (1 - y_true) * torch.log(1 - y_pred + EPS))


def class_loss(cls_true, cls_pred, mask, cls_exists, weight=1., alpha=.25, gamma=2.):    # ClassLoss.call, losses.py:21-41
    cls_true, cls_pred, mask, cls_exists = _t(cls_true), _t(cls_pred), _t(mask), _t(cls_exists)
    batch_size, num_classes = cls_exists.shape
    mask = mask.reshape(batch_size, -1, 1)
    cls_exists = cls_exists.reshape(batch_size, 1, num_classes)
    neg_mask, pos_mask, ignore_mask = split_neg_pos_mask(mask)
    cls_true = torch.where(cls_true != 0, torch.ones_like(cls_true), torch.zeros_like(cls_true))
    num_tot = (pos_mask + neg_mask).sum(dim=(1, 2))
    loss = focal_loss(cls_true, cls_pred, gamma, alpha)
    loss = loss * cls_exists
    loss = (ignore_mask * loss).sum(dim=(1, 2)) / (num_tot + EPS)
    return _c(weight) * loss


def box_loss(loc_true, loc_pred, mask, weight=1., beta=.11):
    """BoxLoss.call from `# smooth l1 loss` on (losses.py:99-104) with `beta` given: a float, or the four values the
    statistics produced -- a constant either way."""
    loc_true, loc_pred, mask = _t(loc_true), _t(loc_pred), _t(mask)
    mask = mask.reshape(mask.shape[0], -1, 1)
    beta = _c(beta) if np.isscalar(beta) else _t(beta).detach()
    neg_mask, pos_mask, ignore_mask = split_neg_pos_mask(mask)
    num_pos = pos_mask.sum(dim=(1, 2))
    loss = smooth_l1(loc_true, loc_pred, beta=beta)
    loss = (pos_mask.squeeze(-1) * loss).sum(dim=1) / (num_pos + EPS)
    return _c(weight) * loss


class BoxLoss:
    """BoxLoss with its two variables (losses.py:67-104); every call assigns them when use_adjust, and the beta read back
    from them is detached: `self.moving_mean - self.moving_var` under control_dependencies reads variables."""

    def __init__(self, weight=1., momentum=0.9, beta=.11, use_adjust=False):
        self.weight, self.momentum, self.beta, self.use_adjust = weight, momentum, beta, use_adjust
        self.moving_mean = torch.full((4,), _c(beta), dtype=torch.float64)
        self.moving_var = torch.zeros(4, dtype=torch.float64)
        self.last_beta = None

    def __call__(self, loc_true, loc_pred, mask):
        loc_true, loc_pred, mask = _t(loc_true), _t(loc_pred), _t(mask)
        if self.use_adjust:
            _, pos_mask, _ = split_neg_pos_mask(mask.reshape(mask.shape[0], -1, 1))
            offsets = torch.abs(loc_true - loc_pred) * pos_mask
            mean = offsets.mean(dim=(0, 1))
            var = ((offsets - mean) ** 2).mean(dim=(0, 1))
            next_mean = self.moving_mean * _c(self.momentum) + mean * _c(1 - self.momentum)
            next_var = self.moving_var * _c(self.momentum) + var * _c(1 - self.momentum)
            self.moving_mean, self.moving_var = next_mean.detach(), next_var.detach()          # .assign
            beta = torch.clamp(self.moving_mean - self.moving_var, _c(1e-3), _c(self.beta))
        else:
            beta = self.beta
        self.last_beta = beta
        return box_loss(loc_true, loc_pred, mask, self.weight, beta)


def mask_loss(mask_true, mask_pred, weight=1., label_smoothing=0.):              # MaskLoss.call, losses.py:126-159
    mask_pred = _t(mask_pred)
    mask_true = torch.from_numpy(np.asarray(mask_true)).long()
    batch_size, num_rois, h, w, num_classes = mask_pred.shape
    mask_classes = mask_true.amin(dim=(2, 3))
    one_hot = torch.nn.functional.one_hot(mask_true, num_classes + 1)[..., :-1]
    transposed_pred = mask_pred.permute(4, 0, 1, 2, 3)
    transposed_true = one_hot.permute(4, 0, 1, 2, 3)
    mask_indices = torch.nonzero(mask_classes < num_classes)                     # tf.where: rows (b, r)
    class_indices = mask_classes[mask_indices[:, 0], mask_indices[:, 1]]
    chosen_pred = transposed_pred[class_indices, mask_indices[:, 0], mask_indices[:, 1]]
    chosen_true = transposed_true[class_indices, mask_indices[:, 0], mask_indices[:, 1]].to(torch.float64)
    loss = binary_cross_entropy(chosen_true, chosen_pred, label_smoothing)
    # MoldBatch + the -1 -> 0 replacement: an image's chosen rows, zero rows for the rest
    molded = torch.zeros((batch_size, num_rois, h, w), dtype=torch.float64)
    slot = torch.zeros(batch_size, dtype=torch.long)
    rows = []
    for b in mask_indices[:, 0].tolist():
        rows.append(int(slot[b]))
        slot[b] += 1
    molded = molded.index_put((mask_indices[:, 0], torch.tensor(rows, dtype=torch.long)), loss)
    molded = molded.mean(dim=(2, 3))
    count = torch.count_nonzero(molded.detach(), dim=1) + 1
    molded = molded.sum(dim=1) / count.to(torch.float64)
    return _c(weight) * molded


def seg_loss(seg_true, seg_pred, seg_exist, weight=1., label_smoothing=0.):      # SegLoss.call, losses.py:179-193
    mask_true, mask_pred, mask_exists = _t(seg_true), _t(seg_pred), _t(seg_exist)
    loss = binary_cross_entropy(mask_true, mask_pred, label_smoothing)
    loss = loss.mean(dim=(1, 2))
    loss = mask_exists * loss
    loss = loss.mean(dim=1)
    return _c(weight) * loss


def default_upstream(B):
    """1 / B as the kernels get it: float32"""
    return np.full(B, F32(1.0) / F32(B), F32)


def autograd(fn, pred, upstream=None):
    """fn(pred tensor) -> loss [B].  -> (loss float64 [B], d sum_b upstream[b] * loss[b] / d pred, float64 like pred)"""
    x = torch.from_numpy(np.asarray(pred, F64).copy()).requires_grad_(True)
    loss = fn(x)
    up = default_upstream(loss.shape[0]) if upstream is None else upstream
    (loss * _t(up)).sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


def central_difference(fn, pred, upstream, where, h=1e-3):
    """The five-point central difference (error O(h^4)) of sum_b upstream[b] * fn(pred)[b] at the flat indices `where`."""
    base = np.asarray(pred, F64)
    up = _t(upstream)
    out = np.empty(len(where), F64)
    for k, i in enumerate(where):
        acc = 0.0
        for step, coef in ((-2, 1.0), (-1, -8.0), (1, 8.0), (2, -1.0)):
            x = base.copy()
            x.reshape(-1)[i] += step * h
            with torch.no_grad():
                acc += coef * float((fn(torch.from_numpy(x)) * up).sum())
        out[k] = acc / (12.0 * h)
    return out


# ----------------------------------------------------------------------------- 2. the closed forms (NumPy)
def _sigmoid_factor(pred, through_sigmoid):
    pred = np.asarray(pred, F32)
    return pred * (F32(1) - pred) if through_sigmoid else np.ones_like(pred)


def class_loss_grad(cls_true, cls_pred, mask, cls_exists, weight, alpha, gamma, upstream, through_sigmoid=False):
    """float32 [B,A,C]: c_b / (num_tot_b + eps) * keep * exists * d focal / d pred"""
    pred = np.asarray(cls_pred, F32)
    B = pred.shape[0]
    m = np.asarray(mask, F32).reshape(B, -1)
    eps, hi = F32(1e-7), F32(1) - F32(1e-7)
    num_tot = ((m == 1) | (m == 0)).sum(axis=1).astype(F64)
    scale = ((F32(weight) * np.asarray(upstream, F32)).astype(F64) / (num_tot + F64(eps))).astype(F32)
    on = np.asarray(cls_true, F32) != 0
    inside = (pred >= eps) & (pred <= hi)
    p = np.where(inside, pred, F32(0.5))                                         # a harmless value where the result is 0 anyway
    pt = np.where(on, p, F32(1) - p)
    q = np.where(on, F32(1) - p, p)
    lg = np.where(on, np.log(p), np.log1p(-p))
    w = np.power(q, F32(gamma) - F32(1))
    d = F32(alpha) * (F32(gamma) * w * lg - w * q / pt)
    d = np.where(on, d, -d)
    g = d * np.asarray(cls_exists, F32)[:, None, :] * scale[:, None, None]
    g = np.where(inside & (m != -1)[..., None], g, F32(0))
    return (g * _sigmoid_factor(pred, through_sigmoid)).astype(F32)


def box_loss_grad(loc_true, loc_pred, mask, weight, beta, upstream):
    """float32 [B,A,4]; beta a scalar or the call's four values"""
    t, p = np.asarray(loc_true, F32), np.asarray(loc_pred, F32)
    B = p.shape[0]
    m = np.asarray(mask, F32).reshape(B, -1)
    beta = np.broadcast_to(np.asarray(beta, F32), (4,))
    num_pos = (m == 0).sum(axis=1).astype(F64)
    scale = ((F32(weight) * np.asarray(upstream, F32)).astype(F64) / (num_pos + F64(F32(1e-7)))).astype(F32) * F32(0.25)
    d = t - p
    quad = np.abs(d) - F32(0.5) * beta < beta
    dl = np.where(quad, -d / beta, -np.sign(d))
    return np.where((m == 0)[..., None], dl * scale[:, None, None], F32(0)).astype(F32)


def _bce_parts(t, p, label_smoothing):
    """the two terms of dBCE/dp = -(first - second), float32"""
    eps = F32(1e-7)
    y = F32(1 - label_smoothing) * np.asarray(t, F32) + F32(label_smoothing / 2.)
    return y / (p + eps), (F32(1) - y) / (F32(1) - p + eps)


def mask_loss_grad(mask_true, mask_pred, weight, label_smoothing, upstream, through_sigmoid=False, with_scale=False):
    """float32 [B,R,h,w,C] (and S, float64)"""
    import trainer_ref as REF
    pred = np.asarray(mask_pred, F32)
    B, R, h, w, C = pred.shape
    classes = np.asarray(mask_true).min(axis=(2, 3))
    g = np.zeros(pred.shape, F32)
    S = np.zeros(pred.shape, F64)
    for b in range(B):
        chosen = np.flatnonzero(classes[b] < C)
        losses = []
        for r in chosen:
            c = classes[b, r]
            loss = REF.binary_cross_entropy((mask_true[b, r] == c).astype(F32), pred[b, r, :, :, c], label_smoothing)
            losses.append(F32(loss.sum(dtype=F64) / (h * w)))
        nz = np.count_nonzero(np.asarray(losses, F32))
        scale = F32(F64(F32(weight) * F32(upstream[b])) / F64(nz + 1) / F64(h * w))
        for r in chosen:
            c = classes[b, r]
            p = pred[b, r, :, :, c]
            first, second = _bce_parts(mask_true[b, r] == c, p, label_smoothing)
            factor = _sigmoid_factor(p, through_sigmoid)
            g[b, r, :, :, c] = -(first - second) * scale * factor
            S[b, r, :, :, c] = (first.astype(F64) + second.astype(F64)) * abs(F64(scale)) * factor.astype(F64)
    return (g, S) if with_scale else g


def seg_loss_grad(seg_true, seg_pred, seg_exist, weight, label_smoothing, upstream, through_sigmoid=False, with_scale=False):
    """float32 [B,H,W,C] (and S, float64)"""
    pred = np.asarray(seg_pred, F32)
    B, H, W, C = pred.shape
    scale = ((F32(weight) * np.asarray(upstream, F32)).astype(F64) / (F64(C) * F64(H * W))).astype(F32)
    per = np.asarray(seg_exist, F32) * scale[:, None]
    first, second = _bce_parts(seg_true, pred, label_smoothing)
    factor = _sigmoid_factor(pred, through_sigmoid)
    g = (-(first - second) * per[:, None, None, :] * factor).astype(F32)
    S = (first.astype(F64) + second.astype(F64)) * np.abs(per.astype(F64))[:, None, None, :] * factor.astype(F64)
    return (g, S) if with_scale else g


# ----------------------------------------------------------------------------- the bar
BAR = 1e-5      # |got - want| <= BAR * S: a term is about a dozen float32 operations plus logf / powf, each within a couple
#                 of ulp (2^-24): about 1e-6 of S, with the tenfold room the forward tests leave


def check(got, want, S=None, name=""):
    """got float32 against autograd's float64 `want` under |got - want| <= BAR * S (S = |want| where nothing cancels), exact
    zeros where want is exactly 0.  Prints and returns the observed maximum of |err| / S."""
    got, want = np.asarray(got), np.asarray(want, F64)
    assert got.dtype == F32 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    S = np.abs(want) if S is None else np.asarray(S, F64)
    assert np.isfinite(got).all(), f"{name}: a non-finite gradient"
    zero = want == 0
    assert not got[zero].any(), f"{name}: {np.count_nonzero(got[zero])} non-zero elements where the gradient is exactly 0"
    err = np.abs(got.astype(F64) - want)
    ratio = np.max(err[~zero] / S[~zero]) if (~zero).any() else 0.0
    print(f"{name}: {np.count_nonzero(~zero)} of {want.size} non-zero, max |err| / S = {ratio:.3g} (bar {BAR:g})")
    assert (err <= BAR * S).all(), f"{name}: max |err| / S = {ratio:.3g} over the bar {BAR:g}"
    return ratio


def raised(fn, *args):
    """-> (the exception type fn(*args) raises or None, its message with the op's name taken out): what a `*_loss_grad` op
    and its forward twin must agree on for the same bad arguments"""
    try:
        fn(*args)
    except Exception as e:                                           # noqa: BLE001  (the comparison is the test)
        return type(e), re.sub(r"\b(\w+_loss)(_grad)?\b", "OP", str(e))
    return None, ""
