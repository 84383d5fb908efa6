"""The reference's optimizers (engine/optimizers.py): RectifiedAdam, which engine/train.py trains with, and AdamW.  Same
constructor arguments, defaults and get_config() keys; a step is two HIP launches over every weight tensor at once
(ops.optimizer_step, csrc/optimizer.hip).  `lr` and `iterations` live on the device, as the reference's K.variables do: a
callback sets lr between steps with a stream-ordered fill, and a step captured into a graph replays with the values of its
replay.

    opt = RectifiedAdam(1e-4)
    opt.apply_gradients(params, grads)            # {name: device tensor}, the names of model.init_weights()

Not here: `constraint`, fp16 parameter copies, gradient reduction across devices.  A step updates Keras-layout tensors only: the packed forms the
kernels read follow them through ops.repack_weights (packings bound with DeviceConv.bind_master), or through load_weights;
folded (fold_bn) weights through load_weights alone."""
import numpy as np
import torch

from . import ops


class _Optimizer:
    kind = None                     # a key of ops.OPTIMIZER_KINDS

    def __init__(self, lr, beta_1, beta_2, epsilon, decay, weight_decay, **kwargs):
        if kwargs:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {sorted(kwargs)} (clipnorm / clipvalue are not built)")
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.decay = self.initial_decay = float(decay)
        self.weight_decay = float(weight_decay)
        self.init_lr = float(lr)
        self._lr, self._iterations = float(lr), 0        # until the first step names the device
        self._state = self._scalars = None
        self._table = ops.OptimizerTable()
        self._names, self._m, self._v = [], {}, {}
        self._pending = None                             # set_weights() before the first step

    # ---- lr and iterations: on the device once a step has named it (K.set_value / K.get_value of the reference)
    @property
    def lr(self):
        if self._state is None:
            return float(np.float32(self._lr))
        return float(ops.optimizer_state_lr(self._state).item())

    @lr.setter
    def lr(self, value):
        if self._state is None:
            self._lr = float(value)
        else:
            with torch.cuda.device(self._state.device):
                ops.fill_(ops.optimizer_state_lr(self._state), float(value))

    @property
    def iterations(self):
        return self._iterations if self._state is None else int(self._state[0].item())

    @property
    def scalars(self):
        """The scalars of the last step as the device holds them (_lib.OptScalars; a host read), None before the first."""
        return None if self._scalars is None else ops.optimizer_scalars_read(self._scalars)

    def _place(self, device):
        if self._state is None:
            self._state = ops.optimizer_state(device, self._iterations, self._lr)
            self._scalars = ops.optimizer_scalars_buffer(device)

    # ---- the step
    @staticmethod
    def _is_trainable(trainable, name):
        if trainable is None:
            return True
        return bool(trainable(name)) if callable(trainable) else name in trainable

    def apply_gradients(self, params, grads, trainable=None):
        """One step.  params, grads: {name: float32 device tensor}; every trainable name of `params` is updated in place
        from grads[name].  trainable: None (all), a set of names or a predicate; any other name is skipped entirely.  The
        moments of a name are created as zeros when it is first seen.  A trainable name without a gradient is a ValueError,
        as Keras raises for a None gradient."""
        names = [n for n in params if self._is_trainable(trainable, n)]
        missing = [n for n in names if grads.get(n) is None]
        if missing:
            raise ValueError(f"{type(self).__name__}: no gradient for {missing[:5]}{' ...' if len(missing) > 5 else ''} "
                             f"(a trainable weight the loss does not reach: leave it out of `trainable`)")
        quads, added = [], []
        for n in names:
            p = params[n]
            if n not in self._m and isinstance(p, torch.Tensor):
                self._m[n], self._v[n] = torch.zeros_like(p), torch.zeros_like(p)
                self._names.append(n)
                added.append(n)
            quads.append((p, grads[n], self._m.get(n), self._v.get(n)))
        try:
            device = next((q[0].device for q in quads if isinstance(q[0], torch.Tensor) and q[0].is_cuda), None)
            if self._state is None:
                if device is None:                       # no device to put lr and iterations on: ops words the refusal
                    ops.optimizer_check(quads)
                    raise RuntimeError(f"{type(self).__name__}: no device tensor among the parameters (no CPU fallback)")
                self._place(device)
            self._load_pending()
            ops.optimizer_step(self.kind, quads, self._table, self._state, self._scalars, self.beta_1, self.beta_2,
                               self.epsilon, self.initial_decay, self.weight_decay, self.init_lr)
        except Exception:
            for n in added:                              # a refused step leaves no moments behind
                self._names.remove(n)
                del self._m[n], self._v[n]
            raise

    # ---- Keras's optimizer weights: [iterations] + ms + vs, in the order the names were first seen
    def get_weights(self):
        return ([np.asarray(self.iterations, dtype=np.int64)] + [self._m[n].cpu().numpy() for n in self._names] +
                [self._v[n].cpu().numpy() for n in self._names])

    def set_weights(self, weights):
        """What get_weights() returned.  Before the first step the moments have no tensors yet: the values are kept and go
        into them, in order, as the first step creates them."""
        weights = [np.asarray(w) for w in weights]
        if len(weights) % 2 != 1:
            raise ValueError(f"{type(self).__name__}.set_weights: expected [iterations] + ms + vs, got {len(weights)} arrays")
        if self._state is None:
            self._iterations, self._pending = int(weights[0]), weights[1:]
            return
        self._pending = weights[1:]
        try:
            self._load_pending(int(weights[0]))
        finally:
            self._pending = None                         # (refused: nothing was changed, nothing is kept)

    def _load_pending(self, iterations=None):
        if self._pending is not None:
            k = len(self._pending) // 2
            if k != len(self._names):
                raise ValueError(f"{type(self).__name__}.set_weights: {k} moment pairs for {len(self._names)} weights")
            pairs = list(zip(self._names, self._pending[:k], self._pending[k:]))
            for n, m, v in pairs:
                for src in (m, v):
                    if tuple(src.shape) != tuple(self._m[n].shape):
                        raise ValueError(f"{type(self).__name__}.set_weights: {n} has shape {tuple(self._m[n].shape)}, got "
                                         f"{tuple(src.shape)}")
            for n, m, v in pairs:                        # nothing is changed unless everything fits
                self._m[n].copy_(torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)))
                self._v[n].copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)))
            self._pending = None
        if iterations is not None:
            self._state.copy_(ops.optimizer_state(self._state.device, iterations, self.lr))

    def get_config(self):
        return {"lr": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "decay": self.decay, "epsilon": self.epsilon,
                "weight_decay": self.weight_decay}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class AdamW(_Optimizer):
    """Adam with decoupled weight decay, as the reference writes it: p' = p - lr_t m' / (sqrt(v') + epsilon) - eta_t wd p with
    eta_t = lr / init_lr (the decay is taken from the weight as it was BEFORE the step, unlike torch.optim.AdamW)."""
    kind = "AdamW"

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, weight_decay=1e-4, epsilon=1e-8, decay=0., **kwargs):
        super().__init__(lr, beta_1, beta_2, epsilon, decay, weight_decay, **kwargs)


class RectifiedAdam(_Optimizer):
    """RAdam (arXiv 1908.03265) as the reference writes it: the unrectified momentum step while the length of the approximated
    SMA is at most 5 (the first 5 steps at beta_2 = 0.999), the rectified adaptive step after; weight_decay is decoupled and
    scaled by lr.  epsilon=None is Keras's K.epsilon() = 1e-7."""
    kind = "RectifiedAdam"

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0., weight_decay=0.0, **kwargs):
        super().__init__(lr, beta_1, beta_2, 1e-7 if epsilon is None else epsilon, decay, weight_decay, **kwargs)


__all__ = ["AdamW",
           "RectifiedAdam"]
