"""The reference's training callbacks (engine/callbacks.py): CyclicLR, the cyclical learning rate policy of arXiv 1506.01186
that engine/train.py drives RectifiedAdam with.  Host arithmetic; the only device work is the optimizer's lr fill.
(SaveInferenceModel is not built: there is no trained model to save yet.)"""
import numpy as np


class CyclicLR:
    """Cycles the learning rate between base_lr and max_lr, step_size iterations per half cycle.
    mode: "triangular" (constant amplitude), "triangular2" (halved every cycle) or "exp_range" (gamma ** iterations).
    scale_fn: a custom amplitude scale in [0, 1], evaluated on the cycle number (scale_mode="cycle") or on the iterations
    since the start (scale_mode="iterations"); `mode` is ignored then.
    Acts on `self.model.optimizer.lr` of whatever set_model() was given: any object with `.optimizer.lr`."""

    def __init__(self, base_lr=0.001, max_lr=0.006, step_size=2000., mode='triangular', gamma=1., scale_fn=None,
                 scale_mode='cycle'):
        self.model = None
        self.base_lr = base_lr
        self.max_lr = max_lr
        self.step_size = step_size
        self.mode = mode
        self.gamma = gamma
        if scale_fn is None:
            if mode not in ('triangular', 'triangular2', 'exp_range'):
                raise ValueError(f"CyclicLR: mode must be triangular, triangular2 or exp_range, got {mode!r}")
            self.scale_fn = {'triangular': lambda x: 1.,
                             'triangular2': lambda x: 1 / (2. ** (x - 1)),
                             'exp_range': lambda x: gamma ** x}[mode]
            self.scale_mode = 'iterations' if mode == 'exp_range' else 'cycle'
        else:
            self.scale_fn = scale_fn
            self.scale_mode = scale_mode
        self.clr_iterations = 0.
        self.trn_iterations = 0.
        self.history = {}

    def set_model(self, model):
        self.model = model

    def _reset(self, new_base_lr=None, new_max_lr=None, new_step_size=None):
        """Restart the cycle, optionally with new boundaries or step size."""
        if new_base_lr is not None:
            self.base_lr = new_base_lr
        if new_max_lr is not None:
            self.max_lr = new_max_lr
        if new_step_size is not None:
            self.step_size = new_step_size
        self.clr_iterations = 0.

    def clr(self):
        it, half = self.clr_iterations, self.step_size
        cycle = np.floor(it / (2 * half)) + 1                    # 1, 2, ...: 2 * step_size iterations each
        rise = max(0., 1 - abs(it / half - 2 * cycle + 1))       # 0 at a cycle's ends, 1 in its middle
        return self.base_lr + (self.max_lr - self.base_lr) * rise * self.scale_fn(cycle if self.scale_mode == 'cycle' else it)

    def on_train_begin(self, logs=None):
        self.model.optimizer.lr = self.base_lr if self.clr_iterations == 0 else self.clr()

    def on_batch_end(self, epoch, logs=None):
        self.trn_iterations += 1
        self.clr_iterations += 1
        self.history.setdefault('lr', []).append(self.model.optimizer.lr)
        self.history.setdefault('iterations', []).append(self.trn_iterations)
        for k, v in (logs or {}).items():
            self.history.setdefault(k, []).append(v)
        self.model.optimizer.lr = self.clr()


__all__ = ["CyclicLR"]
