"""GroupNormalization -- drop-in for reference engine/normalization.py (the Keras layer),
running the chunk-norm HIP kernel (csrc/groupnorm.hip) and its backward (csrc/groupnorm_grad.hip).

The reference layer with axis=-1 on NHWC does NOT group channels: it reshapes [N,H,W,C]
row-major to [N,G,H,W,C/G] and normalises over axes (2,3,4) (normalization.py:123-143), i.e.
each sample's flat H*W*C vector is cut into G contiguous chunks; gamma/beta are indexed
g*(C/G) + (c mod C/G) (:151-156).  That exact behaviour is reproduced.
"""
import numpy as np

from . import ops
from .keras_like import Layer, _check_f32_training


class GroupNormalization(Layer):
    def __init__(self, groups=32, axis=-1, epsilon=1e-5, center=True, scale=True,
                 beta_initializer="zeros", gamma_initializer="ones", beta_regularizer=None,
                 gamma_regularizer=None, beta_constraint=None, gamma_constraint=None, **kwargs):
        super().__init__(**kwargs)
        if axis not in (-1, 3):
            raise NotImplementedError("GroupNormalization: only axis=-1 (NHWC) is on the hot path")
        self.supports_masking = True
        self.groups = groups
        self.axis = axis
        self.epsilon = epsilon
        self.center = center
        self.scale = scale
        self.beta_initializer = beta_initializer
        self.gamma_initializer = gamma_initializer
        self.beta_regularizer = beta_regularizer
        self.gamma_regularizer = gamma_regularizer
        self.beta_constraint = beta_constraint
        self.gamma_constraint = gamma_constraint
        self.gamma = self.beta = None

    def build(self, input_shape):
        dim = input_shape[self.axis]
        # same checks / messages as reference normalization.py:78-92
        if dim is None:
            raise ValueError('Axis ' + str(self.axis) + ' of input tensor should have a defined dimension '
                             'but the layer received an input with shape ' + str(input_shape) + '.')
        if dim < self.groups:
            raise ValueError('Number of groups (' + str(self.groups) + ') cannot be '
                             'more than the number of channels (' + str(dim) + ').')
        if dim % self.groups != 0:
            raise ValueError('Number of groups (' + str(self.groups) + ') must be a '
                             'multiple of the number of channels (' + str(dim) + ').')
        self.dim = int(dim)
        # synthetic-weight init draws non-trivial gamma/beta so parity tests exercise the indexing
        if self.scale:
            self.add_weight("gamma", (dim,), "uniform", low=0.5, high=1.5)
        if self.center:
            self.add_weight("beta", (dim,), "normal", stddev=0.1)
        self.built = True
        return input_shape

    def _load_own(self, weights, device):
        import torch
        self.gamma = torch.from_numpy(self._get(weights, "gamma")).to(device) if self.scale else None
        self.beta = torch.from_numpy(self._get(weights, "beta")).to(device) if self.center else None

    def _own_device_params(self):
        if (self.scale and self.gamma is None) or (self.center and self.beta is None):
            raise RuntimeError(f"layer '{self.name}' has no weights loaded")
        out = {}                                             # the vectors the kernels read: no copy, no re-pack
        if self.scale:
            out[f"{self.name}/gamma"] = self.gamma
        if self.center:
            out[f"{self.name}/beta"] = self.beta
        return out

    def call(self, inputs, fuse_relu=False, inplace=False, **kwargs):
        self._check_loaded(inputs.shape)
        return ops.groupnorm_chunk(inputs, self.gamma, self.beta, self.groups, self.epsilon, relu=fuse_relu,
                                   out=inputs if inplace else None)

    @staticmethod
    def call_multi(layers, inputs, inplace=False, lives=None, partials=None):
        """The same layers applied to their own inputs in ONE launch pair (the un-shared towers normalise five pyramid
        levels at every depth, reference engine/layers/detection.py:124,194): results identical to calling each,
        whatever the shapes.
        lives: per input None or (device int32 [1], slots per image) -- a fixed-capacity RoI batch whose samples past
        max(1, live) per image do not exist and are skipped."""
        probs = []
        lives = lives if lives is not None else [None] * len(inputs)
        partials = partials if partials is not None else [None] * len(inputs)   # per input None or (float64 pairs, per chunk)
        for layer, x, live, part in zip(layers, inputs, lives, partials):
            layer._check_loaded(x.shape)
            probs.append(dict(x=x, gamma=layer.gamma, beta=layer.beta, groups=layer.groups, eps=layer.epsilon,
                              out=x if inplace else None, live=live, partials=part))
        return ops.groupnorm_chunk_multi(probs)

    def _check_loaded(self, shape):
        if not self.built:
            self.build(tuple(shape))
        if (self.scale and self.gamma is None) or (self.center and self.beta is None):
            raise RuntimeError(f"layer '{self.name}' has no weights loaded")

    def _grads(self, dgamma, dbeta):
        """the weights this layer has (`scale` / `center`)"""
        return {k: v for k, v, has in (("gamma", dgamma, self.scale), ("beta", dbeta, self.center)) if has}

    def backward(self, inputs, grad_outputs, fuse_relu=False, input_relu=False, inplace=False, stats=None):
        """The layer's backward (ops.groupnorm_chunk_grad), float32 only.
        inputs: what the layer was CALLED on.  The inference forward normalises in place and so destroys it: a caller that
        wants gradients calls the layer with inplace=False and keeps `inputs`.  grad_outputs: the gradient at the layer's
        output; fuse_relu: as in that call.  input_relu: `inputs` is a ReLU's output and the gradient is wanted in front of
        that ReLU (the tower unit Conv3x3 + ReLU -> GroupNormalization).  inplace: write the result over grad_outputs.
        -> (grad_inputs, {"gamma": ..., "beta": ...}) with the weights the layer has."""
        self._check_loaded(inputs.shape)
        dx, dgamma, dbeta = ops.groupnorm_chunk_grad(inputs, grad_outputs, self.gamma, self.beta, self.groups, self.epsilon,
                                                     relu=fuse_relu, input_relu=input_relu, stats=stats,
                                                     out=grad_outputs if inplace else None)
        return dx, self._grads(dgamma, dbeta)

    @staticmethod
    def backward_multi(layers, inputs, grad_outputs, fuse_relu=False, input_relu=False, inplace=False):
        """backward() of several layers on their own inputs in ONE launch set (the counterpart of call_multi: the towers run
        depth-major over five pyramid levels): results identical to calling each, whatever the shapes.
        -> list of (grad_inputs, {...})"""
        probs = []
        for layer, x, dy in zip(layers, inputs, grad_outputs):
            layer._check_loaded(x.shape)
            probs.append(dict(x=x, dy=dy, gamma=layer.gamma, beta=layer.beta, groups=layer.groups, eps=layer.epsilon,
                              relu=fuse_relu, input_relu=input_relu, out=dy if inplace else None))
        return [(dx, layer._grads(dgamma, dbeta))
                for layer, (dx, dgamma, dbeta) in zip(layers, ops.groupnorm_chunk_grad_multi(probs))]

    def get_config(self):
        config = {
            'groups': self.groups, 'axis': self.axis, 'epsilon': self.epsilon, 'center': self.center,
            'scale': self.scale, 'beta_initializer': self.beta_initializer,
            'gamma_initializer': self.gamma_initializer, 'beta_regularizer': self.beta_regularizer,
            'gamma_regularizer': self.gamma_regularizer, 'beta_constraint': self.beta_constraint,
            'gamma_constraint': self.gamma_constraint,
        }
        base = super().get_config()
        return dict(list(base.items()) + list(config.items()))

    def compute_output_shape(self, input_shape):
        return input_shape


class BatchNormalization(Layer):
    """tf.keras.layers.BatchNormalization on NHWC tensors as a layer of its own (csrc/batchnorm.hip): what
    the reference's train_waist_tune / train_all stages run above the freeze depth.  training=True normalises with the
    statistics of the batch and moves moving_mean / moving_variance toward them on the device; training=False reads the moving
    statistics on the device.  The weights carry Keras's names (gamma, beta, moving_mean, moving_variance): a converted
    checkpoint loads by name.  The backbones still fold their BatchNormalizations into the convs (packing.fold_bn); this
    layer is not wired into them yet."""

    def __init__(self, axis=-1, momentum=0.99, epsilon=1e-3, center=True, scale=True, beta_initializer="zeros",
                 gamma_initializer="ones", moving_mean_initializer="zeros", moving_variance_initializer="ones",
                 beta_regularizer=None, gamma_regularizer=None, beta_constraint=None, gamma_constraint=None, **kwargs):
        super().__init__(**kwargs)
        if axis not in (-1, 3):
            raise NotImplementedError("BatchNormalization: only axis=-1 (NHWC) is on the hot path")
        self.axis = axis
        self.momentum = momentum
        self.epsilon = epsilon
        self.center = center
        self.scale = scale
        self.beta_initializer = beta_initializer
        self.gamma_initializer = gamma_initializer
        self.moving_mean_initializer = moving_mean_initializer
        self.moving_variance_initializer = moving_variance_initializer
        self.beta_regularizer = beta_regularizer
        self.gamma_regularizer = gamma_regularizer
        self.beta_constraint = beta_constraint
        self.gamma_constraint = gamma_constraint
        self.gamma = self.beta = self.moving_mean = self.moving_variance = None

    def build(self, input_shape):
        dim = input_shape[self.axis]
        if dim is None:
            raise ValueError('Axis ' + str(self.axis) + ' of input tensor should have a defined dimension '
                             'but the layer received an input with shape ' + str(input_shape) + '.')
        self.dim = int(dim)
        # the synthetic-weight init of the folded BatchNormalizations (keras_like.Conv2D.bn_specs): non-trivial values
        if self.scale:
            self.add_weight("gamma", (dim,), "uniform", low=0.5, high=1.5)
        if self.center:
            self.add_weight("beta", (dim,), "normal", stddev=0.1)
        self.add_weight("moving_mean", (dim,), "normal", stddev=0.1)
        self.add_weight("moving_variance", (dim,), "uniform", low=0.5, high=1.5)
        self.built = True
        return input_shape

    def _load_own(self, weights, device):
        import torch
        up = lambda key: torch.from_numpy(np.array(self._get(weights, key), np.float32)).to(device)
        self.gamma = up("gamma") if self.scale else None
        self.beta = up("beta") if self.center else None
        self.moving_mean, self.moving_variance = up("moving_mean"), up("moving_variance")

    def _check_loaded(self, shape):
        if not self.built:
            self.build(tuple(shape))
        if self.moving_mean is None:
            raise RuntimeError(f"layer '{self.name}' has no weights loaded")

    def _own_device_params(self):
        _check_f32_training(f"BatchNormalization.device_params ('{self.name}')")
        if self.moving_mean is None:
            raise RuntimeError(f"layer '{self.name}' has no weights loaded")
        return self._params()

    def state(self):
        """The two moving vectors, the device tensors the kernels update in place: not parameters, no gradient."""
        if self.moving_mean is None:
            raise RuntimeError(f"layer '{self.name}' has no weights loaded")
        return {f"{self.name}/moving_mean": self.moving_mean, f"{self.name}/moving_variance": self.moving_variance}

    def get_weights_host(self):
        """{full weight name: ndarray} of all the layer's weights as they stand on the device (a host read)."""
        both = dict(self._params(), **self.state())
        return {k: v.detach().cpu().numpy().copy() for k, v in both.items()}

    def _params(self):
        """gamma / beta, the vectors the kernels read: no copy, no re-pack"""
        return {f"{self.name}/{k}": v for k, v, has in (("gamma", self.gamma, self.scale), ("beta", self.beta, self.center))
                if has}

    def _train(self, x, fuse_relu, residual, out):
        _check_f32_training(f"BatchNormalization ('{self.name}', training=True)")
        self._check_loaded(x.shape)
        return ops.batchnorm_train(x, self.gamma, self.beta, self.moving_mean, self.moving_variance, self.momentum,
                                   self.epsilon, relu=fuse_relu, residual=residual, out=out)

    def call(self, inputs, training=False, fuse_relu=False, residual=None, inplace=False, **kwargs):
        """training=False: the moving statistics, read on the device.  training=True: the batch's statistics, and the moving
        ones move (call_with_tape's bits, nothing kept for a backward).  inplace: y over inputs."""
        out = inputs if inplace else None
        if training:
            return self._train(inputs, fuse_relu, residual, out)[0]
        self._check_loaded(inputs.shape)
        return ops.batchnorm_infer(inputs, self.gamma, self.beta, self.moving_mean, self.moving_variance, self.epsilon,
                                   relu=fuse_relu, residual=residual, out=out)

    def call_with_tape(self, inputs, fuse_relu=False, residual=None):
        """call(training=True), out of place, and what backward() needs: the input, the saved (mean_b, r) and, with a fused
        ReLU, the output (the mask is decided on it).  -> (y, tape)"""
        y, saved, batch_mean, batch_var = self._train(inputs, fuse_relu, residual, None)
        tape = {"x": inputs, "y": y if fuse_relu else None, "saved": saved, "relu": bool(fuse_relu),
                "residual": residual is not None, "batch_mean": batch_mean, "batch_var": batch_var}
        return y, tape

    def backward(self, tape, grad_outputs, inplace=False, need_residual_grad=None):
        """The layer's backward (ops.batchnorm_grad).  tape: call_with_tape's; grad_outputs: the gradient at the layer's
        output; inplace: write the result over grad_outputs.  need_residual_grad: None = as the forward had a residual.
        -> (grad_inputs, grad_residual | None, {"gamma": ..., "beta": ...} with the weights the layer has)"""
        _check_f32_training(f"BatchNormalization.backward ('{self.name}')")
        if need_residual_grad is None:
            need_residual_grad = tape["residual"]
        dx, dres, dgamma, dbeta = ops.batchnorm_grad(tape["x"], grad_outputs, tape["saved"], self.gamma, y=tape["y"],
                                                     relu=tape["relu"], out=grad_outputs if inplace else None,
                                                     want_residual_grad=need_residual_grad)
        grads = {k: v for k, v, has in (("gamma", dgamma, self.scale), ("beta", dbeta, self.center)) if has}
        return dx, dres, grads

    def get_config(self):
        config = {
            'axis': self.axis, 'momentum': self.momentum, 'epsilon': self.epsilon, 'center': self.center,
            'scale': self.scale, 'beta_initializer': self.beta_initializer, 'gamma_initializer': self.gamma_initializer,
            'moving_mean_initializer': self.moving_mean_initializer,
            'moving_variance_initializer': self.moving_variance_initializer, 'beta_regularizer': self.beta_regularizer,
            'gamma_regularizer': self.gamma_regularizer, 'beta_constraint': self.beta_constraint,
            'gamma_constraint': self.gamma_constraint,
        }
        base = super().get_config()
        return dict(list(base.items()) + list(config.items()))

    def compute_output_shape(self, input_shape):
        return input_shape


__all__ = ["GroupNormalization", "BatchNormalization"]
