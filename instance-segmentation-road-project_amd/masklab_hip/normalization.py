"""GroupNormalization -- drop-in for reference engine/normalization.py (the Keras layer),
running the chunk-norm HIP kernel (csrc/groupnorm.hip) and its backward (csrc/groupnorm_grad.hip).

The reference layer with axis=-1 on NHWC does NOT group channels: it reshapes [N,H,W,C]
row-major to [N,G,H,W,C/G] and normalises over axes (2,3,4) (normalization.py:123-143), i.e.
each sample's flat H*W*C vector is cut into G contiguous chunks; gamma/beta are indexed
g*(C/G) + (c mod C/G) (:151-156).  That exact behaviour is reproduced.
"""
import numpy as np

from . import ops
from .keras_like import Layer


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


__all__ = ["GroupNormalization"]
