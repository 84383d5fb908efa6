"""Regenerates tests/golden/senet_layers.json: the layer inventory of the reference's SE-ResNet-50 / SE-ResNeXt-50
backbones, recorded from the reference's own builder.  Run from the repository root with the reference tree at hand:

    python tests/golden/make_senet_golden.py /path/to/reference

It loads thirdparty/classification_models/models/senet.py and _common_blocks.py by path on a recording stand-in of the
Keras namespace (no TensorFlow, no network, `weights=None`, bytecode writing off so nothing is left in the reference
tree), builds `seresnet50` and `seresnext50` at 1024 x 1024 the way load_backbone does (engine/backbone/base.py:220-246),
and reads the two BACKBONE_LAYERS entries from base.py with `ast` (that module imports TensorFlow).  The file holds names
and shapes only: per model the ordered (Keras auto name, class, output channels, kernel shape) of every weighted layer,
the unit and output shape of every Activation, and the tap dict.  Nothing on the GPU side reads it."""
import ast
import importlib.util
import json
import os
import re
import sys
import types

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
SIZE = 1024
REPETITIONS = (3, 4, 6, 3)


class Tensor:
    def __init__(self, h, w, c):
        self.shape = (h, w, c)

    def __getitem__(self, idx):
        if any(i is None for i in idx):                       # expand_dims: x[:, None, None, :]
            return Tensor(1, 1, self.shape[2])
        ch = idx[3]
        return Tensor(self.shape[0], self.shape[1], len(range(*ch.indices(self.shape[2]))))


class Recorder:
    def __init__(self):
        self.counts, self.weighted, self.activations, self.unit = {}, [], [], "stem"

    def name(self, cls):
        base = re.sub("([a-z])([A-Z])", r"\1_\2", re.sub("(.)([A-Z][a-z0-9]+)", r"\1_\2", cls)).lower()   # Keras
        n = self.counts.get(base, 0)
        self.counts[base] = n + 1
        return base if n == 0 else f"{base}_{n}"


def make_keras(rec):
    """Stand-ins of the Keras layers senet.py / _common_blocks.py use: shape propagation and Keras' auto names."""

    def pair(v):
        return (v, v) if isinstance(v, int) else tuple(v)

    class Layer:
        def __init__(self, *args, **kwargs):
            self.args, self.kwargs = args, kwargs
            self.name = kwargs.get("name") or rec.name(type(self).__name__)

    class Conv2D(Layer):
        def __call__(self, x):
            filters, k = self.args[0], pair(self.args[1])
            s = pair(self.kwargs.get("strides", 1))
            assert self.kwargs.get("padding", "valid") == "valid"
            rec.weighted.append([self.name, "Conv2D", filters, [k[0], k[1], x.shape[2], filters],
                                 bool(self.kwargs.get("use_bias", True)), rec.unit])
            return Tensor((x.shape[0] - k[0]) // s[0] + 1, (x.shape[1] - k[1]) // s[1] + 1, filters)

    class BatchNormalization(Layer):
        def __call__(self, x):
            rec.weighted.append([self.name, "BatchNormalization", x.shape[2], None, None, rec.unit])
            return x

    class Activation(Layer):
        def __call__(self, x):
            rec.activations.append([self.name, self.args[0], rec.unit, list(x.shape)])
            return x

    class ZeroPadding2D(Layer):
        def __call__(self, x):
            p = self.args[0]
            return Tensor(x.shape[0] + 2 * p, x.shape[1] + 2 * p, x.shape[2])

    class MaxPooling2D(Layer):
        def __call__(self, x):
            k, s = pair(self.args[0]), pair(self.kwargs.get("strides"))
            return Tensor((x.shape[0] - k[0]) // s[0] + 1, (x.shape[1] - k[1]) // s[1] + 1, x.shape[2])

    class GlobalAveragePooling2D(Layer):
        def __call__(self, x):
            return Tensor(1, 1, x.shape[2])

    class Lambda(Layer):
        def __call__(self, x):
            return self.args[0](x, **self.kwargs.get("arguments", {}))

    class Concatenate(Layer):
        def __call__(self, xs):
            return Tensor(xs[0].shape[0], xs[0].shape[1], sum(x.shape[2] for x in xs))

    class Multiply(Layer):
        def __call__(self, xs):
            return xs[0]

    class Add(Layer):
        def __call__(self, xs):
            assert xs[0].shape == xs[1].shape, (xs[0].shape, xs[1].shape)
            return xs[0]

    layers = types.SimpleNamespace(**{c.__name__: c for c in (
        Conv2D, BatchNormalization, Activation, ZeroPadding2D, MaxPooling2D, GlobalAveragePooling2D, Lambda, Concatenate,
        Multiply, Add)})
    backend = types.SimpleNamespace(image_data_format=lambda: "channels_last", int_shape=lambda t: (None,) + t.shape,
                                    is_keras_tensor=lambda t: True)
    models = types.SimpleNamespace(Model=lambda inputs, outputs: outputs)
    return backend, layers, models, types.SimpleNamespace()


def load_senet(ref):
    """senet.py and _common_blocks.py as modules of a stand-in package (their imports of keras_applications, TensorFlow
    and the weight loader are satisfied by empty stand-ins; the Keras namespace is passed in through kwargs)."""
    root = os.path.join(ref, "thirdparty", "classification_models")
    pkg = types.ModuleType("_ref_cm")
    pkg.__path__ = [root]
    pkg.get_submodules_from_kwargs = lambda kw: (kw["backend"], kw["layers"], kw["models"], kw["utils"])
    sub = types.ModuleType("_ref_cm.models")
    sub.__path__ = [os.path.join(root, "models")]
    weights = types.ModuleType("_ref_cm.weights")
    weights.load_model_weights = None
    ka = types.ModuleType("keras_applications")
    ka.imagenet_utils = None
    tfp = types.ModuleType("tensorflow.python")
    tfp.keras = types.SimpleNamespace(backend=None, layers=None, models=None, utils=None)
    tf = types.ModuleType("tensorflow")
    tf.python = tfp
    saved = {k: sys.modules.get(k) for k in ("keras_applications", "tensorflow", "tensorflow.python")}
    sys.modules.update({"_ref_cm": pkg, "_ref_cm.models": sub, "_ref_cm.weights": weights, "keras_applications": ka,
                        "tensorflow": tf, "tensorflow.python": tfp})
    try:
        mods = {}
        for name in ("_common_blocks", "senet"):
            spec = importlib.util.spec_from_file_location(f"_ref_cm.models.{name}", os.path.join(root, "models", name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = mod
            spec.loader.exec_module(mod)
            mods[name] = mod
        return mods["senet"]
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def record(senet, model_name):
    rec = Recorder()
    backend, layers, models, utils = make_keras(rec)
    params = senet.MODELS_PARAMS[model_name]
    assert tuple(params.repetitions) == REPETITIONS
    units = [f"stage{s + 1}_unit{u + 1}" for s, r in enumerate(REPETITIONS) for u in range(r)]
    block = params.residual_block

    def labelled(*args, **kwargs):                     # each residual block call is the next unit
        inner = block(*args, **kwargs)

        def layer(x):
            rec.unit = units[len(rec.seen)]
            rec.seen.append(rec.unit)
            return inner(x)
        return layer

    rec.seen = []
    senet.SENet(params._replace(residual_block=labelled), input_tensor=Tensor(SIZE, SIZE, 3), include_top=False,
                weights=None, original_input="images", backend=backend, layers=layers, models=models, utils=utils)
    return rec


def reference_taps(ref):
    tree = ast.parse(open(os.path.join(ref, "engine", "backbone", "base.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "BACKBONE_LAYERS" for t in node.targets):
            table = ast.literal_eval(node.value)
            return {k: table[k] for k in ("seresnet50", "seresnext50")}
    raise RuntimeError("BACKBONE_LAYERS not found")


def main(ref):
    senet = load_senet(ref)
    taps = reference_taps(ref)
    out = {"input": [SIZE, SIZE, 3], "models": {}}
    for name in ("seresnet50", "seresnext50"):
        rec = record(senet, name)
        out["models"][name] = {
            "weighted": [dict(zip(("name", "class", "channels", "kernel", "bias", "unit"), r)) for r in rec.weighted],
            "activations": [dict(zip(("name", "kind", "unit", "shape"), a)) for a in rec.activations],
            "taps": taps[name],
        }
    path = os.path.join(HERE, "senet_layers.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    for name, m in out["models"].items():
        print(name, sum(r["class"] == "Conv2D" for r in m["weighted"]), "Conv2D,",
              sum(r["class"] == "BatchNormalization" for r in m["weighted"]), "BatchNormalization,",
              len(m["activations"]), "Activation")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
