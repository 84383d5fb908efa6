"""Regenerates tests/golden/resnet50_layers.json: what pins the ResNet-50 backbone.  Run from the repository root with the
reference tree at hand:

    python tests/golden/make_resnet50_golden.py /path/to/reference

From the reference it reads, with `ast` (engine/backbone/base.py imports TensorFlow), the BACKBONE_LAYERS["resnet50"] tap
dict and load_backbone's default `backbone_type`.  The reference does not vendor the architecture (it imports
tensorflow.keras.applications.ResNet50), so the layer inventory is written out here from the published legacy
Keras-Applications 1.0.x resnet50.py -- the only model whose Activations carry those auto names: conv1 / bn_conv1, then per
stage s = 2..5 and block b = a.. the layers res{s}{b}_branch2a / 2b / 2c [+ res{s}a_branch1] and their bn{s}{b}_branch*,
in creation order; every conv with a bias, every BatchNormalization with gamma, beta and the two moving statistics.  The
file holds names and shapes only: the taps, the 106 layer names, the weight shapes, the Activation that closes each block,
and the parameter totals (23 587 712, of which 53 120 BN moving statistics -- the published no-top count).  Nothing on the
GPU side reads it."""
import ast
import json
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
STAGES = ((2, "abc", (64, 64, 256)), (3, "abcd", (128, 128, 512)), (4, "abcdef", (256, 256, 1024)),
          (5, "abc", (512, 512, 2048)))


def reference_entries(ref):
    tree = ast.parse(open(os.path.join(ref, "engine", "backbone", "base.py")).read())
    taps = default = None
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "BACKBONE_LAYERS" for t in node.targets):
            taps = ast.literal_eval(node.value)["resnet50"]
        if isinstance(node, ast.FunctionDef) and node.name == "load_backbone":
            names = [a.arg for a in node.args.args]
            defaults = dict(zip(names[len(names) - len(node.args.defaults):], node.args.defaults))
            default = ast.literal_eval(defaults["backbone_type"])
    return taps, default


def inventory():
    layers, weights, activations = [], {}, ["activation"]

    def conv(name, kh, cin, cout):
        layers.append(name)
        weights[name + "/kernel"] = [kh, kh, cin, cout]
        weights[name + "/bias"] = [cout]

    def bn(name, c):
        layers.append(name)
        for k in ("gamma", "beta", "moving_mean", "moving_variance"):
            weights[f"{name}/{k}"] = [c]

    conv("conv1", 7, 3, 64)
    bn("bn_conv1", 64)
    cin, n_act, closing = 64, 1, {}
    for stage, blocks, (f1, f2, f3) in STAGES:
        for b in blocks:
            for branch, kh, ci, co in (("2a", 1, cin, f1), ("2b", 3, f1, f2), ("2c", 1, f2, f3)):
                conv(f"res{stage}{b}_branch{branch}", kh, ci, co)
                bn(f"bn{stage}{b}_branch{branch}", co)
            if b == "a":
                conv(f"res{stage}a_branch1", 1, cin, f3)
                bn(f"bn{stage}a_branch1", f3)
            n_act += 3                                   # the ReLUs behind 2a, 2b and the Add
            closing[f"{stage}{b}"] = f"activation_{n_act - 1}"
            cin = f3
    return layers, weights, closing, n_act


def main():
    taps, default = reference_entries(sys.argv[1])
    layers, weights, closing, n_act = inventory()
    size = lambda s: int(__import__("math").prod(s))
    out = {
        "source": "taps and default: the reference's engine/backbone/base.py; layers: the published legacy "
                  "Keras-Applications 1.0.x resnet50.py (include_top=False)",
        "default_backbone_type": default,
        "taps": taps,
        "layers": layers,
        "weights": weights,
        "block_activation": closing,
        "activations": n_act,
        "tap_channels": {"C1": 64, "C2": 256, "C3": 512, "C4": 1024, "C5": 2048},
        "params": sum(size(s) for s in weights.values()),
        "params_bn_moving": sum(size(s) for k, s in weights.items() if "/moving_" in k),
    }
    with open(os.path.join(HERE, "resnet50_layers.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out["params"], out["params_bn_moving"], len(layers), n_act, taps, default)


if __name__ == "__main__":
    main()
