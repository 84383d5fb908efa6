"""Shared by the layer-parameter tests (test infrastructure, not collected): the five head groups of the reference's default
configuration, and a walk over the packings under a layer."""
import numpy as np

from masklab_hip import ModelConfiguration, keras_like as K, retinamasklab as R

HEADS = ("cls", "loc", "mask", "aspp", "seg")


def build_heads():
    """-> ({head name: layer}, weights of the whole model, the inference model)"""
    K.clear_session()
    _, model = R.construct_masklab_networks(ModelConfiguration())
    heads = dict(zip(HEADS, [model.detection_networks[2], model.detection_networks[3], model.instance_networks[3]] +
                     list(model.semantic_networks)))
    return heads, model.init_weights(seed=1), model


def walk(layer):
    yield layer
    for ch in getattr(layer, "children", lambda: [])():      # a backbone also lists holders of packings that are no layers
        yield from walk(ch)


def all_tensors(layer):
    """{label: tensor} of every torch tensor reachable from the objects under `layer`: their attributes, the attributes of
    whatever they hold that has a `wgt` (DeviceConv, its dgrad, the dual packings), and lists / tuples of either."""
    import torch
    out, seen = {}, set()

    def visit(label, v, depth):
        if isinstance(v, torch.Tensor):
            out[label] = v
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                visit(f"{label}[{i}]", e, depth)
        elif hasattr(v, "wgt") and id(v) not in seen and depth < 4:
            seen.add(id(v))
            for k, e in vars(v).items():
                visit(f"{label}.{k}", e, depth + 1)

    for l in walk(layer):
        if id(l) in seen:
            continue
        seen.add(id(l))
        for k, v in vars(l).items():
            if k not in ("_params", "_specs"):
                visit(f"{getattr(l, 'name', type(l).__name__)}:{k}", v, 0)
    return out


def touch(layer, which):
    """Materialises lazy forms of every dense conv under `layer`: which = "wino" (the stride-1 3x3 convs' Winograd form) or
    "dgrad" (the data gradient's packing, with its Winograd form where it has one, the ASPP's concat slices and theirs)."""
    for l in walk(layer):
        if type(l) is K.Conv2D and l.strides[0] == 1:
            p = l.dev.p
            wino = (p.KH, p.KW) == (3, 3) and p.n_pad <= 128
            if which == "wino" and wino:
                l.dev.wgt_wino
            if which == "dgrad":
                d = l.dev.dgrad
                if wino and d.p.n_pad <= 128:
                    d.wgt_wino
        if type(l) is K.Conv2DTranspose and which == "dgrad":
            l.dev1x1.dgrad
        if hasattr(l, "_concat_slices") and which == "dgrad":
            for dc in l._concat_slices():
                dc.dgrad


def packings(layer):
    """{label: tensor} of everything the kernels read under `layer`: every DeviceConv's forms (dgrad's included), the
    depthwise and GroupNorm tensors, the mask tail's tables and operand, the ASPP's concat slices."""
    out = {}

    def conv(label, dc):
        for prefix, d in ((label, dc), (label + ".dgrad", dc._dgrad)):
            if d is None:
                continue
            for name, t in (("wgt", d.wgt), ("x3", d._wgt_x3), ("h", d._wgt_h), ("wino", d._wgt_wino), ("bias", d.bias)):
                if t is not None:
                    out[f"{prefix}.{name}"] = t

    for l in walk(layer):
        for attr in ("dev", "dev1x1"):
            if hasattr(getattr(l, attr, None), "repack_jobs"):
                conv(f"{l.name}:{attr}", getattr(l, attr))
        for attr in ("wgt", "bias", "gamma", "beta"):
            t = getattr(l, attr, None)
            if t is not None and hasattr(t, "data_ptr"):
                out[f"{l.name}:{attr}"] = t
        if getattr(l, "_tail_tables", None):
            for i, ((table, bo), wo) in enumerate(zip(l._tail_tables, l._tail_wo)):
                out.update({f"{l.name}:table{i}": table, f"{l.name}:table_bias{i}": bo, f"{l.name}:wo{i}": wo})
        if getattr(l, "_slices_of", None) is not None:
            for i, dc in enumerate(l._slices):
                conv(f"{l.name}:slice{i}", dc)
    return out


def to_host(tensors):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in tensors.items()}
