"""CPU tests of the SE-ResNet-50 and SE-ResNeXt-50 backbones (the vendored thirdparty/classification_models senet.py that
the reference's load_backbone offers): the loader builds both with the reference's taps and sizes, BACKBONE_LAYERS equals
the reference's entries, weight names and shapes are the expected Keras-shaped ones and their creation order is the
reference's (tests/golden/senet_layers.json, recorded from the reference's own builder), the test-side restatement
(tests/backbone_refs.py) agrees with an independent torch.nn.functional formulation and keeps random-init taps O(1), a
Keras checkpoint with auto-named layers converts, and the new C entry points validate their arguments."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

from backbone_refs import SENET as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "senet_layers.json")))
ALL = ("C1", "C2", "C3", "C4", "C5", "P6", "P7")


def _backbone(bt, outputs=ALL, nf=128):
    from masklab_hip import backbone as BB
    from masklab_hip import keras_like as K
    K.clear_session()
    return BB.load_backbone(bt, outputs, nf)


@pytest.mark.parametrize("bt", REF.TYPES)
@pytest.mark.parametrize("hw,want", [
    ((1024, 1024), [(512, 512, 64), (256, 256, 256), (128, 128, 512), (64, 64, 1024), (32, 32, 2048), (16, 16, 128),
                    (8, 8, 128)]),
    ((200, 328), [(100, 164, 64), (50, 82, 256), (25, 41, 512), (13, 21, 1024), (7, 11, 2048), (4, 6, 128), (2, 3, 128)]),
])
def test_load_backbone_builds_with_the_reference_taps(bt, hw, want):
    bb = _backbone(bt)
    assert bb.output_names == list(ALL)
    shapes = bb.build((2,) + hw + (3,))
    assert [tuple(s[1:]) for s in shapes] == want
    shipped = _backbone(bt, ("C3", "C4", "C5", "P6", "P7"))
    assert shipped.output_names == ["C3", "C4", "C5", "P6", "P7"]


def test_tap_shapes_are_those_of_the_reference_activations():
    """The fixture's Activation output shapes at 1024^2 are what the loader builds for each tap."""
    for bt in REF.TYPES:
        acts = {a["name"]: a for a in GOLDEN["models"][bt]["activations"]}
        shapes = _backbone(bt).build((1, 1024, 1024, 3))
        for tap, shape in zip(("C1", "C2", "C3", "C4", "C5"), shapes):
            assert list(shape[1:]) == acts[GOLDEN["models"][bt]["taps"][tap]]["shape"], (bt, tap)


def test_backbone_layers_equal_the_reference_entries():
    from masklab_hip import backbone as BB
    for bt in REF.TYPES:
        assert BB.BACKBONE_LAYERS[bt] == GOLDEN["models"][bt]["taps"]
    assert GOLDEN["models"]["seresnet50"]["taps"] == {"C1": "activation", "C2": "activation_15", "C3": "activation_35",
                                                      "C4": "activation_65", "C5": "activation_80"}
    assert GOLDEN["models"]["seresnext50"]["taps"] == {"C1": "activation", "C2": "activation_16", "C3": "activation_36",
                                                       "C4": "activation_66", "C5": "activation_80"}
    # SE-ResNeXt-50's C2..C4 are the conv1 ReLU of the next stage's first unit; SE-ResNet-50's the stage outputs
    units = {bt: {a["name"]: a["unit"] for a in GOLDEN["models"][bt]["activations"]} for bt in REF.TYPES}
    assert [units["seresnext50"][GOLDEN["models"]["seresnext50"]["taps"][t]] for t in ("C2", "C3", "C4", "C5")] == \
        ["stage2_unit1", "stage3_unit1", "stage4_unit1", "stage4_unit3"]
    assert [units["seresnet50"][GOLDEN["models"]["seresnet50"]["taps"][t]] for t in ("C2", "C3", "C4", "C5")] == \
        ["stage1_unit3", "stage2_unit4", "stage3_unit6", "stage4_unit3"]


def _expected_specs(bt):
    """Names and shapes written from senet.py SEResNetBottleneck / SEResNeXtBottleneck and _common_blocks.py GroupConv2D
    / ChannelSE (Keras layouts: Conv2D kernel [kh, kw, cin, cout], BatchNormalization gamma / beta / moving stats [C]),
    under this package's hierarchical names, and the P6 / P7 levels of load_backbone."""
    grouped = bt == "seresnext50"
    out = {"conv0/kernel": (7, 7, 3, 64)}

    def bn(name, c):
        for k in ("gamma", "beta", "moving_mean", "moving_variance"):
            out[f"{name}/{k}"] = (c,)

    bn("bn0", 64)
    cin = 64
    for stage, rep in enumerate((3, 4, 6, 3)):
        f = 256 * 2 ** stage
        width = f // 2 if grouped else f // 4
        for block in range(rep):
            b = f"stage{stage + 1}_unit{block + 1}_"
            out[b + "conv1/kernel"] = (1, 1, cin, width)
            bn(b + "bn1", width)
            if grouped:
                for g in range(32):
                    out[f"{b}conv2/group{g}/kernel"] = (3, 3, width // 32, width // 32)
            else:
                out[b + "conv2/kernel"] = (3, 3, width, width)
            bn(b + "bn2", width)
            out[b + "conv3/kernel"] = (1, 1, width, f)
            bn(b + "bn3", f)
            if block == 0:
                out[b + "sc/kernel"] = (1, 1, cin, f)
                bn(b + "sc_bn", f)
            out[b + "se/conv1/kernel"] = (1, 1, f, f // 16)
            out[b + "se/conv1/bias"] = (f // 16,)
            out[b + "se/conv2/kernel"] = (1, 1, f // 16, f)
            out[b + "se/conv2/bias"] = (f,)
            cin = f
    out.update({"P6_conv/kernel": (3, 3, 2048, 128), "P6_conv/bias": (128,), "P6_norm/gamma": (128,),
                "P6_norm/beta": (128,), "P7_conv/kernel": (3, 3, 128, 128), "P7_conv/bias": (128,)})
    return out


@pytest.mark.parametrize("bt", REF.TYPES)
def test_weight_specs_are_the_expected_names_and_shapes(bt):
    got = {k: tuple(v.shape) for k, v in _backbone(bt).weight_specs().items()}
    assert got == _expected_specs(bt)


@pytest.mark.parametrize("bt,nconv", [("seresnet50", 85), ("seresnext50", 581)])
def test_creation_order_is_the_references(bt, nconv):
    """The checkpoint import's creation order of this package's layers, against the reference's recorded one: every
    conv (kernel shape, bias or not, unit) and every BatchNormalization (channels, unit), in order."""
    from masklab_hip import checkpoint as CK
    specs = {k: tuple(v.shape) for k, v in _backbone(bt).weight_specs().items()}
    convs, bns = CK._senet50_order(specs)
    ref = GOLDEN["models"][bt]["weighted"]
    ref_convs = [r for r in ref if r["class"] == "Conv2D"]
    ref_bns = [r for r in ref if r["class"] == "BatchNormalization"]
    assert len(convs) == len(ref_convs) == nconv and len(bns) == len(ref_bns) == 53
    unit = lambda p: "stem" if p in ("conv0", "bn0") else p.split("_")[0] + "_" + p.split("_")[1]
    for ours, r in zip(convs, ref_convs):
        assert specs[ours + "/kernel"] == tuple(r["kernel"]), (ours, r)
        assert (ours + "/bias" in specs) == r["bias"], (ours, r)
        assert unit(ours) == r["unit"], (ours, r)
    for ours, r in zip(bns, ref_bns):
        assert specs[ours + "/gamma"] == (r["channels"],) and unit(ours) == r["unit"], (ours, r)
    # Keras numbers them in the same order: conv2d, conv2d_1, ... and batch_normalization, batch_normalization_1, ...
    assert [r["name"] for r in ref_convs] == ["conv2d"] + [f"conv2d_{n}" for n in range(1, nconv)]
    assert [r["name"] for r in ref_bns] == ["batch_normalization"] + [f"batch_normalization_{n}" for n in range(1, 53)]


def _torch_senet50(images, w, bt):
    """The same network in torch.nn.functional, NCHW, fp64 (independent of oracle.tfops)."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    k = lambda name: t(w[name]).permute(3, 2, 0, 1)                         # [kh,kw,ci,co] -> [co,ci,kh,kw]
    grouped = bt == "seresnext50"

    def bn(x, name):
        return F.batch_norm(x, t(w[name + "/moving_mean"]), t(w[name + "/moving_variance"]), t(w[name + "/gamma"]),
                            t(w[name + "/beta"]), False, 0.0, REF.EPS)

    x = t(images).permute(0, 3, 1, 2)
    x = (x - t([123.68, 116.779, 103.939])[None, :, None, None]) / 255.0 / t([0.225, 0.224, 0.229])[None, :, None, None]
    x = F.relu(bn(F.conv2d(x, k("conv0/kernel"), stride=2, padding=3), "bn0"))
    taps = {"C1": x}
    x = F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2)
    for stage, rep in enumerate((3, 4, 6, 3)):
        for block in range(rep):
            b = f"stage{stage + 1}_unit{block + 1}_"
            s = 2 if (block == 0 and stage > 0) else 1
            y1 = F.relu(bn(F.conv2d(x, k(b + "conv1/kernel"), stride=1 if grouped else s), b + "bn1"))
            if grouped and block == 0 and stage > 0:
                taps[f"C{stage + 1}"] = y1
            if grouped:
                wg = torch.cat([k(f"{b}conv2/group{g}/kernel") for g in range(32)], dim=0)
                y = F.conv2d(y1, wg, stride=s, padding=1, groups=32)
            else:
                y = F.conv2d(y1, k(b + "conv2/kernel"), padding=1)
            y = F.relu(bn(y, b + "bn2"))
            y = bn(F.conv2d(y, k(b + "conv3/kernel")), b + "bn3")
            sc = bn(F.conv2d(x, k(b + "sc/kernel"), stride=s), b + "sc_bn") if block == 0 else x
            g = F.adaptive_avg_pool2d(y, 1)
            g = F.relu(F.conv2d(g, k(b + "se/conv1/kernel"), t(w[b + "se/conv1/bias"])))
            g = torch.sigmoid(F.conv2d(g, k(b + "se/conv2/kernel"), t(w[b + "se/conv2/bias"])))
            x = F.relu(y * g + sc)
        if not grouped or stage == 3:
            taps[f"C{stage + 2}"] = x
    return {n: v.permute(0, 2, 3, 1).numpy() for n, v in taps.items()}


@pytest.mark.parametrize("bt", REF.TYPES)
def test_restatement_agrees_with_torch_functional(bt):
    from masklab_hip import keras_like as K
    from oracle import masklab as O
    w = K.init_weights(_backbone(bt).weight_specs(), 4)
    images = np.random.default_rng(8).integers(0, 256, (1, 64, 96, 3)).astype(np.float64)
    got = REF.senet50(O.backbone_preprocess(images, rgb=True, mean_shift=True, normalize=3), w, bt)
    want = _torch_senet50(images, w, bt)
    assert sorted(got) == sorted(want) == ["C1", "C2", "C3", "C4", "C5"]
    for name in want:
        assert got[name].shape == want[name].shape, name
        np.testing.assert_allclose(got[name], want[name], rtol=1e-5, atol=1e-5, err_msg=name)


@pytest.mark.parametrize("bt", REF.TYPES)
def test_random_init_keeps_every_tap_order_one(bt):
    """16 residual additions on random weights: the synthetic init keeps every tap O(1) (neither vanishing nor growing),
    so the fp32 parity bars of the GPU tests mean what they say."""
    from masklab_hip import keras_like as K
    from oracle import masklab as O
    bb = _backbone(bt)
    for seed in (0, 5):
        w = K.init_weights(bb.weight_specs(), seed)
        images = np.random.default_rng(seed).integers(0, 256, (1, 128, 160, 3)).astype(np.float32)
        taps = REF.senet50(O.backbone_preprocess(images, rgb=True, mean_shift=True, normalize=3), w, bt)
        for name, v in taps.items():
            rms, peak = float(np.sqrt(np.mean(np.square(v, dtype=np.float64)))), float(np.max(np.abs(v)))
            assert 0.05 < rms < 5.0 and peak < 50.0, (bt, seed, name, rms, peak)


def test_restatement_delegates_every_other_backbone(monkeypatch):
    REF.check_patch_keeps_the_oracle_backbones(monkeypatch)


def _fake_keras_file(weights):
    spec = importlib.util.spec_from_file_location("host_cpu_for_senet", os.path.join(ROOT, "tests", "test_host_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._fake_keras_file(weights)


def _load_converter():
    spec = importlib.util.spec_from_file_location("convert_keras_h5", os.path.join(ROOT, "tools", "convert_keras_h5.py"))
    conv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(conv)
    return conv


def _keras_named(weights, specs, bt):
    """Re-key a model's weights the way Keras names them after K.clear_session(): every backbone conv and BN takes the
    fixture's auto name (the reference's creation order, paired by _senet50_order), the head's auto-named convs follow
    (here only FeaturePyramid's laterals, created for strides in descending order, detection.py:39-43)."""
    from masklab_hip import checkpoint as CK
    convs, bns = CK._senet50_order(specs)
    ref = GOLDEN["models"][bt]["weighted"]
    pre = dict(zip(convs, [r["name"] for r in ref if r["class"] == "Conv2D"]))
    pre.update(zip(bns, [r["name"] for r in ref if r["class"] == "BatchNormalization"]))
    for j, p in enumerate((5, 4, 3)):
        pre[f"feature_pyramid/C{p}_lateral"] = f"feature_pyramid/conv2d_{len(convs) + j}"
    out = {}
    for k, v in weights.items():
        head, _, rest = k.rpartition("/")
        out[pre.get(head, head) + "/" + rest] = v
    return out


def _model(bt):
    from masklab_hip import ModelConfiguration, retinamasklab as R
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = bt
    _, model = R.construct_masklab_networks(cfg)
    return model


@pytest.mark.parametrize("bt", REF.TYPES)
def test_keras_checkpoint_with_auto_named_layers_converts(bt):
    conv = _load_converter()
    model = _model(bt)
    w = model.init_weights(2)
    specs = {k: tuple(v.shape) for k, v in model.weight_specs().items()}
    named = _keras_named(w, specs, bt)
    assert "conv2d/kernel" in named and "batch_normalization_52/moving_variance" in named
    assert not any(k.startswith("stage") or k.startswith(("conv0/", "bn0/")) for k in named)
    got = conv.collect_h5_weights(_fake_keras_file(named))
    table = []
    matched, rep = conv.match_to_model(conv.rename_keras_auto_names(got, specs, table), specs)
    assert rep["missing"] == [] and rep["shape_mismatch"] == [] and rep["unexpected"] == []
    for k in w:
        np.testing.assert_array_equal(matched[k], w[k], err_msg=k)
    rows = sorted((r for r in table if r[0] == "backbone" and r[1] == "conv2d"), key=lambda r: r[2])
    assert rows[0][3:] == ("conv2d", "conv0") and rows[-1][4] == "stage4_unit3_se/conv2"
    # the grouped kernels re-assembled exactly: kernel[..., g*c+i, m] = K_g[..., i, m]
    if bt == "seresnext50":
        body = model.backbone_network.body
        for u in (body.stages[0][0], body.stages[3][2]):
            k = u.conv2.kernel(matched)
            c = k.shape[-1]
            for g in (0, 17, 31):
                np.testing.assert_array_equal(k[:, :, g * c:(g + 1) * c, :], w[f"{u.conv2.name}/group{g}/kernel"])


def test_checkpoint_of_the_other_senet_is_refused():
    conv = _load_converter()
    m50, mx50 = _model("seresnet50"), _model("seresnext50")
    specs50 = {k: tuple(v.shape) for k, v in m50.weight_specs().items()}
    specsx = {k: tuple(v.shape) for k, v in mx50.weight_specs().items()}
    got = conv.collect_h5_weights(_fake_keras_file(_keras_named(m50.init_weights(1), specs50, "seresnet50")))
    with pytest.raises(ValueError, match=r"85 auto-named 'conv2d'.*declares 581"):
        conv.rename_keras_auto_names(got, specsx)


def test_se_bottleneck_entry_points_are_exported_and_validate():
    from masklab_hip import _lib
    lib = _lib.load()
    ws = lambda B, HW, C: lib.ml_se_bottleneck_workspace_bytes(B, HW, C)
    # pool chunks: ceil(HW * C / 32768) of them, at most min(128, 65536 / C), then whole chunks of ceil(HW / that)
    # pixels; fp64 slabs
    # [B][chunks][C], then the gate as two fp32 arrays [B][C]
    assert ws(2, 600, 64) == 2 * 2 * 64 * 8 + 2 * 2 * 64 * 4              # 2 chunks of 300 px
    assert ws(8, 65536, 256) == 8 * 128 * 256 * 8 + 2 * 8 * 256 * 4       # capped at 128 slabs
    assert ws(3, 510, 2048) == 3 * 32 * 2048 * 8 + 2 * 3 * 2048 * 4       # 32 chunks of 16 px
    assert ws(8, 1024, 2048) == 8 * 32 * 2048 * 8 + 2 * 8 * 2048 * 4      # capped at 65536 / 2048 = 32 slabs
    assert ws(1, 1, 1024) == 1024 * 8 + 2 * 1024 * 4
    assert ws(0, 600, 64) == 0 and ws(1, 600, 2052) == 0

    def desc(**kw):
        d = _lib.SeBottleneckDesc()
        base = dict(c3=0x100000, residual=0x200000, w1=0x300000, b1=0x310000, w2=0x320000, b2=0x330000, out=0x400000,
                    B=1, HW=16, C=64, Hd=4)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return d

    wsp, big = 0x800000, 1 << 20

    def call(d, w=wsp, n=big, half=False):
        fn = lib.ml_se_bottleneck_f16 if half else lib.ml_se_bottleneck_f32
        return fn(ctypes.byref(d), w, n, None)

    cases = [
        (desc(c3=None), False, b"required"),
        (desc(b2=None), False, b"required"),
        (desc(C=2052), False, b"in 4..2048"),
        (desc(C=66), False, b"multiple of 4"),
        (desc(C=12), True, b"multiple of 8"),
        (desc(Hd=0), False, b"Hd = 0"),
        (desc(Hd=129), False, b"Hd = 129"),
        (desc(B=0), False, b"positive"),
        (desc(c3=0x100004), False, b"16-byte aligned"),
        (desc(residual=0x200008), True, b"16-byte aligned"),
        (desc(out=0x400002), False, b"16-byte aligned"),
        (desc(w1=0x300002), False, b"misaligned FC weights"),
        (desc(out=0x100100), False, b"partially overlaps"),
        (desc(out=0x200010), True, b"partially overlaps"),
        (desc(out=wsp), False, b"workspace overlaps out"),
    ]
    for d, half, msg in cases:
        assert call(d, half=half) == -1, msg
        assert msg in lib.ml_last_error(), (msg, lib.ml_last_error())
    assert call(desc(), None, 0) == -1 and b"workspace" in lib.ml_last_error()
    assert call(desc(), wsp, 64) == -1 and b"need" in lib.ml_last_error()
    assert call(desc(), wsp + 8, big) == -1 and b"16-byte aligned workspace" in lib.ml_last_error()
    # out may be c3 itself or the residual itself: those pass the overlap checks (the workspace check after them fails)
    for alias in (0x100000, 0x200000):
        assert call(desc(out=alias), alias, big) == -1
        assert b"workspace overlaps out" in lib.ml_last_error(), lib.ml_last_error()
