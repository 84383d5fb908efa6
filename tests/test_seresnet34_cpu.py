"""CPU tests of the SE-ResNet-34 backbone (the reference project's own model, road_project/train.py:36-37): the loader
builds it with the reference's taps and sizes, its weight names and shapes are the Keras ones of the vendored
thirdparty/classification_models source, the test-side restatement (tests/backbone_refs.py) agrees with an independent
torch.nn.functional formulation and keeps random-init taps O(1), a Keras checkpoint with auto-numbered ChannelSE convs
converts, and the new C entry points validate their arguments."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from backbone_refs import SERESNET34 as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _backbone(outputs=("C1", "C2", "C3", "C4", "C5", "P6", "P7"), nf=128):
    from masklab_hip import backbone as BB
    from masklab_hip import keras_like as K
    K.clear_session()
    return BB.load_backbone("seresnet34", outputs, nf)


@pytest.mark.parametrize("hw,want", [
    ((1024, 1024), [(512, 512, 64), (256, 256, 64), (128, 128, 128), (64, 64, 256), (32, 32, 512), (16, 16, 128),
                    (8, 8, 128)]),
    ((540, 960), [(270, 480, 64), (135, 240, 64), (68, 120, 128), (34, 60, 256), (17, 30, 512), (9, 15, 128),
                  (5, 8, 128)]),
])
def test_load_backbone_builds_with_the_reference_taps(hw, want):
    from masklab_hip import backbone as BB
    assert BB.BACKBONE_LAYERS["seresnet34"] == {"C1": "relu0", "C2": "stage2_unit1_relu1", "C3": "stage3_unit1_relu1",
                                                "C4": "stage4_unit1_relu1", "C5": "relu1"}
    bb = _backbone()
    assert bb.output_names == ["C1", "C2", "C3", "C4", "C5", "P6", "P7"]
    shapes = bb.build((2,) + hw + (3,))
    assert [tuple(s[1:]) for s in shapes] == want
    shipped = _backbone(("C3", "C4", "C5", "P6"))
    assert shipped.output_names == ["C3", "C4", "C5", "P6"]


def _expected_specs():
    """Names and shapes written from resnet.py ResNet / residual_conv_block and _common_blocks.py ChannelSE (Keras
    layouts: Conv2D kernel [kh, kw, cin, cout], BatchNormalization gamma / beta / moving stats [C], bn_data scale=False);
    the ChannelSE convs under this package's names stage*_unit*_se/conv{1,2}, and the P6 / P7 levels of load_backbone."""
    out = {"bn_data/beta": (3,), "bn_data/moving_mean": (3,), "bn_data/moving_variance": (3,), "conv0/kernel": (7, 7, 3, 64)}

    def bn(name, c):
        for k in ("gamma", "beta", "moving_mean", "moving_variance"):
            out[f"{name}/{k}"] = (c,)

    bn("bn0", 64)
    cin = 64
    for stage, rep in enumerate((3, 4, 6, 3)):
        f = 64 * 2 ** stage
        for block in range(rep):
            base = f"stage{stage + 1}_unit{block + 1}_"
            bn(base + "bn1", cin)
            if block == 0:
                out[base + "sc/kernel"] = (1, 1, cin, f)
            out[base + "conv1/kernel"] = (3, 3, cin, f)
            bn(base + "bn2", f)
            out[base + "conv2/kernel"] = (3, 3, f, f)
            out[base + "se/conv1/kernel"] = (1, 1, f, f // 16)
            out[base + "se/conv1/bias"] = (f // 16,)
            out[base + "se/conv2/kernel"] = (1, 1, f // 16, f)
            out[base + "se/conv2/bias"] = (f,)
            cin = f
    bn("bn1", 512)
    out.update({"P6_conv/kernel": (3, 3, 512, 128), "P6_conv/bias": (128,), "P6_norm/gamma": (128,),
                "P6_norm/beta": (128,), "P7_conv/kernel": (3, 3, 128, 128), "P7_conv/bias": (128,)})
    return out


def test_weight_specs_are_the_keras_names_and_shapes():
    bb = _backbone()
    got = {k: tuple(v.shape) for k, v in bb.weight_specs().items()}
    assert got == _expected_specs()


def _torch_seresnet34(images, w):
    """The same network in torch.nn.functional, NCHW, fp64 (independent of oracle.tfops)."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    k = lambda name: t(w[name]).permute(3, 2, 0, 1)                         # [kh,kw,ci,co] -> [co,ci,kh,kw]

    def bn(x, name, scale=True):
        return F.batch_norm(x, t(w[name + "/moving_mean"]), t(w[name + "/moving_variance"]),
                            t(w[name + "/gamma"]) if scale else None, t(w[name + "/beta"]), False, 0.0, REF.EPS)

    x = t(images).permute(0, 3, 1, 2)
    x = bn(x, "bn_data", scale=False)
    x = F.relu(bn(F.conv2d(x, k("conv0/kernel"), stride=2, padding=3), "bn0"))
    taps = {"C1": x}
    x = F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2)
    for stage, rep in enumerate((3, 4, 6, 3)):
        for block in range(rep):
            base = f"stage{stage + 1}_unit{block + 1}_"
            s = 2 if (block == 0 and stage > 0) else 1
            a = F.relu(bn(x, base + "bn1"))
            if block == 0 and stage > 0:
                taps[f"C{stage + 1}"] = a
            sc = F.conv2d(a, k(base + "sc/kernel"), stride=s) if block == 0 else x
            y = F.relu(bn(F.conv2d(a, k(base + "conv1/kernel"), stride=s, padding=1), base + "bn2"))
            y = F.conv2d(y, k(base + "conv2/kernel"), padding=1)
            g = F.adaptive_avg_pool2d(y, 1)
            g = F.relu(F.conv2d(g, k(base + "se/conv1/kernel"), t(w[base + "se/conv1/bias"])))
            g = torch.sigmoid(F.conv2d(g, k(base + "se/conv2/kernel"), t(w[base + "se/conv2/bias"])))
            x = y * g + sc
    taps["C5"] = F.relu(bn(x, "bn1"))
    return {n: v.permute(0, 2, 3, 1).numpy() for n, v in taps.items()}


def test_restatement_agrees_with_torch_functional():
    from masklab_hip import keras_like as K
    bb = _backbone()
    w = K.init_weights(bb.weight_specs(), 4)
    images = np.random.default_rng(8).integers(0, 256, (1, 64, 96, 3)).astype(np.float64)
    got = REF.seresnet34(images, w)
    want = _torch_seresnet34(images, w)
    assert sorted(got) == sorted(want) == ["C1", "C2", "C3", "C4", "C5"]
    for name in want:
        assert got[name].shape == want[name].shape, name
        np.testing.assert_allclose(got[name], want[name], rtol=1e-5, atol=1e-5, err_msg=name)


def test_random_init_keeps_every_tap_order_one():
    """16 residual additions on random weights: the synthetic init keeps every tap O(1) (neither vanishing nor growing),
    so the fp32 parity bars of the GPU tests mean what they say."""
    from masklab_hip import keras_like as K
    bb = _backbone()
    for seed in (0, 5):
        w = K.init_weights(bb.weight_specs(), seed)
        images = np.random.default_rng(seed).integers(0, 256, (1, 128, 160, 3)).astype(np.float32)
        taps = REF.seresnet34(images, w)
        for name, v in taps.items():
            rms, peak = float(np.sqrt(np.mean(np.square(v, dtype=np.float64)))), float(np.max(np.abs(v)))
            assert 0.05 < rms < 5.0 and peak < 50.0, (seed, name, rms, peak)


def test_restatement_delegates_every_other_backbone(monkeypatch):
    REF.check_patch_keeps_the_oracle_backbones(monkeypatch)


def _fake_keras_file(weights):
    spec = importlib.util.spec_from_file_location("host_cpu_for_seresnet34", os.path.join(ROOT, "tests", "test_host_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._fake_keras_file(weights)


def _load_converter():
    spec = importlib.util.spec_from_file_location("convert_keras_h5", os.path.join(ROOT, "tools", "convert_keras_h5.py"))
    conv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(conv)
    return conv


def _keras_named(weights, first_head_conv):
    """Re-key a seresnet34 model's weights the way Keras names them after K.clear_session(): the backbone is built first,
    its ChannelSE convs take `conv2d`, `conv2d_1`, ... two per unit in unit order; the head's auto-named convs follow
    (here only FeaturePyramid's laterals, created for strides in descending order, detection.py:39-43)."""
    se = sorted({m.groups() for m in (re.match(r"^stage(\d+)_unit(\d+)_se/conv([12])/", k) for k in weights) if m},
                key=lambda g: tuple(int(v) for v in g))
    assert len(se) == 32
    auto = lambda n: "conv2d" if n == 0 else f"conv2d_{n}"
    pre = {f"stage{s}_unit{u}_se/conv{i}": auto(n) for n, (s, u, i) in enumerate(se)}
    for j, p in enumerate((5, 4, 3)):
        pre[f"feature_pyramid/C{p}_lateral"] = "feature_pyramid/" + auto(first_head_conv + j)
    out = {}
    for k, v in weights.items():
        head, _, rest = k.rpartition("/")
        out[pre.get(head, head) + "/" + rest] = v
    return out


def test_keras_checkpoint_with_auto_named_channel_se_converts(tmp_path):
    conv = _load_converter()
    from masklab_hip import ModelConfiguration, retinamasklab as R
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = "seresnet34"
    cfg.backbone.backbone_outputs = ("C3", "C4", "C5", "P6")
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(2)
    specs = {k: tuple(v.shape) for k, v in model.weight_specs().items()}
    named = _keras_named(w, 32)
    assert "conv2d/kernel" in named and "conv2d_31/bias" in named and "feature_pyramid/conv2d_32/kernel" in named
    got = conv.collect_h5_weights(_fake_keras_file(named))
    _, rep0 = conv.match_to_model(got, specs)
    assert len(rep0["missing"]) >= 64                               # the ChannelSE convs are not found without the mapping
    table = []
    matched, rep = conv.match_to_model(conv.rename_keras_auto_names(got, specs, table), specs)
    assert rep["missing"] == [] and rep["shape_mismatch"] == [] and rep["unexpected"] == []
    for k in w:
        np.testing.assert_array_equal(matched[k], w[k], err_msg=k)
    rows = sorted((r for r in table if r[0] == "backbone"), key=lambda r: r[2])
    assert [r[4] for r in rows[:3]] == ["stage1_unit1_se/conv1", "stage1_unit1_se/conv2", "stage1_unit2_se/conv1"]
    assert rows[-1][3] == "conv2d_31" and rows[-1][4] == "stage4_unit3_se/conv2"
    # a checkpoint with another number of backbone convs is refused, not mis-assigned
    short = {k: v for k, v in got.items() if not k.startswith("conv2d_31/")}
    with pytest.raises(ValueError, match="different backbone"):
        conv.rename_keras_auto_names(short, specs)
    # the command-line converter accepts --backbone seresnet34 (the default head configuration, P7 included)
    full_cfg = ModelConfiguration()
    full_cfg.backbone.backbone_type = "seresnet34"
    _, full = R.construct_masklab_networks(full_cfg)
    full_specs = conv.model_specs("seresnet34")
    assert full_specs == {k: tuple(v.shape) for k, v in full.weight_specs().items()}
    assert sum(1 for k in full_specs if re.match(r"^stage\d+_unit\d+_se/", k)) == 64


def test_f16s_is_refused_for_this_backbone():
    from masklab_hip import ops
    bb = _backbone(("C3", "C4", "C5", "P6"))
    ops.set_conv_math("f16s")
    try:
        with pytest.raises(NotImplementedError, match="f16s"):
            bb.body(None, wanted=("C3", "C4", "C5"))
    finally:
        ops.set_conv_math("f32")


def test_se_residual_entry_points_are_exported_and_validate():
    from masklab_hip import _lib
    lib = _lib.load()
    assert lib.ml_se_residual_workspace_bytes(2, 600, 64) == 2 * 3 * 64 * 8          # 600 px: three 256-pixel slabs
    assert lib.ml_se_residual_workspace_bytes(8, 65536, 64) == 8 * 64 * 64 * 8        # at most 64 slabs per sample
    assert lib.ml_se_residual_workspace_bytes(1, 510, 512) == 8 * 512 * 8             # 16 chunks of 32 px, 8 slabs of 64 px
    assert lib.ml_se_residual_workspace_bytes(1, 2040, 256) == 16 * 256 * 8           # 32 chunks of 64 px, 16 slabs
    assert lib.ml_se_residual_workspace_bytes(0, 600, 64) == 0

    def desc(**kw):
        d = _lib.SeResidualDesc()
        base = dict(x=0x10000, shortcut=0x20000, w1=0x30000, b1=0x31000, w2=0x32000, b2=0x33000, scale=0x34000,
                    shift=0x35000, out_act=0x40000, out_y=None, B=1, HW=16, C=64, Hd=4, mode=_lib.SE_RES_GATE)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return d

    ws, big = 0x80000, 1 << 20

    def call(d, w=ws, n=big):
        return lib.ml_se_residual_f32(ctypes.byref(d), w, n, None)

    cases = [
        (desc(x=None), b"required"),
        (desc(mode=7), b"unknown mode"),
        (desc(C=66), b"multiple of 4"),
        (desc(C=1024), b"multiple of 4"),
        (desc(Hd=0), b"Hd = 0"),
        (desc(Hd=33), b"Hd = 33"),
        (desc(w2=None), b"GATE needs"),
        (desc(x=0x10004), b"16-byte aligned"),
        (desc(out_y=0x40008), b"16-byte aligned"),
        (desc(B=0), b"positive"),
        (desc(out_act=0x10100), b"partially overlaps"),
        (desc(out_y=0x40000), b"overlap"),
        (desc(mode=_lib.SE_RES_BN_RELU), b"BN_RELU takes no shortcut"),
    ]
    for d, msg in cases:
        assert call(d) == -1, msg
        assert msg in lib.ml_last_error(), (msg, lib.ml_last_error())
    assert call(desc(), None, 0) == -1 and b"workspace" in lib.ml_last_error()
    assert call(desc(), ws, 64) == -1 and b"need" in lib.ml_last_error()
