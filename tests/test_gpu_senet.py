"""GPU tests of the SE-ResNet-50 and SE-ResNeXt-50 backbones (vendored thirdparty senet.py, offered by the reference's
load_backbone): the fused SE bottleneck tail (csrc/se_bottleneck.hip) against an fp64 NumPy formulation in fp32 and in
half storage, bit-stable run to run and per image; the backbone taps against the test-side restatement
(tests/backbone_refs.py) in every conv math; both backbones end to end against the oracle with detections, device counts
and one hipGraph; SE-ResNeXt-50 in 'f16s' end to end; an .npz checkpoint through load_masklab_inference_model_from_h5 to
the deploy model.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import masklab as O

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import backbone_cases as CASES
from backbone_refs import SENET as REF

F16_MODEL_TOL = 3e-2


# ------------------------------------------------------------------ the tail kernel
def _tail_problem(B, H, W, C, seed, dtype):
    rng = np.random.default_rng(seed)
    Hd = C // 16
    f = lambda *s, sd=1.0: (rng.standard_normal(s, dtype=np.float32) * np.float32(sd)).astype(np.float32)
    return dict(c3=f(B, H, W, C).astype(dtype), res=f(B, H, W, C).astype(dtype), w1=f(C, Hd, sd=np.sqrt(2.0 / C)),
                b1=f(Hd, sd=0.1), w2=f(Hd, C, sd=np.sqrt(2.0 / Hd)), b2=f(C, sd=0.1))


def _tail_ref(p):
    """fp64 from the very inputs the kernel gets (the half ones for a half problem)."""
    x = p["c3"].astype(np.float64)
    m = x.mean(axis=(1, 2))                                                       # [B, C]
    h = np.maximum(m @ p["w1"].astype(np.float64) + p["b1"], 0.0)
    g = 1.0 / (1.0 + np.exp(-(h @ p["w2"].astype(np.float64) + p["b2"])))
    y = x * g[:, None, None, :]
    y += p["res"]
    return np.maximum(y, 0.0, out=y)


def _tail_gpu(p, in_place):
    from masklab_hip import ops
    c3 = dev(p["c3"])
    out = ops.se_bottleneck(c3, dev(p["res"]), dev(p["w1"]), dev(p["b1"]), dev(p["w2"]), dev(p["b2"]),
                            out=c3 if in_place else None)
    assert (out.data_ptr() == c3.data_ptr()) == in_place
    return out


def _check_half(got, want):
    """Within one half-precision ulp of the fp64 value: one rounding after fp32 arithmetic whose error is orders
    smaller than half an ulp."""
    ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / ulp).max())
    assert worst <= 1.0, worst


def _tail_case(B, H, W, C, dtype, in_place):
    p = _tail_problem(B, H, W, C, H * 1000 + C, dtype)
    out = _tail_gpu(p, in_place)
    got = host(out)
    assert got.dtype == dtype and got.shape == (B, H, W, C)
    want = _tail_ref(p)
    if dtype == np.float16:
        _check_half(got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    del want
    # repeated launches: the same bits; image k of the batch == image k alone
    assert torch.equal(out, _tail_gpu(p, in_place))
    for k in range(B):
        one = {n: (v[k:k + 1] if v.ndim == 4 else v) for n, v in p.items()}
        assert torch.equal(out[k:k + 1], _tail_gpu(one, in_place)), k


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("H,W,C", [(135, 240, 256), (64, 64, 1024), (17, 30, 2048), (1, 1, 1024)])
def test_tail_kernel_against_fp64(H, W, C, in_place, dtype):
    _tail_case(3, H, W, C, dtype, in_place)


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("H,W,C", [(256, 256, 256), (32, 32, 2048)])
def test_tail_kernel_on_the_headline_shapes(H, W, C, in_place, dtype):
    """8 x 256^2 x 256 (stage 1 at 8 x 1024^2: 537 MB per fp32 tensor, 128 pool slabs per sample) and 8 x 32^2 x 2048
    (stage 4)."""
    _tail_case(8, H, W, C, dtype, in_place)


# ------------------------------------------------------------------ backbone taps
@pytest.mark.parametrize("bt", REF.TYPES)
@pytest.mark.parametrize("shape,outputs", [
    ((1, 540, 960, 3), ("C3", "C4", "C5", "P6", "P7")),              # the serving size: 68x120 .. 9x15
    ((2, 200, 328, 3), ("C1", "C2", "C3", "C4", "C5", "P6", "P7")),  # odd maps: 50x82, 25x41, 13x21, 7x11, 4x6, 2x3
])
def test_backbone_taps_match_the_restatement(bt, shape, outputs):
    """f32 / f32x3 within the BASELINE tolerance, f16 (fp16 operands, fp32 tensors and tail) within the SE-ResNet-34 f16
    bar; f16s (half tensors from the stem on, half tail, half taps) is reported, not gated."""
    bb, w = CASES.load_backbone(bt, outputs, seed=shape[1])
    images = np.random.default_rng(shape[2]).integers(0, 256, shape, dtype=np.uint8)
    names, want = REF.backbone_forward(images.astype(np.float32), w, bt, outputs)
    assert names == bb.output_names
    for math in ("f32", "f32x3", "f16", "f16s"):
        CASES.check_taps(names, CASES.run_backbone(bb, images, math)[0], want, math, f"senet taps {bt} {shape}")


# ------------------------------------------------------------------ end to end
def _config(bt):
    """The SE-ResNet-34 shipped head configuration (road_project/train.py:36-58) on an SENet-50 backbone with the default
    taps C3, C4, C5, P6, P7."""
    return CASES.shipped_se_config(bt, ('C3', 'C4', 'C5', 'P6', 'P7'))


@pytest.mark.parametrize("bt", REF.TYPES)
def test_end_to_end_on_the_senet_backbones(bt, monkeypatch):
    REF.patch(monkeypatch)
    cfg = _config(bt)
    model, w, images = CASES.order_stable_fixture(cfg, (2, 200, 328, 3), seed=5)
    assert model.backbone_network.output_names == ['C3', 'C4', 'C5', 'P6', 'P7']
    model.load_weights(w, "cuda:0")
    want, internals = O.inference_forward(cfg, w, images, literal_groups=False, return_internals=True)
    CASES.check_kept_rows_device_counts_and_graph(model, images, want, internals["kept"])


def test_f16s_end_to_end_on_seresnext50(monkeypatch):
    """Half tensors from the fused stem on, the half SE tail, half taps into the heads: the predictions within the bar
    of every f16s model test against the fp32 restatement."""
    from masklab_hip import ModelConfiguration, ops, retinamasklab as R
    REF.patch(monkeypatch)
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = "seresnext50"
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(3)
    model.load_weights(w, "cuda:0")
    images = np.random.default_rng(1234).integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)
    ops.set_conv_math("f16s")
    try:
        ops.PROFILE = []
        got = model.predict(images)
        recs, ops.PROFILE = ops.PROFILE, None
    finally:
        ops.PROFILE = None
        ops.set_conv_math("f32")
    kernels = {r["kernel"] for r in recs}
    assert {"se_bottleneck_h", "gconv3x3_mfma4_h", "stem7x7s2_pool_h"} <= kernels, kernels     # the half path ran
    want = O.inference_forward(cfg, w, images, literal_groups=False)
    worst = {}
    for name, g, r in zip(model.output_names, got, want):
        assert g.shape == r.shape and g.dtype == np.float32, name
        if name in ("cls_pred", "loc_pred", "seg_pred"):
            worst[name] = float(np.abs(g.astype(np.float64) - r).max())
    print(f"\n[senet f16s e2e] {worst}")
    assert sorted(worst) == ["cls_pred", "loc_pred", "seg_pred"]
    for name, e in worst.items():
        assert e <= F16_MODEL_TOL, (name, e)
    assert max(worst.values()) > 1e-6, "suspiciously exact: the fp16 path did not run"


def test_checkpoint_to_deploy_model_at_the_serving_size(tmp_path, monkeypatch):
    """An .npz of init_weights through load_masklab_inference_model_from_h5 -> DeployModel on a 1080x1920 frame (down-
    sampled to the 540x960 working size) against oracle.deploy_forward with the restated backbone (seresnext50)."""
    REF.patch(monkeypatch)
    CASES.check_checkpoint_to_deploy(_config("seresnext50"), tmp_path / "seresnext50.npz", (1, 1080, 1920, 3), seed=1080)
