"""GPU tests of the SE-ResNet-34 backbone (the reference project's own model, road_project/train.py:36-37): the fused SE
block tail (csrc/se_residual.hip) against an fp64 NumPy formulation, bit-stable run to run and per image; the backbone
taps against the test-side restatement (tests/backbone_refs.py) in the fp32 conv maths; the shipped configuration on its
real backbone against the oracle with detections, eagerly, with device counts and as one hipGraph; 'f16s' refused; an
.npz checkpoint through load_masklab_inference_model_from_h5 to the deploy model.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import masklab as O

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import backbone_cases as CASES
from backbone_refs import SERESNET34 as REF


# ------------------------------------------------------------------ the tail kernel
def _tail_problem(B, H, W, C, seed):
    rng = np.random.default_rng(seed)
    Hd = max(1, C // 16)
    f = lambda *s, sd=1.0: (rng.standard_normal(s) * sd).astype(np.float32)
    return dict(x=f(B, H, W, C), sc=f(B, H, W, C), w1=f(C, Hd, sd=np.sqrt(2.0 / C)), b1=f(Hd, sd=0.1),
                w2=f(Hd, C, sd=np.sqrt(2.0 / Hd)), b2=f(C, sd=0.1), scale=(rng.uniform(0.3, 1.5, C)).astype(np.float32),
                shift=f(C, sd=0.2))


def _tail_ref(p):
    x = p["x"].astype(np.float64)
    m = x.mean(axis=(1, 2))                                                       # [B, C]
    h = np.maximum(m @ p["w1"].astype(np.float64) + p["b1"], 0.0)
    g = 1.0 / (1.0 + np.exp(-(h @ p["w2"].astype(np.float64) + p["b2"])))
    y = x * g[:, None, None, :] + p["sc"]
    return np.maximum(y * p["scale"] + p["shift"], 0.0), y


def _tail_gpu(p, want_y, mode="gate"):
    from masklab_hip import ops
    if mode == "bn_relu":
        return ops.bn_relu(dev(p["x"]), dev(p["scale"]), dev(p["shift"])), None
    return ops.se_residual(dev(p["x"]), dev(p["sc"]), dev(p["w1"]), dev(p["b1"]), dev(p["w2"]), dev(p["b2"]),
                           dev(p["scale"]), dev(p["shift"]), want_y=want_y)


@pytest.mark.parametrize("H,W,C", [(135, 240, 64), (17, 30, 512), (1, 1, 128)])
@pytest.mark.parametrize("mode", ["gate", "gate+y", "bn_relu"])
def test_tail_kernel_against_fp64(H, W, C, mode):
    B = 3
    p = _tail_problem(B, H, W, C, seed=H * 1000 + C)
    act, y = _tail_gpu(p, mode == "gate+y", "bn_relu" if mode == "bn_relu" else "gate")
    if mode == "bn_relu":
        want = np.maximum(p["x"].astype(np.float64) * p["scale"] + p["shift"], 0.0)
        np.testing.assert_allclose(host(act), want, rtol=1e-5, atol=1e-6)
        assert y is None
    else:
        want_act, want_y = _tail_ref(p)
        np.testing.assert_allclose(host(act), want_act, rtol=1e-5, atol=1e-6)
        if mode == "gate+y":
            np.testing.assert_allclose(host(y), want_y, rtol=1e-5, atol=1e-6)
        else:
            assert y is None
    # repeated launches: the same bits
    act2, y2 = _tail_gpu(p, mode == "gate+y", "bn_relu" if mode == "bn_relu" else "gate")
    assert torch.equal(act, act2)
    if y is not None:
        assert torch.equal(y, y2)
    # image k of the batch == image k alone
    for k in range(B):
        one = {n: (v[k:k + 1] if v.ndim == 4 else v) for n, v in p.items()}
        a1, y1 = _tail_gpu(one, mode == "gate+y", "bn_relu" if mode == "bn_relu" else "gate")
        assert torch.equal(act[k:k + 1], a1), k
        if y is not None:
            assert torch.equal(y[k:k + 1], y1), k


def test_tail_kernel_on_the_stage1_shape_of_the_headline_batch():
    """8 x 256^2 x 64 (the 1024^2 stage-1 map, 134 MB per tensor): 64 pool slabs per sample, 2048 tail blocks."""
    B, H, W, C = 8, 256, 256, 64
    p = _tail_problem(B, H, W, C, seed=11)
    act, y = _tail_gpu(p, True)
    want_act, want_y = _tail_ref(p)
    np.testing.assert_allclose(host(act), want_act, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(y), want_y, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ backbone taps
@pytest.mark.parametrize("math", ["f32", "f32x3"])
@pytest.mark.parametrize("shape,outputs", [
    ((1, 540, 960, 3), ("C3", "C4", "C5", "P6")),                      # the recorded serving size: 68x120 .. 9x15
    ((2, 200, 328, 3), ("C1", "C2", "C3", "C4", "C5", "P6", "P7")),    # odd maps: 50x82, 25x41, 13x21, 7x11, 4x6, 2x3
])
def test_backbone_taps_match_the_restatement(math, shape, outputs):
    bb, w = CASES.load_backbone("seresnet34", outputs, seed=shape[1])
    images = np.random.default_rng(shape[2]).integers(0, 256, shape, dtype=np.uint8)
    names, want = REF.backbone_forward(images.astype(np.float32), w, "seresnet34", outputs)
    assert names == bb.output_names
    CASES.check_taps(names, CASES.run_backbone(bb, images, math)[0], want, math, f"seresnet34 taps {shape}")


def test_backbone_runs_in_the_f16_conv_math():
    """fp16 MFMA operands, fp32 tensors: the tail stays fp32; the taps stay within the fp16-operand model bar."""
    outputs = ("C3", "C4", "C5", "P6")
    bb, w = CASES.load_backbone("seresnet34", outputs, seed=2)
    images = np.random.default_rng(2).integers(0, 256, (1, 200, 328, 3), dtype=np.uint8)
    names, want = REF.backbone_forward(images.astype(np.float32), w, "seresnet34", outputs)
    CASES.check_taps(names, CASES.run_backbone(bb, images, "f16")[0], want, "f16", "seresnet34 taps")


# ------------------------------------------------------------------ the shipped configuration, end to end
def _shipped_config():
    """road_project/train.py:36-58: seresnet34 with taps C3, C4, C5, P6."""
    return CASES.shipped_se_config("seresnet34", ('C3', 'C4', 'C5', 'P6'))


def test_shipped_configuration_on_its_real_backbone(monkeypatch):
    REF.patch(monkeypatch)
    cfg = _shipped_config()
    model, w, images = CASES.order_stable_fixture(cfg, (2, 200, 328, 3), seed=5)
    assert model.backbone_network.output_names == ['C3', 'C4', 'C5', 'P6']
    model.load_weights(w, "cuda:0")
    want, internals = O.inference_forward(cfg, w, images, literal_groups=False, return_internals=True)
    CASES.check_kept_rows_device_counts_and_graph(model, images, want, internals["kept"])


def test_f16s_is_refused_with_this_backbone():
    from masklab_hip import ops, retinamasklab as R
    _, model = R.construct_masklab_networks(_shipped_config())
    model.load_weights(model.init_weights(1), "cuda:0")
    images = np.zeros((1, 64, 64, 3), np.uint8)
    ops.set_conv_math("f16s")
    try:
        with pytest.raises(NotImplementedError, match="f16s"):
            model.predict(images)
    finally:
        ops.set_conv_math("f32")


def test_checkpoint_to_deploy_model_at_the_serving_size(tmp_path, monkeypatch):
    """An .npz of init_weights through load_masklab_inference_model_from_h5 -> DeployModel on a 1080x1920 frame (down-
    sampled to the 540x960 working size) against oracle.deploy_forward with the restated backbone."""
    REF.patch(monkeypatch)
    CASES.check_checkpoint_to_deploy(_shipped_config(), tmp_path / "seresnet34.npz", (1, 1080, 1920, 3), seed=1080)
