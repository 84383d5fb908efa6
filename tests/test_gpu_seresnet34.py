"""GPU tests of the SE-ResNet-34 backbone (the reference project's own model, road_project/train.py:36-37): the fused SE
block tail (csrc/se_residual.hip) against an fp64 NumPy formulation, bit-stable run to run and per image; the backbone
taps against the test-side restatement (tests/seresnet34_ref.py) in the fp32 conv maths; the shipped configuration on its
real backbone against the oracle with detections, eagerly, with device counts and as one hipGraph; 'f16s' refused; an
.npz checkpoint through load_masklab_inference_model_from_h5 to the deploy model.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import masklab as O

import seresnet34_ref as REF

TOL = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


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
def _backbone(outputs, seed):
    from masklab_hip import backbone as BB
    from masklab_hip import keras_like as K
    K.clear_session()
    bb = BB.load_backbone("seresnet34", backbone_outputs=outputs, num_features=128)
    w = K.init_weights(bb.weight_specs(), seed)
    bb.load_weights(w, torch.device("cuda:0"))
    return bb, w


@pytest.mark.parametrize("math", ["f32", "f32x3"])
@pytest.mark.parametrize("shape,outputs", [
    ((1, 540, 960, 3), ("C3", "C4", "C5", "P6")),                      # the recorded serving size: 68x120 .. 9x15
    ((2, 200, 328, 3), ("C1", "C2", "C3", "C4", "C5", "P6", "P7")),    # odd maps: 50x82, 25x41, 13x21, 7x11, 4x6, 2x3
])
def test_backbone_taps_match_the_restatement(math, shape, outputs):
    from masklab_hip import ops
    bb, w = _backbone(outputs, seed=shape[1])
    images = np.random.default_rng(shape[2]).integers(0, 256, shape, dtype=np.uint8)
    names, want = REF.backbone_forward(images.astype(np.float32), w, "seresnet34", outputs)
    ops.set_conv_math(math)
    try:
        got = [host(t) for t in bb(dev(images))]
    finally:
        ops.set_conv_math("f32")
    assert names == bb.output_names
    for n, g, r in zip(names, got, want):
        assert g.shape == r.shape, (n, g.shape, r.shape)
        err = float(np.max(np.abs(g.astype(np.float64) - r)))
        assert err <= TOL, (math, n, err)


def test_backbone_runs_in_the_f16_conv_math():
    """fp16 MFMA operands, fp32 tensors: the tail stays fp32; the taps stay within the fp16-operand model bar."""
    from masklab_hip import ops
    outputs = ("C3", "C4", "C5", "P6")
    bb, w = _backbone(outputs, seed=2)
    images = np.random.default_rng(2).integers(0, 256, (1, 200, 328, 3), dtype=np.uint8)
    names, want = REF.backbone_forward(images.astype(np.float32), w, "seresnet34", outputs)
    ops.set_conv_math("f16")
    try:
        got = [host(t) for t in bb(dev(images))]
    finally:
        ops.set_conv_math("f32")
    for n, g, r in zip(names, got, want):
        assert g.dtype == np.float32 and g.shape == r.shape
        assert float(np.max(np.abs(g - r))) <= 3e-2 * max(1.0, float(np.abs(r).max()) / 4), n


# ------------------------------------------------------------------ the shipped configuration, end to end
def _shipped_config():
    """road_project/train.py:36-58: seresnet34 with taps C3, C4, C5, P6; tower depth 3; prior ratios 1/2, 1, 2, 5, 8;
    SqueezeExcite in every head."""
    from masklab_hip import ModelConfiguration
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = 'seresnet34'
    cfg.backbone.backbone_outputs = ('C3', 'C4', 'C5', 'P6')
    cfg.detection.num_features = 128
    cfg.detection.num_depth = 3
    cfg.detection.use_squeeze_excite = True
    cfg.detection.pr_scales = [2 ** 0, 2 ** (1 / 3), 2 ** (2 / 3)]
    cfg.detection.pr_ratios = [1 / 2, 1, 2, 5, 8]
    cfg.instance.crop_size = (14, 14)
    cfg.instance.max_k = 2
    cfg.instance.num_features = 128
    cfg.instance.num_depth = 4
    cfg.instance.use_squeeze_excite = True
    cfg.semantic.num_features = 128
    cfg.semantic.num_depth = 3
    cfg.semantic.use_squeeze_excite = True
    return cfg


def _check(model, got, want):
    for name, g, r in zip(model.output_names, got, want):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if name == "roi_boxes":
            np.testing.assert_array_equal(g[..., 4], r[..., 4], err_msg="class ids")
            np.testing.assert_array_equal(g == -1, r == -1, err_msg="padding pattern")
            np.testing.assert_allclose(g[..., :4], r[..., :4], rtol=1e-5, atol=TOL)
            np.testing.assert_allclose(g[..., 5], r[..., 5], rtol=0, atol=TOL)
            continue
        err = float(np.max(np.abs(g.astype(np.float64) - r))) if g.size else 0.0
        assert err <= TOL, (name, err)


def test_shipped_configuration_on_its_real_backbone(monkeypatch):
    from masklab_hip import retinamasklab as R
    from oracle import fixtures as FX
    REF.patch(monkeypatch)
    shape = (2, 200, 328, 3)
    cfg = _shipped_config()
    _, model = R.construct_masklab_networks(cfg)
    assert model.backbone_network.output_names == ['C3', 'C4', 'C5', 'P6']
    w = model.init_weights(5)
    images = np.random.default_rng(shape[1] + shape[2]).integers(0, 256, shape, dtype=np.uint8)
    c1, l1 = O.inference_forward(cfg, w, images, literal_groups=False, with_instance=False, with_semantic=False)
    scale, thr = FX.choose_logit_scale(cfg, c1, l1, shape[1], shape[2])
    assert scale is not None, "no order-stable logit scale on the grid"
    w = FX.scale_cls_logits(w, scale)
    model.load_weights(w, "cuda:0")
    cfg.detection.min_confidence = thr
    model.detection_proposal.min_confidence = thr
    want, internals = O.inference_forward(cfg, w, images, literal_groups=False, return_internals=True)
    kept_ref = internals["kept"]
    assert len(kept_ref) > 0, "fixture produced no detections"
    got = model.predict(images, want_kept=True)
    det = model.last_detections
    counts, kept = det["counts"].cpu().numpy(), det["kept"].cpu().numpy()
    for b in range(shape[0]):
        np.testing.assert_array_equal(kept[b, :counts[b]], kept_ref[kept_ref[:, 0] == b][:, 1:])
    _check(model, got, want)
    model.device_counts = True                       # stage 2 at capacity, no host read inside the forward
    eager = model.predict(images)
    _check(model, eager, want)
    model.enable_graphs(True)                        # the whole forward as ONE hipGraph: first pass captures, then replays
    for _ in range(2):
        replay = model.predict(images)
        for name, g, r in zip(model.output_names, replay, eager):
            np.testing.assert_array_equal(g, r, err_msg=name)
    model.enable_graphs(False)
    model.device_counts = "auto"


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
    from masklab_hip import retinamasklab as R
    REF.patch(monkeypatch)
    cfg = _shipped_config()
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(3)
    for k in w:
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)          # some anchors pass min_confidence
    path = tmp_path / "seresnet34.npz"
    np.savez(path, **w)
    deploy = R.load_masklab_inference_model_from_h5(str(path), cfg, device="cuda:0")
    images = np.random.default_rng(1080).integers(0, 256, (1, 1080, 1920, 3), dtype=np.uint8)
    det, inst, sem = deploy.predict(images)
    wdet, winst, wsem = O.deploy_forward(cfg, w, images, literal_groups=False)
    assert det.dtype == inst.dtype == sem.dtype == np.int32
    assert det.shape == wdet.shape and inst.shape == winst.shape and sem.shape == wsem.shape == images.shape
    assert (wdet[..., 4] >= 0).sum() > 0, "fixture produced no detections"
    assert 0 < wsem.mean() < 1 and 0 < winst.mean() < 1, "fixture thresholds are degenerate"
    np.testing.assert_array_equal(det[..., 4], wdet[..., 4])                   # labels and padding pattern
    assert np.abs(det - wdet).max() <= 1                                       # truncation of x*ratio at an integer
    assert (det != wdet).mean() < 0.02
    assert (inst != winst).mean() < 1e-3 and (sem != wsem).mean() < 1e-3      # flips only at |v - 0.5| < 1e-3
