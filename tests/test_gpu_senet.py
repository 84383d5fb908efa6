"""GPU tests of the SE-ResNet-50 and SE-ResNeXt-50 backbones (vendored thirdparty senet.py, offered by the reference's
load_backbone): the fused SE bottleneck tail (csrc/se_bottleneck.hip) against an fp64 NumPy formulation in fp32 and in
half storage, bit-stable run to run and per image; the backbone taps against the test-side restatement
(tests/senet_ref.py) in every conv math; both backbones end to end against the oracle with detections, device counts and
one hipGraph; SE-ResNeXt-50 in 'f16s' end to end; an .npz checkpoint through load_masklab_inference_model_from_h5 to the
deploy model.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import masklab as O

import senet_ref as REF

TOL = 1e-3
F16_MODEL_TOL = 3e-2


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
def _backbone(bt, outputs, seed):
    from masklab_hip import backbone as BB
    from masklab_hip import keras_like as K
    K.clear_session()
    bb = BB.load_backbone(bt, backbone_outputs=outputs, num_features=128)
    w = K.init_weights(bb.weight_specs(), seed)
    bb.load_weights(w, torch.device("cuda:0"))
    return bb, w


@pytest.mark.parametrize("bt", REF.TYPES)
@pytest.mark.parametrize("shape,outputs", [
    ((1, 540, 960, 3), ("C3", "C4", "C5", "P6", "P7")),              # the serving size: 68x120 .. 9x15
    ((2, 200, 328, 3), ("C1", "C2", "C3", "C4", "C5", "P6", "P7")),  # odd maps: 50x82, 25x41, 13x21, 7x11, 4x6, 2x3
])
def test_backbone_taps_match_the_restatement(bt, shape, outputs):
    """f32 / f32x3 within the BASELINE tolerance, f16 (fp16 operands, fp32 tensors and tail) within the SE-ResNet-34 f16
    bar; f16s (half tensors from the stem on, half tail, half taps) is reported, not gated."""
    from masklab_hip import ops
    bb, w = _backbone(bt, outputs, seed=shape[1])
    images = np.random.default_rng(shape[2]).integers(0, 256, shape, dtype=np.uint8)
    names, want = REF.backbone_forward(images.astype(np.float32), w, bt, outputs)
    assert names == bb.output_names
    for math in ("f32", "f32x3", "f16", "f16s"):
        ops.set_conv_math(math)
        try:
            got = [host(t) for t in bb(dev(images))]
        finally:
            ops.set_conv_math("f32")
        errs = {}
        for n, g, r in zip(names, got, want):
            assert g.shape == r.shape, (n, g.shape, r.shape)
            assert g.dtype == (np.float16 if math == "f16s" else np.float32), (math, n, g.dtype)
            errs[n] = float(np.max(np.abs(g.astype(np.float64) - r)))
            bar = TOL if math in ("f32", "f32x3") else 3e-2 * max(1.0, float(np.abs(r).max()) / 4)
            if math != "f16s":
                assert errs[n] <= bar, (bt, math, n, errs[n], bar)
        print(f"\n[senet taps] {bt} {shape} {math}: " + " ".join(f"{n}={e:.3g}" for n, e in errs.items()))


# ------------------------------------------------------------------ end to end
def _config(bt):
    """The SE-ResNet-34 shipped head configuration (road_project/train.py:36-58) on an SENet-50 backbone with the default
    taps C3, C4, C5, P6, P7."""
    from masklab_hip import ModelConfiguration
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = bt
    cfg.backbone.backbone_outputs = ('C3', 'C4', 'C5', 'P6', 'P7')
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


E2E_SHAPE, E2E_SEED = (2, 200, 328, 3), 5


def _fixture(bt):
    """(cfg, model, weights, images) with an order-stable logit scale from the restated forward."""
    from masklab_hip import retinamasklab as R
    from oracle import fixtures as FX
    cfg = _config(bt)
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(E2E_SEED)
    images = np.random.default_rng(E2E_SHAPE[1] + E2E_SHAPE[2]).integers(0, 256, E2E_SHAPE, dtype=np.uint8)
    c1, l1 = O.inference_forward(cfg, w, images, literal_groups=False, with_instance=False, with_semantic=False)
    scale, thr = FX.choose_logit_scale(cfg, c1, l1, E2E_SHAPE[1], E2E_SHAPE[2])
    assert scale is not None, "no order-stable logit scale on the grid"
    w = FX.scale_cls_logits(w, scale)
    cfg.detection.min_confidence = thr
    model.detection_proposal.min_confidence = thr
    return cfg, model, w, images


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


@pytest.mark.parametrize("bt", REF.TYPES)
def test_end_to_end_on_the_senet_backbones(bt, monkeypatch):
    REF.patch(monkeypatch)
    cfg, model, w, images = _fixture(bt)
    assert model.backbone_network.output_names == ['C3', 'C4', 'C5', 'P6', 'P7']
    model.load_weights(w, "cuda:0")
    want, internals = O.inference_forward(cfg, w, images, literal_groups=False, return_internals=True)
    kept_ref = internals["kept"]
    assert len(kept_ref) > 0, "fixture produced no detections"
    got = model.predict(images, want_kept=True)
    det = model.last_detections
    counts, kept = det["counts"].cpu().numpy(), det["kept"].cpu().numpy()
    for b in range(E2E_SHAPE[0]):
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
    from masklab_hip import retinamasklab as R
    REF.patch(monkeypatch)
    cfg = _config("seresnext50")
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(3)
    for k in w:
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)          # some anchors pass min_confidence
    path = tmp_path / "seresnext50.npz"
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
