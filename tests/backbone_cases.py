"""What the GPU tests of the restated backbones share (test infrastructure, not collected: no `test_` prefix): tensors to
and from the device, a backbone with synthetic weights loaded, the bars on its taps per conv math, the bars on the model
outputs, the reference project's shipped SqueezeExcite head configuration, the order-stable detection fixture, and the two
end-to-end sequences (kept rows -> device counts -> one hipGraph replayed twice; checkpoint -> deploy model)."""
import numpy as np
import pytest
import torch

from oracle import masklab as O

TOL = 1e-3                          # BASELINE.json north_star: float outputs within 1e-3 in the fp32 conv maths
ALL_OUTPUTS = ("C1", "C2", "C3", "C4", "C5", "P6", "P7")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------ backbone taps
def load_backbone(bt, outputs, seed):
    """-> (backbone with init_weights(seed) on the device, those weights); the draw is per weight name, so two backbones
    of one type and seed share every weight they both have."""
    from masklab_hip import backbone as BB
    from masklab_hip import keras_like as K
    K.clear_session()
    bb = BB.load_backbone(bt, backbone_outputs=outputs, num_features=128)
    w = K.init_weights(bb.weight_specs(), seed)
    bb.load_weights(w, torch.device("cuda:0"))
    return bb, w


def run_backbone(bb, images, math="f32"):
    """-> (the outputs on the host, the names of the kernels launched, in order) under the conv math `math`."""
    from masklab_hip import ops
    ops.set_conv_math(math)
    ops.PROFILE = []
    try:
        got = [host(t) for t in bb(dev(images))]
        kernels = [r["kernel"] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
        ops.set_conv_math("f32")
    return got, kernels


def check_taps(names, got, want, math, label):
    """f32 / f32x3 within the BASELINE tolerance, f16 (fp16 operands, fp32 tensors) within the fp16-operand model bar; f16s
    (half tensors from the stem on, half taps) is reported, not gated."""
    errs = {}
    for n, g, r in zip(names, got, want):
        assert g.shape == r.shape, (n, g.shape, r.shape)
        assert g.dtype == (np.float16 if math == "f16s" else np.float32), (math, n, g.dtype)
        errs[n] = float(np.max(np.abs(g.astype(np.float64) - r)))
        bar = TOL if math in ("f32", "f32x3") else 3e-2 * max(1.0, float(np.abs(r).max()) / 4)
        if math != "f16s":
            assert errs[n] <= bar, (label, math, n, errs[n], bar)
    print(f"\n[{label}] {math}: " + " ".join(f"{n}={e:.3g}" for n, e in errs.items()))


# ------------------------------------------------------------------ end to end
def check_model(model, got, want):
    for name, g, r in zip(model.output_names, got, want):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if name == "roi_boxes":
            np.testing.assert_array_equal(g[..., 4], r[..., 4], err_msg="class ids")
            np.testing.assert_array_equal(g == -1, r == -1, err_msg="padding pattern")
            # pixel coordinates are O(100): fp32 relative tolerance; confidences absolute
            np.testing.assert_allclose(g[..., :4], r[..., :4], rtol=1e-5, atol=TOL)
            np.testing.assert_allclose(g[..., 5], r[..., 5], rtol=0, atol=TOL)
            continue
        err = float(np.max(np.abs(g.astype(np.float64) - r))) if g.size else 0.0
        assert err <= TOL, (name, err)


def shipped_se_config(bt, outputs):
    """The head configuration the reference project ships (road_project/train.py:36-58) on backbone `bt` with the taps
    `outputs`: tower depth 3; prior ratios 1/2, 1, 2, 5, 8; SqueezeExcite in every head."""
    from masklab_hip import ModelConfiguration
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = bt
    cfg.backbone.backbone_outputs = outputs
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


def order_stable_fixture(cfg, shape, seed):
    """-> (model, weights, images) with an order-stable logit scale from the oracle forward (oracle/fixtures.py): class
    logits scaled so that scores pass min_confidence without saturating, min_confidence (set on `cfg` and the model) in a
    score gap.  A restated backbone needs its patch() in place."""
    from masklab_hip import retinamasklab as R
    from oracle import fixtures as FX
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(seed)
    images = np.random.default_rng(shape[1] + shape[2]).integers(0, 256, shape, dtype=np.uint8)
    c1, l1 = O.inference_forward(cfg, w, images, literal_groups=False, with_instance=False, with_semantic=False)
    scale, thr = FX.choose_logit_scale(cfg, c1, l1, shape[1], shape[2])
    assert scale is not None, "no order-stable logit scale on the grid"
    cfg.detection.min_confidence = thr
    model.detection_proposal.min_confidence = thr
    return model, FX.scale_cls_logits(w, scale), images


def check_kept_rows_device_counts_and_graph(model, images, want, kept_ref):
    """`model` (weights loaded) against the oracle's outputs `want` and kept (image, anchor, class) rows `kept_ref`: eagerly
    with the kept rows in the oracle's order, through the fixed-capacity stage 2, and as one hipGraph replayed twice."""
    assert len(kept_ref) > 0, "fixture produced no detections"
    got = model.predict(images, want_kept=True)
    det = model.last_detections
    counts, kept = det["counts"].cpu().numpy(), det["kept"].cpu().numpy()
    for b in range(images.shape[0]):
        np.testing.assert_array_equal(kept[b, :counts[b]], kept_ref[kept_ref[:, 0] == b][:, 1:])
    check_model(model, got, want)
    model.device_counts = True                       # stage 2 at capacity, no host read inside the forward
    eager = model.predict(images)
    check_model(model, eager, want)
    model.enable_graphs(True)                        # the whole forward as ONE hipGraph: first pass captures, then replays
    for _ in range(2):
        replay = model.predict(images)
        for name, g, r in zip(model.output_names, replay, eager):
            np.testing.assert_array_equal(g, r, err_msg=name)
    model.enable_graphs(False)
    model.device_counts = "auto"


def check_checkpoint_to_deploy(cfg, path, frame, seed):
    """An .npz of init_weights(3) (class logits widened) at `path` through load_masklab_inference_model_from_h5 ->
    DeployModel on one `frame`-sized image drawn from `seed`, against oracle.deploy_forward.  -> the weights."""
    from masklab_hip import retinamasklab as R
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(3)
    for k in w:
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)          # some anchors pass min_confidence
    np.savez(path, **w)
    deploy = R.load_masklab_inference_model_from_h5(str(path), cfg, device="cuda:0")
    images = np.random.default_rng(seed).integers(0, 256, frame, dtype=np.uint8)
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
    return w
