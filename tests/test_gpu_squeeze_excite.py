"""The fused SqueezeExcite (csrc/squeeze_excite.hip, ops.squeeze_excite_multi) and the half skip-add against the fp64
oracle, and the configuration the reference project ships (SqueezeExcite in every head) in every conv math and as ONE
whole-forward hipGraph.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import masklab as O

TOL = 1e-3
F16_MODEL_TOL = 3e-2
SHAPES = [(2, 32, 48, 128, 8), (1, 160, 160, 128, 8), (2, 64, 64, 160, 10), (2, 16, 16, 256, 16)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _weights(rng, C, Hd):
    return ((rng.standard_normal((C, Hd)) * np.sqrt(2.0 / C)).astype(np.float32),
            (rng.standard_normal((Hd, C)) * np.sqrt(1.0 / Hd)).astype(np.float32))


def _oracle(x, w1, w2):
    """oracle.masklab.squeeze_excite in fp64 (the Dense kernels under the names the layer gives them)."""
    return O.squeeze_excite(x.astype(np.float64), {"se/dense1/kernel": w1, "se/dense2/kernel": w2}, "se")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dtype)


def _half_bar(got, ref64):
    """The repo's half bar (tests/test_gpu_f16_heads.py): the fp64 oracle on the half-rounded input, rounded once."""
    want = ref64.astype(np.float16).astype(np.float64)
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=2 ** -10, atol=1e-4)


@pytest.mark.parametrize("B,H,W,C,Hd", SHAPES)
def test_squeeze_excite_f32(B, H, W, C, Hd):
    from masklab_hip import ops
    rng = np.random.default_rng(C + H)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32) + 0.25
    w1, w2 = _weights(rng, C, Hd)
    ref = _oracle(x, w1, w2)
    xd = _dev(x)
    out = ops.squeeze_excite_multi([dict(x=xd, w1=_dev(w1), w2=_dev(w2), out=torch.empty_like(xd))])[0]
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    assert torch.equal(xd.cpu(), torch.from_numpy(x)), "out of place: the input must be unchanged"
    inplace = ops.squeeze_excite_multi([dict(x=xd, w1=_dev(w1), w2=_dev(w2))])[0]
    assert inplace.data_ptr() == xd.data_ptr()
    assert torch.equal(inplace, out)


@pytest.mark.parametrize("B,H,W,C,Hd", SHAPES)
def test_squeeze_excite_half_storage(B, H, W, C, Hd):
    from masklab_hip import ops
    rng = np.random.default_rng(C + H + 1)
    xh = (rng.standard_normal((B, H, W, C)) + 0.25).astype(np.float16)
    w1, w2 = _weights(rng, C, Hd)
    ref = _oracle(xh.astype(np.float32), w1, w2)
    xd = _dev(xh, torch.float16)
    out = ops.squeeze_excite_multi([dict(x=xd, w1=_dev(w1), w2=_dev(w2), out=torch.empty_like(xd))])[0]
    assert out.dtype == torch.float16
    _half_bar(out.cpu().numpy(), ref)
    assert np.array_equal(xd.cpu().numpy(), xh)
    ops.squeeze_excite_multi([dict(x=xd, w1=_dev(w1), w2=_dev(w2))])
    assert torch.equal(xd, out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_squeeze_excite_multi_problem_and_live_slots(dtype):
    """3 levels of a fixed-capacity RoI batch (3 images x 7 slots, 14x14, C 128) in ONE call, with live counts 0, 4, 7:
    the dead slots of `out` keep their sentinel bit for bit, the live ones match the oracle; plus two plain problems of
    other sizes in the same call."""
    from masklab_hip import ops
    rng = np.random.default_rng(5)
    cap, imgs, C, Hd = 7, 3, 128, 8
    probs, refs, lives = [], [], (0, 4, 7)
    for lv in lives:
        x = (rng.standard_normal((imgs * cap, 14, 14, C)) + 0.25).astype(np.float32)
        if dtype == torch.float16:
            x = x.astype(np.float16).astype(np.float32)
        w1, w2 = _weights(rng, C, Hd)
        out = torch.full((imgs * cap, 14, 14, C), -7.0, dtype=dtype, device="cuda")
        probs.append(dict(x=_dev(x, dtype), w1=_dev(w1), w2=_dev(w2), out=out,
                          live=(torch.tensor([lv], dtype=torch.int32, device="cuda"), cap)))
        refs.append(_oracle(x, w1, w2))
    for H, W in ((40, 24), (5, 3)):
        x = (rng.standard_normal((2, H, W, C)) + 0.25).astype(np.float32)
        if dtype == torch.float16:
            x = x.astype(np.float16).astype(np.float32)
        w1, w2 = _weights(rng, C, Hd)
        probs.append(dict(x=_dev(x, dtype), w1=_dev(w1), w2=_dev(w2), out=torch.empty((2, H, W, C), dtype=dtype, device="cuda")))
        refs.append(_oracle(x, w1, w2))
    outs = ops.squeeze_excite_multi(probs)
    for i, (o, r) in enumerate(zip(outs, refs)):
        got = o.float().cpu().numpy()
        if i < len(lives):
            alive = np.array([n % cap < max(1, lives[i]) for n in range(imgs * cap)])
            assert np.all(got[~alive] == -7.0), f"level {i}: a dead slot was written"
            got, r = got[alive], r[alive]
        if dtype == torch.float16:
            _half_bar(got, r)
        else:
            np.testing.assert_allclose(got, r, rtol=1e-5, atol=1e-5)


def test_squeeze_excite_reproducible_and_graph_equals_eager():
    from masklab_hip import ops
    rng = np.random.default_rng(9)
    shapes = [(2, 128, 96), (2, 64, 48), (2, 32, 24), (2, 16, 12)]
    xs = [_dev(rng.standard_normal((b, h, w, 128)).astype(np.float32)) for b, h, w in shapes]
    ws = [tuple(_dev(a) for a in _weights(rng, 128, 8)) for _ in shapes]

    def run(inputs):
        return ops.squeeze_excite_multi([dict(x=x, w1=a, w2=b, out=torch.empty_like(x)) for x, (a, b) in zip(inputs, ws)])

    e1, e2 = run(xs), run(xs)
    assert all(torch.equal(a, b) for a, b in zip(e1, e2))
    static = [x.clone() for x in xs]
    run(static)                                        # warm-up (workspace) before capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = run(static)
    fresh = [_dev(rng.standard_normal(tuple(x.shape)).astype(np.float32)) for x in xs]
    for s, f in zip(static, fresh):
        s.copy_(f)
    g.replay()
    torch.cuda.synchronize()
    eager = run(fresh)
    assert all(torch.equal(a, b) for a, b in zip(gout, eager))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099, 1 << 20])
def test_add_half(n):
    from masklab_hip import ops
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 4).astype(np.float16)
    y = (rng.standard_normal(n) * 4).astype(np.float16)
    xd, yd = _dev(x, torch.float16), _dev(y, torch.float16)
    ops.add_(xd, yd)
    want = (x.astype(np.float32) + y.astype(np.float32)).astype(np.float16)
    got = xd.cpu().numpy()
    ulp = np.abs(np.spacing(want.astype(np.float16))).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 0.5 * ulp + 1e-12)
    assert np.array_equal(yd.cpu().numpy(), y)
    with pytest.raises(ValueError):
        ops.add_(xd, _dev(y[: max(1, n - 1)] if n > 1 else np.zeros(2, np.float16), torch.float16))
    with pytest.raises(NotImplementedError):
        ops.add_(xd, yd.float())
    if n > 9:
        with pytest.raises(RuntimeError, match="aligned"):      # a view 2 bytes in: refused by the library
            ops.add_(xd[1:], yd[1:])


# ------------------------------------------------------------------------------------------- the shipped head config
def _shipped_head_config(bt):
    """The head configuration the reference project ships (road_project/train.py:36-58; restated from
    tests/test_gpu_model.py): four pyramid levels, 128 features, tower depth 3 (mask head 4), SqueezeExcite everywhere."""
    from masklab_hip import ModelConfiguration
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = bt
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


def _check_half(model, got, want):
    from oracle import metrics as OM
    names = model.output_names
    g, w = dict(zip(names, got)), dict(zip(names, want))
    for n in ("cls_pred", "loc_pred", "seg_pred"):
        assert float(np.abs(g[n].astype(np.float64) - w[n]).max()) <= F16_MODEL_TOL, n
    pr, rc, fm = OM.detection_iou_metric(g["roi_boxes"], w["roi_boxes"])
    assert max(abs(float(v[0]) - 1.0) for v in (pr, rc, fm)) <= 1e-6, (pr, rc, fm)


def _half_threshold(cfg, model, images, ref_cls, ref_loc):
    """min_confidence for the fp16-storage mode: the middle of a score gap wider than 2.2x the mode's measured score
    deviation whose oracle detections do not change under that much noise (as test_gpu_f16_heads.py)."""
    from oracle import fixtures as FX
    from oracle import metrics as OM
    H, W = images.shape[1:3]
    got0 = dict(zip(model.output_names, model.predict(images)))
    dev_cls = float(np.abs(got0["cls_pred"].astype(np.float64) - ref_cls).max())
    assert dev_cls <= F16_MODEL_TOL
    boxes_ref = FX.boxes_from(cfg, ref_loc, H, W)
    det = cfg.detection
    args = (det.nms_iou_threshold, det.post_iou_threshold, det.nms_max_output_size)
    sc = np.sort(ref_cls[(ref_cls > 0.5) & (ref_cls < 0.8)].astype(np.float64))
    gaps = np.diff(sc)
    for i in np.argsort(-gaps)[:12]:
        if gaps[i] <= 2.2 * dev_cls:
            break
        cand = float(np.float32((sc[i] + sc[i + 1]) / 2))
        base, _ = O.detection_proposal(ref_cls, boxes_ref, cand, *args)
        if (base[..., 4] >= 0).sum() < 4:
            continue
        rng = np.random.default_rng(0)
        ok = True
        for _ in range(4):
            noisy = (ref_cls.astype(np.float64) + rng.uniform(-dev_cls, dev_cls, ref_cls.shape)).astype(np.float32)
            p2, _ = O.detection_proposal(noisy, boxes_ref, cand, *args)
            ok = ok and abs(float(OM.detection_iou_metric(p2, base)[2][0]) - 1.0) <= 1e-6
        if ok:
            return cand
    pytest.fail(f"no usable score gap for the fp16-storage mode (deviation {dev_cls})")


def _shipped_model(bt, images):
    from masklab_hip import retinamasklab as R
    from oracle import fixtures as FX
    cfg = _shipped_head_config(bt)
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(5)
    c1, l1 = O.inference_forward(cfg, w, images, literal_groups=False, with_instance=False, with_semantic=False)
    scale, thr = FX.choose_logit_scale(cfg, c1, l1, images.shape[1], images.shape[2])
    assert scale is not None, "no order-stable logit scale on the grid"
    w = FX.scale_cls_logits(w, scale)
    model.load_weights(w, "cuda:0")
    return cfg, model, w, thr


@pytest.mark.parametrize("math", ["f32", "f32x3", "f16s"])
def test_shipped_head_config_in_every_conv_math(math):
    """The reference's shipped heads on ResNeXt-50: host-read stage 2, fixed-capacity stage 2 (device_counts) and the
    WHOLE forward as one hipGraph (two replays, bit-identical to the device_counts eager run), against the fp32 oracle."""
    from masklab_hip import ops
    images = np.random.default_rng(640).integers(0, 256, (2, 256, 384, 3), dtype=np.uint8)
    cfg, model, w, thr = _shipped_model("resnext50", images)
    ops.set_conv_math(math)
    try:
        if math == "f16s":
            ref_cls, ref_loc = O.inference_forward(cfg, w, images, literal_groups=False, with_instance=False,
                                                   with_semantic=False)
            thr = _half_threshold(cfg, model, images, ref_cls, ref_loc)
        cfg.detection.min_confidence = thr
        model.detection_proposal.min_confidence = thr
        want, internals = O.inference_forward(cfg, w, images, literal_groups=False, return_internals=True)
        assert len(internals["kept"]) > 0, "fixture produced no detections"
        check = _check_half if math == "f16s" else _check
        got = model.predict(images, want_kept=True)
        if math != "f16s":
            det = model.last_detections
            counts, kept = det["counts"].cpu().numpy(), det["kept"].cpu().numpy()
            kept_ref = internals["kept"]
            for b in range(images.shape[0]):
                np.testing.assert_array_equal(kept[b, :counts[b]], kept_ref[kept_ref[:, 0] == b][:, 1:])
        check(model, got, want)
        model.device_counts = True
        assert model._capacity_wanted(torch.from_numpy(images))
        eager = model.predict(images)
        check(model, eager, want)
        model.enable_graphs(True)
        for rep in range(2):
            g = model.predict(images)
            for name, a, b in zip(model.output_names, g, eager):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} (replay {rep})")
        assert len(model._graphs) == 1
        assert next(iter(model._graphs))[3] is True        # the WHOLE forward is the graph
    finally:
        model.enable_graphs(False)
        model.device_counts = "auto"
        ops.set_conv_math("f32")


def test_shipped_head_config_launch_structure(monkeypatch):
    """One eager fp32 forward under ops.PROFILE: the heads never call the unfused pooling / scaling ops, every SqueezeExcite
    depth is ONE launch pair (class tower 3 + mask head 4 + decoder 3 depths = 20 launches), and the class tower's convs
    are multi-problem launches over its four levels."""
    from masklab_hip import ops, retinamasklab as R
    cfg = _shipped_head_config("resnext50")
    _, model = R.construct_masklab_networks(cfg)
    model.load_weights(model.init_weights(5), "cuda:0")
    images = np.random.default_rng(3).integers(0, 256, (1, 256, 256, 3), dtype=np.uint8)
    model.predict(images)                                  # warm-up outside the hook

    def refuse(*a, **k):
        raise AssertionError("unfused SqueezeExcite op called")
    monkeypatch.setattr(ops, "scale_channels_", refuse)
    aspp_means = []
    real_mean = ops.global_mean
    monkeypatch.setattr(ops, "global_mean", lambda x: aspp_means.append(tuple(x.shape)) or real_mean(x))
    ops.PROFILE = []
    try:
        model.predict(images)
        torch.cuda.synchronize()
        recs = ops.PROFILE
    finally:
        ops.PROFILE = None
    se = [r for r in recs if r["kernel"].startswith("squeeze_excite_")]
    assert len(se) == 2 * (3 + 4 + 3), [r["kernel"] for r in se]
    assert sum(r["kernel"] == "squeeze_excite_pool" for r in se) == 10
    assert all(r["shape"].startswith("multi x") for r in se if r["kernel"] == "squeeze_excite_pool")
    assert sum(r["shape"].startswith("multi x4") for r in se if r["kernel"] == "squeeze_excite_pool") == 3
    assert len(aspp_means) <= 1                           # the ASPP pooling branch only
    multi4 = [r for r in recs if r["kernel"].startswith("conv") and r["shape"].startswith("multi x4")]
    assert len(multi4) >= 2 * 3                            # class + box tower convs of every depth, four levels each


@pytest.mark.parametrize("math,bt", [("f32", "mobilenet"), ("f16s", "resnext50")])
def test_separable_and_se_heads_at_capacity(math, bt):
    """The SqueezeExcite + separable heads of test_full_forward_with_squeeze_excite_and_separable_conv as ONE whole-forward
    graph (the mask head's separable blocks at capacity), against the oracle at the mode's bars."""
    from masklab_hip import ModelConfiguration, ops, retinamasklab as R
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = bt
    cfg.detection.use_separable_conv = True
    cfg.detection.use_squeeze_excite = True
    cfg.instance.use_separable_conv = True
    cfg.instance.use_squeeze_excite = True
    cfg.semantic.use_squeeze_excite = True
    cfg.detection.min_confidence = 0.02
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(4)
    model.load_weights(w, "cuda:0")
    images = np.random.default_rng(77).integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)
    assert model.instance_networks[3].capacity_supported(tuple(cfg.instance.crop_size))
    ops.set_conv_math(math)
    try:
        if math == "f16s":             # scores past 0.5 (order-stable logit scale), threshold in a wide score gap
            from oracle import fixtures as FX
            c1, l1 = O.inference_forward(cfg, w, images, literal_groups=False, with_instance=False, with_semantic=False)
            scale, _ = FX.choose_logit_scale(cfg, c1, l1, 128, 128)
            assert scale is not None, "no order-stable logit scale on the grid"
            w = FX.scale_cls_logits(w, scale)
            model.load_weights(w, "cuda:0")
            ref_cls, ref_loc = O.inference_forward(cfg, w, images, literal_groups=False, with_instance=False,
                                                   with_semantic=False)
            thr = _half_threshold(cfg, model, images, ref_cls, ref_loc)
            cfg.detection.min_confidence = thr
            model.detection_proposal.min_confidence = thr
        want = O.inference_forward(cfg, w, images)
        check = _check_half if math == "f16s" else _check
        model.device_counts = True
        eager = model.predict(images)
        check(model, eager, want)
        model.enable_graphs(True)
        for _ in range(2):
            g = model.predict(images)
            for name, a, b in zip(model.output_names, g, eager):
                np.testing.assert_array_equal(a, b, err_msg=name)
        assert next(iter(model._graphs))[3] is True
    finally:
        model.enable_graphs(False)
        model.device_counts = "auto"
        ops.set_conv_math("f32")
