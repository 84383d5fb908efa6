"""The serving 'visualize' output on the device (road_project/setup/serving.py:30-40): the three Draw* layer kernels
against the NumPy restatement (tests/visualize_ref.py), the fused render against the restatement and the literal
four-layer chain, batch independence, graph capture, and the serving model end to end.  uint8 outputs compare exactly.
-m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import visualize_ref as V
from oracle import masklab as O

ICOL = [[192, 32, 128], [160, 96, 0], [96, 0, 128], [32, 96, 192], [96, 32, 128]]
SCOL = [[64, 0, 128], [128, 96, 0], [128, 192, 0]]
HOT = [[255, 255, 255], [250, 0, 90], [7, 255, 13]]                  # saturating colours


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def scene(B, H, W, n, seed, high_conf=True, Ki=5, Ks=3, mh=14, mw=14, padded_image=None, frac=(0.5, 1.0)):
    """Detections as UpSampleOutput writes them: boxes that overhang or miss the frame, classes up to Ki + 1 (>= Ki is
    never drawn), duplicated rows (same box and class: their pasted values pass 0.5 only together at mask edges), padded
    rows (-2, -2, -2, -2, -1, -100); conf above 50 somewhere (threshold 50) or nowhere (threshold -100)."""
    rng = np.random.default_rng(seed)
    det = np.tile(np.array([-2, -2, -2, -2, -1, -100], np.int32), (B, n, 1))
    ins = (rng.random((B, n, mh, mw)) > 0.45).astype(np.int32)
    for b in range(B):
        k = 0 if b == padded_image else int(rng.integers(int(n * frac[0]), int(n * frac[1]) + 1))
        if k == 0:
            continue
        det[b, :k, 0] = rng.integers(-W // 4, W + W // 4, k)
        det[b, :k, 1] = rng.integers(-H // 4, H + H // 4, k)
        det[b, :k, 2] = rng.integers(0, W // 2 + 2, k)
        det[b, :k, 3] = rng.integers(0, H // 2 + 2, k)
        det[b, :k, 4] = rng.integers(0, Ki + 2, k)
        det[b, :k, 5] = rng.integers(30, 100, k) if high_conf else rng.integers(-60, 50, k)
        for i in range(1, k, 5):                                       # same-class duplicates of the previous row
            det[b, i, :5] = det[b, i - 1, :5]
    seg = (rng.random((B, H, W, Ks)) > 0.6).astype(np.int32)          # multi-hot pixels
    images = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    return images, det, ins, seg


SCENES = {                                                              # (scene kwargs, instance colours, alpha, semantic colours, alpha)
    "w_not_mult4": (dict(B=1, H=37, W=53, n=12, seed=1), ICOL, 0.3, SCOL, 0.3),
    "low_conf_b2": (dict(B=2, H=64, W=260, n=40, seed=2, high_conf=False), ICOL, 0.3, HOT, 0.9),
    "n300_b3": (dict(B=3, H=45, W=132, n=300, seed=3), HOT, 0.8, SCOL, 0.45),
    "padded_image": (dict(B=2, H=20, W=36, n=9, seed=4, padded_image=1), ICOL, 0.3, SCOL, 0.3),
    "sixteen": (dict(B=1, H=33, W=128, n=30, seed=5, Ki=16, Ks=16), [[(13 * k + 40 * c) % 256 for c in range(3)]
                                                                      for k in range(16)], 0.25,
                [[(29 * k + 7 * c) % 256 for c in range(3)] for k in range(16)], 0.2),
}


def _literal(images, det, ins, seg, ic, ia, sc, sa):
    from masklab_hip import ops
    di, dd = dev(images), dev(det)
    cpm = ops.crop_pad_mask(dd, dev(ins), images.shape[1], images.shape[2])
    v1 = ops.draw_boxes(di, dd)
    v2 = ops.draw_instance(v1, dd, cpm, ic, ia)
    return ops.draw_segmentation(v2, dev(seg), sc, sa), cpm


@pytest.mark.parametrize("name", sorted(SCENES))
def test_layers_and_fused_render_match_the_restatement(name):
    from masklab_hip import ops
    kw, ic, ia, sc, sa = SCENES[name]
    images, det, ins, seg = scene(**kw)
    cpm = O.crop_and_pad_mask(images.shape[1:3], det, ins)
    v1 = V.draw_boxes(images, det)
    v2 = V.draw_instance(v1, det, cpm, ic, ia)
    v3 = V.draw_segmentation(v2, seg, sc, sa)
    assert (v1 != images).any() and (v2 != v1).any() and (v3 != v2).any(), "degenerate scene"
    np.testing.assert_array_equal(host(ops.draw_boxes(dev(images), dev(det))), v1)
    np.testing.assert_array_equal(host(ops.draw_instance(dev(v1), dev(det), dev(cpm), ic, ia)), v2)
    np.testing.assert_array_equal(host(ops.draw_segmentation(dev(v2), dev(seg), sc, sa)), v3)
    np.testing.assert_array_equal(host(ops.draw_segmentation(dev(v2), dev(seg.astype(np.float32)), sc, sa)), v3)
    lit, gcpm = _literal(images, det, ins, seg, ic, ia, sc, sa)
    np.testing.assert_array_equal(host(gcpm), cpm)
    np.testing.assert_array_equal(host(lit), v3)
    fused = ops.serving_visualize(dev(images), dev(det), dev(ins), dev(seg), ic, ia, sc, sa)
    np.testing.assert_array_equal(host(fused), v3)
    frame = dev(images)                                                 # in place: the output is the frame buffer
    ops.serving_visualize(frame, dev(det), dev(ins), dev(seg), ic, ia, sc, sa, out=frame)
    np.testing.assert_array_equal(host(frame), v3)
    frame = dev(images)
    ops.draw_boxes(frame, dev(det), out=frame)
    np.testing.assert_array_equal(host(frame), v1)


def test_fused_render_equals_the_literal_chain_at_full_hd():
    from masklab_hip import ops
    images, det, ins, seg = scene(B=2, H=1080, W=1920, n=100, seed=11, frac=(1.0, 1.0), mh=28, mw=28)
    det[..., 2] //= 3                                                  # boxes up to a sixth of the frame
    det[..., 3] //= 3
    lit, cpm = _literal(images, det, ins, seg, ICOL, 0.3, SCOL, 0.3)
    del cpm
    fused = ops.serving_visualize(dev(images), dev(det), dev(ins), dev(seg), ICOL, 0.3, SCOL, 0.3)
    got, want = host(fused), host(lit)
    assert (want != images).mean() > 0.3
    np.testing.assert_array_equal(got, want)


def test_an_image_of_a_batch_renders_as_it_does_alone():
    """Same threshold in the batch and alone (the threshold is batch-wide in the reference): every image has a row
    above conf 50."""
    from masklab_hip import ops
    images, det, ins, seg = scene(B=3, H=50, W=96, n=20, seed=21)
    assert (det[..., 5].max(axis=1) > 50).all()
    batch = host(ops.serving_visualize(dev(images), dev(det), dev(ins), dev(seg), ICOL, 0.3, SCOL, 0.3))
    for k in range(3):
        alone = ops.serving_visualize(dev(images[k:k + 1]), dev(det[k:k + 1]), dev(ins[k:k + 1]), dev(seg[k:k + 1]),
                                      ICOL, 0.3, SCOL, 0.3)
        np.testing.assert_array_equal(batch[k], host(alone)[0], err_msg=f"image {k}")


def test_fused_render_replays_in_a_captured_graph():
    from masklab_hip import ops
    first = scene(B=2, H=72, W=200, n=50, seed=31)
    second = scene(B=2, H=72, W=200, n=50, seed=32, high_conf=False)
    bufs = [dev(a) for a in first]
    ops.serving_visualize(*bufs, ICOL, 0.3, SCOL, 0.3)                 # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.serving_visualize(*bufs, ICOL, 0.3, SCOL, 0.3)
    for arrays in (second, first):
        for buf, a in zip(bufs, arrays):
            buf.copy_(torch.from_numpy(a))
        g.replay()
        eager = ops.serving_visualize(*[dev(a) for a in arrays], ICOL, 0.3, SCOL, 0.3)
        np.testing.assert_array_equal(host(out), host(eager))


def _serving_end_to_end(cfg, model, weights, images):
    from masklab_hip import retinamasklab as R
    model.load_weights(weights, "cuda:0")
    deploy = R.construct_deploy_network(cfg, model)
    plain = R.construct_serving_network(cfg, deploy)
    vis = R.construct_serving_network(cfg, deploy, visualize=True)
    seen = {}

    class _Recorder:                                                   # the deploy outputs of the visualize call itself
        def __init__(self, inner):
            self.inner, self.model = inner, inner.model

        def __call__(self, x):
            seen["outs"] = self.inner(x)
            return seen["outs"]

    vis.deploy_model = _Recorder(deploy)
    got_vis, got_sum = vis.predict(images)
    det, ins, seg = (host(t) for t in seen["outs"])
    assert got_vis.dtype == np.uint8 and got_vis.shape == images.shape
    post = cfg.postprocess
    want = V.visualize(images, det, ins, seg, post.instance_colors, post.instance_alpha, post.semantic_colors,
                       post.semantic_alpha)
    np.testing.assert_array_equal(got_vis, want)
    np.testing.assert_array_equal(got_sum, plain.predict(images))
    lit_vis, lit_sum = vis(torch.from_numpy(images), materialise_masks=True)
    np.testing.assert_array_equal(host(lit_vis), got_vis)
    np.testing.assert_array_equal(host(lit_sum), got_sum)
    return det, seg


def test_serving_visualize_end_to_end_on_the_shipped_seresnet34_configuration():
    from test_gpu_seresnet34 import _shipped_config
    from masklab_hip import ops, retinamasklab as R
    ops.set_conv_math("f32")
    cfg = _shipped_config()
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(3)
    for k in w:
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)                    # some anchors pass min_confidence
    images = np.random.default_rng(1080).integers(0, 256, (1, 1080, 1920, 3), dtype=np.uint8)
    det, seg = _serving_end_to_end(cfg, model, w, images)
    assert (det[..., 4] >= 0).sum() > 0 and 0 < seg.mean() < 1, "degenerate fixture"


def test_serving_visualize_end_to_end_on_a_small_mobilenet_configuration():
    from masklab_hip import ModelConfiguration, retinamasklab as R
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = "mobilenet"
    cfg.postprocess.resolution = (128, 256)
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(3)
    for k in w:
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)
    images = np.random.default_rng(1234).integers(0, 256, (2, 256, 512, 3), dtype=np.uint8)
    det, _ = _serving_end_to_end(cfg, model, w, images)
    assert (det[..., 4] >= 0).sum() > 0, "degenerate fixture"
