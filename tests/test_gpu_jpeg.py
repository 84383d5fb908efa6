"""The serving model's JPEG content on the device (csrc/jpeg.hip): every stream goes through the strict decoder of
tests/jpeg_ref.py and its coefficients are held to the fp64 oracle -- no coefficient off by more than 1 (an fp32 DCT is
far closer to the fp64 one than a quantisation step: only roundings next to a tie can move), and no more of them off
than libjpeg itself has on that frame (tests/golden/jpeg/manifest.json; frames whose dimensions are not multiples of 16
have no libjpeg figure and take the largest one recorded at that quality).  Then stuffing, determinism, batching, graph
capture and the serving model end to end.  -m gpu."""
import io
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import jpeg_ref as J

OTHER_QUALITY_FRAMES = ("noise_64x80", "photo_160x240")              # the two frames with libjpeg streams at 50 and 100


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with np.load(os.path.join(golden_dir, "jpeg", "frames.npz")) as z:
        arrays = {k: z[k] for k in z.files}
    with open(os.path.join(golden_dir, "jpeg", "manifest.json")) as fh:
        return arrays, json.load(fh)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def encode(frames, quality=95):
    """uint8 [B,H,W,3] -> (list of bytes, whole buffer [B,capacity], lengths) through ops.encode_jpeg."""
    from masklab_hip import ops
    buffer, lengths = ops.encode_jpeg(dev(frames), quality)
    torch.cuda.synchronize()
    n = lengths.cpu().numpy()
    buf = buffer.cpu().numpy()
    assert buf.shape == (frames.shape[0], ops.jpeg_capacity(frames.shape[1], frames.shape[2]))
    assert (n > 0).all() and (n <= buf.shape[1]).all()
    return [bytes(buf[b, :n[b]]) for b in range(len(n))], buf, n


def check_coefficients(stream, frame, quality, allowed_share, what):
    dec = J.decode(stream, frame.shape[:2])                           # strict: raises on anything malformed
    for got, want in zip(dec["qtables"], J.quant_tables(quality)):
        np.testing.assert_array_equal(got, want, err_msg=what)
    share, largest = J.compare(dec["coefficients"], frame, quality)
    print(f"{what}: q={quality} bytes={len(stream)} stuffed={dec['stuffed']} share_differing={share:.6f} "
          f"max_difference={largest} allowed_share={allowed_share:.6f}")
    assert largest <= 1, (what, largest)
    assert share <= allowed_share, (what, share, allowed_share)
    return dec


def allowed(manifest, name, quality):
    entry = manifest["frames"][name]
    if entry["multiple_of_16"]:
        return entry["libjpeg"][str(quality)]["share_differing"]
    return manifest["largest_libjpeg_share"][str(quality)]


def test_coefficients_on_every_fixture_frame_at_quality_95(fixtures):
    arrays, manifest = fixtures
    assert len(manifest["frames"]) >= 6
    for name in sorted(manifest["frames"]):
        frame = arrays[name]
        (stream,), _, _ = encode(frame[None], 95)
        assert stream[:len(J.header(*frame.shape[:2], 95))] == J.header(*frame.shape[:2], 95)
        check_coefficients(stream, frame, 95, allowed(manifest, name, 95), name)


@pytest.mark.parametrize("quality", [50, 100])
def test_coefficients_at_other_qualities(fixtures, quality):
    arrays, manifest = fixtures
    for name in OTHER_QUALITY_FRAMES:
        frame = arrays[name]
        (stream,), _, _ = encode(frame[None], quality)
        check_coefficients(stream, frame, quality, allowed(manifest, name, quality), name)


def test_quality_range():
    from masklab_hip import ops
    frame = np.random.default_rng(3).integers(0, 256, (1, 24, 40, 3), dtype=np.uint8)
    for q in (1, 100):
        (stream,), _, _ = encode(frame, q)
        dec = J.decode(stream, (24, 40))
        assert J.compare(dec["coefficients"], frame[0], q)[1] <= 1
    for q in (0, 101, 95.0, True):
        with pytest.raises(ValueError, match="quality"):
            ops.encode_jpeg(dev(frame), q)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.encode_jpeg(dev(frame).float())


def test_stuffing_path_runs(fixtures):
    arrays, _ = fixtures
    frame = arrays["noise_64x80"]
    (stream,), _, _ = encode(frame[None], 100)
    dec = J.decode(stream, frame.shape[:2])
    assert dec["stuffed"] >= 1
    scan = stream[len(J.header(64, 80, 100)):-2]
    assert scan.count(b"\xff\x00") >= dec["stuffed"] and scan.count(b"\xff") == dec["stuffed"]


def test_determinism_batching_and_the_bytes_past_length(fixtures):
    from masklab_hip import ops
    rng = np.random.default_rng(17)
    frames = rng.integers(0, 256, (3, 150, 203, 3), dtype=np.uint8)
    frames[1] = fixtures[0]["photo_150x203"]
    frames[2, 40:] = 200                                               # three very different lengths
    first, buf, n = encode(frames, 95)
    again, _, _ = encode(frames, 95)
    assert first == again
    assert len({len(s) for s in first}) == 3
    for b in range(3):
        (alone,), _, _ = encode(frames[b:b + 1], 95)
        assert alone == first[b], f"image {b}"
        J.decode(first[b], (150, 203))
    # whatever lies past `length` is never needed: the files decode from buffers whose tails were overwritten
    garbled = buf.copy()
    for b in range(3):
        garbled[b, n[b]:] = 0xFF
        assert (J.decode(bytes(garbled[b, :n[b]]), (150, 203))["coefficients"] ==
                J.decode(first[b], (150, 203))["coefficients"]).all()
    # a dirty workspace and a dirty output buffer change nothing (the scratch is shared between calls)
    import dirty_memory as DM
    with DM.poisoned():
        third, _, _ = encode(frames, 95)
    assert third == first


def test_encode_replays_in_a_captured_graph(fixtures):
    from masklab_hip import ops
    arrays, _ = fixtures
    first, second = arrays["photo_160x240"], arrays["photo_160x240"][::-1, ::-1].copy()
    frame = dev(first[None])
    ops.encode_jpeg(frame)                                             # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buffer, lengths = ops.encode_jpeg(frame)
    for arr in (second, first):
        frame.copy_(torch.from_numpy(arr[None]))
        g.replay()
        torch.cuda.synchronize()
        k = int(lengths.cpu()[0])
        replayed = bytes(buffer[0, :k].cpu().numpy())
        (eager,), _, _ = encode(arr[None], 95)
        assert replayed == eager
    assert len(eager) != 0 and J.decode(eager, (160, 240))["height"] == 160


def _mobilenet_serving(seed=3):
    from masklab_hip import ModelConfiguration, retinamasklab as R
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = "mobilenet"
    cfg.postprocess.resolution = (128, 256)
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(seed)
    for k in w:
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)                    # some anchors pass min_confidence
    return cfg, model, w


def test_serving_model_end_to_end():
    """ServingModel(visualize=True, encode=True): the content decodes to the coefficients of the very pixel frame that
    encode=False returns, one `bytes` per image of the batch, and the summary is bit-identical."""
    from masklab_hip import layers, ops, retinamasklab as R
    ops.set_conv_math("f32")
    cfg, model, w = _mobilenet_serving()
    model.load_weights(w, "cuda:0")
    deploy = R.construct_deploy_network(cfg, model)
    pixels = R.construct_serving_network(cfg, deploy, visualize=True)
    content = R.construct_serving_network(cfg, deploy, visualize=True, encode=True)
    images = np.random.default_rng(1234).integers(0, 256, (2, 256, 512, 3), dtype=np.uint8)
    vis, summary = pixels.predict(images)
    got, got_summary = content.predict(images)
    assert (vis != images).any(), "degenerate fixture: nothing was drawn"
    np.testing.assert_array_equal(got_summary, summary)
    assert isinstance(got, list) and len(got) == 2 and all(isinstance(c, bytes) for c in got)
    for b in range(2):
        dec = J.decode(got[b], (256, 512))
        share, largest = J.compare(dec["coefficients"], vis[b], 95)
        print(f"serving image {b}: bytes={len(got[b])} share_differing={share:.6f} max_difference={largest}")
        assert largest <= 1
        (direct,), _, _ = encode(vis[b:b + 1], 95)
        assert got[b] == direct
    lit_content, lit_summary = content(torch.from_numpy(images), materialise_masks=True)
    assert ops.jpeg_contents(*lit_content) == got
    # the layer itself: the first frame of a batch -> object array [1] of bytes
    out = layers.EncodeImageContent()(dev(vis))
    assert isinstance(out, np.ndarray) and out.dtype == object and out.shape == (1,) and out[0] == got[0]


def test_serving_module_from_content_to_content(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from masklab_hip import ops, serving
    ops.set_conv_math("f32")
    cfg, model, w = _mobilenet_serving()
    path = str(tmp_path / "weights.npz")
    np.savez(path, **w)
    served = serving.load_serving_model_from_h5(path, cfg, device="cuda:0")
    assert served.output_names == ['visualize', 'summarize']
    frame = np.random.default_rng(7).integers(0, 256, (250, 500, 3), dtype=np.uint8)
    request = io.BytesIO()
    Image.fromarray(frame).save(request, "JPEG", quality=95)
    contents, summary = served.predict(request.getvalue())
    assert isinstance(contents, np.ndarray) and contents.dtype == object and contents.shape == (1,)
    assert summary.dtype == np.float32 and summary.ndim == 3 and summary.shape[0] == 1 and summary.shape[2] == 11
    with Image.open(io.BytesIO(contents[0])) as im:
        assert im.size == (500, 250) and im.format == "JPEG"
        im.load()
    J.decode(contents[0], (250, 500))
    again, _ = served([request.getvalue()])
    assert again[0] == contents[0]
