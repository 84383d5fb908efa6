"""The JPEG request decoder on the device (csrc/jpeg_decode.hip): every supported fixture stream decodes to exactly the
pixels Pillow (libjpeg-turbo) decoded from it, the device encoder's own streams decode to what the NumPy reference of
tests/jpeg_decode_ref.py gives, batches, determinism, and the layer and the serving model with Pillow hidden.  -m gpu."""
import io
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import jpeg_decode_ref as D

DEVICE = "cuda:0"
IMPORT_ERROR = "install Pillow"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def cases(golden_dir):
    return D.load_cases(golden_dir)


@pytest.fixture()
def no_pillow(monkeypatch):
    """`import PIL` and `from PIL import Image` raise ImportError."""
    for name in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "PIL", None)


def decode(contents):
    from masklab_hip import ops
    out = ops.decode_jpeg(contents, DEVICE)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
    return out.cpu().numpy()


def assert_same_pixels(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        print(f"{what}: {len(bad)} bytes differ, first at (y, x, channel) = {tuple(bad[0])}")
    np.testing.assert_array_equal(got, want, err_msg=what)


def test_every_supported_fixture_decodes_to_the_committed_pixels(cases):
    seen = set()
    for name, c in sorted(cases.items()):
        if c["supported"]:
            got = decode(c["stream"])
            assert got.shape[0] == 1
            assert_same_pixels(got[0], c["pixels"], name)
            seen.add(c["mode"])
    assert seen == {"420", "444", "gray"}


def test_unsupported_streams_are_told_apart_from_malformed_ones(cases):
    from masklab_hip import ops
    for name in ("photo_150x203_progressive", "photo_150x203_422"):
        with pytest.raises(ops.UnsupportedJpeg, match="unsupported"):
            ops.decode_jpeg(cases[name]["stream"], DEVICE)
    with pytest.raises(ops.UnsupportedJpeg, match="not a JPEG"):
        ops.decode_jpeg(b"\x89PNG\r\n\x1a\n" + bytes(32), DEVICE)
    good = cases["photo_150x203_q95"]["stream"]
    with pytest.raises(ops.JpegDecodeError, match="scan ends inside block"):
        ops.decode_jpeg(good[:len(good) // 2], DEVICE)
    assert_same_pixels(decode(good)[0], cases["photo_150x203_q95"]["pixels"], "after the failed calls")


@pytest.mark.parametrize("name", ["noise_37x53", "photo_150x203"])
def test_the_device_encoders_stream_decodes_to_the_reference(golden_dir, name):
    """Encoder and decoder back to back: padded blocks that encode replicated samples, Annex K tables."""
    import os
    from masklab_hip import ops
    with np.load(os.path.join(golden_dir, "jpeg", "frames.npz")) as z:
        frame = z[name]
    buffer, lengths = ops.encode_jpeg(torch.from_numpy(frame[None]).to(DEVICE), 95)
    stream = ops.jpeg_contents(buffer, lengths)[0]
    want = D.decode(stream)
    assert want.shape == frame.shape
    assert_same_pixels(decode(stream)[0], want, name)
    if name.startswith("photo"):                                       # a photograph at quality 95 comes back close
        assert np.abs(want.astype(np.int64) - frame).mean() < 3.0


def test_a_batch_equals_each_stream_alone_and_runs_repeat(cases):
    from masklab_hip import ops
    names = ["photo_150x203_q95", "photo_150x203_restart_rows1", "photo_150x203_optimize"]
    frame = cases[names[0]]["pixels"]
    # three different contents of one size: the photo, the photo upside down and noise, through the device encoder
    frames = np.stack([frame, frame[::-1], np.random.default_rng(3).integers(0, 256, frame.shape, dtype=np.uint8)])
    streams = ops.jpeg_contents(*ops.encode_jpeg(torch.from_numpy(np.ascontiguousarray(frames)).to(DEVICE), 95))
    streams.append(cases[names[1]]["stream"])
    assert len({len(s) for s in streams}) == 4
    first = decode(streams)
    assert first.shape == (4, 150, 203, 3)
    for b, s in enumerate(streams):
        assert_same_pixels(first[b], decode(s)[0], f"image {b} of the batch against itself alone")
    assert_same_pixels(first[3], cases[names[1]]["pixels"], names[1])
    import dirty_memory as DM
    with DM.poisoned():                                                # a dirty workspace and dirty outputs change nothing
        assert_same_pixels(decode(streams), first, "second run")
    # several calls in flight share the two staging buffers: no upload is overwritten before it was read
    outs = [ops.decode_jpeg(streams[k % 4], DEVICE) for k in range(8)]
    torch.cuda.synchronize()
    for k, out in enumerate(outs):
        assert_same_pixels(out.cpu().numpy()[0], first[k % 4], f"call {k} of 8 in flight")


def test_mixed_sizes_and_modes_raise_and_a_batch_of_32_runs(cases):
    from masklab_hip import ops
    for name in ("photo_150x203_444", "photo_150x203_gray"):          # batches of the other two modes
        got = decode([cases[name]["stream"]] * 2)
        for b in range(2):
            assert_same_pixels(got[b], cases[name]["pixels"], name)
    with pytest.raises(ValueError, match="one sampling mode"):
        ops.decode_jpeg([cases["photo_150x203_444"]["stream"], cases["photo_150x203_q95"]["stream"]], DEVICE)
    with pytest.raises(ValueError, match="one size"):
        ops.decode_jpeg([cases["photo_150x203_q95"]["stream"], cases["noise_37x53_q95"]["stream"]], DEVICE)
    with pytest.raises(ValueError, match="1 .. 32 streams"):
        ops.decode_jpeg([cases["crop_1x1_q95"]["stream"]] * 33, DEVICE)
    many = decode([cases["crop_8x9_q95"]["stream"]] * 32)
    assert (many == cases["crop_8x9_q95"]["pixels"][None]).all()


def test_layer_decodes_on_the_device_without_pillow(cases, no_pillow):
    from masklab_hip.layers import DecodeImageContent
    c = cases["photo_150x203_q95"]
    layer = DecodeImageContent(device=DEVICE)
    obj = np.empty((1,), dtype=object)
    obj[0] = c["stream"]
    for given in (c["stream"], [c["stream"]], obj):
        frame = layer(given)
        assert frame.is_cuda and frame.dtype == torch.uint8 and tuple(frame.shape) == (1, 150, 203, 3)
        assert_same_pixels(frame[0].cpu().numpy(), c["pixels"], "layer")
    assert "PIL.Image" not in sys.modules
    with pytest.raises(ImportError, match=IMPORT_ERROR):                 # on_device=False is the host path
        DecodeImageContent(device=DEVICE, on_device=False)(c["stream"])


@pytest.mark.parametrize("name", ["photo_150x203_progressive", "photo_150x203_422"])
def test_layer_falls_back_to_pillow_for_what_the_device_does_not_take(cases, name, monkeypatch):
    Image = pytest.importorskip("PIL.Image")
    from masklab_hip.layers import DecodeImageContent
    stream = cases[name]["stream"]
    with Image.open(io.BytesIO(stream)) as im:
        want = np.asarray(im.convert("RGB"))
    layer = DecodeImageContent(device=DEVICE)
    frame = layer(stream)
    assert frame.is_cuda and tuple(frame.shape) == (1, 150, 203, 3)
    assert_same_pixels(frame[0].cpu().numpy(), want, name)
    with monkeypatch.context() as m:
        m.setitem(sys.modules, "PIL", None)
        with pytest.raises(ImportError, match=IMPORT_ERROR):
            layer(stream)


def test_layer_gives_a_malformed_baseline_stream_to_pillow(cases, monkeypatch):
    """libjpeg resynchronises after a wrong RSTn with a warning, the strict device-path parser does not: the layer asks
    Pillow, as it did before, and returns what Pillow makes of the stream; without Pillow the parser's reason is raised."""
    from masklab_hip import ops
    from masklab_hip.layers import DecodeImageContent
    good = cases["photo_150x203_restart_blocks5"]["stream"]
    at = good.index(b"\xff\xd1")
    stream = good[:at] + b"\xff\xd2" + good[at + 2:]
    layer = DecodeImageContent(device=DEVICE)
    with pytest.raises(ops.JpegDecodeError, match="RST1 expected"):
        ops.decode_jpeg(stream, DEVICE)
    with monkeypatch.context() as m:
        m.setitem(sys.modules, "PIL", None)
        with pytest.raises(ops.JpegDecodeError, match="RST1 expected"):
            layer(stream)
    Image = pytest.importorskip("PIL.Image")
    with Image.open(io.BytesIO(stream)) as im:
        want = np.asarray(im.convert("RGB"))
    frame = layer(stream)
    assert frame.is_cuda and tuple(frame.shape) == (1, 150, 203, 3)
    assert_same_pixels(frame[0].cpu().numpy(), want, "wrong RSTn, through Pillow")


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


def test_serving_model_serves_a_request_without_pillow(cases, tmp_path, no_pillow):
    """Content in, content out, no Pillow anywhere: the bytes equal those of ServingModel.predict fed the committed
    pixels of the request."""
    from masklab_hip import ops, retinamasklab as R, serving
    ops.set_conv_math("f32")
    cfg, model, w = _mobilenet_serving()
    path = str(tmp_path / "weights.npz")
    np.savez(path, **w)
    served = serving.load_serving_model_from_h5(path, cfg, device=DEVICE)
    c = cases["photo_160x240_q95_libjpeg"]
    contents, summary = served.predict(c["stream"])
    assert isinstance(contents, np.ndarray) and contents.dtype == object and contents.shape == (1,)
    assert "PIL.Image" not in sys.modules
    assert isinstance(served.serving, R.ServingModel)
    want_contents, want_summary = served.serving.predict(c["pixels"][None].copy())
    assert contents[0] == want_contents[0]
    np.testing.assert_array_equal(summary, want_summary)
    assert D.parse(contents[0])["height"] == 160
