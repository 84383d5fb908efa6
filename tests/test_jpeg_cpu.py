"""The JPEG content output without a device: the NumPy reference (tests/jpeg_ref.py) against libjpeg's committed streams
and against itself, the C entry points' argument checks, the codec layers and the serving model's signature."""
import inspect
import io
import json
import os
import sys

import numpy as np
import pytest

import jpeg_ref as J


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with np.load(os.path.join(golden_dir, "jpeg", "frames.npz")) as z:
        arrays = {k: z[k] for k in z.files}
    with open(os.path.join(golden_dir, "jpeg", "manifest.json")) as fh:
        return arrays, json.load(fh)


def test_the_built_library_is_abi_7():
    from masklab_hip import _lib
    assert _lib.load().ml_version() == _lib.ABI_VERSION == 7


def test_entry_point_validates_its_arguments():
    """Every precondition is checked before anything reaches a device: ML_E_BADARG (-1) and the reason."""
    from masklab_hip import _lib
    lib = _lib.load()
    H, W = 32, 48
    cap = lib.ml_jpeg_encode_capacity(H, W)
    ws_bytes = lib.ml_jpeg_encode_workspace_bytes(1, H, W)
    assert cap > 0 and ws_bytes > 0
    img, out, lens, ws = 0x100000, 0x200000, 0x300000, 0x400000

    def call(images=img, B=1, H=H, W=W, quality=95, out=out, capacity=cap, lengths=lens, workspace=ws):
        return lib.ml_jpeg_encode_u8(images, B, H, W, quality, out, capacity, lengths, workspace, None)

    def err():
        return lib.ml_last_error()

    for kw in (dict(images=None), dict(out=None), dict(lengths=None), dict(workspace=None)):
        assert call(**kw) == -1 and b"null pointer" in err(), kw
    for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-8)):
        assert call(**kw) == -1 and b"bad dims" in err(), kw
    for kw in (dict(H=65536), dict(W=70000)):
        assert call(**kw) == -1 and b"65535" in err(), kw
    for q in (0, 101, -5):
        assert call(quality=q) == -1 and b"1 <= quality <= 100" in err(), q
    assert call(capacity=cap - 1) == -1 and b"below ml_jpeg_encode_capacity" in err()
    assert call(out=img + 16) == -1 and b"out overlaps images" in err()
    assert call(out=img - cap + 1) == -1 and b"out overlaps images" in err()
    assert call(workspace=out + 16) == -1 and b"overlaps another buffer" in err()
    assert call(workspace=ws + 4) == -1 and b"16-byte aligned" in err()
    assert lib.ml_jpeg_encode_capacity(0, 8) == -1 and b"bad dims" in err()
    assert lib.ml_jpeg_encode_capacity(8, 65536) == -1 and b"65535" in err()
    assert lib.ml_jpeg_encode_workspace_bytes(0, 8, 8) == -1 and b"bad dims" in err()
    assert lib.ml_jpeg_encode_workspace_bytes(2, H, W) > ws_bytes


def test_capacity_bounds_a_quality_100_noise_frame():
    from masklab_hip import _lib
    lib = _lib.load()
    for H, W in ((48, 64), (37, 53)):
        frame = np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8)
        stream = J.encode(frame, 100)
        assert lib.ml_jpeg_encode_capacity(H, W) >= len(stream)
        assert J.decode(stream, (H, W))["stuffed"] > 0
    # the bound does not depend on the content: every coefficient at the longest code and magnitude, all of it stuffed
    nblk = 6 * 3 * 4
    assert lib.ml_jpeg_encode_capacity(48, 64) >= 623 + 2 * ((nblk * (22 + 63 * 26) + 7) // 8) + 2


def test_decoder_reproduces_the_manifest_on_libjpegs_streams(fixtures):
    """What validates the decoder: on streams another implementation wrote, it finds the tables of the quality rule,
    the Annex K Huffman tables and exactly the recorded distance from the oracle."""
    arrays, manifest = fixtures
    seen = 0
    for name, entry in manifest["frames"].items():
        frame = arrays[name]
        assert frame.shape == (entry["height"], entry["width"], 3) and frame.dtype == np.uint8
        assert entry["multiple_of_16"] == (frame.shape[0] % 16 == 0 and frame.shape[1] % 16 == 0)
        assert bool(entry["libjpeg"]) == entry["multiple_of_16"]
        for q, rec in entry["libjpeg"].items():
            dec = J.decode(bytes(arrays[rec["stream"]]), frame.shape[:2])
            share, largest = J.compare(dec["coefficients"], frame, int(q))
            assert share == rec["share_differing"] and largest == rec["max_difference"], (name, q, share, largest)
            for got, want in zip(dec["qtables"], J.quant_tables(int(q))):
                np.testing.assert_array_equal(got, want)
            for key, (bits, vals) in J.STD_HUFFMAN.items():
                assert (list(dec["huffman"][key][0]), list(dec["huffman"][key][1])) == (bits, vals)
            seen += 1
    assert seen >= 7
    for q, share in manifest["largest_libjpeg_share"].items():
        assert share == max(e["libjpeg"][q]["share_differing"] for e in manifest["frames"].values() if q in e["libjpeg"])


def test_quality_rule_gives_libjpegs_tables_at_95(fixtures):
    _, manifest = fixtures
    rec = manifest["frames"]["noise_64x80"]["libjpeg"]["95"]
    lum, chrom = J.quant_tables(95)
    assert lum.tolist() == rec["luminance_table"] and chrom.tolist() == rec["chrominance_table"]
    assert lum[:8].tolist() == [2, 1, 1, 2, 2, 4, 5, 6]
    assert J.quant_tables(100)[0].max() == 1 and J.quant_tables(1)[1].max() == 255


@pytest.mark.parametrize("name,quality", [("noise_37x53", 95), ("noise_64x80", 100), ("photo_150x203", 50), ("smooth_48x70", 95)])
def test_oracle_encoder_round_trips_through_the_decoder(fixtures, name, quality):
    arrays, _ = fixtures
    frame = arrays[name]
    stream = J.encode(frame, quality)
    dec = J.decode(stream, frame.shape[:2])
    np.testing.assert_array_equal(dec["coefficients"], J.oracle_coefficients(frame, quality))
    assert J.compare(dec["coefficients"], frame, quality) == (0.0, 0)
    assert stream.startswith(J.header(frame.shape[0], frame.shape[1], quality)) and stream.endswith(b"\xff\xd9")


def test_decoder_is_strict(fixtures):
    arrays, _ = fixtures
    frame = arrays["noise_37x53"]
    good = J.encode(frame, 95)
    n = len(J.header(37, 53, 95))
    with pytest.raises(J.JpegError, match="inside the scan"):
        J.decode(good[:n + 40] + b"\xff\xd0" + good[n + 40:])
    with pytest.raises(J.JpegError, match="no EOI"):
        J.decode(good[:-2])
    with pytest.raises(J.JpegError, match="after EOI"):
        J.decode(good + b"\x00")
    with pytest.raises(J.JpegError, match="SOF0 says"):
        J.decode(good, (53, 37))
    with pytest.raises(J.JpegError, match="left after the last MCU"):
        J.decode(good[:-2] + b"\xfe\xff\xd9")                     # a whole byte (and a 0-bit) after the last MCU
    sos = good.index(b"\xff\xda")
    wrong_table = bytearray(good)
    wrong_table[sos + 8] = 0x10                                    # Cb's selectors 0x11 -> 0x10: AC table 0
    with pytest.raises(J.JpegError, match="tables 0/0, 1/1, 1/1"):
        J.decode(bytes(wrong_table))
    dht = good.index(b"\xff\xc4")
    missing = bytearray(good)
    missing[dht + 4] = 0x02                                        # DC table 0 is now called table 2
    with pytest.raises(J.JpegError, match="not defined"):
        J.decode(bytes(missing))


def test_pillow_opens_the_oracle_encoders_stream(fixtures):
    Image = pytest.importorskip("PIL.Image")
    arrays, _ = fixtures
    for name, quality in (("photo_150x203", 95), ("noise_37x53", 100), ("smooth_96x128", 50)):
        frame = arrays[name]
        with Image.open(io.BytesIO(J.encode(frame, quality))) as im:
            assert im.size == (frame.shape[1], frame.shape[0]) and im.mode == "RGB"
            got = np.asarray(im.convert("RGB")).astype(np.int64)
        if name.startswith("photo"):                               # a photograph at quality 95 comes back close
            assert np.abs(got - frame).mean() < 3.0


def test_layers_are_exported_and_registered():
    from masklab_hip import get_custom_objects, layers
    from masklab_hip.layers import DecodeImageContent, EncodeImageContent
    reg = get_custom_objects()
    assert reg["EncodeImageContent"] is EncodeImageContent is layers.misc.EncodeImageContent
    assert reg["DecodeImageContent"] is DecodeImageContent is layers.misc.DecodeImageContent
    assert EncodeImageContent().quality == 95 and EncodeImageContent(quality=80).get_config()["quality"] == 80


def test_serving_signatures_and_the_encode_rule():
    from masklab_hip import ModelConfiguration, ops, retinamasklab as R, serving

    class _Deploy:
        model = None

    cfg = ModelConfiguration()
    for fn in (R.ServingModel.__init__, R.construct_serving_network):
        p = inspect.signature(fn).parameters
        assert p["visualize"].default is False and p["encode"].default is False
    assert list(inspect.signature(R.construct_serving_network).parameters) == ["configuration", "deploy_model", "visualize",
                                                                                "encode"]
    with pytest.raises(ValueError, match="visualize=True"):
        R.ServingModel(cfg, _Deploy(), encode=True)
    with pytest.raises(ValueError, match="visualize=True"):
        R.construct_serving_network(cfg, _Deploy(), encode=True)
    both = R.construct_serving_network(cfg, _Deploy(), visualize=True, encode=True)
    assert both.output_names == ['visualize', 'summarize'] and both.encode and both.encode_content.quality == 95
    plain = R.construct_serving_network(cfg, _Deploy(), visualize=True)
    assert plain.output_names == ['visualize', 'summarize'] and not plain.encode
    p = inspect.signature(serving.load_serving_model_from_h5).parameters
    assert list(p) == ["weight_path", "config", "device"] and p["device"].default == "cuda"
    assert inspect.signature(ops.encode_jpeg).parameters["quality"].default == 95
    with pytest.raises(NotImplementedError, match="DecodeImageContent"):     # unchanged
        R.load_masklab_inference_model_from_h5("weights.h5", cfg, serving=True)


def test_decode_image_content(monkeypatch, fixtures):
    import torch
    from masklab_hip.layers import DecodeImageContent
    arrays, _ = fixtures
    content = bytes(arrays["photo_160x240_q95_libjpeg"])
    layer = DecodeImageContent()
    with pytest.raises(ValueError, match="one image content"):
        layer([content, content])
    with pytest.raises(ValueError, match="bytes of an image file"):
        layer(["not bytes"])
    with monkeypatch.context() as m:
        m.setitem(sys.modules, "PIL", None)                        # `from PIL import Image` -> ImportError
        with pytest.raises(ImportError, match="install Pillow"):
            layer(content)
    pytest.importorskip("PIL.Image")
    obj = np.empty((1,), dtype=object)
    obj[0] = content
    for given in (content, [content], obj):
        frame = layer(given)
        assert isinstance(frame, torch.Tensor) and frame.dtype == torch.uint8 and tuple(frame.shape) == (1, 160, 240, 3)
    assert np.abs(frame[0].numpy().astype(np.int64) - arrays["photo_160x240"]).mean() < 3.0
