"""The entropy half of the JPEG request decoder on the device (the jpeg_entropy_* kernels of csrc/jpeg_decode.hip): the
packed form equals the host decoder's byte for byte and the pixels the committed ones -- every fixture, scans across
workgroups, the slowly synchronising flat frame, FF 00 astride a subsequence boundary, malformed streams (the host
decoder's error through the fall-back), batches, and the layer and the serving model.  -m gpu."""
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import jpeg_decode_ref as D
import jpeg_entropy_streams as S
from masklab_hip import _lib

DEVICE = "cuda:0"
OK, NOT_SYNCED = _lib.JPEG_ENTROPY_OK, _lib.JPEG_ENTROPY_NOT_SYNCED


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def cases(golden_dir):
    return D.load_cases(golden_dir)


@pytest.fixture(scope="module")
def lib():
    from masklab_hip import _lib
    return _lib.load()


@pytest.fixture()
def no_pillow(monkeypatch):
    for name in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "PIL", None)


def device_packed(streams):
    """-> ([packed bytes of stream b as far as its header says, or None under a non-zero status], status [B,4])."""
    from masklab_hip import ops
    packed, offsets, status = ops.jpeg_entropy_device(streams, DEVICE)
    assert status.shape == (len(streams), 4) and status.dtype == np.int32
    host = packed.cpu().numpy()
    out = []
    for b in range(len(streams)):
        if status[b, 0] != OK:
            out.append(None)
            continue
        n = int(host[offsets[b] + 24:offsets[b] + 28].view(np.uint32)[0])
        assert 224 < n <= offsets[b + 1] - offsets[b]
        out.append(host[offsets[b]:offsets[b] + n].tobytes())
    return out, status


def assert_equals_host(lib, stream, what):
    want, message = S.host_packed(lib, stream)
    assert want is not None, (what, message)
    got, status = device_packed([stream])
    print(f"{what}: status {status[0].tolist()}")
    assert status[0, 0] == OK, (what, status[0].tolist())
    assert got[0] == want, f"{what}: packed bytes differ from the host decoder's"
    return status[0]


def pixels(stream, entropy):
    from masklab_hip import ops
    out = ops.decode_jpeg(stream, DEVICE, entropy=entropy)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_every_supported_fixture_equals_the_host_decoder_and_the_committed_pixels(lib, cases):
    names = [k for k in sorted(cases) if cases[k]["supported"]]
    assert len(names) == 19
    for name in names:
        assert_equals_host(lib, cases[name]["stream"], name)
        np.testing.assert_array_equal(pixels(cases[name]["stream"], "device")[0], cases[name]["pixels"], err_msg=name)


def test_scans_across_workgroups_with_and_without_restart_intervals(lib):
    from masklab_hip import ops
    bits, per_wg = ops.jpeg_entropy_geometry()
    plain, dri, subsequences = S.noise_across_workgroups(bits, per_wg)
    assert subsequences > 3 * per_wg and subsequences % per_wg != 0
    status = assert_equals_host(lib, plain, "noise across workgroups")
    assert status[3] >= 1, "no state crossed a workgroup boundary"
    assert_equals_host(lib, dri, "noise across workgroups, restart intervals")
    want = pixels(plain, "host")
    np.testing.assert_array_equal(pixels(plain, "device"), want)
    np.testing.assert_array_equal(pixels(dri, "device"), want)


def test_the_flat_frame_is_right_or_not_synced(lib):
    stream = S.flat_with_one_block()
    want, message = S.host_packed(lib, stream)
    assert want is not None, message
    got, status = device_packed([stream])
    print("flat frame: status", status[0].tolist())
    assert status[0, 0] in (OK, NOT_SYNCED)
    if status[0, 0] == OK:
        assert got[0] == want
    np.testing.assert_array_equal(pixels(stream, "device"), pixels(stream, "host"))


def test_stuffing_astride_a_subsequence_boundary(lib):
    from masklab_hip import ops
    bits, _ = ops.jpeg_entropy_geometry()
    stream, k = S.stuffing_astride(bits)
    assert S.straddles(stream, k, bits)
    assert_equals_host(lib, stream, f"FF 00 across the boundary of subsequences {k - 1} and {k}")


def test_malformed_streams_raise_the_host_decoders_error(lib, cases):
    from masklab_hip import ops
    items = S.malformed_set(lib, cases)
    assert 14 <= len(items) <= 30 and {label.split(":")[0] for label, _, _ in items} == set(S.MALFORMED_CLASSES)
    for label, stream, message in items:                               # every one of them: none is skipped
        if S.reference_packed(lib, stream)[0] is not None:             # (a stream without a plan never reaches the kernels)
            assert device_packed([stream])[0][0] is None, (label, "status 0 for a stream the host decoder refuses")
        with pytest.raises(ops.JpegDecodeError) as e:
            ops.decode_jpeg(stream, DEVICE, entropy="device")
        reason = message.split(": ", 1)[1]
        assert reason in str(e.value), (label, str(e.value), message)
    good = cases["photo_150x203_q95"]
    np.testing.assert_array_equal(pixels(good["stream"], "device")[0], good["pixels"], err_msg="after the failed calls")


def test_a_batch_of_32_equals_each_stream_alone_and_a_bad_stream_leaves_its_neighbours(lib, cases):
    names = [k for k in sorted(cases) if cases[k]["supported"]]
    streams = [cases[names[b % len(names)]]["stream"] for b in range(32)]
    streams[5] = streams[5][:len(streams[5]) // 2]                     # ends inside a block
    streams[20] = S.patch_table_value(cases["photo_150x203_q95"]["stream"], 0, 5, 12)
    first, status = device_packed(streams)
    assert status[5, 0] != OK and status[20, 0] != OK and (np.delete(status[:, 0], [5, 20]) == OK).all(), status[:, 0]
    for b, s in enumerate(streams):
        if b not in (5, 20):
            assert first[b] == S.host_packed(lib, s)[0], f"stream {b} of the batch"
    again, status2 = device_packed(streams)                            # the workspace is reused
    assert again == first and np.array_equal(status2[:, :2], status[:, :2])
    big, _ = device_packed([streams[13]])                              # a smaller call, then the batch again
    assert big[0] == first[13]
    assert device_packed(streams)[0] == first


def test_decode_jpeg_batches_and_repeats(cases):
    from masklab_hip import ops
    name = "photo_150x203_q95"
    others = ["photo_150x203_optimize", "photo_150x203_restart_rows1", "photo_150x203_restart_blocks5"]
    streams = [cases[k]["stream"] for k in [name] + others]
    out = pixels(streams, "device")
    for b, k in enumerate([name] + others):
        np.testing.assert_array_equal(out[b], cases[k]["pixels"], err_msg=k)
    outs = [ops.decode_jpeg(streams[k % 4], DEVICE, entropy="device") for k in range(8)]   # calls in flight share the staging
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        np.testing.assert_array_equal(o.cpu().numpy()[0], out[k % 4], err_msg=f"call {k} of 8 in flight")


def test_layer_decodes_with_device_entropy_without_pillow(cases, no_pillow):
    from masklab_hip.layers import DecodeImageContent
    c = cases["photo_150x203_q95"]
    frame = DecodeImageContent(device=DEVICE, entropy="device")(c["stream"])
    assert frame.is_cuda and frame.dtype == torch.uint8 and tuple(frame.shape) == (1, 150, 203, 3)
    np.testing.assert_array_equal(frame[0].cpu().numpy(), c["pixels"])
    assert "PIL.Image" not in sys.modules


def test_serving_model_gives_the_same_answer_with_either_entropy_decoder(cases, tmp_path, no_pillow):
    from masklab_hip import ModelConfiguration, ops, retinamasklab as R, serving
    ops.set_conv_math("f32")
    cfg = ModelConfiguration()
    cfg.backbone.backbone_type = "mobilenet"
    cfg.postprocess.resolution = (128, 256)
    _, model = R.construct_masklab_networks(cfg)
    w = model.init_weights(3)
    for k in w:
        if k.startswith("classification_sub_net/") and k.endswith("/output/kernel"):
            w[k] = (w[k] * 8.0).astype(np.float32)                    # some anchors pass min_confidence
    path = str(tmp_path / "weights.npz")
    np.savez(path, **w)
    c = cases["photo_160x240_q95_libjpeg"]
    answers = {}
    for entropy in ("host", "device"):
        served = serving.load_serving_model_from_h5(path, cfg, device=DEVICE)
        assert served.entropy is None
        served.entropy = entropy                                       # (the loader keeps the reference's signature)
        assert served.decode.entropy == entropy
        answers[entropy] = served.predict(c["stream"])
    assert answers["device"][0][0] == answers["host"][0][0]
    np.testing.assert_array_equal(answers["device"][1], answers["host"][1])
    assert D.parse(answers["device"][0][0])["height"] == 160
