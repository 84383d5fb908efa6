"""GPU tests of the generator: the resize kernels (csrc/cv_resize.hip) against the NumPy restatement of cv2.resize in
tests/generator_ref.py, the device generator against the device="cpu" one, the trainer network on a generated batch and
validate().  Everything is exact equality; every kernel is launched twice and must give the same bits; outputs start out
as stale bytes (tests/dirty_memory.py).  OpenCV parity is unpinned: the restatement is the contract.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import backbone_cases as MODEL_CASES
import dirty_memory as DM
import generator_cases as CASES
import generator_ref as REF


def _want(x, oh, ow):
    """-> (the uint8 path, np.round of the float64 path) of every plane of x [P,H,W,C]."""
    return (np.stack([REF.resize_u8(p, oh, ow) for p in x]), np.round(np.stack([REF.resize_f64(p, oh, ow) for p in x])))


def _launch_all(x, oh, ow):
    from masklab_hip import ops
    return (ops.cv_resize_linear(x, oh, ow), ops.cv_resize_linear_round(x, oh, ow),
            ops.cv_resize_linear_round(x, oh, ow, dtype=torch.uint8))


def _check(x_host, oh, ow):
    """Both ops on stale (0xFF) and on zeroed outputs, twice each: the same bits every time, equal to the restatement."""
    x = dev(x_host)
    with DM.poisoned():
        dirty, again = DM.snapshot(_launch_all(x, oh, ow)), DM.snapshot(_launch_all(x, oh, ow))
    with DM.zeroed():
        clean = DM.snapshot(_launch_all(x, oh, ow))
    DM.assert_same_bits(again, dirty, "two launches")
    DM.assert_same_bits(dirty, clean, "stale against zeroed outputs")
    want_u8, want_round = _want(x_host, oh, ow)
    got_u8, got_f32, got_round_u8 = dirty
    assert got_u8.dtype == np.uint8 and got_f32.dtype == np.float32 and got_round_u8.dtype == np.uint8
    np.testing.assert_array_equal(got_u8, want_u8)
    np.testing.assert_array_equal(got_f32, want_round.astype(np.float32))
    np.testing.assert_array_equal(got_round_u8, want_round.astype(np.uint8))
    return got_u8


@pytest.mark.parametrize("C", CASES.CHANNELS)
@pytest.mark.parametrize("in_hw,out_hw", CASES.RESIZE_SHAPES)
def test_device_ops_equal_the_restatement(in_hw, out_hw, C):
    x = CASES.random_bytes((3, *in_hw, C), seed=in_hw[0] * 1000 + out_hw[1] * 10 + C)
    got = _check(x, *out_hw)
    if in_hw == out_hw:
        np.testing.assert_array_equal(got, x)


def test_one_full_frame_many_blocks():
    _check(CASES.random_bytes((1, 1080, 1920, 3), seed=1080), 512, 960)


@pytest.mark.parametrize("C,out_hw", [(1, (15, 23)), (3, (15, 23)), (1, (16, 1)), (3, (7, 342))])
def test_rows_that_are_no_multiple_of_four_bytes(C, out_hw):
    """ow * C = 23, 69, 1, 1026: the rows of the three planes start at every offset inside a 4-byte word, the last row is
    longer than one block's 1024 bytes by two."""
    assert (out_hw[1] * C) % 4 != 0
    _check(CASES.random_bytes((3, 37, 53, C), seed=C * 100 + out_hw[1]), *out_hw)


@pytest.mark.parametrize("off", [1, 15])
def test_views_off_a_16_byte_boundary(off):
    from masklab_hip import ops
    shape, (oh, ow) = (2, 37, 53, 3), (16, 24)
    x_host = CASES.random_bytes(shape, seed=off)
    want_u8, want_round = _want(x_host, oh, ow)
    n_in, n_out = int(np.prod(shape)), 2 * oh * ow * 3
    src = torch.zeros(n_in + 32, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0
    x = src[off:off + n_in].view(shape)
    x.copy_(dev(x_host))
    assert x.data_ptr() % 16 == off and x.is_contiguous()
    guard = 0xA5
    for dtype, want in ((torch.uint8, want_u8), (torch.uint8, want_round.astype(np.uint8)), (torch.float32, want_round.astype(np.float32))):
        item = 4 if dtype == torch.float32 else 1
        lead = off if item == 1 else (1 if off == 1 else 3)             # float32: 4 and 12 bytes off the boundary
        buf = DM.fill_bytes(torch.empty(n_out + 32, dtype=dtype, device="cuda"), guard)
        assert buf.data_ptr() % 16 == 0
        out = buf[lead:lead + n_out].view(2, oh, ow, 3)
        for _ in range(2):
            if want is want_u8:
                got = ops.cv_resize_linear(x, oh, ow, out=out)
            else:
                got = ops.cv_resize_linear_round(x, oh, ow, dtype=dtype, out=out)
            assert got.data_ptr() == out.data_ptr() == buf.data_ptr() + lead * item
            np.testing.assert_array_equal(host(got), want)
        whole = host(buf)
        assert DM.holds(whole[:lead], guard) and DM.holds(whole[lead + n_out:], guard), "wrote outside the view"


def test_skipped_planes_between_live_ones():
    from masklab_hip import ops
    masks = CASES.TinyDataset(4, 45, 80).instance
    first = masks[:, :, 0, 0] == -1
    assert first.any() and not first.all() and not first[0, 0] and first[0, 3] and not first[3, 3]
    want = np.full((4, 4, 32, 32), -1, np.int8)
    for i, j in zip(*np.nonzero(~first)):
        want[i, j] = REF.resize_u8(masks[i, j].view(np.uint8)[..., None], 32, 32)[..., 0].view(np.int8)
    x = dev(masks)
    with DM.zeroed():
        clean = DM.snapshot([ops.cv_resize_linear(x, 32, 32, skip_minus_one=True) for _ in range(2)])
    with DM.poisoned():
        dirty = DM.snapshot([ops.cv_resize_linear(x, 32, 32, skip_minus_one=True) for _ in range(2)])
    DM.assert_same_bits(dirty, clean, "skip_minus_one")
    np.testing.assert_array_equal(clean[0], want)
    np.testing.assert_array_equal(clean[1], want)
    # a skipped plane is not read: everything but its first byte may be anything
    scribbled = masks.copy()
    scribbled[0, 3].reshape(-1)[1:] = 77
    np.testing.assert_array_equal(host(ops.cv_resize_linear(dev(scribbled), 32, 32, skip_minus_one=True)), want)
    empty = ops.cv_resize_linear(dev(masks[:, :0]), 32, 32, skip_minus_one=True)
    assert tuple(empty.shape) == (4, 0, 32, 32) and empty.dtype == torch.int8


def test_more_planes_than_one_launch_takes():
    """70 007 planes of 1 x 1 -> 1 x 2: the library cuts them into launches of at most 65 535 planes; the later launch starts
    at its own source and destination offsets (1 and 2 bytes per plane)."""
    from masklab_hip import ops
    masks = np.random.default_rng(7).integers(-128, 128, (7, 10001, 1, 1), dtype=np.int8)
    masks[0, :3, 0, 0] = -1
    masks[6, -3:, 0, 0] = (-1, 5, -1)
    want = np.repeat(masks, 2, axis=3)                                # one source pixel: every tap is that pixel
    x = dev(masks)
    with DM.poisoned():
        got = DM.snapshot([ops.cv_resize_linear(x, 1, 2, skip_minus_one=True) for _ in range(2)])
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want)
    sem = dev(masks.view(np.uint8).reshape(70007, 1, 1, 1))
    np.testing.assert_array_equal(host(ops.cv_resize_linear_round(sem, 1, 2)), want.view(np.uint8).reshape(70007, 1, 2, 1).astype(np.float32))


def test_ops_refuse_what_they_cannot_do():
    from masklab_hip import ops
    x = dev(CASES.random_bytes((1, 4, 4, 3), seed=1))
    with pytest.raises(RuntimeError, match="bad dims"):
        ops.cv_resize_linear(x, 0, 4)
    with pytest.raises(RuntimeError):
        ops.cv_resize_linear(x.float(), 4, 4)
    with pytest.raises(RuntimeError):
        ops.cv_resize_linear_round(x, 4, 4, dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.cv_resize_linear(x, 4, 4, out=torch.empty((1, 4, 4, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.cv_resize_linear(x.cpu(), 4, 4)


# ----------------------------------------------------------------------------- the generator
def _host_batch(X):
    return {k: (host(v) if isinstance(v, torch.Tensor) else v) for k, v in X.items()}


@pytest.mark.parametrize("hw,scale", [((45, 80), 0.75), ((64, 128), 0.5)])
def test_device_generator_equals_the_cpu_generator(hw, scale):
    from masklab_hip.utils import MaskLabGenerator
    on_dev = MaskLabGenerator(CASES.TinyDataset(5, *hw), scale, 2, False, device="cuda")
    on_cpu = MaskLabGenerator(CASES.TinyDataset(5, *hw), scale, 2, False, device="cpu")
    assert len(on_dev) == 2
    for i in range(2):
        (got,), (want,) = on_dev[i], on_cpu[i]
        assert all(got[k].is_cuda for k in ("images", "gt_seg", "gt_masks")) and isinstance(got["gt_boxes"], np.ndarray)
        DM.assert_same_bits(_host_batch(got), _host_batch(want), f"batch {i}")
        (ref,) = REF.getitem(CASES.TinyDataset(5, *hw), i, 2, scale)
        ref["gt_seg"] = ref["gt_seg"].astype(np.float32)
        DM.assert_same_bits(_host_batch(got), ref, f"batch {i} against the restated __getitem__")

    class OnDevice(CASES.TinyDataset):                                  # frames that are already on the device
        def __getitem__(self, sl):
            return {k: dev(v) for k, v in super().__getitem__(sl).items()}
    (got,) = MaskLabGenerator(OnDevice(5, *hw), scale, 2, False, device="cuda", seg_dtype=torch.uint8)[1]
    (want,) = MaskLabGenerator(CASES.TinyDataset(5, *hw), scale, 2, False, device="cpu", seg_dtype=torch.uint8)[1]
    DM.assert_same_bits(_host_batch(got), _host_batch(want), "device-resident dataset")


@pytest.fixture(scope="module")
def trainer():
    """The trainer network of tests/test_gpu_trainer.py (ResNeXt-50 under the shipped head configuration, the smallest
    shape whose five levels reach 1 x 1: 64 x 96) with synthetic weights."""
    from masklab_hip import retinamasklab as R
    cfg = MODEL_CASES.shipped_se_config("resnext50", ('C3', 'C4', 'C5', 'P6', 'P7'))
    model, _ = R.construct_masklab_networks(cfg, with_trainer=True)
    model.load_weights(model.init_weights(seed=2), "cuda:0")
    return model


def _dataset():
    return CASES.TinyDataset(4, 90, 130, seed=9)                        # at 0.75: 67 x 97 -> 64 x 96


def test_trainer_takes_the_generated_batch_unchanged(trainer):
    from masklab_hip.utils import MaskLabGenerator
    (X,) = MaskLabGenerator(_dataset(), 0.75, 2, False, device="cuda")[0]
    assert tuple(X["images"].shape) == (2, 64, 96, 3)
    (ref,) = REF.getitem(_dataset(), 0, 2, 0.75)
    ref["gt_seg"] = ref["gt_seg"].astype(np.float32)                  # float64 integers 0..255: the trainer takes float32 / uint8
    state = trainer.box_loss.state.clone()                              # BoxLoss moves its statistics on every call
    got = trainer.predict(X)
    trainer.box_loss.state.copy_(state)
    want = trainer.predict(ref)
    trainer.box_loss.state.copy_(state)
    assert list(got) == trainer.output_names and len(got) == 10
    for name in got:
        print(f"{name}: {got[name]}")
    DM.assert_same_bits(got, want, "trainer outputs")                  # the same input bytes: the same bits


def test_validate_over_two_batches_equals_the_means_by_hand(trainer):
    from masklab_hip.evaluate import validate
    from masklab_hip.utils import MaskLabGenerator
    gen = MaskLabGenerator(_dataset(), 0.75, 2, False, device="cuda")
    assert len(gen) == 2
    state = trainer.box_loss.state.clone()
    got = validate(trainer, gen)
    trainer.box_loss.state.copy_(state)
    batches = [trainer.predict(gen[i][0]) for i in range(2)]
    trainer.box_loss.state.copy_(state)
    want = {}
    for name in trainer.output_names:
        per_sample = np.concatenate([b[name] for b in batches]).astype(np.float64)
        assert per_sample.shape == (4,)
        want["val_" + name] = (per_sample[0] + per_sample[1] + (per_sample[2] + per_sample[3])) / 4   # batch sums, then their sum
    want["val_loss"] = sum(v for k, v in want.items() if "loss" in k)
    assert list(got) == list(want) and len(got) == 11
    for k in want:
        print(f"{k}: {got[k]!r}")
        assert got[k] == want[k], (k, got[k], want[k])
    losses = [got["val_" + n] for n in ("class_loss", "box_loss", "mask_loss", "seg_loss")]
    assert all(np.isfinite(v) and v != 0 for v in losses) and got["val_loss"] == sum(losses)      # full-range truth: seg_loss < 0
