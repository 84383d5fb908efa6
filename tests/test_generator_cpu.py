"""CPU tests of the generator (no GPU): the library's host loops over the resize kernels' per-thread code
(ml_cv_resize_reference_host) against the NumPy restatement of cv2.resize in tests/generator_ref.py, the generator on
device="cpu" against the reference's __getitem__ restated, and validate() on a stub trainer.  Everything is exact equality.
OpenCV parity is unpinned: the restatement, not a run of OpenCV, is the contract."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import generator_cases as CASES
import generator_ref as REF


def _want(x, oh, ow, fn):
    return np.stack([fn(plane, oh, ow) for plane in x])


@pytest.mark.parametrize("C", CASES.CHANNELS)
@pytest.mark.parametrize("in_hw,out_hw", CASES.RESIZE_SHAPES)
def test_host_entry_equals_the_restatement(in_hw, out_hw, C):
    from masklab_hip import ops
    x = CASES.random_bytes((2, *in_hw, C), seed=in_hw[0] * 1000 + out_hw[1] * 10 + C)
    oh, ow = out_hw
    got = ops.cv_resize_reference_host(x, oh, ow)
    assert got.dtype == np.uint8 and got.shape == (2, oh, ow, C)
    np.testing.assert_array_equal(got, _want(x, oh, ow, REF.resize_u8))
    rounded = np.round(_want(x, oh, ow, REF.resize_f64))
    as_f32 = ops.cv_resize_reference_host(x, oh, ow, mode="round_f32")
    as_u8 = ops.cv_resize_reference_host(x, oh, ow, mode="round_u8")
    assert as_f32.dtype == np.float32 and as_u8.dtype == np.uint8
    np.testing.assert_array_equal(as_f32, rounded.astype(np.float32))
    np.testing.assert_array_equal(as_u8, rounded.astype(np.uint8))
    if in_hw == out_hw:                                               # the identity
        np.testing.assert_array_equal(got, x)
        np.testing.assert_array_equal(as_u8, x)


def test_area_branch_equals_the_linear_formula_and_rounds_halves_to_even():
    """Exactly 2x on both axes takes the INTER_AREA formulas.  One would expect them to differ from the linear formulas on
    random bytes; they cannot: at 2x every tap fraction is exactly 0.5, both fixed-point coefficients are 1024, and
    ((1024 * ((S0 + S1) * 1024 >> 4)) >> 16) is S0 + S1 -- the linear formula reduces to (sum + 2) >> 2, and in float64
    (S00 * .5 + S01 * .5) * .5 + ... is exact and equal to sum * 0.25.  So the test holds the stronger, true statement: the
    two formulations agree byte for byte, and the library's host loops (which take the area path there) equal both."""
    from masklab_hip import ops
    (H, W), (oh, ow) = CASES.AREA_SHAPE
    assert REF.is_area(H, W, oh, ow) and not REF.is_area(64, 100, 32, 64)
    x = CASES.random_bytes((1, H, W, 3), seed=5)
    area_u8, lin_u8 = REF.resize_u8(x[0], oh, ow), REF.linear_u8(x[0], oh, ow)
    area_f64, lin_f64 = REF.resize_f64(x[0], oh, ow), REF.linear_f64(x[0], oh, ow)
    np.testing.assert_array_equal(area_u8, lin_u8)
    np.testing.assert_array_equal(area_f64, lin_f64)
    np.testing.assert_array_equal(ops.cv_resize_reference_host(x, oh, ow)[0], area_u8)
    halves = float(np.mean(area_f64 - np.floor(area_f64) == 0.5))
    print(f"float64 area results that end in .5: {halves:.3f}")
    assert halves > 0
    got = ops.cv_resize_reference_host(x, oh, ow, mode="round_u8")[0]
    np.testing.assert_array_equal(got, np.round(area_f64).astype(np.uint8))
    ties = area_f64 - np.floor(area_f64) == 0.5
    assert (got[ties] % 2 == 0).all() and (got[ties] == np.floor(area_f64[ties]) + (np.floor(area_f64[ties]) % 2)).all()


def test_masks_as_bytes_and_skipped_planes():
    from masklab_hip import ops
    ds = CASES.TinyDataset(4, 45, 80)
    masks = ds.instance
    assert (masks[:, :, 0, 0] == -1).any() and (masks[:, :, 0, 0] != -1).any() and (masks < -1).any()
    got = ops.cv_resize_reference_host(masks, 32, 32, skip_minus_one=True)
    assert got.dtype == np.int8 and got.shape == (4, 4, 32, 32)
    for i in range(4):
        for j in range(4):
            if masks[i, j, 0, 0] == -1:
                assert (got[i, j] == -1).all()
            else:
                np.testing.assert_array_equal(got[i, j].view(np.uint8), REF.resize_u8(masks[i, j].view(np.uint8)[..., None], 32, 32)[..., 0])
    # without the flag a -1 plane is resized like any other (255 everywhere stays 255)
    plain = ops.cv_resize_reference_host(masks, 32, 32)
    np.testing.assert_array_equal(plain[2, 0].view(np.uint8), np.full((32, 32), 255, np.uint8))


def test_host_entry_rejects_bad_sizes():
    from masklab_hip import ops
    x = CASES.random_bytes((1, 4, 4, 3), seed=1)
    with pytest.raises(ValueError):
        ops.cv_resize_reference_host(x, 0, 4)
    with pytest.raises(TypeError):
        ops.cv_resize_reference_host(x.astype(np.float32), 4, 4)
    with pytest.raises(ValueError):
        ops.cv_resize_reference_host(x, 4, 4, mode="cubic")
    import ctypes as C
    from masklab_hip import _lib
    lib = _lib.load()
    out = np.zeros(64, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.ml_cv_resize_reference_host(p(x), p(out), 0, 1, 4, 4, 3, -1, 4, 0) != 0
    assert lib.ml_cv_resize_reference_host(p(x), p(out), 0, 1, 1 << 15, 1 << 15, 2, 4, 4, 0) != 0        # H*W*C = 2^31
    assert lib.ml_cv_resize_reference_host(p(x), p(out), 7, 1, 4, 4, 3, 4, 4, 0) != 0
    assert lib.ml_cv_resize_linear_u8(None, None, 1, 4, 4, 3, 0, 4, 0, None) != 0                          # refused before any launch
    assert lib.ml_cv_resize_linear_round_u8(None, None, 1, 1, 1 << 16, 1 << 15, 1, 4, 4, None) != 0
    assert b"cv_resize" in lib.ml_last_error()


# ----------------------------------------------------------------------------- the generator
def _same_batch(got, want, seg_dtype=np.float32):
    assert list(got) == ["images", "gt_seg", "gt_seg_exist", "gt_boxes", "gt_boxes_exist", "gt_masks"]
    for name in ("images", "gt_seg", "gt_masks"):
        assert isinstance(got[name], torch.Tensor)
    g = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    dtypes = dict(images=np.uint8, gt_seg=seg_dtype, gt_masks=np.int8, gt_seg_exist=np.float64, gt_boxes=np.float64,
                  gt_boxes_exist=np.float64)
    for name, dt in dtypes.items():
        assert g[name].dtype == dt and g[name].shape == want[name].shape, (name, g[name].dtype, g[name].shape, want[name].shape)
        np.testing.assert_array_equal(g[name], want[name].astype(dt), err_msg=name)       # gt_seg: float64 integers 0..255
    return g


def test_generator_on_cpu_equals_the_restated_getitem():
    from masklab_hip.utils import MaskLabGenerator
    from masklab_hip.utils.generator.masklab import MaskLabGenerator as Same
    assert Same is MaskLabGenerator
    ds = CASES.TinyDataset(5, 45, 80)
    gen = MaskLabGenerator(ds, scale_ratio=0.75, batch_size=2, shuffle=False, device="cpu")
    assert len(gen) == 2
    before = ds.detection.copy()
    for i in range(2):
        (got,) = gen[i]
        (want,) = REF.getitem(CASES.TinyDataset(5, 45, 80), i, 2, 0.75)
        g = _same_batch(got, want)
        assert g["images"].shape == (2, 32, 32, 3) and g["gt_seg"].shape == (2, 32, 32, 3) and g["gt_masks"].shape == (2, 4, 32, 32)
        live = before[2 * i:2 * i + 2, :, 5] > 0
        assert live.any() and not live.all()
        np.testing.assert_array_equal(g["gt_boxes"][~live], -1.0)
        np.testing.assert_array_equal(g["gt_boxes"][live][:, 0], before[2 * i:2 * i + 2][live][:, 0] * (32 / 80))
    np.testing.assert_array_equal(ds.detection, before)                # the documented deviation: scaled on a copy
    (as_u8,) = MaskLabGenerator(ds, 0.75, 2, False, device="cpu", seg_dtype=torch.uint8)[0]
    _same_batch(as_u8, REF.getitem(CASES.TinyDataset(5, 45, 80), 0, 2, 0.75)[0], seg_dtype=np.uint8)


def test_generator_area_size_tuple_scale_shuffle_and_torch_inputs():
    from masklab_hip.utils import MaskLabGenerator
    ds = CASES.TinyDataset(4, 64, 128, seed=3)
    (got,) = MaskLabGenerator(ds, 0.5, 4, False, device="cpu")[0]       # 64 x 128 -> 32 x 64: the INTER_AREA branch
    _same_batch(got, REF.getitem(CASES.TinyDataset(4, 64, 128, seed=3), 0, 4, 0.5)[0])
    # a tuple draws the scale from the seeded rng, once per batch
    gen = MaskLabGenerator(ds, (0.55, 0.95), 2, False, device="cpu", rng=np.random.default_rng(11))
    rng = np.random.default_rng(11)
    sizes = set()
    for i in (0, 1, 0):
        (got,) = gen[i]
        (want,) = REF.getitem(CASES.TinyDataset(4, 64, 128, seed=3), i, 2, (0.55, 0.95), rng=rng)
        sizes.add(_same_batch(got, want)["images"].shape[1:3])
    assert len(sizes) > 1, sizes
    # None is the global np.random, as in the reference
    np.random.seed(4)
    (got,) = MaskLabGenerator(ds, [0.55, 0.95], 2, False, device="cpu")[1]
    np.random.seed(4)
    _same_batch(got, REF.getitem(CASES.TinyDataset(4, 64, 128, seed=3), 1, 2, [0.55, 0.95])[0])

    class Tensors(CASES.TinyDataset):
        def __getitem__(self, sl):
            return {k: torch.from_numpy(v) for k, v in super().__getitem__(sl).items()}
    (got,) = MaskLabGenerator(Tensors(4, 64, 128, seed=3), 0.5, 4, False, device="cpu")[0]
    _same_batch(got, REF.getitem(CASES.TinyDataset(4, 64, 128, seed=3), 0, 4, 0.5)[0])
    # shuffle=True shuffles at construction and at every epoch end
    shuffled = CASES.TinyDataset(4, 64, 128, seed=3)
    gen = MaskLabGenerator(shuffled, 0.5, 4, True, device="cpu")
    first = shuffled.order.copy()
    twin = CASES.TinyDataset(4, 64, 128, seed=3)
    twin.shuffle()
    np.testing.assert_array_equal(first, twin.order)
    gen.on_epoch_end()
    twin.shuffle()
    np.testing.assert_array_equal(shuffled.order, twin.order)


def test_generator_argument_errors_and_no_instances():
    from masklab_hip.utils import MaskLabGenerator
    with pytest.raises(NotImplementedError, match="out of scope"):
        MaskLabGenerator(dict(image_dir="x"), device="cpu")
    with pytest.raises(ValueError):
        MaskLabGenerator([1, 2, 3], device="cpu")
    with pytest.raises(ValueError):
        MaskLabGenerator(CASES.TinyDataset(2, 45, 80), device="cpu", seg_dtype=torch.float64)
    class Wrong(CASES.TinyDataset):
        def __getitem__(self, sl):
            return {**super().__getitem__(sl), **self.swap}
    for swap in (dict(instance=np.zeros((2, 4, 45, 80), np.uint8)), dict(semantic=np.zeros((2, 45, 80, 3), np.float32)),
                 dict(images=np.zeros((2, 45, 80), np.uint8))):
        wrong = Wrong(2, 45, 80)
        wrong.swap = swap
        with pytest.raises(TypeError, match=next(iter(swap))):
            MaskLabGenerator(wrong, 0.75, 2, False, device="cpu")[0]
    with pytest.raises(ValueError, match="target size"):
        MaskLabGenerator(CASES.TinyDataset(2, 45, 80), 0.5, 2, False, device="cpu")[0]        # 22 x 40 -> 0 x 32
    empty = CASES.TinyDataset(2, 45, 80, n=0)
    (got,) = MaskLabGenerator(empty, 0.75, 2, False, device="cpu")[0]
    g = _same_batch(got, REF.getitem(CASES.TinyDataset(2, 45, 80, n=0), 0, 2, 0.75)[0])
    assert g["gt_masks"].shape == (2, 0, 32, 32) and g["gt_boxes"].shape == (2, 0, 6)


# ----------------------------------------------------------------------------- validate
class _StubTrainer:
    output_names = ["class_loss", "box_loss", "detection_recall_metric", "seg_loss", "my_road_metric"]

    def __init__(self):
        self.seen = []

    def __call__(self, X):
        assert set(X) == {"images", "gt_seg", "gt_seg_exist", "gt_boxes", "gt_boxes_exist", "gt_masks"}
        B = X["images"].shape[0]
        k = len(self.seen)
        self.seen.append(B)
        base = torch.arange(B, dtype=torch.float32) + 10 * k
        return [base * 0.1 + j for j in range(len(self.output_names))]


def test_validate_reports_means_over_all_samples_and_the_loss_sum():
    from masklab_hip.evaluate import validate
    from masklab_hip.utils import MaskLabGenerator
    gen = MaskLabGenerator(CASES.TinyDataset(7, 45, 80), 0.75, 3, False, device="cpu")
    stub = _StubTrainer()
    got = validate(stub, gen)
    assert stub.seen == [3, 3]                                         # the remainder is dropped
    per_sample = np.concatenate([(np.arange(3, dtype=np.float32) + 10 * k) * np.float32(0.1) for k in range(2)])
    want = {f"val_{n}": float(np.mean((per_sample + np.float32(j)).astype(np.float32).astype(np.float64)))
            for j, n in enumerate(stub.output_names)}
    want["val_loss"] = want["val_class_loss"] + want["val_box_loss"] + want["val_seg_loss"]
    assert list(got) == list(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-15, abs=0), k
    one = validate(_StubTrainer(), gen, steps=1)
    assert one["val_class_loss"] == pytest.approx(float(np.mean(per_sample[:3].astype(np.float64))), rel=1e-15)
    with pytest.raises(ValueError):
        validate(_StubTrainer(), gen, steps=3)
    with pytest.raises(ValueError):
        validate(_StubTrainer(), gen, steps=0)
