"""CPU tests of the dataset (no GPU): load_labels against hand-written tables, MaskLabDataset on device="cpu" (the library's
host loops, Pillow for the images) against the reference's __getitem__ restated on tests/polygon_ref.py, and the generator
on the dataset against the generator on its in-memory twin.  Everything is exact equality.  skimage parity is unpinned."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("PIL")

import dataset_cases as DATA


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(DATA.write_data_dir(str(tmp_path_factory.mktemp("data"))))


@pytest.fixture(scope="module")
def images(root):
    return DATA.read_images(root)


def _dataset(root, **kw):
    from masklab_hip.utils import MaskLabDataset
    args = dict(instance_labels=DATA.INSTANCE_LABELS, semantic_labels=DATA.SEMANTIC_LABELS, data_dir=root, min_area=DATA.MIN_AREA,
                except_semantic_labels=DATA.EXCEPT_LABELS, device="cpu")
    return MaskLabDataset(**{**args, **kw})


def _same(got, want, single=False):
    assert list(got) == ["images", "semantic", "semantic_exist", "detection", "instance", "instance_exist"]
    dtypes = dict(images=np.uint8, semantic=np.uint8, instance=np.uint8 if single else np.int8, detection=np.float64,
                  semantic_exist=np.float64, instance_exist=np.float64)
    for name, dt in dtypes.items():
        on_device = name in ("images", "semantic", "instance")
        assert isinstance(got[name], torch.Tensor if on_device else np.ndarray), name
        g = got[name].cpu().numpy() if on_device else got[name]
        assert g.dtype == dt and g.shape == want[name].shape, (name, g.dtype, g.shape, want[name].shape)
        np.testing.assert_array_equal(g, want[name].astype(dt), err_msg=name)


def test_load_labels_equals_the_hand_written_tables(root):
    import os
    from masklab_hip.utils.dataset import load_labels
    exists, annotations = load_labels(os.path.join(root, "labels"))
    assert exists == {"labels": DATA.LABELS, "files": DATA.EXISTS}
    assert [(a["file_name"], a["label"]) for a in annotations] == [(n, l) for n, l, _ in DATA.ANNOTATIONS]
    for a, (_, _, seg) in zip(annotations, DATA.ANNOTATIONS):
        assert set(a) == {"file_name", "cx", "cy", "w", "h", "label", "annotation"}
        assert a["annotation"].dtype == np.float64
        np.testing.assert_array_equal(a["annotation"], DATA._poly(seg))
        assert [a["cx"], a["cy"], a["w"], a["h"]] == DATA._bbox(seg) and a["w"] * a["h"] > 0
    assert annotations[0]["annotation"].shape == (4, 2)                     # two parts became one polygon


def test_slices_equal_the_restated_getitem(root, images):
    ds = _dataset(root)
    assert len(ds) == 4 and list(ds.cases) == DATA.CASES                    # cases=None: images/ listed and sorted
    first = ds[0:2]
    _same(first, DATA.expected_batch(DATA.CASES[0:2], images))
    assert first["instance"].shape == (2, 3, DATA.H, DATA.W) and first["detection"].shape == (2, 3, 6)
    inst = first["instance"].numpy()
    assert (inst[0, 1:] == -1).all() and (inst[0, 0] >= 0).all() and inst[0, 0].any() and (inst[1] >= 0).all()
    np.testing.assert_array_equal(first["detection"][0, 1:], -1.0)
    np.testing.assert_array_equal(first["detection"][1, :, 4], [1.0, 1.0, 0.0])   # bump, bump, car: folders, files, file order
    np.testing.assert_array_equal(first["detection"][..., 5], [[1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    # the window of the car that leaves the image starts at column 0 and is cut at the last row
    assert inst[1, 2, DATA.H - 2, 0] == 1
    # the below-min_area bump of a.jpg is no instance, but its label exists
    np.testing.assert_array_equal(first["instance_exist"], [[1.0, 1.0], [1.0, 1.0]])
    np.testing.assert_array_equal(first["semantic_exist"], [[1.0, 1.0], [0.0, 1.0]])      # b.jpg: listed under my_road, no annotation
    sem = first["semantic"].numpy()
    assert sem[0, :, :, 0].any() and sem[0, :, :, 1].any() and not sem[1].any() and sem.max() == 1
    _same(ds[1:4], DATA.expected_batch(DATA.CASES[1:4], images))
    _same(ds[[3, 0]], DATA.expected_batch(["d.jpg", "a.jpg"], images))
    with pytest.raises(ValueError):
        ds[4:6]


def test_a_batch_without_instances(root, images):
    ds = _dataset(root)
    got = ds[2:4]                                                           # c.jpg: in no file; d.jpg: a semantic label only
    _same(got, DATA.expected_batch(DATA.CASES[2:4], images))
    assert got["instance"].shape == (2, 0, DATA.H, DATA.W) and got["detection"].shape == (2, 0, 6)
    np.testing.assert_array_equal(got["semantic_exist"], [[0.0, 0.0], [1.0, 0.0]])
    np.testing.assert_array_equal(got["instance_exist"], [[0.0, 0.0], [1.0, 0.0]])        # d.jpg: listed under car, no annotation
    assert not got["semantic"][0].any() and got["semantic"][1, :, :, 0].any()


def test_int_and_str_indexing(root, images):
    ds = _dataset(root)
    for i, case in enumerate(DATA.CASES):
        want = DATA.expected_sample(case, images)
        _same(ds[i], want, single=True)
        _same(ds[case], want, single=True)
    assert ds[1]["instance"].shape == (3, DATA.H, DATA.W) and ds[2]["instance"].shape == (0, DATA.H, DATA.W)
    assert ds[np.int64(1)]["detection"].shape == (3, 6)
    with_cases = _dataset(root, cases=["d.jpg", "b.jpg"])
    assert len(with_cases) == 2
    _same(with_cases[0:2], DATA.expected_batch(["d.jpg", "b.jpg"], images))


def test_min_area_and_labels_choose_the_instances(root, images):
    ds = _dataset(root, min_area=10.0)                                      # the small bump of a.jpg is an instance now
    got = ds[0]
    assert got["detection"].shape == (2, 6)
    np.testing.assert_array_equal(got["detection"][:, 4], [1.0, 0.0])
    only_cars = _dataset(root, instance_labels=("car",), except_semantic_labels=())
    got = only_cars[0:2]
    assert got["instance"].shape == (2, 1, DATA.H, DATA.W) and got["instance_exist"].shape == (2, 1)
    # without the except label the car no longer cuts into the roads
    with_car = _dataset(root)[0]["semantic"].numpy()
    without = only_cars[0]["semantic"].numpy()
    assert (without >= with_car).all() and without.sum() > with_car.sum()


def test_images_of_different_sizes_are_refused(tmp_path):
    root = DATA.write_data_dir(str(tmp_path / "mixed"), sizes={"b.jpg": (48, 96)})
    ds = _dataset(root)
    with pytest.raises(ValueError, match="one size"):
        ds[0:2]
    assert ds[1]["images"].shape == (48, 96, 3)                             # alone it is fine


def test_an_instance_polygon_without_vertices_is_refused(root):
    ds = _dataset(root)
    ds._instances["a.jpg"][0] = ds._instances["a.jpg"][0][:5] + (np.zeros((0, 2)),)
    with pytest.raises(ValueError, match="without vertices"):
        ds[0:1]


def test_shuffle_get_config_and_construct(root):
    ds = _dataset(root, rng=np.random.default_rng(3), note="kept")
    want = np.array(DATA.CASES)
    np.random.default_rng(3).shuffle(want)
    ds.shuffle()
    assert list(ds.cases) == list(want) and sorted(want) == DATA.CASES
    np.random.seed(5)
    plain = _dataset(root)
    plain.shuffle()
    np.random.seed(5)
    want = np.array(DATA.CASES)
    np.random.shuffle(want)
    assert list(plain.cases) == list(want)
    assert _dataset(root, note="kept").get_config() == {"cases": DATA.CASES, "instance_labels": DATA.INSTANCE_LABELS,
                                                        "semantic_labels": DATA.SEMANTIC_LABELS, "data_dir": root,
                                                        "min_area": DATA.MIN_AREA, "note": "kept"}
    from masklab_hip import ModelConfiguration, retinamasklab as R
    from masklab_hip.utils import Dataset, MaskLabDataset, get_image_cases
    import os
    assert sorted(get_image_cases(os.path.join(root, "images/"))) == DATA.CASES and issubclass(MaskLabDataset, Dataset)
    with pytest.raises(NotImplementedError):
        len(Dataset())
    cfg = ModelConfiguration()
    cfg.dataset.data_dir = root
    cfg.dataset.train_cases, cfg.dataset.valid_cases = ["a.jpg", "b.jpg", "d.jpg"], ["c.jpg"]
    cfg.dataset.instance_labels, cfg.dataset.semantic_labels = DATA.INSTANCE_LABELS, DATA.SEMANTIC_LABELS
    cfg.dataset.min_area = DATA.MIN_AREA
    trainset, validset = R.construct_masklabdataset(cfg, device="cpu")
    assert list(trainset.cases) == ["a.jpg", "b.jpg", "d.jpg"] and list(validset.cases) == ["c.jpg"]
    assert trainset.except_semantic_labels == ("car",) and trainset.min_area == DATA.MIN_AREA and len(validset) == 1
    with pytest.raises(ValueError):
        _dataset(root, semantic_labels=tuple(f"s{i}" for i in range(17)))


def test_generator_on_the_dataset_equals_the_generator_on_its_in_memory_twin(root):
    from masklab_hip.utils import MaskLabGenerator
    on_files = MaskLabGenerator(_dataset(root), scale_ratio=0.5, batch_size=2, shuffle=False, device="cpu")
    in_memory = MaskLabGenerator(DATA.InMemory(root), scale_ratio=0.5, batch_size=2, shuffle=False, device="cpu")
    assert len(on_files) == len(in_memory) == 2
    for i in range(2):
        (got,), (want,) = on_files[i], in_memory[i]
        assert list(got) == list(want)
        for k in want:
            g, w = (v.numpy() if isinstance(v, torch.Tensor) else v for v in (got[k], want[k]))
            assert g.dtype == w.dtype and g.shape == w.shape, k
            np.testing.assert_array_equal(g, w, err_msg=k)
        assert got["images"].shape == (2, 32, 32, 3) and got["gt_masks"].shape == (2, (3, 0)[i], 32, 32)
