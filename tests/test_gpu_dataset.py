"""GPU tests of the dataset: MaskLabDataset on device="cuda" (device JPEG decode, the polygon kernels) against device="cpu"
(Pillow, the library's host loops) tensor for tensor, the generator on it against the generator on its in-memory twin, and a
batch as the Evaluator's ground truth without a host copy of the masks.  Everything is exact equality.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("PIL")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu, host    # noqa: F401  (_need_gpu: autouse)
import dataset_cases as DATA
import dirty_memory as DM


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(DATA.write_data_dir(str(tmp_path_factory.mktemp("data"))))


def _dataset(root, device):
    from masklab_hip.utils import MaskLabDataset
    return MaskLabDataset(instance_labels=DATA.INSTANCE_LABELS, semantic_labels=DATA.SEMANTIC_LABELS, data_dir=root,
                          min_area=DATA.MIN_AREA, except_semantic_labels=DATA.EXCEPT_LABELS, device=device)


def _host_batch(X):
    return {k: (host(v) if isinstance(v, torch.Tensor) else v) for k, v in X.items()}


def test_device_dataset_equals_the_cpu_dataset(root):
    on_dev, on_cpu = _dataset(root, "cuda"), _dataset(root, "cpu")
    images = DATA.read_images(root)
    for sl in (slice(0, 2), slice(2, 4), slice(0, 4)):
        with DM.poisoned():
            got = on_dev[sl]
        assert all(got[k].is_cuda for k in ("images", "semantic", "instance")) and isinstance(got["detection"], np.ndarray)
        got = _host_batch(got)
        DM.assert_same_bits(got, _host_batch(on_cpu[sl]), f"cases {sl}")           # the images too: both decoders give libjpeg's bytes
        DM.assert_same_bits(got, DATA.expected_batch(DATA.CASES[sl], images), f"cases {sl} against the restated __getitem__")
    for index in (1, "a.jpg", 2):
        DM.assert_same_bits(_host_batch(on_dev[index]), _host_batch(on_cpu[index]), f"sample {index}")


def test_generator_on_the_device_dataset_equals_the_in_memory_twin(root):
    from masklab_hip.utils import MaskLabGenerator
    on_files = MaskLabGenerator(_dataset(root, "cuda"), scale_ratio=0.5, batch_size=2, shuffle=False, device="cuda")
    in_memory = MaskLabGenerator(DATA.InMemory(root), scale_ratio=0.5, batch_size=2, shuffle=False, device="cuda")
    for i in range(2):
        (got,), (want,) = on_files[i], in_memory[i]
        assert got["gt_masks"].is_cuda and tuple(got["gt_masks"].shape) == (2, (3, 0)[i], 32, 32)
        DM.assert_same_bits(_host_batch(got), _host_batch(want), f"batch {i}")


def test_a_batch_is_the_evaluators_ground_truth_without_a_host_copy_of_the_masks(root, monkeypatch):
    from masklab_hip.evaluate import Evaluator
    batch = _dataset(root, "cuda")[0:2]
    B, n = batch["instance"].shape[:2]
    pr_detection = np.full((B, n, 6), -1, np.int32)
    live = batch["detection"][..., 5] > 0
    pr_detection[live] = np.concatenate([np.round(batch["detection"][live][:, :5]), np.full((int(live.sum()), 1), 90.0)], axis=1).astype(np.int32)
    pr_instance = np.ones((B, n, 28, 28), np.int32)
    pr_semantic = host(batch["semantic"]).astype(np.int32)
    pr_semantic[:, ::3] = 0
    labels = (list(DATA.INSTANCE_LABELS), list(DATA.SEMANTIC_LABELS))
    from_host = Evaluator(*labels)
    from_host.update(pr_detection, pr_instance, pr_semantic, batch["detection"], host(batch["instance"]), host(batch["semantic"]))
    moved = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (moved.append(t.numel()), real_cpu(t, *a, **k))[1])
    from_device = Evaluator(*labels)
    from_device.update(pr_detection, pr_instance, pr_semantic, batch["detection"], batch["instance"], batch["semantic"])
    monkeypatch.undo()
    assert moved and max(moved) < DATA.H * DATA.W, moved                             # counts and flags only: never a mask plane
    got, want = from_device.result(), from_host.result()
    for row in got:
        print(row, got[row])
    assert got == want
    assert got["car"]["counts"] == 2 and got["bump"]["counts"] == 2 and got["car"]["iou"] > 0 and got["my_road"]["counts"] == 2
