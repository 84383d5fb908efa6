"""The stale-memory helper (tests/dirty_memory.py) on CPU tensors, and the completeness of the GPU case table: every tag a
`workspace(` call of masklab_hip/ops.py uses has a case in tests/test_gpu_dirty_memory.py.  No GPU needed."""
import ast
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_memory as DM

# every dtype the package allocates with torch.empty / torch.empty_like (masklab_hip/ops.py, layers/, parallel.py)
FLOATS = (torch.float16, torch.float32, torch.float64)
SIGNED = (torch.int8, torch.int32, torch.int64)


@pytest.mark.parametrize("dtype", FLOATS + SIGNED + (torch.uint8,), ids=str)
def test_poison_reads_as_nan_minus_one_or_the_maximum(dtype):
    with DM.poisoned():
        tensors = [torch.empty((3, 5), dtype=dtype), torch.empty(7, dtype=dtype), torch.empty((), dtype=dtype),
                   torch.empty_like(torch.zeros((2, 3), dtype=dtype)), torch.empty((0, 4), dtype=dtype)]
    for t in tensors:
        a = t.numpy()
        assert DM.holds(a, 0xFF) and DM.poison_elements(a).all()
        if dtype in FLOATS:
            assert np.isnan(a).all()
        elif dtype in SIGNED:
            assert (a == -1).all()
        else:
            assert (a == 255).all()
    with DM.poisoned():
        key = torch.empty(4, dtype=torch.int64).numpy().view(np.uint64)          # the u64 sort keys of csrc/detect.hip
    assert (key == np.iinfo(np.uint64).max).all()


def test_a_dense_tensor_whose_last_stride_is_not_one_is_poisoned_too():
    with DM.poisoned():
        t = torch.empty((2, 3, 4, 5), dtype=torch.float32, memory_format=torch.channels_last)
    assert t.stride(-1) != 1 and torch.isnan(t).all()


def test_zeroed_is_the_same_patch_with_zero_bytes():
    with DM.zeroed():
        t = torch.empty((4, 4), dtype=torch.float32)
    assert DM.holds(t.numpy(), 0x00) and not DM.poison_elements(t.numpy()).any()


def test_the_patch_is_undone_on_exit_and_after_an_exception():
    real = (torch.empty, torch.empty_like)
    with DM.poisoned():
        assert torch.empty is not real[0] and torch.empty_like is not real[1]
    assert (torch.empty, torch.empty_like) == real
    with pytest.raises(KeyError):
        with DM.poisoned():
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like) == real
    with DM.poisoned():                                   # nested: each level restores what it found
        inner = torch.empty
        with DM.zeroed():
            assert DM.holds(torch.empty(3).numpy(), 0x00)
        assert torch.empty is inner and torch.isnan(torch.empty(3)).all()
    assert (torch.empty, torch.empty_like) == real


def test_workspaces_are_poisoned_on_entry_and_when_they_grow(monkeypatch):
    from masklab_hip import ops
    monkeypatch.setattr(ops, "_ws_cache", {("cpu", "a", 0): torch.zeros(32, dtype=torch.uint8)})
    monkeypatch.setattr(ops, "_ws_retired", [torch.zeros(16, dtype=torch.uint8)])
    with DM.poisoned():
        assert all(DM.holds(b.numpy(), 0xFF) for b in list(ops._ws_cache.values()) + ops._ws_retired)
        grown = torch.empty(64, dtype=torch.uint8)        # what ops.workspace() does when a buffer is outgrown
    assert DM.holds(grown.numpy(), 0xFF)


def test_interleaved_runs_x_y_x_and_snapshots_each_result():
    calls, buf = [], torch.zeros(3)

    def run_x():
        calls.append("x")
        return {"out": buf.add_(1), "n": len(calls), "raw": b"ab"}

    first, second = DM.interleaved(run_x, lambda: calls.append("y"))
    assert calls == ["x", "y", "x"]
    assert first["out"].tolist() == [1, 1, 1] and second["out"].tolist() == [2, 2, 2]      # copies, not views of `buf`
    DM.assert_same_bits(first["raw"], second["raw"])
    with pytest.raises(AssertionError, match="3 of 3 elements differ"):
        DM.assert_same_bits(second, first, "x")


def test_assert_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    nan = np.array([np.nan, 0.0], np.float32)
    DM.assert_same_bits(nan, nan.copy())
    with pytest.raises(AssertionError):
        DM.assert_same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    with pytest.raises(AssertionError):
        DM.assert_same_bits(nan, nan.astype(np.float64))
    with pytest.raises(AssertionError):
        DM.assert_same_bits(np.full(2, 0xFFFFFFFF, np.uint32).view(np.float32), nan[[0, 0]])


# ------------------------------------------------------------------ completeness of the GPU case table
def workspace_tags(path):
    """The tag of every `workspace(...)` call in the file (third positional argument or `tag=`; "ws" when left out)."""
    with open(path) as fh:
        tree = ast.parse(fh.read())
    tags = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", None)) == "workspace":
            tag = node.args[2] if len(node.args) > 2 else next((k.value for k in node.keywords if k.arg == "tag"), None)
            if tag is None:
                tags.append("ws")
            else:
                assert isinstance(tag, ast.Constant) and isinstance(tag.value, str), \
                    f"{path}:{node.lineno}: the workspace tag must be a string literal (the case table is keyed by it)"
                tags.append(tag.value)
    return tags


def test_every_workspace_tag_has_a_dirty_memory_case():
    import masklab_hip
    import test_gpu_dirty_memory as G                     # importable without a GPU: cases build lazily
    tags = workspace_tags(os.path.join(os.path.dirname(masklab_hip.__file__), "ops.py"))
    assert len(tags) >= 12 and {"conv", "det", "summary", "jpeg_entropy"} <= set(tags), tags
    covered = set().union(*(c.tags for c in G.CASES))
    missing = sorted(set(tags) - covered)
    assert not missing, f"ops.workspace tags without a case in tests/test_gpu_dirty_memory.py: {missing}"
    assert covered <= set(tags), f"cases name tags ops.py does not use: {sorted(covered - set(tags))}"
    names = [c.name for c in G.CASES]
    assert len(set(names)) == len(names)


def test_no_case_is_skipped_or_expected_to_fail():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_dirty_memory.py")
    with open(path) as fh:
        tree = ast.parse(fh.read())
    marks = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)} & {"skip", "skipif", "xfail"}
    assert not marks, f"tests/test_gpu_dirty_memory.py uses {sorted(marks)}"
