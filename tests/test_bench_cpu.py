"""bench.py without a GPU: the option surface (--full, --dump-outputs, --steps) and the output dump's size budget and
fixed sampling, on CPU tensors."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402


def _args(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = _args(monkeypatch, "--steps", "3", "--full", "--dump-outputs", "out")
    assert a.full is True and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        _args(monkeypatch, "--steps", "0")
    with pytest.raises(SystemExit):                     # the per-launch lines come from the --full roofline step
        _args(monkeypatch, "--dump-launches", "l.txt")
    assert _args(monkeypatch, "--full", "--dump-launches", "l.txt").dump_launches == "l.txt"


def test_dump_outputs_whole_when_small(tmp_path):
    g = torch.Generator().manual_seed(0)
    named = [("a", torch.randn(3, 4, generator=g).half()), ("b", torch.arange(10, dtype=torch.int32)),
             ("c", torch.randn(5, generator=g, dtype=torch.float64))]
    info = bench.dump_outputs(named, str(tmp_path))
    for name, t in named:
        x = np.load(tmp_path / f"{name}.npy")
        assert info[name] == {"shape": list(t.shape), "sampled": None}
        assert x.dtype == (np.float32 if name == "a" else np.float64)
        np.testing.assert_array_equal(x, t.double().numpy())


def test_dump_outputs_samples_large_arrays_within_budget_and_repeatably(tmp_path):
    g = torch.Generator().manual_seed(1)
    small = torch.randn(100, generator=g)
    big = torch.randn(40, 1000, generator=g)
    budget = 20000                                      # bytes: `small` whole, `big` sampled to what is left
    info = bench.dump_outputs([("big", big), ("small", small)], str(tmp_path / "1"), budget=budget)
    bench.dump_outputs([("big", big), ("small", small)], str(tmp_path / "2"), budget=budget)
    assert info["small"]["sampled"] is None
    k = info["big"]["sampled"]
    assert k == (budget - small.numel() * 4) // 4 and info["big"]["shape"] == [40, 1000]
    a1, a2 = np.load(tmp_path / "1" / "big.npy"), np.load(tmp_path / "2" / "big.npy")
    assert a1.shape == (k,) and a1.nbytes + small.numel() * 4 <= budget
    np.testing.assert_array_equal(a1, a2)                             # same elements on every run
    flat = big.reshape(-1).numpy()
    idx = np.sort(np.random.default_rng(big.numel()).choice(big.numel(), size=k, replace=False, shuffle=False))
    np.testing.assert_array_equal(a1, flat[idx])                      # distinct, sorted flat indices
    assert len(np.unique(idx)) == k
