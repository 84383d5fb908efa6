"""GPU tests of the layers' device parameters and repack(): a head whose parameters stepped on the device and that re-packed
holds, in every tensor its kernels read, the bits of the same head freshly loaded from host copies of the stepped weights;
nothing moved; and a graph captured before the step replays with the stepped weights."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_memory as D
import layer_params_cases as LC
from masklab_hip import keras_like as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models():
    """Two builds of the default configuration's heads (the second is the freshly loaded witness) and the weights."""
    a, weights, _ = LC.build_heads()
    b, _, _ = LC.build_heads()
    return a, b, weights


def _step(params, seed):
    """Every parameter moves by a fixed pseudo-random amount of about 1e-2 of its scale (an optimizer's job; torch here)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for name in sorted(params):
        p = params[name]
        p.add_(torch.randn(p.shape, device=p.device, generator=gen) * (0.01 * float(p.abs().mean()) + 1e-3))


@pytest.mark.parametrize("name", LC.HEADS)
def test_stepped_and_repacked_head_is_the_freshly_loaded_head(dev, models, name):
    a, b, weights = models
    head, fresh = a[name], b[name]
    head.load_weights(weights, dev)
    LC.touch(head, "wino")                                   # made on the host before binding: re-packed in place
    params = head.device_params()
    assert set(params) == set(head.weight_specs())
    for step in (1, 2):
        _step(params, seed=step)
        if step == 1:
            before = {k: t.data_ptr() for k, t in LC.packings(head).items()}
            for t in LC.packings(head).values():             # the step's launch leans on nothing the forms held
                if not any(t.data_ptr() == p.data_ptr() for p in params.values()):
                    D.fill_bytes(t, D.POISON)
        head.repack()
        LC.touch(head, "dgrad")                              # first asked for after the step: made from the stepped master
        stepped = {k: v.detach().cpu().numpy() for k, v in params.items()}
        fresh.load_weights(dict(weights, **stepped), dev)
        LC.touch(fresh, "wino"), LC.touch(fresh, "dgrad")
        got, want = LC.packings(head), LC.packings(fresh)
        assert set(got) == set(want)
        if step == 1:
            assert all(got[k].data_ptr() == before[k] for k in before), "a packing moved"
        D.assert_same_bits(LC.to_host(got), LC.to_host(want), f"{name}, step {step}")
    assert head._repack_table.uploads <= 2                   # the second step added the dgrad forms: one more upload at most


def test_a_graph_captured_before_the_step_replays_with_the_stepped_weights(dev):
    K.clear_session()
    conv = K.Conv2D(32, 3, padding="same", activation="relu", name="graphed")
    conv.build((2, 24, 40, 32))
    weights = K.init_weights(conv.weight_specs(), 3)
    conv.load_weights(weights, dev)
    params = conv.device_params()
    x = torch.randn((2, 24, 40, 32), device=dev)
    conv(x)                                                  # warm-up: workspaces and lazy forms exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = conv(x)
    graph.replay()
    torch.cuda.synchronize()
    first = y.cpu().numpy().copy()
    _step(params, seed=5)
    conv.repack()
    graph.replay()
    torch.cuda.synchronize()
    fresh = K.Conv2D(32, 3, padding="same", activation="relu", name="graphed")
    fresh.build((2, 24, 40, 32))
    fresh.load_weights({k: v.cpu().numpy() for k, v in params.items()}, dev)
    want = fresh(x).cpu().numpy()
    D.assert_same_bits(y.cpu().numpy(), want, "replay after the step")
    assert not np.array_equal(first, want)
