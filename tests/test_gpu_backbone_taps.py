"""GPU test of the early exit every residual body shares (backbone/body.py): asked for a subset of the taps, a backbone
gives the bits of the full run and launches nothing beyond the last wanted stage.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backbone_cases import _need_gpu    # noqa: F401  (autouse)
import backbone_cases as CASES

SUBSETS = (("C1",), ("C2",), ("C2", "C4"), ("C5",))       # in the order of the stage each one ends at
SHAPE = (1, 72, 104, 3)                                   # odd maps: stem 36x52, then 18x26, 9x13, 5x7, 3x4


@pytest.mark.parametrize("bt", ["resnet50", "resnext50", "resnext101", "seresnet34", "seresnet50", "seresnext50"])
def test_a_tap_subset_gives_the_bits_of_the_full_run_and_stops_at_its_last_stage(bt):
    """The subsets without C1 take the fused stem + pool, the full run the conv + pool pair: documented to give the same
    bits.  A backbone's P6 / P7 read its last tap, so they are compared only where that is the full run's."""
    images = np.random.default_rng(72).integers(0, 256, SHAPE, dtype=np.uint8)
    bb, _ = CASES.load_backbone(bt, CASES.ALL_OUTPUTS, seed=1)
    got, _ = CASES.run_backbone(bb, images)
    full = dict(zip(bb.output_names, got))
    assert [full[k].shape[1:3] for k in ("C1", "C2", "C3", "C4", "C5")] == [(36, 52), (18, 26), (9, 13), (5, 7), (3, 4)]
    launches = []
    for subset in SUBSETS:
        sub, _ = CASES.load_backbone(bt, subset + ("P6", "P7"), seed=1)
        got, kernels = CASES.run_backbone(sub, images)
        assert sub.output_names == list(subset) + ["P6", "P7"]
        for name, g in zip(sub.output_names, got):
            if name in subset or subset[-1] == "C5":
                assert np.array_equal(g, full[name]), (bt, subset, name)
        launches.append(len(kernels))
        if subset == ("C1",):       # the stem conv and the pool, then P6_conv, P6_norm, P7_conv: no stage at all
            body = [k for k in kernels if k != "preprocess"]
            assert [k[:4] for k in body] == ["conv", "maxp", "conv", "grou", "conv"], (bt, kernels)
    assert launches == sorted(set(launches)), (bt, dict(zip(SUBSETS, launches)))
