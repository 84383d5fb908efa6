"""CPU test of tests/backbone_refs.py as a whole: one patch() puts every restated backbone behind the oracle at once."""
import numpy as np

import backbone_refs as REFS

OUTPUTS = ("C1", "C2", "C3", "C4", "C5", "P6", "P7")


def test_every_restated_backbone_resolves_under_one_patch(monkeypatch):
    """(1, 32, 32, 3): stem 16x16, pool 8x8, stages 8, 4, 2, 1.  Each type's taps are its own body function's."""
    from masklab_hip import backbone as BB
    from masklab_hip import keras_like as K
    from oracle import masklab as O
    REFS.patch(monkeypatch)
    assert set(REFS.BODIES) | {"resnext50", "resnext101", "mobilenet"} == set(O.BACKBONES) == set(BB.BACKBONE_LAYERS)
    images = np.random.default_rng(32).integers(0, 256, (1, 32, 32, 3)).astype(np.float32)
    for bt in ("seresnet34", "seresnet50", "seresnext50", "resnet50"):
        K.clear_session()
        bb = BB.load_backbone(bt, OUTPUTS, 128)
        w = K.init_weights(bb.weight_specs(), 1)
        names, feats = O.backbone_forward(images, w, bt, OUTPUTS)
        assert names == list(OUTPUTS) == bb.output_names, bt
        body, preprocess, _ = REFS.BODIES[bt]
        taps = body(O.backbone_preprocess(images, **preprocess), w)
        for n, f in zip(names, feats):
            assert f.shape[1:3] == {"C1": (16, 16), "C2": (8, 8), "C3": (4, 4), "C4": (2, 2)}.get(n, (1, 1)), (bt, n, f.shape)
            if n in taps:
                np.testing.assert_array_equal(f, taps[n], err_msg=f"{bt} {n}")
