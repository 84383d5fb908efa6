"""CPU tests of the layers' device parameters (Layer.device_params / repack_jobs): names, shapes, which tensors are the
kernels' own, what binds, what load_weights unbinds, and the refusals by name.  Packings live on the CPU here; the device's
bits are held in tests/test_gpu_layer_repack.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import layer_params_cases as LC
from masklab_hip import keras_like as K, ops
from masklab_hip.layers.misc import MobileSeparableConv2D, SqueezeExcite
from masklab_hip.normalization import GroupNormalization


@pytest.fixture(scope="module")
def heads():
    hs, weights, model = LC.build_heads()
    for h in hs.values():
        h.load_weights(weights, "cpu")
    return hs, weights, model


@pytest.mark.parametrize("name", LC.HEADS)
def test_names_and_shapes_are_those_of_init_weights(heads, name):
    h = heads[0][name]
    params, specs = h.device_params(), h.weight_specs()
    assert set(params) == set(specs)
    for k, t in params.items():
        assert t.dtype == torch.float32 and tuple(t.shape) == specs[k].shape, k
        assert np.array_equal(t.numpy(), np.asarray(heads[1][k], np.float32)), k      # the masters hold the loaded weights
    again = h.device_params()
    assert all(again[k] is params[k] or again[k].data_ptr() == params[k].data_ptr() for k in params)   # uploaded once
    units, plan = ops.repack_plan(h.repack_jobs())
    assert units > 0 and len(plan) == len(h.repack_jobs())


def test_keras_layout_tensors_are_the_kernels_own(heads):
    hs = heads[0]
    for h in hs.values():
        params = h.device_params()
        for l in LC.walk(h):
            if isinstance(l, GroupNormalization):
                assert params[f"{l.name}/gamma"] is l.gamma and params[f"{l.name}/beta"] is l.beta
            if isinstance(l, K.DepthwiseConv2D):
                assert params[f"{l.name}/depthwise_kernel"].data_ptr() == l.wgt.data_ptr()
                assert tuple(params[f"{l.name}/depthwise_kernel"].shape) == (3, 3, l.C, 1)
            if type(l) is K.Conv2D:
                assert l.dev.follows_master and l.dev.p.wgt is None
    mask = hs["mask"]
    params = mask.device_params()
    for block, wo in zip(mask.blocks, mask._tail_wo):
        assert params[f"{block[-1].name}/kernel"] is wo                  # the tail backward's operand is the master
        assert block[-2].dev.follows_master and block[-2].dev1x1.follows_master
    assert sum(j.get("kind") == "table" for j in mask.repack_jobs()) == len(mask.blocks)
    aspp = hs["aspp"]
    aspp.device_params()
    assert all(dc.follows_master for dc in aspp._concat_slices()) and len(aspp._own_repack_jobs()) == len(aspp._slices)


def test_load_weights_unbinds(heads):
    hs, weights, _ = heads
    seg = hs["seg"]
    before = seg.device_params()
    seg.load_weights(weights, "cpu")
    conv = next(l for l in LC.walk(seg) if type(l) is K.Conv2D)
    assert not conv.dev.follows_master and conv.dev.p.wgt is not None and seg.repack_jobs() == []
    after = seg.device_params()
    assert conv.dev.follows_master and set(after) == set(before)
    assert after[f"{conv.name}/kernel"] is not before[f"{conv.name}/kernel"]


def _loaded(layer, shape):
    layer.build(shape)
    layer.load_weights(K.init_weights(layer.weight_specs(), 0), "cpu")
    return layer


def test_layers_that_cannot_be_trained_yet_refuse_by_name(heads):
    _, weights, model = heads
    bn = ("bn", 1e-3, True)
    with pytest.raises(NotImplementedError, match=r"Conv2D.device_params \('folded'\): a layer with fold_bn"):
        _loaded(K.Conv2D(8, 3, use_bias=False, fold_bn=bn, name="folded"), (1, 8, 8, 8)).device_params()
    with pytest.raises(NotImplementedError, match=r"\('stem'\): a layer with image_input"):
        _loaded(K.Conv2D(8, 3, image_input=True, name="stem"), (1, 8, 8, 3)).device_params()
    with pytest.raises(NotImplementedError, match=r"GroupedConv2D.device_params \('grouped'\): not trainable yet"):
        _loaded(K.GroupedConv2D(64, 32, name="grouped"), (1, 8, 8, 64)).device_params()
    with pytest.raises(NotImplementedError, match=r"DepthwiseConv2D.device_params \('dwf'\): a layer with fold_bn"):
        _loaded(K.DepthwiseConv2D(fold_bn=bn, name="dwf"), (1, 8, 8, 8)).device_params()
    with pytest.raises(NotImplementedError, match=r"SqueezeExcite.device_params \('se'\): SqueezeExcite has no backward"):
        _loaded(SqueezeExcite(16., name="se"), (1, 8, 8, 32)).device_params()
    with pytest.raises(NotImplementedError, match=r"MobileSeparableConv2D.device_params \('sep'\): the separable unit"):
        _loaded(MobileSeparableConv2D(32, name="sep"), (1, 8, 8, 32)).device_params()
    with pytest.raises(NotImplementedError, match=r"Dense.device_params \('fc'\).*cannot be trained yet"):
        _loaded(K.Dense(4, name="fc"), (1, 8)).device_params()
    model.backbone_network.load_weights(weights, "cpu")
    with pytest.raises(NotImplementedError, match="fold_bn"):
        model.backbone_network.device_params()
    plain = _loaded(K.Conv2D(8, 3, name="plain"), (1, 8, 8, 8))
    ops.set_conv_math("f16")
    try:
        with pytest.raises(NotImplementedError, match="float32 only"):
            plain.device_params()
    finally:
        ops.set_conv_math("f32")
    assert not plain.dev.follows_master
    with pytest.raises(RuntimeError, match="no weights loaded"):
        K.Conv2D(8, 3, name="empty").device_params()


def test_a_conv_bound_on_its_own_cannot_take_the_tails_operand_later(heads):
    """MaskSubNet makes `_tail_wo` the output conv's master; a conv that was bound on its own first follows another tensor,
    and the head says so instead of stepping the lane table and the conv while the tail backward's operand stands still."""
    hs, weights, _ = heads
    mask = hs["mask"]
    mask.load_weights(weights, "cpu")
    mask.blocks[0][-1].device_params()
    with pytest.raises(RuntimeError, match="already follows another master kernel"):
        mask.device_params()
    mask.load_weights(weights, "cpu")
    params = mask.device_params()
    assert params[f"{mask.blocks[0][-1].name}/kernel"] is mask._tail_wo[0]


def test_repack_keeps_its_job_list_until_a_form_is_made(heads):
    hs, weights, _ = heads
    seg = hs["seg"]
    seg.load_weights(weights, "cpu")
    seg.device_params()
    epoch = ops.forms_epoch()
    calls = []
    real = ops.repack_weights
    ops.repack_weights = lambda jobs, table=None: calls.append(jobs)
    try:
        seg.repack(), seg.repack()
    finally:
        ops.repack_weights = real
    assert ops.forms_epoch() == epoch and calls[0] is calls[1]     # the same list of the same dicts: the table's fast path
    conv = next(l for l in LC.walk(seg) if type(l) is K.Conv2D)
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # a new form of a bound packing is made on the device
        conv.dev.wgt_x3
    assert ops.forms_epoch() > epoch                               # asking for it moved the epoch: the next repack() rebuilds
