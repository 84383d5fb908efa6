"""GPU tests of TrainerModel.train_on_batch(trainable="head_tune"): the reference's first training stage (everything behind
the C5 tap: the FPN, P6_conv / P6_norm / P7_conv and the head groups) on tests/train_step_cases.py's configuration,
2 x 64 x 96.  The layer backwards the step is composed of are held to float64 autograd in tests/test_gpu_fpn_grad.py and
tests/test_gpu_conv_dgrad_s2.py; here the step is held to their hand composition bit for bit, to finite differences along
the new weights, and to a freshly loaded model.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_memory as D
import layer_params_cases as LC
import train_step_cases as TC
from masklab_hip import ops
from masklab_hip.optimizers import AdamW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.detach().cpu().numpy().copy()


@pytest.fixture(scope="module")
def world():
    """Two (trainer, inference) pairs of one configuration and weights; the second pair is the freshly loaded witness."""
    assert torch.cuda.is_available(), "needs the MI355X"
    trainer, _ = TC.build()
    trainer2, _ = TC.build()
    return dict(trainer=trainer, trainer2=trainer2, weights=trainer.init_weights(seed=2), inputs=TC.inputs())


def _reset(world, which="trainer"):
    t = world[which]
    t.load_weights(world["weights"], DEV)
    return t


def _outputs(outs):
    return [host(o) for o in outs]


def _new_names(trainer):
    """The weights the stage adds to the head groups': the FPN's and the three extra-level layers'"""
    names = set(trainer.detection_networks[1].weight_specs())
    for l in trainer.backbone_network.extra_level_layers():
        names |= set(l.weight_specs())
    return names


def _head_names(trainer):
    names = set()
    for g in trainer.head_groups():
        names |= set(g.weight_specs())
    return names


def hand_head_tune_grads(trainer, batch, upstream=None):
    """The composition the step is held to: the forward with tapes, then the layer backwards called by hand in the order the
    issue fixes -- per pyramid level the class tower's, the box tower's and the RoI align's gradients summed in that order.
    -> (outputs, {name: gradient})"""
    grads, tapes = {}, {}
    outs = trainer._forward(batch, dict(upstream=dict(upstream or {}), through_sigmoid=True, grads=grads, tapes=tapes,
                                        head_tune=True))
    _, fpn, cls, loc = trainer.detection_networks
    _, _, pra, mask = trainer.instance_networks
    aspp, seg = trainer.semantic_networks
    bb = trainer.backbone_network
    wg = {}
    d_cls, g = cls.backward(tapes[cls.name], grads["cls_pred"])
    wg.update(g)
    d_loc, g = loc.backward(tapes[loc.name], grads["loc_pred"])
    wg.update(g)
    d_rois, g = mask.backward(tapes[mask.name], grads["roi_masks"], need_dx=True)
    wg.update(g)
    t = tapes[pra.name]
    n = len(t["fmap_shapes"])
    assert n == trainer.configuration.instance.max_k + 1
    d_roi = pra.backward(d_rois, t["fmap_shapes"], t["rows"], t["image_hw"], t["slots"], t["lcounts"])
    d_feat = []
    for l, (a, b) in enumerate(zip(d_cls, d_loc)):
        s = a + b                                            # torch's float32 addition: the same single rounding
        d_feat.append(s + d_roi[l] if l < n else s)
    assert tapes["feature_names"] == ["C3", "C4", "C5", "P6", "P7"]
    wg.update(bb.backward_extra_levels(tapes[bb.name], d_feat[3], d_feat[4])[1])
    wg.update(fpn.backward(tapes[fpn.name], d_feat[:3])[1])
    (d_aspp, _), g = seg.backward(tapes[seg.name], grads["seg_pred"], need_dx=(True, False))
    wg.update(g)
    wg.update(aspp.backward(tapes[aspp.name], d_aspp, need_dx=False)[1])
    return outs, wg


def test_outputs_are_calls(world):
    want = _outputs(_reset(world)(world["inputs"]))
    trainer = _reset(world)
    got = _outputs(trainer.train_on_batch(world["inputs"], AdamW(1e-3), trainable="head_tune"))
    D.assert_same_bits(got, want, "a head_tune step's outputs against call's")


def test_gradient_keys_and_the_composition(world):
    trainer = _reset(world)
    _, want = hand_head_tune_grads(trainer, world["inputs"])
    want = {k: host(v) for k, v in want.items()}
    trainer = _reset(world)
    trainer.train_on_batch(world["inputs"], AdamW(1e-3))
    heads = {k: host(v) for k, v in trainer.last_forward["weight_grads"].items()}
    trainer = _reset(world)
    assert set(trainer.device_params()) == _head_names(trainer)             # the default stays the head names
    trainer.train_on_batch(world["inputs"], AdamW(1e-3), trainable="head_tune")
    got = {k: host(v) for k, v in trainer.last_forward["weight_grads"].items()}
    new = _new_names(trainer)
    assert {n.split("/")[0] for n in new} >= {"P6_conv", "P6_norm", "P7_conv"} and len(new) == 6 + 12
    assert set(got) == _head_names(trainer) | new == set(trainer.device_params(stage="head_tune"))
    assert not set(got) & set(trainer.backbone_network.body.weight_specs())
    for k in sorted(got):
        D.assert_same_bits(got[k], want[k], f"{k} against the hand composition")
    for k in sorted(heads):                                  # the head gradients do not depend on the stage
        D.assert_same_bits(got[k], heads[k], f"{k} against a 'heads' step")
    assert all(np.isfinite(v).all() for v in got.values()) and all(np.abs(got[k]).max() > 0 for k in new)


def test_the_mask_loss_reaches_the_fpn_through_roi_align(world):
    trainer = _reset(world)
    zero = np.zeros(2, np.float32)
    up = {"class_loss": zero, "box_loss": zero, "seg_loss": zero}
    trainer.train_on_batch(world["inputs"], AdamW(1e-3), trainable="head_tune", upstream=up)
    wg = {k: host(v) for k, v in trainer.last_forward["weight_grads"].items()}
    # The batch's RoIs are small: they are cropped from the finest level.  Its 3x3 conv receives their gradient, and the
    # top-down chain carries it into every lateral; a coarser level's 3x3 conv nobody cropped from has an exact zero.
    fpn = trainer.detection_networks[1]
    reached = [f"{l.name}/{k}" for b in fpn.blocks for l in (b[0],) for k in ("kernel", "bias")]
    reached += [f"{fpn.blocks[-1][1].name}/{k}" for k in ("kernel", "bias")]
    assert len(reached) == 8 and all(np.abs(wg[k]).max() > 0 for k in reached), [k for k in reached if not np.abs(wg[k]).max() > 0]
    assert all(np.isfinite(wg[k]).all() for k in fpn.weight_specs())
    towers = [k for k in wg if k.split("/")[0] in (trainer.detection_networks[2].name, trainer.detection_networks[3].name)]
    assert towers and all(not wg[k].any() for k in towers)


def test_first_order_check_against_finite_differences(world):
    """tests/test_gpu_train_step.py's check with its bound and its 5 % condition, along d = g / |g| over the FPN and
    extra-level weights ONLY: g.d against central differences of L = the sum of the batch means of the class, box and seg
    losses (mask_loss's upstream is zero: its RoIs move discontinuously).  |g.d - fd(eps/2)| <= 3 |fd(eps) - fd(eps/2)| +
    2^-20 |L| / eps, with eps chosen so that the right side is below 5 % of |g.d|."""
    trainer = _reset(world)
    batch, names = world["inputs"], ("class_loss", "box_loss", "seg_loss")
    up = {"mask_loss": np.zeros(2, np.float32)}
    new = _new_names(trainer)
    params = {k: v for k, v in trainer.device_params(stage="head_tune").items() if k in new}
    assert set(params) == new
    state0 = trainer.box_loss.state.clone()
    outs, wg = hand_head_tune_grads(trainer, batch, upstream=up)
    L0 = TC.loss_sum(trainer, outs, names)
    g = {k: host(wg[k]).astype(np.float64) for k in params}
    norm = float(np.sqrt(sum((v ** 2).sum() for v in g.values())))
    w0 = {k: v.clone() for k, v in params.items()}
    d = {k: torch.from_numpy((g[k] / norm).astype(np.float32)).to(DEV) for k in params}
    gd = norm                                                     # g . (g / |g|)

    def L(step):
        for k, p in params.items():
            p.copy_(w0[k] + step * d[k])
        trainer.repack("head_tune")
        trainer.box_loss.state.copy_(state0)
        return TC.loss_sum(trainer, trainer(batch), names)

    def fd(eps):
        return (L(eps) - L(-eps)) / (2 * eps)

    chosen = None
    for eps in (1e-2, 3e-3, 3e-2, 1e-3, 1e-1):
        wide, half = fd(eps), fd(eps / 2)
        rhs = 3 * abs(wide - half) + 2.0 ** -20 * abs(L0) / eps
        print(f"eps {eps:g}: fd(eps) {wide:.9g} fd(eps/2) {half:.9g} g.d {gd:.9g} L {L0:.9g} "
              f"|g.d - fd(eps/2)| {abs(gd - half):.3g} bound {rhs:.3g} ({rhs / abs(gd):.3%} of |g.d|)")
        if rhs < 0.05 * abs(gd):
            chosen = (eps, wide, half, rhs)
            break
    assert chosen is not None, "no eps brings the bound below 5 % of |g.d|"
    eps, wide, half, rhs = chosen
    assert abs(gd - half) <= rhs, (eps, gd, wide, half, rhs)


def _stepped_weights(world, trainer):
    """Host weights of the whole model as they stand: the stage's stepped parameters, the untouched body, box_loss's statistics."""
    w = dict(world["weights"])
    w.update({k: host(v) for k, v in trainer.device_params(stage="head_tune").items()})
    w["box_loss/moving_mean"], w["box_loss/moving_var"] = host(trainer.box_loss.moving_mean), host(trainer.box_loss.moving_var)
    return w


def _same_trainers(world, trainer, what):
    other = world["trainer2"]
    other.load_weights(_stepped_weights(world, trainer), DEV)
    state = trainer.box_loss.state.clone()
    a = _outputs(trainer(world["inputs"]))
    fa = {k: host(trainer.last_forward[k]) for k in ("cls_pred", "loc_pred", "roi_masks", "seg_pred")}
    trainer.box_loss.state.copy_(state)                           # `call` advanced the statistics: put them back
    b = _outputs(other(world["inputs"]))
    fb = {k: host(other.last_forward[k]) for k in fa}
    D.assert_same_bits(a, b, f"{what}: outputs")
    D.assert_same_bits(fa, fb, f"{what}: predictions")


def test_a_step_updates_everything_behind_c5_and_nothing_in_front(world):
    trainer = _reset(world)
    body = trainer.backbone_network.body
    trainer(world["inputs"])                                      # the forward's lazy forms exist before the snapshot
    trainer.box_loss.load_weights(world["weights"], DEV)
    frozen = LC.to_host(LC.all_tensors(body))
    assert len(frozen) > 10
    opt = AdamW(1e-3)
    before = {k: host(v) for k, v in trainer.device_params(stage="head_tune").items()}
    trainer.train_on_batch(world["inputs"], opt, trainable="head_tune")
    after = {k: host(v) for k, v in trainer.device_params(stage="head_tune").items()}
    new = _new_names(trainer)
    still = [k for k in new if np.array_equal(before[k], after[k])]
    assert not still, still
    assert sum(not np.array_equal(before[k], after[k]) for k in before) > len(before) // 2
    D.assert_same_bits(LC.to_host(LC.all_tensors(body)), frozen, "the backbone's body after a head_tune step")
    _same_trainers(world, trainer, "after one step")
    trainer.train_on_batch(world["inputs"], opt, trainable="head_tune")
    D.assert_same_bits(LC.to_host(LC.all_tensors(body)), frozen, "the backbone's body after two head_tune steps")
    _same_trainers(world, trainer, "after two steps")


def test_the_refusal_points_to_the_stage(world):
    trainer = _reset(world)
    fpn_name = next(iter(trainer.detection_networks[1].weight_specs()))
    with pytest.raises(NotImplementedError, match="FPN or the backbone.*head_tune"):
        trainer.train_on_batch(world["inputs"], AdamW(1e-3), trainable={fpn_name})
    with pytest.raises(ValueError, match="'heads', 'head_tune'"):
        trainer.train_on_batch(world["inputs"], AdamW(1e-3), trainable="everything")
    with pytest.raises(ValueError, match="stage must be one of"):
        trainer.device_params(stage="body")
