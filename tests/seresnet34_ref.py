"""CPU restatement of the SE-ResNet-34 backbone (test infrastructure, not collected: no `test_` prefix), written on
oracle.tfops from the vendored thirdparty/classification_models source:
  resnet.py ResNet :173-283 (bn_data scale=False, conv0 7x7/2 + bn0 + relu0, pad 1 + 3x3/2 max-pool, final bn1 + relu1),
  residual_conv_block :60-109 (pre-activation: bn1 + relu1; shortcut = sc(1x1, no bias) of that in a stage's first unit
  ('post' cut), the raw input otherwise; pad 1 + conv1 3x3 + bn2 + relu2; pad 1 + conv2 3x3; attention; Add),
  MODELS_PARAMS['seresnet34'] :297 (repetitions 3, 4, 6, 3; filters 64 * 2^stage), get_bn_params (eps 2e-5),
  _common_blocks.py ChannelSE :88-119 (GAP -> 1x1 conv C/16 + bias -> relu -> 1x1 conv C + bias -> sigmoid -> Multiply).
Taps (engine/backbone/base.py:126-132): C1 relu0, C2..C4 stage{2..4}_unit1_relu1, C5 relu1.

`patch(monkeypatch)` puts it behind oracle.masklab.backbone_forward, which inference_forward / deploy_forward look up at
call time; every other backbone goes to the original function."""
import numpy as np

from oracle import masklab as O
from oracle import tfops as T

EPS = 2e-5
REPETITIONS = (3, 4, 6, 3)
_ORIGINAL = O.backbone_forward


def _bn(x, w, name):
    return T.batch_norm(x, w.get(name + "/gamma"), w[name + "/beta"], w[name + "/moving_mean"],
                        w[name + "/moving_variance"], EPS)


def channel_se(x, w, name):
    dt = x.dtype
    m = x.mean(axis=(1, 2), keepdims=True)                                            # GlobalAveragePooling2D + expand
    h = T.relu(T.conv2d(m, w[name + "/conv1/kernel"], w[name + "/conv1/bias"], padding="valid"))
    g = T.sigmoid(T.conv2d(h, w[name + "/conv2/kernel"], w[name + "/conv2/bias"], padding="valid"))
    return (x * g.astype(dt)).astype(dt)


def unit(x, w, stage, block, stride, cut):
    base = f"stage{stage + 1}_unit{block + 1}_"
    a = T.relu(_bn(x, w, base + "bn1"))
    shortcut = x if cut == "pre" else T.conv2d(a, w[base + "sc/kernel"], None, stride=stride, padding="valid")
    y = T.conv2d(a, w[base + "conv1/kernel"], None, stride=stride, padding=((1, 1), (1, 1)))
    y = T.relu(_bn(y, w, base + "bn2"))
    y = T.conv2d(y, w[base + "conv2/kernel"], None, padding=((1, 1), (1, 1)))
    y = channel_se(y, w, base + "se")
    return y + shortcut, a


def seresnet34(x, w, repetitions=REPETITIONS):
    """x: raw RGB 0..255 (BackBonePreProcess(rgb=True, mean_shift=False, normalize=0) is the identity) -> taps dict."""
    taps = {}
    x = T.batch_norm(x, None, w["bn_data/beta"], w["bn_data/moving_mean"], w["bn_data/moving_variance"], EPS)
    x = T.conv2d(x, w["conv0/kernel"], None, stride=2, padding=((3, 3), (3, 3)))
    x = T.relu(_bn(x, w, "bn0"))
    taps["C1"] = x
    x = T.max_pool(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), 3, 2)
    for stage, rep in enumerate(repetitions):
        for block in range(rep):
            stride = 2 if (block == 0 and stage > 0) else 1
            x, a = unit(x, w, stage, block, stride, "post" if block == 0 else "pre")
            if block == 0 and stage > 0:
                taps[f"C{stage + 1}"] = a                      # stage{s+1}_unit1_relu1: the previous stage's tap
    taps["C5"] = T.relu(_bn(x, w, "bn1"))
    return taps


def backbone_forward(images, w, backbone_type, backbone_outputs, literal_groups=True):
    """oracle.masklab.backbone_forward with 'seresnet34' added."""
    if backbone_type.lower() != "seresnet34":
        return _ORIGINAL(images, w, backbone_type, backbone_outputs, literal_groups)
    taps = seresnet34(O.backbone_preprocess(images, rgb=True, mean_shift=False, normalize=0), w)
    names, feats = [], []
    for key in ("C1", "C2", "C3", "C4", "C5"):
        if key in backbone_outputs:
            names.append(key)
            feats.append(taps[key])
    p6 = T.relu(T.conv2d(feats[-1], w["P6_conv/kernel"], w["P6_conv/bias"], stride=2, padding="same"))
    if "P6" in backbone_outputs:
        names.append("P6")
        feats.append(p6)
    g6 = T.group_norm(p6, w["P6_norm/gamma"], w["P6_norm/beta"], 32)
    p7 = T.relu(T.conv2d(g6, w["P7_conv/kernel"], w["P7_conv/bias"], stride=2, padding="same"))
    if "P7" in backbone_outputs:
        names.append("P7")
        feats.append(p7)
    return names, feats


def patch(monkeypatch):
    monkeypatch.setattr(O, "backbone_forward", backbone_forward)
