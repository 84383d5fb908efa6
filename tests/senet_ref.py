"""CPU restatement of the SE-ResNeXt-50 and SE-ResNet-50 backbones (test infrastructure, not collected: no `test_`
prefix), written on oracle.tfops and oracle.masklab.grouped_conv_fast from the vendored thirdparty/classification_models
source:
  senet.py SENet :198-324 (pad 3 + conv 7x7/2 + BN + ReLU, pad 1 + 3x3/2 max-pool; repetitions 3, 4, 6, 3; outputs
  256 * 2^stage; stride 2 in the first unit of stages 2-4), SEResNetBottleneck :46-88 (conv1 1x1 width out/4 WITH the
  stride + BN + ReLU, pad 1 + dense 3x3 + BN + ReLU, conv3 1x1 + BN), SEResNeXtBottleneck :91-134 (conv1 1x1 width out/2
  + BN + ReLU, pad 1 + GroupConv2D 3x3 with the stride, 32 groups + BN + ReLU, conv3 1x1 + BN), the 1x1 (strided) shortcut
  conv + BN where the stride or the width changes, ChannelSE _common_blocks.py:88-119 (GAP -> 1x1 conv C/16 + bias ->
  relu -> 1x1 conv C + bias -> sigmoid -> Multiply), then Add and ReLU.  BN eps 9.999999747378752e-06.
Preprocess (engine/backbone/base.py:220-246): BackBonePreProcess(rgb=True, mean_shift=True, normalize=3).
Taps (base.py:133-146): C1 the stem ReLU; SE-ResNet-50 C2..C5 the stage outputs; SE-ResNeXt-50 C2..C4 the conv1 ReLU of
the next stage's first unit, C5 the last output.

`patch(monkeypatch)` puts it behind oracle.masklab.backbone_forward, which inference_forward / deploy_forward look up at
call time; every other backbone goes to the original function."""
import numpy as np

from oracle import masklab as O
from oracle import tfops as T

EPS = 9.999999747378752e-06
REPETITIONS = (3, 4, 6, 3)
TYPES = ("seresnet50", "seresnext50")
_ORIGINAL = O.backbone_forward


def _bn(x, w, name):
    return T.batch_norm(x, w[name + "/gamma"], w[name + "/beta"], w[name + "/moving_mean"], w[name + "/moving_variance"],
                        EPS)


def channel_se(x, w, name):
    dt = x.dtype
    m = x.mean(axis=(1, 2), keepdims=True)                                            # GlobalAveragePooling2D + expand
    h = T.relu(T.conv2d(m, w[name + "/conv1/kernel"], w[name + "/conv1/bias"], padding="valid"))
    g = T.sigmoid(T.conv2d(h, w[name + "/conv2/kernel"], w[name + "/conv2/bias"], padding="valid"))
    return (x * g.astype(dt)).astype(dt)


def group_kernel(w, base):
    """The 32 per-group kernels [3,3,c,c] as one [3,3,width,c] kernel: k[.., g*c+i, m] = K_g[.., i, m]."""
    return np.concatenate([w[f"{base}conv2/group{g}/kernel"] for g in range(32)], axis=2)


def unit(x, w, stage, block, stride, grouped):
    """-> (output, conv1 ReLU)."""
    base = f"stage{stage + 1}_unit{block + 1}_"
    y1 = T.conv2d(x, w[base + "conv1/kernel"], None, stride=1 if grouped else stride, padding="valid")
    y1 = T.relu(_bn(y1, w, base + "bn1"))
    if grouped:
        k = group_kernel(w, base)
        y = O.grouped_conv_fast(y1, k, 32, k.shape[-1], stride)
    else:
        y = T.conv2d(y1, w[base + "conv2/kernel"], None, padding=((1, 1), (1, 1)))
    y = T.relu(_bn(y, w, base + "bn2"))
    y = _bn(T.conv2d(y, w[base + "conv3/kernel"], None, padding="valid"), w, base + "bn3")
    if block == 0:
        residual = _bn(T.conv2d(x, w[base + "sc/kernel"], None, stride=stride, padding="valid"), w, base + "sc_bn")
    else:
        residual = x
    y = channel_se(y, w, base + "se")
    return T.relu(y + residual), y1


def senet50(x, w, backbone_type, repetitions=REPETITIONS):
    """x: the preprocessed image -> taps dict."""
    grouped = backbone_type == "seresnext50"
    taps = {}
    x = T.conv2d(x, w["conv0/kernel"], None, stride=2, padding=((3, 3), (3, 3)))
    x = T.relu(_bn(x, w, "bn0"))
    taps["C1"] = x
    x = T.max_pool(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), 3, 2)
    for stage, rep in enumerate(repetitions):
        for block in range(rep):
            stride = 2 if (block == 0 and stage > 0) else 1
            x, y1 = unit(x, w, stage, block, stride, grouped)
            if grouped and block == 0 and stage > 0:
                taps[f"C{stage + 1}"] = y1
        if not grouped or stage == len(repetitions) - 1:
            taps[f"C{stage + 2}"] = x
    return taps


def backbone_forward(images, w, backbone_type, backbone_outputs, literal_groups=True):
    """oracle.masklab.backbone_forward with 'seresnet50' and 'seresnext50' added."""
    bt = backbone_type.lower()
    if bt not in TYPES:
        return _ORIGINAL(images, w, backbone_type, backbone_outputs, literal_groups)
    taps = senet50(O.backbone_preprocess(images, rgb=True, mean_shift=True, normalize=3), w, bt)
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
