"""CPU restatement of the ResNet-50 backbone (test infrastructure, not collected: no `test_` prefix), written on
oracle.tfops from the published legacy Keras-Applications 1.0.x resnet50.py -- the model behind the reference's
`tensorflow.keras.applications.ResNet50` import (engine/backbone/base.py:10,190-195), identified by its Keras auto-named
taps `activation`, `activation_9`, `activation_21`, `activation_39`, `activation_48` (base.py:105-111):
  conv1_pad ZeroPadding 3, conv1 64 x 7x7 / 2 valid with bias, bn_conv1, ReLU (tap C1), pool1_pad ZeroPadding 1, max-pool
  3x3 / 2 valid; stages 2..5 of blocks a..c / a..d / a..f / a..c with filters (64, 64, 256) .. (512, 512, 2048); block `a`
  is a conv_block (shortcut res{s}a_branch1 1x1 + bn{s}a_branch1, the stride on it and on branch2a: 1 in stage 2, 2
  after), the others identity_blocks; a block is branch2a 1x1 + bn + ReLU, branch2b 3x3 'same' + bn + ReLU, branch2c 1x1
  + bn, Add, ReLU; every conv has a bias; BatchNormalization epsilon 1e-3 (the Keras default), scale and centre.
Preprocess: BackBonePreProcess(rgb=False, mean_shift=True, normalize=0).  Taps C2..C5: the last block of stages 2..5.
Like the rest of the oracle this is parity-unpinned against TensorFlow.

`patch(monkeypatch)` puts it behind oracle.masklab.backbone_forward, which inference_forward / deploy_forward look up at
call time; every other backbone goes to the original function."""
import numpy as np

from oracle import masklab as O
from oracle import tfops as T

EPS = 1e-3
STAGES = ((2, "abc", (64, 64, 256), 1), (3, "abcd", (128, 128, 512), 2), (4, "abcdef", (256, 256, 1024), 2),
          (5, "abc", (512, 512, 2048), 2))
TYPES = ("resnet50",)
_ORIGINAL = O.backbone_forward


def _bn(x, w, name):
    return T.batch_norm(x, w[name + "/gamma"], w[name + "/beta"], w[name + "/moving_mean"], w[name + "/moving_variance"],
                        EPS)


def _conv_bn(x, w, stage, block, branch, stride=1, padding="valid"):
    name = f"res{stage}{block}_branch{branch}"
    y = T.conv2d(x, w[name + "/kernel"], w[name + "/bias"], stride=stride, padding=padding)
    return _bn(y, w, f"bn{stage}{block}_branch{branch}")


def block(x, w, stage, blk, stride):
    """conv_block for blk == 'a', identity_block otherwise."""
    y = T.relu(_conv_bn(x, w, stage, blk, "2a", stride))
    y = T.relu(_conv_bn(y, w, stage, blk, "2b", padding="same"))
    y = _conv_bn(y, w, stage, blk, "2c")
    shortcut = _conv_bn(x, w, stage, blk, "1", stride) if blk == "a" else x
    return T.relu(y + shortcut)


def resnet50(x, w):
    """x: the preprocessed image -> taps dict."""
    taps = {}
    x = T.conv2d(x, w["conv1/kernel"], w["conv1/bias"], stride=2, padding=((3, 3), (3, 3)))
    x = T.relu(_bn(x, w, "bn_conv1"))
    taps["C1"] = x
    x = T.max_pool(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), 3, 2)
    for stage, blocks, _filters, stride in STAGES:
        for blk in blocks:
            x = block(x, w, stage, blk, stride if blk == "a" else 1)
        taps[f"C{stage}"] = x
    return taps


def backbone_forward(images, w, backbone_type, backbone_outputs, literal_groups=True):
    """oracle.masklab.backbone_forward with 'resnet50' added."""
    bt = backbone_type.lower()
    if bt not in TYPES:
        return _ORIGINAL(images, w, backbone_type, backbone_outputs, literal_groups)
    taps = resnet50(O.backbone_preprocess(images, rgb=False, mean_shift=True, normalize=0), w)
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
