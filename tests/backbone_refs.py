"""CPU restatements of the backbones the oracle does not carry (test infrastructure, not collected: no `test_` prefix),
written on oracle.tfops: SE-ResNet-34, SE-ResNet-50 / SE-ResNeXt-50 and ResNet-50, each with the citations of its source
in the docstring of its body function.  Like the rest of the oracle they are parity-unpinned against TensorFlow.

BODIES lists them in the format of oracle.masklab.BACKBONES.  `backbone_forward` is the oracle's with both tables;
`patch(monkeypatch)` puts the merged table behind oracle.masklab.backbone_forward, which inference_forward /
deploy_forward look up at call time, so that every restated and every oracle backbone resolves at once.

A test imports its family's names as `REF`: SERESNET34, SENET or RESNET50."""
import types

import numpy as np

from oracle import masklab as O
from oracle import tfops as T

REPETITIONS = (3, 4, 6, 3)


def _bn(x, w, name, eps):
    return T.batch_norm(x, w[name + "/gamma"], w[name + "/beta"], w[name + "/moving_mean"], w[name + "/moving_variance"],
                        eps)


def channel_se(x, w, name):
    """_common_blocks.py ChannelSE :88-119: GAP -> 1x1 conv C/16 + bias -> relu -> 1x1 conv C + bias -> sigmoid ->
    Multiply."""
    dt = x.dtype
    m = x.mean(axis=(1, 2), keepdims=True)                                            # GlobalAveragePooling2D + expand
    h = T.relu(T.conv2d(m, w[name + "/conv1/kernel"], w[name + "/conv1/bias"], padding="valid"))
    g = T.sigmoid(T.conv2d(h, w[name + "/conv2/kernel"], w[name + "/conv2/bias"], padding="valid"))
    return (x * g.astype(dt)).astype(dt)


# =========================================================================== SE-ResNet-34
SERESNET34_EPS = 2e-5


def seresnet34_unit(x, w, stage, block, stride, cut):
    base = f"stage{stage + 1}_unit{block + 1}_"
    a = T.relu(_bn(x, w, base + "bn1", SERESNET34_EPS))
    shortcut = x if cut == "pre" else T.conv2d(a, w[base + "sc/kernel"], None, stride=stride, padding="valid")
    y = T.conv2d(a, w[base + "conv1/kernel"], None, stride=stride, padding=((1, 1), (1, 1)))
    y = T.relu(_bn(y, w, base + "bn2", SERESNET34_EPS))
    y = T.conv2d(y, w[base + "conv2/kernel"], None, padding=((1, 1), (1, 1)))
    y = channel_se(y, w, base + "se")
    return y + shortcut, a


def seresnet34(x, w, repetitions=REPETITIONS):
    """From the vendored thirdparty/classification_models source:
      resnet.py ResNet :173-283 (bn_data scale=False, conv0 7x7/2 + bn0 + relu0, pad 1 + 3x3/2 max-pool, final bn1 +
      relu1), residual_conv_block :60-109 (pre-activation: bn1 + relu1; shortcut = sc(1x1, no bias) of that in a stage's
      first unit ('post' cut), the raw input otherwise; pad 1 + conv1 3x3 + bn2 + relu2; pad 1 + conv2 3x3; attention;
      Add), MODELS_PARAMS['seresnet34'] :297 (repetitions 3, 4, 6, 3; filters 64 * 2^stage), get_bn_params (eps 2e-5).
    Taps (engine/backbone/base.py:126-132): C1 relu0, C2..C4 stage{2..4}_unit1_relu1, C5 relu1.
    x: raw RGB 0..255 (BackBonePreProcess(rgb=True, mean_shift=False, normalize=0) is the identity) -> taps dict."""
    eps = SERESNET34_EPS
    taps = {}
    x = T.batch_norm(x, None, w["bn_data/beta"], w["bn_data/moving_mean"], w["bn_data/moving_variance"], eps)
    x = T.conv2d(x, w["conv0/kernel"], None, stride=2, padding=((3, 3), (3, 3)))
    x = T.relu(_bn(x, w, "bn0", eps))
    taps["C1"] = x
    x = T.max_pool(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), 3, 2)
    for stage, rep in enumerate(repetitions):
        for block in range(rep):
            stride = 2 if (block == 0 and stage > 0) else 1
            x, a = seresnet34_unit(x, w, stage, block, stride, "post" if block == 0 else "pre")
            if block == 0 and stage > 0:
                taps[f"C{stage + 1}"] = a                      # stage{s+1}_unit1_relu1: the previous stage's tap
    taps["C5"] = T.relu(_bn(x, w, "bn1", eps))
    return taps


# =========================================================================== SE-ResNet-50 / SE-ResNeXt-50
SENET_EPS = 9.999999747378752e-06


def group_kernel(w, base):
    """The 32 per-group kernels [3,3,c,c] as one [3,3,width,c] kernel: k[.., g*c+i, m] = K_g[.., i, m]."""
    return np.concatenate([w[f"{base}conv2/group{g}/kernel"] for g in range(32)], axis=2)


def senet50_unit(x, w, stage, block, stride, grouped):
    """-> (output, conv1 ReLU)."""
    eps = SENET_EPS
    base = f"stage{stage + 1}_unit{block + 1}_"
    y1 = T.conv2d(x, w[base + "conv1/kernel"], None, stride=1 if grouped else stride, padding="valid")
    y1 = T.relu(_bn(y1, w, base + "bn1", eps))
    if grouped:
        k = group_kernel(w, base)
        y = O.grouped_conv_fast(y1, k, 32, k.shape[-1], stride)
    else:
        y = T.conv2d(y1, w[base + "conv2/kernel"], None, padding=((1, 1), (1, 1)))
    y = T.relu(_bn(y, w, base + "bn2", eps))
    y = _bn(T.conv2d(y, w[base + "conv3/kernel"], None, padding="valid"), w, base + "bn3", eps)
    if block == 0:
        residual = _bn(T.conv2d(x, w[base + "sc/kernel"], None, stride=stride, padding="valid"), w, base + "sc_bn", eps)
    else:
        residual = x
    y = channel_se(y, w, base + "se")
    return T.relu(y + residual), y1


def senet50(x, w, backbone_type, repetitions=REPETITIONS):
    """From the vendored thirdparty/classification_models source, with oracle.masklab.grouped_conv_fast:
      senet.py SENet :198-324 (pad 3 + conv 7x7/2 + BN + ReLU, pad 1 + 3x3/2 max-pool; repetitions 3, 4, 6, 3; outputs
      256 * 2^stage; stride 2 in the first unit of stages 2-4), SEResNetBottleneck :46-88 (conv1 1x1 width out/4 WITH the
      stride + BN + ReLU, pad 1 + dense 3x3 + BN + ReLU, conv3 1x1 + BN), SEResNeXtBottleneck :91-134 (conv1 1x1 width
      out/2 + BN + ReLU, pad 1 + GroupConv2D 3x3 with the stride, 32 groups + BN + ReLU, conv3 1x1 + BN), the 1x1
      (strided) shortcut conv + BN where the stride or the width changes, ChannelSE, then Add and ReLU.  BN eps
      9.999999747378752e-06.
    Preprocess (engine/backbone/base.py:220-246): BackBonePreProcess(rgb=True, mean_shift=True, normalize=3).
    Taps (base.py:133-146): C1 the stem ReLU; SE-ResNet-50 C2..C5 the stage outputs; SE-ResNeXt-50 C2..C4 the conv1 ReLU
    of the next stage's first unit, C5 the last output.
    x: the preprocessed image -> taps dict."""
    grouped = backbone_type == "seresnext50"
    taps = {}
    x = T.conv2d(x, w["conv0/kernel"], None, stride=2, padding=((3, 3), (3, 3)))
    x = T.relu(_bn(x, w, "bn0", SENET_EPS))
    taps["C1"] = x
    x = T.max_pool(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), 3, 2)
    for stage, rep in enumerate(repetitions):
        for block in range(rep):
            stride = 2 if (block == 0 and stage > 0) else 1
            x, y1 = senet50_unit(x, w, stage, block, stride, grouped)
            if grouped and block == 0 and stage > 0:
                taps[f"C{stage + 1}"] = y1
        if not grouped or stage == len(repetitions) - 1:
            taps[f"C{stage + 2}"] = x
    return taps


# =========================================================================== ResNet-50
RESNET50_EPS = 1e-3
RESNET50_STAGES = ((2, "abc", (64, 64, 256), 1), (3, "abcd", (128, 128, 512), 2), (4, "abcdef", (256, 256, 1024), 2),
                   (5, "abc", (512, 512, 2048), 2))


def _conv_bn(x, w, stage, block, branch, stride=1, padding="valid"):
    name = f"res{stage}{block}_branch{branch}"
    y = T.conv2d(x, w[name + "/kernel"], w[name + "/bias"], stride=stride, padding=padding)
    return _bn(y, w, f"bn{stage}{block}_branch{branch}", RESNET50_EPS)


def resnet50_block(x, w, stage, blk, stride):
    """conv_block for blk == 'a', identity_block otherwise."""
    y = T.relu(_conv_bn(x, w, stage, blk, "2a", stride))
    y = T.relu(_conv_bn(y, w, stage, blk, "2b", padding="same"))
    y = _conv_bn(y, w, stage, blk, "2c")
    shortcut = _conv_bn(x, w, stage, blk, "1", stride) if blk == "a" else x
    return T.relu(y + shortcut)


def resnet50(x, w):
    """From the published legacy Keras-Applications 1.0.x resnet50.py -- the model behind the reference's
    `tensorflow.keras.applications.ResNet50` import (engine/backbone/base.py:10,190-195), identified by its Keras
    auto-named taps `activation`, `activation_9`, `activation_21`, `activation_39`, `activation_48` (base.py:105-111):
      conv1_pad ZeroPadding 3, conv1 64 x 7x7 / 2 valid with bias, bn_conv1, ReLU (tap C1), pool1_pad ZeroPadding 1,
      max-pool 3x3 / 2 valid; stages 2..5 of blocks a..c / a..d / a..f / a..c with filters (64, 64, 256) .. (512, 512,
      2048); block `a` is a conv_block (shortcut res{s}a_branch1 1x1 + bn{s}a_branch1, the stride on it and on branch2a: 1
      in stage 2, 2 after), the others identity_blocks; a block is branch2a 1x1 + bn + ReLU, branch2b 3x3 'same' + bn +
      ReLU, branch2c 1x1 + bn, Add, ReLU; every conv has a bias; BatchNormalization epsilon 1e-3 (the Keras default),
      scale and centre.
    Preprocess: BackBonePreProcess(rgb=False, mean_shift=True, normalize=0).  Taps C2..C5: the last block of stages 2..5.
    x: the preprocessed image -> taps dict."""
    taps = {}
    x = T.conv2d(x, w["conv1/kernel"], w["conv1/bias"], stride=2, padding=((3, 3), (3, 3)))
    x = T.relu(_bn(x, w, "bn_conv1", RESNET50_EPS))
    taps["C1"] = x
    x = T.max_pool(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), 3, 2)
    for stage, blocks, _filters, stride in RESNET50_STAGES:
        for blk in blocks:
            x = resnet50_block(x, w, stage, blk, stride if blk == "a" else 1)
        taps[f"C{stage}"] = x
    return taps


# =========================================================================== behind the oracle
_SENET_PREPROCESS = dict(rgb=True, mean_shift=True, normalize=3)
BODIES = {
    "seresnet34": (seresnet34, dict(rgb=True, mean_shift=False, normalize=0), "same"),
    "seresnet50": (lambda x, w: senet50(x, w, "seresnet50"), _SENET_PREPROCESS, "same"),
    "seresnext50": (lambda x, w: senet50(x, w, "seresnext50"), _SENET_PREPROCESS, "same"),
    "resnet50": (resnet50, dict(rgb=False, mean_shift=True, normalize=0), "same"),
}


def backbone_forward(images, w, backbone_type, backbone_outputs, literal_groups=True):
    """oracle.masklab.backbone_forward with the restated backbones added."""
    return O.backbone_forward(images, w, backbone_type, backbone_outputs, literal_groups, bodies={**O.BACKBONES, **BODIES})


def patch(monkeypatch):
    monkeypatch.setattr(O, "BACKBONES", {**O.BACKBONES, **BODIES})


def check_patch_keeps_the_oracle_backbones(monkeypatch):
    """Under patch() an oracle backbone gives the bits of the unpatched oracle, and an unknown type still raises."""
    import pytest
    from masklab_hip import backbone as BB
    from masklab_hip import keras_like as K
    outputs = ("C1", "C2", "C3", "C4", "C5", "P6", "P7")
    K.clear_session()
    w = K.init_weights(BB.load_backbone("resnext50", outputs, 128).weight_specs(), 1)
    images = np.random.default_rng(1).integers(0, 256, (1, 32, 32, 3)).astype(np.float32)
    names, want = O.backbone_forward(images, w, "resnext50", outputs, literal_groups=False)
    patch(monkeypatch)
    patched_names, got = O.backbone_forward(images, w, "resnext50", outputs, literal_groups=False)
    assert patched_names == names == list(outputs)
    for n, g, r in zip(names, got, want):
        np.testing.assert_array_equal(g, r, err_msg=n)
    with pytest.raises(NotImplementedError):
        O.backbone_forward(np.zeros((1, 32, 32, 3), np.float32), {}, "no_such_backbone", ("C5",))


_shared = dict(patch=patch, backbone_forward=backbone_forward,
               check_patch_keeps_the_oracle_backbones=check_patch_keeps_the_oracle_backbones)
SERESNET34 = types.SimpleNamespace(TYPES=("seresnet34",), EPS=SERESNET34_EPS, seresnet34=seresnet34, unit=seresnet34_unit,
                                   **_shared)
SENET = types.SimpleNamespace(TYPES=("seresnet50", "seresnext50"), EPS=SENET_EPS, senet50=senet50, unit=senet50_unit,
                              **_shared)
RESNET50 = types.SimpleNamespace(TYPES=("resnet50",), EPS=RESNET50_EPS, resnet50=resnet50, block=resnet50_block, **_shared)
