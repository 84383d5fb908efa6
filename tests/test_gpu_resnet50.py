"""GPU tests of the ResNet-50 backbone (the reference's default) and of its projection unit as one GEMM
(csrc/conv1x1_dual.hip): the dual kernel against fp64 from the very inputs it gets, in fp32 and in half storage, at the
bars tests/test_gpu_ops.py (fp32 1x1 conv with residual: atol 3e-5) and tests/test_gpu_f16_storage.py (half 1x1 conv
with residual: rtol 2^-10, atol 1e-4 against the half-rounded fp64 value) already apply, bit-stable run to run and per
image, with the pixels of `x` a strided unit must NOT read filled with 1e3; a K that is no multiple of the chunk is
refused by the library and run by `ops` as the two launches; the backbone taps against the test-side restatement
(tests/backbone_refs.py) in every conv math with the fusion on and off (the bars of tests/test_gpu_senet.py; f16s is
reported, not gated, as there); the default ModelConfiguration() end to end against the oracle with detections, their
order, device counts and one hipGraph; an .npz checkpoint through load_masklab_inference_model_from_h5 to the deploy
model.  -m gpu."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import masklab as O

from backbone_cases import _need_gpu, dev, host    # noqa: F401  (_need_gpu: autouse)
import backbone_cases as CASES
from backbone_refs import RESNET50 as REF

F32_ATOL = 3e-5                              # tests/test_gpu_ops.py test_conv1x1_pipelined_kernel
HALF_RTOL, HALF_ATOL = 2.0 ** -10, 1e-4      # tests/test_gpu_f16_storage.py


@pytest.fixture(params=["on", "off"])
def fusion(request):
    from masklab_hip import ops
    before = ops.PROJECTION_FUSION
    ops.set_projection_fusion(request.param)
    yield request.param
    ops.set_projection_fusion(before)


# ------------------------------------------------------------------ the dual kernel
def _dual_problem(B, H, W, Ka, Kx, N, s, dtype, seed):
    """a, x (the pixels a strided unit must not read = 1e3), the two folded 1x1 kernels [1,1,K,N] and their biases."""
    rng = np.random.default_rng(seed)
    f = lambda *sh, sd=1.0: (rng.standard_normal(sh) * sd).astype(np.float32)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x = f(B, H, W, Kx)
    if s == 2:
        x[:, 1::2] = 1e3
        x[:, :, 1::2] = 1e3
    return dict(a=f(B, Ho, Wo, Ka).astype(dtype), x=x.astype(dtype), ka=f(1, 1, Ka, N, sd=1.0 / np.sqrt(Ka)), ba=f(N),
                kx=f(1, 1, Kx, N, sd=1.0 / np.sqrt(Kx)), bx=f(N), s=s)


def _dual_ref(p):
    """fp64 from the very inputs the kernel gets: the half ones and half-rounded weights for a half problem."""
    half = p["a"].dtype == np.float16
    w = (lambda k: k[0, 0].astype(np.float16).astype(np.float64)) if half else (lambda k: k[0, 0].astype(np.float64))
    s = p["s"]
    y = p["a"].astype(np.float64) @ w(p["ka"])
    y += p["x"][:, ::s, ::s].astype(np.float64) @ w(p["kx"])
    y += (p["ba"].astype(np.float64) + p["bx"].astype(np.float64)).astype(np.float32)    # the packed bias is one fp32 sum
    return np.maximum(y, 0.0, out=y)


def _pack(p):
    from masklab_hip import ops
    return ops.DeviceDualConv(p["ka"], p["ba"], p["kx"], p["bx"], "cuda")


def _check(got, want, dtype):
    assert got.dtype == dtype and got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"\n[conv1x1_dual] {np.dtype(dtype).name} {want.shape}: max|err| {err:.3g}, max|ref| {float(want.max()):.3g}")
    if dtype == np.float16:
        ref = want.astype(np.float16).astype(np.float32)
        np.testing.assert_allclose(got.astype(np.float32), ref, rtol=HALF_RTOL, atol=HALF_ATOL)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=F32_ATOL)


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("B,H,W,Ka,Kx,N,s", [
    (1, 9, 13, 64, 64, 256, 1),          # one partial pixel panel
    (2, 15, 21, 128, 256, 512, 2),       # odd map, Ho x Wo = 8 x 11, a panel spanning two images
    (3, 7, 9, 512, 1024, 2048, 2),
    (1, 64, 64, 64, 64, 256, 1),         # many panels
])
def test_dual_kernel_against_fp64(B, H, W, Ka, Kx, N, s, dtype):
    from masklab_hip import ops
    p = _dual_problem(B, H, W, Ka, Kx, N, s, dtype, seed=H * 1000 + N)
    d = _pack(p)
    ops.PROFILE = []
    try:
        out = ops.conv1x1_dual(dev(p["a"]), dev(p["x"]), d, s)
        recs, ops.PROFILE = ops.PROFILE, None
    finally:
        ops.PROFILE = None
    assert [r["kernel"] for r in recs] == ["conv1x1_dual_h" if dtype == np.float16 else "conv1x1_dual"]   # no fall-back
    _check(host(out), _dual_ref(p), dtype)
    # repeated launches: the same bits; image k of the batch == image k alone
    assert torch.equal(out, ops.conv1x1_dual(dev(p["a"]), dev(p["x"]), d, s))
    for k in range(B):
        assert torch.equal(out[k:k + 1], ops.conv1x1_dual(dev(p["a"][k:k + 1]), dev(p["x"][k:k + 1]), d, s)), k


@pytest.mark.parametrize("dtype,Ka,Kx", [(np.float32, 48, 128), (np.float16, 128, 96)], ids=["f32", "f16"])
def test_k_off_the_chunk_is_refused_and_ops_falls_back(dtype, Ka, Kx):
    """fp32: Ka = 48 is no multiple of 32 floats.  Half: Kx = 96 is no multiple of 64 halves (a half Ka off the chunk has
    no two-launch form either: the half conv with a residual is the persistent kernel's, in 64-deep chunks)."""
    from masklab_hip import _lib, ops
    p = _dual_problem(2, 15, 21, Ka, Kx, 256, 2, dtype, seed=Ka)
    d = _pack(p)
    a, x = dev(p["a"]), dev(p["x"])
    out = torch.empty((2, 8, 11, 256), dtype=a.dtype, device="cuda")
    lib = _lib.load()
    half = dtype == np.float16
    fn, w = (lib.ml_conv1x1_dual_f16, d.wgt_h) if half else (lib.ml_conv1x1_dual_f32, d.wgt)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert fn(vp(a), vp(x), vp(w), vp(d.bias), vp(out), 2, 15, 21, Ka, Kx, 256, 2, None) == -1
    assert b"multiples of the K chunk" in lib.ml_last_error()
    ops.PROFILE = []
    try:
        got = ops.conv1x1_dual(a, x, d, 2)
        recs, ops.PROFILE = ops.PROFILE, None
    finally:
        ops.PROFILE = None
    kernels = [r["kernel"] for r in recs]
    assert len([k for k in kernels if k.startswith("conv")]) == 2 and not any("dual" in k for k in kernels), kernels
    if half:        # what the two launches compute: the shortcut is a half tensor, then the residual conv rounds once more
        h64 = lambda k: k[0, 0].astype(np.float16).astype(np.float64)
        sc = (p["x"][:, ::2, ::2].astype(np.float64) @ h64(p["kx"]) + p["bx"]).astype(np.float16)
        want = np.maximum(p["a"].astype(np.float64) @ h64(p["ka"]) + p["ba"] + sc, 0.0).astype(np.float16)
        np.testing.assert_allclose(host(got).astype(np.float32), want.astype(np.float32), rtol=HALF_RTOL, atol=HALF_ATOL)
    else:
        np.testing.assert_allclose(host(got), _dual_ref(p), rtol=0, atol=F32_ATOL)


def test_ops_refuses_mismatched_tensors():
    from masklab_hip import ops
    p = _dual_problem(1, 9, 13, 64, 64, 256, 1, np.float32, seed=1)
    d = _pack(p)
    with pytest.raises(ValueError):
        ops.conv1x1_dual(dev(p["a"]), dev(p["x"].astype(np.float16)), d, 1)
    with pytest.raises(ValueError):
        ops.conv1x1_dual(dev(p["a"]), dev(p["x"]), d, 2)                    # a is not the strided map's size
    with pytest.raises(ValueError):
        ops.conv1x1_dual(dev(p["a"]), dev(p["x"]), d, 3)
    with pytest.raises(RuntimeError):
        ops.conv1x1_dual(torch.from_numpy(p["a"]), dev(p["x"]), d, 1)       # a host tensor


# ------------------------------------------------------------------ backbone taps
_TAPS = {}


def _taps_fixture(shape, outputs):
    """(backbone with weights loaded, images, restated taps) -- made once per shape and shared, unchanged."""
    if shape not in _TAPS:
        bb, w = CASES.load_backbone("resnet50", outputs, seed=shape[1])
        images = np.random.default_rng(shape[2]).integers(0, 256, shape, dtype=np.uint8)
        names, want = REF.backbone_forward(images.astype(np.float32), w, "resnet50", outputs)
        assert names == bb.output_names
        _TAPS[shape] = (bb, images, names, want)
    return _TAPS[shape]


@pytest.mark.parametrize("shape,outputs", [
    ((1, 540, 960, 3), ("C3", "C4", "C5", "P6", "P7")),              # the serving size: 68x120 .. 9x15
    ((2, 200, 328, 3), ("C1", "C2", "C3", "C4", "C5", "P6", "P7")),  # odd maps: 50x82, 25x41, 13x21, 7x11, 4x6, 2x3
])
def test_backbone_taps_match_the_restatement(shape, outputs, fusion):
    """f32 / f32x3 within the BASELINE tolerance, f16 (fp16 operands, fp32 tensors) within the SE-ResNet f16 bar; f16s
    (half tensors from the stem on, half taps) is reported, not gated.  With the fusion on, the four projection units of
    "f32" and "f16s" run on the one-GEMM kernel; "f32x3" and "f16" keep the two launches either way."""
    bb, images, names, want = _taps_fixture(shape, outputs)
    for math in ("f32", "f32x3", "f16", "f16s"):
        got, kernels = CASES.run_backbone(bb, images, math)
        dual = [k for k in kernels if "dual" in k]
        fused = fusion == "on" and math in ("f32", "f16s")
        assert dual == ([{"f32": "conv1x1_dual", "f16s": "conv1x1_dual_h"}[math]] * 4 if fused else []), (math, dual)
        CASES.check_taps(names, got, want, math, f"resnet50 taps fusion {fusion} {shape}")


# ------------------------------------------------------------------ end to end
E2E_SHAPE, E2E_SEED = (2, 128, 160, 3), 5
_E2E = {}


def _fixture():
    """(cfg, weights, images, oracle outputs, kept rows) of the DEFAULT ModelConfiguration() with an order-stable logit
    scale from the restated forward -- made once and shared, unchanged."""
    if not _E2E:
        from masklab_hip import ModelConfiguration
        cfg = ModelConfiguration()
        assert cfg.backbone.backbone_type == "resnet50"
        _, w, images = CASES.order_stable_fixture(cfg, E2E_SHAPE, E2E_SEED)
        want, internals = O.inference_forward(cfg, w, images, literal_groups=False, return_internals=True)
        assert len(internals["kept"]) > 0, "fixture produced no detections"
        _E2E.update(cfg=cfg, w=w, images=images, want=want, kept=internals["kept"])
    return _E2E


def test_end_to_end_on_the_default_configuration(monkeypatch, fusion):
    from masklab_hip import retinamasklab as R
    REF.patch(monkeypatch)
    fx = _fixture()
    cfg, images, want, kept_ref = fx["cfg"], fx["images"], fx["want"], fx["kept"]
    _, model = R.construct_masklab_networks(cfg)
    assert model.backbone_network.backbone_type == "resnet50"
    assert model.backbone_network.output_names == ['C3', 'C4', 'C5', 'P6', 'P7']
    model.load_weights(fx["w"], "cuda:0")
    CASES.check_kept_rows_device_counts_and_graph(model, images, want, kept_ref)


def test_checkpoint_to_deploy_model(tmp_path, monkeypatch):
    """An .npz keyed by the Keras names through load_masklab_inference_model_from_h5 -> DeployModel on a 272x480 frame
    (down-sampled to a 136x240 working size) against oracle.deploy_forward with the restated backbone."""
    from masklab_hip import ModelConfiguration
    REF.patch(monkeypatch)
    cfg = ModelConfiguration()
    cfg.postprocess.resolution = (136, 240)
    w = CASES.check_checkpoint_to_deploy(cfg, tmp_path / "resnet50.npz", (1, 272, 480, 3), seed=272)
    assert "res5a_branch1/kernel" in w and "bn_conv1/moving_mean" in w      # keyed by the Keras names
