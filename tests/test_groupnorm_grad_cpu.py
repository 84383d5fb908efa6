"""CPU tests of GroupNormalization's backward: the closed form the kernels implement (include/masklab_hip.h) against torch
autograd over the float64 restatement of the reference layer, the index rule, the argument checks of the ops, and the
workspace size."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import groupnorm_grad_ref as R

FLAGS = [(False, False), (False, True), (True, False), (True, True)]


@pytest.mark.parametrize("name", list(R.CASES))
def test_closed_form_equals_autograd_over_the_restatement(name):
    inp = R.inputs(name)
    assert R.mask_margin(inp["x"], inp["gamma"], inp["beta"], inp["groups"]) >= R.GUARD
    assert 0.3 < (inp["x"] == 0).mean() < 0.45                      # exact zeros: the strictness of x > 0 is exercised
    for relu, input_relu in FLAGS:
        for gamma in (inp["gamma"], None):
            args = (inp["x"], inp["dy"], gamma, inp["beta"], inp["groups"], relu, input_relu)
            want = R.autograd(inp["x"], inp["dy"], np.ones_like(inp["gamma"]) if gamma is None else gamma, *args[3:])
            R.check(R.closed_form(*args), want, R.scale(*args), f"{name} relu={relu} input_relu={input_relu} "
                    f"gamma={'None' if gamma is None else 'given'}", bar=1e-10)


def test_mask_margin_holds_for_the_seeds_the_gpu_test_could_use():
    for name in R.CASES:
        for seed in range(3):
            inp = R.inputs(name, seed)
            assert R.mask_margin(inp["x"], inp["gamma"], inp["beta"], inp["groups"]) >= R.GUARD, (name, seed)


def test_index_rule_is_the_chunk_not_the_channel_group():
    """Case B: chunks of 200 values start mid-row (200 mod 32 = 8).  The reference's dgamma differs from the dgamma of group
    norm proper (what torch.nn.functional.group_norm computes: channels grouped, gamma[c]) on the same tensors."""
    inp = R.inputs("B")
    N, H, W, C, G = R.CASES["B"]
    _, dgamma, dbeta = R.closed_form(inp["x"], inp["dy"], inp["gamma"], inp["beta"], G)
    # group norm proper, by hand: channel c belongs to group c // (C/G), statistics over (H, W, C/G), gamma[c] / beta[c]
    xg = inp["x"].astype(np.float64).reshape(N, H * W, G, C // G)
    xhat = (xg - xg.mean(axis=(1, 3), keepdims=True)) / np.sqrt(xg.var(axis=(1, 3), keepdims=True) + R.EPS)
    dyc = inp["dy"].astype(np.float64).reshape(N, H * W, C)
    proper_dgamma, proper_dbeta = (dyc * xhat.reshape(N, H * W, C)).sum(axis=(0, 1)), dyc.sum(axis=(0, 1))
    assert np.abs(proper_dgamma - dgamma).max() > 0.1 * np.abs(dgamma).max()
    # beta[j] is met by channels c with c mod 8 = j mod 8 of chunk j // 8, not by channel j alone
    assert np.abs(proper_dbeta - dbeta).max() > 0.1 * np.abs(dbeta).max()
    # and the rule itself, spelled out for one index: j = 9 collects chunk 1, positions i with (200 + i) mod 32 mod 8 = 1
    d = inp["dy"].astype(np.float64).reshape(N, G, -1)
    i = np.arange(200)
    assert np.isclose(dbeta[9], d[:, 1, ((200 + i) % 32) % 8 == 1].sum(), rtol=1e-12)


def test_argument_checks_raise_on_the_host():
    from masklab_hip import ops
    x, dy = torch.zeros(2, 3, 5, 8), torch.zeros(2, 3, 5, 8)
    gamma, beta = torch.ones(8), torch.zeros(8)
    ok = dict(x=x, dy=dy, gamma=gamma, beta=beta, groups=4)
    for bad, err in ((dict(dy=torch.zeros(2, 3, 5, 4)), ValueError), (dict(groups=3), ValueError), (dict(groups=16), ValueError),
                     (dict(x=x.half()), TypeError), (dict(dy=dy.half()), TypeError), (dict(gamma=torch.ones(4)), ValueError),
                     (dict(beta=beta.double()), ValueError), (dict(stats=torch.zeros(8, 2)), ValueError),
                     (dict(stats=torch.zeros(4, 2, dtype=torch.float64)), ValueError), (dict(out=torch.zeros(2, 3, 5, 4)), ValueError),
                     (dict(), RuntimeError)):                          # all shapes right, but host tensors: no CPU fallback
        with pytest.raises(err):
            ops.groupnorm_chunk_grad(**{**ok, **bad})
        with pytest.raises(err):
            ops.groupnorm_chunk_grad_multi([{**ok, **bad}])
    assert ops.groupnorm_chunk_grad_multi([]) == []
    with pytest.raises(ValueError):
        ops.groupnorm_chunk_stats(x, 3)
    with pytest.raises(ValueError):
        ops.groupnorm_chunk_stats(x.half(), 4)
    with pytest.raises(RuntimeError):
        ops.groupnorm_chunk_stats(x, 4)


def test_grad_workspace_holds_the_partial_sums_of_every_block():
    from masklab_hip import _lib
    lib = _lib.load()
    assert lib.ml_groupnorm_grad_workspace_bytes(8, 16, 256) >= 8 * 64 * 2 * (16 + 256) * 8


def test_forward_refuses_more_chunks_than_a_grid_has_blocks():
    """N*G >= 2^31 chunks would wrap the int block counts: refused on the host, before any launch, by both forward entries."""
    from masklab_hip import _lib
    lib = _lib.load()
    p = lambda k: ctypes.c_void_p(4096 * k)                                  # aligned, never dereferenced
    N, G = 1 << 16, 1 << 15
    assert lib.ml_groupnorm_chunk_f32(p(1), p(2), None, None, N, G, G, G, 1e-5, 0, G, 0, p(3), None) != 0
    assert b"N*G too large" in lib.ml_last_error(), lib.ml_last_error()
    d = (_lib.GnDesc * 1)()
    d[0].x, d[0].y, d[0].HWC, d[0].N, d[0].C, d[0].G, d[0].out_cstride = 4096, 8192, G, N, G, G, G
    assert lib.ml_groupnorm_multi_f32(d, 1, p(3), 1 << 20, None) != 0
    assert b"N*G too large" in lib.ml_last_error(), lib.ml_last_error()
