"""Stale memory for the tests (test infrastructure, not collected: no `test_` prefix).

Every op of masklab_hip/ops.py returns `torch.empty` tensors and works in a grow-only scratch buffer (`ops.workspace`) that
nothing zeroes between launches; in service a launch finds there the bytes of an earlier launch of another shape, and in its
outputs whatever the caching allocator last held.  `poisoned()` makes that state on purpose, `interleaved()` puts a launch
of another shape between two launches of the same one.

The poison is the byte 0xFF and nothing else: NaN as fp32 / fp16 / fp64, -1 as any signed integer (the padding value the
project's own consumers already meet), the maximum as a u64 key.  A stale read then changes a result, but it can form
neither a far address nor a long loop bound -- which a large positive pattern could."""
import contextlib

import numpy as np
import torch

POISON = 0xFF


def fill_bytes(t, byte):
    """Every byte of tensor `t` = `byte` (any dtype, any device, pinned host memory included).  -> t"""
    if t.is_meta or t.layout != torch.strided or t.numel() == 0:
        return t
    try:
        (t if t.dim() else t.view(1)).view(torch.uint8).fill_(byte)
    except RuntimeError:                 # a dense tensor whose last stride is not 1 (channels_last): it owns its storage
        t.untyped_storage().fill_(byte)
    return t


@contextlib.contextmanager
def filled(byte):
    """Inside: every scratch buffer of ops.workspace() and every result of torch.empty / torch.empty_like (workspaces that
    grow inside included) starts out as `byte` repeated.  The patch is undone on exit, also after an exception."""
    from masklab_hip import ops
    for buf in list(ops._ws_cache.values()) + list(ops._ws_retired):
        fill_bytes(buf, byte)
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def empty(*args, **kwargs):
        return fill_bytes(real_empty(*args, **kwargs), byte)

    def empty_like(*args, **kwargs):
        return fill_bytes(real_empty_like(*args, **kwargs), byte)

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like


def poisoned():
    """Eager launches on stale memory: workspaces and fresh outputs hold 0xFF bytes."""
    return filled(POISON)


def zeroed():
    """The same launches on zeroed workspaces and outputs: what a poisoned result is compared with, bit for bit."""
    return filled(0x00)


def snapshot(result):
    """A launch's result (tensors, arrays, bytes, numbers in dicts / lists / tuples) copied to the host, so that a later launch
    cannot change it: tensors become NumPy arrays."""
    if isinstance(result, torch.Tensor):
        if result.is_cuda:
            torch.cuda.synchronize(result.device)
        return result.detach().cpu().numpy().copy()
    if isinstance(result, np.ndarray):
        return result.copy()
    if isinstance(result, dict):
        return {k: snapshot(v) for k, v in result.items()}
    if isinstance(result, (list, tuple)):
        return type(result)(snapshot(v) for v in result)
    return result


def interleaved(run_x, run_y):
    """X, then Y (another shape on the same workspace tags), then X again -> (first X, second X), as snapshots."""
    first = snapshot(run_x())
    snapshot(run_y())
    return first, snapshot(run_x())


def assert_same_bits(got, want, what=""):
    """Two snapshots equal bit for bit (NaNs and signed zeros included), with the path of the first difference."""
    if isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, \
            (what, getattr(got, "dtype", type(got)), getattr(got, "shape", None), want.dtype, want.shape)
        if got.tobytes() != want.tobytes():
            g = np.ascontiguousarray(got).reshape(-1).view(np.uint8).reshape(got.size, -1)
            w = np.ascontiguousarray(want).reshape(-1).view(np.uint8).reshape(want.size, -1)
            bad = np.flatnonzero((g != w).any(axis=1))
            at = np.unravel_index(int(bad[0]), want.shape) if want.ndim else ()
            raise AssertionError(f"{what}: {len(bad)} of {want.size} elements differ, first at {at}: "
                                 f"{got[at]!r} against {want[at]!r}")
    elif isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), (what, list(got), list(want))
        for k in want:
            assert_same_bits(got[k], want[k], f"{what}[{k!r}]")
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, type(want)) and len(got) == len(want), (what, len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same_bits(g, w, f"{what}[{i}]")
    else:
        assert type(got) is type(want) and got == want, (what, got, want)


def poison_elements(a):
    """bool array shaped like `a`: the elements all of whose bytes are 0xFF (NaN / -1 / the maximum)."""
    a = np.ascontiguousarray(a)
    return (a.reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize) == POISON).all(axis=1).reshape(a.shape)


def holds(a, byte):
    """True if every byte of array `a` is `byte`: a region nobody wrote."""
    return bool((np.ascontiguousarray(a).reshape(-1).view(np.uint8) == byte).all())
