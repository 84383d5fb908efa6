"""The case table of the generic conv kernel (tests/conv_cases.py) against the library's host-only planning entries: every
case's launch is planned onto the instantiation it names, the table names every row of `kGenericKernels`, and the ReLU /
ReLU6 data really reaches the clamps.  No GPU: without a device the library plans for 256 compute units, the MI355X's."""
import ctypes as C

import pytest

import conv_cases as CC


def _plan(ds, ws=None):
    """-> (rc of the checked plan, family is generic, tile rows, tile columns, K slices per problem)"""
    from masklab_hip import _lib
    lib = _lib.load()
    arr = (_lib.ConvDesc * len(ds))(*ds)
    sp = (C.c_int32 * len(ds))()
    rc = lib.ml_conv2d_launch_splits(arr, len(ds), lib.ml_conv2d_workspace_bytes() if ws is None else ws, sp)
    bm, bn = lib.ml_conv2d_launch_mtile(arr, len(ds), 1), lib.ml_conv2d_launch_ntile(arr, len(ds), 1)
    return rc, bm != 0 and bn != 0, bm, bn, list(sp)          # (the tile entries answer 0 for every other kernel family)


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.name)
def test_case_is_planned_onto_the_instantiation_it_names(case):
    from masklab_hip import _lib
    lib = _lib.load()
    ds = CC.launch_descs(case)
    assert 1 <= len(ds) <= 12
    for d in ds:                                     # explicit tiles only: never the Winograd or persistent 1x1 families
        assert d.tile == case.tile and case.tile in (1, 2, 3) and d.math == CC.MATH_CODE[case.math]
    rc, generic, bm, bn, splits = _plan(ds)
    assert rc == 0, lib.ml_last_error()
    assert generic and (bm, bn) == (case.bm, case.bn)
    n = len(CC.case_probs(case))
    assert splits[:n] == [case.splits] * n and all(s == 1 for s in splits[n:])
    assert any(p.gn for p in CC.case_probs(case)) == case.gns          # (no reporting entry tells a gns row from its twin)
    assert bool(ds[0].gn_partials) == case.gns


@pytest.mark.parametrize("case", [c for c in CC.CASES if c.filler], ids=lambda c: c.name)
def test_problems_launched_alone_run_on_narrow_tiles_with_the_k_slices_the_table_names(case):
    for prob in CC.case_probs(case):
        if not prob.alone_splits(case.math):
            continue
        rc, generic, bm, bn, splits = _plan([CC.host_desc(prob, case.math, case.tile)])
        assert rc == 0 and generic and (bm, bn) == (128, 32), (prob.name, bm, bn)
        assert splits == [prob.alone_splits(case.math)], (prob.name, splits)


def test_the_table_names_every_generic_instantiation():
    """The rows of kGenericKernels as the library itself reports them: one 1x1 problem per (math, gn_partials, tile class,
    launch size), planned with its checks on (a refusal is no row)."""
    rows = set()
    for math in CC.MATH_CODE:
        for gns in (False, True):
            for tile, cout in ((1, 128), (2, 64), (3, 32)):
                for nrows in (256, 38400, 66560, 4 * 66560):
                    d = CC.filler_desc((nrows, 64, cout), math, tile)
                    if gns:
                        d.gn_partials = 0x600000
                    rc, generic, bm, bn, _ = _plan([d])
                    if rc == 0 and generic:
                        rows.add((math, gns, bm, bn))
    named = {(c.math, c.gns, c.bm, c.bn) for c in CC.CASES}
    assert rows == named, (sorted(rows - named), sorted(named - rows))


def test_relu_and_relu6_data_reaches_the_clamps():
    """On the fp64 reference alone: at least 5 % of a ReLU6 problem's pre-activation values above 6 and 5 % below 0; at
    least 5 % of a ReLU problem's below 0."""
    seen = set()
    for case in CC.CASES:
        for prob in CC.case_probs(case):
            key = (prob, case.math in ("f16", "f16s"), CC.has_res(prob, case.math))
            if key in seen or prob.act not in ("relu", "relu6"):
                continue
            seen.add(key)
            pre, _ = CC.reference(*key)
            below, above = float((pre < 0).mean()), float((pre > 6).mean())
            assert below >= 0.05, (prob.name, below)
            if prob.act == "relu6":
                assert above >= 0.05, (prob.name, above)
    assert any(p.act == "relu6" for p, _, _ in seen)
