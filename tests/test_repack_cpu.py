"""CPU tests of the re-pack's host half: ml_repack_plan's unit counts and refusals, and the bookkeeping of
DeviceConv.bind_master on packings that live on the CPU (no kernel runs here; tests/test_gpu_repack.py holds the device's bits
to the host's)."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repack_cases as RC
from masklab_hip import _lib, ops, packing


def _bound(name, seed=0, dgrad=True):
    return RC.bound_conv(*RC.conv_case(name, np.random.default_rng(seed)), "cpu", dgrad)


def test_plan_of_no_jobs_is_no_units():
    assert _lib.load().ml_repack_plan(None, 0) == 0


# tiles along n x tiles along c (+ 1 for a bias), worked out by hand from the padded extents of every form of the case:
#   tiny    forward 32 rows but a Winograd form of four blocks (4), K 32 / half 64 (2); transposed the same -> 4 x 4 + 1
#   ragged  forward 64 rows, Winograd 128 (4), K 64 (2); transposed 64 rows, Winograd 128 (4), K 64 (2) -> 4 x 4 + 1
#   priors  forward n_pad 32 -> 4 with Winograd, K 64 (2); transposed 64 rows -> 4, K 32 / half 64 (2) -> 4 x 4 + 1
#   wide    forward 256 rows (8), K 32 / half 64 (2); transposed 32 rows, Winograd 128 (4), K 160 / half 192 (6) -> 8 x 4 + 1
#   skip    forward 64 rows (2), K 64 (2); transposed 64 rows (2), K 64 (2); no bias -> 2 x 2
#   k5      forward 32 rows (1), K 32 / half 64 (2); transposed the same -> 2 x 2 + 1
UNITS = {"tiny": (4, 4, 17), "ragged": (4, 4, 17), "priors": (4, 4, 17), "wide": (8, 4, 33), "skip": (2, 2, 4), "k5": (2, 2, 5)}


@pytest.mark.parametrize("name", list(RC.CONV_CASES))
def test_plan_counts_the_units_of_a_case(name):
    dc, _, _ = _bound(name)
    units, plan = ops.repack_plan(dc.repack_jobs())
    nb, cb, total = UNITS[name]
    assert (units, plan) == (total, [(nb, cb, 0)])


def test_plan_of_several_jobs_is_a_prefix_sum_and_a_table_is_one_unit():
    convs = [_bound(name)[0] for name in ("tiny", "skip", "wide")]
    k = torch.zeros((1, 1, 128, 3))
    table = ops.repack_table_job(k, torch.zeros(3), torch.zeros((4, 16, 2, 4)), torch.zeros(4))
    jobs = convs[0].repack_jobs() + [table] + convs[1].repack_jobs() + convs[2].repack_jobs()
    units, plan = ops.repack_plan(jobs)
    assert units == 17 + 1 + 4 + 33 and [p[2] for p in plan] == [0, 17, 18, 22]
    assert ops.repack_plan([]) == (0, [])
    # only the forward dense form: the grid shrinks to that form's own extent
    dc, _, _ = _bound("tiny", dgrad=False)
    job = dc.repack_jobs()[0]
    assert ops.repack_plan([dict(job, bias=None, fwd=dict(n_pad=32, span_pad=32, span_pad_h=64, wgt=dc.wgt))])[0] == 1


def test_repack_jobs_lists_exactly_the_materialised_forms():
    rng = np.random.default_rng(3)
    k, b = RC.conv_case("ragged", rng)
    dc = ops.DeviceConv(packing.pack_dense(k, b), "cpu")
    with pytest.raises(RuntimeError, match="follows no master"):
        dc.repack_jobs()
    assert not dc.follows_master
    mk, mb = torch.from_numpy(k.copy()), torch.from_numpy(b.copy())
    dc.bind_master(mk, mb)
    assert dc.follows_master and dc.p.wgt is None and dc.p.bias is None and dc.p.n_pad == 64
    (job,) = dc.repack_jobs()
    forms = lambda side: sorted(k_ for k_ in side if k_ in ("wgt", "x3", "h", "wino"))
    assert forms(job["fwd"]) == ["wgt"] and job["tr"] is None and job["bias"] is dc.bias and job["src"] is mk
    with pytest.raises(RuntimeError, match="follows master weights"):
        packing.unpack_dense(dc.p)
    # forms made on the host BEFORE binding are listed once bound, dgrad and the forms it owns included
    dc2 = ops.DeviceConv(packing.pack_dense(k, b), "cpu")
    dc2.wgt_x3, dc2.dgrad.wgt_wino
    dc2.bind_master(mk, mb)
    (job,) = dc2.repack_jobs()
    assert forms(job["fwd"]) == ["wgt", "x3"] and forms(job["tr"]) == ["wgt", "wino"]
    assert job["tr"]["wino"] is dc2.dgrad._wgt_wino and job["tr"]["n_pad"] == 64 and job["tr"]["span_pad"] == 64
    assert dc2.dgrad.follows_master and dc2.dgrad.p.wgt is None
    with pytest.raises(RuntimeError, match="follows master weights"):
        packing.unpack_dense(dc2.dgrad.p)
    # a form first asked for after binding is made on the device: on the CPU there is none, and the stale host weights are
    # not a fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dc2.wgt_wino
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dc.dgrad
    assert dc2._wgt_wino is None and dc._dgrad is None
    with pytest.raises(ValueError, match="data-gradient packing"):
        dc2.dgrad.bind_master(mk)


def test_bind_master_refusals():
    rng = np.random.default_rng(4)
    k, b = RC.conv_case("tiny", rng)
    mk, mb = torch.from_numpy(k.copy()), torch.from_numpy(b.copy())
    stem = ops.DeviceConv(packing.pack_rowspan(RC.exact_weights(rng, (7, 7, 3, 64))), "cpu")
    with pytest.raises(NotImplementedError, match=r"row-span \(image_input\)"):
        stem.bind_master(torch.zeros((7, 7, 3, 64)))
    grouped = ops.DeviceConv(packing.pack_grouped(RC.exact_weights(rng, (3, 3, 64, 2)), 32), "cpu")
    with pytest.raises(NotImplementedError, match="grouped"):
        grouped.bind_master(torch.zeros((3, 3, 64, 2)))
    dc = ops.DeviceConv(packing.pack_dense(k, b), "cpu")
    with pytest.raises(ValueError, match="the master is a 3x3 kernel of 8 -> 8"):
        dc.bind_master(torch.zeros((3, 3, 8, 8)), mb)
    with pytest.raises(ValueError, match="has a bias"):
        dc.bind_master(mk)
    with pytest.raises(TypeError, match="float32"):
        dc.bind_master(mk.double(), mb)
    with pytest.raises(ValueError, match="cin_slice"):
        dc.bind_master(mk, mb, cin_slice=(4, 16))
    assert not dc.follows_master and dc.p.wgt is not None


def _plan_error(jobs):
    with pytest.raises(RuntimeError) as e:
        ops.repack_plan(jobs)
    return str(e.value)


def test_plan_refuses_by_name():
    dc, mk, mb = _bound("tiny")
    (job,) = dc.repack_jobs()
    fwd = job["fwd"]
    # a destination on a master, on another destination of its job, on a destination of another job
    assert re.search(r"`(wgt|kernel)` of job 0 overlaps `(wgt|kernel)` of job 0", _plan_error([_onto_master(job)]))
    assert re.search(r"`wgt(_x3)?` of job 0 overlaps `wgt(_x3)?` of job 0", _plan_error([dict(job, fwd=dict(fwd, x3=fwd["wgt"]))]))
    other, _, _ = _bound("tiny", seed=1)
    (job2,) = other.repack_jobs()
    assert re.search(r"`wgt_h` of job [01] overlaps `wgt_h` of job [01]",
                     _plan_error([job, dict(job2, fwd=dict(job2["fwd"], h=fwd["h"]))]))
    # masters may share memory: two jobs on one kernel plan fine
    third = RC.materialise(ops.DeviceConv(packing.pack_dense(mk.numpy(), mb.numpy().copy()), "cpu"))
    third.bind_master(mk, mb)
    assert ops.repack_plan([job] + third.repack_jobs())[0] == 34
    # packings that are not re-packed on the device
    assert "row-span (image_input) packing" in _plan_error([dict(job, cpp_shift=2)])
    assert "grouped packing" in _plan_error([dict(job, group_cin_step=32)])
    # more than 5 x 5 taps
    big = dict(job, src=torch.zeros((6, 6, 8, 4)), KH=6, KW=6, fwd=None, tr=None, bias=None)
    big["fwd"] = dict(n_pad=32, span_pad=32, span_pad_h=64, wgt=torch.zeros(32 * 36 * 32))
    assert "6 x 6 taps; at most 5 x 5" in _plan_error([big])
    # a Winograd form of what pack_winograd refuses
    k5, _, _ = _bound("k5")
    (j5,) = k5.repack_jobs()
    assert "winograd packing needs a dense 3x3 conv" in _plan_error(
        [dict(j5, fwd=dict(j5["fwd"], wino=torch.zeros(128 * 32 * 16)))])
    with pytest.raises(ValueError, match="winograd packing needs a dense 3x3 conv"):
        packing.pack_winograd(packing.pack_dense(np.zeros((5, 5, 4, 4), np.float32)))
    # extents that do not hold the kernel; cin % 4
    assert "n_pad 16 must be a multiple of 32 and at least 4" in _plan_error(
        [dict(job, tr=None, bias=None, fwd=dict(n_pad=16, span_pad=32, span_pad_h=64, wgt=torch.zeros(16 * 9 * 32)))])
    odd = dict(job, src=torch.zeros((3, 3, 6, 4)), C=6, s_tap=24, fwd=None, tr=None, bias=None)
    odd["fwd"] = dict(n_pad=32, span_pad=32, span_pad_h=64, wgt=torch.zeros(32 * 9 * 32))
    assert "cin % 4 == 0" in _plan_error([odd])


def _onto_master(job):
    """The job with its forward dense form written onto its own master."""
    buf = torch.zeros(32 * 9 * 32)
    return dict(job, src=buf, tr=None, bias=None, fwd=dict(n_pad=32, span_pad=32, span_pad_h=64, wgt=buf))


def test_driver_refusals_on_the_host():
    dc, mk, mb = _bound("tiny")
    (job,) = dc.repack_jobs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.repack_weights([job])
    with pytest.raises(ValueError, match="elements"):
        ops.repack_plan([dict(job, fwd=dict(job["fwd"], n_pad=64))])
    with pytest.raises(ValueError, match="does not lie inside the master"):
        ops.repack_plan([dict(job, offset=1)])
    with pytest.raises(TypeError, match="contiguous torch.float16"):
        ops.repack_plan([dict(job, fwd=dict(job["fwd"], h=job["fwd"]["wgt"]))])
    with pytest.raises(ValueError, match="kind must be"):
        ops.repack_plan([dict(job, kind="dense")])
    assert ops.repack_weights([]) is None


def test_table_job_refusals():
    k = torch.zeros((1, 1, 128, 3))
    job = ops.repack_table_job(k, None, torch.zeros((4, 16, 2, 4)), torch.zeros(4))
    assert ops.repack_plan([job]) == (1, [(0, 0, 0)])
    assert "cp = 4, the power of two >= 3" in _plan_error([dict(job, cp=8, table=torch.zeros(128 * 8), table_bias=torch.zeros(8))])
    k40 = torch.zeros((1, 1, 40, 3))
    assert "C_mid % 32 == 0" in _plan_error([dict(ops.repack_table_job(k40, None, torch.zeros(160), torch.zeros(4)))])
    with pytest.raises(ValueError, match=r"\[1,1,C_mid,ncls\]"):
        ops.repack_table_job(torch.zeros((3, 3, 32, 3)), None, None, None)


@pytest.mark.parametrize("name", list(RC.CONV_CASES))
def test_geometry_helpers_are_the_packings_geometry(name):
    """What a data-gradient packing made on the device is sized by: every non-array field of the host packings."""
    import dataclasses
    kh, kw, cin, cout, _ = RC.CONV_CASES[name]
    k = np.zeros((kh, kw, cin, cout), np.float32)
    for made, geom in ((packing.pack_dense(k), packing.dense_geometry(kh, kw, cin, cout)),
                       (packing.pack_dense_transposed(k), packing.transposed_geometry(kh, kw, cin, cout))):
        assert dataclasses.replace(made, wgt=None, bias=None) == geom
