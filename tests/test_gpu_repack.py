"""GPU tests of the re-pack (csrc/repack.hip, ops.repack_weights, DeviceConv.bind_master): master weights on the device ->
every packed form, in place, in one launch.  Every form must equal, bit for bit, the host function that defines it
(tests/repack_cases.py); the destinations are filled with 0xFF bytes first, so a result that leans on old contents shows.

Weights of the bit-equality cases are integers times 2^-20 (|w| < 8, with exact zeros and -0.0): every fp64 partial sum of
G g G^T is then exact, so the Winograd forms are the host's bits whatever order the device adds in."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_memory as D
import repack_cases as RC
from masklab_hip import ops, packing

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _poison(tensors):
    for t in tensors.values():
        D.fill_bytes(t, D.POISON)


def _check(tensors, ptrs, want, what):
    assert set(tensors) == set(want), (what, sorted(tensors), sorted(want))
    assert {k: t.data_ptr() for k, t in tensors.items()} == ptrs, f"{what}: a form moved"
    got = RC.to_host(tensors)
    for k in sorted(want):
        D.assert_same_bits(got[k].reshape(-1), np.ascontiguousarray(want[k]).reshape(-1), f"{what}: {k}")


def _stepped_conv(dev, name, seed, weights=RC.exact_weights):
    """The case's DeviceConv bound to masters that were stepped to new weights; its forms poisoned.
    -> (dc, tensors, their addresses, the host's forms of the stepped weights, the stepped kernel)"""
    rng = np.random.default_rng(seed)
    k0, b0 = RC.conv_case(name, rng)
    k1, b1 = RC.conv_case(name, rng, weights)
    dc, mk, mb = RC.bound_conv(k0, b0, dev)
    mk.copy_(torch.from_numpy(k1))
    if mb is not None:
        mb.copy_(torch.from_numpy(b1))
    tensors = RC.device_tensors(dc)
    ptrs = {k: t.data_ptr() for k, t in tensors.items()}
    _poison(tensors)
    return dc, tensors, ptrs, RC.host_forms(k1, b1), k1


def _slices(dev, seed):
    n, nf, cout = RC.SLICES
    rng = np.random.default_rng(seed)
    k0, k1 = RC.exact_weights(rng, (1, 1, n * nf, cout)), RC.exact_weights(rng, (1, 1, n * nf, cout))
    master = torch.from_numpy(k0).to(dev)
    made = []
    for i in range(n):
        dc = RC.materialise(ops.DeviceConv(packing.pack_dense(np.ascontiguousarray(k0[:, :, i * nf:(i + 1) * nf, :])), dev))
        dc.bind_master(master, cin_slice=(i * nf, (i + 1) * nf))
        tensors = RC.device_tensors(dc)
        made.append((dc, tensors, {k: t.data_ptr() for k, t in tensors.items()},
                     RC.host_forms(np.ascontiguousarray(k1[:, :, i * nf:(i + 1) * nf, :]))))
        _poison(tensors)
    master.copy_(torch.from_numpy(k1))
    return made


def _deconv(dev, seed):
    cout, cin = RC.DECONV
    rng = np.random.default_rng(seed)
    (k0, b0), (k1, b1) = [(RC.exact_weights(rng, (2, 2, cout, cin)), RC.exact_weights(rng, (cout,))) for _ in range(2)]
    mk, mb = torch.from_numpy(k0).to(dev), torch.from_numpy(b0).to(dev)
    d2 = RC.materialise(ops.DeviceConv(packing.pack_transpose2x2(k0, b0), dev), dgrad=False)
    d1 = RC.materialise(ops.DeviceConv(packing.pack_dense(packing.transpose2x2_as_1x1(k0), np.tile(b0, 4)), dev))
    d2.bind_master(mk, mb, layout="deconv")
    d1.bind_master(mk, mb, layout="deconv", bias_reps=4)
    mk.copy_(torch.from_numpy(k1))
    mb.copy_(torch.from_numpy(b1))
    made = []
    for dc, want in ((d2, RC.side_forms(packing.pack_transpose2x2(k1, b1))),
                     (d1, RC.host_forms(packing.transpose2x2_as_1x1(k1), np.tile(b1, 4)))):
        tensors = RC.device_tensors(dc)
        made.append((dc, tensors, {k: t.data_ptr() for k, t in tensors.items()}, want))
        _poison(tensors)
    return made


def _tables(dev, seed):
    """-> [(job, tensors, addresses, host forms)] of the fused mask tail's table, with a bias and without"""
    rng = np.random.default_rng(seed)
    made = []
    for (cmid, ncls), has_bias in zip(RC.TABLES, (True, False)):
        k = RC.exact_weights(rng, (1, 1, cmid, ncls))
        b = RC.exact_weights(rng, (ncls,)) if has_bias else None
        table, bo, cp = packing.pack_out1x1_table(k, b)
        tensors = {"table": torch.empty(table.shape, dtype=torch.float32, device=dev),
                   "bias": torch.empty((cp,), dtype=torch.float32, device=dev)}
        _poison(tensors)
        job = ops.repack_table_job(torch.from_numpy(k).to(dev), None if b is None else torch.from_numpy(b).to(dev),
                                   tensors["table"], tensors["bias"])
        made.append((job, tensors, {k_: t.data_ptr() for k_, t in tensors.items()}, {"table": table, "bias": bo}))
    return made


@pytest.mark.parametrize("name", list(RC.CONV_CASES))
def test_conv_forms_are_the_hosts_bits_on_poisoned_destinations(dev, name):
    dc, tensors, ptrs, want, _ = _stepped_conv(dev, name, seed=11)
    jobs = dc.repack_jobs()
    assert len(jobs) == 1
    ops.repack_weights(jobs)
    _check(tensors, ptrs, want, name)
    with pytest.raises(RuntimeError, match="follows master weights"):
        packing.unpack_dense(dc.p)


def test_cin_slices_of_one_master(dev):
    made = _slices(dev, seed=12)
    ops.repack_weights([j for dc, *_ in made for j in dc.repack_jobs()])
    for i, (dc, tensors, ptrs, want) in enumerate(made):
        _check(tensors, ptrs, want, f"slice {i}")


def test_transposed_conv_and_its_1x1_twin(dev):
    made = _deconv(dev, seed=13)
    ops.repack_weights([j for dc, *_ in made for j in dc.repack_jobs()])
    for (dc, tensors, ptrs, want), what in zip(made, ("dev", "dev1x1")):
        _check(tensors, ptrs, want, what)


def test_mask_tail_tables(dev):
    made = _tables(dev, seed=14)
    ops.repack_weights([job for job, *_ in made])
    for (job, tensors, ptrs, want), shape in zip(made, RC.TABLES):
        _check(tensors, ptrs, want, f"table {shape}")


def test_all_cases_in_one_call_give_the_bits_of_one_call_each(dev):
    """One launch for everything: conv cases, slices, the transposed conv and the tables.  Each single call was held to the
    host's bits above, and so is the joint call: the bits of one call each."""
    convs = [_stepped_conv(dev, name, seed=11)[:4] for name in RC.CONV_CASES]
    rest = _slices(dev, seed=12) + _deconv(dev, seed=13)
    tables = _tables(dev, seed=14)
    jobs = [j for dc, *_ in convs + rest for j in dc.repack_jobs()] + [job for job, *_ in tables]
    table = ops.RepackTable()
    ops.repack_weights(jobs, table)
    assert table.n == len(jobs) and table.uploads == 1
    for i, (_, tensors, ptrs, want) in enumerate(convs + rest + tables):
        _check(tensors, ptrs, want, f"joint job {i}")
    # the same jobs again: the table is not uploaded twice, and the bits stay
    for _, tensors, _, _ in convs + rest + tables:
        _poison(tensors)
    ops.repack_weights(jobs, table)
    assert table.uploads == 1
    for i, (_, tensors, ptrs, want) in enumerate(convs + rest + tables):
        _check(tensors, ptrs, want, f"joint job {i}, second call")


def _ulps_apart(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


def _fp64_sum_is_exact(kernel):
    """bool [cout, cin, 16]: the elements of U = G g G^T all of whose fp64 partial sums are exact in ANY order: every term is a
    multiple of 2^low and the sum of the terms' magnitudes is below 2^(low + 53).  Exact integer arithmetic on the weights
    scaled by 2^56 (they are multiples of 2^-53 below 2^11; G's entries are multiples of 1/2)."""
    kh, kw, cin, cout = kernel.shape
    g = np.transpose(kernel, (3, 2, 0, 1)).astype(np.float64)                  # [n][c][3][3]
    G2 = (2 * packing.WINO_G).astype(np.int64)                                 # integers
    ints = np.vectorize(lambda v: int(v * 2.0 ** 54), otypes=[object])(g)      # exact: v * 2^54 is an integer below 2^65
    exact = np.zeros((cout, cin, 16), bool)
    for a in range(4):
        for b in range(4):
            terms = [ints[:, :, i, j] * (int(G2[a, i]) * int(G2[b, j])) for i in range(3) for j in range(3)
                     if G2[a, i] and G2[b, j]]
            for n in range(cout):
                for c in range(cin):
                    ts = [int(t[n, c]) for t in terms if t[n, c] != 0]
                    if not ts:
                        exact[n, c, 4 * a + b] = True
                        continue
                    low = min((t & -t).bit_length() - 1 for t in ts)
                    exact[n, c, 4 * a + b] = sum(abs(t) for t in ts).bit_length() - low <= 53
    return exact


def test_winograd_fp64_sum_on_wide_range_weights(dev):
    """`ragged` with magnitudes 2^-30 ... 2^10: the device's U is within 1 fp32 ulp of pack_winograd's everywhere, and its bits
    wherever the fp64 sum is exact in any order (counted: there must be such elements)."""
    dc, tensors, ptrs, want, kernel = _stepped_conv(dev, "ragged", seed=21, weights=RC.wide_range_weights)
    ops.repack_weights(dc.repack_jobs())
    got = RC.to_host(tensors)
    p = packing.pack_dense(kernel)
    exact = np.zeros((p.n_pad, p.span_pad, 16), bool)
    exact[:36, :40] = _fp64_sum_is_exact(kernel)
    exact[36:], exact[:, 40:] = True, True
    layout = exact.reshape(p.n_pad // 32, 32, p.span_pad // 8, 8, 16).transpose(0, 2, 3, 1, 4)
    layout = np.concatenate([layout, np.ones((4 - layout.shape[0],) + layout.shape[1:], bool)])
    real = exact[:36, :40].sum()
    print(f"ragged, wide-range weights: {real} of {36 * 40 * 16} real elements have an exact fp64 sum")
    assert 0 < real < 36 * 40 * 16
    for k in ("wino", "tr.wino"):
        apart = _ulps_apart(got[k], want[k])
        print(f"{k}: max {apart.max():.3f} ulp apart, {int((got[k] != want[k]).sum())} of {got[k].size} elements differ")
        assert apart.max() <= 1.0, k
    assert np.array_equal(got["wino"][layout].view(np.uint32), want["wino"][layout].view(np.uint32))
    # the transposed side: the same criterion on the kernel the data gradient convolves with (its pad channel is all zeros)
    kt = packing.transposed_kernel(kernel)                                     # [3,3,cp = 36,cout' = 40]
    pt = packing.pack_dense(kt)
    exact_t = np.ones((pt.n_pad, pt.span_pad, 16), bool)
    exact_t[:40, :36] = _fp64_sum_is_exact(kt)
    layout_t = exact_t.reshape(pt.n_pad // 32, 32, pt.span_pad // 8, 8, 16).transpose(0, 2, 3, 1, 4)
    layout_t = np.concatenate([layout_t, np.ones((4 - layout_t.shape[0],) + layout_t.shape[1:], bool)])
    assert 0 < exact_t[:40, :36].sum() < 40 * 36 * 16
    assert np.array_equal(got["tr.wino"][layout_t].view(np.uint32), want["tr.wino"][layout_t].view(np.uint32))
    for k in sorted(set(want) - {"wino", "tr.wino"}):                          # everything else is still the host's bits
        D.assert_same_bits(got[k].reshape(-1), np.ascontiguousarray(want[k]).reshape(-1), k)


def test_split_and_half_forms_among_subnormal_halves(dev):
    dc, tensors, ptrs, want, _ = _stepped_conv(dev, "ragged", seed=22, weights=RC.small_weights)
    ops.repack_weights(dc.repack_jobs())
    got = RC.to_host(tensors)
    halves = want["h"].view(np.uint16)
    assert ((halves & 0x7C00) == 0).sum() > (halves != 0).sum() // 2, "the case must land in subnormal halves"
    for k in ("x3", "h", "tr.x3", "tr.h", "wgt", "tr.wgt"):
        D.assert_same_bits(got[k].reshape(-1), np.ascontiguousarray(want[k]).reshape(-1), k)


def test_forms_first_touched_after_binding_come_from_the_stepped_master(dev):
    rng = np.random.default_rng(31)
    k0, b0 = RC.conv_case("ragged", rng)
    k1, b1 = RC.conv_case("ragged", rng)
    dc = ops.DeviceConv(packing.pack_dense(k0, b0), dev)
    mk, mb = torch.from_numpy(k0).to(dev), torch.from_numpy(b0).to(dev)
    dc.bind_master(mk, mb)
    assert [sorted(k for k in j["fwd"] if k in ("wgt", "x3", "h", "wino")) for j in dc.repack_jobs()] == [["wgt"]]
    assert dc.repack_jobs()[0]["tr"] is None
    mk.copy_(torch.from_numpy(k1))
    mb.copy_(torch.from_numpy(b1))
    with D.poisoned():                                          # the lazily made forms start as 0xFF bytes
        RC.materialise(dc)
    want = RC.host_forms(k1, b1)
    got = RC.to_host(RC.device_tensors(dc))
    for k in sorted(set(want) - {"wgt", "bias"}):               # those two were not re-packed: they still hold k0
        D.assert_same_bits(got[k].reshape(-1), np.ascontiguousarray(want[k]).reshape(-1), k)
    D.assert_same_bits(got["wgt"], packing.pack_dense(k0, b0).wgt, "wgt before its re-pack")
    ops.repack_weights(dc.repack_jobs())
    got = RC.to_host(RC.device_tensors(dc))
    assert set(got) == set(want)
    for k in sorted(want):
        D.assert_same_bits(got[k].reshape(-1), np.ascontiguousarray(want[k]).reshape(-1), k)


def test_refusals_change_nothing(dev):
    dc, tensors, ptrs, want, _ = _stepped_conv(dev, "tiny", seed=41)
    before = RC.to_host(tensors)
    job = dc.repack_jobs()[0]
    clash = dict(job, fwd=dict(job["fwd"], x3=job["fwd"]["wgt"]))
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.repack_weights([clash])
    onto_master = dict(job, fwd=None, tr=None, bias=None)
    onto_master["fwd"] = dict(n_pad=32, span_pad=32, span_pad_h=64, wgt=torch.empty(32 * 9 * 32, device=dev))
    onto_master["src"] = onto_master["fwd"]["wgt"]
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.repack_weights([onto_master])
    with pytest.raises(ValueError, match="elements"):
        ops.repack_weights([dict(job, fwd=dict(job["fwd"], n_pad=64))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.repack_weights([dict(job, src=job["src"].cpu())])
    D.assert_same_bits(RC.to_host(tensors), before, "after the refusals")
