"""The device entropy decoder without a device: ml_jpeg_entropy_reference_host runs the very per-thread code of the
kernels (guess, synchronise, scan, write) in CPU loops, and is held to the host decoder ml_jpeg_decode_entropy byte for
byte -- every fixture, scans across several workgroups with and without restart intervals, the slowly synchronising
flat frame, FF 00 astride a subsequence boundary, and a few thousand truncated and corrupted streams.

Two statuses mean "ask the host decoder" rather than "malformed".  ML_JPEG_ENTROPY_NOT_SYNCED (11): the states had not
settled in the fixed number of rounds; a scan inside one workgroup always settles (a workgroup runs as many rounds as it
has subsequences), so none of the small streams here may end so.  ML_JPEG_ENTROPY_ASK_HOST (10): whole bytes lie between
an MCU's last bit and a due RSTn -- the host decoder takes that marker only if its 64-bit reader happens to have read up
to it, which depends on every refill since the interval began and is not a function of any bounded part of the scan.
Only a malformed stream with restart intervals can end so (the test asserts that), and ops.decode_jpeg(entropy="device")
runs the host decoder on every non-zero status, so its answer is the host's in every case.  Otherwise the reference
entry takes a stream exactly when the host decoder does.  Measured on the 3 000 corruptions below: 1 stream the host
takes and 89 it refuses end ASK_HOST."""
import ctypes as C

import numpy as np
import pytest

import jpeg_decode_ref as D
import jpeg_entropy_streams as S
import jpeg_ref as J

from masklab_hip._lib import JPEG_ENTROPY_ASK_HOST as ASK_HOST, JPEG_ENTROPY_NOT_SYNCED as NOT_SYNCED, JPEG_ENTROPY_OK as OK

MALFORMED = range(1, 10)                                               # the host decoder refuses these for certain


@pytest.fixture(scope="module")
def cases(golden_dir):
    return D.load_cases(golden_dir)


@pytest.fixture(scope="module")
def lib():
    from masklab_hip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def geometry(lib):
    g = (C.c_int32 * 2)()
    assert lib.ml_jpeg_entropy_geometry(g) == 0
    return tuple(g)


def assert_equals_host(lib, stream, what):
    want, message = S.host_packed(lib, stream)
    assert want is not None, (what, message)
    status, got = S.reference_packed(lib, stream)
    assert status is not None and status[0] == OK, (what, status)
    assert got == want, f"{what}: packed bytes differ from the host decoder's"
    return status


def test_geometry_and_plan_size_are_within_their_bounds(lib, geometry):
    from masklab_hip import _lib
    bits, per_wg = geometry
    assert bits % 8 == 0 and 256 <= bits <= 8192 and 64 <= per_wg <= 1024
    assert 0 < lib.ml_jpeg_entropy_plan_bytes() < 16384                # the tables fit LDS many times over
    assert lib.ml_version() == _lib.ABI_VERSION


def test_every_supported_fixture_equals_the_host_decoder(lib, cases):
    names = [k for k in sorted(cases) if cases[k]["supported"]]
    assert len(names) == 19
    for name in names:
        assert_equals_host(lib, cases[name]["stream"], name)


def test_the_fast_encoder_is_the_reference_encoder(lib):
    frame = np.random.default_rng(2).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    assert S.encode(frame, 90) == J.encode(frame, 90)
    dri = S.encode(frame, 90, restart=3)
    assert dri.count(b"\xff\xd0") >= 1 and D.decode(dri).shape == (40, 56, 3)
    np.testing.assert_array_equal(D.decode(dri), D.decode(J.encode(frame, 90)))


def test_scans_across_workgroups_with_and_without_restart_intervals(lib, geometry):
    bits, per_wg = geometry
    plain, dri, subsequences = S.noise_across_workgroups(bits, per_wg)
    assert subsequences > 3 * per_wg and subsequences % per_wg != 0
    status = assert_equals_host(lib, plain, "noise across workgroups")
    assert status[3] >= 1, "no state crossed a workgroup boundary: the case does not test what it is for"
    assert sum(dri.count(bytes([0xFF, 0xD0 + m])) for m in range(8)) >= 12      # the sequence wraps past RST7
    assert_equals_host(lib, dri, "noise across workgroups, restart intervals")


def test_the_flat_frame_is_right_or_not_synced(lib):
    stream = S.flat_with_one_block()
    want, message = S.host_packed(lib, stream)
    assert want is not None, message
    status, got = S.reference_packed(lib, stream)
    print("flat frame: status", status)
    assert status[0] in (OK, NOT_SYNCED), status
    if status[0] == OK:
        assert got == want


def test_stuffing_astride_a_subsequence_boundary(lib, geometry):
    stream, k = S.stuffing_astride(geometry[0])
    assert S.straddles(stream, k, geometry[0])
    assert_equals_host(lib, stream, f"FF 00 across the boundary of subsequences {k - 1} and {k}")


def test_restart_markers_with_fill_bytes_and_at_subsequence_boundaries(lib, cases, geometry):
    good = cases["photo_150x203_restart_rows1"]["stream"]
    at = good.index(b"\xff\xd1")
    assert_equals_host(lib, good[:at] + b"\xff\xff\xff" + good[at:], "fill bytes before RST1")
    # every alignment of a marker against the subsequence grid: a COM segment cannot move the scan's own grid, so the
    # first interval grows instead (fill bytes in front of RST0 shift all later markers)
    first = good.index(b"\xff\xd0")
    for shift in range(0, 12):
        assert_equals_host(lib, good[:first] + b"\xff" * shift + good[first:], f"{shift} fill bytes before RST0")


def test_truncated_and_corrupted_streams_are_taken_exactly_when_the_host_takes_them(lib, cases):
    names = [k for k in sorted(cases) if cases[k]["supported"] and len(cases[k]["stream"]) < 20000]
    rng = np.random.default_rng(5)
    seen = {"both take": 0, "both refuse": 0, "ask host, host takes": 0, "ask host, host refuses": 0, "not taken": 0}
    for it in range(3000):
        stream = S.corrupted(cases[names[it % len(names)]]["stream"], rng)
        info = (C.c_int32 * 4)()
        if lib.ml_jpeg_decode_info(stream, len(stream), info) != 0:
            seen["not taken"] += 1
            continue
        want, message = S.host_packed(lib, stream)
        status, got = S.reference_packed(lib, stream)
        what = (it, names[it % len(names)], status, message)
        if status is None:                                             # no plan: a table is missing, the header is cut ...
            assert want is None, what
            seen["both refuse"] += 1
        elif status[0] == OK:
            assert want is not None, what
            assert got == want, what
            seen["both take"] += 1
        elif status[0] in MALFORMED:
            assert want is None, what
            seen["both refuse"] += 1
        else:
            assert status[0] == ASK_HOST and b"\xff\xdd\x00\x04" in stream, what   # (NOT_SYNCED: one workgroup always settles)
            seen["ask host, host takes" if want is not None else "ask host, host refuses"] += 1
    print(seen)
    assert seen["both take"] > 500 and seen["both refuse"] > 1000


def test_the_malformed_set_covers_every_class(lib, cases):
    items = S.malformed_set(lib, cases)
    assert 14 <= len(items) <= 30
    for label, stream, message in items:
        status, got = S.reference_packed(lib, stream)
        assert status is None or status[0] != OK, (label, status)
    assert {label.split(":")[0] for label, _, _ in items} == set(S.MALFORMED_CLASSES)


def test_a_plan_of_another_file_and_a_small_capacity_are_refused(lib, cases):
    a, b = cases["photo_150x203_q95"]["stream"], cases["photo_150x203_optimize"]["stream"]
    plan = S.aligned(lib.ml_jpeg_entropy_plan_bytes())
    assert lib.ml_jpeg_entropy_plan(a, len(a), C.c_void_p(plan.ctypes.data)) == 0
    cap = lib.ml_jpeg_decode_packed_bytes(b, len(b))
    offsets = (C.c_int64 * 2)(0, len(b))
    ws, buf = S.aligned(lib.ml_jpeg_entropy_workspace_bytes(offsets, 1)), S.aligned(cap)
    status = (C.c_int32 * 4)()
    args = (C.c_void_p(plan.ctypes.data), C.c_void_p(buf.ctypes.data))
    assert lib.ml_jpeg_entropy_reference_host(b, len(b), args[0], args[1], cap, status, C.c_void_p(ws.ctypes.data)) < 0
    assert b"plan" in lib.ml_last_error()
    offsets = (C.c_int64 * 2)(0, len(a))
    ws = S.aligned(lib.ml_jpeg_entropy_workspace_bytes(offsets, 1))
    assert lib.ml_jpeg_entropy_reference_host(a, len(a), args[0], args[1], 224 + 64, status, C.c_void_p(ws.ctypes.data)) < 0
    bad = (C.c_int64 * 2)(0, 0)
    assert lib.ml_jpeg_entropy_workspace_bytes(bad, 1) < 0 and lib.ml_jpeg_entropy_workspace_bytes(offsets, 33) < 0


def test_the_option_is_validated_without_a_device():
    from masklab_hip import ops
    from masklab_hip.layers import DecodeImageContent
    assert ops.JPEG_ENTROPY == ("host", "device") and ops.JPEG_ENTROPY_DEFAULT in ops.JPEG_ENTROPY
    with pytest.raises(ValueError, match="entropy must be one of"):
        ops.decode_jpeg(b"\xff\xd8", "cuda:0", entropy="gpu")
    with pytest.raises(ValueError, match="entropy must be one of"):
        DecodeImageContent(device="cuda:0", entropy="gpu")
    assert DecodeImageContent(device="cuda:0", entropy="device").get_config()["entropy"] == "device"
    assert DecodeImageContent().get_config()["entropy"] is None
    import inspect
    from masklab_hip import serving
    assert inspect.signature(serving.ContentServingModel.__init__).parameters["entropy"].default is None
    assert isinstance(serving.ContentServingModel.entropy, property)
