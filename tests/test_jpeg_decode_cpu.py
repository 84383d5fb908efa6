"""The JPEG request decoder without a device: the NumPy reference (tests/jpeg_decode_ref.py) against the pixels Pillow
decoded (tests/golden/jpeg_decode), the library's host side -- classification, the entropy decoder and its packed form,
malformed input -- and the per-thread code of the two kernels run in CPU loops (ml_jpeg_decode_reference_host)."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

import jpeg_decode_ref as D
import jpeg_ref as J

MODES = {"gray": D.GRAY, "444": D.S444, "420": D.S420}


@pytest.fixture(scope="module")
def cases(golden_dir):
    return D.load_cases(golden_dir)


@pytest.fixture(scope="module")
def lib():
    from masklab_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.load()


def aligned(nbytes, fill=0):
    """uint8 [nbytes] whose first byte is 16-byte aligned."""
    raw = np.full(nbytes + 16, fill, np.uint8)
    off = -raw.ctypes.data % 16
    return raw[off:off + nbytes]


def info(lib, data):
    out = (C.c_int32 * 4)()
    return lib.ml_jpeg_decode_info(data, len(data), out), tuple(out)


def entropy(lib, data, guard=64):
    """-> (status or bytes written, packed uint8 [capacity], error text); the bytes past the capacity must stay 0xA5."""
    cap = lib.ml_jpeg_decode_packed_bytes(data, len(data))
    if cap < 0:
        return cap, None, lib.ml_last_error().decode()
    buf = aligned(cap + guard, 0xA5)
    n = lib.ml_jpeg_decode_entropy(data, len(data), C.c_void_p(buf.ctypes.data), cap)
    assert (buf[cap:] == 0xA5).all(), "wrote past the capacity"
    assert n <= cap
    return n, buf[:cap], lib.ml_last_error().decode()


def host_pixels(lib, data):
    """The kernels' per-thread code in CPU loops -> uint8 [H,W,3]."""
    rc, (H, W, mode, _) = info(lib, data)
    assert rc == 0, lib.ml_last_error()
    n, packed, err = entropy(lib, data)
    assert n > 0, err
    ws = aligned(lib.ml_jpeg_decode_workspace_bytes(1, H, W, mode))
    out = aligned(H * W * 3)
    offsets = (C.c_int64 * 2)(0, (n + 15) // 16 * 16)
    rc = lib.ml_jpeg_decode_reference_host(C.c_void_p(packed.ctypes.data), offsets, 1, H, W, mode, C.c_void_p(out.ctypes.data),
                                           C.c_void_p(ws.ctypes.data))
    assert rc == 0, lib.ml_last_error()
    return out.reshape(H, W, 3)


def assert_same_pixels(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        pytest.fail(f"{what}: {len(bad)} bytes differ, first at (y, x, channel) = {tuple(bad[0])}")


# ----------------------------------------------------------------------------- the reference against the fixtures
def test_the_fixture_set_is_the_one_the_decoder_is_held_to(cases):
    supported = {k for k, c in cases.items() if c["supported"]}
    assert len(supported) == 19 and {k for k in cases if not cases[k]["supported"]} == {"photo_150x203_progressive",
                                                                                        "photo_150x203_422"}
    assert {cases[k]["mode"] for k in supported} == {"420", "444", "gray"}
    for k in supported:
        assert cases[k]["pixels"].dtype == np.uint8 and cases[k]["pixels"].ndim == 3


def test_reference_reproduces_every_committed_pixel_array(cases):
    for name, c in sorted(cases.items()):
        if c["supported"]:
            parsed = D.parse(c["stream"])
            assert parsed["mode"] == MODES[c["mode"]], name
            assert_same_pixels(D.reconstruct(parsed), c["pixels"], name)
        else:
            with pytest.raises(D.Unsupported):
                D.parse(c["stream"])


def test_reference_matches_live_pillow(cases):
    Image = pytest.importorskip("PIL.Image")
    for name, c in sorted(cases.items()):
        if c["supported"]:
            with Image.open(io.BytesIO(c["stream"])) as im:
                assert_same_pixels(D.decode(c["stream"]), np.asarray(im.convert("RGB")), name)


def test_reference_restart_parser_is_strict(cases):
    good = cases["photo_150x203_restart_blocks5"]["stream"]
    at = good.index(b"\xff\xd1")
    with pytest.raises(J.JpegError, match="RSTn"):
        D.parse(good[:at] + b"\xff\xd2" + good[at + 2:])


# ----------------------------------------------------------------------------- the C ABI
def test_mode_codes_are_the_reference_decoders(lib):
    from masklab_hip import _lib
    assert lib.ml_version() == _lib.ABI_VERSION == 7
    assert (_lib.JPEG_GRAY, _lib.JPEG_444, _lib.JPEG_420) == (D.GRAY, D.S444, D.S420)


def test_device_entry_point_validates_its_arguments(lib):
    """Every precondition is checked before anything reaches a device."""
    H, W, mode = 32, 48, D.S420
    ws_bytes = lib.ml_jpeg_decode_workspace_bytes(1, H, W, mode)
    assert ws_bytes == 32 * 48 + 2 * 16 * 24
    least = 224 + 4 * (36 + 1) + 4 * 36
    packed, out, ws = 0x100000, 0x200000, 0x300000

    def call(packed=packed, offsets=(0, 4096), B=1, H=H, W=W, mode=mode, out=out, workspace=ws):
        offs = (C.c_int64 * len(offsets))(*offsets) if offsets is not None else None
        return lib.ml_jpeg_decode_u8(packed, offs, B, H, W, mode, out, workspace, None)

    def err():
        return lib.ml_last_error()

    for kw in (dict(packed=None), dict(offsets=None), dict(out=None), dict(workspace=None)):
        assert call(**kw) == -1 and b"null pointer" in err(), kw
    for kw in (dict(B=0), dict(B=33), dict(H=0), dict(W=-3), dict(H=16385)):
        assert call(**kw) == -1 and b"bad dims" in err(), kw
    assert call(mode=3) == -1 and b"bad mode" in err()
    assert call(B=3, H=16384, W=16384, offsets=(0, 1 << 27, 2 << 27, 3 << 27)) == -1 and b"below 2^31 bytes" in err()
    assert call(packed=packed + 8) == -1 and b"16-byte aligned" in err()
    assert call(workspace=ws + 4) == -1 and b"16-byte aligned" in err()
    assert call(out=out + 2) == -1 and b"4-byte aligned" in err()
    for offsets in ((8, 4096), (0, least - 16), (-16, 4096)):
        assert call(offsets=offsets) == -1 and b"offsets[0]" in err(), offsets
    assert call(B=2, offsets=(0, 4096, 4096)) == -1 and b"offsets[1]" in err()
    assert lib.ml_jpeg_decode_workspace_bytes(33, H, W, mode) == -1 and b"bad dims" in err()
    assert lib.ml_jpeg_decode_workspace_bytes(2, H, W, mode) == 2 * ws_bytes
    assert lib.ml_jpeg_decode_workspace_bytes(1, 37, 53, D.GRAY) == 40 * 56
    assert lib.ml_jpeg_decode_workspace_bytes(1, 37, 53, D.S444) == 3 * 40 * 56


# ----------------------------------------------------------------------------- the host entropy decoder
def test_entropy_decoder_equals_the_strict_decoder_on_420_streams(lib, cases):
    """jpeg_ref.decode takes 4:2:0 streams with the JFIF table assignment: [mcus, 6, 64] zigzag."""
    seen = 0
    for name, c in sorted(cases.items()):
        if c["mode"] != "420" or "restart" in name:
            continue
        dec = J.decode(c["stream"])
        n, packed, err = entropy(lib, c["stream"])
        assert n > 0, (name, err)
        got = D.unpack(packed[:n])
        assert (got["height"], got["width"], got["mode"]) == (dec["height"], dec["width"], D.S420)
        np.testing.assert_array_equal(got["coefficients"][:, J.ZIGZAG].reshape(-1, 6, 64), dec["coefficients"], err_msg=name)
        np.testing.assert_array_equal(got["qtables"], [dec["qtables"][0], dec["qtables"][1], dec["qtables"][1]])
        assert got["entries"] == np.count_nonzero(dec["coefficients"][:, :, 1:]) + dec["coefficients"].shape[0] * 6
        assert n % 16 == 0 and n == (224 + 4 * (got["coefficients"].shape[0] + 1) + 4 * got["entries"] + 15) // 16 * 16
        seen += 1
    assert seen >= 15


@pytest.mark.parametrize("name", ["photo_150x203_444", "photo_150x203_gray", "photo_150x203_restart_blocks5",
                                  "photo_150x203_restart_rows1", "photo_150x203_optimize"])
def test_entropy_decoder_equals_the_general_parser(lib, cases, name):
    c = cases[name]
    want = D.parse(c["stream"])
    rc, (H, W, mode, blocks) = info(lib, c["stream"])
    assert rc == 0 and (H, W, mode, blocks) == (150, 203, MODES[c["mode"]], want["coefficients"].shape[0])
    n, packed, err = entropy(lib, c["stream"])
    assert n > 0, err
    got = D.unpack(packed[:n])
    np.testing.assert_array_equal(got["coefficients"], want["coefficients"])
    for k, q in enumerate(want["qtables"]):
        np.testing.assert_array_equal(got["qtables"][k], q)
    if "restart" in name:
        assert want["restart"] == (5 if "blocks5" in name else 13)


def test_kernel_bodies_on_the_host_give_the_committed_pixels(lib, cases):
    """The __host__ __device__ bodies of both launches in CPU loops: every supported fixture, byte for byte."""
    for name, c in sorted(cases.items()):
        if c["supported"]:
            assert_same_pixels(host_pixels(lib, c["stream"]), c["pixels"], name)


def test_dc_only_blocks_are_the_constant(lib):
    """clamp(((dc * Q0 + 4) >> 3) + 128): through the shortcut (one word a block) and through both IDCT passes (the
    reference), over the DC values a stream can carry at Q0 = 1, 3 and 16."""
    for q0 in (1, 3, 16):
        q = np.full(64, 7, np.int64)
        q[0] = q0
        dc = np.array([-2047, -1024, -1020, -5, -4, -3, -1, 0, 1, 3, 4, 5, 11, 12, 1015, 1016, 1023, 2047], np.int64)
        coef = np.zeros((len(dc), 64), np.int64)
        coef[:, 0] = dc
        want = np.clip(((dc * q0 + 4) >> 3) + 128, 0, 255)
        got = D.idct_blocks(coef, q)
        assert (got == want[:, None, None]).all(), q0
    # and through the library: a flat gray frame is one DC word a block
    flat = np.full((16, 24, 3), 77, np.uint8)
    stream = J.encode(flat, 95)
    n, packed, _ = entropy(lib, stream)
    assert D.unpack(packed[:n])["entries"] == 6 * 2
    assert_same_pixels(host_pixels(lib, stream), D.decode(stream), "flat frame")


def test_the_formulas_hold_for_any_int16_coefficient(lib):
    """Beyond 16-bit intermediates libjpeg wraps; here the formulas define the result: the library's 64-bit IDCT equals
    the int64 reference on blocks of extreme coefficients (packed by hand)."""
    rng = np.random.default_rng(5)
    H, W = 16, 16                                                        # grayscale: 4 blocks
    coef = rng.integers(-32768, 32768, (4, 64))
    coef[1] = 32767
    coef[2] = -32768
    coef[3, 1:] = 0                                                      # the shortcut with an extreme DC
    q = rng.integers(1, 256, 64)
    q[0] = 255
    words, start = [], [0]
    for b in range(4):
        for i in np.flatnonzero(coef[b] | (np.arange(64) == 0)):
            words.append(int(i) << 16 | (int(coef[b, i]) & 0xFFFF))
        start.append(len(words))
    nbytes = (224 + 4 * 5 + 4 * len(words) + 15) // 16 * 16
    packed = aligned(nbytes)
    packed[:32].view(np.uint32)[:] = [0x4B50444A, H, W, D.GRAY, 4, len(words), nbytes, 0]
    packed[32:96] = q
    packed[224:224 + 20].view(np.uint32)[:] = start
    packed[244:244 + 4 * len(words)].view(np.uint32)[:] = words
    ws, out = aligned(lib.ml_jpeg_decode_workspace_bytes(1, H, W, D.GRAY)), aligned(H * W * 3)
    rc = lib.ml_jpeg_decode_reference_host(C.c_void_p(packed.ctypes.data), (C.c_int64 * 2)(0, nbytes), 1, H, W, D.GRAY,
                                           C.c_void_p(out.ctypes.data), C.c_void_p(ws.ctypes.data))
    assert rc == 0, lib.ml_last_error()
    want = D.reconstruct(dict(height=H, width=W, mode=D.GRAY, qtables=[q], coefficients=coef))
    assert_same_pixels(out.reshape(H, W, 3), want, "extreme coefficients")


# ----------------------------------------------------------------------------- classification
def _patched(stream, marker, offset, value):
    at = stream.index(marker) + offset
    return stream[:at] + bytes([value]) + stream[at + 1:]


def test_classification(lib, cases):
    from masklab_hip import _lib
    good = cases["photo_150x203_q95"]["stream"]
    for name, c in cases.items():
        rc, (H, W, mode, blocks) = info(lib, c["stream"])
        assert rc == (0 if c["supported"] else _lib.JPEG_UNSUPPORTED), name
        if c["supported"]:
            assert (H, W, mode) == (*c["pixels"].shape[:2], MODES[c["mode"]]), name
        else:
            assert b"unsupported" in lib.ml_last_error() and lib.ml_jpeg_decode_packed_bytes(c["stream"], len(c["stream"])) == -1
    assert b"0xFFC2" in (info(lib, cases["photo_150x203_progressive"]["stream"]), lib.ml_last_error())[1]
    assert b"sampling 2x1" in (info(lib, cases["photo_150x203_422"]["stream"]), lib.ml_last_error())[1]
    sof, app0 = good.index(b"\xff\xc0"), good.index(b"\xff\xe0")
    assert good[app0 + 4:app0 + 9] == b"JFIF\x00"
    no_jfif = good[:app0 + 4] + b"JFXX" + good[app0 + 8:]
    rgb_ids = no_jfif[:sof + 10] + b"R" + no_jfif[sof + 11:sof + 13] + b"G" + no_jfif[sof + 14:sof + 16] + b"B" + no_jfif[sof + 17:]
    sos = rgb_ids.index(b"\xff\xda")
    rgb_ids = rgb_ids[:sos + 5] + b"R" + rgb_ids[sos + 6:sos + 7] + b"G" + rgb_ids[sos + 8:sos + 9] + b"B" + rgb_ids[sos + 10:]
    adobe = lambda transform: (good[:app0] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform]) + good[app0:])
    four = good[:sof + 9] + b"\x04" + good[sof + 10:]
    tall = good[:sof + 5] + (16385).to_bytes(2, "big") + good[sof + 7:]
    table = [
        (good, 0, b""),
        (no_jfif, 0, b""),                                               # ids 1 2 3 are YCbCr with or without JFIF
        (adobe(1), 0, b""),
        (good[:sof + 4] + b"\x0c" + good[sof + 5:], 1, b"12-bit"),
        (_patched(good, b"\xff\xc0", 1, 0xC1), 1, b"0xFFC1"),            # extended sequential
        (_patched(good, b"\xff\xc0", 1, 0xC3), 1, b"0xFFC3"),            # lossless
        (_patched(good, b"\xff\xc0", 1, 0xC9), 1, b"0xFFC9"),            # arithmetic
        (_patched(good, b"\xff\xc0", 11, 0x12), 1, b"sampling 1x2"),     # 4:4:0
        (_patched(good, b"\xff\xc0", 11, 0x41), 1, b"sampling 4x1"),
        (four, 1, b"4 components"),
        (adobe(0), 1, b"Adobe transform 0"),
        (adobe(2), 1, b"Adobe transform 2"),
        (rgb_ids, 1, b"R, G, B"),
        (_patched(good, b"\xff\xda", 4, 1), 1, b"a scan of 1 of the 3"),
        (_patched(good, b"\xff\xdb", 4, 0x10), 1, b"16-bit quantisation"),
        (tall, 1, b"above 16384"),
        (b"\x89PNG\r\n\x1a\n" + bytes(40), 1, b"not a JPEG"),
        (b"", 1, b"not a JPEG"),
        (b"\xff\xd8", 1, b"not a JPEG"),
        (good[:sof + 6], 1, b"truncated"),                               # a header that cannot be read is not vouched for
    ]
    for k, (stream, want, text) in enumerate(table):
        rc, _ = info(lib, stream)
        assert rc == want and text in lib.ml_last_error(), (k, rc, lib.ml_last_error())
    assert lib.ml_jpeg_decode_info(None, 0, (C.c_int32 * 4)()) == 1
    assert lib.ml_jpeg_decode_info(good, len(good), None) == -1


# ----------------------------------------------------------------------------- malformed input
def test_malformed_streams_fail_with_the_reason(lib, cases):
    good = cases["photo_150x203_q95"]["stream"]
    restart = cases["photo_150x203_restart_blocks5"]["stream"]
    sos = good.index(b"\xff\xda")
    scan = sos + 14
    assert entropy(lib, good)[0] > 0

    def fails(stream, text):
        n, _, err = entropy(lib, stream)
        assert n == -1 and text in err, (n, err, text)

    fails(good[:scan + 50], "scan ends inside block")
    fails(good[:-2], "no EOI")
    fails(good[:-2] + b"\xff\xd0", "where EOI was expected")
    fails(good[:sos - 20], "truncated segment")
    fails(good[:scan + 40] + b"\xff\xd0" + good[scan + 40:], "scan ends inside block")          # a marker inside the scan
    fails(_patched(good, b"\xff\xc4", 4, 0x02), "DC Huffman table 0 is not defined")
    fails(_patched(good, b"\xff\xdb", 4, 0x03), "quantisation table 0 is not defined")
    fails(_patched(good, b"\xff\xc4", 5, 3), "bad DHT segment")             # BITS now count more symbols than the segment has
    at = restart.index(b"\xff\xd1")
    fails(restart[:at] + b"\xff\xd2" + restart[at + 2:], "RST1 expected")
    fails(restart[:at] + restart[at + 2:], "RST1 expected")
    n, packed, err = entropy(lib, restart[:at] + b"\xff\xff" + restart[at:])                 # fill bytes before a marker are legal
    assert n > 0, err
    np.testing.assert_array_equal(D.unpack(packed[:n])["coefficients"], D.parse(restart)["coefficients"])
    # tables whose only codes make the error paths certain: (class, id) -> (BITS, HUFFVAL) in place of the Annex K ones
    def with_tables(dc_vals=None, ac_vals=None):
        out = J.header(16, 16, 95)
        for cls, vals in ((0, dc_vals), (1, ac_vals)):
            if vals is not None:
                seg = bytes([cls << 4]) + bytes([0, len(vals)] + [0] * 14) + bytes(vals)    # all codes 2 bits long
                old = J._segment(0xC4, bytes([cls << 4]) + bytes(J.STD_HUFFMAN[(cls, 0)][0]) + bytes(J.STD_HUFFMAN[(cls, 0)][1]))
                assert old in out
                out = out.replace(old, J._segment(0xC4, seg))
        return out

    zeros = bytes(64) + b"\xff\xd9"
    fails(with_tables(dc_vals=[12]) + zeros, "DC category 12 above 11")
    fails(with_tables(dc_vals=[0], ac_vals=[0x0B]) + zeros, "AC size 11 above 10")
    fails(with_tables(dc_vals=[0], ac_vals=[0xF1]) + zeros, "a run past coefficient 63")
    fails(with_tables(dc_vals=[0], ac_vals=[0xF0]) + zeros, "a zero run past coefficient 63")
    fails(with_tables(dc_vals=[0], ac_vals=[0x30]) + zeros, "run/size symbol 0x30")
    fails(with_tables(dc_vals=[0, 1]) + b"\xaa" * 64 + b"\xff\xd9", "a code that is not in DC table 0")
    # a capacity that is too small is an error, not an overrun
    cap = lib.ml_jpeg_decode_packed_bytes(good, len(good))
    buf = aligned(cap, 0xA5)
    small = 224 + 4 * (6 * 130 + 1) + 4 * 6 * 130 + 64
    assert lib.ml_jpeg_decode_entropy(good, len(good), C.c_void_p(buf.ctypes.data), small) == -1
    assert b"packed buffer is full" in lib.ml_last_error() and (buf[small:] == 0xA5).all()
    assert lib.ml_jpeg_decode_entropy(good, len(good), C.c_void_p(buf.ctypes.data), 100) == -1 and b"capacity" in lib.ml_last_error()


def guarded(data, guard=4096):
    """A copy of `data` with 0xA5 on both sides -> (whole array, address of the copy)."""
    raw = np.full(len(data) + 2 * guard, 0xA5, np.uint8)
    raw[guard:guard + len(data)] = np.frombuffer(data, np.uint8)
    return raw, raw.ctypes.data + guard


def test_huffman_tables_with_more_codes_than_a_length_holds(lib):
    """A DHT segment whose length agrees with its BITS, but whose BITS give a length more codes than it has: refused
    before the lookup table is touched.  Every entry point that parses a header sees it, on a bare SOI + DHT + EOI and on
    a whole stream, for both table classes and for short and long code lengths."""
    def dht(cls, bits):
        assert len(bits) == 16
        return J._segment(0xC4, bytes([cls << 4]) + bytes(bits) + bytes(k & 255 for k in range(sum(bits))))

    def at_length(length, count):
        bits = [0] * 16
        bits[length - 1] = count
        return bits

    overflowing = [at_length(1, 3), at_length(1, 200), at_length(2, 5), at_length(2, 255),
                   [0] * 6 + [1, 255] + [0] * 8,                         # one 7-bit code, then 255 of the 254 8-bit ones left
                   [1, 2, 1] + [0] * 13,                                 # 0, 10, 11: no 3-bit code is left
                   [1] * 15 + [3],                                       # beyond the lookup table's lengths: 2 codes are left
                   at_length(4, 17), [2] + [0] * 14 + [1]]
    old = {cls: J._segment(0xC4, bytes([cls << 4]) + bytes(J.STD_HUFFMAN[(cls, 0)][0]) + bytes(J.STD_HUFFMAN[(cls, 0)][1]))
           for cls in (0, 1)}
    whole = J.header(16, 16, 95)
    seen = 0
    for bits in overflowing:
        for cls in (0, 1):
            assert old[cls] in whole
            streams = [b"\xff\xd8" + dht(cls, bits) + b"\xff\xd9", whole.replace(old[cls], dht(cls, bits)) + bytes(64) + b"\xff\xd9"]
            for stream in streams:
                raw, at = guarded(stream)
                out, out_at = guarded(bytes(16))
                rc = lib.ml_jpeg_decode_info(C.c_void_p(at), len(stream), C.c_void_p(out_at))
                assert rc == 1 and b"more codes than their length holds" in lib.ml_last_error(), (bits, cls, lib.ml_last_error())
                assert lib.ml_jpeg_decode_packed_bytes(C.c_void_p(at), len(stream)) == -1
                assert b"more codes than their length holds" in lib.ml_last_error()
                packed, packed_at = guarded(bytes(4096))
                assert lib.ml_jpeg_decode_entropy(C.c_void_p(at), len(stream), C.c_void_p(packed_at), 4096) == -1
                assert b"more codes than their length holds" in lib.ml_last_error()
                for buf, n in ((raw, len(stream)), (out, 16), (packed, 4096)):
                    assert (buf[:4096] == 0xA5).all() and (buf[4096 + n:] == 0xA5).all()
                assert not out[4096:4096 + 16].view(np.int32)[:2].any() and not (packed[4096:-4096]).any()
                seen += 1
    assert seen == 36
    # tables that fill their lengths exactly are taken: two 1-bit codes; 1 + 1 + 2 codes of lengths 1, 2, 3
    for bits in (at_length(1, 2), [1, 1, 2] + [0] * 13, at_length(8, 255), [1] * 15 + [2]):
        stream = whole.replace(old[0], dht(0, bits)) + bytes(64) + b"\xff\xd9"
        assert info(lib, stream)[0] == 0, lib.ml_last_error()


def test_ff00_unstuffing(lib, cases):
    """The noise frames at quality 100 carry stuffed bytes; the reader must take FF 00 as FF."""
    stream = cases["noise_64x80_q100_libjpeg"]["stream"]
    assert J.decode(stream)["stuffed"] > 0
    n, packed, err = entropy(lib, stream)
    assert n > 0, err


def test_truncations_and_corruptions_end_in_ok_or_an_error(lib, cases):
    """Truncations at every 97th byte and 200 seeded single-byte corruptions of the header and of the scan: each call
    returns (no crash, nothing written past the capacity), and whatever it accepts passes the packed form's invariants
    and runs through the kernels' code on the host."""
    good = cases["photo_150x203_restart_rows1"]["stream"]
    scan = good.index(b"\xff\xda") + 14
    rng = np.random.default_rng(97)
    streams = [good[:k] for k in range(0, len(good), 97)]
    for region in ((2, scan), (scan, len(good))):
        for _ in range(100):
            at = int(rng.integers(*region))
            streams.append(good[:at] + bytes([int(rng.integers(0, 256))]) + good[at + 1:])
    # and 64 seeded corruptions of a Huffman table's BITS with the segment rebuilt to the length they imply
    dht = good.index(b"\xff\xc4")
    length = int.from_bytes(good[dht + 2:dht + 4], "big")
    for _ in range(64):
        bits = bytearray(good[dht + 5:dht + 21])
        bits[int(rng.integers(0, 16))] = int(rng.integers(0, 256))
        vals = (good[dht + 21:dht + 2 + length] * 32)[:sum(bits)]
        streams.append(good[:dht] + J._segment(0xC4, good[dht + 4:dht + 5] + bytes(bits) + vals) + good[dht + 2 + length:])
    ok = 0
    for stream in streams:
        rc, (H, W, mode, blocks) = info(lib, stream)
        assert rc in (0, 1)
        if len(stream) == 0 or rc == 1:
            continue
        n, packed, err = entropy(lib, stream)
        assert n == -1 or n > 0, n
        if n == -1:
            assert err
            continue
        got = D.unpack(packed[:n])                                       # index < 64, monotone offsets, entries <= 64 blocks
        assert (got["height"], got["width"], got["mode"]) == (H, W, mode) and got["coefficients"].shape[0] == blocks
        host_pixels(lib, stream)
        ok += 1
    assert 0 < ok < len(streams)


# ----------------------------------------------------------------------------- the layer and ops, as far as a host goes
def test_layer_without_a_device_is_untouched(monkeypatch, cases):
    import torch
    from masklab_hip.layers import DecodeImageContent
    layer = DecodeImageContent()
    assert layer.device is None and layer.on_device is None and not layer._decodes_on_device()
    assert not DecodeImageContent(device="cpu")._decodes_on_device()
    assert not DecodeImageContent(device="cuda:0", on_device=False)._decodes_on_device()
    assert DecodeImageContent(device="cuda:0")._decodes_on_device()
    config = DecodeImageContent(device="cuda:0", on_device=False).get_config()
    assert config["device"] == "cuda:0" and config["on_device"] is False
    content = cases["photo_150x203_q95"]["stream"]
    with monkeypatch.context() as m:
        m.setitem(sys.modules, "PIL", None)
        with pytest.raises(ImportError, match="install Pillow"):
            layer(content)
    pytest.importorskip("PIL.Image")
    frame = layer(content)
    assert isinstance(frame, torch.Tensor) and not frame.is_cuda and tuple(frame.shape) == (1, 150, 203, 3)
    assert_same_pixels(frame[0].numpy(), cases["photo_150x203_q95"]["pixels"], "host path")


def test_ops_classifies_before_it_touches_a_device(lib, cases):
    from masklab_hip import ops
    assert ops.jpeg_info(cases["photo_150x203_444"]["stream"]) == (150, 203, D.S444, 3 * 19 * 26)
    with pytest.raises(ops.UnsupportedJpeg, match="0xFFC2"):
        ops.jpeg_info(cases["photo_150x203_progressive"]["stream"])
    assert not issubclass(ops.UnsupportedJpeg, (ValueError, RuntimeError)) and issubclass(ops.JpegDecodeError, ValueError)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_jpeg(cases["photo_150x203_q95"]["stream"], "cpu")
    with pytest.raises(ValueError, match="1 .. 32 streams"):
        ops.decode_jpeg([], "cuda:0")
