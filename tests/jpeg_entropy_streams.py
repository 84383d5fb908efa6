"""Streams for the device entropy decoder's tests (tests/test_jpeg_entropy_cpu.py, tests/test_gpu_jpeg_entropy.py): a
vectorised twin of jpeg_ref.encode_stream that also writes restart intervals (the reference encoder shifts one Python
integer per code, which is quadratic in the scan), frames sized from the decoder's geometry, the flat frame that
synchronises slowly, a stream with FF 00 astride a subsequence boundary, and malformed streams by class."""
import ctypes as C

import numpy as np

import jpeg_ref as J


def encode_stream(coefficients, H, W, quality=95, restart=0):
    """jpeg_ref.encode_stream's file for restart = 0 (held to it by a test); restart = n > 0 writes DRI n and RSTm."""
    dc = [J.huffman_codes(*J.STD_HUFFMAN[(0, t)]) for t in (0, 1)]
    ac = [J.huffman_codes(*J.STD_HUFFMAN[(1, t)]) for t in (0, 1)]
    coefficients = np.asarray(coefficients).astype(np.int64)
    assert coefficients.shape == ((-(-H // 16)) * (-(-W // 16)), 6, 64), coefficients.shape

    def pack(codes, lengths):
        codes, lengths = np.asarray(codes, np.int64), np.asarray(lengths, np.int64)
        total = int(lengths.sum())
        pad = -total % 8
        if pad:
            codes, lengths = np.append(codes, (1 << pad) - 1), np.append(lengths, pad)
        starts = np.cumsum(lengths) - lengths
        within = np.arange(total + pad) - np.repeat(starts, lengths)
        bits = (np.repeat(codes, lengths) >> (np.repeat(lengths, lengths) - 1 - within)) & 1
        return np.packbits(bits.astype(np.uint8)).tobytes().replace(b"\xff", b"\xff\x00")

    pieces, codes, lengths = [], [], []
    pred = [0, 0, 0]

    def put(code, length):
        codes.append(code)
        lengths.append(length)

    for m, mcu in enumerate(coefficients.tolist()):
        if restart and m and m % restart == 0:
            pieces.append(pack(codes, lengths) + bytes([0xFF, 0xD0 + (m // restart - 1) % 8]))
            codes, lengths, pred = [], [], [0, 0, 0]
        for b, block in enumerate(mcu):
            comp = max(b - 3, 0)
            t = min(comp, 1)
            size, extra = J._magnitude(block[0] - pred[comp])
            pred[comp] = block[0]
            put(*dc[t][size])
            put(extra, size)
            run = 0
            for v in block[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    put(*ac[t][0xF0])
                    run -= 16
                size, extra = J._magnitude(v)
                put(*ac[t][run << 4 | size])
                put(extra, size)
                run = 0
            if run:
                put(*ac[t][0x00])
    pieces.append(pack(codes, lengths))
    head = J.header(H, W, quality)
    if restart:
        sos = head.rindex(b"\xff\xda")
        head = head[:sos] + J._segment(0xDD, restart.to_bytes(2, "big")) + head[sos:]
    return head + b"".join(pieces) + b"\xff\xd9"


def encode(frame, quality=95, restart=0):
    frame = np.asarray(frame)
    return encode_stream(J.oracle_coefficients(frame, quality), frame.shape[0], frame.shape[1], quality, restart)


def scan_offset(stream):
    """First byte of entropy-coded data (these streams have one SOS)."""
    sos = stream.index(b"\xff\xda")
    return sos + 2 + int.from_bytes(stream[sos + 2:sos + 4], "big")


def noise_across_workgroups(sub_bits, per_wg, workgroups=3):
    """A seeded noise frame at quality 100 whose scan spans `workgroups` workgroups of subsequences and part of one more,
    and its restart-interval twin -> (plain, with DRI, subsequences)."""
    need = (workgroups * per_wg + per_wg // 4) * (sub_bits // 8)
    side = 64
    while side * side * 2 < need:                                      # about two bytes a pixel at quality 100
        side += 16
    frame = np.random.default_rng(11).integers(0, 256, (side, side, 3), dtype=np.uint8)
    coefficients = J.oracle_coefficients(frame, 100)
    plain = encode_stream(coefficients, side, side, 100)
    dri = encode_stream(coefficients, side, side, 100, restart=side // 16 + 3)   # intervals that do not follow the MCU rows
    return plain, dri, -(-(len(plain) - scan_offset(plain)) // (sub_bits // 8))


def flat_with_one_block(side=512):
    """A flat 4:2:0 frame whose first block differs: past the first MCU the scan repeats with a short period, and a
    decoder that starts out of phase may never fall into step."""
    frame = np.full((side, side, 3), 117, np.uint8)
    frame[:8, :8] = np.random.default_rng(5).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    return encode(frame, 75)


def stuffing_astride(sub_bits, tries=400):
    """Seeded noise at quality 100 until an FF 00 pair lies across a subsequence boundary: the FF is the last byte of a
    subsequence and the stuffed 00 the first of the next -> (stream, index of that subsequence boundary)."""
    step = sub_bits // 8
    for seed in range(tries):
        frame = np.random.default_rng(1000 + seed).integers(0, 256, (64, 64, 3), dtype=np.uint8)
        stream = encode(frame, 100)
        scan = scan_offset(stream)
        for k in range(1, (len(stream) - scan) // step):
            at = scan + k * step
            if stream[at - 1] == 0xFF and stream[at] == 0x00:
                return stream, k
    raise AssertionError("no FF 00 pair across a subsequence boundary in %d seeds" % tries)


def straddles(stream, k, sub_bits):
    at = scan_offset(stream) + k * (sub_bits // 8)
    return stream[at - 1] == 0xFF and stream[at] == 0x00


# ----------------------------------------------------------------------------- the library's two host entries
def aligned(nbytes, fill=0):
    raw = np.full(nbytes + 16, fill, np.uint8)
    off = -raw.ctypes.data % 16
    return raw[off:off + nbytes]


def host_packed(lib, data):
    """ml_jpeg_decode_entropy -> (packed bytes or None, error text)."""
    cap = lib.ml_jpeg_decode_packed_bytes(data, len(data))
    if cap < 0:
        return None, lib.ml_last_error().decode()
    buf = aligned(cap)
    n = lib.ml_jpeg_decode_entropy(data, len(data), C.c_void_p(buf.ctypes.data), cap)
    if n < 0:
        return None, lib.ml_last_error().decode()
    return buf[:n].tobytes(), ""


def reference_packed(lib, data, guard=64):
    """ml_jpeg_entropy_reference_host -> (status int32[4] as a tuple or None if the stream has no plan, packed bytes
    under status 0).  Nothing may be written past the capacity or the workspace."""
    cap = lib.ml_jpeg_decode_packed_bytes(data, len(data))
    plan = aligned(lib.ml_jpeg_entropy_plan_bytes())
    if cap < 0 or lib.ml_jpeg_entropy_plan(data, len(data), C.c_void_p(plan.ctypes.data)) != 0:
        return None, None
    offsets = (C.c_int64 * 2)(0, len(data))
    nws = lib.ml_jpeg_entropy_workspace_bytes(offsets, 1)
    assert nws > 0
    ws, buf = aligned(nws + guard, 0x5A), aligned(cap + guard, 0xA5)
    status = (C.c_int32 * 4)()
    rc = lib.ml_jpeg_entropy_reference_host(data, len(data), C.c_void_p(plan.ctypes.data), C.c_void_p(buf.ctypes.data), cap,
                                            status, C.c_void_p(ws.ctypes.data))
    assert rc == 0, lib.ml_last_error()
    assert (buf[cap:] == 0xA5).all(), "wrote past the capacity"
    assert (ws[nws:] == 0x5A).all(), "wrote past the workspace"
    if status[0] != 0:
        return tuple(status), None
    n = int(buf[24:28].view(np.uint32)[0])                             # the header's `bytes`
    assert 224 < n <= cap
    return tuple(status), buf[:n].tobytes()


# ----------------------------------------------------------------------------- malformed streams
def corrupted(stream, rng):
    """One seeded truncation or corruption of up to three bytes, mostly behind the headers."""
    s = bytearray(stream)
    if rng.random() < 0.3:
        return bytes(s[:int(rng.integers(2, len(s)))])
    for _ in range(int(rng.integers(1, 4))):
        at = int(rng.integers(len(s) // 3, len(s))) if rng.random() < 0.8 else int(rng.integers(0, len(s)))
        s[at] = int(rng.integers(0, 256)) if rng.random() < 0.7 else (0xFF if rng.random() < 0.5 else 0xD0 + int(rng.integers(0, 10)))
    return bytes(s)


def patch_table_value(stream, cls, old, new):
    """The first DHT table of class `cls` (0 DC, 1 AC) that lists symbol `old` lists `new` instead."""
    at = 2
    while stream[at + 1] != 0xDA:
        length = int.from_bytes(stream[at + 2:at + 4], "big")
        if stream[at + 1] == 0xC4:
            p, end = at + 4, at + 2 + length
            while p < end:
                count = sum(stream[p + 1:p + 17])
                vals = stream[p + 17:p + 17 + count]
                if stream[p] >> 4 == cls and old in vals:
                    k = p + 17 + vals.index(old)
                    return stream[:k] + bytes([new]) + stream[k + 1:]
                p += 17 + count
        at += 2 + length
    raise AssertionError("no table of class %d lists 0x%02X" % (cls, old))


MALFORMED_CLASSES = {                                                  # class -> what the host decoder says
    "code": r"a code that is not in (DC|AC) table",
    "dc": r"DC category \d+ above 11",
    "ac": r"AC size \d+ above 10",
    "run": r"run past coefficient 63",
    "truncated": r"the scan ends inside block",
    "restart": r"RST\d expected before MCU",
    "eoi": r"no EOI after the last MCU|where EOI was expected",
}


def malformed_set(lib, cases, per_class=3, tries=6000):
    """A fixed (seeded) set of malformed streams, `per_class` of each class at most and one at least, in a stable
    order -> [(label, stream, the host's message)].  The block-count class has no message of its own in the host
    decoder: a scan with too few blocks ends inside a block or without EOI, one with too many ends before its EOI."""
    import re
    found = {k: [] for k in MALFORMED_CLASSES}

    def take(label, stream):
        packed, message = host_packed(lib, stream)
        if packed is not None:
            return
        for k, pattern in MALFORMED_CLASSES.items():
            if re.search(pattern, message) and len(found[k]) < per_class and all(stream != s for _, s, _ in found[k]):
                found[k].append((f"{k}:{label}", stream, message))

    photo = cases["photo_150x203_q95"]["stream"]
    take("dc-category-12", patch_table_value(photo, 0, 5, 12))
    take("ac-size-11", patch_table_value(photo, 1, 0x03, 0x0B))
    take("dc-category-15", patch_table_value(cases["noise_37x53_q95"]["stream"], 0, 4, 15))
    take("ac-size-15", patch_table_value(cases["noise_37x53_q95"]["stream"], 1, 0x11, 0x1F))
    rows = cases["photo_150x203_restart_rows1"]["stream"]
    at = rows.index(b"\xff\xd1")
    take("rst-out-of-sequence", rows[:at] + b"\xff\xd2" + rows[at + 2:])
    take("rst-without-dri-position", rows[:at] + rows[at + 2:])
    take("no-eoi", photo[:-2])
    take("marker-for-eoi", photo[:-2] + b"\xff\xc4")
    take("half", photo[:len(photo) // 2])
    names = [k for k in sorted(cases) if cases[k]["supported"] and len(cases[k]["stream"]) < 12000]
    rng = np.random.default_rng(2024)
    for it in range(tries):
        if all(len(v) >= per_class for v in found.values()):
            break
        name = names[it % len(names)]
        stream = corrupted(cases[name]["stream"], rng)
        info = (C.c_int32 * 4)()
        if lib.ml_jpeg_decode_info(stream, len(stream), info) == 0:
            take(f"{name}#{it}", stream)
    assert all(found.values()), {k: len(v) for k, v in found.items()}
    return [item for k in MALFORMED_CLASSES for item in found[k]]
