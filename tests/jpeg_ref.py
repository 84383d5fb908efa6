"""NumPy reference of the baseline JPEG encoder (csrc/jpeg.hip), for the tests only:

(a) `decode`: a strict baseline decoder down to the quantised coefficients;
(b) `oracle_real` / `oracle_coefficients`: the sample stage and the 8x8 DCT in fp64, per coefficient the real value
    v / Q and its rounding;
(c) `encode`: an fp64 encoder built from (b) that writes a whole stream.

Coefficients are laid out as the encoder writes them: int [mcus, 6, 64], the six blocks of a 4:2:0 MCU in scan order
(Y00 Y01 Y10 Y11 Cb Cr), each block in zigzag order.  The tables are the ones of ITU-T T.81 Annex K."""
import numpy as np

# zigzag position -> natural (row-major) index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                   46, 53, 60, 61, 54, 47, 55, 62, 63])
BASE_LUMINANCE = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                           14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMINANCE = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                             47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
_AC_LUM = ("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
           "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
           "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHR = ("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536"
           "3738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2"
           "a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
# (class, id) -> (BITS[16], HUFFVAL)
STD_HUFFMAN = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], list(bytes.fromhex(_AC_LUM))),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], list(bytes.fromhex(_AC_CHR))),
}


class JpegError(ValueError):
    pass


def quant_tables(quality):
    """The libjpeg quality rule -> (luminance, chrominance), natural order."""
    if not 1 <= quality <= 100:
        raise ValueError("quality 1..100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (BASE_LUMINANCE, BASE_CHROMINANCE))


def huffman_codes(bits, vals):
    """BITS / HUFFVAL -> {symbol: (code, length)} (T.81 Annex C)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


# ----------------------------------------------------------------------------- (b) the fp64 oracle
def _fix(x):
    return int(x * 65536 + 0.5)


def ycc_planes(frame):
    """uint8 [H,W,3] -> Y [Hp,Wp], Cb and Cr [Hp/2,Wp/2] as integers: the JFIF fixed-point conversion, planes padded to
    a multiple of 16 by replicating the last column and row, chroma the 2x2 box with bias 1, 2, 1, 2 ... along a row."""
    frame = np.asarray(frame)
    H, W = frame.shape[:2]
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    p = np.pad(frame, ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (_fix(.299) * R + _fix(.587) * G + _fix(.114) * B + 32768) >> 16
    Cb = (-_fix(.16874) * R - _fix(.33126) * G + _fix(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (_fix(.5) * R - _fix(.41869) * G - _fix(.08131) * B + (128 << 16) + 32767) >> 16
    bias = np.tile(np.array([1, 2]), Wp // 4)[None, :]

    def box(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2

    return Y, box(Cb), box(Cr)


def _dct_matrix():
    x = np.arange(8)
    m = 0.5 * np.cos((2 * x[None, :] + 1) * x[:, None] * np.pi / 16)
    m[0] *= 1 / np.sqrt(2)
    return m                                                             # m[u, x]


def oracle_real(frame, quality=95):
    """float64 [mcus, 6, 64]: v / Q per coefficient, zigzag order (v = the orthonormal DCT of T.81 A.3.3 of the
    level-shifted samples)."""
    Y, Cb, Cr = ycc_planes(frame)
    ql, qc = quant_tables(quality)
    D = _dct_matrix()
    Hp, Wp = Y.shape
    mh, mw = Hp // 16, Wp // 16

    def blocks(plane, q):                                                # [h8, w8, 64] zigzag
        h8, w8 = plane.shape[0] // 8, plane.shape[1] // 8
        s = (plane.astype(np.float64) - 128).reshape(h8, 8, w8, 8).transpose(0, 2, 1, 3)
        v = D @ s @ D.T
        return (v.reshape(h8, w8, 64) / q.astype(np.float64))[..., ZIGZAG]

    y, cb, cr = blocks(Y, ql), blocks(Cb, qc), blocks(Cr, qc)
    out = np.empty((mh, mw, 6, 64))
    for k in range(4):
        out[:, :, k] = y[k // 2::2, k % 2::2]
    out[:, :, 4], out[:, :, 5] = cb, cr
    return out.reshape(mh * mw, 6, 64)


def round_half_away(real):
    return (np.sign(real) * np.trunc(np.abs(real) + 0.5)).astype(np.int64)


def oracle_coefficients(frame, quality=95):
    return round_half_away(oracle_real(frame, quality))


def compare(coefficients, frame, quality=95):
    """(share of coefficients that differ from the oracle's rounding, largest difference)."""
    want = oracle_coefficients(frame, quality)
    diff = np.abs(np.asarray(coefficients, dtype=np.int64) - want)
    return float((diff != 0).mean()), int(diff.max())


# ----------------------------------------------------------------------------- (c) the encoder
def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(H, W, quality=95):
    """SOI, APP0 (JFIF 1.01, 300 x 300 dpi: the defaults of tf.io.encode_jpeg), 2 DQT, SOF0, 4 DHT, SOS."""
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x01\x01\x2c\x01\x2c\x00\x00")
    out += _segment(0xDB, bytes([0]) + bytes(ql[ZIGZAG].tolist())) + _segment(0xDB, bytes([1]) + bytes(qc[ZIGZAG].tolist()))
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") +
                    bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for key in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = STD_HUFFMAN[key]
        out += _segment(0xC4, bytes([key[0] << 4 | key[1]]) + bytes(bits) + bytes(vals))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def _magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def encode_stream(coefficients, H, W, quality=95):
    """Coefficients [mcus, 6, 64] -> the whole file."""
    dc = [huffman_codes(*STD_HUFFMAN[(0, t)]) for t in (0, 1)]
    ac = [huffman_codes(*STD_HUFFMAN[(1, t)]) for t in (0, 1)]
    acc, nbits = 0, 0
    pred = [0, 0, 0]
    coefficients = np.asarray(coefficients).astype(np.int64)
    assert coefficients.shape == ((-(-H // 16)) * (-(-W // 16)), 6, 64), coefficients.shape

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | code
        nbits += length

    for mcu in coefficients.tolist():
        for b, block in enumerate(mcu):
            comp = max(b - 3, 0)
            t = min(comp, 1)
            size, extra = _magnitude(block[0] - pred[comp])
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
                size, extra = _magnitude(v)
                put(*ac[t][run << 4 | size])
                put(extra, size)
                run = 0
            if run:
                put(*ac[t][0x00])
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    scan = acc.to_bytes((nbits + pad) // 8, "big").replace(b"\xff", b"\xff\x00")
    return header(H, W, quality) + scan + b"\xff\xd9"


def encode(frame, quality=95):
    frame = np.asarray(frame)
    return encode_stream(oracle_coefficients(frame, quality), frame.shape[0], frame.shape[1], quality)


# ----------------------------------------------------------------------------- (a) the strict decoder
def decode(data, expect_hw=None):
    """Baseline 4:2:0 stream -> dict(height, width, qtables=(lum, chr) natural order, coefficients [mcus, 6, 64] zigzag,
    stuffed = number of stuffed 0xFF bytes in the scan, huffman = {(class, id): (bits, vals)}).  Raises JpegError on
    anything a baseline decoder has to guess about: a marker inside the scan, a table id that was not defined or is not
    the JFIF assignment (Y: 0, Cb / Cr: 1), bits left over beyond fewer than eight 1-bits, a missing EOI, bytes after
    EOI, SOF dimensions other than `expect_hw`."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise JpegError("no SOI")
    q, huff, frame, scan = {}, {}, None, None
    i = 2
    while scan is None:
        if i + 4 > len(data) or data[i] != 0xFF:
            raise JpegError(f"marker expected at byte {i}")
        m, L = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        seg = data[i + 4:i + 2 + L]
        if len(seg) != L - 2:
            raise JpegError("truncated segment")
        if m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    raise JpegError("16-bit quantisation table in a baseline stream")
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = list(seg[p + 1:p + 65])
                q[seg[p] & 15] = nat
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                bits = list(seg[p + 1:p + 17])
                n = sum(bits)
                huff[(seg[p] >> 4, seg[p] & 15)] = (bits, list(seg[p + 17:p + 17 + n]))
                p += 17 + n
        elif m == 0xC0:
            if seg[0] != 8 or seg[5] != 3:
                raise JpegError("8-bit three-component frame expected")
            frame = (int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"),
                     [tuple(seg[6 + 3 * c:9 + 3 * c]) for c in range(3)])
        elif m == 0xDA:
            scan = seg
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise JpegError("not a baseline frame")
        elif m == 0xDD:
            raise JpegError("restart interval defined")
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise JpegError(f"unexpected marker 0xFF{m:02X}")
        i += 2 + L
    if frame is None:
        raise JpegError("SOS before SOF0")
    H, W, comps = frame
    if expect_hw is not None and (H, W) != tuple(expect_hw):
        raise JpegError(f"SOF0 says {H}x{W}, the frame is {expect_hw[0]}x{expect_hw[1]}")
    if [c[1] for c in comps] != [0x22, 0x11, 0x11] or [c[2] for c in comps] != [0, 1, 1]:
        raise JpegError(f"4:2:0 sampling with quantisation tables 0, 1, 1 expected, got {comps}")
    if tuple(scan) != (3, comps[0][0], 0x00, comps[1][0], 0x11, comps[2][0], 0x11, 0, 63, 0):
        raise JpegError(f"one interleaved scan with tables 0/0, 1/1, 1/1 expected, got {scan.hex()}")
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):
        if key not in huff:
            raise JpegError(f"Huffman table {key} is not defined")
    for t in (0, 1):
        if t not in q:
            raise JpegError(f"quantisation table {t} is not defined")
    # undo the stuffing
    body, stuffed, end = bytearray(), 0, None
    while i < len(data):
        b = data[i]
        if b != 0xFF:
            body.append(b)
            i += 1
            continue
        if i + 1 >= len(data):
            raise JpegError("stream ends inside a marker")
        nxt = data[i + 1]
        if nxt == 0x00:
            body.append(0xFF)
            stuffed += 1
            i += 2
        elif nxt == 0xD9:
            end = i + 2
            break
        else:
            raise JpegError(f"marker 0xFF{nxt:02X} inside the scan")
    if end is None:
        raise JpegError("no EOI")
    if end != len(data):
        raise JpegError(f"{len(data) - end} bytes after EOI")
    bits = np.unpackbits(np.frombuffer(bytes(body), np.uint8)).tolist()
    lookup = {}
    for key, (b_, v_) in huff.items():
        lookup[key] = {(length, code): sym for sym, (code, length) in huffman_codes(b_, v_).items()}
    pos = 0

    def symbol(table):
        nonlocal pos
        code = 0
        for length in range(1, 17):
            if pos >= len(bits):
                raise JpegError("scan data ends inside a code")
            code = code << 1 | bits[pos]
            pos += 1
            s = table.get((length, code))
            if s is not None:
                return s
        raise JpegError("no such Huffman code")

    def receive(size):
        nonlocal pos
        if size == 0:
            return 0
        if pos + size > len(bits):
            raise JpegError("scan data ends inside a value")
        v = 0
        for k in range(size):
            v = v << 1 | bits[pos + k]
        pos += size
        return v if v >> (size - 1) else v - (1 << size) + 1

    mcus = (-(-H // 16)) * (-(-W // 16))
    out = np.zeros((mcus, 6, 64), np.int64)
    pred = [0, 0, 0]
    for m_ in range(mcus):
        for b in range(6):
            comp = max(b - 3, 0)
            t = min(comp, 1)
            size = symbol(lookup[(0, t)])
            if size > 11:
                raise JpegError("DC category above 11")
            pred[comp] += receive(size)
            out[m_, b, 0] = pred[comp]
            k = 1
            while k < 64:
                rs = symbol(lookup[(1, t)])
                run, size = rs >> 4, rs & 15
                if size == 0:
                    if run == 15:
                        k += 16
                        continue
                    if run == 0:
                        break
                    raise JpegError("bad run/size symbol")
                k += run
                if k > 63:
                    raise JpegError("run past the end of a block")
                out[m_, b, k] = receive(size)
                k += 1
            if k > 64:
                raise JpegError("ZRL past the end of a block")
    left = bits[pos:]
    if len(left) >= 8 or any(v != 1 for v in left):
        raise JpegError(f"{len(left)} bits left after the last MCU: {left[:16]}")
    return dict(height=H, width=W, qtables=(q[0], q[1]), coefficients=out, stuffed=stuffed, huffman=huff)
