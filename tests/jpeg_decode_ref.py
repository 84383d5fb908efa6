"""NumPy reference of the baseline JPEG decoder (csrc/jpeg_decode.hip), for the tests only:

(a) `parse`: a general baseline parser -- any table ids, restart intervals, 4:2:0 / 4:4:4 / grayscale -- down to the
    quantised coefficients of every block in scan order, natural order within a block;
(b) `reconstruct` / `decode`: libjpeg-turbo's default decode restated in integer NumPy (JDCT_ISLOW, the "h2v2 fancy"
    triangle upsampling, the fixed-point YCbCr -> RGB), which Pillow reproduces byte for byte.

It reuses the helpers of tests/jpeg_ref.py."""
import numpy as np

import jpeg_ref as J

GRAY, S444, S420 = 0, 1, 2                                               # ML_JPEG_*


class Unsupported(J.JpegError):
    pass


# ----------------------------------------------------------------------------- (a) the parser
class _Bits:
    """The bits of one entropy-coded segment (between markers), FF 00 unstuffed."""

    def __init__(self, body):
        self.bits = np.unpackbits(np.frombuffer(bytes(body), np.uint8)).tolist()
        self.pos = 0

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            if self.pos >= len(self.bits):
                raise J.JpegError("scan data ends inside a code")
            code = code << 1 | self.bits[self.pos]
            self.pos += 1
            s = table.get((length, code))
            if s is not None:
                return s
        raise J.JpegError("no such Huffman code")

    def receive(self, size):
        if size == 0:
            return 0
        if self.pos + size > len(self.bits):
            raise J.JpegError("scan data ends inside a value")
        v = 0
        for k in range(size):
            v = v << 1 | self.bits[self.pos + k]
        self.pos += size
        return v if v >> (size - 1) else v - (1 << size) + 1


def _segments(data, i):
    """The entropy-coded data from byte i: ([unstuffed body of each restart segment], [the RSTn numbers between them]);
    ends at EOI."""
    bodies, markers, body = [], [], bytearray()
    while True:
        if i >= len(data):
            raise J.JpegError("no EOI")
        b = data[i]
        if b != 0xFF:
            body.append(b)
            i += 1
            continue
        if i + 1 >= len(data):
            raise J.JpegError("stream ends inside a marker")
        nxt = data[i + 1]
        if nxt == 0x00:
            body.append(0xFF)
            i += 2
        elif 0xD0 <= nxt <= 0xD7:
            bodies.append(body)
            markers.append(nxt - 0xD0)
            body = bytearray()
            i += 2
        elif nxt == 0xD9:
            bodies.append(body)
            return bodies, markers
        else:
            raise J.JpegError(f"marker 0xFF{nxt:02X} inside the scan")


def parse(data):
    """Baseline stream -> dict(height, width, mode, qtables [ncomp][64] natural order, coefficients int64 [blocks, 64]
    natural order with blocks in scan order, restart).  Unsupported for what the device path does not take."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise Unsupported("no SOI")
    q, huff, frame, scan, restart, i = {}, {}, None, None, 0, 2
    while scan is None:
        if i + 4 > len(data) or data[i] != 0xFF:
            raise J.JpegError(f"marker expected at byte {i}")
        m, L = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        seg = data[i + 4:i + 2 + L]
        if len(seg) != L - 2:
            raise J.JpegError("truncated segment")
        if m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    raise Unsupported("16-bit quantisation table")
                nat = np.zeros(64, np.int64)
                nat[J.ZIGZAG] = list(seg[p + 1:p + 65])
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
            if seg[0] != 8 or seg[5] not in (1, 3):
                raise Unsupported("8-bit frame of one or three components expected")
            frame = (int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"),
                     [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])])
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Unsupported("not a baseline frame")
        elif m == 0xDD:
            restart = int.from_bytes(seg[0:2], "big")
        elif m == 0xDA:
            scan = seg
        i += 2 + L
    if frame is None:
        raise J.JpegError("SOS before SOF0")
    H, W, comps = frame
    sampling = [(c[1], c[2]) for c in comps]
    if len(comps) == 1:
        mode, per_mcu, unit = GRAY, [0], 8
    elif sampling == [(2, 2), (1, 1), (1, 1)]:
        mode, per_mcu, unit = S420, [0, 0, 0, 0, 1, 2], 16
    elif sampling == [(1, 1)] * 3:
        mode, per_mcu, unit = S444, [0, 1, 2], 8
    else:
        raise Unsupported(f"sampling {sampling}")
    if scan[0] != len(comps):
        raise Unsupported("a scan of some of the components")
    tables = []
    for c in range(len(comps)):
        if scan[1 + 2 * c] != comps[c][0]:
            raise Unsupported("scan components out of frame order")
        td, ta = scan[2 + 2 * c] >> 4, scan[2 + 2 * c] & 15
        for key in ((0, td), (1, ta)):
            if key not in huff:
                raise J.JpegError(f"Huffman table {key} is not defined")
        if comps[c][3] not in q:
            raise J.JpegError(f"quantisation table {comps[c][3]} is not defined")
        tables.append(tuple({(length, code): sym for sym, (code, length) in J.huffman_codes(*huff[key]).items()}
                            for key in ((0, td), (1, ta))))
    bodies, markers = _segments(data, i)
    mcus = (-(-H // unit)) * (-(-W // unit))
    if restart:
        if len(bodies) != -(-mcus // restart) or markers != [k % 8 for k in range(len(markers))]:
            raise J.JpegError("wrong or missing RSTn")
    elif markers:
        raise J.JpegError("RSTn without a restart interval")
    out = np.zeros((mcus * len(per_mcu), 64), np.int64)
    blk = 0
    for s, body in enumerate(bodies):
        bits = _Bits(body)
        pred = [0, 0, 0]
        for _ in range(min(restart, mcus - s * restart) if restart else mcus):
            for c in per_mcu:
                dc, ac = tables[c]
                size = bits.symbol(dc)
                if size > 11:
                    raise J.JpegError("DC category above 11")
                pred[c] += bits.receive(size)
                out[blk, 0] = pred[c]
                k = 1
                while k < 64:
                    rs = bits.symbol(ac)
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if run == 15:
                            k += 16
                            continue
                        if run == 0:
                            break
                        raise J.JpegError("bad run/size symbol")
                    k += run
                    if k > 63:
                        raise J.JpegError("run past the end of a block")
                    out[blk, J.ZIGZAG[k]] = bits.receive(size)
                    k += 1
                blk += 1
    return dict(height=H, width=W, mode=mode, qtables=[q[c[3]] for c in comps], coefficients=out, restart=restart)


# ----------------------------------------------------------------------------- (b) libjpeg-turbo's default decode
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(i, shift):
    """The LLM integer IDCT along the last axis (CONST_BITS 13), int64."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (i[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i7, i5, i3, i1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = (t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3)
    return np.stack([_descale(v, shift) for v in out], axis=-1)


def idct_blocks(coefficients, qtable):
    """int [n, 64] natural order -> uint8 samples [n, 8, 8]."""
    c = (np.asarray(coefficients, np.int64) * np.asarray(qtable, np.int64)).reshape(-1, 8, 8)
    ws = _idct_1d(c.transpose(0, 2, 1), 11).transpose(0, 2, 1)          # pass 1 down the columns
    return np.clip(_idct_1d(ws, 18) + 128, 0, 255).astype(np.uint8)     # pass 2 along the rows


def planes(parsed):
    """The padded component planes the blocks tile: [Y] or [Y, Cb, Cr], uint8."""
    H, W, mode, coef = parsed["height"], parsed["width"], parsed["mode"], parsed["coefficients"]
    unit = 16 if mode == S420 else 8
    mh, mw = -(-H // unit), -(-W // unit)

    def tile(blocks, bh, bw):                                            # [bh * bw, 8, 8] raster -> [bh * 8, bw * 8]
        return blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)

    if mode == GRAY:
        return [tile(idct_blocks(coef, parsed["qtables"][0]), mh, mw)]
    per = 6 if mode == S420 else 3
    coef = coef.reshape(mh * mw, per, 64)
    if mode == S444:
        return [tile(idct_blocks(coef[:, c], parsed["qtables"][c]), mh, mw) for c in range(3)]
    y = idct_blocks(coef[:, :4].reshape(-1, 64), parsed["qtables"][0]).reshape(mh, mw, 2, 2, 8, 8)
    luma = y.transpose(0, 2, 4, 1, 3, 5).reshape(mh * 16, mw * 16)
    return [luma] + [tile(idct_blocks(coef[:, 3 + c], parsed["qtables"][c]), mh, mw) for c in (1, 2)]


def upsample_h2v2_fancy(plane, H, W):
    """The real ceil(H/2) x ceil(W/2) part of a chroma plane -> int64 [H, W] (triangle filter, edges replicated)."""
    ch, cw = -(-H // 2), -(-W // 2)
    c = np.pad(plane[:ch, :cw].astype(np.int64), 1, mode="edge")
    mid = c[1:-1]
    colsum = np.empty((2 * ch, cw + 2), np.int64)
    colsum[0::2] = 3 * mid + c[:-2]
    colsum[1::2] = 3 * mid + c[2:]
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * colsum[:, 1:-1] + colsum[:, :-2] + 8) >> 4
    out[:, 1::2] = (3 * colsum[:, 1:-1] + colsum[:, 2:] + 7) >> 4
    return out[:H, :W]


def _fix(a):
    return int(a * 65536 + 0.5)


def reconstruct(parsed):
    """dict of `parse` -> uint8 [H, W, 3]."""
    H, W, mode = parsed["height"], parsed["width"], parsed["mode"]
    p = planes(parsed)
    Y = p[0][:H, :W].astype(np.int64)
    if mode == GRAY:
        return np.repeat(Y[..., None], 3, axis=2).astype(np.uint8)
    if mode == S444:
        cb, cr = (c[:H, :W].astype(np.int64) - 128 for c in p[1:])
    else:
        cb, cr = (upsample_h2v2_fancy(c, H, W) - 128 for c in p[1:])
    R = Y + ((_fix(1.402) * cr + 32768) >> 16)
    G = Y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    B = Y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    return reconstruct(parse(data))


# ----------------------------------------------------------------------------- (c) the fixtures and the packed form
def load_cases(golden_dir):
    """tests/golden/jpeg_decode -> {case: dict(stream bytes, pixels uint8 [H,W,3] or None, mode, supported)}."""
    import json
    import os
    with open(os.path.join(golden_dir, "jpeg_decode", "manifest.json")) as fh:
        manifest = json.load(fh)
    files = {}

    def array(ref):
        name, key = ref.split(":")
        if name not in files:
            with np.load(os.path.join(golden_dir, *name.split("/"))) as z:
                files[name] = {k: z[k] for k in z.files}
        return files[name][key]

    cases = {}
    for case, e in manifest["cases"].items():
        pixels = None
        if e["pixels"] is not None:
            pixels = array(f"jpeg_decode/pixels.npz:{e['pixels']}")
            if pixels.ndim == 2:                                         # grayscale: the three channels agree
                pixels = np.repeat(pixels[..., None], 3, axis=2)
            pixels.setflags(write=False)
        cases[case] = dict(stream=bytes(array(e["stream"])), pixels=pixels, mode=e["mode"], supported=e["supported"])
    return cases


HEADER_BYTES = 224


def unpack(packed):
    """The packed form ml_jpeg_decode_entropy writes (uint8 array) -> dict(height, width, mode, qtables [3][64],
    coefficients int64 [blocks, 64] natural order, entries); asserts the invariants the kernels rely on."""
    packed = np.ascontiguousarray(packed, np.uint8)
    head = packed[:32].view(np.uint32)
    magic, H, W, mode, blocks, entries, nbytes, _ = (int(v) for v in head)
    assert magic == 0x4B50444A, hex(magic)
    assert nbytes % 4 == 0 and HEADER_BYTES + 4 * (blocks + 1) + 4 * entries <= nbytes <= packed.size, (nbytes, packed.size)
    start = packed[HEADER_BYTES:HEADER_BYTES + 4 * (blocks + 1)].view(np.uint32).astype(np.int64)
    words = packed[HEADER_BYTES + 4 * (blocks + 1):][:4 * entries].view(np.uint32)
    assert entries <= 64 * blocks
    assert start[0] == 0 and start[-1] == entries
    per_block = np.diff(start)
    assert (per_block >= 1).all() and (per_block <= 64).all(), "monotone offsets, 1 .. 64 words a block"
    index = (words >> 16).astype(np.int64)
    assert (index < 64).all()
    assert (index[start[:-1]] == 0).all(), "a block's first word is its DC term"
    block_of = np.repeat(np.arange(blocks), per_block)
    coef = np.zeros((blocks, 64), np.int64)
    coef[block_of, index] = (words & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
    assert len(set(zip(block_of.tolist(), index.tolist()))) == entries, "indices are distinct within a block"
    q = packed[32:HEADER_BYTES].reshape(3, 64).astype(np.int64)
    return dict(height=H, width=W, mode=mode, qtables=q, coefficients=coef, entries=entries)
