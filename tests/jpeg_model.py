"""Test-owned restatements of the video stream, written from that section and from the JPEG standard (ITU-T T.81), not
from the kernels:

  encode(rgb, quality, chroma)  the file bytes, by the textbook sequential route: whole planes in numpy int64, the transform as two
                                matrix products per plane of blocks, one Python loop over the blocks in stream order that emits Huffman
                                symbols the way T.81 F.1.2 describes them (run counter, ZRL, EOB), and a bit writer that appends to one
                                growing integer per restart interval.
  decode(data)                  a baseline decoder: marker parser, Huffman decoding bit by bit, restart markers, destuffing, dequantisation,
                                float64 IDCT, 4:2:0 by replication.  Returns the picture and the dequantised coefficients.
  reference_coefficients(...)   the float64 DCT of the float64 YCbCr planes (the yardstick of the coefficient bound).

The tables below are the data of T.81 Annex K (K.1, K.2: quantisation; K.3 - K.6: Huffman), typed from the standard."""
import numpy as np

# --- T.81 Annex K ------------------------------------------------------------------------------------------------------------------
K1_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64)
K2_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int64)

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFF = {(0, 0): DC_LUMA, (1, 0): AC_LUMA, (0, 1): DC_CHROMA, (1, 1): AC_CHROMA}   # (class, table id)

# zigzag position -> natural index (T.81 figure A.6)
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
    57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)

# --- the fixed-point formats -------------------------------------------------------------------------------------------
RESTART_MCUS = 8          # MCUs per restart interval
SAMPLE_BITS = 16          # fraction bits of a sample, of the row pass's output and of the coefficient
COS_BITS = 20             # fraction bits of the transform matrix
# rows: Y, Cb, Cr; columns: R, G, B; in units of 2^-16 (each row of the chroma pair sums to zero, the luma row to 2^16)
COLOUR = np.array([[19595, 38470, 7471], [-11058, -21710, 32768], [32768, -27439, -5329]], np.int64)


def dct_matrix_float():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    return np.where(u == 0, np.sqrt(0.125), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)


DCT_INT = np.rint(dct_matrix_float() * (1 << COS_BITS)).astype(np.int64)


def quant_tables(quality):
    """The two Annex K tables scaled by the IJG rule (natural order), each entry 1..255."""
    if not 1 <= quality <= 100:
        raise ValueError("quality 1..100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((t * scale + 50) // 100, 1, 255) for t in (K1_LUMA, K2_CHROMA)]


def huffman_codes(bits, vals):
    """symbol -> (code, length), T.81 annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(width, height, quality, chroma):
    """SOI, APP0 (JFIF 1.01, no density), two DQT, SOF0, four DHT (DC0, AC0, DC1, AC1), DRI, SOS."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k, t in enumerate(quant_tables(quality)):
        out += seg(0xDB, bytes([k]) + bytes(int(v) for v in t[ZIGZAG]))
    samp = 0x22 if chroma == "420" else 0x11
    out += seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([3, 1, samp, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls, tid in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = HUFF[(cls, tid)]
        out += seg(0xC4, bytes([cls << 4 | tid]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, RESTART_MCUS.to_bytes(2, "big"))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def _mcu_size(chroma):
    if chroma not in ("420", "444"):
        raise ValueError("chroma '420' or '444'")
    return 16 if chroma == "420" else 8


def _padded(rgb, chroma):
    a = np.asarray(rgb)
    assert a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8
    h, w = a.shape[:2]
    m = _mcu_size(chroma)
    return np.pad(a, ((0, -h % m), (0, -w % m), (0, 0)), mode="edge")


def planes_fixed(rgb, chroma):
    """[Y, Cb, Cr] as int64 planes with SAMPLE_BITS fraction bits, level-shifted; chroma halved in 4:2:0 ((sum of 4 + 2) >> 2)."""
    p = _padded(rgb, chroma).astype(np.int64)
    out = []
    for c in range(3):
        s = p @ COLOUR[c]
        if c == 0:
            s = s - (128 << SAMPLE_BITS)
        elif chroma == "420":
            s = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
        out.append(s)
    return out


def planes_float(rgb, chroma):
    """The float64 source: full-range BT.601 (Kr = 0.299, Kb = 0.114), level-shifted; 4:2:0 chroma is the mean of the four samples."""
    p = _padded(rgb, chroma).astype(np.float64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    out = [y - 128.0, (b - y) / 1.772, (r - y) / 1.402]
    if chroma == "420":
        out[1:] = [(s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]) / 4 for s in out[1:]]
    return out


def _blocks(plane):
    """(H, W) -> (H/8, W/8, 8, 8)"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def reference_coefficients(rgb, chroma):
    """float64 DCT of the float64 planes: per component (H/8, W/8, 8, 8), natural order."""
    c = dct_matrix_float()
    return [c @ _blocks(s) @ c.T for s in planes_float(rgb, chroma)]


def coefficients_fixed(rgb, chroma):
    """The coefficients with SAMPLE_BITS fraction bits: rows first (round to SAMPLE_BITS), then columns (round to SAMPLE_BITS)."""
    half = 1 << (COS_BITS - 1)
    out = []
    for s in planes_fixed(rgb, chroma):
        rows = (_blocks(s) @ DCT_INT.T + half) >> COS_BITS
        out.append((DCT_INT @ rows + half) >> COS_BITS)
    return out


def quantise(coef, table):
    """Half away from zero, straight from the fixed-point coefficient: sign(f) * ((|f| + D / 2) // D), D = step * 2^SAMPLE_BITS."""
    d = table.reshape(8, 8) << SAMPLE_BITS
    return np.sign(coef) * ((np.abs(coef) + (d >> 1)) // d)


class _Bits:
    """MSB-first bit writer of one restart interval: one growing integer."""
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def flush(self):
        """The interval's bytes: padded with ones to a byte, 0xFF followed by a stuffed zero."""
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        raw = self.acc.to_bytes(self.n // 8, "big")
        return raw.replace(b"\xff", b"\xff\x00"), raw.count(b"\xff")


def _magnitude(v):
    """(size, extra bits) of T.81 F.1.2.1 / F.1.2.2"""
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


def encode(rgb, quality=90, chroma="420", info=None):
    """The complete file.  info (a dict): blocks, scan_bytes, stuffed_bytes, restart_intervals."""
    h, w = np.asarray(rgb).shape[:2]
    tables = quant_tables(quality)
    q = [quantise(c, tables[min(k, 1)]) for k, c in enumerate(coefficients_fixed(rgb, chroma))]
    zz = [c.reshape(c.shape[0], c.shape[1], 64)[:, :, ZIGZAG] for c in q]
    dc = [huffman_codes(*HUFF[(0, t)]) for t in (0, 1)]
    ac = [huffman_codes(*HUFF[(1, t)]) for t in (0, 1)]
    m = _mcu_size(chroma)
    mh, mw = -(-h // m), -(-w // m)
    # the blocks of one MCU: (component, row offset, column offset) in units of blocks
    layout = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)] if chroma == "420" else [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    f = 2 if chroma == "420" else 1
    scan, stuffed, intervals = bytearray(), 0, 0
    bits, pred = _Bits(), [0, 0, 0]
    n_mcu = mh * mw
    for k in range(n_mcu):
        my, mx = divmod(k, mw)
        for comp, oy, ox in layout:
            fy = f if comp == 0 else 1
            z = zz[comp][my * fy + oy, mx * fy + ox]
            t = min(comp, 1)
            size, extra = _magnitude(int(z[0]) - pred[comp])
            pred[comp] = int(z[0])
            bits.put(*dc[t][size])
            bits.put(extra, size)
            run = 0
            for pos in range(1, 64):
                v = int(z[pos])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    bits.put(*ac[t][0xF0])
                    run -= 16
                size, extra = _magnitude(v)
                bits.put(*ac[t][run << 4 | size])
                bits.put(extra, size)
                run = 0
            if run > 0:
                bits.put(*ac[t][0x00])
        if (k + 1) % RESTART_MCUS == 0 or k + 1 == n_mcu:
            data, ff = bits.flush()
            scan += data
            stuffed += ff
            if k + 1 < n_mcu:
                scan += bytes([0xFF, 0xD0 + intervals % 8])
            intervals += 1
            bits, pred = _Bits(), [0, 0, 0]
    if info is not None:
        info.update(blocks=n_mcu * len(layout), scan_bytes=len(scan), stuffed_bytes=stuffed, restart_intervals=intervals)
    return header(w, h, quality, chroma) + bytes(scan) + b"\xff\xd9"


# --- decoder --------------------------------------------------------------------------------------------------------------------------
class _Reader:
    def __init__(self, data):
        self.data, self.pos, self.n = data, 0, len(data) * 8

    def bit(self):
        if self.pos >= self.n:
            raise ValueError("scan data exhausted")
        b = (self.data[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return b

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise ValueError("no Huffman code matches")

    def value(self, size):
        if size == 0:
            return 0
        v = self.bits(size)
        return v if v >> (size - 1) else v - (1 << size) + 1


def decode(data):
    """dict(width, height, chroma, rgb uint8 (H, W, 3), coef: per component the dequantised coefficients (H/8, W/8, 8, 8) float64 in
    natural order, quant: per component its table, restart_interval, intervals)"""
    assert data[:2] == b"\xff\xd8", "no SOI"
    pos, qt, ht, ri = 2, {}, {}, 0
    frame = comps = None
    while True:
        assert data[pos] == 0xFF, f"marker expected at {pos}"
        marker = data[pos + 1]
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0, "16-bit quantisation table"
                t = np.zeros(64)
                t[ZIGZAG] = list(body[1:65])
                qt[body[0] & 15] = t.reshape(8, 8)
                body = body[65:]
        elif marker == 0xC0:
            assert body[0] == 8 and body[5] == 3
            frame = (int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"))
            comps = [(body[6 + 3 * k], body[7 + 3 * k] >> 4, body[7 + 3 * k] & 15, body[8 + 3 * k]) for k in range(3)]
        elif marker == 0xC4:
            while body:
                bits, cnt = list(body[1:17]), sum(body[1:17])
                codes = huffman_codes(bits, list(body[17:17 + cnt]))
                ht[(body[0] >> 4, body[0] & 15)] = {(ln, c): s for s, (c, ln) in codes.items()}
                body = body[17 + cnt:]
        elif marker == 0xDD:
            ri = int.from_bytes(body, "big")
        elif marker == 0xDA:
            assert body[0] == 3 and tuple(body[7:10]) == (0, 63, 0)
            sel = {body[1 + 2 * k]: (body[2 + 2 * k] >> 4, body[2 + 2 * k] & 15) for k in range(3)}
            break
        elif marker in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise ValueError("not a baseline stream")
        else:
            assert 0xE0 <= marker <= 0xFE, f"unexpected marker {marker:02x}"
    height, width = frame
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    assert (hmax, vmax) in ((1, 1), (2, 2)) and comps[1][1:3] == (1, 1) and comps[2][1:3] == (1, 1) and comps[0][1:3] == (hmax, vmax)
    mh, mw = -(-height // (8 * vmax)), -(-width // (8 * hmax))
    # split the entropy-coded data at the markers; destuff each interval
    end = data.rindex(b"\xff\xd9")
    assert end == len(data) - 2, "bytes after EOI"
    chunks, start, k = [], pos, pos
    while k < end:
        if data[k] == 0xFF and data[k + 1] != 0:
            assert data[k + 1] == 0xD0 + len(chunks) % 8, f"marker {data[k + 1]:02x} inside the scan at {k}"
            chunks.append(data[start:k])
            k += 2
            start = k
        else:
            k += 2 if data[k] == 0xFF else 1
    chunks.append(data[start:end])
    n_mcu = mh * mw
    assert len(chunks) == (-(-n_mcu // ri) if ri else 1), (len(chunks), n_mcu, ri)
    coef = [np.zeros((mh * c[2], mw * c[1], 64)) for c in comps]
    k = 0
    for chunk in chunks:
        rd = _Reader(chunk.replace(b"\xff\x00", b"\xff"))
        pred = [0, 0, 0]
        for _ in range(min(ri, n_mcu - k) if ri else n_mcu):
            my, mx = divmod(k, mw)
            for ci, (cid, hs, vs, tq) in enumerate(comps):
                tdc, tac = sel[cid]
                for oy in range(vs):
                    for ox in range(hs):
                        z = np.zeros(64)
                        pred[ci] += rd.value(rd.symbol(ht[(0, tdc)]))
                        z[0] = pred[ci]
                        p = 1
                        while p < 64:
                            s = rd.symbol(ht[(1, tac)])
                            if s == 0:
                                break
                            if s == 0xF0:
                                p += 16
                                continue
                            p += s >> 4
                            assert p < 64, "run past the block"
                            z[p] = rd.value(s & 15)
                            p += 1
                        coef[ci][my * vs + oy, mx * hs + ox] = z
            k += 1
        left = rd.n - rd.pos
        assert left < 8 and rd.bits(left) == (1 << left) - 1, "interval does not end in its one-padding"
    c = dct_matrix_float()
    nat, planes = [], []
    for ci, (cid, hs, vs, tq) in enumerate(comps):
        a = np.zeros_like(coef[ci])
        a[:, :, ZIGZAG] = coef[ci]
        a = a.reshape(a.shape[0], a.shape[1], 8, 8) * qt[tq]
        nat.append(a)
        px = c.T @ a @ c
        plane = px.swapaxes(1, 2).reshape(px.shape[0] * 8, px.shape[1] * 8)
        planes.append(np.repeat(np.repeat(plane, vmax // vs, axis=0), hmax // hs, axis=1))
    y, cb, cr = planes[0] + 128.0, planes[1], planes[2]
    rgb = np.stack([y + 1.402 * cr, y - (0.114 * 1.772 * cb + 0.299 * 1.402 * cr) / 0.587, y + 1.772 * cb], axis=2)
    rgb = np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)[:height, :width]
    return dict(width=width, height=height, chroma="420" if hmax == 2 else "444", rgb=rgb, coef=nat, quant=[qt[c[3]] for c in comps],
                restart_interval=ri, intervals=len(chunks))
