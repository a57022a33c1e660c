"""Video on the GPU: RGB frames -> baseline JPEG streams -> one Motion-JPEG AVI (C-ABI sph_video_* in include/sph_hip.h).

Stands in for the reference's make_video.py, which needs imageio.  The frames are compressed by the HIP passes of csrc/sph_video.hpp,
where a rendered frame already lies; the AVI container (AviWriter) and the PNG reader of make_video.py (decode_png) are plain host
code on the standard library.  No CPU fallback for the encoder."""
from __future__ import annotations

import struct
import zlib

import numpy as np

from . import _lib as L

CHROMA = {"420": 420, "444": 444}
AVI_LIMIT = (1 << 31) - 1   # a classic (non-OpenDML) AVI keeps every size and offset in a signed 32-bit range


class VideoError(L.SphError):
    pass


class VideoEncoder(L.FrameEncoder):
    """One JPEG encoder for frames of one size.  The bytes of a frame depend on (pixels, width, height, quality, chroma) alone."""
    ABI, Error, Stats = "sph_video", VideoError, L.SphVideoStats

    def __init__(self, width, height, quality=90, chroma="420", device=-1, fast_math=False):
        super().__init__()
        if str(chroma) not in CHROMA:
            raise ValueError(f"chroma must be '420' or '444', not {chroma!r}")
        self.width, self.height, self.quality, self.chroma = int(width), int(height), int(quality), str(chroma)
        p = L.SphVideoParams(width=self.width, height=self.height, quality=self.quality, chroma=CHROMA[self.chroma],
                             fast_math=int(bool(fast_math)), device=int(device), reserved=0)
        self.h = self._create(p)

    def write_jpeg(self, path, rgb):
        with open(path, "wb") as f:
            f.write(self.encode(rgb))


def _fourcc_chunk(tag, data):
    return tag + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b"")


class AviWriter:
    """A classic RIFF AVI with one Motion-JPEG video stream: `hdrl` (avih, one strl: strh + strf, handler and compression MJPG),
    `movi` with one `00dc` chunk per frame (padded to even length), `idx1`.  Sizes and the frame count are patched on close.
    add() raises before the file would pass the 2 GiB of a classic AVI."""

    def __init__(self, path, width, height, fps, limit=AVI_LIMIT):
        if int(fps) != fps or not 1 <= fps <= 1000:
            raise ValueError(f"fps must be an integer in 1..1000, not {fps!r}")
        self.path, self.width, self.height, self.fps, self.limit = path, int(width), int(height), int(fps), int(limit)
        self.frames, self.index, self.largest = 0, [], 0
        self.f = open(path, "wb")
        self.f.write(self._head(0))
        self.movi = self.f.tell() - 4   # offset of the 'movi' tag: idx1 offsets count from here
        self.size = self.f.tell()

    def _head(self, movi_bytes):
        """Everything up to and including 'LIST size movi'."""
        w, h, n = self.width, self.height, self.frames
        avih = struct.pack("<14I", 1000000 // self.fps, self.largest * self.fps, 0, 0x10, n, 0, 1, self.largest, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, 1, self.fps, 0, n, self.largest, 0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + _fourcc_chunk(b"strh", strh) + _fourcc_chunk(b"strf", strf)
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + _fourcc_chunk(b"avih", avih) + strl
        riff_size = 4 + len(hdrl) + 8 + 4 + movi_bytes + 8 + 16 * n
        return b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"

    def add(self, jpeg):
        if self.f is None:
            raise ValueError("AviWriter is closed")
        jpeg = bytes(jpeg)
        chunk = _fourcc_chunk(b"00dc", jpeg)
        if self.size + len(chunk) + 8 + 16 * (self.frames + 1) > self.limit:
            raise VideoError(f"{self.path}: frame {self.frames} would take the file past the {self.limit} bytes of a classic AVI "
                             "(start another file, or lower the quality)", L.ERR_CAPACITY)
        self.index.append((self.size - self.movi, len(jpeg)))
        self.f.write(chunk)
        self.size += len(chunk)
        self.frames += 1
        self.largest = max(self.largest, len(jpeg))

    def close(self):
        if self.f is None:
            return
        idx = b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, n) for off, n in self.index)
        self.f.write(_fourcc_chunk(b"idx1", idx))
        self.f.seek(0)
        self.f.write(self._head(self.size - self.movi - 4))
        self.f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _png_chunks(data):
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("decode_png: not a PNG file")
    pos = 8
    while pos + 12 <= len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if len(body) != n or struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + body) & 0xFFFFFFFF:
            raise ValueError(f"decode_png: chunk {tag!r} is truncated or fails its CRC")
        yield tag, body
        pos += 12 + n


def decode_png(data):
    """uint8 (H, W, 3) of an 8-bit greyscale, RGB or RGBA PNG (alpha dropped), non-interlaced, any row filters.  Everything else --
    other bit depths, palette, grey + alpha, interlace -- raises ValueError naming what it met."""
    ihdr, idat = None, []
    for tag, body in _png_chunks(bytes(data)):
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
    if ihdr is None:
        raise ValueError("decode_png: no IHDR chunk")
    w, h, depth, ctype, comp, filt, inter = ihdr
    if depth != 8:
        raise ValueError(f"decode_png: bit depth {depth} (8 only)")
    if ctype not in (0, 2, 6):
        raise ValueError(f"decode_png: colour type {ctype} ({ {3: 'palette', 4: 'greyscale with alpha'}.get(ctype, 'unknown') }); "
                         "greyscale, RGB and RGBA only")
    if inter != 0:
        raise ValueError("decode_png: interlaced (Adam7) files are not read")
    if comp != 0 or filt != 0:
        raise ValueError(f"decode_png: compression method {comp}, filter method {filt}")
    bpp = {0: 1, 2: 3, 6: 4}[ctype]
    stride = w * bpp
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != h * (stride + 1):
        raise ValueError(f"decode_png: {len(raw)} bytes of image data, expected {h * (stride + 1)}")
    rows = np.frombuffer(raw, np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    zero = np.zeros(stride, np.int64)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = out[y - 1].astype(np.int64) if y else zero
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = line + up
        elif ft in (1, 3, 4):   # the byte to the left is part of the prediction: one pixel column at a time
            cur = np.zeros(stride, np.int64)
            pix, upp = line.reshape(w, bpp), up.reshape(w, bpp)
            res = cur.reshape(w, bpp)
            left, upleft = np.zeros(bpp, np.int64), np.zeros(bpp, np.int64)
            for x in range(w):
                b = upp[x]
                if ft == 1:
                    pred = left
                elif ft == 3:
                    pred = (left + b) >> 1
                else:
                    p = left + b - upleft
                    pa, pb, pc = np.abs(p - left), np.abs(p - b), np.abs(p - upleft)
                    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, b, upleft))
                left = (pix[x] + pred) & 255
                res[x] = left
                upleft = b
        else:
            raise ValueError(f"decode_png: row {y} uses filter type {ft}")
        out[y] = (cur & 255).astype(np.uint8)
    px = out.reshape(h, w, bpp)
    if ctype == 0:
        return np.repeat(px, 3, axis=2)
    return np.ascontiguousarray(px[:, :, :3])
