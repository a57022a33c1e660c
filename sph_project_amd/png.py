"""PNG files on the GPU: RGB frames -> lossless 8-bit RGB .png files (C-ABI sph_png_* in include/sph_hip.h).

Stands in for the zlib pass of render.encode_png over a downloaded frame: row filters, LZ77 tokens, the fixed Huffman code (or, with
coding="dynamic", per segment a dynamic Huffman block where that is shorter: smaller files, a slower count pass; with coding="window"
also matches from the 32 KB before a position, found by a sort of the whole filtered stream: smaller files again), Adler-32 and the chunk
CRCs are computed by the HIP passes of csrc/sph_png.hpp where a rendered frame already lies, and only the finished file
crosses to the host.  No CPU fallback for the encoder (render.encode_png remains what the drivers use without --png_device)."""
from __future__ import annotations

import ctypes as C

from . import _lib as L

class PngError(L.SphError):
    pass


def _filter(f):
    """"adaptive" -> -1; a PNG filter type 0..4 (None, Sub, Up, Average, Paeth) on every row -> itself"""
    if f == "adaptive":
        return -1
    if isinstance(f, str) or int(f) != f or not 0 <= int(f) <= 4:
        raise ValueError(f"filter must be 'adaptive' or a PNG filter type 0..4, not {f!r}")
    return int(f)


CODINGS = {"fixed": L.PNG_CODING_FIXED, "dynamic": L.PNG_CODING_DYNAMIC, "window": L.PNG_CODING_WINDOW}
NO_CANDIDATE = 0xFFFFFFFF


def _coding(c):
    if not isinstance(c, str) or c not in CODINGS:
        raise ValueError(f"coding must be 'fixed', 'dynamic' or 'window', not {c!r}")
    return CODINGS[c]


def bound(width, height, filter="adaptive"):
    """The longest file PngEncoder(width, height) can return in any coding (sph_png_bound: host only)."""
    p = L.SphPngParams(width=int(width), height=int(height), filter=_filter(filter), fast_math=0, device=-1, reserved=0)
    n = C.c_int64()
    lib = L.load()
    if lib.sph_png_bound(C.byref(p), C.byref(n)) != 0:
        raise PngError("sph_png_bound failed: " + (lib.sph_png_last_error(None) or b"").decode(), L.ERR_INVALID)
    return n.value


class PngEncoder(L.FrameEncoder):
    """One PNG encoder for frames of one size.  The bytes of a file depend on (pixels, width, height, filter, coding) alone; a file in
    coding "dynamic" is never longer than the "fixed" one of the same picture, and one in coding "window" never longer than that."""
    ABI, Error, Stats = "sph_png", PngError, L.SphPngStats

    def __init__(self, width, height, filter="adaptive", coding="fixed", fast_math=False, device=-1):
        super().__init__()
        self.width, self.height, self.filter = int(width), int(height), _filter(filter)
        code = _coding(coding)
        p = L.SphPngParams(width=self.width, height=self.height, filter=self.filter, fast_math=int(bool(fast_math)),
                           device=int(device), reserved=0)
        self.h = self._create(p)
        self.coding = "fixed"
        if code != L.PNG_CODING_FIXED:
            self.set_coding(coding)

    def set_coding(self, coding):
        """"fixed" | "dynamic" | "window": the coding of the encodes that follow"""
        self._call("set_coding", _coding(coding))
        self.coding = coding

    def stats(self):
        st = self._stats()
        w = L.SphPngWindowStats()
        self._call("window_stats", C.byref(w))
        return dict(L.struct_dict(st), filter_rows=list(st.filter_rows), **L.struct_dict(w))

    def candidates(self):
        """uint32 per byte of the filtered stream, of the last encode (coding "window"): the position of the most recent earlier
        occurrence of the three bytes that start there, within 32768 bytes; NO_CANDIDATE for none.  For tests and diagnosis."""
        import numpy as np
        prev = np.empty(self.height * (1 + 3 * self.width), np.uint32)
        self._call("download_candidates", prev.ctypes.data, prev.size)
        return prev

    write_png = L.FrameEncoder.write
