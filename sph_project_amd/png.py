"""PNG files on the GPU: RGB frames -> lossless 8-bit RGB .png files (C-ABI sph_png_* in include/sph_hip.h).

Stands in for the zlib pass of render.encode_png over a downloaded frame: row filters, LZ77 tokens, the fixed Huffman code (or, with
coding="dynamic", per segment a dynamic Huffman block where that is shorter: smaller files, a slower count pass), Adler-32 and the chunk
CRCs are computed by the HIP passes of csrc/sph_png.hpp where a rendered frame already lies, and only the finished file
crosses to the host.  No CPU fallback for the encoder (render.encode_png remains what the drivers use without --png_device)."""
from __future__ import annotations

import ctypes as C

import numpy as np

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


CODINGS = {"fixed": L.PNG_CODING_FIXED, "dynamic": L.PNG_CODING_DYNAMIC}


def _coding(c):
    if not isinstance(c, str) or c not in CODINGS:
        raise ValueError(f"coding must be 'fixed' or 'dynamic', not {c!r}")
    return CODINGS[c]


def bound(width, height, filter="adaptive"):
    """The longest file PngEncoder(width, height) can return in either coding (sph_png_bound: host only)."""
    p = L.SphPngParams(width=int(width), height=int(height), filter=_filter(filter), fast_math=0, device=-1, reserved=0)
    n = C.c_int64()
    lib = L.load()
    if lib.sph_png_bound(C.byref(p), C.byref(n)) != 0:
        raise PngError("sph_png_bound failed: " + (lib.sph_png_last_error(None) or b"").decode(), L.ERR_INVALID)
    return n.value


class PngEncoder(L.NativeObject):
    """One PNG encoder for frames of one size.  The bytes of a file depend on (pixels, width, height, filter, coding) alone; a file in
    coding "dynamic" is never longer than the "fixed" one of the same picture."""
    ABI, Error = "sph_png", PngError

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

    def _need_open(self, what):
        if self.h is None:
            raise PngError(f"{what}: the encoder is closed", L.ERR_INVALID)

    def set_coding(self, coding):
        """"fixed" | "dynamic": the entropy coding of the encodes that follow"""
        code = _coding(coding)
        self._need_open("set_coding")
        self._chk(self.lib.sph_png_set_coding(self.h, code), "sph_png_set_coding")
        self.coding = coding

    def _download(self):
        self._need_open("download")
        n = C.c_int64()
        self._chk(self.lib.sph_png_size(self.h, C.byref(n)), "sph_png_size")
        buf = np.empty(n.value, np.uint8)
        self._chk(self.lib.sph_png_download(self.h, buf.ctypes.data), "sph_png_download")
        return buf.tobytes()

    def encode(self, rgb):
        """The .png file of uint8 (height, width, 3)."""
        self._need_open("encode")
        a = np.ascontiguousarray(rgb, dtype=np.uint8)
        if a.shape != (self.height, self.width, 3):
            raise ValueError(f"encode: expected ({self.height}, {self.width}, 3), got {a.shape}")
        self._chk(self.lib.sph_png_encode_rgb(self.h, a.ctypes.data), "sph_png_encode_rgb")
        return self._download()

    def encode_last(self, frame_renderer):
        """The .png file of a FrameRenderer's last frame (particles or meshes), read from its device buffer."""
        self._need_open("encode_last")
        if frame_renderer._last is None:
            raise PngError("encode_last: the renderer holds no frame", L.ERR_INVALID)
        self._chk(self.lib.sph_png_encode_render(self.h, frame_renderer._last), "sph_png_encode_render")
        return self._download()

    def stats(self):
        self._need_open("stats")
        st = L.SphPngStats()
        self._chk(self.lib.sph_png_stats(self.h, C.byref(st)), "sph_png_stats")
        out = L.struct_dict(st)
        out["filter_rows"] = list(st.filter_rows)
        return out

    def write_png(self, path, frame_renderer):
        """{path} <- the renderer's last frame; the pixels never reach the host."""
        with open(path, "wb") as f:
            f.write(self.encode_last(frame_renderer))
