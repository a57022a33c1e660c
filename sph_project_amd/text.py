"""Frame exports formatted on the GPU: particles -> ASCII PLY, meshes -> ASCII OBJ (C-ABI sph_text_* in include/sph_hip.h).

Stands in for a download followed by the host writers (run_simulation.write_ply_ascii, surface.write_obj): HIP passes turn the device
state into the files' characters -- the same bytes as sph_write_ply_ascii / sph_write_obj_ascii -- and the host only copies finished
text into the file.  No CPU fallback for the exporter (the host writers remain what the drivers use without --export_device)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L


class TextError(L.SphError):
    pass


class TextExporter(L.NativeObject):
    """One exporter (device and pinned buffers reused from file to file).  Bind a source with ply_points / ply_object / obj_mesh /
    obj_surface, then write(path) or bytes() produce its file, piece_rows rows at a time (0: about 2^20)."""
    ABI, Error = "sph_text", TextError

    def __init__(self, piece_rows=0, fast_math=False, device=-1):
        super().__init__()
        p = L.SphTextParams(piece_rows=int(piece_rows), fast_math=int(bool(fast_math)), device=int(device), reserved=0)
        self.h = self._create(p)
        self._keep = None   # the object whose device memory the bound source reads in place

    def ply_points(self, xyz):
        """PLY of the points xyz f32[n,3] (uploaded)."""
        x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._keep = None
        self._chk(self.lib.sph_text_ply_points(self.h, x.ctypes.data, x.shape[0]), "sph_text_ply_points")
        return self

    def ply_object(self, container, obj_id):
        """PLY of object obj_id of a live container (or an Engine): its particles in the order of container.dump(obj_id)["position"],
        compacted on the device."""
        engine = getattr(container, "engine", container)
        self._keep = None
        self._chk(self.lib.sph_text_ply_object(self.h, engine.h, int(obj_id)), "sph_text_ply_object")
        return self

    def obj_mesh(self, v, t, n=None):
        """OBJ of a host mesh: vertices f32[nv,3], triangles i32[nt,3] (0-based), normals f32[nv,3] or None."""
        v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)
        n = None if n is None else np.ascontiguousarray(n, dtype=np.float32).reshape(-1, 3)
        if n is not None and n.shape != v.shape:
            raise ValueError(f"obj_mesh: {n.shape[0]} normals for {v.shape[0]} vertices")
        self._keep = None
        self._chk(self.lib.sph_text_obj_mesh(self.h, v.ctypes.data, v.shape[0], None if n is None else n.ctypes.data, t.ctypes.data,
                                             t.shape[0]), "sph_text_obj_mesh")
        return self

    def obj_surface(self, reconstructor):
        """OBJ of a SurfaceReconstructor's last mesh, read where it lies on the device (from_points / from_container with
        download=False leave it there).  The reconstructor must not reconstruct again before the file has been produced."""
        self._keep = None
        self._chk(self.lib.sph_text_obj_surface(self.h, reconstructor.h), "sph_text_obj_surface")
        self._keep = reconstructor
        return self

    def write(self, path):
        """{path} <- the file of the bound source"""
        self._chk(self.lib.sph_text_write(self.h, os.fsencode(path)), "sph_text_write")

    def bytes(self):
        """The same file in memory."""
        n = C.c_int64()
        self._chk(self.lib.sph_text_size(self.h, C.byref(n)), "sph_text_size")
        buf = np.empty(max(n.value, 1), np.uint8)
        self._chk(self.lib.sph_text_read(self.h, buf.ctypes.data, n.value), "sph_text_read")
        return buf[:n.value].tobytes()

    def stats(self):
        """rows, values, bytes, pieces, longest_row and the stage times (ms) of the last write() / bytes()"""
        st = L.SphTextStats()
        self._chk(self.lib.sph_text_stats(self.h, C.byref(st)), "sph_text_stats")
        return L.struct_dict(st)


def format_f32_host(values):
    """The device's number routine run on the host (sph_text_format_f32_host): the list of the values' texts as bytes.  For tests."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    out = np.empty(max(19 * v.shape[0], 1), np.uint8)
    lengths = np.empty(max(v.shape[0], 1), np.int64)
    lib = L.load()
    rc = lib.sph_text_format_f32_host(v.ctypes.data, v.shape[0], out.ctypes.data, 19 * v.shape[0], lengths.ctypes.data)
    if rc != 0:
        raise TextError(f"sph_text_format_f32_host failed ({rc}): " + (lib.sph_text_last_error(None) or b"").decode(), rc)
    raw = out.tobytes()
    ends = np.cumsum(lengths[:v.shape[0]])
    return [raw[e - l:e] for e, l in zip(ends.tolist(), lengths[:v.shape[0]].tolist())]
