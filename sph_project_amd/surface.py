"""Surface reconstruction on the GPU: fluid particles -> triangle mesh (C-ABI sph_surface_* in include/sph_hip.h).

Replaces the reference's `splashsurf reconstruct` call (surface_reconstruction.py:8) with the project's own method: a Shepard colour
field of the project's cubic spline and marching cubes, evaluated by the HIP passes of csrc/sph_surface.hpp.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L

SPH_ERR_CAPACITY = L.ERR_CAPACITY


class SurfaceError(L.SphError):
    pass


class SurfaceReconstructor(L.NativeObject):
    """One reconstruction object (device buffers reused from frame to frame).  Defaults: the reference's splashsurf command
    (`-l 3.5 -c=0.5 -t=0.6 --normals=on`)."""
    ABI, Error = "sph_surface", SurfaceError

    def __init__(self, radius, smoothing_length=3.5, cube_size=0.5, iso=0.6, normals=True, memory_cap_bytes=0, fast_math=False,
                 device=-1):
        super().__init__()
        self.normals = bool(normals)
        p = L.SphSurfaceParams(radius=float(radius), smoothing_length=float(smoothing_length), cube_size=float(cube_size), iso=float(iso),
                               normals=int(self.normals), fast_math=int(bool(fast_math)), device=int(device), reserved=0,
                               memory_cap_bytes=int(memory_cap_bytes))
        self.h = self._create(p)
        self.mesh = None
        self._on_device_only = False   # the last reconstruction was not downloaded (download=False)

    def _finish(self, download):
        """the mesh of the reconstruction just made, or with download=False None: it stays on the device (FrameRenderer.from_meshes
        and TextExporter.obj_surface read it there)"""
        self._on_device_only = not download
        if download:
            return self._download()
        self.mesh = None
        return None

    def _download(self):
        nv, nt = C.c_int64(), C.c_int64()
        self._chk(self.lib.sph_surface_mesh_size(self.h, C.byref(nv), C.byref(nt)), "sph_surface_mesh_size")
        v = np.empty((nv.value, 3), np.float32)
        n = np.empty((nv.value, 3), np.float32) if self.normals else None
        t = np.empty((nt.value, 3), np.int32)
        self._chk(self.lib.sph_surface_download(self.h, v.ctypes.data, None if n is None else n.ctypes.data, t.ctypes.data),
                  "sph_surface_download")
        self.mesh = (v, t, n)
        return self.mesh

    def from_points(self, xyz, download=True):
        """(vertices f32[nv,3], triangles i32[nt,3], normals f32[nv,3] or None) of the particles xyz f32[n,3]; download=False: None,
        the mesh stays on the device."""
        x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._chk(self.lib.sph_surface_reconstruct(self.h, x.ctypes.data, x.shape[0]), "sph_surface_reconstruct")
        return self._finish(download)

    def from_container(self, container, obj_id, download=True):
        """The same for object obj_id of a live container (or an Engine), compacted on the device."""
        engine = getattr(container, "engine", container)
        self._chk(self.lib.sph_surface_reconstruct_object(self.h, engine.h, int(obj_id)), "sph_surface_reconstruct_object")
        return self._finish(download)

    def stats(self):
        st = L.SphSurfaceStats()
        self._chk(self.lib.sph_surface_stats(self.h, C.byref(st)), "sph_surface_stats")
        return L.struct_dict(st, skip=("reserved",))

    def set_postprocess(self, mesh_smoothing_iters=0, mesh_smoothing_weights=False, weights_normalization=13.0, normals_smoothing_iters=0):
        """Smoothing of the reconstructions that follow (splashsurf's --mesh-smoothing-iters, --mesh-smoothing-weights,
        --mesh-smoothing-weights-normalization, --normals-smoothing-iters).  All zero: off (the default)."""
        p = L.SphSurfacePostParams(mesh_smoothing_iters=int(mesh_smoothing_iters), mesh_smoothing_weights=int(bool(mesh_smoothing_weights)),
                                   weights_normalization=float(weights_normalization), normals_smoothing_iters=int(normals_smoothing_iters),
                                   reserved=0)
        self._chk(self.lib.sph_surface_set_postprocess(self.h, C.byref(p)), "sph_surface_set_postprocess")

    def post_stats(self):
        st = L.SphSurfacePostStats()
        self._chk(self.lib.sph_surface_post_stats(self.h, C.byref(st)), "sph_surface_post_stats")
        return L.struct_dict(st, skip=("reserved",))

    def adjacency(self):
        """(offsets i32[nv+1], neighbours i32[offsets[-1]]): the vertex adjacency (CSR) of the last reconstruction's smoothing."""
        nv = self._post_size()
        off = np.empty(nv + 1, np.int32)
        self._chk(self.lib.sph_surface_download_post(self.h, off.ctypes.data, None, None), "sph_surface_download_post")
        nb = np.empty(int(off[-1]), np.int32)
        self._chk(self.lib.sph_surface_download_post(self.h, None, nb.ctypes.data, None), "sph_surface_download_post")
        return off, nb

    def smoothing_weights(self):
        """w f32[nv] of the last reconstruction's smoothing (all 1 without mesh_smoothing_weights)."""
        w = np.empty(self._post_size(), np.float32)
        self._chk(self.lib.sph_surface_download_post(self.h, None, None, w.ctypes.data), "sph_surface_download_post")
        return w

    def set_anisotropy(self, max_ratio=2.0, min_neighbours=25, sparse_scale=0.5):
        """Anisotropic kernels for the reconstructions that follow: every particle's kernel shrinks, by at most
        max_ratio, along the directions in which its neighbourhood is thin; a particle with fewer than min_neighbours neighbours
        gets the support sparse_scale h.  Off by default; clear_anisotropy() switches it off again."""
        p = L.SphSurfaceAnisoParams(enabled=1, min_neighbours=int(min_neighbours), max_ratio=float(max_ratio),
                                    sparse_scale=float(sparse_scale))
        self._chk(self.lib.sph_surface_set_anisotropy(self.h, C.byref(p)), "sph_surface_set_anisotropy")

    def clear_anisotropy(self):
        self._chk(self.lib.sph_surface_set_anisotropy(self.h, None), "sph_surface_set_anisotropy")

    def anisotropy(self):
        """The last (anisotropic) reconstruction's particles in the binned key order: dict of xyz f32[n,3], A f32[n,6] = (xx, xy, xz,
        yy, yz, zz) of the kernel matrices, neighbours i32[n], V f32[n]."""
        n = self.stats()["particles"]
        out = dict(xyz=np.empty((n, 3), np.float32), A=np.empty((n, 6), np.float32), neighbours=np.empty(n, np.int32),
                   V=np.empty(n, np.float32))
        self._chk(self.lib.sph_surface_download_anisotropy(self.h, out["xyz"].ctypes.data, out["A"].ctypes.data,
                                                           out["neighbours"].ctypes.data, out["V"].ctypes.data),
                  "sph_surface_download_anisotropy")
        return out

    def anisotropy_stats(self):
        st = L.SphSurfaceAnisoStats()
        self._chk(self.lib.sph_surface_anisotropy_stats(self.h, C.byref(st)), "sph_surface_anisotropy_stats")
        return L.struct_dict(st)

    def _post_size(self):
        nv, nt = C.c_int64(), C.c_int64()
        self._chk(self.lib.sph_surface_mesh_size(self.h, C.byref(nv), C.byref(nt)), "sph_surface_mesh_size")
        return nv.value

    def write_obj(self, path):
        """The last mesh as ASCII OBJ (write_obj below)."""
        if self.mesh is None and self._on_device_only:
            raise SurfaceError("write_obj: the last reconstruction was made with download=False and its mesh is on the device only; "
                               "write it with sph_project_amd.text.TextExporter.obj_surface(reconstructor)", L.ERR_INVALID)
        if self.mesh is None:
            raise SurfaceError("write_obj: no mesh reconstructed yet", L.ERR_INVALID)
        write_obj(path, *self.mesh)


def aniso_matrix_host(C6, neighbours=None, max_ratio=2.0, min_neighbours=25, sparse_scale=0.5):
    """A f32[n,6] from covariances C6 f32[n,6] by the device's eigen and clamp routine, run on the host (no GPU)."""
    c = np.ascontiguousarray(C6, dtype=np.float32).reshape(-1, 6)
    nb = None if neighbours is None else np.ascontiguousarray(neighbours, dtype=np.int32).reshape(-1)
    if nb is not None and len(nb) != len(c):
        raise ValueError("aniso_matrix_host: one neighbour count per matrix")
    p = L.SphSurfaceAnisoParams(enabled=1, min_neighbours=int(min_neighbours), max_ratio=float(max_ratio), sparse_scale=float(sparse_scale))
    out = np.empty_like(c)
    rc = L.load().sph_surface_aniso_matrix_host(c.ctypes.data, len(c), None if nb is None else nb.ctypes.data, C.byref(p), out.ctypes.data)
    if rc != 0:
        raise SurfaceError(f"sph_surface_aniso_matrix_host: invalid parameters ({rc})", rc)
    return out


def write_obj(path, vertices, triangles, normals=None):
    """v / vn / `f a//a b//b c//c` (1-based) in the PLY writer's number format, by the native writer (sph_write_obj_ascii)."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    rc = L.load().sph_write_obj_ascii(os.fsencode(path), v.ctypes.data, v.shape[0], None if n is None else n.ctypes.data,
                                      t.ctypes.data, t.shape[0])
    if rc != 0:
        raise OSError(f"sph_write_obj_ascii({path!r}) failed ({rc})")
