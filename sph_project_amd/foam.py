"""Diffuse particles on the GPU: spray, foam and bubbles generated from the fluid state (C-ABI sph_foam_* in
include/sph_hip.h).

A second, one-way-coupled particle set after Ihmsen, Akinci, Akinci, Teschner, "Unified spray, foam and bubbles for particle-based
fluids" (2012), evaluated by the HIP passes of csrc/sph_foam.hpp.  The reference has nothing of the kind.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

# the starting values of DESIGN.md 26 (every one a field of SphFoamParams)
DEFAULTS = dict(padding=None, ta_min=5.0, ta_max=20.0, wc_min=2.0, wc_max=8.0, e_min=2.0, e_max=20.0, k_ta=1000.0, k_wc=5000.0,
                life_min=2.0, life_max=5.0, k_b=2.0, k_d=0.8, normal_min=0.5, n_spray=6, n_bubble=20, max_per_particle=8,
                max_diffuse=0, seed=0, fast_math=False, device=-1)
CLASS_NAMES = ("spray", "foam", "bubble", "born")


class FoamError(L.SphError):
    pass


class DiffuseParticles(L.NativeObject):
    """One diffuse particle set over a domain [domain_lo, domain_hi].  params: the keys of DEFAULTS (padding None: the support
    radius 4 radius, the margin at which the containers clamp the fluid; max_diffuse 0: twice the fluid capacity seen at the first step)."""
    ABI, Error = "sph_foam", FoamError

    def __init__(self, radius, domain_lo, domain_hi, gravity=(0.0, -9.81, 0.0), **params):
        super().__init__()
        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"DiffuseParticles: unknown parameter(s) {sorted(unknown)}")
        kw = dict(DEFAULTS, **params)
        if kw["padding"] is None:
            kw["padding"] = 4.0 * float(radius)
        p = L.SphFoamParams()
        p.radius = float(radius)
        p.domain_lo[:] = [float(v) for v in domain_lo]
        p.domain_hi[:] = [float(v) for v in domain_hi]
        p.gravity[:] = [float(v) for v in gravity]
        for k in ("padding", "ta_min", "ta_max", "wc_min", "wc_max", "e_min", "e_max", "k_ta", "k_wc", "life_min", "life_max", "k_b", "k_d",
                  "normal_min"):
            setattr(p, k, float(kw[k]))
        for k in ("n_spray", "n_bubble", "max_per_particle", "max_diffuse", "seed", "device"):
            setattr(p, k, int(kw[k]))
        p.fast_math = int(bool(kw["fast_math"]))
        p.reserved = 0
        self.params = kw
        self.h = self._create(p)
        self._n_fluid = 0

    def step(self, container_or_engine, dt):
        """One step of length dt from the active fluid particles of a live container (or an Engine), read on the device."""
        engine = getattr(container_or_engine, "engine", container_or_engine)
        self._chk(self.lib.sph_foam_step_handle(self.h, engine.h, float(dt)), "sph_foam_step_handle")
        self._n_fluid = self.stats()["fluid"]

    def step_points(self, xyz, vel, ids, dt):
        """The same from host arrays: xyz f32[n,3], vel f32[n,3], ids i32[n] (distinct)."""
        x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        v = np.ascontiguousarray(vel, dtype=np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if not (len(x) == len(v) == len(i)):
            raise ValueError("step_points: xyz, vel and ids must have one row per particle")
        self._chk(self.lib.sph_foam_step_points(self.h, x.ctypes.data, v.ctypes.data, i.ctypes.data, len(x), float(dt)), "sph_foam_step_points")
        self._n_fluid = len(x)

    def seed(self, xyz, vel, life):
        """Diffuse particles of the caller's own; their keys are 2^63 | serial number."""
        x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        v = np.ascontiguousarray(vel, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(life, dtype=np.float32).reshape(-1)
        if not (len(x) == len(v) == len(t)):
            raise ValueError("seed: xyz, vel and life must have one row per particle")
        self._chk(self.lib.sph_foam_seed(self.h, x.ctypes.data, v.ctypes.data, t.ctypes.data, len(x)), "sph_foam_seed")

    def count(self):
        n = C.c_int64()
        self._chk(self.lib.sph_foam_count(self.h, C.byref(n)), "sph_foam_count")
        return n.value

    def download(self, sort=True):
        """dict(x f32[n,3], v f32[n,3], life f32[n], key u64[n], cls i32[n]) of the diffuse set, sorted by key (sort=False: in the
        device's order)."""
        n = self.count()
        out = dict(x=np.empty((n, 3), np.float32), v=np.empty((n, 3), np.float32), life=np.empty(n, np.float32),
                   key=np.empty(n, np.uint64), cls=np.empty(n, np.int32))
        self._chk(self.lib.sph_foam_download(self.h, *(out[k].ctypes.data for k in ("x", "v", "life", "key", "cls"))), "sph_foam_download")
        if sort and n:
            o = np.argsort(out["key"], kind="stable")
            out = {k: np.ascontiguousarray(a[o]) for k, a in out.items()}
        return out

    def potentials(self):
        """dict(ta, wc, e, nd f32[n], normal f32[n,3], ids i32[n]) of the last step's fluid particles: in input order after
        step_points, in the container's order (active fluid only) after step."""
        n = self._n_fluid
        out = dict(ta=np.zeros(n, np.float32), wc=np.zeros(n, np.float32), e=np.zeros(n, np.float32), nd=np.zeros(n, np.float32),
                   normal=np.zeros((n, 3), np.float32), ids=np.zeros(n, np.int32))
        self._chk(self.lib.sph_foam_download_potentials(self.h, *(out[k].ctypes.data for k in ("ta", "wc", "e", "nd", "normal", "ids"))),
                  "sph_foam_download_potentials")
        return out

    def stats(self):
        st = L.SphFoamStats()
        self._chk(self.lib.sph_foam_stats(self.h, C.byref(st)), "sph_foam_stats")
        d = L.struct_dict(st)
        d["pairs_visited"] = list(st.pairs_visited)
        d["pairs_accepted"] = list(st.pairs_accepted)
        return d

    def clear(self):
        self._chk(self.lib.sph_foam_clear(self.h), "sph_foam_clear")
