"""ms per frame of the surface reconstruction with anisotropic kernels beside the isotropic one, on C2
(product.c2_scene(), 1.23 M particles), from rest and again after the in-motion steps of the bench line (2500).  Two reconstruction
objects on the same live handle, one per mode; per state one untimed frame each, then --frames rounds in which the isotropic and the
anisotropic frame alternate on the same particles.  Per state one JSON line per mode (the stage times of the best frame by events, the
median beside it; pair tests, triangles, bytes held, ns per candidate test of the field kernel) and one line of ratios anisotropic /
isotropic.  The kernels' registers, LDS and occupancy come from the build's resource remarks (csrc/build/kernels_strict.resources)."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.surface import SurfaceReconstructor  # noqa: E402


def kernel_resources(build):
    """{kernel: (VGPRs, LDS bytes, waves / SIMD)} of the k_surf_field* and k_surf_aniso* kernels, or {} without a build directory"""
    path = os.path.join(ROOT, "sph_project_amd", "csrc", "build", f"kernels_{build}.resources")
    if not os.path.exists(path):
        return {}
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            name = name if re.search(r"k_surf_(field|aniso|normals|volume)", name) else None
            if name:
                out[name] = {}
        elif name:
            for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, line)
                if m:
                    out[name][key] = int(m.group(1))
    return out


def one_frame(r, eng, obj):
    eng.synchronize()
    t0 = time.perf_counter()
    rc = r.lib.sph_surface_reconstruct_object(r.h, eng.h, obj)
    host = 1e3 * (time.perf_counter() - t0)
    assert rc == 0, rc
    st = r.stats()
    st.update(host=host, **{"aniso_" + k: v for k, v in r.anisotropy_stats().items()})
    return st


def summary(label, step, mode, frames):
    best = min(frames, key=lambda s: s["ms_total"])
    med = sorted(s["ms_total"] for s in frames)[len(frames) // 2]
    out = dict(state=label, step=step, mode=mode, frames=len(frames), particles=best["particles"], B=best["B"],
               ms_per_frame_events=round(best["ms_total"], 3), ms_per_frame_events_median=round(med, 3),
               ms_per_frame_host=round(min(s["host"] for s in frames), 3),
               ms_bin=round(best["ms_bin"], 3), ms_bricks=round(best["ms_bricks"], 3), ms_field=round(best["ms_field"], 3),
               ms_mesh=round(best["ms_mesh"], 3), ms_normals=round(best["ms_normals"], 3),
               active_bricks=best["active_bricks"], points=best["points_evaluated"], pair_tests=best["pair_tests"],
               vertices=best["vertices"], triangles=best["triangles"], bytes_allocated=best["bytes_allocated"],
               field_ns_per_candidate_test=1e6 * best["ms_field"] / best["pair_tests"] if best["pair_tests"] else 0.0,
               identical_frames=all(s["triangles"] == best["triangles"] and s["vertices"] == best["vertices"] for s in frames))
    if mode == "anisotropic":
        out.update(ms_moments=round(best["aniso_ms_moments"], 3), ms_volume=round(best["aniso_ms_volume"], 3),
                   sparse_particles=best["aniso_sparse_particles"], clamped_particles=best["aniso_clamped_particles"])
    print(json.dumps(out), flush=True)
    return out


def measure(iso, ani, container, obj, frames, label, step):
    eng = container.engine
    one_frame(iso, eng, obj)   # untimed: allocations, first touch
    one_frame(ani, eng, obj)
    fi, fa = [], []
    for _ in range(frames):
        fi.append(one_frame(iso, eng, obj))
        fa.append(one_frame(ani, eng, obj))
    a, b = summary(label, step, "isotropic", fi), summary(label, step, "anisotropic", fa)
    keys = ("ms_per_frame_events", "ms_bin", "ms_field", "ms_mesh", "ms_normals", "triangles", "bytes_allocated", "field_ns_per_candidate_test")
    print(json.dumps(dict(state=label, ratio_anisotropic_to_isotropic={k: round(b[k] / a[k], 3) for k in keys if a[k]})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--fast-math", action="store_true")
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--min-neighbours", type=int, default=25)
    ap.add_argument("--sparse-scale", type=float, default=0.5)
    a = ap.parse_args()
    build = "fast" if a.fast_math else "strict"
    print(json.dumps(dict(build=build, kernels=kernel_resources(build))), flush=True)
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    (obj,) = tuple(container.object_id_fluid_body)
    iso = SurfaceReconstructor(container.dx, fast_math=a.fast_math)
    ani = SurfaceReconstructor(container.dx, fast_math=a.fast_math)
    ani.set_anisotropy(max_ratio=a.ratio, min_neighbours=a.min_neighbours, sparse_scale=a.sparse_scale)
    measure(iso, ani, container, obj, a.frames, "rest", 0)
    if a.motion_step > 0:
        container.engine.step(a.motion_step)
        container.engine.synchronize()
        measure(iso, ani, container, obj, a.frames, "in_motion", a.motion_step)


if __name__ == "__main__":
    main()
