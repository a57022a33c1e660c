"""ms per frame of the traced mesh frames on C2 (product.c2_scene(), 1.23 M particles) at the reference's camera and
1024^2 with the domain box (so the floor is there), from rest and again after the in-motion steps of the bench line (2500).  Per state
the fluid surface is reconstructed once with the reference's settings (smoothing 25 / weights on / normalization 13 / normal smoothing
10); then, from the surface object (device to device), one untimed and --frames timed raster frames and one untimed and
--frames timed traced frames with the fluid as water.  Reports the medians of the stage times from HIP events, rays per second of the
trace stage, node visits and triangle tests per ray, and -- measured in the same process -- the raster frame and the reconstruction
with post-processing.  One JSON line per state."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.render import FrameRenderer  # noqa: E402
from sph_project_amd.surface import SurfaceReconstructor  # noqa: E402

STAGES = ("ms_setup", "ms_sort", "ms_hierarchy", "ms_fit", "ms_trace", "ms_finish", "ms_total")


def median(values):
    return sorted(values)[len(values) // 2]


def measure(r, recon, container, frames, label, step, trace_kw):
    recon.from_container(container, 0)   # untimed: allocations
    recon.from_container(container, 0)
    ss, ps = recon.stats(), recon.post_stats()
    r.clear_trace()
    r.from_meshes([(recon, (50, 100, 200))], download=False)
    raster = []
    for _ in range(frames):
        r.from_meshes([(recon, (50, 100, 200))], download=False)
        raster.append(r.mesh_stats()["ms_total"])
    r.set_trace(**trace_kw)
    r.from_meshes([(recon, (50, 100, 200), "water")], download=False)   # untimed: the mode's buffers, first touch
    stats = []
    for _ in range(frames):
        r.from_meshes([(recon, (50, 100, 200), "water")], download=False)
        stats.append(r.trace_stats())
    st = stats[0]
    rays = st["rays_primary"] + st["rays_path"] + st["rays_reflect"] + st["rays_shadow"]
    out = dict(state=label, step=step, triangles=st["triangles"], nodes=st["nodes"], depth=st["depth"], frames=frames, width=r.width,
               height=r.height, **{k: round(median([s[k] for s in stats]), 4) for k in STAGES})
    out.update(rays=rays, rays_primary=st["rays_primary"], rays_path=st["rays_path"], rays_reflect=st["rays_reflect"],
               rays_shadow=st["rays_shadow"], truncated=st["truncated"], aborted_rays=st["aborted_rays"],
               Mrays_per_s=round(rays / (1e3 * max(out["ms_trace"], 1e-9)), 1),
               node_visits_per_ray=round(st["node_visits"] / max(rays, 1), 1), triangle_tests_per_ray=round(st["triangle_tests"] / max(rays, 1), 2),
               raster_frame_ms=round(median(raster), 4), reconstruct_ms_events=round(ss["ms_total"] + ps["ms_total"], 2),
               traced_frame_below_reconstruction=bool(out["ms_total"] < ss["ms_total"] + ps["ms_total"]))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--fast-math", action="store_true")
    a = ap.parse_args()
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    box = (np.zeros(3), np.asarray(container.domain_end, dtype=np.float64))
    r = FrameRenderer(container.dx, width=a.size, height=a.size, box=box, fast_math=a.fast_math)
    recon = SurfaceReconstructor(container.dx, fast_math=a.fast_math)
    recon.set_postprocess(mesh_smoothing_iters=25, mesh_smoothing_weights=True, weights_normalization=13.0, normals_smoothing_iters=10)
    kw = dict(max_depth=6, ior=1.33, absorb=0.05)
    measure(r, recon, container, a.frames, "rest", 0, kw)
    if a.motion_step > 0:
        container.engine.step(a.motion_step)
        container.engine.synchronize()
        measure(r, recon, container, a.frames, "in_motion", a.motion_step, kw)


if __name__ == "__main__":
    main()
