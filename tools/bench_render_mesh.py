"""ms per frame of the mesh renderer on C2 (product.c2_scene(), 1.23 M particles) at the reference's camera and 1024^2,
from rest and again after the in-motion steps of the bench line (2500).  Per state the fluid surface is reconstructed once with the
reference's settings (smoothing 25 / weights on / normalization 13 / normal smoothing 10), then one untimed mesh frame and --frames timed
ones are drawn from the surface object (device to device).  Reports the stage times from HIP events (best and median with the spread),
the host clock around the whole from_meshes call, the triangles that reach no pixel centre, atomics per covered pixel, the depth pass's
gather rate at 48 B per triangle, and -- measured in the same process -- what the frame costs already: the reconstruction with
post-processing and the PNG encode.  One JSON line per state."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.render import FrameRenderer, encode_png  # noqa: E402
from sph_project_amd.surface import SurfaceReconstructor  # noqa: E402


def measure(r, recon, container, frames, label, step):
    recon.from_container(container, 0)   # untimed: allocations
    t0 = time.perf_counter()
    recon.from_container(container, 0)
    recon_host = 1e3 * (time.perf_counter() - t0)
    ss, ps = recon.stats(), recon.post_stats()
    rgb = r.from_meshes([(recon, (50, 100, 200))])   # untimed: list buffers, first touch
    host, stats = [], []
    for _ in range(frames):
        t0 = time.perf_counter()
        r.from_meshes([(recon, (50, 100, 200))])
        host.append(1e3 * (time.perf_counter() - t0))
        stats.append(r.mesh_stats())
    t0 = time.perf_counter()
    png = encode_png(rgb)
    png_ms = 1e3 * (time.perf_counter() - t0)
    srt = lambda key: sorted(s[key] for s in stats)  # noqa: E731
    st = stats[0]
    out = dict(state=label, step=step, triangles=st["triangles"], vertices=st["vertices"], frames=frames, width=r.width, height=r.height)
    for key in ("ms_depth", "ms_shade", "ms_finish", "ms_total"):
        v = srt(key)
        out[key] = dict(min=round(v[0], 4), median=round(v[frames // 2], 4), max=round(v[-1], 4))
    out.update(ms_host_from_meshes_median=round(sorted(host)[frames // 2], 3),
               hit=st["hit"], share_without_a_pixel_centre=round(1.0 - st["hit"] / max(st["triangles"], 1), 4), large=st["large"],
               covered_pixels=st["covered_pixels"], atomics=st["atomics"],
               atomics_per_covered_pixel=round(st["atomics"] / max(st["covered_pixels"], 1), 3),
               depth_gather_GBps=round(48.0 * st["triangles"] / (1e6 * max(srt("ms_depth")[frames // 2], 1e-9)), 1),
               reconstruct_ms_events=round(ss["ms_total"] + ps["ms_total"], 2), reconstruct_ms_host=round(recon_host, 2),
               png_encode_ms=round(png_ms, 1), png_bytes=len(png))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--fast-math", action="store_true")
    a = ap.parse_args()
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    r = FrameRenderer(container.dx, fast_math=a.fast_math)
    recon = SurfaceReconstructor(container.dx, fast_math=a.fast_math)
    recon.set_postprocess(mesh_smoothing_iters=25, mesh_smoothing_weights=True, weights_normalization=13.0, normals_smoothing_iters=10)
    measure(r, recon, container, a.frames, "rest", 0)
    if a.motion_step > 0:
        container.engine.step(a.motion_step)
        container.engine.synchronize()
        measure(r, recon, container, a.frames, "in_motion", a.motion_step)


if __name__ == "__main__":
    main()
