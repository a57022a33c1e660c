"""ms per frame of the screen-space surface mode on C2 (product.c2_scene(), 1.23 M particles) at the reference's camera and
1024^2, strict build, from rest and again after the in-motion steps of the bench line (2500).  Per state: one untimed frame, then
--frames timed frames, each the whole from_container + surface() from the live handle (both synchronous, nothing downloaded).  Reports
the medians of the stage times from HIP events (the particle frame's total; base, smooth, shade of the surface passes), of the host
clock around the two calls, and the counters: surface pixels, window taps visited and accepted, pixels clamped at rmax.  One JSON line
per state, also written to --out (default profiles/render_surface_bench_c2.txt).
Set against: the particle frame (profiles/render_bench_c2.txt) and the surface by reconstruction (profiles/render_mesh_bench_c2.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.render import FrameRenderer  # noqa: E402


def measure(r, container, frames, label, step):
    eng = container.engine
    r.from_container(container, download=False)   # untimed: allocations, first touch
    r.surface(download=False)
    host, frame, surf = [], [], []
    for _ in range(frames):
        eng.synchronize()
        t0 = time.perf_counter()
        r.from_container(container, download=False)
        r.surface(download=False)
        host.append(1e3 * (time.perf_counter() - t0))
        frame.append(r.stats())
        surf.append(r.surface_stats())
    med = lambda rows, key: round(sorted(s[key] for s in rows)[frames // 2], 3)  # noqa: E731
    st = surf[-1]
    out = dict(state=label, step=step, particles=frame[-1]["particles"], drawn=frame[-1]["drawn"], frames=frames, width=r.width, height=r.height,
               ms_particle_frame=med(frame, "ms_total"), ms_base=med(surf, "ms_base"), ms_smooth=med(surf, "ms_smooth"),
               ms_shade=med(surf, "ms_shade"),
               ms_surface_passes=round(med(surf, "ms_base") + med(surf, "ms_smooth") + med(surf, "ms_shade"), 3),
               ms_host_frame_and_surface=round(sorted(host)[frames // 2], 3), ms_host_min=round(min(host), 3),
               covered_pixels=frame[-1]["covered_pixels"], surface_pixels=st["surface_pixels"], iterations=st["iterations"],
               taps_visited=st["taps_visited"], taps_accepted=st["taps_accepted"], clamped_rmax=st["clamped_rmax"],
               taps_per_surface_pixel_per_iteration=round(st["taps_visited"] / max(st["surface_pixels"] * max(st["iterations"], 1), 1), 1),
               identical_counters=all({k: s[k] for k in ("surface_pixels", "taps_visited", "taps_accepted", "clamped_rmax")} ==
                                      {k: st[k] for k in ("surface_pixels", "taps_visited", "taps_accepted", "clamped_rmax")} for s in surf))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--fast-math", action="store_true")
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_surface_bench_c2.txt"))
    a = ap.parse_args()
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    r = FrameRenderer(container.dx, fast_math=a.fast_math)
    r.set_surface(iterations=a.iterations)
    rows = [measure(r, container, a.frames, "rest", 0)]
    if a.motion_step > 0:
        container.engine.step(a.motion_step)
        container.engine.synchronize()
        rows.append(measure(r, container, a.frames, "in_motion", a.motion_step))
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"python tools/bench_render_surface.py --frames {a.frames}   (MI355X, {'fast' if a.fast_math else 'strict'} build; one JSON line per state)\n")
            f.write("product.c2_scene() (WCSPH, 1,231,200 particles), reference camera, 1024 x 1024, surface mode at its defaults "
                    f"(iterations {a.iterations}): from rest, then after engine.step({a.motion_step}); medians of {a.frames} frames\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
