"""ms per frame of the thickness mode of the surface frames on C2 (product.c2_scene(), 1.23 M particles) at the reference's
camera and 1024^2, strict build, defaults, from rest and again after the in-motion steps of the bench line (2500).  Per state: one
untimed frame per mode, then --frames timed pairs of frames of the same particles -- the thickness mode off, then on -- each the whole
from_container + surface() from the live handle (both synchronous, nothing downloaded), so that the comparison is with the thickness-off
surface frame of the same run.  Reports the medians of the stage times from HIP events (the particle frame's total in both modes; base,
smooth, shade of the surface passes; opaque, splat, smooth, shade of the thickness passes), of the host clock around the two calls, and
the counters: adds issued and adds per second of the splat, pairs cut and removed, surface pixels, taps.  One JSON line per state, also
written to --out (default profiles/render_thickness_bench_c2.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.render import FrameRenderer  # noqa: E402


def one(r, container):
    container.engine.synchronize()
    t0 = time.perf_counter()
    r.from_container(container, download=False)
    r.surface(download=False)
    return 1e3 * (time.perf_counter() - t0), r.stats(), r.surface_stats()


def measure(r, container, frames, label, step, thickness):
    for on in (False, True):   # untimed: allocations, first touch
        r.set_thickness(**thickness) if on else r.clear_thickness()
        one(r, container)
    off, on, thick = [], [], []
    for _ in range(frames):
        r.clear_thickness()
        off.append(one(r, container))
        r.set_thickness(**thickness)
        on.append(one(r, container))
        thick.append(r.thickness_stats())
    mid = lambda v: round(sorted(v)[frames // 2], 3)  # noqa: E731
    t = thick[-1]
    ms_splat = mid([s["ms_splat"] for s in thick])
    out = dict(state=label, step=step, particles=on[-1][1]["particles"], drawn=on[-1][1]["drawn"], frames=frames, width=r.width, height=r.height,
               ms_particle_frame_off=mid([o[1]["ms_total"] for o in off]), ms_particle_frame_on=mid([o[1]["ms_total"] for o in on]),
               ms_particle_frame_off_min_max=[round(min(o[1]["ms_total"] for o in off), 3), round(max(o[1]["ms_total"] for o in off), 3)],
               ms_base=mid([o[2]["ms_base"] for o in on]), ms_depth_smooth=mid([o[2]["ms_smooth"] for o in on]),
               ms_shade_off=mid([o[2]["ms_shade"] for o in off]),
               ms_opaque=mid([s["ms_opaque"] for s in thick]), ms_splat=ms_splat, ms_smooth=mid([s["ms_smooth"] for s in thick]),
               ms_shade=mid([s["ms_shade"] for s in thick]),
               ms_host_off=mid([o[0] for o in off]), ms_host_on=mid([o[0] for o in on]),
               adds=t["adds"], adds_per_second=round(t["adds"] / max(ms_splat, 1e-6) * 1e3), clipped=t["clipped"], removed=t["removed"],
               surface_pixels=on[-1][2]["surface_pixels"], empty_pixels=t["empty_pixels"], max_thickness=t["max_thickness"],
               iterations=t["iterations"], taps_visited=t["taps_visited"],
               identical_counters=all({k: s[k] for k in ("adds", "clipped", "removed", "empty_pixels", "max_thickness", "taps_visited")} ==
                                      {k: t[k] for k in ("adds", "clipped", "removed", "empty_pixels", "max_thickness", "taps_visited")} for s in thick))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--fast-math", action="store_true")
    ap.add_argument("--absorb", type=float, default=0.05)
    ap.add_argument("--scatter", type=float, default=0.01)
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_thickness_bench_c2.txt"))
    a = ap.parse_args()
    thickness = dict(absorb=a.absorb, scatter=a.scatter, iterations=a.iterations)
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    r = FrameRenderer(container.dx, fast_math=a.fast_math)
    r.set_surface()
    rows = [measure(r, container, a.frames, "rest", 0, thickness)]
    if a.motion_step > 0:
        container.engine.step(a.motion_step)
        container.engine.synchronize()
        rows.append(measure(r, container, a.frames, "in_motion", a.motion_step, thickness))
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"python tools/bench_render_thickness.py --frames {a.frames}   (MI355X, {'fast' if a.fast_math else 'strict'} build; one JSON line per state)\n")
            f.write("product.c2_scene() (WCSPH, 1,231,200 particles), reference camera, 1024 x 1024, surface mode at its defaults, thickness "
                    f"mode absorb {a.absorb} scatter {a.scatter} iterations {a.iterations}: from rest, then after engine.step({a.motion_step}); "
                    f"medians of {a.frames} frames, the thickness mode off and on in turn on the same particles\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
