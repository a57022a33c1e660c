"""ms per frame of the diffuse particles in the surface frames on C2 (product.c2_scene(), 1.23 M particles) at the
reference's camera and 1024^2, strict build, defaults, in the two states of tools/bench_foam.py: early in the collapse (1,020 steps from
rest) and --motion-step (2500) steps later, each after 21 diffuse steps of 4 simulation steps as that bench takes them.  Per state and
per mode of the surface frames (opaque, then with the thickness mode): one untimed frame with the diffuse set cleared and one with it
set, then --frames timed pairs of frames of the same particles -- cleared, then set -- each the whole from_container + surface() from the
live handle (both synchronous, nothing downloaded).  Reports the medians of the stage times from HIP events (the particle frame's total
in both; base, smooth, shade of the surface passes in both; opaque, splat, smooth, shade of the thickness passes in both; the new
splat, raw-sphere merge and composite), of the host clock around the two calls, and the counters: adds issued over / under and adds per
second of the splat, pairs cut and removed, pixels covered.  One JSON line per state and mode, also written to --out (default
profiles/render_surface_foam_bench_c2.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.foam import DiffuseParticles  # noqa: E402
from sph_project_amd.render import FrameRenderer  # noqa: E402


def one(r, container, thick):
    container.engine.synchronize()
    t0 = time.perf_counter()
    r.from_container(container, download=False)
    r.surface(download=False)
    return 1e3 * (time.perf_counter() - t0), r.stats(), r.surface_stats(), r.thickness_stats() if thick else None


def measure(r, container, d, a, label, step, thick):
    r.set_thickness() if thick else r.clear_thickness()
    foam = dict(raw_spheres=a.raw_spheres)
    for on in (False, True):   # untimed: allocations, first touch
        r.set_surface_foam(d, **foam) if on else r.clear_surface_foam()
        one(r, container, thick)
    off, on, fs = [], [], []
    for _ in range(a.frames):
        r.clear_surface_foam()
        off.append(one(r, container, thick))
        r.set_surface_foam(d, **foam)
        on.append(one(r, container, thick))
        fs.append(r.surface_foam_stats())
    n = a.frames
    mid = lambda v: round(sorted(v)[n // 2], 3)  # noqa: E731
    span = lambda v: [round(min(v), 3), round(max(v), 3)]  # noqa: E731
    f = fs[-1]
    ms_splat = mid([s["ms_splat"] for s in fs])
    adds = f["adds_over"] + f["adds_under"]
    out = dict(state=label, step=step, thickness=bool(thick), raw_spheres=bool(a.raw_spheres), particles=on[-1][1]["particles"], diffuse=f["diffuse"],
               frames=n, width=r.width, height=r.height,
               ms_particle_frame_off=mid([o[1]["ms_total"] for o in off]), ms_particle_frame_on=mid([o[1]["ms_total"] for o in on]),
               ms_particle_frame_off_min_max=span([o[1]["ms_total"] for o in off]),
               ms_base_off=mid([o[2]["ms_base"] for o in off]), ms_base_on=mid([o[2]["ms_base"] for o in on]),
               ms_smooth_off=mid([o[2]["ms_smooth"] for o in off]), ms_smooth_on=mid([o[2]["ms_smooth"] for o in on]),
               ms_shade_off=mid([o[2]["ms_shade"] for o in off]), ms_shade_on=mid([o[2]["ms_shade"] for o in on]),
               ms_surface_passes_off_min_max=span([o[2]["ms_base"] + o[2]["ms_smooth"] + o[2]["ms_shade"] for o in off]))
    if thick:
        for k in ("ms_opaque", "ms_splat", "ms_smooth", "ms_shade"):
            out[f"thick_{k}_off"] = mid([o[3][k] for o in off])
            out[f"thick_{k}_on"] = mid([o[3][k] for o in on])
    out.update(ms_foam_splat=ms_splat, ms_foam_splat_min_max=span([s["ms_splat"] for s in fs]), ms_foam_raw=mid([s["ms_raw"] for s in fs]),
               ms_foam_composite=mid([s["ms_composite"] for s in fs]), ms_foam_composite_min_max=span([s["ms_composite"] for s in fs]),
               ms_host_off=mid([o[0] for o in off]), ms_host_on=mid([o[0] for o in on]),
               adds_over=f["adds_over"], adds_under=f["adds_under"], adds_per_second=round(adds / max(ms_splat, 1e-6) * 1e3),
               clipped=f["clipped"], removed=f["removed"], large=f["large"], pixels_over=f["pixels_over"], pixels_under=f["pixels_under"],
               surface_pixels=on[-1][2]["surface_pixels"],
               identical_counters=all({k: v for k, v in s.items() if not k.startswith("ms_")} == {k: v for k, v in f.items() if not k.startswith("ms_")}
                                      for s in fs))
    print(json.dumps(out), flush=True)
    return out


def diffuse_steps(d, container, solver, every, steps):
    dt = every * float(solver.dt[None])
    for _ in range(steps):
        container.engine.step(every)
        d.step(container, dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--first-step", type=int, default=1020, help="simulation steps before the first state")
    ap.add_argument("--motion-step", type=int, default=2500, help="0: the first state only")
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--diffuse-steps", type=int, default=21)
    ap.add_argument("--raw-spheres", action="store_true", help="also merge the diffuse spheres into the particle frame (section 26's layer)")
    ap.add_argument("--fast-math", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_surface_foam_bench_c2.txt"))
    a = ap.parse_args()
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    eng = container.engine
    eng.step(a.first_step)
    d = DiffuseParticles(container.dx, container.domain_start, container.domain_end, gravity=[float(g) for g in solver.g],
                         padding=float(container.padding), max_diffuse=2 * int(container.particle_max_num))
    r = FrameRenderer(container.dx, fast_math=a.fast_math)
    r.set_surface()
    rows = []
    diffuse_steps(d, container, solver, a.every, a.diffuse_steps)
    at = a.first_step + a.every * a.diffuse_steps
    for thick in (False, True):
        rows.append(measure(r, container, d, a, "early_collapse", at, thick))
    if a.motion_step > 0:
        eng.step(a.motion_step)
        diffuse_steps(d, container, solver, a.every, a.diffuse_steps)
        at += a.motion_step + a.every * a.diffuse_steps
        for thick in (False, True):
            rows.append(measure(r, container, d, a, "in_motion", at, thick))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"python tools/bench_render_surface_foam.py --frames {a.frames}   (MI355X, {'fast' if a.fast_math else 'strict'} build; one JSON line "
                    "per state and mode)\n")
            f.write("product.c2_scene() (WCSPH, 1,231,200 particles), reference camera, 1024 x 1024, surface / thickness / diffuse modes at their "
                    f"defaults (raw_spheres {bool(a.raw_spheres)}); medians of {a.frames} frames, the diffuse set cleared and set in turn on the same particles\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
