"""ms per diffuse-particle step on C2 (product.c2_scene(), 1.23 M particles), strict build, default parameters, early in the collapse
(the state called "rest" follows the 20 + 5 x --sim-steps steps of the simulation timing; its `step` says so) and again --motion-step
(2500) steps later.  Per state: one untimed step, then --steps timed steps with --every
simulation steps between them, as the driver runs them.  Reports the medians of the stage times from HIP events, of the host clock
around the call, the pairs visited and accepted per walk, the diffuse count and classes, the particle frame (1024^2, the reference's
camera) without and with set_foam, and the simulation's own ms/step over --sim-steps steps with no diffuse object in the process yet
(measured first) and again with one alive.  One JSON line per state, also written to --out (default profiles/foam_bench_c2.txt)."""
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


def sim_ms(engine, steps, repeats=5):
    out = []
    for _ in range(repeats):
        engine.synchronize()
        t0 = time.perf_counter()
        engine.step(steps)
        engine.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return sorted(out)


def frame_ms(r, container, frames=5):
    r.from_container(container, download=False)
    out = []
    for _ in range(frames):
        container.engine.synchronize()
        t0 = time.perf_counter()
        r.from_container(container, download=False)
        out.append(1e3 * (time.perf_counter() - t0))
    return round(sorted(out)[frames // 2], 3)


def measure(d, container, solver, a, label, step):
    dt = a.every * float(solver.dt[None])
    d.step(container, dt)   # untimed: allocations, first touch
    rows, host = [], []
    for _ in range(a.steps):
        container.engine.step(a.every)
        container.engine.synchronize()
        t0 = time.perf_counter()
        d.step(container, dt)
        host.append(1e3 * (time.perf_counter() - t0))
        rows.append(d.stats())
    mid = lambda v: round(sorted(v)[len(v) // 2], 3)  # noqa: E731
    s = rows[-1]
    out = dict(state=label, step=step, fluid=s["fluid"], steps=a.steps, every=a.every,
               ms_step=mid([r["ms_total"] for r in rows]), ms_step_min_max=[round(min(r["ms_total"] for r in rows), 3), round(max(r["ms_total"] for r in rows), 3)],
               ms_host=mid(host), ms_per_simulated_step=round(mid([r["ms_total"] for r in rows]) / a.every, 3),
               **{k: mid([r[k] for r in rows]) for k in ("ms_grid", "ms_advect", "ms_normals", "ms_potentials", "ms_generate")},
               pairs_visited=s["pairs_visited"], pairs_accepted=s["pairs_accepted"], diffuse=s["diffuse"], spray=s["spray"], foam=s["foam"],
               bubble=s["bubble"], born_total=s["born_total"], died_total=s["died_total"], dropped_total=s["dropped_total"],
               bytes_allocated=s["bytes_allocated"])
    r = FrameRenderer(container.dx)
    out["ms_frame_plain"] = frame_ms(r, container)
    r.set_foam(d)
    out["ms_frame_with_foam"] = frame_ms(r, container)
    r.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--sim-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foam_bench_c2.txt"))
    a = ap.parse_args()
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    eng = container.engine
    eng.step(20)
    absent = sim_ms(eng, a.sim_steps)
    d = DiffuseParticles(container.dx, container.domain_start, container.domain_end, gravity=[float(g) for g in solver.g],
                         padding=float(container.padding), max_diffuse=2 * int(container.particle_max_num))
    rows = [dict(state="simulation", sim_steps=a.sim_steps, ms_step_object_absent=[round(v, 4) for v in absent])]
    print(json.dumps(rows[0]), flush=True)
    rows.append(measure(d, container, solver, a, "rest", 20 + 5 * a.sim_steps))
    if a.motion_step > 0:
        eng.step(a.motion_step)
        eng.synchronize()
        rows.append(measure(d, container, solver, a, "in_motion", a.motion_step))
        rows.append(dict(state="simulation", sim_steps=a.sim_steps, ms_step_object_alive=[round(v, 4) for v in sim_ms(eng, a.sim_steps)]))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
