"""ms/step of product.wave_tank_scene() at C2's particle count (WCSPH, strict build) with the scripted paddle moved by the native backend
(the host evaluates the program and pushes the pose every step) and by the device backend (one launch per step, the whole window one
device call), alternating in one process: `warmup` steps each, then `windows` windows of `steps` steps per backend, native and device in
turn.  The steps go through solver.advance(), the driver's path.  A last window of the device backend runs with the HIP-event profiler
on SPH_K_RIGID_MOTION alone: the launch's own time.  One JSON line per window, a summary line at the end; --out FILE also writes the
report (profiles/rigid_motion_bench.txt)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import _lib as L  # noqa: E402
from sph_project_amd import product as P  # noqa: E402


def build(backend, size):
    os.environ["SPH_RIGID_NATIVE_OK"] = "1"
    container, solver = P.build_product(P.wave_tank_scene(**size), rigid_backend=backend)
    solver.prepare()
    return container, solver


def window(container, solver, steps):
    e = container.engine
    e.synchronize()
    t0 = time.perf_counter()
    solver.advance(steps)
    e.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--length", type=float, default=8.25)   # 400 x 20 x 154 = 1,232,000 fluid particles: C2's count (1,231,200)
    ap.add_argument("--width", type=float, default=3.2)
    ap.add_argument("--depth", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    size = dict(length=a.length, width=a.width, depth=a.depth)
    runs = {b: build(b, size) for b in ("native", "device")}
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    for b, (container, solver) in runs.items():
        solver.advance(a.warmup)
        container.engine.synchronize()
    res = {b: [] for b in runs}
    for w in range(a.windows):
        for b, (container, solver) in runs.items():
            ms = window(container, solver, a.steps)
            res[b].append(ms)
            emit(dict(backend=b, window=w, steps=a.steps, particles=container.engine.particle_num,
                      fluid_particles=container.engine.fluid_particle_num, ms_per_step=round(ms, 4)))
    container, solver = runs["device"]
    e = container.engine
    e.profile_enable(L.K_RIGID_MOTION, True); e.profile_reset()
    solver.advance(a.steps)
    e.synchronize()
    launches, kms = e.profile_read(L.K_RIGID_MOTION)
    force, torque, impulse, _ = solver.rigid_solver.scripted_wrench(1)
    emit(dict(kernel="rigid_motion", launches=launches, us_per_launch=round(1e3 * kms / max(launches, 1), 3),
              paddle_force_x=float(force[0]), paddle_impulse_x=float(impulse[0]), scene_time=round(container.total_time, 4)))
    emit({"summary": {b: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for b, v in res.items()}})
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/bench_rigid_motion.py: wave_tank_scene(length=%g, width=%g, depth=%g), WCSPH, strict build; %d warm-up steps, then "
                    "%d windows of %d steps per backend, native and device alternating; ms/step is the wall clock around advance() + synchronize\n"
                    % (a.length, a.width, a.depth, a.warmup, a.windows, a.steps))
            f.write("\n".join(lines) + "\n")
    for container, _ in runs.values():
        container.engine.close()


if __name__ == "__main__":
    main()
