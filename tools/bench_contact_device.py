"""ms/step of product.coupling_scene() (DFSPH, strict build) with the contact and the device_contact rigid backends once bodies touch,
alternated in one process under tools/bench_rigid_device.py's protocol: a fresh scene per measurement, `warmup` steps, then `steps`
timed steps through solver.advance() -- n round trips through the host and its Python solve with `contact`, one device call with
`device_contact`.

The scene's bodies start metres apart and meet only after thousands of steps, so the eight spheres are moved into one touching 3 x 3
layer (one cell empty) above the fluid, 2 mm inside each other's contact distance: they fall together, the split impulses leave them at
the slop depth, and the contact table is non-empty in every step of the window.  The cube stays where it is.

Per measurement one JSON line with
  ms_per_step            wall clock around advance(steps) + synchronize
  event_ms_per_step      the same number of steps once more with the HIP-event profiler on every kernel id: the sum of the launches' times
  contact_pass_us_per_step, solve_us_per_step   kernel ids 25 (rigid_contact) and 27 (rigid_contact_solve) from that second pass
  rows                   contacts of the last step (device_contact: the solve's rows; contact: contacts_from_table of the last table)
  us_per_row_visit       solve_us_per_step / (rows * 2 * iterations): every row is visited by `iterations` velocity sweeps and as many
                         split-impulse sweeps of the one lane that runs them; the launch's fixed part (velocity half, table scan, row
                         build, positions, clearing the table) is in the numerator too, so this is an upper bound of a visit
and a summary line (minimum and maximum ms/step over the rounds).  --backend X --rounds 1 times one backend only (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.SPH.rigid_solver import host_rigid_solver as R  # noqa: E402

D, RADIUS = 0.02, 0.12   # contact distance (the particle pitch) and the spheres' outer particle layer (sphere.obj at scale 0.6)


def touching_scene():
    cfg = P.coupling_scene()
    pitch = 2 * RADIUS + D - 0.002
    cells = [(i, k) for i in range(3) for k in range(3)][:8]
    spheres = [b for b in cfg["RigidBodies"] if b["geometryFile"].endswith("sphere.obj")]
    assert len(spheres) == 8
    for b, (i, k) in zip(spheres, cells):
        b["translation"] = [1.0 + i * pitch, 2.4, 1.0 + k * pitch]
    return cfg


def run(backend, steps, warmup):
    os.environ["SPH_RIGID_BACKEND"] = backend
    os.environ["SPH_RIGID_NATIVE_OK"] = "1"
    container, solver = P.build_product(touching_scene())
    solver.prepare()
    e, rs = container.engine, solver.rigid_solver
    solver.advance(warmup)
    e.synchronize()
    t0 = time.perf_counter()
    solver.advance(steps)
    e.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    e.profile_enable(-1, True); e.profile_reset()
    tables = []
    if backend == "contact":   # the rows the host solves: look at the table it reads
        read = e.get_rigid_contacts
        def spy(reset=True):
            tables.append(read(reset))
            return tables[-1]
        e.get_rigid_contacts = spy
    solver.advance(steps)
    e.synchronize()
    per_kernel = {}
    for k in range(64):
        name = e.lib.sph_kernel_name(k).decode()
        if name == "?":
            break
        launches, kms = e.profile_read(k)
        if launches:
            per_kernel[name] = kms
    rows = len(R.contacts_from_table(tables[-1], rs.bodies)) if backend == "contact" else e.get_rigid_contact_row_count()
    solve_us = 1e3 * per_kernel.get("rigid_contact_solve", 0.0) / steps
    iterations = rs.contact_parameters.iterations
    out = dict(backend=backend, particles=e.particle_num, steps=steps, ms_per_step=round(ms, 4),
               event_ms_per_step=round(sum(per_kernel.values()) / steps, 4),
               contact_pass_us_per_step=round(1e3 * per_kernel.get("rigid_contact", 0.0) / steps, 2),
               solve_us_per_step=round(solve_us, 2), rows=rows, iterations=iterations,
               us_per_row_visit=round(solve_us / (rows * 2 * iterations), 4) if rows and solve_us else None)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--backend", default=None, choices=["contact", "device_contact"])
    a = ap.parse_args()
    order = [a.backend] if a.backend else ["contact", "device_contact"]
    res = {b: [] for b in order}
    for _ in range(a.rounds):
        for b in order:
            r = run(b, a.steps, a.warmup)
            res[b].append(r["ms_per_step"])
            print(json.dumps(r), flush=True)
    print(json.dumps({"summary": {b: dict(min=min(v), max=max(v)) for b, v in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
