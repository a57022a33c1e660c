"""IISPH fixtures from the reference's own IISPH.py / iisph_container.py, run unmodified on the Taichi stand-in
(oracle/taichi_shim) exactly as oracle/gen_golden.py runs the other solvers.  Writes tests/golden/iisph/<name>.npz.

    python tools/gen_golden_iisph.py                 # every scene of SCENES
    python tools/gen_golden_iisph.py iisph_late      # one (several may run side by side, one process each)

oracle/gen_golden.py (not changed) knows three methods; this generator imports its sys.path set-up, late_scene() and
snapshot() and adds what the IISPH checks need.  At each checkpoint step the solver's refine() is wrapped ON THE
INSTANCE (the reference file stays as it is) to record
  * before the first iteration: positions, velocities (v* = v + dt a_np), densities, rest volumes, materials, dii, aii, rho*
    -- the inputs and outputs of compute_dii / compute_aii / compute_density_star (IISPH.py:18-90);
  * around the last iteration: the pressures it started from (`it_p_prev`), and after the loop dij_pj, sum_i, the
    pressures and density_error -- inputs and outputs of compute_dij_pj / compute_sum_i / update_pressure (:98-183);
and the per-step history of refine's iteration counts and errors (the line IISPH.py:199 prints).  All scenes are all
fluid: next to rigid particles the reference divides by a density it has not computed yet.
Deterministic: seeded jitter, fixed velocity fields; a second run writes the same arrays."""
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as G  # noqa: E402  (puts the stand-in and the reference on sys.path)

OUT = os.path.join(ROOT, "tests", "golden", "iisph")
ITER_RE = r"IISPH - iteration: (\d+) Avg density err: (\S+)"


def late_compressed():
    """gen_golden.late_scene under IISPH with both blocks packed tighter than the rest spacing, so that the loop is live at
    step 1 (at the rest spacing every step takes a single iteration)."""
    cfg = G.late_scene("iisph", 4e-4)
    cfg["Configuration"]["particleSpacing"] = 0.017
    return cfg


def converging(center, rate):
    """v = -rate (x - center): a block flowing into its own middle, so that rho* > rho0 inside after the first step too."""
    return lambda pos: (-rate * (pos - np.asarray(center, np.float64))).astype(np.float32)


SCENES = {
    # name: (scene dict, jitter amplitude, seed, velocity field or None, checkpoints)
    # lattice packed tighter than the rest spacing: the loop is live at step 1, then rho* <= rho0 everywhere (p = 0, 1 iteration)
    "iisph_compressed": (G.dam_break_scene(method="iisph", end=(0.1, 0.1, 0.1), particleSpacing=0.0165, dt=4e-4,
                                           velocity=(0.1, -0.3, 0.0)), 0.0015, 91, None, [1, 2, 4]),
    # a slightly packed lattice flowing into its own middle (at the rest spacing the loop first iterates at step 3)
    "iisph_converging": (G.dam_break_scene(method="iisph", end=(0.108, 0.108, 0.108), particleSpacing=0.0185, dt=4e-4), 0.002, 92,
                         converging((0.1555, 0.1555, 0.1555), 40.0), [1, 2, 3]),
    # late entry (base_container.py:218-221): block 1 lands on block 0 during step 4 (IISPH.py:223 inserts it)
    "iisph_late": (late_compressed(), 0.0, 0, None, [2, 4, 5]),
    # implicit viscosity under IISPH: the CG solve runs inside compute_non_pressure_acceleration, before dii / aii / rho*
    "iisph_implicit": (G.dam_break_scene(method="iisph", end=(0.1, 0.1, 0.1), particleSpacing=0.0175, dt=4e-4, viscosity=50.0,
                                         viscosity_method="implicit", velocity=(0.2, -0.5, 0.1)), 0.002, 93, None, [1, 2]),
}


def _np(field, n):
    return field.to_numpy()[:n].copy()


def run_scene(name):
    cfg, jitter, seed, vfield, checkpoints = SCENES[name]
    tmp = tempfile.NamedTemporaryFile("w", suffix=".json", delete=False)
    json.dump(cfg, tmp)
    tmp.close()
    log = io.StringIO()
    t0 = time.time()
    with contextlib.redirect_stdout(log):
        from SPH.utils import SimConfig
        from SPH.containers import IISPHContainer
        from SPH.fluid_solvers import IISPHSolver
        container = IISPHContainer(SimConfig(scene_file_path=tmp.name))
        solver = IISPHSolver(container)
        # ---- solver.prepare() (base_solver.py:683-690), spelled out so ids / jitter / velocities can be set after insertion
        solver.init_object_id()
        container.insert_object()
        n = container.particle_num[None]
        colors = container.particle_colors._data
        colors[:n, 0] = np.arange(n)
        colors[:n, 1:] = 0
        fl = np.nonzero(container.particle_materials._data[:n] == 1)[0]
        pos = container.particle_positions._data
        if jitter > 0:
            rng = np.random.default_rng(seed)
            pos[fl] = (pos[fl] + rng.uniform(-jitter, jitter, (len(fl), 3))).astype(np.float32)
        if vfield is not None:
            container.particle_velocities._data[fl] = vfield(pos[fl].astype(np.float64))
        init = {"positions": pos[:n].copy(), "velocities": container.particle_velocities._data[:n].copy(),
                "densities": container.particle_densities._data[:n].copy(),
                "materials": container.particle_materials._data[:n].copy(),
                "object_ids": container.particle_object_ids._data[:n].copy(),
                "is_dynamic": container.particle_is_dynamic._data[:n].copy()}
        solver.prepare_emitter()
        solver.rigid_solver.insert_rigid_object()
        solver.renew_rigid_particle_state()
        container.prepare_neighborhood_search()
        solver.compute_rigid_particle_volume()

    rec = {}
    orig_refine, orig_dij = solver.refine, solver.compute_dij_pj

    def dij_recording():
        m = container.particle_num[None]
        rec["p_prev"] = _np(container.particle_pressures, m)   # overwritten every iteration: the last one's survives
        orig_dij()

    def refine_recording():
        m = container.particle_num[None]
        rec.update(ids=_np(container.particle_colors, m)[:, 0], positions=_np(container.particle_positions, m),
                   velocities=_np(container.particle_velocities, m), densities=_np(container.particle_densities, m),
                   rest_volumes=_np(container.particle_rest_volumes, m), materials=_np(container.particle_materials, m),
                   dii=_np(container.dii, m), aii=_np(container.iisph_aii, m),
                   densities_star=_np(container.particle_densities_star, m))
        solver.compute_dij_pj = dij_recording
        orig_refine()
        solver.compute_dij_pj = orig_dij
        rec.update(dij_pj=_np(container.dij_pj, m), sum_i=_np(container.sum_i, m), p_after=_np(container.particle_pressures, m),
                   density_error=np.float32(container.density_error[None]))

    out = {"scene_json": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), "jitter": np.float64(jitter),
           "seed": np.int64(seed), "checkpoints": np.array(checkpoints),
           "geo_dx": np.float64(container.dx), "geo_dh": np.float64(container.dh), "geo_V0": np.float64(container.V0),
           "geo_particle_max_num": np.int64(container.particle_max_num), "dt": np.float64(solver.dt[None]),
           "density_0": np.float64(solver.density_0)}
    for k, v in init.items():
        out["init_" + k] = v
    step = 0
    for cp in checkpoints:
        while step < cp:
            rec.clear()
            solver.refine = refine_recording if step + 1 == cp else orig_refine
            with contextlib.redirect_stdout(log):
                solver.step()
            solver.refine = orig_refine
            step += 1
            # late entrants: persistent id = insertion index (count so far + rank in lattice order), as gen_golden.run_scene
            n_now = container.particle_num[None]
            colors = container.particle_colors._data
            late = np.nonzero((colors[:n_now, 0] == G.LATE_COLOR[0]) & (colors[:n_now, 1] == G.LATE_COLOR[1]))[0]
            if len(late):
                lp = container.particle_positions._data[late]
                order = np.lexsort((lp[:, 2], lp[:, 1], lp[:, 0]))
                first = n_now - len(late)
                colors[late[order], 0] = first + np.arange(len(late))
                colors[late, 1:] = 0
                out["late_step"] = np.int64(step)
                out["late_first_id"] = np.int64(first)
        for k, v in rec.items():
            out[f"it{cp}_" + k] = v
        for k, v in G.snapshot(container, solver, "iisph", log).items():
            if k in ("ids", "positions", "velocities", "densities", "pressures", "materials", "accelerations"):
                out[f"s{cp}_" + k] = v
        out[f"s{cp}_densities_star"] = _np(container.particle_densities_star, container.particle_num[None])
        print(f"  {name}: step {step} done ({time.time() - t0:.0f} s)", flush=True)
    hist = re.findall(ITER_RE, log.getvalue())
    out["hist_iter"] = np.array([int(a) for a, _ in hist], np.int32)
    out["hist_err"] = np.array([float(b) for _, b in hist], np.float64)   # printed: density_error * density_0
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    os.unlink(tmp.name)
    print(f"{name}: n={n} written ({time.time() - t0:.0f} s); iterations per step {out['hist_iter'].tolist()}")


if __name__ == "__main__":
    for nm in sys.argv[1:] or list(SCENES):
        run_scene(nm)
