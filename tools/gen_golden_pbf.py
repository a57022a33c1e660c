"""PBF fixtures from the reference's own PBF.py / pbf_container.py, run unmodified on the Taichi stand-in (oracle/taichi_shim) as
oracle/gen_golden.py and tools/gen_golden_iisph.py run the other solvers.  Writes tests/golden/pbf/<name>.npz.

    python tools/gen_golden_pbf.py                 # every scene of SCENES
    python tools/gen_golden_pbf.py pbf_moving      # one (several may run side by side, one process each)

The only substitutions are made ON THE INSTANCE, for the two places the reference cannot be followed literally:
  * D2: particle_old_positions and particle_pbf_lambdas are re-sized to particle_max_num (the reference sizes them with
    particle_num[None], still 0 when PBFContainer.__init__ runs);
  * D1: the reference's own fix_position runs with container.particle_positions behind a view whose reads come from a copy
    taken at the start of the pass and whose writes go to the field (Jacobi: every delta from the start-of-pass positions; the
    reference's in-place update is a race in parallel and Gauss-Seidel in index order on a serial interpreter);
and one that makes the reference's grid indexing defined where it is not: grid_num_particles and grid_num_particles_temp get one
extra slot G (= the grid's cell count) and flatten_grid_index returns G for a cell outside the grid.  The reference indexes
grid_num_particles at whatever flatten_grid_index gives there (negative, or another cell's); with the substitution such a cell
holds exactly the particles whose own position lies in no cell (non-finite ones, whose distance test fails), so walks skip it.  The
refine iterations move particles by up to a few cm, so centre cells at and beyond the grid's faces do occur.
Recorded per step s (1-based), arrays in the step-end sorted order with persistent ids `s{s}_ids`:
  * s{s}_positions / _velocities / _densities, s{s}_sort_positions (the positions the step's sort filed, in the same order);
  * per refine iteration k: s{s}_k{k}_rho and _lambda (compute_density / compute_lambda), _x_before and _x_after (around
    fix_position), _recentred (fluid particles whose current cell differs from the one the sort filed them in).
Two steps per scene (the late-entry scene: five, past its entryTime): in 3-D the reference's PBF scatters a block within the first
step (unclamped lambda, the tensile regime of a poly6 density without self term: rho ~ 0.65 rho0 at rest) and leaves fluid
particles with rho = 0, whose next viscosity term divides by zero (non-finite velocities in step 2).  Step 2 is recorded to show
that; its refine iterations are recorded like step 1's.
Deterministic: seeded jitter, fixed velocity fields; a second run writes the same arrays."""
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as G  # noqa: E402  (puts the stand-in and the reference on sys.path)
import taichi as ti  # noqa: E402  (the stand-in)

OUT = os.path.join(ROOT, "tests", "golden", "pbf")


def swirl(center, omega, shear):
    """A fast rotation about y plus a shear in y: particles cross cell faces between the sort and the refine walks."""
    c = np.asarray(center, np.float64)

    def f(pos):
        d = pos - c
        v = np.stack([-omega * d[:, 2], shear * d[:, 0], omega * d[:, 0]], axis=1)
        return v.astype(np.float32)
    return f


SCENES = {
    # name: (scene dict, jitter amplitude, seed, velocity field or None, steps)
    # all fluid at the rest spacing: the tensile regime (rho ~ 0.6-0.7 rho0 at rest with poly6 and no self term)
    "pbf_rest": (G.dam_break_scene(method="pbf", end=(0.16, 0.16, 0.16), dt=4e-4), 0.0, 0, None, 2),
    # packed tighter than the rest spacing
    "pbf_compressed": (G.dam_break_scene(method="pbf", end=(0.12, 0.12, 0.12), particleSpacing=0.0125, dt=4e-4,
                                         velocity=(0.1, -0.3, 0.0)), 0.001, 101, None, 2),
    # a block inside the domain box: rigid neighbours in lambda / fix_position, poly6 rigid volumes
    "pbf_box": (G.dam_break_scene(method="pbf", domain_end=(0.24, 0.24, 0.24), start=(0.0, 0.0, 0.0), end=(0.08, 0.08, 0.08),
                                  translation=(0.03, 0.03, 0.03), dt=4e-4, add_domain_box=True, velocity=(-0.5, -0.5, 0.0)),
                0.001, 102, None, 2),
    # fast velocity field: the recentred path of the refine walks
    "pbf_moving": (G.dam_break_scene(method="pbf", end=(0.14, 0.14, 0.14), dt=4e-4), 0.002, 103,
                   swirl((0.17, 0.17, 0.17), 60.0, 40.0), 2),
    # late entry: PBF.py's _step never calls insert_object, so block 1 never appears
    "pbf_late": (G.late_scene("pbf", 4e-4), 0.0, 0, None, 5),
}


def _np(field, n):
    return field.to_numpy()[:n].copy()


def _cells(x, grid_size, grid_num):
    """(linear cell, inside the grid) of base_container.py:468 pos_to_index (truncation); a non-finite position is in no cell."""
    with np.errstate(invalid="ignore"):
        q = x / np.float32(grid_size)
        c = np.where(np.isfinite(q), q, -1.0).astype(np.int64)
    inside = np.all((c >= 0) & (c < np.asarray(grid_num)), axis=1)
    return (c[:, 0] * grid_num[1] + c[:, 1]) * grid_num[2] + c[:, 2], inside


def run_scene(name):
    cfg, jitter, seed, vfield, steps = SCENES[name]
    tmp = tempfile.NamedTemporaryFile("w", suffix=".json", delete=False)
    json.dump(cfg, tmp)
    tmp.close()
    log = io.StringIO()
    t0 = time.time()
    with contextlib.redirect_stdout(log):
        from SPH.utils import SimConfig
        from SPH.containers import PBFContainer
        from SPH.fluid_solvers import PBFSolver
        container = PBFContainer(SimConfig(scene_file_path=tmp.name))
        solver = PBFSolver(container)
        # D2: the PBF fields, sized particle_max_num
        container.particle_old_positions = ti.Vector.field(container.dim, dtype=ti.f32, shape=container.particle_max_num)
        container.particle_pbf_lambdas = ti.field(dtype=ti.f32, shape=container.particle_max_num)
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

    grid_size = float(container.grid_size)
    grid_num = [int(g) for g in np.asarray(container.grid_num)]
    rec = {}
    it = [0]
    orig_search, orig_density, orig_lambda = container.prepare_neighborhood_search, solver.compute_density, solver.compute_lambda

    def search_recording():
        orig_search()
        m = container.particle_num[None]
        rec["sort_positions"] = _np(container.particle_positions, m)
        it[0] = 0

    def density_recording():
        m = container.particle_num[None]
        x = _np(container.particle_positions, m)
        flm = container.particle_materials._data[:m] == 1
        cur, inside = _cells(x, grid_size, grid_num)
        moved = ~inside | (cur != _cells(rec["sort_positions"], grid_size, grid_num)[0])
        it[0] += 1
        rec[f"k{it[0]}_recentred"] = np.int64(np.count_nonzero(moved & flm))
        orig_density()
        rec[f"k{it[0]}_rho"] = _np(container.particle_densities, m)

    def lambda_recording():
        orig_lambda()
        m = container.particle_num[None]
        rec[f"k{it[0]}_lambda"] = _np(container.particle_pbf_lambdas, m)

    orig_fix = solver.fix_position

    def fix_position_jacobi():
        """D1: the reference's own fix_position, reading the positions at the start of the pass."""
        m = container.particle_num[None]
        rec[f"k{it[0]}_x_before"] = _np(container.particle_positions, m)
        live = container.particle_positions
        frozen = ti.Vector.field(container.dim, dtype=ti.f32, shape=container.particle_max_num)
        frozen._data[...] = live._data
        container.particle_positions = _ReadFrom(live, frozen)
        try:
            orig_fix()
        finally:
            container.particle_positions = live
        rec[f"k{it[0]}_x_after"] = _np(container.particle_positions, m)

    # cells outside the grid: one extra, normally empty slot G behind the grid's cells
    G = int(np.prod(grid_num))
    for nm in ("grid_num_particles", "grid_num_particles_temp"):
        old = getattr(container, nm)
        new = ti.field(int, shape=G + 1)
        new._data[:G] = old._data
        new._data[G] = old._data[G - 1] if nm == "grid_num_particles" else 0
        setattr(container, nm, new)
    container.flatten_grid_index = lambda cell: _lin_or_outside(cell, grid_num, G)
    container.prepare_neighborhood_search = search_recording
    solver.compute_density = density_recording
    solver.compute_lambda = lambda_recording
    solver.fix_position = fix_position_jacobi

    out = {"scene_json": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), "jitter": np.float64(jitter),
           "seed": np.int64(seed), "steps": np.int64(steps),
           "geo_dx": np.float64(container.dx), "geo_dh": np.float64(container.dh), "geo_V0": np.float64(container.V0),
           "geo_grid_size": np.float64(grid_size), "geo_grid_num": np.array(grid_num, np.int64),
           "geo_particle_max_num": np.int64(container.particle_max_num), "dt": np.float64(solver.dt[None]),
           "density_0": np.float64(solver.density_0)}
    for k, v in init.items():
        out["init_" + k] = v
    for step in range(1, steps + 1):
        rec.clear()
        with contextlib.redirect_stdout(log):
            solver.step()
        m = container.particle_num[None]
        out[f"s{step}_ids"] = _np(container.particle_colors, m)[:, 0].astype(np.int64)
        out[f"s{step}_materials"] = _np(container.particle_materials, m)
        out[f"s{step}_rest_volumes"] = _np(container.particle_rest_volumes, m)
        out[f"s{step}_masses"] = _np(container.particle_masses, m)
        out[f"s{step}_positions"] = _np(container.particle_positions, m)
        out[f"s{step}_velocities"] = _np(container.particle_velocities, m)
        out[f"s{step}_densities"] = _np(container.particle_densities, m)
        out[f"s{step}_particle_num"] = np.int64(m)
        for k, v in rec.items():
            out[f"s{step}_{k}"] = v
        print(f"  {name}: step {step} done ({time.time() - t0:.0f} s)", flush=True)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    os.unlink(tmp.name)
    rc = [int(out[f"s{s}_k{k}_recentred"]) for s in range(1, steps + 1) for k in range(1, 6)]
    print(f"{name}: n={n} written ({time.time() - t0:.0f} s); recentred per iteration {rc}")


class _ReadFrom:
    """A field view for D1: element reads from `frozen`, element writes to `live`, everything else from `live`."""

    def __init__(self, live, frozen):
        self.__dict__["_live"], self.__dict__["_frozen"] = live, frozen

    def __getitem__(self, k):
        return self._frozen[k]

    def __setitem__(self, k, v):
        self._live[k] = v

    def __getattr__(self, name):
        return getattr(self._live, name)


def _lin_or_outside(cell, grid_num, G):
    """The linear index of an in-grid cell (x slowest, z fastest, as the reference orders them), G for any other cell."""
    c = [int(cell[d]) for d in range(3)]
    if any(c[d] < 0 or c[d] >= grid_num[d] for d in range(3)):
        return G
    return (c[0] * grid_num[1] + c[1]) * grid_num[2] + c[2]


if __name__ == "__main__":
    for nm in sys.argv[1:] or list(SCENES):
        run_scene(nm)
