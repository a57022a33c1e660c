"""Time-step front end with the surface of the reference's BaseSolver
(SPH/fluid_solvers/base_solver.py).  The physics (kernels :57-:103, density :522, pressure
:136, surface tension :210, viscosity :232, boundary :575, integration :643-:666) runs inside
libsph_hip; this class keeps the constants, the prepare()/step() protocol (:683-:696), late object
insertion and the host rigid-solver hook."""
import os

import numpy as np

from sph_project_amd import _lib as F
from ..containers import BaseContainer
from ..rigid_solver import PyBulletSolver


class _DtField:
    def __init__(self, value):
        self._v = float(np.float32(value))

    def __getitem__(self, key):
        return self._v


class EmitterView:
    """Read-only view of one fluid emitter; every attribute is read from sph_get_emitter_state when somebody looks."""

    def __init__(self, engine, index):
        self._engine, self.index = engine, index

    def _state(self):
        return self._engine.get_emitter_state(self.index)

    object_id = property(lambda self: self._state()["object_id"])
    layer_particles = property(lambda self: self._state()["layer_particles"])
    max_layers = property(lambda self: self._state()["max_layers"])
    emitted = property(lambda self: self._state()["emitted"])
    layers = property(lambda self: self._state()["layers"])
    held_layers = property(lambda self: self._state()["held_layers"])
    exhausted = property(lambda self: bool(self._state()["exhausted"]))


class OutflowView:
    """Read-only view of one outflow volume; every attribute is read from sph_get_outflow_state when somebody looks."""

    def __init__(self, engine, index):
        self._engine, self.index = engine, index

    def _state(self):
        return self._engine.outflow_state(self.index)

    removed = property(lambda self: self._state()["removed"])
    removed_last_step = property(lambda self: self._state()["removed_last_step"])
    active = property(lambda self: bool(self._state()["active"]))


class BaseSolver:
    def __init__(self, container: BaseContainer):
        self.container = container
        self.cfg = container.cfg
        sol = container.solver_constants
        self.g = sol.g
        self.g_upper = sol.g_upper
        self.viscosity_method = sol.viscosity_method
        self.viscosity = sol.viscosity
        self.viscosity_b = sol.viscosity_b
        self.density_0 = sol.density_0
        # the surface tension model: under "reference" the coefficient is the reference's fixed 0.01 (base_solver.py:32),
        # under "akinci" it is gamma (scene key surfaceTension) and surface_adhesion is beta (surfaceAdhesion)
        self.surface_tension_method = getattr(container, "surface_tension_method", "reference")
        akinci = self.surface_tension_method == "akinci"
        self.surface_tension = container.surface_tension if akinci else sol.surface_tension
        self.surface_adhesion = container.surface_adhesion if akinci else 0.0
        # the vorticity model: "none", or "micropolar" with nu_t (scene key vorticity), zeta (viscosityOmega) and
        # theta_inv (inertiaInverse)
        self.vorticity_method = getattr(container, "vorticity_method", "none")
        self.vorticity = getattr(container, "vorticity", 0.01)
        self.viscosity_omega = getattr(container, "viscosity_omega", 0.1)
        self.inertia_inverse = getattr(container, "inertia_inverse", 0.5)
        # air drag and wind: "none", or "gissler" with k (scene key drag), the wind u (airVelocity) and rho_a (airDensity)
        self.drag_method = getattr(container, "drag_method", "none")
        self.drag = getattr(container, "drag", 1.0)
        self.air_velocity = tuple(getattr(container, "air_velocity", (0.0, 0.0, 0.0)))
        self.air_density = getattr(container, "air_density", 1.2041)
        # heat: "none", or "conduction" with alpha (scene key thermalDiffusivity), beta (thermalExpansion) and T_ref
        # (referenceTemperature); thermal_dt_limit: the explicit update's step limit on the rest lattice (advice), or None
        self.thermal_method = getattr(container, "thermal_method", "none")
        self.thermal_diffusivity = getattr(container, "thermal_diffusivity", 1.0e-4)
        self.thermal_expansion = getattr(container, "thermal_expansion", 0.0)
        self.reference_temperature = getattr(container, "reference_temperature", 0.0)
        self.thermal_dt_limit = getattr(container, "thermal_dt_limit", None)
        # elastic solids: {object id: (E, nu)} of the scene's elastic objects
        self.elastic_objects = dict(getattr(container, "elastic_objects", {}))
        self.elastic_dt_limit = getattr(container, "elastic_dt_limit", None)   # 0.4 spacing / c of the stiffest object (advice), or None
        # adaptive time stepping: "none", or "velocity" with cflFactor and the clamps; while it is on, dt[None] and the
        # total_time of container and rigid solver are the library's (_sync_time)
        self.cfl_method = getattr(container, "cfl_method", "none")
        self.cfl_factor = getattr(container, "cfl_factor", 0.5)
        self.cfl_min_time_step = getattr(container, "cfl_min_time_step", 0.0)
        self.cfl_max_time_step = getattr(container, "cfl_max_time_step", 0.0)
        self.dt = _DtField(sol.dt)
        self.rigid_solver = PyBulletSolver(container, gravity=self.g, dt=self.dt[None])
        self.engine = container.engine
        self.emitters = [EmitterView(self.engine, k) for k in range(len(getattr(container, "emitters", [])))]
        self.outflows = [OutflowView(self.engine, k) for k in range(len(getattr(container, "outflows", [])))]
        if self.viscosity_method == "implicit":
            self.cg_tol = 1e-6

    # ---- individually callable reference kernels (tests / notebooks)
    def compute_rigid_particle_volume(self):
        self.engine.run_phase(F.PH_RIGID_VOLUME)

    def compute_density(self):
        self.engine.run_phase(F.PH_DENSITY)

    def compute_non_pressure_acceleration_and_update_velocity(self):
        self.engine.run_phase(F.PH_NON_PRESSURE)

    # ---- protocol
    def prepare(self):
        """base_solver.py:683."""
        self.container.insert_object()
        self.rigid_solver.insert_rigid_object()
        self.engine.prepare()
        self._sync_time()

    def _adaptive(self):
        return getattr(self, "cfl_method", "none") == "velocity"

    def _sync_time(self):
        """Adaptive time stepping: the step size and the scene time are the library's."""
        if not self._adaptive():
            return
        st = self.engine.time_state()
        self.dt._v = st["dt_next"]
        self.container.total_time = st["time"]
        self.rigid_solver.total_time = st["time"]

    def _step(self):
        """WCSPH.py:27 / DFSPH.py:298 / PCISPH.py:165: the device runs _step() up to the point where the reference
        calls rigid_solver.step(); the host then integrates the rigid bodies and inserts the objects whose entryTime
        has come (base_container.py:218-221) exactly where the reference does; the device finishes the step
        (renew_rigid_particle_state, boundary, DFSPH's neighbour search + density + alpha + divergence solve)."""
        self.engine.step_begin()
        if self._adaptive():   # the host rigid backends take the running step's size (a stale maximum may just have changed it)
            self.dt._v = self.engine.time_state()["dt_next"]
            self.rigid_solver.set_dt(self.dt[None])
        self.container.in_step = True   # what enters now enters at the time this step ends at (scripted bodies: motion.py)
        try:
            self.rigid_solver.step()
            self.container.insert_object()
            self.rigid_solver.insert_rigid_object()
        finally:
            self.container.in_step = False
        self.engine.step_end()
        self._update_exported_meshes()

    def _update_exported_meshes(self):
        """base_solver.py:634-641 (renew_rigid_particle_state with exportObj): the mesh of every dynamic rigid body
        follows its pose, so that run_simulation.py can write mesh_object_{id}.obj."""
        if not self.cfg.get_cfg("exportObj"):
            return
        for oid in list(self.rigid_solver.bodies) + list(self._scripted()):
            posed = self.posed_mesh_vertices(oid)
            if posed is not None:
                self.container.object_collection[oid]["mesh"].vertices = posed

    def posed_mesh_vertices(self, oid):
        """f64[nv, 3]: the mesh vertices of rigid body oid at its current pose (rest shape about the rest centre of mass, turned and
        moved by the body's state); the mesh as loaded for a body the rigid solver does not move; None for a body without a mesh."""
        obj = self.container.object_collection.get(oid)
        if not isinstance(obj, dict) or "mesh" not in obj:
            return None
        b = self.rigid_solver.bodies.get(oid) or self._scripted().get(oid)   # (a scripted body follows its program's pose)
        if b is None:
            return np.asarray(obj["mesh"].vertices, dtype=np.float64)
        rest = np.asarray(obj["restPosition"], dtype=np.float64) - np.asarray(obj["restCenterOfMass"], dtype=np.float64)
        return (b.rot @ rest.T).T + b.com

    def _scripted(self):
        """The rigid solver's scripted bodies (object id -> body)."""
        return getattr(self.rigid_solver, "scripted", None) or {}

    def _count_step(self):
        """A step is complete: scripted bodies take their time from the count (t_k = k dt, a product)."""
        self.container.step_count = getattr(self.container, "step_count", 0) + 1

    def _bodies_on_device(self):
        """The "device" rigid backend is active: the device integrates the dynamic bodies between the halves of its own steps."""
        return getattr(self.rigid_solver, "on_device", False)

    def _host_acts_inside_a_step(self):
        """A dynamic rigid body to integrate or an object still waiting for its entryTime: the host has to act in the middle
        of _step(), where the reference does (WCSPH.py:39-42).  Bodies the device integrates itself (the "device" rigid backend)
        need nothing from the host."""
        moved = bool(self.rigid_solver.bodies) or bool(self._scripted())   # (scripted bodies: the host evaluates their programs)
        return (moved and not self._bodies_on_device()) or self.container.objects_pending()

    def _device_steps(self, n):
        """n whole steps on the device.  WCSPH, reference-variant PBF (and solvers with a fixed iteration count) need nothing back from the device:
        the steps are only enqueued -- like a Taichi kernel launch, observable behaviour stays synchronous because every
        read of a field / of stats() drains the stream first.  Solver loops with their own stop tests read a flag back per
        batch of iterations anyway."""
        free_running = self.container.METHOD == "wcsph" or (self.container.METHOD == "pbf" and   # (the consistent PBF variant has a stop test)
                                                            getattr(self.container, "pbf_variant", "reference") == "reference")
        asynchronous = free_running or self.container.params_dict.get("fixed_iterations", 0) > 0
        if asynchronous and os.environ.get("SPH_SYNC_STEPS", "0") not in ("", "0"):
            asynchronous = False   # opt-out: every step() returns only when the device is done, errors surface in the call that caused them
        if self._adaptive():
            asynchronous = False   # adaptive time stepping: the largest speed is read back at every step, sph_step_async refuses
        if getattr(self, "outflows", None):
            asynchronous = False   # outflow volumes: the removed count is read back at every slot, sph_step_async refuses
        if asynchronous:
            self.engine.step_async(n)
        else:
            self.engine.step(n)
        if self._bodies_on_device():   # the bodies moved with the steps: their state is read back when somebody looks, and the
            self.rigid_solver.mark_stale()   # exported meshes are posed once, from the state at the end
            self._update_exported_meshes()

    def step(self):
        """base_solver.py:692.  Without anything for the host to do inside the step it is one enqueue (no step_begin / step_end
        pair, no host synchronisation: tools/step_overhead.py)."""
        if self._host_acts_inside_a_step() or (self.cfg.get_cfg("exportObj") and not self._bodies_on_device()):
            self._step()
        else:
            self._device_steps(1)
        self.container.total_time += self.dt[None]
        self.rigid_solver.total_time += self.dt[None]
        self._count_step()
        self._sync_time()

    def advance_to(self, t, max_steps=None):
        """Adaptive time stepping: steps until the scene time reaches t (the last steps land on it) or max_steps steps are done;
        returns the steps done.  One sph_advance_until where the host has nothing to do inside a step, else sph_set_time_target and
        step() until the target is reached."""
        if not self._adaptive():
            raise ValueError("advance_to needs Configuration.cflMethod \"velocity\"")
        cap = (1 << 30) if max_steps is None else int(max_steps)
        if not (self._host_acts_inside_a_step() or (self.cfg.get_cfg("exportObj") and not self._bodies_on_device())):
            done = self.engine.advance_until(t, cap)
            for _ in range(done):
                self._count_step()
            if done and self._bodies_on_device():
                self.rigid_solver.mark_stale()
                self._update_exported_meshes()
            self._sync_time()
            return done
        done = 0
        self.engine.set_time_target(t)
        try:
            while done < cap and t - self.engine.time_state()["time"] > self.cfl_max_time_step / 1048576.0:
                self.step()
                done += 1
        finally:
            self.engine.set_time_target(None)
            self._sync_time()
        return done

    def advance(self, n):
        """n calls of step().  Where the host has nothing to do inside a step -- no dynamic rigid body to integrate, no object
        still waiting for its entryTime -- they go to the device as ONE sph_step(h, n): no Python, no host synchronisation
        between them (not in the reference, whose driver can only call step())."""
        n = int(n)
        if n <= 0:
            return
        if self._bodies_on_device():   # only objects still to enter keep the host in the loop: step by step until they are in
            while n > 0 and self._host_acts_inside_a_step():
                self.step()
                n -= 1
            if n == 0:
                return
        if self._host_acts_inside_a_step():
            for _ in range(n):
                self.step()
            return
        self._device_steps(n)
        for _ in range(n):   # the same float additions as n calls of step()
            self.container.total_time += self.dt[None]
            self.rigid_solver.total_time += self.dt[None]
            self._count_step()
        self._sync_time()

    def stats(self):
        return self.engine.stats()
