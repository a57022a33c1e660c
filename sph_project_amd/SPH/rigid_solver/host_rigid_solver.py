"""Host-side rigid-body solver behind the reference's interface (SPH/rigid_solver/bullet_solver.py: PyBulletSolver with
insert_rigid_object() / step() / total_time).

Rigid-body dynamics stays on the CPU (<= 20 bodies); the device side only accumulates the fluid->rigid force / torque
per object and consumes the pose.  `step()` is bullet_solver.py:144-167: pull the wrench (sph_get_rigid_wrench =
rigid_body_forces / rigid_body_torques read + reset), integrate, push centre of mass, rotation, linear and angular
velocity back (sph_set_rigid_pose); the device turns the pose into particle positions / velocities
(_renew_rigid_particle_state, base_solver.py:616) at sph_step_end.

Built-in backends:
  * "native" (default): free rigid bodies under gravity and the fluid wrench, semi-implicit Euler, inertia tensor of the
    body's own particle set, inelastic contact of the body's particle-set EXTENT (its axis-aligned bounds in the current
    orientation) with the reference's boundary walls (bullet_solver.py:53-71) -- the reference collides the body's mesh
    with those wall boxes, so a body comes to rest ON the floor, not with its centre of mass in it.  No body-body
    contacts, no friction, no contact torque: that is Bullet's job, and a scene that needs it diverges from the
    reference -- the first dynamic body integrated by this backend therefore prints a one-time warning to stderr
    (silence it with SPH_RIGID_NATIVE_OK=1).  Unit-tested (tests/test_rigid_host.py).
  * "contact" (opt-in, SPH_RIGID_BACKEND=contact): the native integrator plus body-body and body-wall contact.  The device's
    rigid contact pass (sph_set_rigid_contact) reduces the touching particle pairs of every step to a table keyed by (dynamic body,
    partner, normal bin); each non-empty key becomes ONE contact (mean midpoint, normalised sum of depth * n, maximum depth), and a
    sequential-impulse solver resolves all of them together: restitution, Coulomb friction, split-impulse position correction;
    static bodies, the domain box and the wall planes have infinite mass.  No AABB clamp.  Parameters: the optional Configuration keys
    rigidContactRestitution / rigidContactFriction / rigidContactIterations.  Unit-tested (tests/test_contact_host.py).
  * "device" (opt-in, SPH_RIGID_BACKEND=device): the native backend's physics -- the same integrator, the same wall rule, NO body-body
    contacts, no friction, no contact torque (those are "device_contact") -- run by the device between the two halves of every step (sph_set_rigid_integrator,
    csrc/sph_rigid.hpp), so that a scene with dynamic bodies advances in one device call: no wrench read-back, no pose upload, no
    host synchronisation per step.  The float64 state lives on the device; `bodies[oid].com / rot / vel / angvel`,
    get_rigid_body_states() and container.rigid_body_velocities are read back when somebody asks for them.
    Not for PBF (which moves no body) and not for sharded scenes.
  * "device_contact" (opt-in, SPH_RIGID_BACKEND=device_contact): the contact backend's physics -- the same contacts from the same table,
    the same sequential-impulse solve, statement by statement -- run by the device between the two halves of every step
    (sph_set_rigid_contact_solver, csrc/sph_contact_solve.hpp), with the device backend's plumbing: the float64 state on the device, lazy
    read-back, no wrench read, no table read, no pose upload.  A scene with stacking, colliding, sliding bodies advances in one device
    call.  Not for PBF and not for sharded scenes.
  * "pybullet": the reference's calls (URDF from the mesh file, applyExternalForce / Torque at the base,
    stepSimulation, base pose read-back) when the package is importable.  It is not installed in this image, so this
    backend has never run here; select it with SPH_RIGID_BACKEND=pybullet.
Static bodies need no backend at all (bullet_solver.py:31-42 makes the same distinction).

Scripted bodies (a RigidBodies entry with a "motion" key, motion.py) are a third kind: their pose is a function of the step
count.  They live in `scripted`, not in `bodies` -- no integrator, contact solver or wall rule touches them, and to the contact backends
they are infinite-mass partners.  The native and contact backends evaluate the next pose on the host every step and push it; the device
backends hand the program to the library once (sph_set_rigid_motion) and read the state back when somebody looks.
"""
import math
import os
import sys

import numpy as np

from .motion import RigidMotion, is_scripted

_WARNED = [False]
# contact backend: resting contacts keep this much depth (in units of the contact distance D), so that the touching particle set of a
# resting face -- and with it the contact point -- does not flicker from step to step
CONTACT_SLOP = 0.05
# ... and every contact resists rolling within mu lambda_n times this radius (units of D): one aggregated point per key cannot carry the
# torque the pressure distribution of a face does.  Both are Configuration keys (rigidContactSlop, rigidContactRollingRadius).
CONTACT_ROLLING_RADIUS = 1.0


def _rotation(angle, axis):
    """Orientation bullet_solver.py:97-101 builds: Euler angles (axis * angle) -> quaternion -> matrix (XYZ order)."""
    ex, ey, ez = [float(a) * angle for a in axis]
    cx, sx, cy, sy, cz, sz = math.cos(ex), math.sin(ex), math.cos(ey), math.sin(ey), math.cos(ez), math.sin(ez)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def _skew_exp(w):
    """exp([w]x): rotation by |w| about w (Rodrigues)."""
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


class _Body:
    def __init__(self, oid, mass, inertia_body, com, rot, vel):
        self.oid, self.mass = oid, float(mass)
        self.I_body = np.asarray(inertia_body, dtype=np.float64)
        self.I_body_inv = np.linalg.inv(self.I_body)
        self.com = np.asarray(com, dtype=np.float64).copy()
        self.rot = np.asarray(rot, dtype=np.float64).copy()
        self.vel = np.asarray(vel, dtype=np.float64).copy()
        self.angvel = np.zeros(3)
        self.points = None   # body-frame particle positions (wall contact uses their extent)


class _DeviceBody(_Body):
    """A body the device integrates: its state is read back from the device when it is looked at after a step."""
    _solver = None

    def _get(name):
        def get(self):
            if self._solver is not None:
                self._solver.refresh()
            return self.__dict__["_" + name]
        return property(get, lambda self, v: self.__dict__.__setitem__("_" + name, v))
    com, rot, vel, angvel = _get("com"), _get("rot"), _get("vel"), _get("angvel")
    del _get


class _Scripted:
    """A scripted body: its program, its state after the last step, the wrench that step consumed and the impulse sums."""

    def __init__(self, oid, motion, com, rot, points):
        self.oid, self.motion, self.points = oid, motion, points
        self.com, self.rot = np.asarray(com, np.float64).copy(), np.asarray(rot, np.float64).copy()
        self.vel, self.angvel = np.zeros(3), np.zeros(3)
        self.force, self.torque, self.impulse, self.angular_impulse = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)


class _DeviceScripted(_Scripted):
    """A scripted body the device moves: its record is read back from the device when it is looked at after a step."""
    _solver = None

    def _get(name):
        def get(self):
            if self._solver is not None:
                self._solver.refresh()
            return self.__dict__["_" + name]
        return property(get, lambda self, v: self.__dict__.__setitem__("_" + name, v))
    com, rot, vel, angvel = _get("com"), _get("rot"), _get("vel"), _get("angvel")
    force, torque, impulse, angular_impulse = _get("force"), _get("torque"), _get("impulse"), _get("angular_impulse")
    del _get


class _DeviceVelocities:
    """container.rigid_body_velocities of the device backend: the container's array, brought up to date before it is read."""

    def __init__(self, array, solver):
        self._a, self._solver = array, solver

    def _fresh(self):
        self._solver.refresh()
        return self._a

    def __getitem__(self, k):
        return self._fresh()[k]

    def __setitem__(self, k, v):
        self._a[k] = v

    def __array__(self, dtype=None, copy=None):
        a = self._fresh()
        return a.copy() if dtype is None else a.astype(dtype)

    def __len__(self):
        return len(self._a)

    shape = property(lambda self: self._a.shape)
    dtype = property(lambda self: self._a.dtype)


class HostRigidSolver:
    def __init__(self, container, gravity=(0, -9.8, 0), dt=1e-3):
        self.container = container
        self.total_time = 0.0
        self.present_rigid_object = []
        assert container.dim == 3, "the rigid solver only supports 3-D scenes (bullet_solver.py:19)"
        self.gravity, self.dt = np.asarray(gravity, dtype=np.float64), float(dt)
        self.rigid_bodies = container.cfg.get_rigid_bodies()
        self.rigid_blocks = container.cfg.get_rigid_blocks()
        self.bodies = {}   # object id -> _Body (dynamic ones)
        self.scripted = {}   # object id -> _Scripted (bodies with a motion program)
        # the container's rigid_backend option (run_simulation.py --rigid_backend) first, then SPH_RIGID_BACKEND
        self.backend = getattr(container, "rigid_backend", None) or os.environ.get("SPH_RIGID_BACKEND", "native")
        self._bullet = None
        self.on_device = False   # "device" / "device_contact" is active: the device moves the bodies, the host only reads them back
        self._stale = False
        if not self.rigid_bodies and not self.rigid_blocks:
            print("No rigid body in the scene, skip bullet solver initialization.")
        elif self.backend == "pybullet":
            try:
                self._bullet = _BulletBackend(container, self.gravity, self.dt)
            except ImportError as e:   # asked for explicitly: never fall back silently
                raise NotImplementedError("SPH_RIGID_BACKEND=pybullet, but pybullet is not importable") from e
        elif self.backend not in ("native", "contact", "device", "device_contact"):
            raise ValueError(f"SPH_RIGID_BACKEND={self.backend!r}: expected 'native', 'contact', 'device', 'device_contact' or 'pybullet'")
        # walls no part of a body may cross (bullet_solver.py:57-61)
        eps = container.padding + container.particle_diameter + container.domain_box_thickness
        self.wall_lo = np.asarray(container.domain_start, dtype=np.float64) + eps
        self.wall_hi = np.asarray(container.domain_end, dtype=np.float64) - eps
        self.contact = None              # the host's solver ("contact")
        self.contact_parameters = None   # ... and the ContactSolver that holds its parameters ("contact" and "device_contact")
        dynamic = any(b["isDynamic"] for b in self.rigid_bodies)
        scripted = any(is_scripted(b) for b in self.rigid_bodies)
        if scripted and self.backend == "pybullet":
            raise ValueError("motion: the pybullet rigid backend does not move scripted bodies")
        pbf = getattr(container, "METHOD", None) == "pbf"
        if pbf and self.backend in ("contact", "device", "device_contact"):
            what = {"contact": "contact", "device": "the device integrator", "device_contact": "the device contact solver"}[self.backend]
            print(f"SPH_RIGID_BACKEND={self.backend}: PBF moves no rigid body (PBF.py _step), {what} stays off.")
        elif self.backend in ("contact", "device_contact") and dynamic:   # (static bodies alone: nothing would read the table)
            cfg = container.cfg
            get = lambda k, d: d if cfg.get_cfg(k) is None else cfg.get_cfg(k)
            solver = ContactSolver(restitution=float(get("rigidContactRestitution", 0.2)),
                                   friction=float(get("rigidContactFriction", 0.5)),
                                   iterations=int(get("rigidContactIterations", 10)),
                                   gravity=self.gravity, dt=self.dt)
            # D: the pitch bodies and box are sampled at; wall planes only where no domain box stands in for them
            self.contact_distance = float(getattr(container, "particle_spacing", container.particle_diameter))
            solver.slop = float(get("rigidContactSlop", CONTACT_SLOP)) * self.contact_distance
            solver.patch = float(get("rigidContactRollingRadius", CONTACT_ROLLING_RADIUS)) * self.contact_distance
            walls = not getattr(container, "add_domain_box", False)
            container.engine.set_rigid_contact(True, self.contact_distance, self.wall_lo if walls else None,
                                               self.wall_hi if walls else None)
            self.contact_parameters = solver
            if self.backend == "contact":
                self.contact = solver   # the host solves
        if self.backend in ("device", "device_contact") and (dynamic or scripted) and not pbf:
            # (a sharded scene: the library refuses, and the error is the caller's)
            container.engine.set_rigid_integrator(True, self.gravity, self.wall_lo, self.wall_hi)
            if self.backend == "device_contact" and dynamic:   # the device solves, with the parameters the host solver would use
                container.engine.set_rigid_contact_solver(True, solver.e, solver.mu, solver.iterations, solver.beta, solver.slop,
                                                          solver.patch)
            container.rigid_body_velocities = _DeviceVelocities(np.asarray(container.rigid_body_velocities), self)
            self.on_device = True

    # ------------------------------------------------------------------ bullet_solver.py:46-51, :75-131
    def insert_rigid_object(self):
        for body in self.rigid_bodies:
            oid = body["objectId"]
            if oid in self.present_rigid_object or body["entryTime"] > self.total_time:
                continue
            self.present_rigid_object.append(oid)
            if is_scripted(body):
                self._insert_scripted(body)
                continue
            if not body["isDynamic"]:
                continue
            c = self.container
            translation = np.asarray(body["translation"], dtype=np.float64)
            angle = body["rotationAngle"] / 360 * (2 * math.pi)
            rot = _rotation(angle, body["rotationAxis"])
            vel = np.asarray(body["velocity"], dtype=np.float64)
            # the body's particles were voxelised from the scaled, untransformed mesh (base_container.py:616-626): their
            # positions ARE the body-frame coordinates, with the base frame origin taken as centre of mass (:12-13)
            pts = np.asarray(body["voxelizedPoints"], dtype=np.float64)
            m_p = float(body["density"]) * float(c.V0)
            r2 = (pts * pts).sum(1)
            inertia = m_p * (np.eye(3) * r2.sum() - pts.T @ pts)
            if np.linalg.matrix_rank(inertia) < 3:   # degenerate (a single row of particles): regularise
                inertia = inertia + np.eye(3) * m_p * c.particle_diameter ** 2
            mass = float(c.rigid_body_masses[oid]) or m_p * len(pts)
            self.refresh()   # (device backend: what the other bodies did so far, before this one joins the read-back)
            self.bodies[oid] = (_DeviceBody if self.on_device else _Body)(oid, mass, inertia, translation, rot, vel)
            self.bodies[oid].points = pts
            if self.on_device:   # bullet_solver.py:86-127 on the device: the body, its particle set and its first pose
                c.engine.set_rigid_body(oid, mass, inertia, translation, rot, vel, np.zeros(3), com0=np.zeros(3), points=pts)
                self.bodies[oid]._solver = self
                c.rigid_body_velocities[oid] = vel
                continue
            if self._bullet is None and self.contact is None and not _WARNED[0] and not os.environ.get("SPH_RIGID_NATIVE_OK"):
                _WARNED[0] = True
                print("WARNING: dynamic rigid body %d is integrated by the built-in 'native' rigid backend: free-body motion under "
                      "gravity + the fluid wrench, wall contact by the body's axis-aligned extent, NO body-body contacts, friction or "
                      "contact torque (the reference uses PyBullet, bullet_solver.py).  Trajectories of bodies in contact diverge "
                      "from the reference; install pybullet and set SPH_RIGID_BACKEND=pybullet for its behaviour "
                      "(SPH_RIGID_NATIVE_OK=1 silences this).  SPH_RIGID_BACKEND=contact adds body-body contact, friction and "
                      "contact torque." % oid, file=sys.stderr, flush=True)
            if self._bullet is not None:
                self._bullet.add(body, mass, translation, angle, vel)
            self._push(self.bodies[oid], com0=np.zeros(3))
        for _ in self.rigid_blocks:
            raise NotImplementedError  # bullet_solver.py:133-135

    def _insert_scripted(self, body):
        """A scripted body enters with the zero-velocity pose of the time the running step ends at (prepare(): t = 0)."""
        c, oid = self.container, body["objectId"]
        motion = body.get("motionProgram") or RigidMotion.from_body(body, self.dt, method=getattr(c, "METHOD", None), dim=c.dim,
                                                                    backend=self.backend)
        pts = np.asarray(body["voxelizedPoints"], dtype=np.float64)
        com, rot = motion.pose(c.entry_step() * motion.dt)
        self.refresh()
        s = (_DeviceScripted if self.on_device else _Scripted)(oid, motion, com, rot, pts)
        self.scripted[oid] = s
        if self.on_device:   # the program goes to the device once; its launch moves the body from the next step on
            com_rest, rot_rest = motion.rest()
            c.engine.set_rigid_motion(oid, motion.to_struct(), com_rest, rot_rest, com0=np.zeros(3))
            s._solver = self
        else:
            self._push(s, com0=np.zeros(3))
        c.rigid_body_velocities[oid] = np.zeros(3)

    def scripted_wrench(self, oid):
        """(force, torque, impulse, angular impulse) of a scripted body: the fluid wrench its last step consumed and the sums of
        dt * force, dt * torque since it entered -- what wave tanks are validated with."""
        s = self.scripted[oid]
        return s.force.copy(), s.torque.copy(), s.impulse.copy(), s.angular_impulse.copy()

    def _push(self, b, com0=None):
        self.container.engine.set_rigid_pose(b.oid, b.com, b.rot, b.vel, b.angvel, com0=com0)
        self.container.rigid_body_velocities[b.oid] = b.vel

    # ------------------------------------------------------------------ bullet_solver.py:144-167
    def step(self):
        if not self.bodies and not self.scripted:
            return
        if self.on_device:
            self.container.engine.rigid_integrate()
            self._stale = True
            return
        force, torque = self.container.engine.get_rigid_wrench(reset=True)
        for s in self.scripted.values():   # every rank of a sharded scene evaluates the same closed form of the step count
            s.com, s.rot, s.vel, s.angvel = s.motion.step(self.container.step_count)
            s.force, s.torque = force[s.oid].astype(np.float64), torque[s.oid].astype(np.float64)
            s.impulse = s.impulse + self.dt * s.force
            s.angular_impulse = s.angular_impulse + self.dt * s.torque
            self._push(s)
        if self.contact is not None:
            table = self.container.engine.get_rigid_contacts(reset=True)
            self.contact.step(self.bodies, force.astype(np.float64), torque.astype(np.float64), contacts_from_table(table, self.bodies))
        elif self._bullet is not None:
            self._bullet.step(self.bodies, force, torque)
        else:
            for b in self.bodies.values():
                self.integrate(b, force[b.oid].astype(np.float64), torque[b.oid].astype(np.float64))
        for b in self.bodies.values():
            self._push(b)

    def integrate(self, b, force, torque):
        """One semi-implicit Euler step of a free rigid body: external force at the centre of mass + gravity, external
        torque, gyroscopic term; then the walls."""
        dt = self.dt
        b.vel = b.vel + dt * (force / b.mass + self.gravity)
        I_inv = b.rot @ b.I_body_inv @ b.rot.T
        I_w = b.rot @ b.I_body @ b.rot.T
        b.angvel = b.angvel + dt * (I_inv @ (torque - np.cross(b.angvel, I_w @ b.angvel)))
        b.com = b.com + dt * b.vel
        b.rot = _skew_exp(dt * b.angvel) @ b.rot
        u, _, vt = np.linalg.svd(b.rot)   # keep it a rotation
        b.rot = u @ vt
        # inelastic wall contact of the body's extent: bounds of its particle set in the current orientation, about the
        # centre of mass (a body without a particle set -- unit tests -- is a point)
        if b.points is not None and len(b.points):
            w = b.points @ b.rot.T
            ext_lo, ext_hi = w.min(0), w.max(0)
        else:
            ext_lo = ext_hi = np.zeros(3)
        for k in range(3):
            if b.com[k] + ext_lo[k] < self.wall_lo[k] and self.wall_lo[k] - ext_lo[k] <= self.wall_hi[k] - ext_hi[k]:
                b.com[k] = self.wall_lo[k] - ext_lo[k]
                b.vel[k] = max(b.vel[k], 0.0)
            elif b.com[k] + ext_hi[k] > self.wall_hi[k]:
                b.com[k] = max(self.wall_hi[k] - ext_hi[k], self.wall_lo[k] - ext_lo[k])
                b.vel[k] = min(b.vel[k], 0.0)

    def set_dt(self, dt):
        """Adaptive time stepping: the size of the running step, for the integrator and the host contact solver."""
        self.dt = float(dt)
        if self.contact_parameters is not None:
            self.contact_parameters.dt = self.dt

    def mark_stale(self):
        """The device has stepped: what the host holds of the bodies' state is out of date."""
        self._stale = self.on_device and bool(self.bodies or self.scripted)

    def refresh(self):
        """Device backend: bring the bodies' state back (one small copy per body, after draining the stream) if the device has stepped
        since the last time."""
        if not self._stale:
            return
        self._stale = False
        for oid, b in self.bodies.items():
            b.com, b.rot, b.vel, b.angvel = self.container.engine.get_rigid_state(oid)
            self.container.rigid_body_velocities[oid] = b.vel
        for oid, s in self.scripted.items():
            st = self.container.engine.get_rigid_motion_state(oid)
            for name in ("com", "rot", "vel", "angvel", "force", "torque", "impulse", "angular_impulse"):
                setattr(s, name, st[name])
            self.container.rigid_body_velocities[oid] = st["vel"]

    def get_rigid_body_states(self, container_idx):
        b = self.bodies.get(container_idx) or self.scripted[container_idx]
        return {"position": b.com.copy(), "rotation_matrix": b.rot.copy(), "linear_velocity": b.vel.copy(),
                "angular_velocity": b.angvel.copy()}


def contacts_from_table(table, bodies):
    """One contact per non-empty key (A, B, bin) of a dynamic body A: (A, B or None for an infinite-mass partner, point = mean midpoint,
    normal = normalised sum of depth * n (from B towards A), depth = maximum depth).  For the domain box and the wall planes (B >= 20)
    the normal is the bin's axis: their faces are axis-aligned planes, and the pair normals of a lattice sliding over the box's lattice
    tilt by up to 45 degrees with the offset between the two.  A pair of dynamic bodies is taken from the row of
    the lower id only: the other row holds the same pairs with opposite normals."""
    out = []
    A_idx, B_idx, bins = np.nonzero(table[..., 0] > 0)
    for a, b, k in zip(A_idx.tolist(), B_idx.tolist(), bins.tolist()):
        if a not in bodies:
            continue
        partner = b if (b < 20 and b in bodies) else None
        if partner is not None and partner < a:
            continue
        v = table[a, b, k]
        dn = v[4:7]
        nrm = float(np.linalg.norm(dn))
        if nrm <= 0.0:
            continue
        n = dn / nrm
        if b >= 20:   # the domain box / a wall plane: an axis-aligned face, its normal is the bin's axis
            n = np.zeros(3)
            n[k // 2] = -1.0 if k % 2 else 1.0
        out.append((a, partner, v[1:4] / v[0], n, float(v[7])))
    return out


def _tangents(n):
    t1 = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    t1 /= np.linalg.norm(t1)
    return t1, np.cross(n, t1)


class ContactSolver:
    """Sequential impulses on aggregated contacts, one body-level solve per step.

    Per step: v += dt (F / m + g), w += dt I^-1 (tau - w x I w) (the native integrator's velocity half); then `iterations` sweeps over
    all contacts with accumulated, clamped impulses -- normal lambda >= 0 towards the target normal velocity max(-e v_n, 0) (restitution
    only for approach speeds above 2 |g| dt, so a resting contact does not bounce), friction lambda_t within the Coulomb disc mu lambda_n
    -- and a rolling resistance within mu lambda_n * patch about the tangents (one aggregated point cannot carry the torque a face's
    pressure distribution does) -- then `iterations` sweeps of split impulses on pseudo-velocities that remove beta (depth - slop) / dt of the depth; positions move
    with v + the pseudo-velocity, which is then dropped (position correction adds no energy)."""

    def __init__(self, restitution=0.2, friction=0.5, iterations=10, gravity=(0.0, -9.81, 0.0), dt=1e-3, beta=0.2, slop=0.0):
        self.e, self.mu, self.iterations = float(restitution), float(friction), int(iterations)
        self.gravity, self.dt = np.asarray(gravity, dtype=np.float64), float(dt)
        self.beta, self.slop = float(beta), float(slop)
        self.patch = 0.0   # rolling-resistance radius of a contact patch (the backend sets D)

    def step(self, bodies, force, torque, contacts):
        dt = self.dt
        inv_i = {}
        for oid, b in bodies.items():
            b.vel = b.vel + dt * (force[oid] / b.mass + self.gravity)
            I_w = b.rot @ b.I_body @ b.rot.T
            inv_i[oid] = b.rot @ b.I_body_inv @ b.rot.T
            b.angvel = b.angvel + dt * (inv_i[oid] @ (torque[oid] - np.cross(b.angvel, I_w @ b.angvel)))
        pv = {oid: np.zeros(3) for oid in bodies}
        pw = {oid: np.zeros(3) for oid in bodies}
        rows = []
        v_thr = 2.0 * float(np.linalg.norm(self.gravity)) * dt
        for a, bb, p, n, depth in contacts:
            ra = p - bodies[a].com
            rb = p - bodies[bb].com if bb is not None else None
            t1, t2 = _tangents(n)

            def k_of(d):
                k = 1.0 / bodies[a].mass + d @ np.cross(inv_i[a] @ np.cross(ra, d), ra)
                if bb is not None:
                    k += 1.0 / bodies[bb].mass + d @ np.cross(inv_i[bb] @ np.cross(rb, d), rb)
                return k
            vn0 = self._rel(bodies, a, bb, ra, rb) @ n
            target = -self.e * vn0 if vn0 < -v_thr else 0.0
            bias = self.beta * max(depth - self.slop, 0.0) / dt
            kr = tuple(t @ inv_i[a] @ t + (t @ inv_i[bb] @ t if bb is not None else 0.0) for t in (t1, t2))
            rows.append(dict(a=a, b=bb, ra=ra, rb=rb, n=n, t=(t1, t2), kn=k_of(n), kt=(k_of(t1), k_of(t2)), kr=kr, target=target,
                             bias=bias, ln=0.0, lt=np.zeros(2), lr=np.zeros(2), lp=0.0))
        for _ in range(self.iterations):
            for c in rows:
                vrel = self._rel(bodies, c["a"], c["b"], c["ra"], c["rb"])
                ln = max(c["ln"] + (c["target"] - vrel @ c["n"]) / c["kn"], 0.0)
                self._apply(bodies, inv_i, c, (ln - c["ln"]) * c["n"])
                c["ln"] = ln
                vrel = self._rel(bodies, c["a"], c["b"], c["ra"], c["rb"])
                lt = c["lt"] - np.array([vrel @ c["t"][0] / c["kt"][0], vrel @ c["t"][1] / c["kt"][1]])
                cap, mag = self.mu * c["ln"], float(np.linalg.norm(lt))
                if mag > cap:
                    lt = lt * (cap / mag)
                d = lt - c["lt"]
                self._apply(bodies, inv_i, c, d[0] * c["t"][0] + d[1] * c["t"][1])
                c["lt"] = lt
                # rolling resistance of the contact patch (radius D): the relative spin about the tangents, within mu lambda_n D
                wrel = bodies[c["a"]].angvel - (bodies[c["b"]].angvel if c["b"] is not None else 0.0)
                lr = c["lr"] - np.array([wrel @ c["t"][0] / c["kr"][0], wrel @ c["t"][1] / c["kr"][1]])
                cap, mag = self.mu * c["ln"] * self.patch, float(np.linalg.norm(lr))
                if mag > cap:
                    lr = lr * (cap / mag)
                d = lr - c["lr"]
                self._apply_angular(bodies, inv_i, c, d[0] * c["t"][0] + d[1] * c["t"][1])
                c["lr"] = lr
        for _ in range(self.iterations):
            for c in rows:
                a, bb = c["a"], c["b"]
                vp = pv[a] + np.cross(pw[a], c["ra"])
                if bb is not None:
                    vp = vp - pv[bb] - np.cross(pw[bb], c["rb"])
                lp = max(c["lp"] + (c["bias"] - vp @ c["n"]) / c["kn"], 0.0)
                j = (lp - c["lp"]) * c["n"]
                c["lp"] = lp
                pv[a] = pv[a] + j / bodies[a].mass
                pw[a] = pw[a] + inv_i[a] @ np.cross(c["ra"], j)
                if bb is not None:
                    pv[bb] = pv[bb] - j / bodies[bb].mass
                    pw[bb] = pw[bb] - inv_i[bb] @ np.cross(c["rb"], j)
        for oid, b in bodies.items():
            b.com = b.com + dt * (b.vel + pv[oid])
            b.rot = _skew_exp(dt * (b.angvel + pw[oid])) @ b.rot
            u, _, vt = np.linalg.svd(b.rot)
            b.rot = u @ vt
        return rows

    @staticmethod
    def _rel(bodies, a, bb, ra, rb):
        v = bodies[a].vel + np.cross(bodies[a].angvel, ra)
        if bb is not None:
            v = v - bodies[bb].vel - np.cross(bodies[bb].angvel, rb)
        return v

    @staticmethod
    def _apply_angular(bodies, inv_i, c, m):
        bodies[c["a"]].angvel = bodies[c["a"]].angvel + inv_i[c["a"]] @ m
        if c["b"] is not None:
            bodies[c["b"]].angvel = bodies[c["b"]].angvel - inv_i[c["b"]] @ m

    @staticmethod
    def _apply(bodies, inv_i, c, j):
        a, bb = c["a"], c["b"]
        bodies[a].vel = bodies[a].vel + j / bodies[a].mass
        bodies[a].angvel = bodies[a].angvel + inv_i[a] @ np.cross(c["ra"], j)
        if bb is not None:
            bodies[bb].vel = bodies[bb].vel - j / bodies[bb].mass
            bodies[bb].angvel = bodies[bb].angvel - inv_i[bb] @ np.cross(c["rb"], j)


class _BulletBackend:   # pragma: no cover - needs pybullet (absent in this image)
    """The reference's PyBullet calls (bullet_solver.py:30-40, :86-127, :137-176)."""

    def __init__(self, container, gravity, dt):
        import pybullet as p
        import pybullet_data
        self.p, self.container, self.ids = p, container, {}
        self.client = p.connect(p.DIRECT)
        p.setAdditionalSearchPath(pybullet_data.getDataPath())
        p.setTimeStep(dt)
        p.setGravity(*[float(g) for g in gravity])

    def add(self, body, mass, translation, angle, vel):
        p = self.p
        mesh = body["geometryFile"]
        urdf = mesh[:-4] + ".urdf"
        s = body["scale"]
        with open(urdf, "w") as f:   # what SPH/utils create_urdf writes: one link, the mesh as visual + collision geometry
            f.write(f'<?xml version="1.0"?><robot name="b"><link name="base"><inertial><mass value="{mass}"/>'
                    f'<inertia ixx="1" ixy="0" ixz="0" iyy="1" iyz="0" izz="1"/></inertial>'
                    f'<collision><geometry><mesh filename="{mesh}" scale="{s[0]} {s[1]} {s[2]}"/></geometry></collision>'
                    f'</link></robot>')
        d = body["rotationAxis"]
        quat = p.getQuaternionFromEuler([d[0] * angle, d[1] * angle, d[2] * angle])
        self.ids[body["objectId"]] = p.loadURDF(urdf, basePosition=list(translation), baseOrientation=quat)
        os.remove(urdf)
        p.resetBaseVelocity(self.ids[body["objectId"]], list(vel))

    def step(self, bodies, force, torque):
        p = self.p
        for oid, b in bodies.items():
            pos, _ = p.getBasePositionAndOrientation(self.ids[oid])
            p.applyExternalForce(self.ids[oid], -1, forceObj=[float(x) for x in force[oid]], posObj=pos, flags=p.WORLD_FRAME)
            p.applyExternalTorque(self.ids[oid], -1, torqueObj=[float(x) for x in torque[oid]], flags=p.WORLD_FRAME)
        p.stepSimulation()
        for oid, b in bodies.items():
            lin, ang = p.getBaseVelocity(self.ids[oid])
            pos, orn = p.getBasePositionAndOrientation(self.ids[oid])
            b.com, b.vel, b.angvel = np.array(pos), np.array(lin), np.array(ang)
            b.rot = np.array(p.getMatrixFromQuaternion(orn)).reshape(3, 3)


PyBulletSolver = HostRigidSolver
