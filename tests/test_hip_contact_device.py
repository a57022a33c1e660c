"""GPU: the "device_contact" rigid backend (csrc/sph_contact_solve.hpp) -- the solve launch step by step against the host
solver it restates (contacts_from_table + ContactSolver.step), the consumed inputs, one device call against many, determinism, the
strict build against the fast one, no host work inside advance(), stacks at rest, late entry, the refusals and the driver.

The comparison to the host uses the project's bound for a device launch against its host statement, 1e-12 max(1, |x|), plus 256 S,
where S is how far the HOST solve moves when every input moves by one ulp: the conditioning of the contact system, measured on the
reference and not on the code under test.

Measured on an MI355X (30 steps of each of the two scenes, worst over both):
    strict build: worst difference to the host 8.9e-16, worst S 1.7e-14
    fast build:   worst difference to the host 1.8e-15, worst S 1.8e-14"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd.SPH.rigid_solver import host_rigid_solver as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
D = 0.02
DT = 4e-4
CUBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models", "cube.obj")


def _scene(bodies, box=True, method="wcsph", fluid_end=0.12):
    """tests/test_hip_contact.py's scene: a tiny fluid block in a corner of a 0.6-wide domain and cube.obj bodies at scale 0.2
    (3 x 3 x 3 particles): (object id, translation, axis, angle[, entryTime])."""
    cfg = P.dam_break_scene(method=method, domain_end=(0.6, 0.6, 0.6), start=(0.08, 0.08, 0.08), end=(fluid_end,) * 3,
                            translation=(0, 0, 0), dt=DT, add_domain_box=box)
    cfg["RigidBodies"] = [{"objectId": b[0], "geometryFile": CUBE, "translation": [float(x) for x in b[1]],
                           "rotationAxis": [float(x) for x in b[2]], "rotationAngle": float(b[3]), "scale": [0.2, 0.2, 0.2],
                           "velocity": [0, 0, 0], "density": 800.0, "color": [255, 255, 255], "isDynamic": True,
                           "entryTime": b[4] if len(b) > 4 else -1.0} for b in bodies]
    return cfg


def _build(cfg, monkeypatch, backend="device_contact", **opts):
    monkeypatch.delenv("SPH_RIGID_BACKEND", raising=False)
    monkeypatch.setenv("SPH_RIGID_NATIVE_OK", "1")
    container, solver = H.build_product(cfg, rigid_backend=backend, **opts)
    assert solver.rigid_solver.backend == backend
    solver.prepare()
    return container, solver


def _five():
    """the five jittered cubes of test_hip_contact.test_contact_pass_matches_the_restatement (its strict case)"""
    rng = np.random.default_rng(7)
    base = [(0.30, 0.098, 0.30), (0.356, 0.10, 0.30), (0.30, 0.10, 0.357), (0.33, 0.155, 0.33), (0.245, 0.10, 0.30)]
    return [(k + 1, np.array(t) + rng.uniform(-0.003, 0.003, 3), rng.normal(size=3), rng.uniform(-8, 8)) for k, t in enumerate(base)]


def _stack(box):
    return [(1, (0.3, 0.16, 0.3), (0, 1, 0), 0.0), (2, (0.3, 0.30, 0.3), (0, 1, 0), 0.0)]


_TWO = [(1, (0.3, 0.101, 0.3), (1, 0, 0), 7.0), (2, (0.31, 0.16, 0.305), (0, 0, 1), -5.0)]   # test_two_runs_are_bit_identical's cubes

# what the bodies are registered with once more (sph_set_rigid_body): linear and angular velocity, and for the stack the resting heights
# (penetration above the slop of 0.05 D, so the split impulses act).  Scene "five": 1 slides along the floor faster than friction can
# stop it, 2 all but rests (a body released at rest meets the restitution threshold 2 |g| dt exactly one step later), 3 leaves the floor, 4 comes down onto 1 / 2 / 3, 5 slides slowly.  Scene "stack": the lower cube rests on the floor
# plane, the upper one on it with a tangential speed friction removes within its cone.
_MOTION = {"five": {1: ((0.5, -0.003, 0.1), (0.0, 0.5, 0.0)), 2: ((0.002, -0.001, 0.0), (0.0, 0.01, 0.0)), 3: ((0.0, 0.3, 0.0), (0.3, 0.0, 0.0)),
                    4: ((0.0, -0.3, 0.0), (0.2, 0.1, -0.2)), 5: ((-0.004, -0.002, 0.002), (0.0, 0.0, 0.0))},
           "stack": {1: ((0.0, -0.001, 0.0), (0.0, 0.0, 0.0)), 2: ((0.001, 0.0, 0.0005), (0.0, 0.02, 0.0))}}


def _setup(monkeypatch, which, fast=0):
    """Scene `which` with every body registered once more through sph_set_rigid_body, as test_hip_rigid_device._setup does.  Returns
    container, solver and the test's own copy of what it uploaded: oid -> dict(mass, inertia, points)."""
    bodies, box = (_five(), True) if which == "five" else (_stack(False), False)
    container, solver = _build(_scene(bodies, box=box), monkeypatch, fast_math=fast)
    e, rs = container.engine, solver.rigid_solver
    assert rs.on_device and rs.contact is None
    mine = {}
    for oid, b in rs.bodies.items():
        pts = np.asarray(b.points, np.float64)
        rot, com = b.rot.copy(), b.com.copy()
        half = -pts[:, 1].min()
        if which == "stack":   # 1.5 mm inside the contact distance of the floor plane / of the lower cube's top layer
            com[1] = rs.wall_lo[1] + 0.5 * D + half - 0.0015 if oid == 1 else rs.wall_lo[1] + 0.5 * D + 3 * half + D - 0.003
        vel, angvel = (np.array(v, np.float64) for v in _MOTION[which][oid])
        e.set_rigid_body(oid, b.mass, b.I_body, com, rot, vel, angvel, com0=np.zeros(3), points=pts)
        mine[oid] = dict(mass=b.mass, inertia=b.I_body.copy(), points=pts)
    rs.mark_stale()
    return container, solver, mine


def _states(e, oids):
    return {oid: e.get_rigid_state(oid) for oid in oids}


def _snapshot(container, oids):
    e = container.engine
    ids = e.download(L.F_PARTICLE_ID)
    out = [H.by_id(ids, e.download(f)) for f in (L.F_POSITION, L.F_VELOCITY, L.F_DENSITY)]
    for oid in sorted(oids):
        out.extend(e.get_rigid_state(oid))
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the host side of the comparison
def host_solve(params, mine, before, force, torque, table, iterations=None):
    """contacts_from_table + ContactSolver.step on _Body copies of the states `before`.  Returns bodies, contacts, rows."""
    bodies = {}
    for oid, m in mine.items():
        com, rot, vel, angvel = before[oid]
        bodies[oid] = R._Body(oid, m["mass"], m["inertia"], com, rot, vel)
        bodies[oid].angvel = np.array(angvel, np.float64)
    solver = copy.copy(params)
    if iterations is not None:
        solver.iterations = iterations
    contacts = R.contacts_from_table(table, bodies)
    return bodies, contacts, solver.step(bodies, force, torque, contacts)


def flatten(bodies, contacts, rows):
    out = {name: np.stack([getattr(bodies[o], name) for o in sorted(bodies)]) for name in ("com", "rot", "vel", "angvel")}
    out["point"] = np.array([c[2] for c in contacts]).reshape(-1, 3)
    out["normal"] = np.array([c[3] for c in contacts]).reshape(-1, 3)
    out["depth"] = np.array([c[4] for c in contacts])
    out["ln"] = np.array([r["ln"] for r in rows])
    out["lt"] = np.array([r["lt"] for r in rows]).reshape(-1, 2)
    out["lr"] = np.array([r["lr"] for r in rows]).reshape(-1, 2)
    out["lp"] = np.array([r["lp"] for r in rows])
    return out


def one_ulp(rng, x):
    """every non-zero entry one ulp up or down"""
    x = np.array(x, np.float64)
    return np.where(x != 0.0, np.nextafter(x, np.where(rng.integers(0, 2, x.shape) == 1, np.inf, -np.inf)), x)


class Cases:
    """What the host rows of a run contained, and the conditions under which the bound of the comparison says something."""

    def __init__(self):
        self.seen = dict.fromkeys(("dynamic-dynamic", "domain box", "wall plane", "separating (ln == 0)", "friction at its cap",
                                   "friction inside its cap", "target > 0", "target == 0 and ln > 0", "lp > 0"), False)
        self.worst_s = 0.0

    def step(self, params, which, want, perturbed, bodies0, rows0, rows):
        """want / perturbed: the flattened host results; bodies0 / rows0: the host solve without sweeps (velocities behind the velocity
        half); rows: the host's rows after the solve"""
        s = max((float(np.max(np.abs(want[k] - perturbed[k]))) for k in want if want[k].size), default=0.0)
        assert s <= 1e-9, f"move the bodies: an ulp on the inputs moves the host solve by {s:.3e}"
        self.worst_s = max(self.worst_s, s)
        v_thr = 2.0 * float(np.linalg.norm(params.gravity)) * params.dt
        for c0, c in zip(rows0, rows):
            vn0 = float(R.ContactSolver._rel(bodies0, c0["a"], c0["b"], c0["ra"], c0["rb"]) @ c0["n"])
            assert abs(vn0 + v_thr) > 1e-6, f"move the bodies: approach speed {vn0} at the restitution threshold {-v_thr}"
            assert abs(abs(c["n"][0]) - 0.9) > 1e-3, f"move the bodies: normal {c['n']} at the tangent basis' switch"
            for name, cap, mag in (("friction", params.mu * c["ln"], float(np.linalg.norm(c["lt"]))),
                                   ("rolling", params.mu * c["ln"] * params.patch, float(np.linalg.norm(c["lr"])))):
                if cap <= 0.0:
                    continue
                at_cap, inside = abs(mag - cap) <= 1e-12 * cap, mag < cap * (1.0 - 1e-6)
                assert at_cap or inside, f"move the bodies: {name} {mag} within 1e-6 of its cap {cap}"
                if name == "friction":
                    self.seen["friction at its cap"] |= at_cap
                    self.seen["friction inside its cap"] |= inside
            self.seen["dynamic-dynamic"] |= c["b"] is not None
            self.seen["domain box"] |= c["b"] is None and which == "five"
            self.seen["wall plane"] |= c["b"] is None and which == "stack"
            self.seen["separating (ln == 0)"] |= c["ln"] == 0.0
            self.seen["target > 0"] |= c["target"] > 0.0
            self.seen["target == 0 and ln > 0"] |= c["target"] == 0.0 and c["ln"] > 0.0
            self.seen["lp > 0"] |= c["lp"] > 0.0
        return s

    def check(self):
        for name, seen in self.seen.items():
            assert seen, f"move the bodies: no row with {name} in the run"


def device_results(after, rows):
    """the device's states and rows in flatten's layout, and (A, B) of every row"""
    out = {name: np.stack([after[o][k] for o in sorted(after)]) for k, name in enumerate(("com", "rot", "vel", "angvel"))}
    out.update(point=rows[:, 2:5], normal=rows[:, 5:8], depth=rows[:, 8], ln=rows[:, 9], lt=rows[:, 10:12], lr=rows[:, 12:14], lp=rows[:, 14])
    return out, [(int(r[0]), int(r[1])) for r in rows]


# ------------------------------------------------------------------------------------------------ 1. one launch against the host
@pytest.mark.parametrize("fast", [0, 1])
def test_one_launch_against_the_host_solver(gpu, monkeypatch, fast):
    """30 steps of each scene; in each the launch on its own (sph_rigid_integrate between the halves) against contacts_from_table +
    ContactSolver.step applied to copies of the states before it, with the same wrench and the same table."""
    cases, worst = Cases(), 0.0
    rng = np.random.default_rng(2024)
    for which in ("five", "stack"):
        container, solver, mine = _setup(monkeypatch, which, fast)
        e, params = container.engine, solver.rigid_solver.contact_parameters
        for step in range(30):
            e.step_begin()
            before = _states(e, mine)
            force, torque = (w.astype(np.float64) for w in e.get_rigid_wrench(reset=False))
            table = e.get_rigid_contacts(reset=False)
            e.rigid_integrate()
            after, rows = _states(e, mine), e.get_rigid_contact_rows()
            e.step_end()
            bodies, contacts, host_rows = host_solve(params, mine, before, force, torque, table)
            want = flatten(bodies, contacts, host_rows)
            moved = {oid: tuple(one_ulp(rng, x) for x in st) for oid, st in before.items()}
            perturbed = flatten(*host_solve(params, mine, moved, one_ulp(rng, force), one_ulp(rng, torque), one_ulp(rng, table)))
            bodies0, _, rows0 = host_solve(params, mine, before, force, torque, table, iterations=0)
            s = cases.step(params, which, want, perturbed, bodies0, rows0, host_rows)
            got, pairs = device_results(after, rows)
            assert pairs == [(c[0], -1 if c[1] is None else c[1]) for c in contacts], (which, step, pairs, [c[:2] for c in contacts])
            for name in want:
                d = np.abs(got[name] - want[name])
                worst = max(worst, float(d.max()) if d.size else 0.0)
                assert np.all(d <= 1e-12 * np.maximum(1.0, np.abs(want[name])) + 256.0 * s), (which, step, name, float(d.max()), s)
        for oid in mine:   # the rotation stayed a rotation
            rot = e.get_rigid_state(oid)[1]
            assert np.allclose(rot @ rot.T, np.eye(3), rtol=0, atol=1e-12) and abs(np.linalg.det(rot) - 1.0) < 1e-12
        e.close()
    print(f"fast={fast}: worst difference to the host solve over 2 x 30 steps {worst:.3e}, worst S {cases.worst_s:.3e}")
    cases.check()


# ------------------------------------------------------------------------------------------------ 2. the launch consumes its inputs
def test_the_launch_consumes_its_inputs(gpu, monkeypatch):
    """a cube on the box floor (a table from the first step on) and test_hip_rigid_device's cube falling into a larger fluid block (a wrench)"""
    container, solver = _build(_scene([(1, (0.3, 0.099, 0.3), (0, 1, 0), 0.0), (2, (0.12, 0.18, 0.12), (0, 1, 0), 10.0)], fluid_end=0.16),
                               monkeypatch)
    e, rs = container.engine, solver.rigid_solver
    b = rs.bodies[2]   # on its way down and spinning, as test_hip_rigid_device registers it: viscous and pressure forces from the first steps
    e.set_rigid_body(2, b.mass, b.I_body, b.com, b.rot, np.array([0.0, -0.5, 0.0]), np.array([0.5, 1.0, -0.5]), com0=np.zeros(3), points=b.points)
    rs.mark_stale()
    wrench_seen = table_seen = False
    for _ in range(30):
        e.step_begin()
        force, torque = e.get_rigid_wrench(reset=False)
        table = e.get_rigid_contacts(reset=False)
        pairs = e.get_rigid_contact_pairs()
        wrench_seen |= bool(np.any(force != 0) and np.any(torque != 0))
        table_seen |= bool(table[..., 0].sum() > 0)
        e.rigid_integrate()
        f2, t2 = e.get_rigid_wrench(reset=False)
        assert not np.any(f2) and not np.any(t2) and not np.any(e.get_rigid_contacts(reset=False))
        assert e.get_rigid_contact_pairs() == pairs == int(table[..., 0].sum())   # the last pass is still reported
        e.step_end()
        if wrench_seen and table_seen:
            break
    assert wrench_seen and table_seen, (wrench_seen, table_seen)


# ------------------------------------------------------------------------------------------------ 3. one call equals many, repeats
@pytest.mark.parametrize("method", ["wcsph", "dfsph"])
def test_one_call_equals_many(gpu, monkeypatch, method):
    def run(how):
        container, solver = _build(_scene(_TWO, method=method), monkeypatch)
        how(solver)
        snap = _snapshot(container, (1, 2))
        rows = container.engine.get_rigid_contact_rows()
        container.engine.close()
        return snap, rows
    one, rows = run(lambda solver: solver.advance(25))
    many, _ = run(lambda solver: [solver.advance(1) for _ in range(25)])
    assert np.all(np.isfinite(one[0])) and len(rows) > 0   # the cubes touch
    assert _same(one, many)


def test_two_runs_are_bit_identical(gpu, monkeypatch):
    runs = []
    for _ in range(2):
        container, solver = _build(_scene(_TWO), monkeypatch)
        solver.advance(150)
        runs.append(_snapshot(container, (1, 2)) + [container.engine.get_rigid_contact_rows()])
        container.engine.close()
    assert len(runs[0][-1]) > 0 and _same(runs[0], runs[1])


def test_strict_and_fast_builds_give_the_same_bits(gpu, monkeypatch):
    """One launch from the same uploaded state and the same table in both builds.  The table is the contact pass's of the first step: an
    axis-aligned stack on the floor plane, whose pairs differ along one axis only, is the same table in both builds (no sum that a
    fused multiply-add could round differently) -- asserted, not assumed; the state is uploaded, tilted and moving, so that no product of
    the solve is trivial."""
    rot = R._rotation(0.3, np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0))
    got = []
    for fast in (0, 1):
        container, solver = _build(_scene([(1, (0.3, 0.0885, 0.3), (0, 1, 0), 0.0), (2, (0.3, 0.147, 0.3), (0, 1, 0), 0.0)], box=False),
                                   monkeypatch, fast_math=fast)
        e, rs = container.engine, solver.rigid_solver
        assert abs(rs.wall_lo[1] + 0.5 * D + 0.02 - 0.09) < 1e-9   # the lower cube's bottom layer is 1.5 mm inside the plane's distance
        for oid, b in rs.bodies.items():
            e.set_rigid_body(oid, b.mass, b.I_body, b.com + [0.001 * oid, 0.0005, -0.002], rot if oid == 1 else rot.T,
                             np.array([0.3, -0.2, 0.1]) * oid, np.array([1.0, -2.0, 0.5]) / oid, com0=np.zeros(3), points=b.points)
        e.step_begin()
        table = e.get_rigid_contacts(reset=False)
        before = _states(e, (1, 2))
        e.rigid_integrate()
        got.append((table, before, _states(e, (1, 2)), e.get_rigid_contact_rows()))
        e.step_end()
        e.close()
    (t0, b0, a0, r0), (t1, b1, a1, r1) = got
    assert np.array_equal(t0, t1) and t0[1, 20:, :, 0].sum() > 0 and t0[1, 2, :, 0].sum() > 0   # the floor plane and the dynamic pair
    assert len(r0) >= 2 and np.array_equal(r0, r1)
    for oid in (1, 2):
        assert _same(b0[oid], b1[oid]) and _same(a0[oid], a1[oid]), oid
        assert not np.array_equal(a0[oid][2], b0[oid][2])   # the solve moved it


# ------------------------------------------------------------------------------------------------ 4. no host in the loop
def test_no_host_in_the_loop(gpu, monkeypatch):
    container, solver = _build(_scene(_TWO), monkeypatch)
    e, rs = container.engine, solver.rigid_solver
    start = {oid: rs.bodies[oid].com.copy() for oid in (1, 2)}

    def never(*a, **k):
        raise AssertionError("the host was asked for the wrench, the table or a pose inside advance()")
    e.get_rigid_wrench = e.get_rigid_contacts = e.set_rigid_pose = never
    calls = []
    for name in ("step", "step_async", "step_begin"):
        def spy(*a, _orig=getattr(e, name), _name=name, **k):
            calls.append((_name, a))
            return _orig(*a, **k)
        setattr(e, name, spy)
    solver.advance(50)
    assert calls in ([("step", (50,))], [("step_async", (50,))]), calls
    assert len(e.get_rigid_contact_rows()) > 0   # touching bodies
    for oid in (1, 2):
        assert np.linalg.norm(rs.bodies[oid].com - start[oid]) > 1e-6, (oid, rs.bodies[oid].com, start[oid])


# ------------------------------------------------------------------------------------------------ 5. the physics holds
def _run(cfg, monkeypatch, steps):
    container, solver = _build(cfg, monkeypatch)
    rs = solver.rigid_solver
    gaps = []
    for _ in range(steps):
        solver.step()
        b1, b2 = rs.bodies[1], rs.bodies[2]
        x1 = b1.com + b1.points @ b1.rot.T
        x2 = b2.com + b2.points @ b2.rot.T
        gaps.append(np.sqrt(((x1[:, None] - x2[None]) ** 2).sum(-1)).min())
    return container, rs, np.array(gaps)


def test_cubes_rest_on_the_box_floor_and_on_each_other(gpu, monkeypatch):
    """tests/test_hip_contact.py's stack in a domain box, and that file's assertions"""
    container, rs, gaps = _run(_scene(_stack(True)), monkeypatch, 2000)
    b1, b2 = rs.bodies[1], rs.bodies[2]
    pts = b1.points
    half = -pts[:, 1].min()
    top_layer = 0.06                                   # the box floor's upper particle layer (padding 0.04 + one pitch)
    assert abs(b1.com[1] - (top_layer + D + half)) < 0.25 * D, b1.com
    assert abs(b2.com[1] - (b1.com[1] + pts[:, 1].max() + D + half)) < 0.25 * D, b2.com   # one pitch above the lower cube's top
    assert np.linalg.norm(b1.vel) < 0.02 and np.linalg.norm(b2.vel) < 0.02, (b1.vel, b2.vel)
    assert gaps.min() > 0.5 * D, gaps.min()


def test_stack_without_a_domain_box_rests_on_the_wall_planes(gpu, monkeypatch):
    container, rs, gaps = _run(_scene(_stack(False), box=False), monkeypatch, 2000)
    b1, b2 = rs.bodies[1], rs.bodies[2]
    half = -b1.points[:, 1].min()
    assert abs(b1.com[1] - (rs.wall_lo[1] + 0.5 * D + half)) < 0.25 * D, (b1.com, rs.wall_lo)
    assert abs(b2.com[1] - (b1.com[1] + b1.points[:, 1].max() + D + half)) < 0.25 * D, b2.com
    assert gaps.min() > 0.5 * D, gaps.min()
    assert np.linalg.norm(b1.vel) < 0.02 and np.linalg.norm(b2.vel) < 0.02, (b1.vel, b2.vel)


# ------------------------------------------------------------------------------------------------ 6. late entry
def test_a_late_body_lands_on_a_resting_one(gpu, monkeypatch):
    bodies = [(1, (0.3, 0.101, 0.3), (0, 1, 0), 0.0), (2, (0.3, 0.20, 0.3), (0, 1, 0), 0.0, 3 * DT)]
    container, solver = _build(_scene(bodies), monkeypatch)
    rs = solver.rigid_solver
    assert sorted(rs.bodies) == [1] and solver._host_acts_inside_a_step()
    solver.advance(10)
    assert sorted(rs.bodies) == [1, 2] and not solver._host_acts_inside_a_step()   # registered when it entered
    assert rs.bodies[2].com[1] < 0.20 - 1e-7
    solver.advance(1490)
    b1, b2 = rs.bodies[1], rs.bodies[2]
    half = -b1.points[:, 1].min()
    x1 = b1.com + b1.points @ b1.rot.T
    x2 = b2.com + b2.points @ b2.rot.T
    assert np.sqrt(((x1[:, None] - x2[None]) ** 2).sum(-1)).min() > 0.5 * D
    assert abs(b2.com[1] - (b1.com[1] + 2 * half + D)) < 0.25 * D, (b1.com, b2.com)
    assert np.linalg.norm(b1.vel) < 0.02 and np.linalg.norm(b2.vel) < 0.02, (b1.vel, b2.vel)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(gpu, monkeypatch):
    container, solver = H.build_product(P.pbf_scene(domain_end=(0.4, 0.4, 0.4), start=(0.1, 0.1, 0.1), end=(0.2, 0.2, 0.2)))
    with pytest.raises(L.SphError, match="PBF") as err:
        container.engine.set_rigid_contact_solver(True)
    assert err.value.code == L.ERR_UNSUPPORTED
    container.engine.close()
    # a sharded handle: one rank that owns every layer
    monkeypatch.setenv("SPH_COMM_TRANSPORT", "shm+ipc")
    buf = ctypes.create_string_buffer(128)
    assert L.load().sph_comm_unique_id(buf) == 0
    cfg = P.dam_break_scene(end=(0.2, 0.2, 0.2))
    from sph_project_amd import scene
    layers = int(scene.derive_geometry(H.SimConfig(config=cfg)).grid_num[2])
    container, solver = H.build_product(cfg, slab=dict(rank=0, nranks=1, unique_id=buf.raw, cuts=[0, layers]))
    with pytest.raises(L.SphError, match="sharded") as err:
        container.engine.set_rigid_contact_solver(True)
    assert err.value.code == L.ERR_UNSUPPORTED
    container.engine.close()
    # a plain handle
    z = np.zeros(3)
    container, solver = _build(_scene(_TWO), monkeypatch, backend="native")
    e = container.engine

    def invalid(call, match):
        with pytest.raises(L.SphError, match=match) as err:
            call()
        assert err.value.code == L.ERR_INVALID
    invalid(lambda: e.set_rigid_contact_solver(True), "integrator")
    e.set_rigid_integrator(True, (0.0, -9.8, 0.0), z, z + 0.6)
    invalid(lambda: e.set_rigid_contact_solver(True), "sph_set_rigid_contact is off")
    invalid(lambda: e.get_rigid_contact_rows(), "never enabled")
    e.set_rigid_contact(True, D, None, None)
    invalid(lambda: e.set_rigid_contact_solver(True, iterations=0), "iterations")
    invalid(lambda: e.set_rigid_contact_solver(True, iterations=65), "iterations")
    invalid(lambda: e.set_rigid_contact_solver(True, friction=-0.1), "negative")
    invalid(lambda: e.set_rigid_contact_solver(True, slop=float("nan")), "not finite")
    e.set_rigid_contact_solver(True, iterations=64)
    n = ctypes.c_int(-1)
    assert e.lib.sph_get_rigid_contact_rows(e.h, None, 0, ctypes.byref(n)) == 0 and n.value == 0   # capacity 0: still the count
    # without the integrator it cannot be turned on again
    e.set_rigid_contact(False)
    e.set_rigid_contact(True, D, None, None)
    e.set_rigid_integrator(False)
    invalid(lambda: e.set_rigid_contact_solver(True), "integrator")
    e.close()
    # capacity 0 after a solve with rows
    container, solver = _build(_scene(_TWO), monkeypatch)
    e = container.engine
    solver.advance(3)
    assert e.lib.sph_get_rigid_contact_rows(e.h, None, 0, ctypes.byref(n)) == 0 and n.value == len(e.get_rigid_contact_rows()) > 0
    one = np.zeros((1, L.CONTACT_ROW_VALUES))
    assert e.lib.sph_get_rigid_contact_rows(e.h, L._ptr(one), 1, ctypes.byref(n)) == 0 and n.value > 0
    assert np.array_equal(one[0], e.get_rigid_contact_rows()[0])


# ------------------------------------------------------------------------------------------------ 8. the driver
def test_driver_runs_the_coupling_scene_with_the_device_contact_backend(gpu, tmp_path, monkeypatch):
    from sph_project_amd import run_simulation
    cfg = P.coupling_scene(fluid_end=(0.8, 0.5, 0.8))
    cfg["Configuration"].update(exportPly=True, exportObj=True, outputInterval=1)
    f = tmp_path / "coupling.json"
    f.write_text(json.dumps(cfg))
    monkeypatch.delenv("SPH_RIGID_BACKEND", raising=False)
    out = tmp_path / "out"
    container, solver = run_simulation.main(["--scene_file", str(f), "--max_steps", "20", "--output_dir", str(out),
                                             "--rigid_backend", "device_contact"])
    rs = solver.rigid_solver
    assert rs.on_device and rs.backend == "device_contact" and len(rs.bodies) == 9
    frames = sorted(d for d in os.listdir(out) if (out / d).is_dir())
    assert len(frames) == 20, frames
    for oid in rs.bodies:
        st = rs.get_rigid_body_states(oid)
        assert all(np.all(np.isfinite(v)) for v in st.values()), (oid, st)
    names = os.listdir(out / frames[-1])
    assert any(n.endswith(".ply") for n in names) and any(n.startswith("mesh_object_") for n in names), names
