"""GPU: the rigid contact pass under z-slab sharding.  Two cubes slide into each other across the slab cut, 2 ranks on this box's one GPU
(shared-memory control plane and mailboxes), default and SPH_SLAB_LAYOUT=slow: every rank walks its own targets with ghosts as partners,
sph_get_rigid_contacts sums the table over the ranks (maxima for the depth) and maps it back to the scene frame, and every rank's host
solver integrates the same bodies.  Reference: the unsharded run of the same scene."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests.test_hip_contact import _scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0.02


def _collision_scene():
    # the box (its particles span all of z: the cut lands near the middle, z ~ 0.32) and, without gravity, two cubes flying head-on towards
    # each other along z at 0.5 m/s each (off the lattice by a few tenths of a millimetre: no pair sits at exactly D); they meet across the
    # cut after ~0.07 s
    cfg = _scene([(1, (0.3013, 0.3007, 0.2604), (0, 1, 0), 0.0), (2, (0.3031, 0.3019, 0.3811), (0, 1, 0), 0.0)], domain=0.64)
    cfg["Configuration"]["gravitation"] = [0.0, 0.0, 0.0]
    cfg["RigidBodies"][0]["velocity"] = [0.0, 0.0, 0.5]
    cfg["RigidBodies"][1]["velocity"] = [0.0, 0.0, -0.5]
    return cfg


@pytest.mark.parametrize("layout", ["", "slow"])
def test_two_cubes_colliding_across_a_slab_cut_match_the_unsharded_run(gpu, tmp_path, monkeypatch, layout):
    cfg = _collision_scene()
    steps = 300
    (tmp_path / "scene.json").write_text(json.dumps(cfg))
    uid = os.urandom(128).hex()
    env = dict(os.environ, SPH_COMM_TRANSPORT="shm", SPH_SLAB_REBALANCE="0", SPH_COMM_TIMEOUT_S="40", SPH_RIGID_NATIVE_OK="1")
    env.pop("SPH_RIGID_BACKEND", None)
    if layout:
        env["SPH_SLAB_LAYOUT"] = layout
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "contact_slab_worker.py"), str(r), "2", uid,
                               str(tmp_path / "scene.json"), str(steps), str(tmp_path / f"rank{r}.npz")], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-1500:] for l in logs)
    outs = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    assert all(str(o["transport"]) == "shm" for o in outs)
    # reference: one GPU
    monkeypatch.delenv("SPH_RIGID_BACKEND", raising=False)
    monkeypatch.setenv("SPH_RIGID_NATIVE_OK", "1")
    container, solver = H.build_product(cfg, rigid_backend="contact")
    solver.prepare()
    e, rs = container.engine, solver.rigid_solver
    tables, poses = [], []
    orig = e.get_rigid_contacts

    def spy(reset=True):
        t = orig(reset)
        tables.append(t[1:3].copy())
        return t
    e.get_rigid_contacts = spy
    for _ in range(steps):
        solver.step()
        poses.append(np.concatenate([rs.bodies[1].com, rs.bodies[2].com, rs.bodies[1].vel, rs.bodies[2].vel,
                                     rs.bodies[1].rot.ravel(), rs.bodies[2].rot.ravel()]))
    tables, poses = np.array(tables), np.array(poses)
    cut = int(outs[0]["z_hi"])
    # the cubes start on either side of the cut and collide: body-body keys appear, the bodies stop approaching
    z_cut = cut * float(container.dh)
    assert poses[0, 2] < z_cut < poses[0, 5], (poses[0, [2, 5]], z_cut)
    assert tables[:, 0, 2, :, 0].sum() > 0 and tables[:, 1, 1, :, 0].sum() > 0   # keys (1, 2, bin) and (2, 1, bin)
    assert poses[-1, 8] < 0.2 and poses[-1, 11] > -0.2, poses[-1, 6:12]   # the impact took the approach speed (restitution 0.2)
    for o in outs:   # both ranks read the same summed table and integrate the same bodies
        np.testing.assert_array_equal(o["tables"][..., 0], tables[..., 0])
        scale = np.maximum(np.abs(tables[..., 1:]), 1.0)
        assert np.all(np.abs(o["tables"][..., 1:] - tables[..., 1:]) <= 1e-5 * scale), np.abs(o["tables"][..., 1:] - tables[..., 1:]).max()
        assert np.abs(o["poses"] - poses).max() <= 1e-5, np.abs(o["poses"] - poses).max()
    np.testing.assert_array_equal(outs[0]["tables"], outs[1]["tables"])
    np.testing.assert_array_equal(outs[0]["poses"], outs[1]["poses"])
