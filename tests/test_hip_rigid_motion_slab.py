"""GPU, two ranks: a scripted rigid body under slab sharding with the native backend -- the scene of
test_hip_slab.py::test_dynamic_rigid_body_under_slab_sharding with the cube scripted to cross the slab face.  Every rank evaluates the
same closed form of the step index, so the body's particles are bit-equal to the unsharded run's; the fluid is held to that test's
drift bound.  Ranks are started the way test_hip_slab.py starts them (tests/slab_worker.py)."""
import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import slab
from tests import helpers as H
from tests import test_hip_slab as S

pytestmark = pytest.mark.gpu


def test_scripted_rigid_body_under_slab_sharding(gpu, tmp_path):
    (tmp_path / "cube.obj").write_text(S._CUBE_OBJ)
    cfg = H.dam_break_scene(domain_end=(0.6, 0.8, 0.64), end=(0.3, 0.16, 0.4), translation=(0.12, 0.06, 0.12), dt=4e-4, viscosity_b=0.5)
    # a quarter period in 62.5 steps: 7 cm along (0, -1, 2) / sqrt(5) -- across the slab face and 3 cm down into the fluid
    cfg["RigidBodies"] = [{"objectId": 1, "geometryFile": str(tmp_path / "cube.obj"), "isDynamic": False, "entryTime": -1.0,
                           "density": 600.0, "color": [200, 50, 50], "velocity": [0.0, 0.0, 0.0], "translation": [0.27, 0.27, 0.30],
                           "scale": [1, 1, 1], "rotationAngle": 20.0, "rotationAxis": [0, 1, 0],
                           "motion": {"harmonic": {"frequency": 10.0, "direction": [0, -1, 2], "amplitude": 0.07}}}]
    steps = 60
    S.TRANSPORT[0], S.LAYOUT[0] = "shm+ipc", ""
    outs, logs = S._run_ranks(cfg, 2, steps, tmp_path)
    container, solver = H.build_product(cfg)
    solver.prepare()
    for _ in range(steps):
        solver.step()
    e = container.engine
    ids = e.download(L.F_PARTICLE_ID)
    x_ref = H.by_id(ids, e.download(L.F_POSITION))
    v_ref = H.by_id(ids, e.download(L.F_VELOCITY))
    mat = H.by_id(ids, e.download(L.F_MATERIAL))
    body = solver.rigid_solver.scripted[1]
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids), "every particle owned by exactly one rank"
    x, v = np.empty_like(x_ref), np.empty_like(v_ref)
    owner = np.empty(len(ids), np.int32)
    for r, o in enumerate(outs):
        x[o["ids"]] = o["pos"]; v[o["ids"]] = o["vel"]; owner[o["ids"]] = r
    rigid = mat == 2
    d = H.drift(x, x_ref, container.dh)
    # where the body's particles started: the rest pose, t = 0
    com0, rot0 = body.motion.pose(0.0)
    z0 = (com0 + np.asarray(body.points, np.float64) @ rot0.T)[:, 2].astype(np.float32)
    started_up = int((slab.cell_layer(z0, container.dh, int(container.grid_num[2])) >= int(outs[0]["z_hi"])).sum())
    ended_up = int((owner[rigid] == 1).sum())
    print("scripted rigid under slab: drift fluid %.3e, rigid particles per rank %s, body com %s" % (
        d[~rigid].max(), np.bincount(owner[rigid], minlength=2), body.com))
    assert len(z0) == int(rigid.sum()) and 0 < started_up < ended_up, (started_up, ended_up, "particles changed owner across the face")
    assert body.com[2] > 0.30 + 0.05 and body.com[1] < 0.27 - 0.02, "it crossed the face and dipped into the fluid"
    np.testing.assert_array_equal(x[rigid], x_ref[rigid])
    np.testing.assert_array_equal(v[rigid], v_ref[rigid])
    assert d[~rigid].max() <= 1e-4
