"""GPU: surface reconstruction (csrc/sph_surface.hpp) against the float64 restatement in tests/surface_model.py, its
determinism, the in-situ path from a live handle, several fluid objects, C2 at full size with the memory cap, and the drivers."""
import json
import os

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd.surface import SPH_ERR_CAPACITY, SurfaceError, SurfaceReconstructor
from tests import helpers as H
from tests import surface_cases as SC
from tests import surface_model as SM

pytestmark = pytest.mark.gpu

# the three smooth shapes (tests/surface_cases.py): a jittered block with a coarse grid (B = 7, P = 343: 4 points per thread), a ball at
# the defaults (B = 14, 12 per thread, one part) and a torus at B = 10 (P = 1000: the 4-points-per-thread kernel again).  The paths these
# three never take -- 8 per thread, bricks in parts, chunked runs, the scan's carry, the other table rows -- are forced in
# tests/test_hip_surface_paths.py
CASES = SC.SMOOTH_CASES


@pytest.fixture(scope="module")
def models():
    return {name: SC.model(name) for name in CASES}


@pytest.mark.parametrize("name", list(CASES))
def test_mesh_matches_the_model(gpu, models, name):
    SC.check_mesh_against_model(*models[name], label=name)


@pytest.mark.parametrize("name", list(CASES))
def test_fast_build_mesh_matches_the_model(gpu, models, name):
    """The fast build (reciprocal-multiply binning, q = r * (1 / h), fused multiply-adds) gives the model's triangles and counts, and
    vertices and normals within the strict build's bounds: the extra rounding of 1 / h is one more ulp per term, inside the 12 u the
    bound allows per term."""
    SC.check_mesh_against_model(*models[name], fast_math=True, label=name)


def test_bytes_do_not_depend_on_runs_or_particle_order(gpu, models):
    x, c, t, _ = models["block"]
    r = SurfaceReconstructor(0.01, cube_size=c, iso=t)
    a = [arr.copy() for arr in r.from_points(x)]
    b = [arr.copy() for arr in r.from_points(x)]
    s = [arr.copy() for arr in r.from_points(x[np.random.default_rng(11).permutation(len(x))])]
    for u, w in zip(a, b):
        assert u.tobytes() == w.tobytes()
    for u, w in zip(a, s):
        assert u.tobytes() == w.tobytes()
    # the fast build is deterministic too (its own bytes)
    f = SurfaceReconstructor(0.01, cube_size=c, iso=t, fast_math=True)
    fa = [arr.copy() for arr in f.from_points(x)]
    fs = f.from_points(x[::-1].copy())
    assert all(u.tobytes() == w.tobytes() for u, w in zip(fa, fs))
    assert SM.closed_and_oriented(fa[1])


def test_from_container_equals_from_points_after_dfsph_steps(gpu):
    container, solver = H.build_product(P.dam_break_scene(method="dfsph", end=(0.2, 0.2, 0.2), dt=6e-4))
    solver.prepare()
    for _ in range(5):
        solver.step()
    (obj,) = tuple(container.object_id_fluid_body)
    r = SurfaceReconstructor(container.dx)
    a = [arr.copy() for arr in r.from_container(container, obj)]
    assert r.stats()["particles"] == container.particle_num[None]
    b = r.from_points(container.dump(obj_id=obj)["position"])
    assert len(a[1]) > 1000
    for u, w in zip(a, b):
        assert u.tobytes() == w.tobytes()
    assert SM.closed_and_oriented(a[1])


def _two_blocks():
    cfg = P.dam_break_scene(method="wcsph", end=(0.16, 0.16, 0.16))
    second = dict(cfg["FluidBlocks"][0])
    second.update(objectId=1, translation=[0.55, 0.1, 0.5])
    cfg["FluidBlocks"].append(second)
    return cfg


def test_two_fluid_objects_give_two_closed_meshes(gpu):
    container, solver = H.build_product(_two_blocks())
    solver.prepare()
    solver.step()
    assert sorted(container.object_id_fluid_body) == [0, 1]
    r = SurfaceReconstructor(container.dx)
    boxes = []
    for obj in (0, 1):
        v, tri, _ = r.from_container(container, obj)
        assert SM.closed_and_oriented(tri)
        assert SM.components_and_euler(len(v), tri) == (1, 2)
        pos = container.dump(obj_id=obj)["position"]
        assert r.stats()["particles"] == len(pos)
        h = 2 * 3.5 * container.dx
        assert (v.min(axis=0) >= pos.min(axis=0) - h).all() and (v.max(axis=0) <= pos.max(axis=0) + h).all()
        boxes.append((v.min(axis=0), v.max(axis=0)))
    assert (boxes[0][1][0] < boxes[1][0][0]) or (boxes[0][1][2] < boxes[1][0][2])   # apart


def _phi_at(points, x, h):
    """phi at a few points from the particles around them (their V from their own neighbours): cKDTree on f64."""
    from scipy.spatial import cKDTree
    tree = cKDTree(x)
    near = tree.query_ball_point(points, h)
    js = np.unique(np.concatenate([np.array(n, dtype=np.int64) for n in near]))
    V = np.zeros(len(x))
    for j, nb in zip(js, tree.query_ball_point(x[js], h)):
        V[j] = 1.0 / SM.kernel_w(np.linalg.norm(x[nb] - x[j], axis=1), h).sum()
    return np.array([(SM.kernel_w(np.linalg.norm(x[n] - p, axis=1), h) * V[n]).sum() if n else 0.0 for p, n in zip(points, near)])


def test_c2_full_size_from_rest_closed_inside_and_capped(gpu):
    container, solver = H.build_product(P.c2_scene())
    solver.prepare()
    (obj,) = tuple(container.object_id_fluid_body)
    n = container.particle_num[None]
    assert n > 1_200_000
    cap = 6 << 30
    r = SurfaceReconstructor(container.dx, memory_cap_bytes=cap)
    v, tri, nrm = r.from_container(container, obj)
    st = r.stats()
    assert st["particles"] == n and st["bytes_allocated"] <= cap
    print("c2 surface:", st)
    assert SM.closed_and_oriented(tri)
    assert SM.components_and_euler(len(v), tri)[0] == 1
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-5)
    # the inside test on points sampled around the block, off the grid lines
    x = container.dump(obj_id=obj)["position"].astype(np.float64)
    rng = np.random.default_rng(5)
    lo, hi = x.min(axis=0) - 0.05, x.max(axis=0) + 0.05
    axes = [np.sort(rng.uniform(lo[a], hi[a], 10)) for a in range(3)]
    inside = np.zeros(10 ** 3, np.uint8)
    vd = np.ascontiguousarray(v, dtype=np.float64)
    assert L.load().sph_points_in_mesh(vd.ctypes.data, len(vd), tri.ctypes.data, len(tri), axes[0].ctypes.data, 10, axes[1].ctypes.data, 10,
                                       axes[2].ctypes.data, 10, inside.ctypes.data) == 0
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    phi = _phi_at(pts, x, 2 * 3.5 * container.dx)
    sel = np.abs(phi - 0.6) > 1e-3
    assert sel.sum() > 500 and (phi[sel] > 0.6).sum() > 50
    assert ((inside[sel] == 1) == (phi[sel] > 0.6)).all()
    # a cap below what the frame needs: SPH_ERR_CAPACITY, nothing over-allocated, the object still usable
    small = SurfaceReconstructor(container.dx, memory_cap_bytes=64 << 20)
    with pytest.raises(SurfaceError) as ei:
        small.from_container(container, obj)
    assert ei.value.code == SPH_ERR_CAPACITY
    assert small.stats()["bytes_allocated"] <= 64 << 20
    v2, t2, _ = small.from_points(SM.lattice_ball((0.3, 0.3, 0.3), 0.06, 0.02))
    assert SM.closed_and_oriented(t2)


def test_reconstruct_object_checks_the_object_id(gpu):
    container, solver = H.build_product(P.dam_break_scene(end=(0.1, 0.1, 0.1)))
    solver.prepare()
    r = SurfaceReconstructor(container.dx)
    with pytest.raises(SurfaceError):
        r.from_container(container, 99)
    v, tri, _ = r.from_container(container, 5)   # no particle of that object: the empty mesh
    assert len(v) == 0 and len(tri) == 0


def test_driver_reconstruct_and_the_cli_write_the_same_obj_files(gpu, tmp_path):
    from sph_project_amd import run_simulation, surface_reconstruction
    cfg = _two_blocks()
    cfg["Configuration"].update(exportPly=True, outputInterval=2)
    f = tmp_path / "two.json"
    f.write_text(json.dumps(cfg))
    out = tmp_path / "out"
    run_simulation.main(["--scene_file", str(f), "--max_steps", "5", "--output_dir", str(out), "--reconstruct"])
    frames = sorted(d for d in os.listdir(out) if (out / d).is_dir())
    assert len(frames) >= 2
    first = {}
    for d in frames:
        files = sorted(os.listdir(out / d))
        assert files == ["particle_object_0.obj", "particle_object_0.ply", "particle_object_1.obj", "particle_object_1.ply"], files
        for k in (0, 1):
            p = out / d / f"particle_object_{k}.obj"
            first[p] = p.read_bytes()
            assert first[p].startswith(b"v ") and b"\nvn " in first[p] and b"\nf " in first[p]
            os.remove(p)
    jobs = surface_reconstruction.main(["--input_dir", str(out), "--radius", str(cfg["Configuration"]["particleRadius"])])
    assert len(jobs) == 2 * len(frames)
    for p, data in first.items():
        assert p.read_bytes() == data, p
