"""GPU: the PBF method (PBF.py of the reference) -- against the fixtures of tools/gen_golden_pbf.py phase by phase in both builds; the
refine walks per term against the float64 restatement of tests/pbf_terms.py (current positions, the step-start cell lists, recentred
walks counted) on the full-size C2 geometry from rest and in motion and next to domain-box particles; determinism and asynchronous
steps; the refusals; late entry; the driver."""
import ctypes
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from tests import helpers as H
from tests import pbf_terms as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pbf", "*.npz")))
FIX_IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
ULP = 2.0 ** -23


def _near_h_pairs(x, sort_x, h, gs, gn, rows):
    """Accepted pairs of the restatement's walk whose distance lies within a few ulp of h (f32 and f64 may decide them apart)."""
    o, i, j, R, r = T.stale_pairs(x, sort_x, h * (1 + 1e-5), gs, gn, rows)
    return int(np.count_nonzero(np.abs(r - h) <= 4e-6 * h))


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_pbf_matches_fixture(gpu, path, fast_math):
    """Step 1 of every fixture, phase by phase: rest volumes after prepare(), the non-pressure forces + x += dt v* + boundary
    (PH_NON_PRESSURE, PH_PBF_PREDICT) against the positions the reference's first refine iteration starts from, each refine
    iteration (PH_PBF_DENSITY_LAMBDA, PH_PBF_FIX_POSITION) from the reference's positions at its start -- rho, lambda, recentred
    walks, accepted pairs, positions after fix_position -- and the closing boundary + velocity (PH_PBF_FINISH) from the reference's
    last positions.  Each refine iteration starts from the REFERENCE's positions: after the first iteration the block scatters
    (centimetre moves, rho = 0 particles), and f32 differences of a device run left to itself grow without bound, so an
    end-of-step comparison of a free-running step is not meaningful."""
    z = np.load(path)
    cfg = json.loads(bytes(z["scene_json"]).decode())
    c, s = H.build_product(cfg, fast_math=fast_math)
    c.insert_object()
    s.rigid_solver.insert_rigid_object()
    e = c.engine
    assert e.particle_num == z["init_positions"].shape[0]
    np.testing.assert_array_equal(e.download(L.F_MATERIAL), z["init_materials"])
    e.upload(L.F_POSITION, z["init_positions"])
    e.upload(L.F_VELOCITY, z["init_velocities"])
    s.prepare()
    h, gs, gn = float(z["geo_dh"]), float(np.float32(z["geo_grid_size"])), z["geo_grid_num"]
    rho0, dt = float(z["density_0"]), float(z["dt"])
    fid = z["s1_ids"]
    mat_f = z["s1_materials"]
    vol_f, mass_f = z["s1_rest_volumes"], z["s1_masses"]
    sort_x = z["s1_sort_positions"]
    ids = e.download(L.F_PARTICLE_ID)
    to_dev = lambda a: H.by_id(fid, a)[ids]          # fixture order -> device order
    get = lambda f: H.by_id(ids, e.download(f))[fid]  # device order -> fixture order
    # rigid volumes (poly6, W(0) = 0): computed at prepare(), unchanged by the step (static boundary)
    rg = mat_f == 2
    if rg.any():
        v = get(L.F_REST_VOLUME)
        np.testing.assert_allclose(v[rg], vol_f[rg], rtol=2e-6, atol=0)
    # non-pressure forces (poly6 surface tension incl. the kernel_W(diameter) branch, spiky viscosity) + predict + boundary
    s.engine.run_phase(L.PH_NEIGHBOR_SEARCH)
    s.engine.run_phase(L.PH_NON_PRESSURE)
    s.engine.run_phase(L.PH_PBF_PREDICT)
    x_dev = get(L.F_POSITION).astype(np.float64)
    x0 = z["s1_k1_x_before"].astype(np.float64)
    a_est = np.abs((x0 - sort_x) / dt - z["init_velocities"][fid]) / dt
    bound = 4 * ULP * np.abs(x0) + dt * dt * (1e-4 * a_est + 1e-3)
    err = np.abs(x_dev - x0)
    assert (err <= bound).all(), (err / bound).max()
    np.testing.assert_array_equal(get(L.F_PBF_OLD_POSITION), sort_x)   # save_old_position: the sort's positions
    fl = mat_f == 1
    for k in range(1, 6):
        xk = z[f"s1_k{k}_x_before"]
        e.upload(L.F_POSITION, to_dev(xk))
        ev0 = e.stats()["pair_evaluations"]
        s.compute_density_and_lambda()
        st = e.stats()
        assert st["pbf_recentred"] == int(z[f"s1_k{k}_recentred"]), k
        rows = np.nonzero(fl & np.isfinite(xk).all(axis=1))[0]
        r = T.density_lambda(xk, sort_x, vol_f, mass_f, mat_f, h, gs, gn, rho0, rows)
        pairs = st["pair_evaluations"] - ev0
        assert abs(pairs - r["pairs"]) <= _near_h_pairs(xk, sort_x, h, gs, gn, rows), (k, pairs, r["pairs"])
        rho, lam = get(L.F_DENSITY), get(L.F_PBF_LAMBDA)
        err = np.abs(rho[rows] - z[f"s1_k{k}_rho"][rows])
        assert (err <= 2 * r["rho_b"]).all(), (k, (err / r["rho_b"]).max())
        err = np.abs(lam[rows] - z[f"s1_k{k}_lambda"][rows])
        assert (err <= 2 * r["lam_b"]).all(), (k, (err / r["lam_b"]).max())
        s.fix_position()
        xa = get(L.F_POSITION).astype(np.float64)
        f_dev = T.fix_delta(xk, sort_x, lam, vol_f, mass_f, mat_f, h, gs, gn, rho0, rows)
        f_ref = T.fix_delta(xk, sort_x, z[f"s1_k{k}_lambda"], vol_f, mass_f, mat_f, h, gs, gn, rho0, rows)
        bound = f_dev["dx_b"] + f_ref["dx_b"] + np.abs(f_dev["dx"] - f_ref["dx"]) + 4 * ULP * np.abs(xk[rows])
        err = np.abs(xa[rows] - z[f"s1_k{k}_x_after"][rows])
        assert (err <= bound).all(), (k, (err / bound).max())
        assert xa[~fl].tobytes() == z[f"s1_k{k}_x_after"][~fl].astype(np.float64).tobytes()
    # boundary + v = (x - x_old) / dt from the reference's last positions
    e.upload(L.F_POSITION, to_dev(z["s1_k5_x_after"]))
    s.engine.run_phase(L.PH_PBF_FINISH)
    xe, ve = get(L.F_POSITION), get(L.F_VELOCITY)
    np.testing.assert_array_equal(xe[fl], z["s1_positions"][fl])
    vz = z["s1_velocities"].astype(np.float64)
    np.testing.assert_allclose(ve[fl], vz[fl], rtol=4 * ULP, atol=4 * ULP * np.abs(xe[fl]).max() / dt)
    c.engine.close()


def _geo(container):
    from sph_project_amd import scene
    g = scene.derive_geometry(container.cfg)
    return float(container.dh), float(np.float32(g.grid_size)), np.asarray(g.grid_num, np.int64)


def _check_refine_terms(container, solver, nrows=3000, seed=0):
    """One refine iteration (PH_PBF_DENSITY_LAMBDA, PH_PBF_FIX_POSITION) on the product's state against the restatement; returns
    the recentred count of the walk."""
    e = container.engine
    h, gs, gn = _geo(container)
    rho0 = float(solver.density_0)
    x = e.download(L.F_POSITION)
    sort_x = e.download(L.F_PBF_OLD_POSITION)
    mat = e.download(L.F_MATERIAL)
    vol, mass = e.download(L.F_REST_VOLUME), e.download(L.F_MASS)
    fl = np.nonzero((mat == 1) & np.isfinite(x).all(axis=1))[0]
    rows = np.sort(np.random.default_rng(seed).choice(fl, size=min(nrows, len(fl)), replace=False))
    solver.compute_density_and_lambda()
    st = solver.stats()
    want = T.recentred(x, sort_x, gs, gn, mat)
    assert st["pbf_recentred"] == want, (st["pbf_recentred"], want)
    rho, lam = e.download(L.F_DENSITY), e.download(L.F_PBF_LAMBDA)
    r = T.density_lambda(x, sort_x, vol, mass, mat, h, gs, gn, rho0, rows)
    err = np.abs(rho[rows] - r["rho"])
    assert (err <= r["rho_b"]).all(), (err / r["rho_b"]).max()
    err = np.abs(lam[rows] - r["lam"])
    assert (err <= r["lam_b"]).all(), (err / r["lam_b"]).max()
    solver.fix_position()
    x2 = e.download(L.F_POSITION)
    f = T.fix_delta(x, sort_x, lam, vol, mass, mat, h, gs, gn, rho0, rows)
    dx = x2[rows].astype(np.float64) - x[rows].astype(np.float64)
    bound = f["dx_b"] + 2 * np.abs(x[rows]) * 2.0 ** -24 + 1e-12
    err = np.abs(dx - f["dx"])
    assert (err <= bound).all(), (err / bound).max()
    assert x2[mat != 1].tobytes() == x[mat != 1].tobytes()   # only fluid particles move
    return want


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("steps", [1, 10])
def test_pbf_per_term_c2(gpu, fast_math, steps):
    """C2 geometry (1,231,200 particles) after `steps` steps: from rest and in motion; in motion particles have crossed cell faces
    since the step's sort, so the recentred walks are exercised."""
    c, s = H.build_product(P.c2_scene("pbf"), fast_math=fast_math)
    s.prepare()
    s.advance(steps)
    rc = _check_refine_terms(c, s, nrows=2000, seed=steps)
    if steps > 1:
        assert rc > 0
    c.engine.close()


def check_per_term_boundary(fast_math, layers=None):
    """layers: in a domain of that many cell layers in z (tests/helpers.py with_layers; tests/test_hip_tall_grid.py)"""
    cfg = P.pbf_scene(domain_end=(0.5, 0.5, 0.5), end=(0.3, 0.3, 0.3))
    if layers is not None:
        cfg = H.with_layers(cfg, layers)
    c, s = H.build_product(cfg, fast_math=fast_math)
    s.prepare()
    assert layers is None or c.engine.grid_layout()["nz"] == layers
    s.advance(3)
    mat = c.engine.download(L.F_MATERIAL)
    assert (mat == 2).any()
    _check_refine_terms(c, s, nrows=3000)
    c.engine.close()


@pytest.mark.parametrize("fast_math", [0, 1])
def test_pbf_per_term_boundary(gpu, fast_math):
    """A block in the domain box: rigid neighbours in lambda and fix_position, poly6 rigid volumes."""
    check_per_term_boundary(fast_math)


def _small(**opts):
    c, s = H.build_product(P.pbf_scene(domain_end=(0.5, 0.5, 0.5), end=(0.25, 0.3, 0.25)), **opts)
    s.prepare()
    return c, s


def test_pbf_deterministic_and_async(gpu):
    runs = []
    for asynchronous in (False, True, False):
        c, s = _small()
        if asynchronous:
            c.engine.step_async(20)
            c.engine.synchronize()
        else:
            c.engine.step(20)
        st = c.engine.stats()
        assert st["steps"] == 20
        runs.append([c.engine.download(f) for f in (L.F_POSITION, L.F_VELOCITY, L.F_DENSITY, L.F_PBF_LAMBDA)])
        c.engine.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.tobytes() == b.tobytes()


def test_pbf_refuses_implicit_viscosity(gpu):
    cfg = P.pbf_scene(domain_end=(0.5, 0.5, 0.5), end=(0.2, 0.2, 0.2))
    cfg["Configuration"]["viscosityMethod"] = "implicit"
    c, s = H.build_product(cfg)
    with pytest.raises(L.SphError) as ei:
        s.prepare()
    assert "implicit viscosity" in str(ei.value), str(ei.value)
    c.engine.close()


def test_pbf_sharded_is_unsupported(gpu, monkeypatch):
    monkeypatch.setenv("SPH_COMM_TRANSPORT", "shm+ipc")
    lib = L.load()
    buf = ctypes.create_string_buffer(128)
    assert lib.sph_comm_unique_id(buf) == 0
    cfg = P.dam_break_scene(method="pbf", end=(0.2, 0.2, 0.2))
    from sph_project_amd import scene
    from sph_project_amd.SPH.utils import SimConfig
    layers = int(scene.derive_geometry(SimConfig(config=cfg)).grid_num[2])
    c, s = H.build_product(cfg, slab=dict(rank=0, nranks=1, unique_id=buf.raw, cuts=[0, layers]))
    with pytest.raises(L.SphError) as ei:
        s.prepare()
    assert "one GPU only" in str(ei.value), str(ei.value)
    c.engine.close()


def test_pbf_late_entry_never_inserted(gpu):
    """PBF.py's _step calls no insert_object: block 1 (entryTime 2.5 dt) never appears."""
    cfg = P.dam_break_scene(method="pbf", end=(0.12, 0.1, 0.12), velocity=(0.0, -0.5, 0.0))
    cfg["FluidBlocks"].append({
        "objectId": 1, "start": [0.0, 0.0, 0.0], "end": [0.07, 0.07, 0.09], "translation": [0.12, 0.2, 0.11],
        "scale": [1, 1, 1], "velocity": [0.0, -1.0, 0.0], "density": 1000.0, "color": [9, 9, 9], "entryTime": 2.5 * 4e-4,
    })
    c, s = H.build_product(cfg)
    s.prepare()
    n0 = c.particle_num[None]
    for _ in range(6):
        s.step()
    assert c.particle_num[None] == n0
    assert c.engine.stats()["steps"] == 6
    c.engine.close()


def test_run_simulation_pbf(gpu, tmp_path):
    cfg = P.pbf_scene(domain_end=(0.5, 0.5, 0.5), start=(0.1, 0.1, 0.1), end=(0.2, 0.2, 0.2), add_domain_box=False, dt=8e-4)
    cfg["Configuration"].update(exportPly=True, outputInterval=5, totalTime=0.0204)   # 25 steps, a frame every 5
    scene_file = tmp_path / "pbf_scene.json"
    scene_file.write_text(json.dumps(cfg))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sph_project_amd", "run_simulation.py"), "--scene_file", str(scene_file),
                        "--output_dir", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Simulation method: pbf" in r.stdout
    frames = sorted(p.name for p in out.iterdir())
    assert frames == [f"{k:06}" for k in range(0, 25, 5)], frames
    for f in frames:
        head = (out / f / "particle_object_0.ply").read_text(errors="replace").splitlines()
        assert head[0] == "ply" and "element vertex 125" in head
