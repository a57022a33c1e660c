"""GPU: the consistent PBF variant (Configuration.pbfVariant "consistent") against the float64 restatement of
tests/pbf_consistent_terms.py phase by phase in both builds, the stop test, repeatability, a block that holds together, the refusals,
the untouched reference variant and the driver.

Tolerance of every compared quantity q: 4 max|model32(q) - model64(q)| + 1e-6 max|model64(q)| (the foam tests' bound):
the model's own float32 error on the same input, never the device's.  Worst observed error / bound ratios:
profiles/pbf_consistent_gpu_tests.txt."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from tests import helpers as H
from tests import pbf_consistent_terms as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _check(what, dev, m32, m64, rows=slice(None)):
    """|dev - model64| <= 4 max|model32 - model64| + 1e-6 max|model64| on `rows`; prints the worst error / bound ratio."""
    d, a, b = np.asarray(dev, F64)[rows], np.asarray(m32, F64)[rows], np.asarray(m64, F64)[rows]
    bound = 4.0 * float(np.abs(a - b).max()) + 1e-6 * float(np.abs(b).max())
    err = float(np.abs(d - b).max())
    print(f"  {what}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound > 0 else 0.0:.3f}")
    assert err <= bound, (what, err, bound)


def _start(case, **opts):
    """The product on the seeded state of a phase case, prepared: (container, solver, x, v, vol, mat, geo) in device order."""
    scene, spacing, jitter, seed = M.PHASE_CASES[case]
    keys = opts.pop("keys", {})
    layers = opts.pop("layers", None)   # in a domain of that many cell layers in z (tests/helpers.py with_layers)
    cfg = scene(**keys)
    if layers is not None:
        cfg = H.with_layers(cfg, layers)
    c, s = H.build_product(cfg, **opts)
    c.insert_object()
    s.rigid_solver.insert_rigid_object()
    e = c.engine
    x0, v0, _, mat0, _, geo = M.host_state(cfg, spacing, jitter, seed)
    assert e.particle_num == len(x0)
    np.testing.assert_array_equal(e.download(L.F_MATERIAL), mat0)
    e.upload(L.F_POSITION, x0)
    e.upload(L.F_VELOCITY, v0)
    s.prepare()
    ids = e.download(L.F_PARTICLE_ID)
    x, v = e.download(L.F_POSITION), e.download(L.F_VELOCITY)
    assert x.tobytes() == x0[ids].tobytes() and v.tobytes() == v0[ids].tobytes()
    return c, s, x, v, e.download(L.F_REST_VOLUME), e.download(L.F_MATERIAL), geo


def check_phases(case, fast_math, layers=None):
    """layers: on the case's twin in a domain of that many cell layers in z (tests/test_hip_tall_grid.py)"""
    c, s, x, v, vol, mat, geo = _start(case, fast_math=fast_math, layers=layers)
    e = c.engine
    assert layers is None or (e.grid_layout()["nz"] == layers == int(geo.grid_num[2]))
    fl = mat == 1
    assert s.variant == "consistent" and (case == "box") == bool((~fl).any())
    pairs = M.sorted_pairs(x, geo.h, geo.grid_num, fl)
    assert M.near_h_pairs(x, geo.h, geo.grid_num, fl) == 0
    print(f"{case} fast_math={fast_math}: {len(x)} particles, {int(fl.sum())} fluid, {len(pairs[0])} pairs")
    s.predict_position()
    xs = e.download(L.F_PREDICTED_POS)
    _check("predict x*", xs, M.predict(x, v, mat, geo, F32), M.predict(x, v, mat, geo), fl)
    assert xs[~fl].tobytes() == x[~fl].tobytes() and e.download(L.F_POSITION).tobytes() == x.tobytes()   # posv keeps x
    xs = M.predict(x, v, mat, geo).astype(F32)
    eps = M.DEFAULTS["epsilon"]
    for k in range(3):
        e.upload(L.F_PREDICTED_POS, xs)
        ev0 = e.stats()["pair_evaluations"]
        s.compute_density_and_lambda()
        assert e.stats()["pair_evaluations"] - ev0 == len(pairs[0]), k
        a32, a64 = M.walk_a(x, xs, vol, mat, pairs, geo, eps, F32), M.walk_a(x, xs, vol, mat, pairs, geo, eps)
        _check(f"k{k} rho", e.download(L.F_DENSITY), a32["rho"], a64["rho"], fl)
        _check(f"k{k} lambda", e.download(L.F_PBF_LAMBDA), a32["lam"], a64["lam"], fl)
        st = e.pbf_stats()
        assert st["iterations"] == 1 and st["variant"] == 1
        _check(f"k{k} sum C", [st["error"] * int(fl.sum())], [a32["sumC"]], [a64["sumC"]])
        lam = a64["lam"].astype(F32)
        e.upload(L.F_PBF_LAMBDA, lam)
        ev0 = e.stats()["pair_evaluations"]
        s.fix_position()
        assert e.stats()["pair_evaluations"] - ev0 == len(pairs[0]), k
        b64 = M.walk_b(x, xs, lam, vol, mat, pairs, geo)
        _check(f"k{k} x* after B", e.download(L.F_PREDICTED_POS), M.walk_b(x, xs, lam, vol, mat, pairs, geo, F32), b64, fl)
        assert e.download(L.F_POSITION).tobytes() == x.tobytes()
        xs = b64.astype(F32)
    e.upload(L.F_PREDICTED_POS, xs)
    s.finish_position()
    x32, v32 = M.finish(x, xs, v, mat, geo, F32)
    x64, v64 = M.finish(x, xs, v, mat, geo)
    xe, ve = e.download(L.F_POSITION), e.download(L.F_VELOCITY)
    _check("finish x", xe, x32, x64, fl)
    _check("finish v", ve, v32, v64, fl)
    assert xe[~fl].tobytes() == x[~fl].tobytes() and ve[~fl].tobytes() == v[~fl].tobytes()
    c.engine.close()


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("case", sorted(M.PHASE_CASES))
def test_phases_match_the_model(gpu, case, fast_math):
    """predict, three iterations of walk A and walk B, finish; every phase starts from inputs uploaded from the model."""
    check_phases(case, fast_math)


def _solve_start(**opts):
    """x* at the start of step 1's solve, read from a handle that runs the step's phases up to predict."""
    c, s, x, v, vol, mat, geo = _start("block", keys=M.STOP_KEYS, **opts)
    e = c.engine
    for ph in (L.PH_NEIGHBOR_SEARCH, L.PH_DENSITY, L.PH_NON_PRESSURE, L.PH_PBFC_PREDICT):
        e.run_phase(ph)
    assert e.download(L.F_POSITION).tobytes() == x.tobytes()   # nothing moved in the sort
    xs = e.download(L.F_PREDICTED_POS)
    e.close()
    return x, xs, vol, mat, geo


@pytest.mark.parametrize("fast_math", [0, 1])
def test_stop_test_matches_the_model(gpu, fast_math):
    x, xs, vol, mat, geo = _solve_start(fast_math=fast_math)
    thr = M.STOP_KEYS["pbfMaxError"]
    r32 = M.solve(x, xs, vol, mat, geo, max_error=thr, dtype=F32)
    r64 = M.solve(x, xs, vol, mat, geo, max_error=thr)
    assert all(not (thr / 1.5 <= err <= thr * 1.5) for err in r64["errs"]), r64["errs"]
    assert r32["iterations"] == r64["iterations"] > 2
    c, s, *_ = _start("block", keys=M.STOP_KEYS, fast_math=fast_math)
    c.engine.step(1)
    print(f"stop test fast_math={fast_math}: {s.iterations} iterations, error {s.density_error:.4e}; model {r64['iterations']}, {r64['error']:.4e}")
    assert s.iterations == r64["iterations"]
    _check("reported error", [s.density_error], [r32["error"]], [r64["error"]])
    assert s.density_error <= thr
    c.engine.close()
    c, s, *_ = _start("block", keys=M.STOP_KEYS, fast_math=fast_math, fixed_iterations=4)
    c.engine.step(1)
    assert s.iterations == 4 and s.density_error == 0.0
    c.engine.close()


def _box(**opts):
    c, s = H.build_product(M.box_scene(), **opts)
    s.prepare()
    return c, s


FIELDS = (L.F_POSITION, L.F_VELOCITY, L.F_DENSITY, L.F_PBF_LAMBDA, L.F_PARTICLE_ID)


def test_repeatable_and_step_counts_agree(gpu):
    """deterministic = 1 (the containers' default): two runs of 20 steps give the same bits, and one sph_step(h, 20) equals 20 calls."""
    runs = []
    for mode in ("one", "one", "twenty"):
        c, s = _box()
        if mode == "one":
            c.engine.step(20)
        else:
            for _ in range(20):
                c.engine.step(1)
        assert c.engine.stats()["steps"] == 20 and c.engine.stats()["pbf_recentred"] == 0
        runs.append([c.engine.download(f) for f in FIELDS] + [c.engine.pbf_stats()])
        c.engine.close()
    assert np.isfinite(runs[0][0]).all() and 0 < runs[0][-1]["iterations"] < 50
    for other in runs[1:]:
        assert other[-1] == runs[0][-1]
        for a, b in zip(runs[0][:-1], other[:-1]):
            assert a.tobytes() == b.tobytes()


def test_async_needs_fixed_iterations_and_matches_the_synchronous_run(gpu):
    c, s = _box()
    with pytest.raises(L.SphError) as ei:
        c.engine.step_async(2)
    assert ei.value.code == L.ERR_UNSUPPORTED and "fixed_iterations" in str(ei.value)
    s.step()   # the solver's own rule (base_solver.py) takes the synchronous call
    assert c.engine.stats()["steps"] == 1
    c.engine.close()
    runs = []
    for asynchronous in (False, True):
        c, s = _box(fixed_iterations=4)
        if asynchronous:
            c.engine.step_async(20)
            c.engine.synchronize()
        else:
            c.engine.step(20)
        assert c.engine.pbf_stats() == dict(variant=1, iterations=4, error=0.0)
        runs.append([c.engine.download(f) for f in FIELDS])
        c.engine.close()
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_a_block_holds_together(gpu):
    """An 8 x 12 x 8 block in a corner of a clamp-only box, 300 steps at the defaults: finite, inside the box, every sampled solve
    converged, and the block has slumped.  (The reference variant on this scene is what DESIGN.md 12 describes.)"""
    cfg = P.pbf_consistent_scene(domain_end=(0.5, 0.5, 0.5), start=(0.05, 0.05, 0.05), end=(0.205, 0.285, 0.205), add_domain_box=False, dt=1e-3)
    c, s = H.build_product(cfg)
    s.prepare()
    e = c.engine
    x0 = e.download(L.F_POSITION)
    assert len(x0) == 8 * 12 * 8 and abs(float(x0[:, 1].max()) - 0.27) < 1e-6
    worst_it, worst_err = 0, 0.0
    for _ in range(15):
        s.advance(20)
        worst_it, worst_err = max(worst_it, s.iterations), max(worst_err, s.density_error)
        assert s.iterations < 50, s.iterations   # so err <= max_error by construction
    x = e.download(L.F_POSITION)
    pad, hi = np.float32(c.padding), (np.asarray(c.domain_size) - c.padding).astype(np.float32)
    print(f"holds together: top {float(x[:, 1].max()):.4f} from {float(x0[:, 1].max()):.4f}, most iterations {worst_it}, largest error {worst_err:.3e}")
    assert e.stats()["steps"] == 300
    assert np.isfinite(x).all() and np.isfinite(e.download(L.F_VELOCITY)).all()
    assert (x >= pad).all() and (x <= hi).all()
    assert worst_err <= 1e-3
    assert float(x[:, 1].max()) < float(x0[:, 1].max()) - 0.02
    e.close()


def test_refusals(gpu):
    c, s = _box()
    e = c.engine
    with pytest.raises(L.SphError) as ei:
        e.set_pbf_variant("consistent")
    assert ei.value.code == L.ERR_INVALID and "sph_prepare" in str(ei.value)
    with pytest.raises(L.SphError) as ei:
        e.set_rigid_contact(True, 0.02)
    assert ei.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.SphError) as ei:
        e.download(L.F_PBF_OLD_POSITION)
    assert ei.value.code == L.ERR_UNSUPPORTED
    e.close()
    c, s = H.build_product(P.dam_break_scene(method="dfsph", end=(0.2, 0.2, 0.2)))
    with pytest.raises(L.SphError) as ei:
        c.engine.set_pbf_variant("consistent")
    assert ei.value.code == L.ERR_UNSUPPORTED
    c.engine.close()
    c, s = H.build_product(P.pbf_scene(domain_end=(0.5, 0.5, 0.5), end=(0.2, 0.2, 0.2)))
    for field, kw in [("variant", dict(variant=2)), ("min_iterations", dict(min_iterations=0)), ("max_iterations", dict(min_iterations=3, max_iterations=2)),
                      ("max_error", dict(max_error=0.0)), ("max_error", dict(max_error=float("nan"))), ("epsilon", dict(epsilon=-1.0))]:
        with pytest.raises(L.SphError) as ei:
            c.engine.set_pbf_variant(**kw)
        assert ei.value.code == L.ERR_INVALID and field in str(ei.value), (field, str(ei.value))
    c.engine.close()
    cfg = M.box_scene()
    cfg["Configuration"]["viscosityMethod"] = "implicit"
    c, s = H.build_product(cfg)
    with pytest.raises(L.SphError) as ei:
        s.prepare()
    assert "implicit viscosity" in str(ei.value)
    c.engine.close()


def test_reference_variant_is_untouched(gpu):
    """No setter = variant 0 set explicitly, byte for byte over 5 steps; pbf_recentred counts as before there and stays 0 here."""
    runs = []
    for explicit in (False, True):
        c, s = H.build_product(P.pbf_scene(domain_end=(0.5, 0.5, 0.5), end=(0.25, 0.3, 0.25)))
        if explicit:
            c.engine.set_pbf_variant("reference", min_iterations=7, max_iterations=9, max_error=0.5, epsilon=3.0)   # (ignored)
        s.prepare()
        assert s.variant == "reference"
        c.engine.step(5)
        st = c.engine.stats()
        assert c.engine.pbf_stats() == dict(variant=0, iterations=5, error=0.0)
        runs.append([c.engine.download(f) for f in FIELDS + (L.F_PBF_OLD_POSITION,)] + [st["pbf_recentred"], st["pair_interactions"]])
        c.engine.close()
    assert runs[0][-2] > 0   # the block scatters: walks are recentred
    for a, b in zip(*runs):
        assert (a.tobytes() == b.tobytes()) if isinstance(a, np.ndarray) else a == b
    c, s = _box()
    c.engine.step(5)
    assert c.engine.stats()["pbf_recentred"] == 0
    c.engine.close()


def _drive(tmp_path, name, cfg):
    scene_file = tmp_path / f"{name}.json"
    scene_file.write_text(json.dumps(cfg))
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sph_project_amd", "run_simulation.py"), "--scene_file", str(scene_file),
                        "--output_dir", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Simulation method: pbf" in r.stdout
    return {f"{d.name}/{f.name}": f.read_bytes() for d in sorted(out.iterdir()) for f in sorted(d.iterdir())}


def test_driver(gpu, tmp_path):
    """A scene file with the key writes PLY frames with finite coordinates; without it the frames are those of an explicit "reference"."""
    base = P.pbf_scene(domain_end=(0.5, 0.5, 0.5), start=(0.1, 0.1, 0.1), end=(0.2, 0.2, 0.2), add_domain_box=False, dt=8e-4)
    base["Configuration"].update(exportPly=True, outputInterval=5, totalTime=0.0124)   # 15 steps, a frame every 5
    cons = json.loads(json.dumps(base))
    cons["Configuration"]["pbfVariant"] = "consistent"
    frames = _drive(tmp_path, "consistent", cons)
    assert sorted(frames) == [f"{k:06}/particle_object_0.ply" for k in range(0, 15, 5)]
    for name, data in frames.items():
        lines = data.decode().splitlines()
        assert lines[0] == "ply" and "element vertex 125" in lines
        xyz = np.array([[float(t) for t in ln.split()] for ln in lines[lines.index("end_header") + 1:]])
        assert xyz.shape == (125, 3) and np.isfinite(xyz).all()
    ref = json.loads(json.dumps(base))
    ref["Configuration"]["pbfVariant"] = "reference"
    plain, explicit = _drive(tmp_path, "plain", base), _drive(tmp_path, "explicit", ref)
    assert plain == explicit and sorted(plain) == sorted(frames)
    assert plain["000010/particle_object_0.ply"] != frames["000010/particle_object_0.ply"]
