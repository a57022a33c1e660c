"""GPU: the Akinci surface tension (sph_set_surface_tension) against the float64 model of
tests/surface_tension_terms.py -- pass by pass through the C-ABI, then the methods it reaches through the shared non-pressure pass,
the mode switched off (the old code, bit for bit), determinism, a cube that becomes a drop, adhesion, and the refusals."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from tests import helpers as H
from tests import nonpressure_terms as T
from tests import surface_tension_terms as A

pytestmark = pytest.mark.gpu
U = A.U
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_FIELDS = dict(x=L.F_POSITION, v=L.F_VELOCITY, rho=L.F_DENSITY, vol=L.F_REST_VOLUME, mass=L.F_MASS, mat=L.F_MATERIAL, obj=L.F_OBJECT_ID,
               dyn=L.F_IS_DYNAMIC)
_SCENES = {}


def _scene(method, kind, implicit=False, layers=None):
    """layers: the scene's twin in a domain of that many cell layers in z (tests/helpers.py with_layers)"""
    key = (method, kind, implicit, layers)
    if key not in _SCENES:
        _SCENES[key] = A.scene(method, kind, viscosity_method="implicit" if implicit else "standard", layers=layers)
    return _SCENES[key]


def _engine(sc, method, fast_math, gamma=None, beta=0.0, fixed_iterations=0):
    pd = sc["pd"]
    p = L.SphParams()
    for k in ("particle_radius", "support_radius", "V0", "padding", "g_upper", "viscosity", "viscosity_b", "density_0",
              "surface_tension", "dt", "particle_max_num", "viscosity_implicit"):
        setattr(p, k, pd[k])
    p.domain_size[:] = pd["domain_size"]; p.grid_num[:] = pd["grid_num"]; p.gravity[:] = pd["gravity"]
    p.method = L.METHOD[method]; p.device = -1; p.deterministic = 1; p.fast_math = fast_math; p.fixed_iterations = fixed_iterations
    eng = L.Engine(p)
    T.feed(eng, sc, oracle=False)
    if gamma is not None:
        eng.set_surface_tension("akinci", gamma, beta)
    eng.prepare()
    eng.get_rigid_wrench(reset=True)
    return eng


def _state(eng, extra=()):
    ids = eng.download(L.F_PARTICLE_ID)
    st = {k: H.by_id(ids, eng.download(f)) for k, f in _FIELDS.items()}
    for k, f in extra:
        st[k] = H.by_id(ids, eng.download(f))
    return st


def _visc_density(eng, st, method, rho0):
    """The density the viscous term (and the surface tension) of the method reads, as the device holds it: WCSPH keeps the raw density
    of the last density pass in the buffer SPH_F_DEBUG_CAPTURE hands out; the clamped one is its maximum with rho0, bit for bit."""
    if method != "wcsph":
        return st["rho"]
    raw = H.by_id(eng.download(L.F_PARTICLE_ID), eng.download(L.F_DEBUG_CAPTURE))
    fl = st["mat"] == 1
    np.testing.assert_array_equal(np.maximum(raw, np.float32(rho0))[fl], st["rho"][fl])
    return raw


def _tiny_wrench(n):
    return 2 * (n // 256 + 1) * 2.0 ** -33


def _check_passes(eng, sc, method, gamma, beta, tag, fast_math, implicit=False):
    """The phases up to the normals, then the non-pressure pass, each against the model fed with the device's own inputs."""
    Pm = sc["params"]
    for ph in (L.PH_NEIGHBOR_SEARCH, L.PH_RIGID_VOLUME, L.PH_DENSITY, L.PH_SURFACE_NORMALS):
        eng.run_phase(ph)
    st0 = _state(eng, extra=[("n", L.F_SURFACE_NORMAL)])
    fl = st0["mat"] == 1
    rho = np.where(fl, _visc_density(eng, st0, method, Pm["rho0"]), 1.0)
    fr = {}
    n64, nb, nterms = A.normals_f64(st0["x"], rho, st0["mass"], st0["mat"], Pm["h"])
    assert nterms.max() <= A.N_MAX
    err = np.abs(st0["n"].astype(np.float64) - n64)[fl]
    fr["normals"] = float((err / nb[fl]).max())
    assert np.isfinite(st0["n"][fl]).all() and (err <= nb[fl]).all(), fr
    eng.get_rigid_wrench(reset=True)
    if implicit:   # the solve in pieces (SPH_PH_NON_PRESSURE with fixed_iterations = k, bit for bit): the solved velocities are cg_x in
        eng.run_phase(L.PH_CG_PREPARE)   # front of SPH_PH_CG_END, which reads them and then stores the next step's guess there
        for _ in range(implicit):
            for ph in (L.PH_CG_AP, L.PH_CG_UPDATE_XR, L.PH_CG_UPDATE_P):
                eng.run_phase(ph)
        solved = H.by_id(eng.download(L.F_PARTICLE_ID), eng.download(L.F_CG_X))
        eng.run_phase(L.PH_CG_END)
    else:
        eng.run_phase(L.PH_NON_PRESSURE)
    st1 = _state(eng, extra=[("a_np", L.F_NON_PRESSURE_ACCEL)])
    f, t = eng.get_rigid_wrench(reset=False)
    visc_v = np.where(fl[:, None], solved, st0["v"]) if implicit else None
    rv = T.non_pressure_f64(st0["x"], st0["v"], rho, st0["mass"], st0["vol"], st0["mat"], st0["dyn"], st0["obj"], sc["com"], Pm, visc_v=visc_v)
    rs = A.surface_tension_f64(st0["x"], rho, st0["mass"], st0["vol"], st0["mat"], st0["dyn"], st0["obj"], sc["com"], st0["n"], Pm, gamma, beta)
    A.assert_alive(rs, n64, fl, sc["rigid"], beta)
    a = rv["a"] + rs["a"]
    bound = T.accel_bound(rv) + rs["bound"]
    assert np.isfinite(st1["a_np"][fl]).all() and np.isfinite(st1["v"]).all()
    err = np.abs(st1["a_np"].astype(np.float64) - a)[fl]
    fr["acceleration"] = float((err / bound[fl]).max())
    assert (err <= bound[fl]).all(), fr
    vs = st0["v"].astype(np.float64) + Pm["dt"] * a
    err = np.abs(st1["v"].astype(np.float64) - vs)[fl]
    vb = (Pm["dt"] * bound + 2 * U * np.abs(vs))[fl]
    fr["v*"] = float((err / vb).max())
    assert (err <= vb).all(), fr
    np.testing.assert_array_equal(st1["v"][~fl], st0["v"][~fl])
    if sc["rigid"]:
        w = T.add_wrenches(rv["wrench"], rs["wrench"])
        for part, got in (("force", f), ("torque", t)):
            got = got[:A.BODY + 1].astype(np.float64)
            err = np.abs(got - w[part])[A.BODY]
            wb = T.wrench_bound(w, part)[A.BODY] + _tiny_wrench(len(fl)) + U * np.abs(w[part][A.BODY])
            fr["wrench " + part] = float((err / wb).max())
            assert np.isfinite(got).all() and (err <= wb).all(), (fr, got[A.BODY], w[part][A.BODY])
            assert (got[A.PLATE] == 0).all()   # a static body takes no reaction
    print("surface tension [%s, fast_math=%d, beta=%g]: " % (tag, fast_math, beta) + ", ".join("%s %.3f" % kv for kv in fr.items()))


# (without a boundary beta changes nothing: the all-fluid twins run with beta = 0 only)
_KINDS = [("rigid", 0.0), ("rigid", 1.0), ("fluid", 0.0), ("lattice", 0.0), ("lattice", 1.0), ("lattice_fluid", 0.0)]


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("kind, beta", _KINDS)
@pytest.mark.parametrize("method", ["wcsph", "dfsph"])
def test_pass_by_pass(gpu, method, kind, beta, fast_math):
    """SPH_PH_SURFACE_NORMALS, then SPH_PH_NON_PRESSURE on the stored normals: SurfaceNormalPass / AkinciNonPressurePass<false> (the
    scenes with the plate and the dynamic cube) and <true> (their all-fluid twins), jittered and on the exact rest lattice."""
    sc = _scene(method, kind)
    eng = _engine(sc, method, fast_math, gamma=1.0, beta=beta)
    try:
        _check_passes(eng, sc, method, 1.0, beta, "%s, %s" % (method, kind), fast_math)
    finally:
        eng.close()


@pytest.mark.parametrize("fast_math", [0, 1])
def test_pass_by_pass_under_implicit_viscosity(gpu, fast_math):
    """visc_vel: the pass at the end of the CG solve (SPH_PH_CG_END, on the stored normals) evaluates the viscous formula with the
    solved velocities and advances the original ones."""
    sc = _scene("dfsph", "rigid", implicit=True)
    eng = _engine(sc, "dfsph", fast_math, gamma=1.0, beta=1.0, fixed_iterations=4)
    try:
        _check_passes(eng, sc, "dfsph", 1.0, 1.0, "dfsph implicit, rigid", fast_math, implicit=4)
    finally:
        eng.close()


@pytest.mark.parametrize("method", ["pcisph", "iisph"])
def test_whole_step_reaches_the_method(gpu, method):
    """One whole step: the non-pressure acceleration it leaves is the model's at the state before the step, fed with the normals and
    densities the same phases produce from that state (a step recomputes both from the same positions: bit-identical).  Both
    methods sort at the start of a step, so the two buffers are still in the order of the ids behind it."""
    sc = _scene(method, "rigid")
    Pm = sc["params"]
    eng = _engine(sc, method, 0, gamma=1.0, beta=1.0)
    try:
        for ph in (L.PH_NEIGHBOR_SEARCH, L.PH_RIGID_VOLUME, L.PH_DENSITY, L.PH_SURFACE_NORMALS):
            eng.run_phase(ph)
        st0 = _state(eng, extra=[("n", L.F_SURFACE_NORMAL)])
        fl = st0["mat"] == 1
        rho = np.where(fl, st0["rho"], 1.0)
        eng.step(1)
        st1 = _state(eng, extra=[("a_np", L.F_NON_PRESSURE_ACCEL), ("n", L.F_SURFACE_NORMAL)])
    finally:
        eng.close()
    np.testing.assert_array_equal(st1["n"][fl], st0["n"][fl])
    rv = T.non_pressure_f64(st0["x"], st0["v"], rho, st0["mass"], st0["vol"], st0["mat"], st0["dyn"], st0["obj"], sc["com"], Pm)
    rs = A.surface_tension_f64(st0["x"], rho, st0["mass"], st0["vol"], st0["mat"], st0["dyn"], st0["obj"], sc["com"], st0["n"], Pm, 1.0, 1.0)
    err = np.abs(st1["a_np"].astype(np.float64) - (rv["a"] + rs["a"]))[fl]
    bound = (T.accel_bound(rv) + rs["bound"])[fl]
    print("whole step [%s]: acceleration %.3f of its bound" % (method, (err / bound).max()))
    assert np.isfinite(st1["x"]).all() and np.isfinite(st1["v"]).all() and (err <= bound).all()
    assert np.abs(st1["x"] - st0["x"])[fl].max() > 0


@pytest.mark.parametrize("method", ["wcsph", "dfsph"])
def test_whole_step_under_implicit_viscosity_is_its_phases(gpu, method):
    """Implicit viscosity: the step against its phase sequence, bit for bit -- WCSPH a whole step (sort, density, normals, the solve
    and its end, pressure + integration), DFSPH the first half of one (normals, the solve and its end, the density solve: the
    velocities; the position update has no phase of its own)."""
    sc = _scene(method, "rigid", implicit=True)
    outs = []
    for how in ("step", "phases"):
        eng = _engine(sc, method, 0, gamma=1.0, beta=1.0)
        if how == "step":
            eng.step(1) if method == "wcsph" else eng.step_begin()
        elif method == "wcsph":
            for ph in (L.PH_NEIGHBOR_SEARCH, L.PH_RIGID_VOLUME, L.PH_DENSITY, L.PH_SURFACE_NORMALS, L.PH_NON_PRESSURE, L.PH_PRESSURE_INTEGRATE):
                eng.run_phase(ph)
        else:
            for ph in (L.PH_SURFACE_NORMALS, L.PH_NON_PRESSURE, L.PH_DFSPH_DENSITY):
                eng.run_phase(ph)
        outs.append(_state(eng))
        if how == "step" and method == "dfsph":
            eng.step_end()
            assert np.isfinite(eng.download(L.F_POSITION)).all()
        eng.close()
    fl = outs[0]["mat"] == 1
    for k in ("v",) + (("x", "rho") if method == "wcsph" else ()):
        np.testing.assert_array_equal(_bits(outs[1][k][fl]), _bits(outs[0][k][fl]), err_msg=k)
    assert np.isfinite(outs[0]["v"]).all()


def _profile(eng):
    return {k: eng.profile_read(k)[0] for k in (3, 4, 5, 18, L.K_SURFACE_NORMALS)}


@pytest.mark.parametrize("fast_math", [0, 1])
def test_mode_off_is_the_old_code(gpu, fast_math):
    """Never touched, set to "reference", set to "akinci" and back: 20 WCSPH steps, bit-identical; the fused force pass (kernel id 18)
    ran and the unfused non-pressure pass (4) did not.  With the mode on: 4, 5 and the normal pass run, 18 does not."""
    sc = _scene("wcsph", "rigid")
    outs, profs = [], []
    for how in ("untouched", "reference", "back", "on"):
        eng = _engine(sc, "wcsph", fast_math)
        if how == "reference":
            eng.set_surface_tension("reference")
        elif how == "back":
            eng.set_surface_tension("akinci", 1.0, 0.5)
            assert eng.get_surface_tension() == dict(method="akinci", gamma=1.0, beta=0.5)
            eng.set_surface_tension("reference", 1.0, 0.5)
        elif how == "on":
            eng.set_surface_tension("akinci", 1.0, 0.5)
        eng.profile_enable(-1, True)
        eng.step(20)
        profs.append(_profile(eng))
        outs.append(_state(eng))
        eng.close()
    for o in outs[1:3]:
        for k in ("x", "v", "rho"):
            np.testing.assert_array_equal(o[k], outs[0][k])
    for pr in profs[:3]:
        assert pr[18] == 20 and pr[4] == 0 and pr[5] == 0 and pr[L.K_SURFACE_NORMALS] == 0, pr
    assert profs[3][18] == 0 and profs[3][4] == 20 and profs[3][5] == 20 and profs[3][L.K_SURFACE_NORMALS] == 20, profs[3]
    assert np.abs(outs[3]["x"] - outs[0]["x"]).max() > 1e-6 and np.isfinite(outs[3]["x"]).all()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("fast_math", [0, 1])
def test_determinism_and_async_steps(gpu, fast_math):
    """Mode on: one sph_step(h, 25) is 25 calls bit for bit, two runs give the same wrench bits, sph_step_async works (no read-back)."""
    sc = _scene("wcsph", "rigid")
    outs = []
    for how in ("once", "one_by_one", "async"):
        eng = _engine(sc, "wcsph", fast_math, gamma=1.0, beta=1.0)
        if how == "once":
            eng.step(25)
        elif how == "one_by_one":
            for _ in range(25):
                eng.step(1)
        else:
            eng.step_async(25)
            eng.synchronize()
        st = _state(eng)
        st["f"], st["t"] = eng.get_rigid_wrench(reset=False)
        outs.append(st)
        eng.close()
    assert np.abs(outs[0]["f"][A.BODY]).max() > 0
    for o in outs[1:]:
        for k in ("x", "v", "rho", "f", "t"):
            np.testing.assert_array_equal(_bits(o[k]), _bits(outs[0][k]), err_msg=k)


def shape_number(x):
    """(max distance from the centre of mass) / (rms distance): 1.73 for a cube, 1.29 for a ball."""
    d = np.linalg.norm(x - x.mean(axis=0), axis=1)
    return float(d.max() / np.sqrt((d * d).mean()))


def run_droplet(fast_math, max_steps=2000, chunk=25, gamma=1.0):
    """droplet_scene(10) until its shape number first falls below 1.5: (steps or None, trajectory [(step, s)], relative momentum,
    positions, domain)."""
    cfg = P.droplet_scene(10, gamma=gamma)
    container, solver = P.build_product(cfg, fast_math=fast_math)
    solver.prepare()
    eng = container.engine
    traj, hit = [(0, shape_number(eng.download(L.F_POSITION)))], None
    for k in range(chunk, max_steps + 1, chunk):
        solver.advance(chunk)
        x = eng.download(L.F_POSITION)
        traj.append((k, shape_number(x)))
        if not np.isfinite(x).all() or traj[-1][1] < 1.5:
            hit = k if np.isfinite(x).all() else None
            break
    x, v, m = eng.download(L.F_POSITION), eng.download(L.F_VELOCITY).astype(np.float64), eng.download(L.F_MASS).astype(np.float64)
    mom = float(np.linalg.norm((m[:, None] * v).sum(axis=0)) / (m * np.linalg.norm(v, axis=1)).sum())
    eng.close()
    return hit, traj, mom, x, np.asarray(cfg["Configuration"]["domainEnd"])


# |sum m v| / sum m |v| when the shape number first falls below 1.5, measured in the strict build (profiles/surface_tension_droplet.txt)
DROPLET_MOMENTUM_STRICT = 3.4e-5
DROPLET_MOMENTUM_BOUND = min(10 * DROPLET_MOMENTUM_STRICT, 1e-3)


@pytest.mark.parametrize("fast_math", [0, 1])
def test_a_cube_becomes_a_drop(gpu, fast_math):
    """droplet_scene(10): zero gravity, WCSPH, 1000 particles, gamma = 1.  s = max / rms distance from the centre of mass falls from the
    cube's 1.57 (1.73 in the continuum) below 1.5 (the midpoint between 1.73 and a ball's 1.29) within 2000 steps -- measured: after
    100 steps, s = 1.432, in both builds; everything stays finite and inside the box; the momentum
    a one-mass fluid conserves stays below ten times the strict build's measured value (a missing or one-sided term gives O(1))."""
    hit, traj, mom, x, dom = run_droplet(fast_math)
    print("droplet fast_math=%d: s %.3f -> %.3f, below 1.5 after %s steps, relative momentum %.3e (bound %.1e)"
          % (fast_math, traj[0][1], traj[-1][1], hit, mom, DROPLET_MOMENTUM_BOUND))
    assert abs(traj[0][1] - 1.5667) < 1e-3   # (10^3 lattice points: sqrt(3) 4.5 / sqrt(24.75); the continuum cube's is 1.73)
    assert np.isfinite(x).all() and (x > 0).all() and (x < dom).all()
    assert hit is not None and hit <= 2000, traj[-5:]
    assert mom <= DROPLET_MOMENTUM_BOUND, mom


def _com_drop(beta, cube=False):
    cfg = P.droplet_scene(6, beta=beta, plate_gap=1.0, cube_gap=1.0 if cube else None)
    container, solver = P.build_product(cfg, fast_math=0)
    solver.prepare()
    eng = container.engine
    fl = eng.download(L.F_MATERIAL) == 1
    y0 = eng.download(L.F_POSITION)[fl].astype(np.float64).mean(axis=0)
    out = {}
    if cube:   # the pass alone: the wrench of the dynamic cube beside the +x face, and the fluid's mean acceleration
        for ph in (L.PH_NEIGHBOR_SEARCH, L.PH_RIGID_VOLUME, L.PH_DENSITY, L.PH_SURFACE_NORMALS):
            eng.run_phase(ph)
        eng.get_rigid_wrench(reset=True)
        eng.run_phase(L.PH_NON_PRESSURE)
        out["force"] = eng.get_rigid_wrench(reset=True)[0][2].astype(np.float64)
        out["a"] = eng.download(L.F_NON_PRESSURE_ACCEL)[eng.download(L.F_MATERIAL) == 1].astype(np.float64).mean(axis=0)
    else:
        solver.advance(200)
        x = eng.download(L.F_POSITION)
        assert np.isfinite(x).all()
        out["shift"] = x[eng.download(L.F_MATERIAL) == 1].astype(np.float64).mean(axis=0) - y0
    eng.close()
    return out


def test_adhesion_pulls(gpu):
    """A 6^3 droplet at zero gravity one diameter above a static plate, 200 steps: with beta = 1 its centre of mass moves towards the
    plate, and by more than with beta = 0.  With a dynamic cube beside it the cube is pulled towards the fluid (-x) while the
    adhesion part of the fluid's acceleration points at the cube (+x)."""
    on, off = _com_drop(1.0)["shift"], _com_drop(0.0)["shift"]
    print("adhesion: centre of mass moved by %.3e (beta = 1) / %.3e (beta = 0) in y" % (on[1], off[1]))
    assert on[1] < 0 and on[1] < off[1] - 1e-5
    w1, w0 = _com_drop(1.0, cube=True), _com_drop(0.0, cube=True)
    print("adhesion: force on the cube %s, mean fluid acceleration beta = 1 less beta = 0 %s" % (w1["force"], w1["a"] - w0["a"]))
    assert (w0["force"] == 0).all()          # at rest the viscous reaction vanishes: the wrench is adhesion's alone
    assert w1["force"][0] < -1e-6 and (w1["a"] - w0["a"])[0] > 0


def _params(method):
    sc = _scene("wcsph", "fluid")
    pd = sc["pd"]
    p = L.SphParams()
    for k in ("particle_radius", "support_radius", "V0", "padding", "g_upper", "viscosity", "viscosity_b", "density_0",
              "surface_tension", "dt", "particle_max_num", "viscosity_implicit"):
        setattr(p, k, pd[k])
    p.domain_size[:] = pd["domain_size"]; p.grid_num[:] = pd["grid_num"]; p.gravity[:] = pd["gravity"]
    p.method = L.METHOD[method]; p.device = -1; p.deterministic = 1
    return p


def _rc(call):
    try:
        call()
    except L.SphError as e:
        return e.code
    return 0


def test_refusals(gpu, monkeypatch, tmp_path):
    eng = L.Engine(_params("pbf"))
    assert _rc(lambda: eng.set_surface_tension("akinci")) == L.ERR_UNSUPPORTED
    eng.set_pbf_variant("consistent")
    assert _rc(lambda: eng.set_surface_tension("akinci")) == L.ERR_UNSUPPORTED
    eng.close()
    eng = L.Engine(_params("wcsph"))
    for bad in (dict(gamma=-1.0), dict(beta=-1.0), dict(gamma=float("nan")), dict(beta=float("inf")), dict(method=2)):
        assert _rc(lambda: eng.set_surface_tension(**bad)) == L.ERR_INVALID, bad
    assert eng.get_surface_tension()["method"] == "reference"
    assert _rc(lambda: eng.run_phase(L.PH_SURFACE_NORMALS)) == L.ERR_INVALID
    assert _rc(lambda: eng.download(L.F_SURFACE_NORMAL)) == L.ERR_UNSUPPORTED
    eng.close()
    # sharded handles: two ranks on one GPU over the shared-memory transport, one thread each
    monkeypatch.setenv("SPH_COMM_TRANSPORT", "shm")
    monkeypatch.setenv("SPH_COMM_TIMEOUT_S", "20")
    engs = [L.Engine(_params("wcsph")) for _ in range(2)]
    uid = engs[0].comm_unique_id()
    nz = int(_params("wcsph").grid_num[2])
    got = [None, None]

    def rank(k):
        engs[k].comm_init(k, 2, uid)
        if k == 1:   # the other order: the mode first, then the slab
            engs[k].set_surface_tension("akinci")
            got[k] = _rc(lambda: engs[k].comm_set_slab(nz // 2, nz))
            engs[k].set_surface_tension("reference")
        engs[k].comm_set_slab(*((0, nz // 2) if k == 0 else (nz // 2, nz)))
        if k == 0:
            got[k] = _rc(lambda: engs[k].set_surface_tension("akinci"))

    threads = [threading.Thread(target=rank, args=(k,), daemon=True) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads)
    assert got == [L.ERR_UNSUPPORTED, L.ERR_UNSUPPORTED], got
    for e in engs:
        e.close()
    # the driver: --gpus 2 on an Akinci scene ends in the parent with code 2, before a rank starts
    path = tmp_path / "drop.json"
    path.write_text(json.dumps(P.droplet_scene(4)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sph_project_amd", "run_simulation.py"), "--scene_file", str(path), "--gpus", "2"],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "akinci" in r.stderr, (r.returncode, r.stderr[-400:])
