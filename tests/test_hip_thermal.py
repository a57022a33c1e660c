"""GPU: heat (sph_set_thermal) against the float64 model of tests/thermal_terms.py -- the walk through the C-ABI, the
buoyancy behind the non-pressure phase of every method, the carry of the temperatures through the sort, new particles, the mode
switched off (the old code, bit for bit), determinism, a heated plate, the neighbouring features, and the refusals."""
import copy
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd import scene as S
from tests import helpers as H
from tests import nonpressure_terms as T
from tests import drag_terms as D
from tests import outflow_model as OM
from tests import thermal_terms as M

pytestmark = pytest.mark.gpu
U = M.U
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA = 2.0e-3

_FIELDS = dict(x=L.F_POSITION, v=L.F_VELOCITY, rho=L.F_DENSITY, vol=L.F_REST_VOLUME, mass=L.F_MASS, mat=L.F_MATERIAL, obj=L.F_OBJECT_ID,
               dyn=L.F_IS_DYNAMIC)
_HEAT = [("T", L.F_TEMPERATURE)]
_SCENES = {}
_SORTED = (L.PH_NEIGHBOR_SEARCH, L.PH_RIGID_VOLUME, L.PH_DENSITY)


def _alpha(Pm):
    """Half the diffusivity at which the scene's step IS the step limit (tests/test_thermal_host.py)."""
    return 0.5 * 0.5 / (2.0 * 1.25 * M.lattice_sum(Pm["h"], Pm["diameter"]) * Pm["dt"])


def _scene(method, kind, implicit=False):
    key = (method, kind, implicit)
    if key not in _SCENES:
        sc = M.scene(method, kind, viscosity_method="implicit" if implicit else "standard")
        sc["T"] = M.temperatures(sc)
        _SCENES[key] = sc
    return _SCENES[key]


def _params(sc, method, fast_math=0, fixed_iterations=0, spare=0, force_global=0):
    pd = sc["pd"]
    p = L.SphParams()
    for k in ("particle_radius", "support_radius", "V0", "padding", "g_upper", "viscosity", "viscosity_b", "density_0",
              "surface_tension", "dt", "particle_max_num", "viscosity_implicit"):
        setattr(p, k, pd[k])
    p.particle_max_num = pd["particle_max_num"] + spare
    p.domain_size[:] = pd["domain_size"]; p.grid_num[:] = pd["grid_num"]; p.gravity[:] = pd["gravity"]
    p.method = L.METHOD[method]; p.device = -1; p.deterministic = 1; p.fast_math = fast_math; p.fixed_iterations = fixed_iterations
    p.force_global = force_global
    return p


def _upload_by_id(eng, field, by_id):
    eng.upload(field, np.ascontiguousarray(by_id[eng.download(L.F_PARTICLE_ID)]))


def _engine(sc, method, fast_math, heat="scene", temp=True, fixed_iterations=0, spare=0, vel=None, force_global=0, others=False):
    """heat: (alpha, beta) or "scene" (the scene's alpha, BETA) or None (mode never touched); temp: upload the scene's temperatures
    (True) or given ones; the plate is held at T_WALL, the cube stays adiabatic; others: Akinci, micropolar and drag on as well."""
    eng = L.Engine(_params(sc, method, fast_math, fixed_iterations, spare, force_global))
    T.feed(eng, sc, oracle=False)
    if others:
        eng.set_surface_tension("akinci", 1.0, 1.0)
        eng.set_micropolar("micropolar", 0.3, 0.5, 2.0)
        eng.set_drag("gissler", 5.0, 1.2041, (3.0, -1.0, 0.5))
    if heat is not None:
        alpha, beta = (_alpha(sc["params"]), BETA) if heat == "scene" else heat
        eng.set_thermal("conduction", alpha, beta, M.T_REF)
        if sc["rigid"]:
            eng.set_object_temperature(M.PLATE, M.T_WALL)
        if temp is not False:
            _upload_by_id(eng, L.F_TEMPERATURE, sc["T"] if temp is True else temp)
    if vel is not None:
        _upload_by_id(eng, L.F_VELOCITY, vel)
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
    """The density the viscous term (and this model) of the method reads, as the device holds it (tests/test_hip_micropolar.py)."""
    if method != "wcsph":
        return st["rho"]
    raw = H.by_id(eng.download(L.F_PARTICLE_ID), eng.download(L.F_DEBUG_CAPTURE))
    fl = st["mat"] == 1
    np.testing.assert_array_equal(np.maximum(raw, np.float32(rho0))[fl], st["rho"][fl])
    return raw


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_walk(eng, sc, method, alpha=None, beta=BETA):
    """The phases up to SPH_PH_HEAT: the new T and dT/dt against the model fed with the device's own inputs."""
    Pm = sc["params"]
    alpha = _alpha(Pm) if alpha is None else alpha
    for ph in _SORTED:
        eng.run_phase(ph)
    st0 = _state(eng, extra=_HEAT)
    fl = st0["mat"] == 1
    np.testing.assert_array_equal(_bits(st0["T"][fl]), _bits(sc["T"][fl]))   # what was uploaded, through prepare() and the sort
    if sc["rigid"]:   # a row that is not fluid reads what its object is held at, or the reference temperature
        assert (st0["T"][st0["obj"] == M.PLATE] == np.float32(M.T_WALL)).all() and (st0["T"][st0["obj"] == M.BODY] == np.float32(M.T_REF)).all()
    rho = np.where(fl, _visc_density(eng, st0, method, Pm["rho0"]), 1.0)
    wrench0 = eng.get_rigid_wrench(reset=False)
    eng.run_phase(L.PH_HEAT)
    st1 = _state(eng, extra=_HEAT + [("rate", L.F_TEMPERATURE_RATE)])
    wrench1 = eng.get_rigid_wrench(reset=False)
    res = M.thermal_f64(st0["x"], st0["T"], rho, st0["mass"], st0["vol"], st0["mat"], st0["obj"], M.WALLS if sc["rigid"] else {}, Pm,
                        alpha, beta, M.T_REF)
    M.assert_alive(res, st0["T"].astype(np.float64), fl, sc["rigid"])
    for k in ("x", "v", "rho"):
        np.testing.assert_array_equal(_bits(st1[k]), _bits(st0[k]), err_msg=k)   # the walk writes nothing else
    for a, b in zip(wrench0, wrench1):
        np.testing.assert_array_equal(a, b)                                       # heat never reaches a body
    np.testing.assert_array_equal(_bits(st1["T"][~fl]), _bits(st0["T"][~fl]))
    fr = {}
    assert np.isfinite(st1["rate"][fl]).all() and np.isfinite(st1["T"]).all()
    err = np.abs(st1["rate"].astype(np.float64) - res["rate"])[fl]
    fr["rate"] = float((err / res["rate_bound"][fl]).max())
    print("heat walk: dT/dt error / bound %.3f" % fr["rate"])
    assert (err <= res["rate_bound"][fl]).all(), fr
    err = np.abs(st1["T"].astype(np.float64) - res["T_new"])[fl]
    fr["T"] = float((err / res["T_bound"][fl]).max())
    print("heat walk: T error / bound %.3f" % fr["T"])
    assert (err <= res["T_bound"][fl]).all(), fr
    return st0, st1, fl, res, fr


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("method", ["wcsph", "dfsph"])
def test_pass_by_pass(gpu, method, kind, fast_math):
    """SPH_PH_HEAT, then SPH_F_TEMPERATURE / SPH_F_TEMPERATURE_RATE against the model: HeatPass<false> (the scenes with the heated
    plate and the adiabatic dynamic cube) and <true> (their all-fluid twins), jittered and on the exact rest lattice."""
    sc = _scene(method, kind)
    eng = _engine(sc, method, fast_math)
    try:
        _, _, _, _, fr = _check_walk(eng, sc, method)
        print("heat [%s, %s, fast_math=%d]: " % (method, kind, fast_math) + ", ".join("%s %.3f" % kv for kv in fr.items()))
    finally:
        eng.close()


def _cg(eng, k):
    eng.run_phase(L.PH_CG_PREPARE)
    for _ in range(k):
        for ph in (L.PH_CG_AP, L.PH_CG_UPDATE_XR, L.PH_CG_UPDATE_P):
            eng.run_phase(ph)
    eng.run_phase(L.PH_CG_END)


def _check_buoyancy_phase(sc, method, fast_math, tag, implicit=0, others=False):
    """Two handles that differ in beta alone, the same phases: behind SPH_PH_NON_PRESSURE (or SPH_PH_CG_END) the one with beta != 0 holds
    v_0 + dt a_b, where v_0 is the other's velocity and a_b the model's buoyancy of the temperatures the walk READ (not the ones it
    stored); one more f32 update: dt a_b_bound + 2 u (|v_0| + |v|).  The same for the kept non-pressure acceleration, where there is one."""
    Pm = sc["params"]
    alpha = _alpha(Pm)
    out = {}
    for how, beta in (("zero", 0.0), ("on", BETA)):
        eng = _engine(sc, method, fast_math, heat=(alpha, beta), fixed_iterations=implicit, others=others)
        try:
            for ph in _SORTED + ((L.PH_SURFACE_NORMALS, L.PH_MICROPOLAR, L.PH_DRAG) if others else ()) + (L.PH_HEAT,):
                eng.run_phase(ph)
            before = _state(eng, extra=_HEAT)
            if implicit:
                _cg(eng, implicit)
            else:
                eng.run_phase(L.PH_NON_PRESSURE)
            extra = _HEAT + ([("a_np", L.F_NON_PRESSURE_ACCEL)] if (others or method == "pcisph") else [])
            out[how] = (before, _state(eng, extra=extra))
        finally:
            eng.close()
    fl = out["on"][0]["mat"] == 1
    np.testing.assert_array_equal(_bits(out["on"][1]["T"]), _bits(out["on"][0]["T"]))   # no second walk
    np.testing.assert_array_equal(_bits(out["on"][0]["T"]), _bits(out["zero"][0]["T"]))
    a_b = M.thermal_f64(out["on"][0]["x"], sc["T"], np.ones(len(fl)), out["on"][0]["mass"], out["on"][0]["vol"], out["on"][0]["mat"],
                        out["on"][0]["obj"], {}, Pm, 0.0, BETA, M.T_REF)
    v0, v1 = out["zero"][1]["v"].astype(np.float64), out["on"][1]["v"].astype(np.float64)
    want = v0 + Pm["dt"] * a_b["a_b"]
    bound = Pm["dt"] * a_b["a_b_bound"] + 2 * U * (np.abs(v0) + np.abs(want))
    fr = {"v": float((np.abs(v1 - want)[fl, 1] / bound[fl, 1]).max())}
    assert np.isfinite(v1).all() and (np.abs(v1 - want)[fl] <= bound[fl]).all(), fr
    assert np.abs(Pm["dt"] * a_b["a_b"])[fl].max() > 100 * bound[fl].max()             # a_b is far above what the bound could hide
    np.testing.assert_array_equal(out["on"][1]["v"][~fl], out["zero"][1]["v"][~fl])
    if "a_np" in out["on"][1]:
        a0, a1 = out["zero"][1]["a_np"].astype(np.float64), out["on"][1]["a_np"].astype(np.float64)
        want = a0 + a_b["a_b"]
        bound = a_b["a_b_bound"] + 2 * U * (np.abs(a0) + np.abs(want))
        fr["a_np"] = float((np.abs(a1 - want)[fl, 1] / bound[fl, 1]).max())
        assert (np.abs(a1 - want)[fl] <= bound[fl]).all(), fr
    print("buoyancy [%s, fast_math=%d]: " % (tag, fast_math) + ", ".join("%s %.3f" % kv for kv in fr.items()))


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("method", ["wcsph", "dfsph", "pcisph", "iisph"])
def test_buoyancy_phase_under_every_method(gpu, method, fast_math):
    _check_buoyancy_phase(_scene(method, "rigid"), method, fast_math, method)


@pytest.mark.parametrize("fast_math", [0, 1])
def test_buoyancy_phase_under_implicit_viscosity(gpu, fast_math):
    """a_b goes in behind SPH_PH_CG_END, on top of the pass that advances the original velocities."""
    _check_buoyancy_phase(_scene("dfsph", "rigid", implicit=True), "dfsph", fast_math, "dfsph implicit", implicit=4)


@pytest.mark.parametrize("fast_math", [0, 1])
def test_beside_akinci_micropolar_and_drag(gpu, fast_math):
    """All four opt-in models at once: the walk is the model's (it reads none of the others' results), and a_b is added behind the
    air drag's, to the velocity and to the acceleration the Akinci pass keeps."""
    sc = _scene("wcsph", "rigid")
    eng = _engine(sc, "wcsph", fast_math, others=True)
    try:
        _check_walk(eng, sc, "wcsph")
    finally:
        eng.close()
    _check_buoyancy_phase(sc, "wcsph", fast_math, "wcsph + akinci + micropolar + drag", others=True)


@pytest.mark.parametrize("fast_math", [0, 1])
def test_group_overflow_fallback_gives_the_same_sums(gpu, fast_math):
    """force_global = 1 sends every candidate run through the tile in chunks, the path a group takes when it overflows its slots:
    within the model's bounds like the tiled walk, and in the strict build (one order of accumulation) the same bits."""
    sc = _scene("wcsph", "rigid")
    outs = []
    for fg in (0, 1):
        eng = _engine(sc, "wcsph", fast_math, force_global=fg)
        try:
            _, st1, fl, _, fr = _check_walk(eng, sc, "wcsph")
            outs.append((st1, eng.stats()["lds_fallback_blocks"]))
        finally:
            eng.close()
        print("heat [force_global=%d, fast_math=%d]: " % (fg, fast_math) + ", ".join("%s %.3f" % kv for kv in fr.items()))
    assert outs[0][1] < outs[1][1]
    if not fast_math:
        for k in ("T", "rate"):
            np.testing.assert_array_equal(_bits(outs[1][0][k][fl]), _bits(outs[0][0][k][fl]), err_msg=k)


_STEP_PHASES = {
    "wcsph": _SORTED + (L.PH_HEAT, L.PH_NON_PRESSURE, L.PH_PRESSURE_INTEGRATE),
    "pcisph": _SORTED + (L.PH_HEAT, L.PH_NON_PRESSURE, L.PH_PCISPH_INIT, L.PH_PCISPH_RHO_STAR, L.PH_PCISPH_PRESSURE_ACCEL, L.PH_PRESSURE_INTEGRATE),
    "iisph": _SORTED + (L.PH_HEAT, L.PH_NON_PRESSURE, L.PH_IISPH_PREPARE, L.PH_IISPH_ITERATION, L.PH_PRESSURE_INTEGRATE),
}


@pytest.mark.parametrize("case", ["wcsph", "pcisph", "iisph", "dfsph", "dfsph_implicit"])
def test_whole_steps_reach_the_method(gpu, case):
    """WCSPH, PCISPH, IISPH: after each of 5 steps the handle equals, bit for bit, a twin whose steps run as their phases one by one
    (one solver iteration).  DFSPH and DFSPH with implicit viscosity: the position update of a DFSPH step is no phase of its own, so
    the first half of EACH of the 5 steps -- everything heat touches -- is compared: sph_step_begin against SPH_PH_HEAT,
    SPH_PH_NON_PRESSURE (or the pieces of the CG solve), SPH_PH_DFSPH_DENSITY on a fresh twin that whole steps brought to the start of
    that step.  And the mode does reach the method: T changes, and v differs from a handle with beta = 0."""
    method = case.split("_")[0]
    implicit = 3 if case.endswith("implicit") else 0
    sc = _scene(method, "rigid", implicit=bool(implicit))
    fixed = implicit if implicit else (0 if method in ("wcsph", "dfsph") else 1)
    a = _engine(sc, method, 0, fixed_iterations=fixed)
    b = _engine(sc, method, 0, fixed_iterations=fixed)
    z = _engine(sc, method, 0, heat=(_alpha(sc["params"]), 0.0), fixed_iterations=fixed)
    try:
        keys = ("x", "v", "rho", "T")
        if method == "dfsph":
            for step in range(5):   # b: a fresh twin per step, brought to the start of that step by whole steps
                a.step_begin()
                z.step_begin()
                b.close()
                b = _engine(sc, method, 0, fixed_iterations=fixed)
                if step:
                    b.step(step)
                b.run_phase(L.PH_HEAT)
                if implicit:
                    _cg(b, implicit)
                else:
                    b.run_phase(L.PH_NON_PRESSURE)
                b.run_phase(L.PH_DFSPH_DENSITY)
                sa, sb, sz = _state(a, extra=_HEAT), _state(b, extra=_HEAT), _state(z, extra=_HEAT)
                for k in ("v", "T"):
                    np.testing.assert_array_equal(_bits(sa[k]), _bits(sb[k]), err_msg="%s in the first half of step %d" % (k, step + 1))
                a.step_end()
                z.step_end()
            assert np.isfinite(a.download(L.F_POSITION)).all() and np.isfinite(a.download(L.F_TEMPERATURE)).all()
        else:
            for step in range(5):
                a.step(1)
                z.step(1)
                for ph in _STEP_PHASES[method]:
                    b.run_phase(ph)
                sa, sb = _state(a, extra=_HEAT), _state(b, extra=_HEAT)
                for k in keys:
                    np.testing.assert_array_equal(_bits(sa[k]), _bits(sb[k]), err_msg="%s after step %d" % (k, step + 1))
            sz = _state(z, extra=_HEAT)
        fl = sa["mat"] == 1
        assert np.isfinite(sa["T"]).all() and np.abs(sa["T"] - sc["T"])[fl].max() > 1.0
        assert np.abs(sa["v"] - sz["v"])[fl].max() > 1e-6
    finally:
        for e in (a, b, z):
            e.close()


@pytest.mark.parametrize("fast_math", [0, 1])
def test_fused_route_walks_between_density_and_forces(gpu, fast_math):
    """WCSPH, alpha > 0, beta = 0: the step keeps its fused force pass (kernel id 18 timed, 4 and 5 not) and the walk runs between the
    density pass and it.  After each of 3 steps T equals, bit for bit, a twin that ran the sort, the density pass and SPH_PH_HEAT as
    phases from the same state (a fresh twin per step, brought there by whole steps) -- the sequence _check_walk holds to the model --
    and x, v, rho are those of a handle without the mode."""
    sc = _scene("wcsph", "rigid")
    heat = (_alpha(sc["params"]), 0.0)
    a, off = _engine(sc, "wcsph", fast_math, heat=heat), _engine(sc, "wcsph", fast_math, heat=None)
    try:
        a.profile_enable(-1, True)
        for step in range(3):
            b = _engine(sc, "wcsph", fast_math, heat=heat)
            try:
                if step:
                    b.step(step)
                for ph in _SORTED + (L.PH_HEAT,):
                    b.run_phase(ph)
                tb = _state(b, extra=_HEAT)["T"]
            finally:
                b.close()
            a.step(1)
            off.step(1)
            sa, so = _state(a, extra=_HEAT), _state(off)
            np.testing.assert_array_equal(_bits(sa["T"]), _bits(tb), err_msg="T after step %d" % (step + 1))
            for k in ("x", "v", "rho"):
                np.testing.assert_array_equal(_bits(sa[k]), _bits(so[k]), err_msg="%s after step %d" % (k, step + 1))
        pr = _profile(a)
        assert pr[18] == 3 and pr[4] == 0 and pr[5] == 0 and pr[L.K_HEAT] == 3, pr
        fl = sa["mat"] == 1
        assert np.abs(sa["T"] - sc["T"])[fl].max() > 1.0
    finally:
        a.close(); off.close()


def _profile(eng):
    return {k: eng.profile_read(k)[0] for k in (3, 4, 5, 18, L.K_HEAT)}


def _sheared(sc):
    st = M.host_state(sc)
    x, vel = st["x"].astype(np.float64), st["v"].astype(np.float64)
    vel[:, 0] += 2.0 + 10.0 * (x[:, 1] - x[:, 1].mean())
    vel[:, 2] += 1.0
    return vel.astype(np.float32)


def test_temperature_follows_its_particle_through_the_sort(gpu):
    """WCSPH, alpha = beta = 0 (T <- T + dt 0: the same bits), random T, a sheared, moving block: at least a quarter of the particles
    change cell within 50 steps; T by particle id is what was uploaded, bit for bit, and positions, velocities and densities are those
    of a handle without the mode -- the fused force pass (kernel id 18) kept running, and the walk ran in front of it.  A late object
    starts at its own temperature and the old particles keep theirs."""
    sc = _scene("wcsph", "fluid")
    vel = _sheared(sc)
    outs = {}
    for how in ("off", "on"):
        eng = _engine(sc, "wcsph", 0, heat=None if how == "off" else (0.0, 0.0), spare=64, vel=vel)
        try:
            ids0, cell0 = eng.download(L.F_PARTICLE_ID), eng.download(L.F_GRID_ID)
            eng.profile_enable(-1, True)
            eng.step(50)
            pr = _profile(eng)
            assert pr[18] == 50 and pr[4] == 0 and pr[5] == 0 and pr[L.K_HEAT] == (50 if how == "on" else 0), pr
            ids1, cell1 = eng.download(L.F_PARTICLE_ID), eng.download(L.F_GRID_ID)
            outs[how] = _state(eng, extra=[] if how == "off" else _HEAT)
            if how == "on":
                moved = (H.by_id(ids0, cell0) != H.by_id(ids1, cell1)).mean()
                assert moved >= 0.25 and (ids0 != ids1).mean() > 0.25, moved     # the condition: cells and slots changed
                np.testing.assert_array_equal(_bits(outs["on"]["T"]), _bits(sc["T"]))
                n_old, k = len(ids1), 27
                late = (np.array([0.45, 0.4, 0.4]) + 0.02 * np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)).astype(np.float32)
                eng.set_object(5, 1, 0)
                eng.set_object_temperature(5, 41.5)
                eng.append_particles(5, late, np.zeros((k, 3), np.float32), np.full(k, 1000.0, np.float32), np.zeros(k, np.float32),
                                     np.ones(k, np.int32), np.ones(k, np.int32), np.zeros((k, 3), np.int32))
                t_now = H.by_id(eng.download(L.F_PARTICLE_ID), eng.download(L.F_TEMPERATURE))
                assert (t_now[n_old:] == np.float32(41.5)).all()
                eng.step(2)
                t_end = H.by_id(eng.download(L.F_PARTICLE_ID), eng.download(L.F_TEMPERATURE))
                assert len(t_end) == n_old + k and (t_end[n_old:] == np.float32(41.5)).all()
                np.testing.assert_array_equal(_bits(t_end[:n_old]), _bits(sc["T"]))
        finally:
            eng.close()
    assert np.isfinite(outs["on"]["x"]).all()
    for k in ("x", "v", "rho"):
        np.testing.assert_array_equal(_bits(outs["on"][k]), _bits(outs["off"][k]), err_msg=k)


def test_emitted_layers_and_late_objects_start_at_their_temperature(gpu):
    """The scene keys through the product path: an emitter with "temperature" 70, a block that enters after 5 steps with 33, alpha = 0:
    every particle of either object holds exactly its object's temperature after 40 steps, dump() carries the key."""
    cfg = P.faucet_scene(nozzle=(4, 4), speed=5.0, hold=0, max_layers=12)
    d = 2 * cfg["Configuration"]["particleRadius"]
    dt = cfg["Configuration"]["timeStepSize"]
    cfg["Configuration"].update(thermalMethod="conduction", thermalDiffusivity=0.0, referenceTemperature=20.0)
    em = cfg["Emitters"][0]
    em["temperature"] = 70.0
    late_id = max([em["objectId"]] + [b["objectId"] for b in cfg.get("FluidBlocks", [])]) + 1
    cfg.setdefault("FluidBlocks", []).append({
        "objectId": late_id, "start": [5 * d] * 3, "end": [7.5 * d] * 3, "translation": [0.0, 0.0, 0.0], "scale": [1, 1, 1],
        "velocity": [0.0, 0.0, 0.0], "density": 1000.0, "color": [50, 100, 200], "entryTime": 4.5 * dt, "temperature": 33.0})
    container, solver = P.build_product(cfg)
    try:
        solver.prepare()
        solver.advance(40)
        eng = container.engine
        obj, mat, temp = eng.download(L.F_OBJECT_ID), eng.download(L.F_MATERIAL), eng.download(L.F_TEMPERATURE)
        emitted = (obj == em["objectId"]) & (mat == 1)
        assert emitted.sum() >= 2 * 16 and (temp[emitted] == np.float32(70.0)).all()
        assert (obj == late_id).sum() == 27 and (temp[obj == late_id] == np.float32(33.0)).all()
        dump = container.dump(late_id)
        assert set(dump) == {"position", "velocity", "temperature"} and (dump["temperature"] == np.float32(33.0)).all()
        assert solver.thermal_method == "conduction" and solver.thermal_diffusivity == 0.0 and solver.reference_temperature == 20.0
        assert solver.thermal_expansion == 0.0 and solver.thermal_dt_limit == float("inf")
    finally:
        container.engine.close()


@pytest.mark.parametrize("fast_math", [0, 1])
def test_buoyancy_of_one_particle_over_whole_steps(gpu, fast_math):
    """One isolated particle, T - T_ref = 10, beta = 0.01, 400 WCSPH steps against explicit Euler on the same ODE in float64:
        V_{n+1} = V_n + dt (g + a_b),  X_{n+1} = X_n + dt V_{n+1},  a_b = -beta 10 g.
    The device does, per step and component: v' = fl(v + fl(dt g)), v'' = fl(v' + fl(dt a_b)), x' = fl(x + fl(dt v'')) (an isolated
    particle has no other force and no neighbour to exchange heat with).  With b the model's bound of a_b:
        e_{n+1} <= e_n + dt b + u (dt |g| + dt |a_b|) + 2 u |V_{n+1}|;    ex_{n+1} <= ex_n + dt e_{n+1} + u dt |V_{n+1}| + u |X_{n+1}|
    (the air drag test's form, with a constant acceleration).  With beta = 0 the handle is a handle without the mode, bit for bit."""
    x0 = np.array([0.3, 0.45, 0.26])
    sc = D.particles_scene("wcsph", x0[None, :], np.zeros((1, 3)), gravity=(0.0, -9.81, 0.0))
    sc["T"] = np.array([M.T_REF + 10.0], np.float32)
    Pm = sc["params"]
    dt, g = Pm["dt"], np.asarray(sc["pd"]["gravity"], np.float32).astype(np.float64)
    got = {}
    for how, heat in (("on", (1.0e-4, 0.01)), ("zero", (1.0e-4, 0.0)), ("off", None)):
        eng = _engine(sc, "wcsph", fast_math, heat=heat)
        try:
            xs = eng.download(L.F_POSITION)[0].astype(np.float64)
            eng.step(400)
            got[how] = (eng.download(L.F_VELOCITY)[0], eng.download(L.F_POSITION)[0])
            if heat is not None:
                assert eng.download(L.F_TEMPERATURE)[0] == np.float32(M.T_REF + 10.0)
        finally:
            eng.close()
    for k in (0, 1):
        np.testing.assert_array_equal(_bits(got["zero"][k]), _bits(got["off"][k]))
    r = M.thermal_f64(x0[None, :], sc["T"], np.ones(1), np.ones(1), np.ones(1), np.ones(1, np.int32), np.zeros(1, np.int32), {}, Pm, 0.0, 0.01, M.T_REF)
    a, b = r["a_b"][0], r["a_b_bound"][0]
    V, X, e, ex = np.zeros(3), xs.copy(), np.zeros(3), np.zeros(3)
    for n in range(400):
        V = V + dt * (g + a)
        e = e + dt * b + U * dt * (np.abs(g) + np.abs(a)) + 2 * U * np.abs(V)
        X = X + dt * V
        ex = ex + dt * e + U * dt * np.abs(V) + U * np.abs(X)
    v_dev, x_dev = got["on"][0].astype(np.float64), got["on"][1].astype(np.float64)
    free = dt * 400 * 9.81
    print("buoyant particle [fast_math=%d]: v_y %.6f (model %.6f, free fall %.4f), |err| / bound v %.3f x %.3f"
          % (fast_math, v_dev[1], V[1], -free, (np.abs(v_dev - V) / np.maximum(e, 1e-300)).max(), (np.abs(x_dev - X) / np.maximum(ex, 1e-300)).max()))
    assert abs(a[1] - 0.981) < 1e-6 and a[0] == 0 and a[2] == 0      # upwards: a tenth of g
    assert (np.abs(v_dev - V) <= e).all() and (np.abs(x_dev - X) <= ex).all()
    assert free - abs(V[1]) > 1000 * e.max()      # the buoyancy's effect is far above what the bound could hide


TANK_ALPHA = 0.08


def run_heated_tank(fast_math, hot=60.0, cold=20.0, steps=200, edge=8, beta=0.0):
    """heated_tank_scene(edge) at 0.9 thermal_dt_limit: (T by id per fluid particle, initial positions by id, the solver's limit, dt)."""
    limit = S.thermal_dt_limit(TANK_ALPHA, 0.04, 0.02)
    cfg = P.heated_tank_scene(edge, hot=hot, cold=cold, alpha=TANK_ALPHA, beta=beta, dt=0.9 * limit)
    container, solver = P.build_product(cfg, fast_math=fast_math)
    try:
        solver.prepare()
        eng = container.engine
        ids = eng.download(L.F_PARTICLE_ID)
        fl = H.by_id(ids, eng.download(L.F_MATERIAL)) == 1
        x0 = H.by_id(ids, eng.download(L.F_POSITION))
        solver.advance(steps)
        ids = eng.download(L.F_PARTICLE_ID)
        temp = H.by_id(ids, eng.download(L.F_TEMPERATURE))
        x1 = H.by_id(ids, eng.download(L.F_POSITION))
        return temp[fl], x0[fl], x1[fl], solver.thermal_dt_limit, float(solver.dt[None])
    finally:
        container.engine.close()


@pytest.mark.parametrize("fast_math", [0, 1])
def test_a_heated_plate(gpu, fast_math):
    """heated_tank_scene(8), 200 steps at 0.9 thermal_dt_limit: every T stays within [cold, hot], the layer on the plate is warmer than
    the layer above it, which is warmer than the top one; an adiabatic twin (the plate without the key) keeps every T bit-equal to cold."""
    temp, x0, x1, limit, dt = run_heated_tank(fast_math)
    assert abs(limit / S.thermal_dt_limit(TANK_ALPHA, 0.04, 0.02) - 1) < 1e-12 and abs(dt / (0.9 * limit) - 1) < 1e-6
    assert len(temp) == 512 and np.isfinite(temp).all() and np.isfinite(x1).all()
    assert temp.min() >= np.float32(20.0) and temp.max() <= np.float32(60.0)
    layer = np.rint((x0[:, 1] - x0[:, 1].min()) / 0.02).astype(int)
    means = [float(temp[layer == k].mean()) for k in range(8)]
    print("heated tank fast_math=%d: mean T per initial layer " % fast_math + " ".join("%.3f" % m for m in means))
    assert means[0] > means[1] + 0.5 and means[1] > means[7] and means[0] > 25.0
    cold, _, _, _, _ = run_heated_tank(fast_math, hot=None)
    assert (cold == np.float32(20.0)).all()


def test_beside_outflow(gpu):
    """A block that falls into a kill volume, alpha > 0, random T: finite, the ids stay consistent, and T of the survivors is bit-equal
    to a twin without the volume that removes the model's particles by id between the halves of each step."""
    hi = 0.08 + 7.5 * 0.02
    cfg = P.dam_break_scene(method="wcsph", domain_end=(0.6, 0.6, 0.6), start=(0.08, 0.08, 0.08), end=(hi, hi, hi), translation=(0, 0, 0),
                            dt=4e-4, viscosity=0.05, velocity=(0.0, -3.0, 0.0))
    cfg["Configuration"].update(thermalMethod="conduction", thermalDiffusivity=0.02, thermalExpansion=1e-3, referenceTemperature=M.T_REF)
    kill = {"shape": "box", "min": [0.0, 0.0, 0.0], "max": [0.6, 0.0775, 0.6]}
    with_volume = copy.deepcopy(cfg)
    with_volume["Outflows"] = [kill]
    volumes = [OM.Volume.from_entry(kill)]
    (ca, sa), (cb, sb) = H.build_product(with_volume, jitter=0.004, seed=5), H.build_product(cfg, jitter=0.004, seed=5)
    a, b = ca.engine, cb.engine
    try:
        for s in (sa, sb):
            s.prepare()
        n0 = a.particle_num
        temp = np.random.default_rng(3).uniform(M.T_LO, M.T_HI, n0).astype(np.float32)
        for e in (a, b):
            _upload_by_id(e, L.F_TEMPERATURE, temp)
        dt = float(np.float32(4e-4))
        for k in range(1, 31):
            a.step(1)
            b.step_begin()
            ids, pos = b.download(L.F_PARTICLE_ID), b.download(L.F_POSITION)
            hit = OM.attribute(volumes, pos, k, dt, object_ids=b.download(L.F_OBJECT_ID), fluid=b.download(L.F_MATERIAL) == L.MAT_FLUID)
            if (hit >= 0).any():
                b.remove_particles(ids[hit >= 0])
            b.step_end()
        ia, ib = a.download(L.F_PARTICLE_ID), b.download(L.F_PARTICLE_ID)
        assert a.particle_num < n0 - 50 and len(np.unique(ia)) == len(ia) and ia.max() < n0
        ta, tb = a.download(L.F_TEMPERATURE), b.download(L.F_TEMPERATURE)
        assert np.isfinite(ta).all() and np.isfinite(a.download(L.F_POSITION)).all()
        np.testing.assert_array_equal(np.sort(ia), np.sort(ib))
        np.testing.assert_array_equal(_bits(ta[np.argsort(ia)]), _bits(tb[np.argsort(ib)]))
        assert np.abs(ta[np.argsort(ia)] - temp[np.sort(ia)]).max() > 0.5    # it did conduct
    finally:
        a.close(); b.close()


def test_beside_the_cfl_step(gpu):
    """cflMethod "velocity": the update takes the step's own dt from the constants every kernel reads.  20 steps of a falling block:
    finite, ids consistent, T within the range it started in (the steps are far below the limit), and the step did change."""
    hi = 0.08 + 7.5 * 0.02
    cfg = P.dam_break_scene(method="wcsph", domain_end=(0.6, 0.6, 0.6), start=(0.08, 0.08, 0.08), end=(hi, hi, hi), translation=(0, 0, 0),
                            dt=4e-4, viscosity=0.05, velocity=(0.0, -3.0, 0.0))
    cfg["Configuration"].update(thermalMethod="conduction", thermalDiffusivity=0.02, thermalExpansion=1e-3, referenceTemperature=M.T_REF,
                                cflMethod="velocity", cflFactor=0.05, cflMinTimeStepSize=1e-5, cflMaxTimeStepSize=4e-4)
    container, solver = H.build_product(cfg, jitter=0.004, seed=5)
    eng = container.engine
    try:
        solver.prepare()
        n0 = eng.particle_num
        temp = np.random.default_rng(3).uniform(M.T_LO, M.T_HI, n0).astype(np.float32)
        _upload_by_id(eng, L.F_TEMPERATURE, temp)
        solver.advance(20)
        ids, t1 = eng.download(L.F_PARTICLE_ID), eng.download(L.F_TEMPERATURE)
        assert eng.particle_num == n0 and np.array_equal(np.sort(ids), np.arange(n0))
        assert np.isfinite(t1).all() and t1.min() >= temp.min() and t1.max() <= temp.max()
        assert np.abs(H.by_id(ids, t1) - temp).max() > 0.5
        assert float(solver.dt[None]) < 4e-4 and solver.thermal_dt_limit > 4e-4
    finally:
        eng.close()


@pytest.mark.parametrize("fast_math", [0, 1])
def test_mode_off_is_the_old_code(gpu, fast_math):
    """Never touched, set to "none", set to "conduction" and back: 20 WCSPH steps, bit-identical; the fused force pass (kernel id 18)
    ran and the new id did not.  With the mode on and beta != 0: 4, 5 and the new id run, 18 does not."""
    sc = _scene("wcsph", "rigid")
    outs, profs = [], []
    for how in ("untouched", "none", "back", "on"):
        eng = _engine(sc, "wcsph", fast_math, heat=None)
        try:
            if how == "none":
                eng.set_thermal("none")
            elif how == "back":
                eng.set_thermal("conduction", 0.2, 0.3, 0.4)
                assert eng.get_thermal() == dict(method="conduction", alpha=0.2, beta=0.3, t_ref=0.4)
                eng.set_object_temperature(M.PLATE, M.T_WALL)
                _upload_by_id(eng, L.F_TEMPERATURE, sc["T"])
                eng.set_thermal("none", 0.2, 0.3, 0.4)
                assert eng.get_thermal() == dict(method="none", alpha=0.2, beta=0.3, t_ref=0.4)
                eng.set_thermal("conduction", 0.2, 0.3, 0.4)
                eng.set_thermal(None)
                assert eng.get_thermal()["method"] == "none"
            elif how == "on":
                eng.set_thermal("conduction", _alpha(sc["params"]), BETA, M.T_REF)
                eng.set_object_temperature(M.PLATE, M.T_WALL)
                _upload_by_id(eng, L.F_TEMPERATURE, sc["T"])
            eng.profile_enable(-1, True)
            eng.step(20)
            profs.append(_profile(eng))
            outs.append(_state(eng, extra=_HEAT if how in ("back", "on") else []))
        finally:
            eng.close()
    for o in outs[1:3]:
        for k in ("x", "v", "rho"):
            np.testing.assert_array_equal(_bits(o[k]), _bits(outs[0][k]), err_msg=k)
    fl = outs[0]["mat"] == 1
    np.testing.assert_array_equal(_bits(outs[2]["T"][fl]), _bits(sc["T"][fl]))   # switched off: the temperatures are kept, nothing walks
    for pr in profs[:3]:
        assert pr[18] == 20 and pr[4] == 0 and pr[5] == 0 and pr[L.K_HEAT] == 0, pr
    assert profs[3][18] == 0 and profs[3][4] == 20 and profs[3][5] == 20 and profs[3][L.K_HEAT] == 20, profs[3]
    assert np.abs(outs[3]["x"] - outs[0]["x"]).max() > 1e-7 and np.isfinite(outs[3]["x"]).all() and np.isfinite(outs[3]["T"]).all()


@pytest.mark.parametrize("fast_math", [0, 1])
def test_determinism_and_async_steps(gpu, fast_math):
    """Mode on: two runs give the same bits, one sph_step(h, 25) is 25 calls bit for bit, sph_step_async agrees."""
    sc = _scene("wcsph", "rigid")
    outs = []
    for how in ("once", "again", "one_by_one", "async"):
        eng = _engine(sc, "wcsph", fast_math)
        try:
            if how in ("once", "again"):
                eng.step(25)
            elif how == "one_by_one":
                for _ in range(25):
                    eng.step(1)
            else:
                eng.step_async(25)
                eng.synchronize()
            outs.append(_state(eng, extra=_HEAT))
        finally:
            eng.close()
    fl = outs[0]["mat"] == 1
    assert np.isfinite(outs[0]["T"]).all() and np.abs(outs[0]["T"] - sc["T"])[fl].max() > 1.0
    for o in outs[1:]:
        for k in ("x", "v", "rho", "T"):
            np.testing.assert_array_equal(_bits(o[k]), _bits(outs[0][k]), err_msg=k)


def _rc(call, *words):
    try:
        call()
    except L.SphError as e:
        assert all(w in str(e) for w in words), (str(e), words)
        return e.code
    return 0


def test_refusals(gpu, monkeypatch, tmp_path):
    sc = _scene("wcsph", "fluid")
    eng = L.Engine(_params(sc, "pbf"))
    assert _rc(lambda: eng.set_thermal("conduction"), "sph_set_thermal", "PBF") == L.ERR_UNSUPPORTED
    eng.set_pbf_variant("consistent")
    assert _rc(lambda: eng.set_thermal("conduction"), "sph_set_thermal", "PBF") == L.ERR_UNSUPPORTED
    eng.close()
    eng = L.Engine(_params(sc, "wcsph"))
    for bad in (dict(alpha=-1.0), dict(beta=-1.0), dict(alpha=float("nan")), dict(beta=float("inf")), dict(t_ref=float("nan")), dict(method=2)):
        assert _rc(lambda: eng.set_thermal(**bad), "sph_set_thermal") == L.ERR_INVALID, bad
    assert eng.get_thermal() == dict(method="none", alpha=1e-4, beta=0.0, t_ref=0.0)
    assert _rc(lambda: eng.set_object_temperature(20, 1.0), "sph_set_object_temperature") == L.ERR_INVALID
    assert _rc(lambda: eng.set_object_temperature(-2, 1.0), "sph_set_object_temperature") == L.ERR_INVALID
    assert _rc(lambda: eng.set_object_temperature(1, float("inf")), "sph_set_object_temperature") == L.ERR_INVALID
    assert _rc(lambda: eng.run_phase(L.PH_HEAT)) == L.ERR_INVALID
    assert _rc(lambda: eng.download(L.F_TEMPERATURE)) == L.ERR_UNSUPPORTED
    assert _rc(lambda: eng.download(L.F_TEMPERATURE_RATE)) == L.ERR_UNSUPPORTED
    # the ids: the temperatures are stored by id, in append order
    T.feed(eng, sc, oracle=False)
    n = eng.particle_num
    eng.set_object_temperature(3, 44.0)   # (before the mode: the particles present start at their object's temperature)
    eng.set_thermal("conduction", 1e-4, 0.0, 7.0)
    t0, obj = eng.download(L.F_TEMPERATURE), eng.download(L.F_OBJECT_ID)
    assert (t0[obj == 3] == np.float32(44.0)).all() and (t0[obj == 0] == np.float32(7.0)).all() and (obj == 3).sum() > 0
    assert _rc(lambda: eng.set_appended_ids(np.arange(n, dtype=np.int32)), "set_appended_ids", "heat") == L.ERR_UNSUPPORTED
    assert _rc(lambda: eng.upload(L.F_PARTICLE_ID, np.arange(n, dtype=np.int32)), "upload", "heat") == L.ERR_UNSUPPORTED
    assert _rc(lambda: eng.upload(L.F_TEMPERATURE_RATE, np.zeros(n, np.float32))) == L.ERR_UNSUPPORTED   # download only
    bad = t0.copy(); bad[0] = np.nan
    assert _rc(lambda: eng.upload(L.F_TEMPERATURE, bad), "upload") == L.ERR_INVALID
    eng.set_thermal("none")
    eng.set_appended_ids(np.arange(n, dtype=np.int32))
    assert _rc(lambda: eng.set_thermal("conduction"), "sph_set_thermal", "ids") == L.ERR_UNSUPPORTED
    eng.close()
    # sharded handles: two ranks on one GPU over the shared-memory transport, one thread each
    monkeypatch.setenv("SPH_COMM_TRANSPORT", "shm")
    monkeypatch.setenv("SPH_COMM_TIMEOUT_S", "20")
    engs = [L.Engine(_params(sc, "wcsph")) for _ in range(2)]
    uid = engs[0].comm_unique_id()
    nz = int(_params(sc, "wcsph").grid_num[2])
    got = [None, None]

    def rank(k):
        engs[k].comm_init(k, 2, uid)
        if k == 1:   # the other order: the mode first, then the slab
            engs[k].set_thermal("conduction")
            got[k] = _rc(lambda: engs[k].comm_set_slab(nz // 2, nz), "comm_set_slab", "heat")
            engs[k].set_thermal("none")
        engs[k].comm_set_slab(*((0, nz // 2) if k == 0 else (nz // 2, nz)))
        if k == 0:
            got[k] = _rc(lambda: engs[k].set_thermal("conduction"), "sph_set_thermal", "sharded")

    threads = [threading.Thread(target=rank, args=(k,), daemon=True) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads)
    assert got == [L.ERR_UNSUPPORTED, L.ERR_UNSUPPORTED], got
    for e in engs:
        e.close()
    # the driver: --gpus 2 on a thermal scene ends in the parent with code 2, before a rank starts
    path = tmp_path / "tank.json"
    path.write_text(json.dumps(P.heated_tank_scene(4)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sph_project_amd", "run_simulation.py"), "--scene_file", str(path), "--gpus", "2"],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "conduction" in r.stderr, (r.returncode, r.stderr[-400:])
