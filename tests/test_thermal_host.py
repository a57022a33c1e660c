"""No GPU: the float64 model of the heat conduction (tests/thermal_terms.py) -- its mutants, the kernels' pair arithmetic and finish run
on the CPU (sph_heat_pair_host, sph_heat_finish_host) against it, the Laplacian of a linear and of a quadratic profile on the rest
lattice, conservation, the maximum principle below the step limit -- and the scene keys."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd import scene as S
from sph_project_amd.SPH.utils import SimConfig
from tests import thermal_terms as H
from tests import nonpressure_terms as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = H.U
BETA = 2.0e-3
_CACHE = {}


def _alpha(Pm):
    """Half the diffusivity at which the scene's step IS the step limit: every term of the update is of the size of T itself."""
    return 0.5 * 0.5 / (2.0 * 1.25 * H.lattice_sum(Pm["h"], Pm["diameter"]) * Pm["dt"])


def _case(kind):
    """The scene, its host state (f32 inputs, both densities), the temperatures and the model's answer."""
    if kind not in _CACHE:
        sc = H.scene("wcsph", kind)
        st = H.host_state(sc)
        st["rho_raw"] = st["rho_raw"].astype(np.float32)
        st["rho"] = st["rho"].astype(np.float32)
        st["T"] = H.temperatures(sc)
        _CACHE[kind] = (sc, st, _model(sc, st))
    return _CACHE[kind]


def _model(sc, st, mutant=None, temp=None):
    Pm = sc["params"]
    return H.thermal_f64(st["x"], st["T"] if temp is None else temp, st["rho_raw"], st["mass"], st["vol"], st["mat"], st["obj"], H.WALLS,
                         Pm, _alpha(Pm), BETA, H.T_REF, mutant=mutant, rho_alt=st["rho"])


def _fractions(st, ref, rate, t_new, a_b):
    """error / bound of a candidate (dT/dt, new T, buoyancy) against the model's answer"""
    fl = st["mat"] == 1
    return {"rate": float((np.abs(rate - ref["rate"])[fl] / ref["rate_bound"][fl]).max()),
            "T": float((np.abs(t_new - ref["T_new"])[fl] / ref["T_bound"][fl]).max()),
            "a_b": float((np.abs(a_b - ref["a_b"])[fl, 1] / ref["a_b_bound"][fl, 1]).max()),   # (gravity acts along y alone:
            "a_b xz": float(np.abs(a_b - ref["a_b"])[fl][:, (0, 2)].max())}                       #  the other two are exactly zero)


@pytest.mark.parametrize("kind", H.KINDS)
def test_scenes_are_alive(kind):
    sc, st, ref = _case(kind)
    fl = st["mat"] == 1
    H.assert_alive(ref, st["T"].astype(np.float64), fl, sc["rigid"])
    assert st["T"][fl].min() >= H.T_LO and st["T"][fl].max() <= H.T_HI and np.ptp(st["T"][fl]) > 0.9 * (H.T_HI - H.T_LO)
    assert abs(sc["params"]["g"][1]) > 9.0 and sc["params"]["g"][0] == 0 and sc["params"]["g"][2] == 0


@pytest.mark.parametrize("mutant", H.MUTANTS)
def test_every_mutant_of_the_model_misses_a_bound(mutant):
    """On EVERY scene it applies to (the mutants that need a boundary: on the two scenes that have one)."""
    kinds = [k for k in H.KINDS if k in ("rigid", "lattice") or mutant not in H.RIGID_MUTANTS]
    worst = {}
    for kind in kinds:
        sc, st, ref = _case(kind)
        mut = _model(sc, st, mutant)
        worst[kind] = max(_fractions(st, ref, mut["rate"], mut["T_new"], mut["a_b"]).values())
    print("mutant %s, worst error / bound per scene:" % mutant, ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert min(worst.values()) > 1.0, (mutant, worst)


def _pair_records(st, ref, Pm):
    """One record of 12 float32 per pair of the model's pair list, as sph_hip.h lists them; the kernel values from the float64 spline."""
    p = ref["pairs"]
    i, j, fl, wall = p["i"], p["j"], p["fluid_j"], p["wall_j"]
    f32 = np.float32
    x, t = st["x"].astype(f32), st["T"].astype(f32)
    rho, m, vol = st["rho_raw"].astype(f32), st["mass"].astype(f32), st["vol"].astype(f32)
    d = x[i] - x[j]
    r2 = (d.astype(np.float64) ** 2).sum(axis=1)
    s, _ = T.kernel_grad_scale(np.sqrt(r2), Pm["h"])
    t_wall = np.array([H.WALLS.get(int(o), 0.0) for o in st["obj"][j]], f32)
    rec = np.zeros((len(i), 12), f32)
    rec[:, 0] = t[i]
    rec[:, 1] = np.where(fl, m[j] / rho[j], np.where(wall, vol[j], f32(0)))
    rec[:, 2] = np.where(fl, t[j], np.where(wall, t_wall, f32(0)))
    rec[:, 3:6] = d
    rec[:, 6] = r2
    rec[:, 7] = 0.01 * Pm["h"] ** 2
    rec[:, 8] = s
    rec[:, 9:12] = s[:, None] * d.astype(np.float64)
    return rec


def _host_answer(sc, st, ref, fast):
    """The rows of sph_heat_pair_host summed in float64, then sph_heat_finish_host: (dT/dt, T_new, a_b)."""
    Pm = sc["params"]
    terms = L.heat_pair_host(_pair_records(st, ref, Pm), fast).astype(np.float64)
    assert np.isfinite(terms).all()
    n = len(st["x"])
    sums = T._sum(ref["pairs"]["i"], n, terms)
    rec = np.zeros((n, 12), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = sums, 2.0 * _alpha(Pm), Pm["rho0"], st["rho_raw"]
    rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 7] = Pm["dt"], st["T"], -BETA, H.T_REF
    rec[:, 8:11] = np.asarray(Pm["g"], np.float32)
    out = L.heat_finish_host(rec, fast).astype(np.float64)
    fl = st["mat"] == 1
    return np.where(fl, out[:, 0], 0.0), np.where(fl, out[:, 1], st["T"]), np.where(fl[:, None], out[:, 2:5], 0.0), terms


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("kind", H.KINDS)
def test_pair_arithmetic_of_the_kernel_source_against_the_model(kind, fast):
    """sph_heat_pair_host runs heat_pair<FAST> of csrc/sph_thermal.hpp pair by pair, sph_heat_finish_host heat_finish<FAST> and
    heat_buoyancy: dT/dt, the new T and a_b within the model's bounds; an adiabatic neighbour's term is exactly zero."""
    sc, st, ref = _case(kind)
    rate, t_new, a_b, terms = _host_answer(sc, st, ref, fast)
    p = ref["pairs"]
    assert (terms[~p["fluid_j"] & ~p["wall_j"]] == 0).all()
    assert (terms[(p["c"] != 0) & (terms != 0)] * (st["T"][p["i"]] - np.where(p["fluid_j"], st["T"][p["j"]], H.T_WALL))[(p["c"] != 0) & (terms != 0)] < 0).all()   # F < 0
    fr = _fractions(st, ref, rate, t_new, a_b)
    print("pair arithmetic [%s, fast=%d], error / bound:" % (kind, fast), ", ".join("%s %.3f" % kv for kv in fr.items()))
    assert max(fr.values()) <= 1.0, fr


def test_host_entries_refuse_bad_arguments():
    lib = L.load()
    r = np.zeros(12, np.float32)
    for f in (lib.sph_heat_pair_host, lib.sph_heat_finish_host):
        assert f(r.ctypes.data, -1, r.ctypes.data, 0) == L.ERR_INVALID
        assert f(None, 1, r.ctypes.data, 0) == L.ERR_INVALID
        assert f(None, 0, None, 1) == 0


def _lattice_model(temp, alpha=1.0e-4):
    lat = H.rest_lattice()
    Pm = dict(h=0.04, rho0=1000.0, dt=4e-4, g=(0.0, -9.81, 0.0))
    n = len(lat["x"])
    res = H.thermal_f64(lat["x"], temp(lat["x"]), lat["rho_raw"], lat["mass"], lat["vol"], lat["mat"], np.zeros(n, np.int32), {}, Pm, alpha, 0.0, 0.0)
    c = np.abs(lat["x"] - lat["x"][lat["centre"]]).max(axis=1)
    interior = c <= 2 * 0.02 * (1 + 1e-9)   # the particles whose whole support lies inside the 9^3 block
    return lat, res, interior


def test_a_linear_profile_has_no_rate_in_the_interior():
    """T = a . x on the exact 9^3 rest lattice: the neighbours of an interior particle come in opposite pairs, so dT/dt = 0 to the
    model's own bound (which measures the cancelled terms)."""
    a = np.array([130.0, -70.0, 210.0])
    lat, res, interior = _lattice_model(lambda x: x @ a, alpha=0.05)
    assert interior.sum() == 125 and lat["neighbours"] == 32
    assert (res["mag"][interior] > 10.0).all()   # the terms that cancel, K / s
    assert (np.abs(res["rate"][interior]) <= res["rate_bound"][interior]).all()
    assert np.abs(res["rate"][~interior]).max() > 1.0   # ... and a particle at the block's face does see the gradient


def test_a_quadratic_profile_measures_kappa():
    """T = x^2 (Laplacian 2): an interior particle of the rest lattice gets dT/dt = 2 alpha kappa.  kappa is MEASURED here by the float64
    model and quoted in DESIGN.md 40 and the README; what is asserted is that it is one number: the same along x, y and z and in
    every interior particle, proportional to alpha, and not far from the 1 an exact Laplacian would give."""
    alpha = 1.0e-4
    kappa = []
    for axis in range(3):
        lat, res, interior = _lattice_model(lambda x, k=axis: x[:, k] ** 2, alpha=alpha)
        kappa.append(res["rate"][interior] / (2.0 * alpha))
    kappa = np.array(kappa)
    print("kappa on the rest lattice (raw density, 0.800 rho0): %.4f (spread %.2e over 3 x 125 interior particles)" % (kappa.mean(), np.ptp(kappa)))
    assert np.ptp(kappa) <= 1e-9 * kappa.mean()
    assert 0.5 < kappa.mean() < 2.0
    lat, res, interior = _lattice_model(lambda x: x[:, 0] ** 2, alpha=3 * alpha)
    np.testing.assert_allclose(res["rate"][interior] / (6.0 * alpha), kappa.mean(), rtol=1e-9)


def test_one_mass_all_fluid_conserves_heat():
    """m_i dT_i/dt is antisymmetric in (i, j) for equal masses: sum m_i rate_i = 0 -- in the model to float64 roundoff, in the kernel
    source's answer to the sum of the rows' bounds."""
    sc, st, ref = _case("lattice_fluid")
    m = st["mass"].astype(np.float64)
    assert np.ptp(m) == 0
    assert abs((m * ref["rate"]).sum()) <= 1e-12 * (m * ref["mag"]).sum()
    for fast in (False, True):
        rate, _, _, _ = _host_answer(sc, st, ref, fast)
        assert abs((m * rate).sum()) <= (m * ref["rate_bound"]).sum()
    assert (m * ref["mag"]).sum() > 1e3 * (m * ref["rate_bound"]).sum()


def test_maximum_principle_below_the_step_limit():
    """At 0.9 thermal_dt_limit, 100 Jacobi steps of the model on the jittered block with the heated plate and the adiabatic cube keep
    every T inside [min, max] of the initial and the wall values."""
    sc, st, _ = _case("rigid")
    Pm = dict(sc["params"])
    alpha = _alpha(Pm)
    limit = S.thermal_dt_limit(alpha, Pm["h"], Pm["diameter"])
    assert abs(limit / H.dt_limit(alpha, Pm["h"], Pm["diameter"]) - 1) < 1e-12 and abs(limit / (2 * Pm["dt"]) - 1) < 1e-9
    Pm["dt"] = 0.9 * limit
    fl = st["mat"] == 1
    temp = st["T"].astype(np.float64)
    lo, hi = min(temp[fl].min(), H.T_WALL), max(temp[fl].max(), H.T_WALL)
    spread0 = np.ptp(temp[fl])
    for _ in range(100):
        temp = H.thermal_f64(st["x"], temp, st["rho_raw"], st["mass"], st["vol"], st["mat"], st["obj"], H.WALLS, Pm, alpha, 0.0, H.T_REF)["T_new"]
        assert temp[fl].min() >= lo and temp[fl].max() <= hi
    assert temp[fl].mean() > st["T"][fl].mean() + 5.0 and temp[fl].max() > st["T"][fl].max() + 5.0   # the plate did heat: past the fluid's own hottest
    assert spread0 > 50.0


# ------------------------------------------------------------------------------------------------------------ scene keys
def _cfg(objects=None, **keys):
    cfg = P.heated_tank_scene(4, alpha=None)
    cfg["Configuration"].update(keys)
    for (group, index), temp in (objects or {}).items():
        cfg[group][index]["temperature"] = temp
    return cfg


ON = dict(thermalMethod="conduction")


@pytest.mark.parametrize("keys, objects, word", [
    (dict(thermalMethod="radiation"), None, "thermalMethod"),
    (dict(thermalMethod=1), None, "thermalMethod"),
    (dict(thermalDiffusivity=1e-4), None, "thermalDiffusivity"),
    (dict(thermalMethod="none", thermalExpansion=1e-3), None, "thermalExpansion"),
    (dict(referenceTemperature=20.0), None, "referenceTemperature"),
    (dict(domainBoxTemperature=20.0), None, "domainBoxTemperature"),
    (dict(), {("FluidBlocks", 0): 30.0}, "temperature"),
    (dict(thermalMethod="none"), {("RigidBodies", 0): 30.0}, "temperature"),
    (dict(ON, thermalDiffusivity=-1e-4), None, "thermalDiffusivity"),
    (dict(ON, thermalDiffusivity=float("nan")), None, "thermalDiffusivity"),
    (dict(ON, thermalExpansion=-1.0), None, "thermalExpansion"),
    (dict(ON, thermalExpansion=float("inf")), None, "thermalExpansion"),
    (dict(ON, thermalExpansion="0.1"), None, "thermalExpansion"),
    (dict(ON, referenceTemperature=float("inf")), None, "referenceTemperature"),
    (dict(ON, domainBoxTemperature=float("nan")), None, "domainBoxTemperature"),
    (dict(ON), {("FluidBlocks", 0): float("nan")}, "temperature"),
    (dict(ON), {("RigidBodies", 0): "hot"}, "temperature"),
    (dict(ON, simulationMethod="pbf"), None, "thermalMethod"),
    (dict(ON, gravitationUpper=0.5), None, "gravitationUpper"),
])
def test_bad_keys_raise_before_a_device_is_opened(monkeypatch, keys, objects, word):
    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(L, "Engine", no_device)
    with pytest.raises(ValueError, match=word):
        P.build_product(_cfg(objects, **keys))


def test_emitter_temperature_is_a_known_key_and_needs_the_mode():
    cfg = P.faucet_scene()
    cfg["Emitters"][0]["temperature"] = 70.0
    with pytest.raises(ValueError, match="temperature"):
        S.thermal_of(SimConfig(config=cfg), "wcsph")
    cfg["Configuration"]["thermalMethod"] = "conduction"
    th = S.thermal_of(SimConfig(config=cfg), "wcsph")
    assert th["objects"] == {cfg["Emitters"][0]["objectId"]: 70.0}
    assert S.emitters_of(SimConfig(config=cfg), "wcsph")[0]["objectId"] == cfg["Emitters"][0]["objectId"]


def test_two_d_scene_is_refused_by_name():
    cfg = SimConfig(config=_cfg(**ON))
    with pytest.raises(ValueError, match="thermalMethod"):
        S.thermal_of(cfg, "dfsph", dim=2)
    assert S.thermal_of(cfg, "dfsph", dim=3) == dict(method="conduction", alpha=1e-4, beta=0.0, t_ref=0.0, box=None, objects={})


def test_scene_without_the_keys_is_the_scene_it_was():
    plain = SimConfig(config=_cfg())
    keyed = SimConfig(config=P.heated_tank_scene(4, hot=55.0, cold=12.0, alpha=2e-4, beta=1e-3, domainBoxTemperature=5.0))
    off = dict(method="none", alpha=1e-4, beta=0.0, t_ref=0.0, box=None, objects={})
    assert S.thermal_of(plain, "wcsph") == off
    assert S.thermal_of(SimConfig(config=_cfg(thermalMethod="none")), "wcsph") == off
    assert S.thermal_of(keyed, "wcsph") == dict(method="conduction", alpha=2e-4, beta=1e-3, t_ref=12.0, box=5.0, objects={0: 12.0, 1: 55.0})
    pds = [S.params_dict(S.derive_geometry(c), S.derive_solver_constants(c), "wcsph", 64) for c in (plain, keyed)]
    assert pds[0] == pds[1]   # the parameter block never sees the keys
    a, b = P.scene_particles(_cfg())[2], P.scene_particles(P.heated_tank_scene(4))[2]
    assert len(a) == len(b)
    for x, y in zip(a, b):   # ... nor do the particles
        for k in ("pos", "vel", "material"):
            np.testing.assert_array_equal(x[k], y[k])


def test_step_past_the_limit_warns_and_stays(monkeypatch):
    """The treatment elastic_dt_limit gets: a warning that names the key; the container is built all the same (here: up to the device)."""
    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(L, "Engine", no_device)
    limit = S.thermal_dt_limit(0.2, 0.04, 0.02)
    assert limit < 4e-4
    with pytest.warns(UserWarning, match="timeStepSize .* exceeds the thermal limit"):
        with pytest.raises(AssertionError, match="a device was opened"):
            P.build_product(P.heated_tank_scene(4, alpha=0.2))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(AssertionError, match="a device was opened"):
            P.build_product(P.heated_tank_scene(4, alpha=0.01))
    assert S.thermal_dt_limit(0.0, 0.04, 0.02) == float("inf")


def test_driver_refuses_gpus_2_on_a_thermal_scene(tmp_path):
    path = tmp_path / "tank.json"
    path.write_text(json.dumps(P.heated_tank_scene(4)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sph_project_amd", "run_simulation.py"), "--scene_file", str(path), "--gpus", "2"],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "conduction" in r.stderr and "--gpus 2" in r.stderr, (r.returncode, r.stderr[-400:])


def test_heated_tank_scene_shapes():
    cfg = P.heated_tank_scene(6, hot=70.0, cold=10.0, alpha=3e-4, beta=2e-3)
    conf = cfg["Configuration"]
    assert (conf["thermalMethod"], conf["thermalDiffusivity"], conf["thermalExpansion"], conf["referenceTemperature"]) == ("conduction", 3e-4, 2e-3, 10.0)
    assert cfg["FluidBlocks"][0]["temperature"] == 10.0 and cfg["RigidBodies"][0]["temperature"] == 70.0
    c, geo, batches = P.scene_particles(cfg)
    box, fluid = batches
    body = cfg["RigidBodies"][0]
    p = np.asarray(body["voxelizedPoints"], np.float64)
    assert len(fluid["pos"]) == 216 and (box["material"] == 2).all() and len(p) == 10 * 2 * 10 and body["isDynamic"] is False
    d = geo.particle_diameter
    x = fluid["pos"].astype(np.float64)
    assert abs((x[:, 1].min() - p[:, 1].max()) / d - 1.0) < 1e-5                    # one diameter above the plate's upper layer
    assert abs((x[:, 0].min() - p[:, 0].min()) / d - 2.0) < 1e-5 and abs((p[:, 2].max() - x[:, 2].max()) / d - 2.0) < 1e-5
    assert (p.min(0) - box["pos"].min(0) - geo.domain_box_thickness).min() > 0      # the plate lies inside the shell
    assert "temperature" not in P.heated_tank_scene(6, hot=None)["RigidBodies"][0]
    assert "RigidBodies" not in P.heated_tank_scene(6, plate=False)
    bare = P.heated_tank_scene(6, alpha=None)
    assert "thermalMethod" not in bare["Configuration"] and "temperature" not in bare["FluidBlocks"][0]


# ------------------------------------------------------------------------------------------------------------ C-ABI
def test_abi_additions(tmp_path):
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    for name in ("sph_set_thermal", "sph_get_thermal", "sph_set_object_temperature", "sph_heat_pair_host", "sph_heat_finish_host"):
        assert f"int {name}(" in header and name in L.EXPORTED_SYMBOLS and getattr(L.load(), name) is not None
    assert re.search(r"\bSPH_F_TEMPERATURE\s*=\s*52\b", header) and L.F_TEMPERATURE == 52
    assert re.search(r"\bSPH_F_TEMPERATURE_RATE\s*=\s*53\b", header) and L.F_TEMPERATURE_RATE == 53
    assert re.search(r"\bSPH_PH_HEAT\s*=\s*35\b", header) and L.PH_HEAT == 35
    assert re.search(r"\bSPH_K_HEAT\s*=\s*38\b", header) and L.K_HEAT == 38
    assert L._FIELD_SPEC[L.F_TEMPERATURE] == (np.float32, 1) and L._FIELD_SPEC[L.F_TEMPERATURE_RATE] == (np.float32, 1)
    lib = L.load()
    lib.sph_kernel_name.restype = C.c_char_p
    assert lib.sph_kernel_name(38) == b"?" and lib.sph_kernel_name(29) == b"pbfc_delta"
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sph_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(SphThermal), offsetof(SphThermal, alpha), offsetof(SphThermal, beta), '
                   'offsetof(SphThermal, t_ref), sizeof(SphParams), sizeof(SphStats)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    Th = L.SphThermal
    assert got == [C.sizeof(Th), Th.alpha.offset, Th.beta.offset, Th.t_ref.offset, C.sizeof(L.SphParams), C.sizeof(L.SphStats)]
