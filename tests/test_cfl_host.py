"""CPU: adaptive time stepping without a device -- the rule and the reduce's per-particle arithmetic run on the host
(sph_cfl_dt_host, sph_cfl_speed2_host) against the numpy model tests/cfl_model.py: zero speed, speeds exactly at both clamp edges and
one float32 step either side, landing with 1, 1.5, 2 and 5.3 CFL steps to go and with less than the tolerance, NaN and inf; mutants of the
model; every refusal of the scene parser by message; the container's refusals before a device is opened; the ABI symbols.

The rule is defined in float64 with exactly rounded operations and the speed in float32 with a fixed evaluation order, so model and
library must agree bit for bit: every comparison here is an equality, no tolerance."""
import copy
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd import scene
from sph_project_amd.SPH.utils import SimConfig
from tests import cfl_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = 0.02
FACTOR, DT_MIN, DT_MAX = 0.15, 1e-5, 6e-4
PARAMS = (FACTOR, DT_MIN, DT_MAX)
LIM = FACTOR * 0.4 * D


def _p(factor=FACTOR, dt_min=DT_MIN, dt_max=DT_MAX):
    return L.cfl_params("velocity", factor, dt_min, dt_max)


def _edge_v2(dt_edge):
    """The float32 squares around the speed at which the unclamped step equals dt_edge: three below, the nearest, three above."""
    v2 = F((LIM / dt_edge) ** 2)
    out = [v2]
    lo = hi = v2
    for _ in range(3):
        lo, hi = np.nextafter(lo, F(0)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return sorted(out)


def speeds():
    """float32 squares of speed: zero, the smallest normal, ordinary speeds, both clamp edges and float32 steps either side."""
    out = [F(0.0), F(np.finfo(F).tiny), F(1e-6), F(1.0), F(9.0), F(3.0) ** 2, F(37.5), F(1e4), F(1e8), F(3e38)]
    out += _edge_v2(DT_MAX) + _edge_v2(DT_MIN)
    rng = np.random.default_rng(5)
    out += list(np.exp(rng.uniform(np.log(0.5), np.log(3e4), 200)).astype(F))
    return out


def landings(v2):
    """remaining times for a square: none, 1, 1.5, 2 and 5.3 CFL steps, below / at / just above the tolerance."""
    dt, _ = M.rule(*PARAMS, D, v2)
    tol = M.REACHED * DT_MAX
    return [None, dt, 1.5 * dt, 2.0 * dt, 5.3 * dt, 0.5 * tol, tol, math.nextafter(tol, 1.0), 0.3 * dt]


def test_rule_equals_the_model():
    seen = set()
    for v2 in speeds():
        for rem in landings(v2):
            want = M.rule(*PARAMS, D, v2, rem)
            got = L.cfl_dt_host(_p(), D, v2, float("nan") if rem is None else rem)
            assert got == want, (v2, rem, got, want)
            seen.add(want[1])
            if rem is not None and rem > M.REACHED * DT_MAX:
                free, _ = M.rule(*PARAMS, D, v2)
                assert want[1] & M.LANDING and want[0] <= free and (rem < free or want[0] >= F(0.5 * free)), (v2, rem, want, free)
    assert seen == {0, M.CLAMPED_MAX, M.CLAMPED_MIN, M.LANDING, M.LANDING | M.CLAMPED_MAX, M.LANDING | M.CLAMPED_MIN}


def test_rule_at_the_clamp_edges():
    """Exactly at an edge and one float32 step to either side: the flag changes where the model says, the step never leaves the clamps."""
    for edge, flag in ((DT_MAX, M.CLAMPED_MAX), (DT_MIN, M.CLAMPED_MIN)):
        flags = []
        for v2 in _edge_v2(edge):
            dt, f = L.cfl_dt_host(_p(), D, v2)
            assert (dt, f) == M.rule(*PARAMS, D, v2) and float(F(DT_MIN)) <= dt <= float(F(DT_MAX))
            flags.append(f)
        assert flags[0] != flags[-1] and {flag} == set(flags) - {0}, (edge, flags)   # the edge lies inside the seven squares
        assert flags == sorted(flags, reverse=(flag == M.CLAMPED_MAX))                # ... and is crossed once
    assert L.cfl_dt_host(_p(), D, F(0.0)) == (float(F(DT_MAX)), M.CLAMPED_MAX)        # zero speed: no division
    assert L.cfl_dt_host(_p(), D, F(9.0)) == (float(F(LIM / 3.0)), 0)                 # 3 m/s: 4e-4, the step the small GPU shapes start with
    assert float(F(LIM / 3.0)) == float(F(4e-4))


def test_landing_sequences_reach_the_target():
    rng = np.random.default_rng(11)
    for t_end in (5.3 * 4e-4, 1.0 * 4e-4, 0.01):
        v2s = np.exp(rng.uniform(np.log(4.0), np.log(1e4), 4000)).astype(F)
        t, k = 0.0, 0
        while not M.reached(t, t_end, DT_MAX):
            dt, _ = L.cfl_dt_host(_p(), D, v2s[k], t_end - t)
            assert dt == M.rule(*PARAMS, D, v2s[k], t_end - t)[0] and dt <= float(F(DT_MAX))
            t, k = t + dt, k + 1
            assert k < 4000
        assert abs(t_end - t) <= 2.0 ** -20 * DT_MAX and abs(t_end - t) <= 2.0 ** -24 * DT_MAX * 1.0000001, (t_end, t)
    dts, t = M.advance(*PARAMS, D, lambda k: F(9.0), 0.0, 5.3 * 4e-4)
    assert len(dts) == 6 and abs(5.3 * 4e-4 - t) <= 2.0 ** -20 * DT_MAX


def test_rule_refusals():
    for v2 in (F(np.nan), F(np.inf), F(-1.0)):
        with pytest.raises(L.SphError, match="non-finite velocity") as e:
            L.cfl_dt_host(_p(), D, v2)
        assert e.value.code == L.ERR_INVALID
    for bad, word in ((_p(factor=0.0), "factor"), (_p(factor=float("nan")), "factor"), (_p(dt_min=0.0), "min_dt"), (_p(dt_max=float("inf")), "max_dt"),
                      (_p(dt_min=-1.0), "min_dt"), (_p(dt_min=7e-4), "min_dt .* > max_dt"), (L.cfl_params(2, 0.5, 1e-5, 1e-4), "method 2"),
                      (L.cfl_params(0, 0.5, 1e-5, 1e-4), "method 0")):
        with pytest.raises(L.SphError, match=word):
            L.cfl_dt_host(bad, D, F(1.0))
    with pytest.raises(L.SphError, match="diameter"):
        L.cfl_dt_host(_p(), 0.0, F(1.0))


# ------------------------------------------------------------------------------------------- the reduce's arithmetic and selection
def particles(seed=3, n=400):
    """Velocities with negative components, every material / dynamic / ghost / removed combination, the fastest particle of each kind
    faster than every particle of the kinds in front of it: a wrong selection changes the maximum."""
    rng = np.random.default_rng(seed)
    vel = rng.uniform(-2.0, 2.0, (n, 3)).astype(F)
    material = rng.choice([M.MAT_FLUID, M.MAT_RIGID], n).astype(np.int32)
    dynamic = rng.integers(0, 2, n).astype(np.int32)
    ghost = (rng.random(n) < 0.1).astype(np.int32)
    removed = (rng.random(n) < 0.1).astype(np.int32)
    return vel, material, dynamic, ghost, removed


def _host(vel, material, dynamic, ghost=None, removed=None):
    return L.cfl_speed2_host(vel, L.cfl_meta(material, dynamic, ghost, removed))


def _same(a, b):
    return F(a[0]).tobytes() == F(b[0]).tobytes() and a[1] == b[1]


def test_speed_equals_the_model():
    vel, material, dynamic, ghost, removed = particles()
    assert _same(_host(vel, material, dynamic, ghost, removed), M.vmax2(vel, material, dynamic, ghost, removed))
    assert _same(_host(vel, material, dynamic), M.vmax2(vel, material, dynamic))
    # who counts: each kind in turn holds the fastest particle
    kinds = {"fluid": (M.MAT_FLUID, 0, 0, 0, True), "dynamic rigid": (M.MAT_RIGID, 1, 0, 0, True), "static rigid": (M.MAT_RIGID, 0, 0, 0, False),
             "ghost fluid": (M.MAT_FLUID, 0, 1, 0, False), "ghost rigid": (M.MAT_RIGID, 1, 1, 0, False), "removed": (M.MAT_FLUID, 0, 0, 1, False),
             "removed rigid": (M.MAT_RIGID, 1, 0, 1, False)}
    base = _host(vel, material, dynamic, ghost, removed)
    for name, (mat, dyn, gh, rm, counts) in kinds.items():
        v, m, d, g, r = vel.copy(), material.copy(), dynamic.copy(), ghost.copy(), removed.copy()
        v[17], m[17], d[17], g[17], r[17] = (-1e3, 5e2, -7e2), mat, dyn, gh, rm
        got = _host(v, m, d, g, r)
        assert _same(got, M.vmax2(v, m, d, g, r)), name
        assert (got[0] == M.speed2(v[17:18])[0]) == counts and (counts or got[0] <= base[0]), name
    # one value per float32 rounding: the sum (x x + y y) + z z is not x x + (y y + z z)
    rng = np.random.default_rng(9)
    for _ in range(200):
        v = rng.uniform(-3.0, 3.0, (1, 3)).astype(F)
        got = _host(v, [M.MAT_FLUID], [0])
        assert got[0].tobytes() == M.speed2(v)[0].tobytes()
    assert _same(_host(np.zeros((5, 3), F), [1] * 5, [0] * 5), (F(0.0), False))
    assert _same(_host(np.zeros((0, 3), F), [], []), (F(0.0), False))
    assert _same(_host(-np.ones((2, 3), F), [1, 2], [0, 0]), (F(3.0), False))


def test_speed_non_finite():
    vel, material, dynamic, _, _ = particles()
    material[:] = M.MAT_FLUID
    for bad in (np.nan, np.inf, -np.inf, 3e19):   # (3e19 squared overflows float32)
        v = vel.copy()
        v[123, 1] = bad
        got = _host(v, material, dynamic)
        assert got[1] and _same(got, M.vmax2(v, material, dynamic)) and got[0] == M.vmax2(np.delete(v, 123, 0), material[1:], dynamic[1:])[0]
        m = material.copy(); m[123] = M.MAT_RIGID; d = dynamic.copy(); d[123] = 0   # ... on a particle that does not count: no flag
        assert not _host(v, m, d)[1]


def test_every_mutant_fails_a_check():
    """Each wrong variant of the model disagrees with the library on at least one of this file's cases."""
    vel, material, dynamic, ghost, removed = particles()
    fast = vel.copy(); fast[5] = (40.0, -30.0, 20.0)
    for mutant in M.MUTANTS:
        differs = False
        for v2 in speeds():
            for rem in landings(v2):
                differs |= L.cfl_dt_host(_p(), D, v2, float("nan") if rem is None else rem) != M.rule(*PARAMS, D, v2, rem, mutant=mutant)
        for v in (vel, fast):
            for mat, dyn in ((M.MAT_RIGID, 0), (M.MAT_RIGID, 1), (M.MAT_FLUID, 0)):
                m, d = material.copy(), dynamic.copy()
                m[5], d[5] = mat, dyn
                differs |= not _same(_host(v, m, d, ghost, removed), M.vmax2(v, m, d, ghost, removed, mutant=mutant))
        assert differs, mutant


# ------------------------------------------------------------------------------------------- the scene parser
def _cfg(method="wcsph", **keys):
    cfg = P.dam_break_scene(method=method, domain_end=(0.6, 0.6, 0.6), start=(0.08, 0.08, 0.08), end=(0.16, 0.16, 0.16), translation=(0, 0, 0), dt=4e-4,
                            **keys)
    return cfg


def _sc(method="wcsph", **keys):
    return SimConfig(config=_cfg(method, **keys))


def test_cfl_of_defaults_and_integers():
    assert scene.cfl_of(_sc(), "wcsph", 3)[0] == "none"
    assert scene.cfl_of(_sc(cflMethod="none"), "wcsph", 3)[0] == "none" and scene.cfl_of(_sc(cflMethod=0), "wcsph", 3)[0] == "none"
    for m in ("velocity", 1):
        assert scene.cfl_of(_sc(cflMethod=m), "dfsph", 3) == ("velocity", 0.5, 4e-4 / 64, 4e-4)
    got = scene.cfl_of(_sc(cflMethod="velocity", cflFactor=0.15, cflMinTimeStepSize=1e-5, cflMaxTimeStepSize=6e-4), "wcsph", 3)
    assert got == ("velocity", 0.15, 1e-5, 6e-4)
    # the keys pass through product.dam_break_scene's **keys into Configuration
    assert _cfg(cflMethod="velocity", cflFactor=0.3)["Configuration"]["cflFactor"] == 0.3


def test_cfl_of_refusals():
    on = dict(cflMethod="velocity")
    cases = [
        (dict(cflMethod="iterations"), "cflMethod"), (dict(cflMethod=2), "cflMethod.*2"), (dict(cflMethod=True), "cflMethod"), (dict(cflMethod=1.0), "cflMethod"),
        (dict(cflFactor=0.5), "cflFactor needs cflMethod"), (dict(cflMethod="none", cflMaxTimeStepSize=1e-3), "cflMaxTimeStepSize needs cflMethod"),
        (dict(cflMethod=0, cflMinTimeStepSize=1e-5), "cflMinTimeStepSize needs cflMethod"),
        (dict(on, cflFactor=0.0), "cflFactor"), (dict(on, cflFactor=float("nan")), "cflFactor"), (dict(on, cflFactor="0.5"), "cflFactor"),
        (dict(on, cflMinTimeStepSize=-1e-5), "cflMinTimeStepSize"), (dict(on, cflMaxTimeStepSize=float("inf")), "cflMaxTimeStepSize"),
        (dict(on, cflMaxTimeStepSize=True), "cflMaxTimeStepSize"),
        (dict(on, cflMinTimeStepSize=1e-3, cflMaxTimeStepSize=1e-4), "cflMinTimeStepSize.*exceeds cflMaxTimeStepSize"),
        (dict(on, cflMinTimeStepSize=1e-3), "cflMinTimeStepSize.*exceeds cflMaxTimeStepSize"),
        (dict(on, gravitationUpper=0.5), "gravitationUpper"),
    ]
    for keys, word in cases:
        with pytest.raises(ValueError, match=word):
            scene.cfl_of(_sc(**keys), "wcsph", 3)
    with pytest.raises(ValueError, match="cflMethod.*PBF"):
        scene.cfl_of(_sc("pbf", **on), "pbf", 3)
    with pytest.raises(ValueError, match="cflMethod.*3-D"):
        scene.cfl_of(_sc(**on), "dfsph", 2)
    for key, entry in (("Emitters", [{"objectId": 5}]), ("Outflows", [{"shape": "box", "min": [0, 0, 0], "max": [1, 1, 1]}])):
        cfg = _cfg(**on)
        cfg[key] = entry
        with pytest.raises(ValueError, match=f"{key}.*cflMethod"):
            scene.cfl_of(SimConfig(config=cfg), "wcsph", 3)
    cfg = _cfg(**on)
    cfg["RigidBodies"] = [{"objectId": 3, "motion": {"keyframes": []}}]
    with pytest.raises(ValueError, match="object 3.*motion.*cflMethod"):
        scene.cfl_of(SimConfig(config=cfg), "wcsph", 3)


def test_container_refuses_before_a_device(monkeypatch):
    from sph_project_amd.SPH import containers
    monkeypatch.setattr(L, "Engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device was opened")))
    with pytest.raises(ValueError, match="cflMethod"):
        containers.WCSPHContainer(_sc(cflMethod=2), GGUI=False)
    with pytest.raises(ValueError, match="cflMethod.*sharded"):
        containers.WCSPHContainer(_sc(cflMethod="velocity"), GGUI=False, slab=dict(rank=0, nranks=2, unique_id=b"", cuts=[0, 1, 2]))
    with pytest.raises(ValueError, match="cflMethod.*PBF"):
        containers.PBFContainer(_sc("pbf", cflMethod="velocity"), GGUI=False)


def test_abi_symbols(tmp_path):
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    for name in ("sph_set_time_step", "sph_set_cfl", "sph_get_cfl", "sph_get_time_state", "sph_set_time_target", "sph_advance_until",
                 "sph_cfl_dt_host", "sph_cfl_speed2_host"):
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS and f"int {name}(" in header, name
    assert L.PH_CFL == 34 and L.K_CFL == 37
    for text in ("SPH_PH_CFL = 34", "SPH_K_CFL = 37", "#define SPH_CFL_VELOCITY 1", "#define SPH_CFL_LANDING 4"):
        assert text in header, text
    assert lib.sph_kernel_name(37) == b"?" and lib.sph_kernel_name(29) == b"pbfc_delta"
    assert (L.CFL_CLAMPED_MAX, L.CFL_CLAMPED_MIN, L.CFL_LANDING) == (M.CLAMPED_MAX, M.CLAMPED_MIN, M.LANDING)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sph_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(SphCflParams), sizeof(SphTimeState), offsetof(SphCflParams, min_dt), offsetof(SphTimeState, steps)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(L.SphCflParams), C.sizeof(L.SphTimeState), L.SphCflParams.min_dt.offset, L.SphTimeState.steps.offset]


def test_driver_refuses_gpus_2_on_an_adaptive_scene(tmp_path):
    path = tmp_path / "adaptive.json"
    path.write_text(json.dumps(P.dam_break_scene(cflMethod="velocity")))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sph_project_amd", "run_simulation.py"), "--scene_file", str(path), "--gpus", "2"],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--gpus 2" in r.stderr and "cflMethod" in r.stderr, (r.returncode, r.stderr[-400:])
