"""GPU: every pass of the implicit-viscosity CG solve (csrc/sph_cg.hpp, csrc/sph_cg_steps.hpp, the l_cg_* launchers) against the float64
model of tests/implicit_viscosity_terms.py, each pass from the inputs the device itself held in front of it, with the derived bounds of
that module and no row left out: both builds x {rigid scene, all-fluid twin} x {the state behind prepare(), K_STEPS whole steps
later}, through the phases SPH_PH_CG_* (tests/implicit_viscosity_probe.py holds the sequence).  The production library runs the split
A p pass with the p update folded into the next one; the test-hook library's two switches reach the unsplit pass and the separate p
update, in child processes that select that library with SPH_HIP_LIB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sph_project_amd import _lib as L
from tests import helpers as H
from tests import implicit_viscosity_probe as PR
from tests import implicit_viscosity_terms as M
from tests import nonpressure_terms as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(tag, fr):
    print("implicit viscosity bounds [%s]: " % tag + ", ".join("%s %.3f" % kv for kv in fr.items()))


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("state", [0, 1])
@pytest.mark.parametrize("kind", ["rigid", "fluid"])
def test_every_pass_against_the_model(gpu, kind, state, fast_math):
    """The production forms: split, k_cg_ap_combine in front of the loop, parts only inside it, the p update folded into the next A p pass
    (the second A p pass is the first folded one, the second x / r update reads the other parity)."""
    check_every_pass(kind, state, fast_math)


def check_every_pass(kind, state, fast_math, layers=None):
    """layers: on the scene's twin in a domain of that many cell layers in z (tests/test_hip_tall_grid.py)"""
    assert PR.forms() == (True, True)
    fr = PR.pass_by_pass(kind, state, fast_math, layers=layers)
    assert any(k.endswith("A p (parts)") for k in fr) and "it 2 beta" in fr and "end v" in fr
    _report("split, folded p update; %s, state %d, fast_math=%d%s" % (kind, state, fast_math, ", %d layers" % layers if layers else ""), fr)


@pytest.mark.parametrize("switches", [dict(SPH_TEST_CG_SPLIT_LIMIT="0"), dict(SPH_TEST_CG_SEPARATE_P="1"),
                                      dict(SPH_TEST_CG_SPLIT_LIMIT="0", SPH_TEST_CG_SEPARATE_P="1")],
                         ids=["unsplit", "separate_p", "unsplit_separate_p"])
def test_every_pass_in_the_other_launch_forms(gpu, switches):
    """The same sequence (both builds, both scenes, both states) in a child process on the test-hook library: the unsplit A p pass with
    the folded own_p(), k_cg_update_p2 with k_cg_ap_combine inside the loop, and both."""
    check_other_launch_forms(switches)


def check_other_launch_forms(switches, probe_args=(), cases=8):
    """probe_args: arguments of tests/implicit_viscosity_probe.py (tests/test_hip_tall_grid.py: the tall twins, the fast build only)"""
    hooks = os.path.join(ROOT, "sph_project_amd", "libsph_hip_testhooks.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "implicit_viscosity_probe.py"), *probe_args],
                       env=dict(os.environ, SPH_HIP_LIB=hooks, **switches), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert got["split"] == ("SPH_TEST_CG_SPLIT_LIMIT" not in switches) and got["fused"] == ("SPH_TEST_CG_SEPARATE_P" not in switches)
    assert len(got["cases"]) == cases
    for tag, fr in got["cases"].items():
        assert max(fr.values()) <= 1, (tag, fr)
        assert ("it 1 A p (parts)" in fr) == (got["split"] and got["fused"]) and "it 2 beta" in fr
        _report("%s; %s" % ("unsplit" if not got["split"] else "split", "separate p update" if not got["fused"] else "folded") + "; " + tag, fr)


def test_prepare_pass_on_a_wcsph_handle(gpu):
    """WCSPH clamps the density only behind the non-pressure forces: its solve reads the RAW density, which a step does not keep.  The
    model computes its own float64 density and carries that density's bound through every term that divides by it
    (nonpressure_terms.wcsph_step_check does the same)."""
    sc = M.scene("wcsph", rigid=True)
    eng = PR.engine(sc, "wcsph", 0)
    for ph in PR.SORTED:
        eng.run_phase(ph)
    ids = eng.download(L.F_PARTICLE_ID)
    s0 = PR.get(eng, PR.BASE, ids)
    eng.run_phase(L.PH_CG_PREPARE)
    s1 = PR.get(eng, PR.VECTORS, ids)
    eng.close()
    P = sc["params"]
    fl = s0["mat"] == 1
    rho64, mag, mag_amp, _ = T.density_f64(s0["x"], s0["vol"], s0["mat"], P["h"], P["rho0"])
    db = np.where(fl, T.density_bound(mag, mag_amp), 0.0)
    assert int((rho64[fl] < P["rho0"]).sum()) >= 100, "rows whose raw density the clamp would have changed"
    s0["rho"] = np.where(fl, rho64, 1.0)
    fr = {}
    M.check_prepare(sc, s0, s1, fr, rho_bound=db)
    M.check_guess(s0, s1)
    M.check_ap(sc, s0, s1["x"], s1["X"], s1["Ap"].astype(np.float64), fr, "first A p", rho_bound=db)
    r0, rb = M.r0_f64(s1["X"], s1["b"], s1["Ap"])
    fr["r0"] = M._frac(np.abs(s1["r"] - r0)[fl], rb[fl])
    _report("prepare on a WCSPH handle (raw density)", fr)
    assert max(fr.values()) <= 1, fr
    # the clamped density the handle holds would not do: the bounds see it
    s0["rho"] = np.where(fl, np.maximum(rho64, P["rho0"]), 1.0)
    bad = {}
    M.check_prepare(sc, s0, s1, bad, rho_bound=db)
    assert bad["|D X - I|"] > 2, bad


_CG_PHASES = (L.PH_CG_PREPARE,) + (L.PH_CG_AP, L.PH_CG_UPDATE_XR, L.PH_CG_UPDATE_P) * M.FIXED_ITERATIONS + (L.PH_CG_END,)


def _all(eng):
    ids = eng.download(L.F_PARTICLE_ID)
    out = {k: H.by_id(ids, eng.download(f)) for k, f in dict(cg_x=L.F_CG_X, v=L.F_VELOCITY, x=L.F_POSITION, mat=L.F_MATERIAL).items()}
    out["cg_x by slot"] = eng.download(L.F_CG_X)
    return out


def _same(a, b, what, keys=("cg_x", "v", "x")):
    """fluid rows only: the other rows' solver vectors are never written"""
    fl = a["mat"] == 1
    for k in keys:
        np.testing.assert_array_equal(a[k][fl], b[k][fl], err_msg="%s: %s" % (what, k))


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("kind", ["rigid", "fluid"])
def test_whole_step_is_the_phase_sequence(gpu, kind, fast_math):
    """fixed_iterations = 2, the second state (warm start, exchanged slots).  On the DFSPH handle the solve is the first thing a step
    does and the step has no phase for its position update: SPH_PH_NON_PRESSURE -- implicit_viscosity_non_pressure as the step calls it
    -- against the phase sequence in cg_x and velocity, and a whole step(1) in cg_x (which nothing behind the solve touches).  On a WCSPH
    handle every pass of the step is a phase: step(1) against the sort, the density, the CG phases and SPH_PH_PRESSURE_INTEGRATE in
    cg_x, velocity AND position."""
    rigid = kind == "rigid"
    sc = M.scene("dfsph", rigid=rigid)
    a = PR.engine(sc, "dfsph", fast_math, steps=M.K_STEPS)
    a.run_phase(L.PH_NON_PRESSURE)
    solve = _all(a)
    assert a.stats()["iter_cg"] == M.FIXED_ITERATIONS
    a.close()
    b = PR.engine(sc, "dfsph", fast_math, steps=M.K_STEPS)
    for ph in _CG_PHASES:
        b.run_phase(ph)
    by_phases = _all(b)
    b.close()
    _same(solve, by_phases, "DFSPH: SPH_PH_NON_PRESSURE against the CG phases")
    c = PR.engine(sc, "dfsph", fast_math, steps=M.K_STEPS)
    c.step(1)
    whole = _all(c)
    c.close()
    # (the sort at the end of the step moves the particles to other slots and leaves cg_x where it is: the guess is slot-indexed,
    #  base_container.py:506 does not reorder it -- so it is compared slot by slot, every slot)
    assert not np.array_equal(whole["x"], solve["x"])
    np.testing.assert_array_equal(whole["cg_x by slot"], by_phases["cg_x by slot"], err_msg="DFSPH: step(1) against the CG phases: cg_x")
    sc = M.scene("wcsph", rigid=rigid)
    d = PR.engine(sc, "wcsph", fast_math, steps=M.K_STEPS)
    d.step(1)
    whole = _all(d)
    assert d.stats()["iter_cg"] == M.FIXED_ITERATIONS
    d.close()
    e = PR.engine(sc, "wcsph", fast_math, steps=M.K_STEPS)
    for ph in PR.SORTED + _CG_PHASES + (L.PH_PRESSURE_INTEGRATE,):
        e.run_phase(ph)
    by_phases = _all(e)
    e.close()
    _same(whole, by_phases, "WCSPH: step(1) against its phases")
    assert np.abs(whole["cg_x"][whole["mat"] == 1]).max() > 0


@pytest.mark.parametrize("fast_math", [0, 1])
def test_scalars_above_65536_rows(gpu, fast_math):
    """An all-fluid 41^3 lattice: 270 workgroups of partial sums, the smallest size at which cg_total's `k += 256` loop makes a second
    trip.  alpha, beta and error of two iterations against float64 sums of the downloaded vectors; no pair model."""
    cfg = H.dam_break_scene(method="dfsph", domain_end=(1.2, 1.2, 1.2), start=(0.0, 0.0, 0.0), end=(0.81, 0.81, 0.81),
                            viscosity_method="implicit", viscosity=M.MU)
    container, solver = H.build_product(cfg, jitter=0.003, seed=3, fast_math=fast_math, fixed_iterations=M.FIXED_ITERATIONS)
    solver.prepare()
    eng = container.engine
    n = eng.particle_num
    assert n == 41 ** 3 and n > 65536 and -(-n // 256) > 256
    ids = eng.download(L.F_PARTICLE_ID)
    x = eng.download(L.F_POSITION)
    rng = np.random.default_rng(5)
    v = rng.uniform(-0.5, 0.5, x.shape).astype(np.float32)
    v[:, 0] += 3.0 * x[:, 1]
    eng.upload(L.F_VELOCITY, v)
    fr = PR.scalars_only(eng, np.ones(n, bool), dict(dt=float(np.float32(4e-4)), rho0=1000.0))
    assert set(fr) == {"it %d %s" % (k, s) for k in (1, 2) for s in ("alpha", "beta", "error")}
    _report("scalars, 41^3 rows, fast_math=%d" % fast_math, fr)
    assert max(fr.values()) <= 1, fr
    assert eng.cg_scalars()[0] > 0 and eng.cg_scalars()[2] > 0
