"""GPU: surface tension, explicit viscosity (fluid and boundary branch), gravity, the density sum, the rigid rest volume and the
fluid -> rigid wrench of the HIP passes against the float64 model of tests/nonpressure_terms.py, term sum by term sum, with the
derived backward-error bounds of that module -- through the C-ABI only.  The scene (nonpressure_terms.scene) has two fluid masses,
compressed pairs, a shear with noise, two walls of the domain box and a dynamic cube in a notch of the block; its all-fluid twin
selects the AF passes and, with one fluid mass, the uniform-mass force pass of the fast build.  No row is left out of any
comparison: nobody meets enforce_boundary in the one step taken (asserted)."""
import numpy as np
import pytest

from sph_project_amd import _lib as L
from tests import helpers as H
from tests import nonpressure_terms as T

pytestmark = pytest.mark.gpu
U = T.U

_FIELDS = dict(x=L.F_POSITION, v=L.F_VELOCITY, rho=L.F_DENSITY, prs=L.F_PRESSURE, vol=L.F_REST_VOLUME, mass=L.F_MASS,
               mat=L.F_MATERIAL, obj=L.F_OBJECT_ID, dyn=L.F_IS_DYNAMIC)


def _engine(sc, method, fast_math):
    pd = sc["pd"]
    p = L.SphParams()
    for k in ("particle_radius", "support_radius", "V0", "padding", "g_upper", "viscosity", "viscosity_b", "density_0",
              "surface_tension", "dt", "particle_max_num", "viscosity_implicit"):
        setattr(p, k, pd[k])
    p.domain_size[:] = pd["domain_size"]; p.grid_num[:] = pd["grid_num"]; p.gravity[:] = pd["gravity"]
    p.method = L.METHOD[method]; p.device = -1; p.deterministic = 1; p.fast_math = fast_math
    eng = L.Engine(p)
    T.feed(eng, sc, oracle=False)
    eng.prepare()
    eng.get_rigid_wrench(reset=True)
    return eng


def _state(eng, extra=()):
    """per-particle state by particle id (insertion order)"""
    ids = eng.download(L.F_PARTICLE_ID)
    st = {k: H.by_id(ids, eng.download(f)) for k, f in _FIELDS.items()}
    for k, f in extra:
        st[k] = H.by_id(ids, eng.download(f))
    return st


def _wrench(eng):
    f, t = eng.get_rigid_wrench(reset=False)
    return f[:T.BODY + 1].astype(np.float64), t[:T.BODY + 1].astype(np.float64)


def _tiny_wrench(n):
    """The library sums the wrench in 64-bit fixed point: every workgroup of 256 particles of every pass rounds its six partial sums
    to 2^-32 (half a unit each; at most two passes in the calls below)."""
    return 2 * (n // 256 + 1) * 2.0 ** -33


def _report(tag, fast_math, fr):
    print("nonpressure bounds [%s, fast_math=%d]: " % (tag, fast_math) + ", ".join("%s %.3f" % kv for kv in fr.items()))


def _scene(kind, layers=None):
    """layers: the scene's twin in a domain of that many cell layers in z (tests/helpers.py with_layers)"""
    return T.scene("wcsph", rigid=kind == "rigid", masses=1 if kind == "fluid_one_mass" else 2, layers=layers)


def _phase_model(sc, st0, st1):
    """The model's terms for the phases run from st0 (densities: the product's own f32, which DFSPH and PCISPH read unclamped)."""
    return T.non_pressure_f64(st0["x"], st0["v"], st1["rho"], st1["mass"], st1["vol"], st0["mat"], st0["dyn"], st0["obj"], sc["com"],
                              sc["params"])


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("kind", ["rigid", "fluid"])
def test_dfsph_handle_volume_density_vstar_and_viscous_wrench(gpu, kind, fast_math):
    """PH_NEIGHBOR_SEARCH, PH_RIGID_VOLUME, PH_DENSITY, PH_NON_PRESSURE on a DFSPH handle: NonPressurePass<false> (rigid scene) /
    NonPressurePass<true> (twin), RigidVolumePass, DensityPass."""
    sc = _scene(kind)
    P = sc["params"]
    eng = _engine(sc, "dfsph", fast_math)
    st0 = _state(eng)
    for ph in (L.PH_NEIGHBOR_SEARCH, L.PH_RIGID_VOLUME, L.PH_DENSITY, L.PH_NON_PRESSURE):
        eng.run_phase(ph)
    st1 = _state(eng)
    wrench = _wrench(eng)
    with pytest.raises(L.SphError):   # the kept non-pressure acceleration is PCISPH's
        eng.download(L.F_NON_PRESSURE_ACCEL)
    eng.close()
    np.testing.assert_array_equal(st1["x"], st0["x"])
    fl, rg = st0["mat"] == 1, st0["mat"] == 2
    fr = {}
    if kind == "rigid":
        V, Vb, _ = T.rigid_volume_f64(st0["x"], st0["mat"], st0["obj"], P["h"])
        assert rg.sum() > 1000
        err = np.abs(st1["vol"].astype(np.float64) - V)[rg]
        fr["rest volume"] = float((err / Vb[rg]).max())
        assert (err <= Vb[rg]).all(), fr
        assert (np.abs(st1["mass"].astype(np.float64) - P["rho0"] * V)[rg] <= P["rho0"] * (Vb[rg] + U * V[rg])).all()
    else:
        assert rg.sum() == 0
    rho, mag, mag_amp, _ = T.density_f64(st0["x"], st1["vol"], st0["mat"], P["h"], P["rho0"])
    err = np.abs(st1["rho"].astype(np.float64) - rho)[fl]
    bound = T.density_bound(mag, mag_amp)[fl]
    fr["density"] = float((err / bound).max())
    assert (err <= bound).all(), fr
    res = _phase_model(sc, st0, st1)
    T.assert_alive(res, fl, kind == "rigid")
    vs = st0["v"].astype(np.float64) + P["dt"] * res["a"]
    err = np.abs(st1["v"].astype(np.float64) - vs)[fl]
    bound = (P["dt"] * T.accel_bound(res) + 2 * U * np.abs(vs))[fl]
    fr["v*"] = float((err / bound).max())
    assert (err <= bound).all(), fr
    np.testing.assert_array_equal(st1["v"][~fl], st0["v"][~fl])
    if kind == "rigid":
        w = res["wrench"]
        for part, got in (("force", wrench[0]), ("torque", wrench[1])):
            err = np.abs(got - w[part])[T.BODY]
            wb = T.wrench_bound(w, part)[T.BODY] + _tiny_wrench(len(fl)) + U * np.abs(w[part][T.BODY])
            fr["viscous " + part] = float((err / wb).max())
            assert (err <= wb).all(), (fr, got[T.BODY], w[part][T.BODY])
    _report("DFSPH handle, %s" % kind, fast_math, fr)


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("kind", ["rigid", "fluid"])
def test_pcisph_handle_non_pressure_acceleration(gpu, kind, fast_math):
    """The acceleration itself: a PCISPH handle keeps what PH_NON_PRESSURE computed (NonPressurePass::acc_out, PCISPH.py:22) and hands
    it out as F_NON_PRESSURE_ACCEL."""
    sc = _scene(kind)
    eng = _engine(sc, "pcisph", fast_math)
    st0 = _state(eng)
    for ph in (L.PH_NEIGHBOR_SEARCH, L.PH_RIGID_VOLUME, L.PH_DENSITY, L.PH_NON_PRESSURE):
        eng.run_phase(ph)
    st1 = _state(eng, extra=[("a_np", L.F_NON_PRESSURE_ACCEL)])
    eng.close()
    fl = st0["mat"] == 1
    res = _phase_model(sc, st0, st1)
    T.assert_alive(res, fl, kind == "rigid")
    err = np.abs(st1["a_np"].astype(np.float64) - res["a"])[fl]
    bound = T.accel_bound(res)[fl]
    fr = {"acceleration": float((err / bound).max())}
    assert (err <= bound).all(), fr
    _report("PCISPH handle, %s" % kind, fast_math, fr)


def _wcsph_step(sc, fast_math):
    eng = _engine(sc, "wcsph", fast_math)
    before = _state(eng)
    eng.step(1)
    after = _state(eng)
    wrench = _wrench(eng)
    eng.close()
    return before, after, wrench


ENVS = {"default": None, "no_uniform_mass": "SPH_NO_UNIFORM_MASS", "count_own": "SPH_FORCES_COUNT_OWN"}


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("kind", ["rigid", "fluid", "fluid_one_mass"])
def test_wcsph_whole_step_velocity_and_wrench(gpu, monkeypatch, kind, env, fast_math):
    """One engine step from the downloaded x0, v0: v1 against v0 + dt (a_np + a_p) with a_p from the product's own (clamped) density
    and pressure, and the whole wrench -- WcsphForcePass<false> (rigid scene), <true> (two-mass twin), <true, true> (one-mass twin,
    fast build), each also as the instantiation that counts its own pairs (SPH_FORCES_COUNT_OWN) and with the uniform-mass pass
    switched off (SPH_NO_UNIFORM_MASS).  The library has no counter that names the instantiation a launch took, so the choice is
    seen by its effect: the two-mass twin must reject the model with m_ij = m_i -- what the uniform-mass pass computes -- on at least
    one affected row in ten; the one-mass twin meets the pass's condition (sph_api.hip refresh_counts: all fluid, one mass) and, in
    the fast build, gives the bits of the generic pass (SPH_NO_UNIFORM_MASS), which tests/test_hip_wcsph.py states as its property."""
    for name in ENVS.values():
        if name:
            monkeypatch.delenv(name, raising=False)
    if ENVS[env]:
        monkeypatch.setenv(ENVS[env], "1")
    sc = _scene(kind)
    before, after, wrench = _wcsph_step(sc, fast_math)
    fl = before["mat"] == 1
    n_mass = len(np.unique(before["mass"][fl]))
    assert n_mass == (1 if kind == "fluid_one_mass" else 2)
    assert (kind == "rigid") == bool((~fl).any())
    fr = T.wcsph_step_check(sc, before, after, wrench, tiny_wrench=_tiny_wrench(len(fl)))
    _report("WCSPH step, %s, %s" % (kind, env), fast_math, fr)
    if kind == "fluid":
        # not the uniform-mass pass: v1 is further than twice the bound from the model whose m_ij is m_i
        P = sc["params"]
        rho64, mag, mag_amp, _ = T.density_f64(before["x"], before["vol"], before["mat"], P["h"], P["rho0"])
        args = (before["x"], before["v"], rho64, before["mass"], before["vol"], before["mat"], before["dyn"], before["obj"], sc["com"], P)
        res = T.non_pressure_f64(*args, rho_bound=T.density_bound(mag, mag_amp))
        mut = T.non_pressure_f64(*args, mutant="mij_is_mi")
        a_p, pmag, pamp = H.wcsph_pressure_accel_f64(before["x"], after["rho"], after["prs"], before["mass"], before["vol"], before["mat"],
                                                     P["h"], P["rho0"])
        v_mut = before["v"].astype(np.float64) + P["dt"] * (mut["a"] + a_p)
        bound = P["dt"] * (T.accel_bound(res) + 1e-5 * pmag + 5e-7 * pamp) + 4 * U * np.abs(v_mut)
        p = res["pairs"]
        rows = np.zeros(len(fl), bool)
        rows[p["i"][before["mass"][p["i"]] != before["mass"][p["j"]]]] = True
        far = (np.abs(after["v"].astype(np.float64) - v_mut) > 2 * bound).any(axis=1)
        assert rows.sum() >= 100 and far[rows].mean() >= 0.1, (rows.sum(), far[rows].mean())
    if kind == "fluid_one_mass" and env == "default" and fast_math:
        monkeypatch.setenv("SPH_NO_UNIFORM_MASS", "1")
        _, generic, _ = _wcsph_step(sc, fast_math)
        for k in ("x", "v", "rho", "prs"):
            np.testing.assert_array_equal(after[k], generic[k])
