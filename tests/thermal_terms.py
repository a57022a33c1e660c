"""Heat (Cleary and Monaghan 1999 with constant conductivity, Boussinesq buoyancy) restated in float64 over a KD-tree
pair list -- written from the formulas, independent of the device code -- with backward-error bounds in the style of
tests/micropolar_terms.py, the mutants that every comparison has to catch, and the scenes of tests/surface_tension_terms.py with a
temperature per fluid particle.

For an active fluid particle i, j over fluid and k over boundary (non-fluid) neighbours within h, R = x_i - x, gradW = gradW(R),
F = (R . gradW) / (|R|^2 + 0.01 h^2) <= 0:
    dT_i/dt = 2 alpha (rho0 / rho_i) [ sum_j (m_j / rho_j) (T_i - T_j) F_ij + sum_k c_k (T_i - T_k) F_ik ]
              c_k = V_k where the object of k is held at a temperature T_k, 0 otherwise (adiabatic)
    T_i <- T_i + dt dT_i/dt   (Jacobi)
    a_b_i = -beta (T_i - T_ref) g   (the T of the previous step)
rho is the density the viscous term of the method reads (WCSPH: the raw density, before the clamp of the equation of state).

Bounds.  |got - model| <= C1 sum|term| + C2 sum|term| amp, for ANY f32 evaluation of the sum in any order; C1 = 1e-5 and C2 = 5e-7
are nonpressure_terms'.  Roundings of one pair term in the longest form, the strict HeatPass::pair() (heat_pair<false> of
csrc/sph_thermal.hpp) with kernGrad() and geom() of csrc/sph_device.hpp:
  x_i - x_j per component 1; r^2 3; rn = sqrt 1 (5 of the geometry); the gradient: q = rn / h 1, the polynomial 4, its constant 1,
  1 / (rn h) 2, x dx 1 (9); R . gradW: three products of one sign and two additions 3; r^2 + eps 1 (+ 1 of the constant); the
  quotient 1; c_j = m_j / rho_j 1; T_i - T_j 1 (relative to the difference: the inputs are f32); x c_j 1; x F 1: 25.  Behind the
  sum: rho0 / rho_i 1, the constant 2 alpha 1, their product 1, x sum 1 (4); the update: x dt 1, + T 1 (carried by the 2 u term).
The fast form takes R . gradW = gs r^2 (fewer operations) through v_rsq / v_rcp worth 1-2 ulp each: + 4.  Every pair adds ONE term,
so with at most N_MAX = 100 neighbours per row (a condition, asserted from the pair list): (29 + 4 + 100 + 3) u = 8.1e-6 <= C1.
C2 carries the conditioning of gradW in q = r / h, as in nonpressure_terms; r^2 / (r^2 + eps) has a condition below 2 eps /
(r^2 + eps) <= 2 in r, which the same 2.5 u of the geometry reach: 5 u sum|term|, inside what C1 leaves (1e-5 - 8.1e-6 = 32 u).
The update T + dt rate adds 2 u (|T| + |T_new|).  The buoyancy: T_ref to f32 (u |T_ref| absolute), T - T_ref 1, -beta to f32 1, the
product 1, g 1, the product 1: 5 u |a_b| + u |beta g| |T_ref| (1.01 for the second order)."""
import numpy as np

from tests.helpers import _pair_list
from tests import nonpressure_terms as T
from tests import surface_tension_terms as A
from tests import micropolar_terms as M

U, C1, C2, N_MAX = T.U, T.C1, T.C2, T.N_MAX
BODY, PLATE = A.BODY, A.PLATE
T_REF, T_LO, T_HI, T_WALL = 15.0, 0.0, 60.0, 80.0   # the fluid's random temperatures lie in [T_LO, T_HI]; the plate is held at T_WALL

MUTANTS = ("laplacian_sign", "no_factor_2", "rho_j_for_rho_i", "rho0_over_rho_dropped", "no_eps", "w_for_f", "rho0vk_for_vk",
           "adiabatic_conducts", "heated_wall_skipped", "wall_heated_by_fluid", "gauss_seidel", "rho_for_rho_raw", "buoyancy_sign",
           "t_ref_dropped", "buoyancy_updated_t", "drop_neighbour")
# mutants that need a boundary to differ at all
RIGID_MUTANTS = ("rho0vk_for_vk", "adiabatic_conducts", "heated_wall_skipped", "wall_heated_by_fluid")


def big_f(r, h, mutant=None):
    """(F, |F| amp): F = (R . gradW) / (r^2 + 0.01 h^2) = s r^2 / (r^2 + eps)."""
    s, s_amp = T.kernel_grad_scale(r, h)
    eps = 0.0 if mutant == "no_eps" else 0.01 * h * h
    den = np.where(r * r + eps > 0, r * r + eps, 1.0)
    if mutant == "w_for_f":
        W, W_amp = T.kernel_w(r, h)
        return W, W_amp
    return s * r * r / den, s_amp * r * r / den


def thermal_f64(x, temp, rho, mass, vol, mat, obj, wall_t, params, alpha, beta, t_ref, mutant=None, rho_alt=None):
    """dict(rate, rate_bound, mag, T_new, T_bound, a_b, a_b_bound, n_terms, pairs).  temp: a temperature per row (fluid rows count);
    wall_t: {object id: temperature} of the bodies held at one (every other body is adiabatic); rho_alt: the other density (mutant
    rho_for_rho_raw reads it).  rate = dT/dt on fluid rows, zero elsewhere; T_new = T + dt rate; a_b = -beta (T - T_ref) g."""
    x, temp = x.astype(np.float64), np.asarray(temp, np.float64)
    n = len(x)
    h, rho0, dt = params["h"], params["rho0"], params["dt"]
    g = np.asarray(params["g"], np.float64)
    rho = np.asarray(rho_alt if mutant == "rho_for_rho_raw" else rho, np.float64)
    m, vl = mass.astype(np.float64), vol.astype(np.float64)
    _, i, j = _pair_list(x, h)
    R = x[i] - x[j]
    r = np.linalg.norm(R, axis=1)
    keep = (mat[i] == 1) & (r <= h) & ((mat[j] == 1) | (mat[j] == 2))
    if mutant == "drop_neighbour":
        keep = T._drop_first(i, keep)
    i, j, R, r = i[keep], j[keep], R[keep], r[keep]
    fl = mat[j] == 1
    has = np.array([int(o) in wall_t for o in obj[j]], dtype=bool) & ~fl
    t_wall = np.array([wall_t.get(int(o), 0.0) for o in obj[j]], dtype=np.float64)
    F, F_amp = big_f(r, h, mutant)
    c = np.where(fl, m[j] / rho[j], np.where(has, vl[j], 0.0))
    if mutant == "rho0vk_for_vk":
        c = np.where(fl, c, rho0 * c)
    if mutant == "adiabatic_conducts":
        c = np.where(fl | has, c, vl[j])
        t_wall = np.where(has, t_wall, t_ref)
    if mutant == "heated_wall_skipped":
        c = np.where(fl, c, 0.0)
    lead = np.full(len(i), 2.0 * alpha)
    if mutant == "no_factor_2":
        lead = lead / 2
    if mutant != "rho0_over_rho_dropped":
        lead = lead * rho0 / np.where(fl & (mutant == "rho_j_for_rho_i"), rho[j], rho[i])
    if mutant == "laplacian_sign":
        lead = -lead

    def rates(tv):
        tj = np.where(fl, tv[j], t_wall)
        if mutant == "wall_heated_by_fluid":   # the wall's temperature follows the fluid particle it touches half way
            tj = np.where(has, t_wall + 0.5 * (tv[i] - t_wall), tj)
        term = lead * c * (tv[i] - tj) * F
        amp = np.abs(lead * c * (tv[i] - tj)) * F_amp
        return term, amp

    fluid = mat == 1
    term, amp = rates(temp)
    rate = np.where(fluid, T._sum(i, n, term), 0.0)
    mag = np.where(fluid, T._sum(i, n, np.abs(term)), 0.0)
    rate_bound = C1 * mag + C2 * np.where(fluid, T._sum(i, n, amp), 0.0)
    t_new = np.where(fluid, temp + dt * rate, temp)
    if mutant == "gauss_seidel":   # rows with a lower index have been updated when row i is summed
        tv = np.where(fluid, t_new, temp)
        tj = np.where(fl, np.where(j < i, tv[j], temp[j]), t_wall)
        rate = np.where(fluid, T._sum(i, n, lead * c * (temp[i] - tj) * F), 0.0)
        t_new = np.where(fluid, temp + dt * rate, temp)
    t_bound = np.where(fluid, dt * rate_bound + 2 * U * (np.abs(temp) + np.abs(t_new)), 0.0)
    tb = t_new if mutant == "buoyancy_updated_t" else temp
    kb = beta if mutant == "buoyancy_sign" else -beta
    a_b = np.where(fluid[:, None], (kb * (tb - (0.0 if mutant == "t_ref_dropped" else t_ref)))[:, None] * g[None, :], 0.0)
    a_b_bound = 5 * U * np.abs(a_b) + 1.01 * U * np.abs(beta * t_ref) * np.abs(g)[None, :]
    return dict(rate=rate, rate_bound=rate_bound, mag=mag, T_new=t_new, T_bound=t_bound, a_b=a_b, a_b_bound=a_b_bound,
                n_terms=np.bincount(i, minlength=n), pairs=dict(i=i, j=j, R=R, r=r, fluid_j=fl, wall_j=has, c=c, F=F))


def assert_alive(res, temp, fl, rigid):
    """A scene change must not hollow the checks out."""
    p = res["pairs"]
    assert res["n_terms"].max() <= N_MAX, "more summed terms in a row than the derivation of C1 allows"
    assert np.abs(res["rate"][fl]).max() > 100.0, "dT/dt, K / s"
    assert np.abs(res["T_new"] - temp)[fl].max() > 0.05, "the update, K"
    assert np.abs(res["a_b"][fl]).max() > 0.1, "a_b, m / s^2"
    if rigid:
        assert int(p["wall_j"].sum()) > 300 and int((~p["fluid_j"] & ~p["wall_j"]).sum()) > 30, "pairs with the heated plate / the adiabatic cube"


# ---------------------------------------------------------------------------------------------------------------------------
# The scenes: those of surface_tension_terms.scene, with a temperature per fluid particle drawn uniformly from a fixed seed; the plate is
# held at T_WALL, the dynamic cube is adiabatic.
KINDS = ("rigid", "fluid", "lattice", "lattice_fluid")
WALLS = {PLATE: T_WALL}


def scene(method, kind="rigid", **kw):
    return A.scene(method, kind, **kw)


def temperatures(sc, seed=29):
    """(n,) float32 in insertion order, uniform in [T_LO, T_HI]; T_REF on non-fluid rows (never read)."""
    mat = np.concatenate([np.asarray(b["material"]) for b in sc["batches"]])
    rng = np.random.default_rng(seed)
    t = rng.uniform(T_LO, T_HI, len(mat))
    return np.where(mat == 1, t, T_REF).astype(np.float32)


host_state = A.host_state


def lattice_sum(h, d):
    """S = sum over the interior rest lattice (spacing d, V = d^3) of V |F|, float64."""
    k = int(np.ceil(h / d)) + 1
    ax = d * np.arange(-k, k + 1)
    R = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    r = np.linalg.norm(R, axis=1)
    r = r[(r > 0) & (r <= h * (1 + 1e-12))]
    F, _ = big_f(r, h)
    return float((d ** 3 * np.abs(F)).sum())


def dt_limit(alpha, h, d):
    """0.5 / (2 alpha 1.25 S): the step below which the explicit update is a convex combination with a margin of two (1.25: the rest
    lattice's rho0 / rho_raw under WCSPH)."""
    return np.inf if alpha == 0 else 0.5 / (2.0 * alpha * 1.25 * lattice_sum(h, d))


rest_lattice = M.rest_lattice
