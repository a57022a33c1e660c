"""The micropolar vorticity model (Bender, Koschier, Kugelstadt, Weiler 2017) restated in float64 over a KD-tree pair
list -- written from the formulas, independent of the device code -- with backward-error bounds in the style of
tests/nonpressure_terms.py, the mutants that every comparison has to catch, and the scenes of tests/surface_tension_terms.py with an
angular velocity per fluid particle.

For an active fluid particle i, j over fluid and k over boundary (non-fluid) neighbours within h, R = x_i - x, gradW = gradW(R):
    a_mp_i  = nu_t / rho_i [ sum_j m_j (w_i - w_j) x gradW_ij + sum_k Psi_k w_i x gradW_ik ],          Psi_k = rho0 V_k
    alpha_i = theta_inv { nu_t / rho_i [ sum_j m_j (v_i - v_j) x gradW_ij + sum_k Psi_k (v_i - v_k) x gradW_ik ]
                          - 2 nu_t w_i - zeta sum_j (m_j / rho_j) (w_i - w_j) W_ij }
    w_i <- w_i + dt alpha_i   (Jacobi)
    body of a dynamic k:  force += -m_i nu_t / rho_i Psi_k w_i x gradW_ik  at x_k,  torque += (x_k - com) x force
rho is the density the viscous term of the method reads (WCSPH: the raw density, before the clamp of the equation of state).

Bounds.  |got - model| <= C1 sum|term| + C2 sum|term| amp, for ANY f32 evaluation of the sums in any order; C1 = 1e-5 and
C2 = 5e-7 are nonpressure_terms'.  Roundings of one pair term in the longest form, the curl term of alpha in the strict
MicropolarPass::pair() (mp_pair<false> of csrc/sph_micropolar.hpp) with kernGrad() and geom() of csrc/sph_device.hpp:
  x_i - x_j per component 1; r^2 3; rn = sqrt 1 (5 of the geometry); the gradient: q = rn / h 1, the polynomial 4, its constant 1,
  1 / (rn h) 2, x dx 1 (9); v_i - v_j 1; the cross product: two products and their difference, relative to the sum of the two
  magnitudes (which is what the magnitudes below carry), 2; c1 = nu_t / rho_i 1 (+ 1 of the constant nu_t); c1 m_j 1; x the cross
  product 1; the dissipation term that leaves the same accumulator in the same statement: its own product chain is shorter (w_i - w_j
  1, m_j / rho_j 1, zeta x 1 + 1, W: 5 + 6, x 1, x 1 = 18 < 21) and its subtraction is one more addition of the row; behind the sum:
  2 nu_t 1, x w_i 1, the difference 1, x theta_inv 1, x dt 1, + w_i 1 (6).
That is 21 + 6 = 27 (the fast form takes the cross products with R and applies the scalars m_j gs, c1 m_j gs once: fewer operations,
v_rsq / v_rcp worth 1-2 ulp each: + 4).  Every pair adds TWO terms to the accumulator of alpha (curl and dissipation), so with at
most N_MAX / 2 = 50 neighbours per row (a condition, asserted from the pair list): (31 + 100 + 3) u = 8.0e-6 <= C1.  The terms of a_mp
(14 + 1 + 2 + 1 per term, c1 x behind the sum) are shorter.  C2 carries the conditioning of gradW (the cross-product terms) and of W
(the dissipation term) in q = r / h, as in nonpressure_terms.  The update w + dt alpha adds 2 u (|w| + |w_new|)."""
import numpy as np

from tests.helpers import _pair_list
from tests import nonpressure_terms as T
from tests import surface_tension_terms as A

U, C1, C2, N_MAX = T.U, T.C1, T.C2, T.N_MAX
BODY, PLATE = A.BODY, A.PLATE
W_MAX = 20.0   # |w| <= 20 / s

MUTANTS = ("curl_sign", "w_sum", "rho_j_for_rho_i", "no_2nu_w", "theta_inv_dropped", "dissipation_gradw", "dissipation_on_boundary",
           "boundary_skipped", "vk_for_psik", "reaction_sign", "reaction_arm_xi", "updated_velocity", "gauss_seidel",
           "rho_for_rho_raw", "drop_neighbour")
# mutants that need a boundary / a dynamic body to differ at all
RIGID_MUTANTS = ("dissipation_on_boundary", "boundary_skipped", "vk_for_psik", "reaction_sign", "reaction_arm_xi")


def _cross(a, b):
    return np.cross(a, b)


def micropolar_f64(x, v, w, rho, mass, vol, mat, is_dynamic, obj, com, params, nu_t, zeta, theta_inv, mutant=None, rho_alt=None,
                   v_new=None):
    """dict(a, a_bound, w_new, w_bound, alpha, curl, a_mag, n_terms, pairs, wrench).  a = a_mp, w_new = w + dt alpha on fluid rows
    (zero / w elsewhere); curl: nu_t-free bracket 1 / rho_i [ sum m (v_i - v_j) x gradW ] (the estimate of curl v).  rho_alt: the
    other density (mutant rho_for_rho_raw reads it); v_new: the velocities behind the non-pressure update (mutant updated_velocity
    reads them).  wrench: per body, in the form of nonpressure_terms._body_sums."""
    x, v, w = x.astype(np.float64), np.asarray(v, np.float64), np.asarray(w, np.float64)
    n = len(x)
    h, rho0, dt = params["h"], params["rho0"], params["dt"]
    rho = np.asarray(rho_alt if mutant == "rho_for_rho_raw" else rho, np.float64)
    m, vl = mass.astype(np.float64), vol.astype(np.float64)
    if mutant == "updated_velocity":
        v = np.asarray(v_new, np.float64)
    _, i, j = _pair_list(x, h)
    R = x[i] - x[j]
    r = np.linalg.norm(R, axis=1)
    keep = (mat[i] == 1) & (r <= h) & ((mat[j] == 1) | (mat[j] == 2))
    if mutant == "drop_neighbour":
        keep = T._drop_first(i, keep)
    i, j, R, r = i[keep], j[keep], R[keep], r[keep]
    fl = mat[j] == 1
    aR = np.abs(R)
    s, s_amp = T.kernel_grad_scale(r, h)
    W, W_amp = T.kernel_w(r, h)
    g = s[:, None] * R
    m_nb = np.where(fl, m[j], (vl[j] if mutant == "vk_for_psik" else rho0 * vl[j]))
    if mutant == "boundary_skipped":
        m_nb = np.where(fl, m_nb, 0.0)
    c1 = nu_t / rho[j if mutant == "rho_j_for_rho_i" else i]
    c1 = np.where(fl, c1, nu_t / rho[i])

    def sums(wv):
        wj = np.where(fl[:, None], wv[j], 0.0)
        dw = wv[i] + wj if mutant == "w_sum" else wv[i] - wj
        adw = np.abs(dw)
        tA = (c1 * m_nb)[:, None] * _cross(dw, g)
        tA_mag = (c1 * m_nb * np.abs(s))[:, None] * T._cross_mag(adw, aR)
        tA_amp = (c1 * m_nb * s_amp)[:, None] * T._cross_mag(adw, aR)
        dv = v[i] - v[j]
        sign = -1.0 if mutant == "curl_sign" else 1.0
        tC = sign * (c1 * m_nb)[:, None] * _cross(dv, g)
        tC_mag = (c1 * m_nb * np.abs(s))[:, None] * T._cross_mag(np.abs(dv), aR)
        tC_amp = (c1 * m_nb * s_amp)[:, None] * T._cross_mag(np.abs(dv), aR)
        volj = np.where(fl, m[j] / rho[j], (vl[j] if mutant == "dissipation_on_boundary" else 0.0))
        kern, kern_amp = (np.abs(s) * r, s_amp * r) if mutant == "dissipation_gradw" else (W, W_amp)
        tD = (zeta * volj * kern)[:, None] * dw
        tD_amp = (zeta * volj * kern_amp)[:, None] * adw
        return dict(tA=tA, tA_mag=tA_mag, tA_amp=tA_amp, tC=tC, tC_mag=tC_mag, tC_amp=tC_amp, tD=tD, tD_amp=tD_amp, dw=dw)

    def update(wv, q):
        two_nu = 0.0 if mutant == "no_2nu_w" else 2.0 * nu_t
        th = 1.0 if mutant == "theta_inv_dropped" else theta_inv
        braces = T._sum(i, n, q["tC"]) - two_nu * wv - T._sum(i, n, q["tD"])
        mag = T._sum(i, n, q["tC_mag"] + np.abs(q["tD"])) + two_nu * np.abs(wv)
        amp = T._sum(i, n, q["tC_amp"] + q["tD_amp"])
        alpha = th * braces
        return alpha, th * (C1 * mag + C2 * amp)

    q = sums(w)
    fluid = (mat == 1)[:, None]
    a = np.where(fluid, T._sum(i, n, q["tA"]), 0.0)
    a_mag = np.where(fluid, T._sum(i, n, q["tA_mag"]), 0.0)
    a_bound = C1 * a_mag + C2 * np.where(fluid, T._sum(i, n, q["tA_amp"]), 0.0)
    alpha, alpha_bound = update(w, q)
    w_new = np.where(fluid, w + dt * alpha, w)
    if mutant == "gauss_seidel":   # rows with a lower index have been updated when row i is summed
        wj_gs = np.where((j < i)[:, None] & fl[:, None], w_new[j], np.where(fl[:, None], w[j], 0.0))
        dw = w[i] - wj_gs
        q2 = dict(q)
        q2["tD"] = (zeta * np.where(fl, m[j] / rho[j], 0.0) * W)[:, None] * dw
        alpha, alpha_bound = update(w, q2)
        w_new = np.where(fluid, w + dt * alpha, w)
        a = np.where(fluid, T._sum(i, n, (c1 * m_nb)[:, None] * _cross(dw, g)), 0.0)
    w_bound = np.where(fluid, dt * alpha_bound + 2 * U * (np.abs(w) + np.abs(w_new)), 0.0)
    curl = np.where(fluid, T._sum(i, n, (m_nb / rho[i])[:, None] * _cross(v[i] - v[j], g)), 0.0)
    # ---- reaction on dynamic bodies: -m_i x the pair's share of a_mp
    dyn = ~fl & (mat[j] == 2) & (is_dynamic[j] != 0)
    di, dj = i[dyn], j[dyn]
    sign = 1.0 if mutant == "reaction_sign" else -1.0
    f = sign * m[di][:, None] * q["tA"][dyn]
    f_mag = m[di][:, None] * q["tA_mag"][dyn]
    f_amp = m[di][:, None] * q["tA_amp"][dyn]
    com = np.asarray(com, np.float64)
    arm_pos = x[di] if mutant == "reaction_arm_xi" else x[dj]
    wrench = T._body_sums(obj[dj], com, arm_pos, f, f_mag, f_amp)
    return dict(a=a, a_bound=a_bound, a_mag=a_mag, w_new=w_new, w_bound=w_bound, alpha=np.where(fluid, alpha, 0.0), curl=curl,
                n_terms=np.bincount(i, minlength=n), pairs=dict(i=i, j=j, R=R, r=r, fluid_j=fl, dynamic_j=dyn), wrench=wrench)


def assert_alive(res, w, fl, rigid):
    """A scene change must not hollow the checks out."""
    p = res["pairs"]
    assert 2 * res["n_terms"].max() <= N_MAX, "more summed terms in a row than the derivation of C1 allows"
    assert np.abs(res["a"][fl]).max() > 1.0, "a_mp, m / s^2"
    assert np.abs(res["alpha"][fl]).max() > 1.0 and np.abs(res["w_new"] - w)[fl].max() > 1e-4, "alpha, 1 / s^2"
    if rigid:
        assert int((~p["fluid_j"]).sum()) > 300 and int(p["dynamic_j"].sum()) > 30, "boundary pairs / pairs with the dynamic body"
        assert np.abs(res["wrench"]["force"][BODY]).max() > 1e-6, "reaction on the body"


# ---------------------------------------------------------------------------------------------------------------------------
# The scenes: those of surface_tension_terms.scene, with an angular velocity per fluid particle drawn uniformly from a fixed seed.
KINDS = ("rigid", "fluid", "lattice", "lattice_fluid")


def scene(method, kind="rigid", **kw):
    return A.scene(method, kind, **kw)


def angular_velocities(sc, seed=23):
    """(n, 3) float32 in insertion order, uniform in the cube of half edge W_MAX / sqrt(3) (|w| <= W_MAX); zero on non-fluid rows."""
    mat = np.concatenate([np.asarray(b["material"]) for b in sc["batches"]])
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, (len(mat), 3)) * (W_MAX / np.sqrt(3.0))
    return np.where((mat == 1)[:, None], w, 0.0).astype(np.float32)


host_state = A.host_state


# ---------------------------------------------------------------------------------------------------------------------------
def rest_lattice(n=9, d=0.02, rho_i=None, rho0=1000.0):
    """An n^3 block on the exact rest lattice (h = 2 d, V0 = 0.8 d^3, one mass): dict(x, mass, vol, mat, rho_raw, centre: index of the middle particle, neighbours: its count within h)."""
    ax = d * np.arange(n)
    x = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + 0.2
    k = len(x)
    vol = np.full(k, 0.8 * d ** 3)
    mat = np.ones(k, np.int32)
    rho_raw, _, _, _ = T.density_f64(x, vol, mat, 2 * d, rho0)
    c = n // 2
    centre = (c * n + c) * n + c
    # (the six neighbours at exactly h = 2 d carry W = 0 and gradW = 0: whether rounding leaves them inside r <= h changes no sum)
    nbrs = int((np.linalg.norm(x - x[centre], axis=1) <= 2 * d * (1 + 1e-9)).sum()) - 1
    return dict(x=x, mass=rho0 * vol, vol=vol, mat=mat, rho_raw=rho_raw, centre=centre, neighbours=nbrs)
