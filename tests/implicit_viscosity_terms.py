"""The implicit-viscosity solve of the reference (SPH/fluid_solvers/base_solver.py:282-517: a block-Jacobi-scaled, matrix-free CG over the
neighbour graph) restated in float64 over a KD-tree pair list, pass by pass -- written from the reference's text, independent of the
oracle (oracle/sph_ref.c) and of the device code, in the style of tests/nonpressure_terms.py, whose pair list, kernel functions,
sums, scene and feed it uses.

The rule.  Every pass is checked on its own, from the inputs the device (or the oracle) itself held in front of it: the f32 D^-1, p,
r, A p, alpha, beta it stored are fed to the model as they are.  No rounding is carried through the CG recurrence, and every bound
is a one-pass backward-error bound |got - model| <= C1 sum|term| + C2 sum|term| amp + extra, relative to the sum of the MAGNITUDES of
the terms, valid for ANY f32 evaluation of the same sums in any order.  U = 2^-24.

Notation, for a fluid row i and a neighbour j within the support radius h: R = x_i - x_j, g = grad W_ij = s(r) R,
  -A_ij = k_j g R^T,  k_j = 2 (dim + 2) mu m_ij / rho_j / (r^2 + 0.01 h^2), m_ij = (m_i + m_j) / 2               (fluid j, :349-361)
                      k_j = 2 (dim + 2) mu_b rho0 V_j / rho_i / (r^2 + 0.01 h^2)                                    (rigid j, :362-371)
  D_i = I - dt / rho0 sum_j (-A_ij)   over fluid AND rigid j (:303-308, :326),  b_i = v_i - dt / rho0 sum_{j rigid} k_j (v_j . R) g (:334-346),
  (A p)_i = p_i + dt / rho0 sum_{j fluid} D_i^-1 (-A_ij) p_j (:374-391).
g is parallel to R, so -A_ij = k_j s R R^T is SYMMETRIC (and negative semidefinite: s < 0), and so are D_i and D_i^-1: the mutants "R g^T
for g R^T" and "D^-T for D^-1" are equivalent to the model, and the tests assert that they are.

Rounding counts (strict forms of csrc/sph_cg.hpp, kernGrad() and geom() of csrc/sph_device.hpp).
  One term of D (CgPreparePass::pair): the gradient 14 (x_i - x_j 1, r^2 3, sqrt 1, q 1, polynomial 4, its constant 1, 1 / (rn h) 2,
  x dx 1); r^2 + eps 1 (+ 1 of eps); m_i + m_j 1; cv m_ij 1 (+ 1 of cv); fdiv2 2; g_p R_q 1; s x 1: 24, then N additions, x dt 1, / rho0
  1 (2 in the fast build), 1 - 1.  With N <= N_MAX = 100 (asserted from the pair list): (24 + 100 + 4) u <= C1 = 1e-5; C2 = 5e-7 as in
  nonpressure_terms (the conditioning of the gradient in q).  The last subtraction rounds relative to |I| + |sum|: + U (|I| + mag).
  The boundary term of b: the gradient 14, cvb rho0 V_j 2 (+ 1), / rho_i 1 (2), v_j . R 5 relative to sum_c |v_jc R_c| (carried by the
  magnitude), x 1, / (r^2 + eps) 1 + 2, x g 1: 30; then N additions, dt x 1, / rho0 1 (2), v - 1: inside C1 too; + U (|v| + mag).
  mat3_inverse (cofactor form, 1 / det first), for the f32 D the pass held: every cofactor is a b - c d: 3 roundings relative to
  cofmag = |a b| + |c d|; det = sum_k a_k cof_k over the first column: the cofactor's 3, the product 1, two additions 2: 6 u detmag with
  detmag = sum_k |a_k| cofmag_k; 1 / det 1 (the fast build's v_rcp: 1 ulp, so 2 is taken); inv x cofactor 1.  Hence, to first order,
      |X - D^-1| <= 3 u cofmag^T / |det| + |D^-1| (6 u detmag / |det| + 3 u) =: E_inv
  and the residual of the stored inverse X against the float64 D:  |D X - I| <= E_D |X| + |D| E_inv (1 + 1e-3 for the second order),
  E_D the bound of D itself.  Nothing is fitted: |D|, |cof D| and |det D| come from the float64 D.
  One term of A p, strict build (CgApPass::pair, per-pair D^-1 (-A) p column by column): the gradient 14, r^2 + eps 2, m_ij 1, cv m_ij 2,
  fdiv2 2, n = s (g R_q) 2, M = D^-1 n 5, M p_q 1, two additions 2: 31; the fast build applies D^-1 to the sum (t = -s (R . p) 5, t g 1,
  then 5 for D^-1 once): fewer.  Behind the sum: x dt 1, / rho0 1 (2), + p 1; the three-way split adds two additions.  (31 + 100 + 6) u
  <= C1.  The magnitude that covers BOTH orders is |D^-1| sum_j |t_j| |g_j| with |t_j| = k_j sum_c |R_c p_jc|: it dominates the
  per-pair form sum_j sum_q |(D^-1 n_j)_pq| |p_jq|.  The last addition: + U (|p_i| + dt / rho0 mag).
  r0 = D^-1 b - A p from the device's own D^-1, b and A p: three products, two additions, one subtraction: 4 U (|D^-1| |b| + |A p|).
  The sums |r|^2, p . A p, |new r|^2: 3 N_f terms (N_f fluid rows) added in any order, each a product: (3 N_f + 2) U sum|term|.  Where the
  last A p pass left parts only (the split walk inside the loop), p . A p = sum_g p . (dt / rho0 part_g) + |p|^2: 12 N_f terms, each
  part x dt 1, / rho0 1 (2), x p 1: (12 N_f + 5) U sum|term|, the magnitude being the sum of the absolute values of exactly these terms.
  A quotient: (e_num + |q| e_den) / |den| + 2 U |q| (the division: 1, the fast build's 2).  error = sqrt(num): e_num / (2 sqrt(num)) + 2 U.
  x += alpha p, r -= alpha A p, p = r + beta p with the device's own alpha, beta: two roundings each (one under fma): 2 U (|a| + |s b|).
  Where A p comes from parts, A p = ((a0 + a1) + a2) dt / rho0 + p is evaluated in f32 first: two additions, x dt, / rho0 (2), + p:
  + |alpha| 6 U ((|a0| + |a1| + |a2|) dt / rho0 + |p|).
  The initial guess x = x_warm + v: ONE f32 addition, held to the bits (so is p = x and v0 = v; where the warm start is zero x = v).
  The end (:514-517): nonpressure_terms.non_pressure_f64 with the solved velocities in the viscous term and its bounds unchanged."""
import numpy as np

from tests.helpers import _pair_list
from tests.nonpressure_terms import C1, C2, N_MAX, U, _drop_first, _sum, kernel_grad_scale

PREPARE_MUTANTS = ("mij_is_mi", "rho_i_for_rho_j", "mu_for_mu_b", "no_rigid_in_D", "b_without_boundary", "no_eps", "D_without_identity",
                   "drop_neighbour")
AP_MUTANTS = ("mij_is_mi", "rho_i_for_rho_j", "rigid_in_offdiagonal", "no_eps", "Ap_without_p", "drop_neighbour")
EQUIVALENT_MUTANTS = ("R_gT_for_g_RT", "Dinv_transposed")
SCALAR_MUTANTS = ("alpha_den_r_Ap", "beta_inverted", "beta_from_previous_partials")
UPDATE_MUTANTS = ("r0_without_Dinv", "x_with_new_p")
END_MUTANTS = ("end_reads_original_velocity", "end_advances_solved_velocity", "guess_not_reduced")


def _pairs(x, mat, h, mutant=None):
    _, i, j = _pair_list(x, h)
    R = x[i] - x[j]
    r = np.linalg.norm(R, axis=1)
    keep = (mat[i] == 1) & (r <= h) & ((mat[j] == 1) | (mat[j] == 2))
    if mutant == "drop_neighbour":
        keep = _drop_first(i, keep)
    return i[keep], j[keep], R[keep], r[keep]


def _coef(i, j, r, fl_j, rho, mass, vol, params, mutant):
    """k_j of the module docstring per pair, and the index of the density it divides by"""
    h, rho0, mu, mu_b, dim = params["h"], params["rho0"], params["mu"], params["mu_b"], params.get("dim", 3)
    m_ij = mass[i] if mutant == "mij_is_mi" else 0.5 * (mass[i] + mass[j])
    den_idx = np.where(fl_j, i if mutant == "rho_i_for_rho_j" else j, i)
    eps = 0.0 if mutant == "no_eps" else 0.01 * h * h
    k = 2 * (dim + 2) * np.where(fl_j, mu * m_ij, (mu if mutant == "mu_for_mu_b" else mu_b) * rho0 * vol[j]) / rho[den_idx] / (r * r + eps)
    return k, den_idx


def _outer(a, b):
    return a[:, :, None] * b[:, None, :]


def _sum33(o, n, t):
    return np.stack([_sum(o, n, t[:, a, :]) for a in range(3)], axis=1)


def prepare_f64(x, v, rho, mass, vol, mat, params, mutant=None, rho_bound=None):
    """prepare_conjugate_gradient_solver1 (:282-316) for fluid rows: D (n, 3, 3) with its bound E_D, b (n, 3) with its bound.  `rho`: the
    density the pass reads, `rho_bound` the bound of its error (WCSPH: the raw density, nonpressure_terms' docstring): every term then
    carries |term| rho_bound / rho on top.  Rows of non-fluid particles: D = I, b = 0.  Returns dict D, D_bound, b, b_bound, n_terms,
    n_rigid (rigid neighbours per row), vb_mag (sum_j |v_j . R| over the rigid neighbours)."""
    x, v = x.astype(np.float64), v.astype(np.float64)
    n = len(x)
    rho0, dt = params["rho0"], params["dt"]
    rho = np.asarray(rho, np.float64)
    rb = np.zeros(n) if rho_bound is None else np.asarray(rho_bound, np.float64)
    mass, vol = mass.astype(np.float64), vol.astype(np.float64)
    i, j, R, r = _pairs(x, mat, params["h"], mutant)
    fl_j = mat[j] == 1
    s, s_amp = kernel_grad_scale(r, params["h"])
    k, den_idx = _coef(i, j, r, fl_j, rho, mass, vol, params, mutant)
    rel_rho = (rb[den_idx] / rho[den_idx])
    in_D = fl_j | (mutant != "no_rigid_in_D")
    RR = _outer(R, R)
    if mutant == "R_gT_for_g_RT":
        RR = np.transpose(RR, (0, 2, 1))
    T = np.where(in_D, k * s, 0.0)[:, None, None] * RR * (dt / rho0)           # dt / rho0 (-A_ij)
    Tmag = np.abs(T)
    Tamp = np.where(in_D, k * s_amp, 0.0)[:, None, None] * np.abs(RR) * (dt / rho0)
    eye = np.eye(3)[None]
    fluid = (mat == 1)
    S, mag = _sum33(i, n, T), _sum33(i, n, Tmag)
    D = (0.0 if mutant == "D_without_identity" else eye) - S
    D_bound = C1 * mag + C2 * _sum33(i, n, Tamp) + _sum33(i, n, Tmag * rel_rho[:, None, None]) + U * (eye + mag)
    D = np.where(fluid[:, None, None], D, eye)
    # ---- b
    rg = ~fl_j
    vR = (v[j] * R).sum(axis=1)
    vR_mag = (np.abs(v[j]) * np.abs(R)).sum(axis=1)
    cb = np.where(rg, k, 0.0) * (dt / rho0)
    tb = (cb * vR * s)[:, None] * R
    tb_mag = (cb * vR_mag * np.abs(s))[:, None] * np.abs(R)
    tb_amp = (cb * vR_mag * s_amp)[:, None] * np.abs(R)
    bsum = 0.0 if mutant == "b_without_boundary" else _sum(i, n, tb)
    bmag = _sum(i, n, tb_mag)
    b = np.where(fluid[:, None], v - bsum, 0.0)
    b_bound = C1 * bmag + C2 * _sum(i, n, tb_amp) + _sum(i, n, tb_mag * rel_rho[:, None]) + U * (np.abs(v) + bmag)
    return dict(D=D, D_bound=np.where(fluid[:, None, None], D_bound, 0.0), b=b, b_bound=np.where(fluid[:, None], b_bound, 0.0),
                n_terms=np.bincount(i, minlength=n), n_rigid=np.bincount(i[rg], minlength=n), vb_mag=_sum(i, n, np.where(rg, vR_mag, 0.0)),
                b_shift=_sum(i, n, tb))


def _cof(D):
    """cofactor matrices and the sums of the magnitudes of their two products, (n, 3, 3)"""
    c, m = np.empty_like(D), np.empty_like(D)
    for a in range(3):
        for b in range(3):
            a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
            p, q = D[:, a1, b1] * D[:, a2, b2], D[:, a2, b1] * D[:, a1, b2]
            c[:, a, b], m[:, a, b] = p - q, np.abs(p) + np.abs(q)
    return c, m


def inverse_residual(D, D_bound, X):
    """(|D X - I|, its bound) for the stored f32 inverse X of a float64 D known within D_bound (module docstring)"""
    X = X.astype(np.float64)
    cof, cofmag = _cof(D)
    det = (D[:, :, 0] * cof[:, :, 0]).sum(axis=1)
    detmag = (np.abs(D[:, :, 0]) * cofmag[:, :, 0]).sum(axis=1)
    ad = np.abs(det)[:, None, None]
    Dinv = np.transpose(cof, (0, 2, 1)) / det[:, None, None]
    e_inv = 3 * U * np.transpose(cofmag, (0, 2, 1)) / ad + np.abs(Dinv) * (6 * U * detmag[:, None, None] / ad + 3 * U)
    res = np.abs(D @ X - np.eye(3)[None])
    return res, D_bound @ np.abs(X) + (np.abs(D) @ e_inv) * (1 + 1e-3)


def ap_f64(x, p, X, rho, mass, vol, mat, params, mutant=None, rho_bound=None):
    """compute_Ap (:374-391) from a GIVEN D^-1 (X, the stored f32 one) and search direction p, for fluid rows.  Returns dict Ap, bound, off
    (dt / rho0 D^-1 sum: what a split walk's parts add up to, times dt / rho0), n_terms (fluid neighbours)."""
    x, p, X = x.astype(np.float64), p.astype(np.float64), X.astype(np.float64)
    n = len(x)
    rho0, dt = params["rho0"], params["dt"]
    rho = np.asarray(rho, np.float64)
    rb = np.zeros(n) if rho_bound is None else np.asarray(rho_bound, np.float64)
    mass, vol = mass.astype(np.float64), vol.astype(np.float64)
    i, j, R, r = _pairs(x, mat, params["h"], mutant)
    fl_j = mat[j] == 1
    use = fl_j | (mutant == "rigid_in_offdiagonal")
    i, j, R, r, fl_j = i[use], j[use], R[use], r[use], fl_j[use]
    s, s_amp = kernel_grad_scale(r, params["h"])
    k, den_idx = _coef(i, j, r, fl_j, rho, mass, vol, params, mutant)
    Rp = (R * p[j]).sum(axis=1)
    Rp_mag = (np.abs(R) * np.abs(p[j])).sum(axis=1)
    t = (k * Rp * s)[:, None] * R                              # (-A_ij) p_j = k (R . p_j) g
    tmag = (k * Rp_mag * np.abs(s))[:, None] * np.abs(R)
    tamp = (k * Rp_mag * s_amp)[:, None] * np.abs(R)
    trho = tmag * (rb[den_idx] / rho[den_idx])[:, None]
    if mutant == "Dinv_transposed":
        X = np.transpose(X, (0, 2, 1))
    aX = np.abs(X)
    f = dt / rho0
    mv = lambda M, w: np.einsum("nab,nb->na", M, w)
    off = f * mv(X, _sum(i, n, t))
    mag = f * mv(aX, _sum(i, n, tmag))
    own = 0.0 if mutant == "Ap_without_p" else p
    fluid = (mat == 1)[:, None]
    Ap = np.where(fluid, own + off, 0.0)
    bound = C1 * mag + C2 * f * mv(aX, _sum(i, n, tamp)) + f * mv(aX, _sum(i, n, trho)) + U * (np.abs(p) + mag)
    return dict(Ap=Ap, off=np.where(fluid, off, 0.0), bound=np.where(fluid, bound, 0.0), n_terms=np.bincount(i, minlength=n))


def ap_from_parts(parts, p, params):
    """A p = ((a0 + a1) + a2) dt / rho0 + p in float64 from the three parts of a split walk (3, n, 3), with the sum of the magnitudes of
    its terms"""
    f = params["dt"] / params["rho0"]
    a = parts.astype(np.float64)
    return a.sum(axis=0) * f + p.astype(np.float64), np.abs(a).sum(axis=0) * f + np.abs(p.astype(np.float64))


def r0_f64(X, b, Ap, mutant=None):
    """prepare_conjugate_gradient_solver2 (:318-323): r0 = D^-1 b - A p (p0 = r0) from the stored D^-1, b and A p; (r0, bound)"""
    X, b, Ap = X.astype(np.float64), b.astype(np.float64), Ap.astype(np.float64)
    Xb = b if mutant == "r0_without_Dinv" else np.einsum("nab,nb->na", X, b)
    return Xb - Ap, 4 * U * (np.einsum("nab,nb->na", np.abs(X), np.abs(b)) + np.abs(Ap))


def _dot(a, b, fl, k=2):
    """(sum over the fluid rows of a . b, its bound (3 N_f + k) U sum|term|)"""
    t = a.astype(np.float64)[fl] * b.astype(np.float64)[fl]
    return t.sum(), (3 * int(fl.sum()) + k) * U * np.abs(t).sum()


def _quot(num, e_num, den, e_den):
    q = num / den if den > 1e-18 else 0.0
    return q, (e_num + abs(q) * e_den) / abs(den) + 2 * U * abs(q)


def alpha_f64(r, p, Ap, fl, parts=None, params=None, mutant=None):
    """compute_cg_alpha (:394-406): |r|^2 / (p . A p) over the fluid rows from the stored vectors; with `parts` (the split walk inside the
    loop left no A p) the denominator is sum_g p . (dt / rho0 part_g) + |p|^2.  Returns (alpha, bound)."""
    num, e_num = _dot(r, r, fl)
    if mutant == "alpha_den_r_Ap":
        p = r
    if parts is None:
        den, e_den = _dot(p, Ap, fl)
    else:
        f = params["dt"] / params["rho0"]
        pp = p.astype(np.float64)[fl]
        t = np.concatenate([(pp * (f * parts[g].astype(np.float64)[fl])).ravel() for g in range(3)] + [(pp * pp).ravel()])
        den, e_den = t.sum(), (12 * int(fl.sum()) + 5) * U * np.abs(t).sum()
    return _quot(num, e_num, den, e_den)


def beta_error_f64(r_new, r_old, fl, mutant=None, r_older=None):
    """update_cg_r_and_beta (:415-431): beta = |new r|^2 / |old r|^2, error = sqrt(|new r|^2); ((beta, bound), (error, bound)).  The mutant
    'beta_from_previous_partials' takes the two sums one iteration late (the parity hazard of the fused p update)."""
    num, e_num = _dot(r_new, r_new, fl)
    den, e_den = _dot(r_old, r_old, fl)
    err = np.sqrt(num)
    eb = (err, e_num / (2 * err) + 2 * U * err if err > 0 else 0.0)
    if mutant == "beta_inverted":
        num, den = den, num
    if mutant == "beta_from_previous_partials":
        num, den = den, _dot(r_older, r_older, fl)[0]
    return _quot(num, e_num, den, e_den), eb


def axpy_f64(a, scal, b, extra=None):
    """a + scal b with two roundings: (value, bound 2 U (|a| + |scal b|) [+ |scal| extra])"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    s = float(scal)
    return a + s * b, 2 * U * (np.abs(a) + np.abs(s * b)) + (abs(s) * extra if extra is not None else 0.0)


# ---- the scene: nonpressure_terms.scene with the implicit method.  mu, mu_b: the median over the fluid rows of max |D - I|, computed with
# prepare_f64 from the oracle's state behind prepare(), is 0.0078 / 0.0074 (rigid scene / twin) per unit of mu at mu_b = 4 mu (D - I is
# linear in (mu, mu_b)): the default mu = 1 is far too small, MU = 150, MU_B = 600 give 1.17 / 1.12, inside [0.5, 5]
# (test_implicit_viscosity_host.py asserts it).
MU, MU_B = 150.0, 600.0
# K_STEPS: the second state, K whole steps (two fixed CG iterations each) behind prepare().  Slots that hold a fluid row now and held a
# rigid particle at the first state / the reverse, by the oracle's sort of the rigid scene: K = 0: 0 / 0, K = 1: 36 / 36, K = 2: 73 / 73.
# K = 1 is the smallest with at least 20 of each (test_second_state_exchanges_slots asserts both halves); the warm start is nonzero
# there in 1215 of 1251 fluid rows.
K_STEPS = 1
FIXED_ITERATIONS = 2


def scene(method="dfsph", rigid=True, layers=None):
    from tests import nonpressure_terms as T
    sc = T.scene(method, rigid=rigid, viscosity=MU, viscosity_b=MU_B, viscosity_method="implicit", layers=layers)
    assert sc["pd"]["viscosity_implicit"] == 1
    sc["pd"]["fixed_iterations"] = FIXED_ITERATIONS
    return sc


def _frac(err, bound):
    """worst err / bound; a row with a zero bound has to be exact"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(f.max()) if f.size else 0.0


# ---- the comparisons, shared by the CPU tests (oracle) and the GPU tests (library): every array by the same particle order

def check_prepare(sc, s0, s1, fr, rho_bound=None, mutant=None):
    """The prepare phase.  s0: x, v, rho, mass, vol, mat and `xw` (cg_x in front of the pass); s1: X (n, 3, 3), b, x, p, r, Ap, v0 behind it,
    with `Ap` the A p of the first walk.  Fills `fr` with the worst fractions and returns the model's pieces."""
    P = sc["params"]
    fl = s0["mat"] == 1
    pre = prepare_f64(s0["x"], s0["v"], s0["rho"], s0["mass"], s0["vol"], s0["mat"], P, mutant=mutant, rho_bound=rho_bound)
    res, rb = inverse_residual(pre["D"], pre["D_bound"], s1["X"])
    fr["|D X - I|"] = _frac(res[fl], rb[fl])
    fr["b"] = _frac(np.abs(s1["b"] - pre["b"])[fl], pre["b_bound"][fl])
    return pre


def check_guess(s0, s1):
    """x = x_warm + v in ONE f32 addition, v0 = v: to the bits (fluid rows)"""
    fl = s0["mat"] == 1
    x32 = s0["xw"].astype(np.float32) + s0["v"].astype(np.float32)
    assert x32.dtype == np.float32
    np.testing.assert_array_equal(s1["x"][fl], x32[fl], err_msg="initial guess x_warm + v")
    np.testing.assert_array_equal(s1["v0"][fl], s0["v"][fl], err_msg="original velocity")


def check_ap(sc, s0, p, X, got_off_plus_p, fr, tag, rho_bound=None, mutant=None):
    P = sc["params"]
    fl = s0["mat"] == 1
    ap = ap_f64(s0["x"], p, X, s0["rho"], s0["mass"], s0["vol"], s0["mat"], P, mutant=mutant, rho_bound=rho_bound)
    fr[tag] = _frac(np.abs(got_off_plus_p - ap["Ap"])[fl], ap["bound"][fl])
    return ap


def assert_alive(sc, s0, pre, ap):
    """conditions (a)-(d) of the inputs"""
    fl = s0["mat"] == 1
    dev = np.abs(pre["D"] - np.eye(3)[None]).max(axis=(1, 2))[fl]
    assert 0.5 <= np.median(dev) <= 5.0, ("(a) median over the fluid rows of max |D - I|", float(np.median(dev)))
    assert pre["n_terms"].max() <= N_MAX and ap["n_terms"].max() <= N_MAX, "(c) more summed terms in a row than the derivation of C1 allows"
    nf = int(fl.sum())
    assert nf % 64 and nf % 256 and len(fl) % 64 and len(fl) % 256, "(d) a row count that is a multiple of 64 or 256"
    if sc["rigid"]:
        from tests.nonpressure_terms import BODY
        near_cube = np.zeros(len(fl), bool)
        x = s0["x"].astype(np.float64)
        _, i, j = _pair_list(x, sc["params"]["h"])
        r = np.linalg.norm(x[i] - x[j], axis=1)
        sel = (s0["mat"][i] == 1) & (s0["obj"][j] == BODY) & (s0["mat"][j] == 2) & (r <= sc["params"]["h"] * (1 - 1e-6))
        near_cube[i[sel]] = True
        assert int(near_cube.sum()) >= 50, "fluid rows with a neighbour in the cube"
        # (b) the cube moves: every row that sees it has b != v and a nonzero boundary velocity.  The domain box stands still, so a row
        # that sees ONLY the box has b == v exactly (v_j = 0 in every term): held to the bits by check_wall_rows.
        assert (np.abs(pre["b_shift"][near_cube]).max(axis=1) > 0).all() and (pre["vb_mag"][near_cube] > 0).all(), "(b)"
        assert int(((pre["n_rigid"] > 0) & fl & ~near_cube).sum()) >= 200, "fluid rows near the box only"


def check_wall_rows(s0, pre, b_got):
    """rows whose rigid neighbours all stand still: b == v to the bits"""
    still = (pre["n_rigid"] > 0) & (pre["vb_mag"] == 0) & (s0["mat"] == 1)
    np.testing.assert_array_equal(b_got[still], s0["v"][still])
    return int(still.sum())


def check_end(sc, s0, solved, v1, guess, wrench, fr, tiny_wrench=0.0, mutant=None):
    """The end of the solve (:514-517).  s0: x, v (the ORIGINAL velocity), rho, mass, vol, mat, dyn, obj; `solved`: cg_x in front of it; v1,
    `guess` (cg_x) behind it; wrench = (forces, torques) accumulated over it."""
    from tests import nonpressure_terms as T
    P = sc["params"]
    fl = s0["mat"] == 1
    vv = np.where(fl[:, None], solved, s0["v"]).astype(np.float64)
    if mutant == "end_reads_original_velocity":
        vv = s0["v"].astype(np.float64)
    res = T.non_pressure_f64(s0["x"], s0["v"], s0["rho"], s0["mass"], s0["vol"], s0["mat"], s0["dyn"], s0["obj"], sc["com"], P, visc_v=vv)
    dt = P["dt"]
    base = (solved if mutant == "end_advances_solved_velocity" else s0["v"]).astype(np.float64)
    want = base + dt * res["a"]
    bound = dt * T.accel_bound(res) + 2 * U * (np.abs(base) + dt * np.abs(res["a"]))
    fr["end v"] = _frac(np.abs(v1 - want)[fl], bound[fl])
    g32 = solved.astype(np.float32) - (0 if mutant == "guess_not_reduced" else s0["v"].astype(np.float32))
    fr["end guess (bits)"] = 0.0 if np.array_equal(guess[fl], g32[fl]) else np.inf
    assert res["visc_mag"][fl].min() > 0.5, "the viscous term of the end is alive"
    if sc["rigid"]:
        w = res["wrench"]
        assert np.abs(w["force"][T.BODY]).min() > 1e-4 and w["pairs"][T.BODY] > 50
        for part, g in (("force", wrench[0]), ("torque", wrench[1])):
            wb = T.wrench_bound(w, part)[T.BODY] + tiny_wrench + U * np.abs(w[part][T.BODY])
            fr["end wrench " + part] = _frac(np.abs(g - w[part])[T.BODY], wb)
    return res


def check_iteration(sc, s0, X, cur, got, fr, tag, rho_bound=None):
    """One A p pass and the x / r update behind it.  cur: x, r, p -- p the search direction of THIS iteration (where the p update is folded
    into the A p pass: as stored behind that pass).  got: `Ap` (n, 3), or `parts` (3, n, 3) where the walk left parts only; alpha; x1, r1
    behind the update.  Fills fr."""
    P = sc["params"]
    fl = s0["mat"] == 1
    parts = got.get("parts")
    if parts is None:
        Ap64, extra = got["Ap"].astype(np.float64), None
    else:
        Ap64, apmag = ap_from_parts(parts, cur["p"], P)
        extra = 6 * U * apmag
    check_ap(sc, s0, cur["p"], X, Ap64, fr, tag + " A p" + (" (parts)" if parts is not None else ""), rho_bound=rho_bound)
    a, ab = alpha_f64(cur["r"], cur["p"], got.get("Ap"), fl, parts=parts, params=P)
    fr[tag + " alpha"] = _frac(abs(float(got["alpha"]) - a), ab)
    x1, xb = axpy_f64(cur["x"], got["alpha"], cur["p"])
    fr[tag + " x"] = _frac(np.abs(got["x1"] - x1)[fl], xb[fl])
    r1, rb = axpy_f64(cur["r"], -float(got["alpha"]), Ap64, extra=extra)
    fr[tag + " r"] = _frac(np.abs(got["r1"] - r1)[fl], rb[fl])


def check_p_update(s0, r_old, r1, p, got, fr, tag):
    """beta, error and p = r + beta p.  got: beta, error, p1."""
    fl = s0["mat"] == 1
    (b, bb), (e, eb) = beta_error_f64(r1, r_old, fl)
    fr[tag + " beta"] = _frac(abs(float(got["beta"]) - b), bb)
    fr[tag + " error"] = _frac(abs(float(got["error"]) - e), eb)
    p1, pb = axpy_f64(r1, got["beta"], p)
    fr[tag + " p"] = _frac(np.abs(got["p1"] - p1)[fl], pb[fl])
