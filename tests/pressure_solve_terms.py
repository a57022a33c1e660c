"""The inner passes of the two iterative pressure solvers restated in float64 over a KD-tree pair list -- the velocity correction of
the DFSPH divergence and density solve with its fluid -> rigid wrench (DFSPH.py:162-202, :246-283), the DFSPH rho* (:105-126), the
PCISPH rho* with its pressure update (PCISPH.py:33-71), pcisph_k (:129-151) and the predicted velocity and position (:19-29,
:154-162) -- written from the reference's text, independent of the oracle (oracle/sph_ref.c) and of the device code, in the style
of tests/nonpressure_terms.py, whose kernel functions, sums, scene and wrench bound it uses.

What a solve phase of the library leaves behind with fixed_iterations = 1 (csrc/sph_steps.hpp run_solve, dfsph_density,
dfsph_divergence).  `pre` runs the rho* (D rho / Dt) pass, which writes rho* and the kappa derived from it into kappa_next.  The one
iteration swaps kappa and kappa_next, runs the correction with kappa, and runs the rho* pass again, which writes into kappa_next.
In fixed mode run_solve reports launched == fixed == *sp.iter, so the parity swap behind the loop, (launched - iter) & 1, is 0 and
nothing is swapped back.  Hence after SPH_PH_DFSPH_DENSITY (SPH_PH_DFSPH_DIVERGENCE): F_DFSPH_KAPPA (F_DFSPH_KAPPA_V) holds the kappa
the correction used, F_VELOCITY the corrected velocity, and F_DENSITY_STAR (F_DENSITY_DERIV) belongs to that corrected velocity.

Bounds.  As in nonpressure_terms: |got - model| <= C1 sum|term| + C2 sum|term| amp + extra, for ANY f32 evaluation of the sums.
Roundings of one pair term in the longest strict form, DfsphCorrectPass::pair() of csrc/sph_solvers.hpp (fluid branch) with
kernGrad() and geom() of csrc/sph_device.hpp: x_i - x_j 1; r^2 3; sqrt 1; q 1; the polynomial 4; its constant 1; 1 / (rn h) 2;
x dx 1 (the gradient: 14); V_j x 1; k_i / rho_i 1, k_j / rho_j 1, their sum 1 -- relative to |k_i / rho_i| + |k_j / rho_j|, which is
why the term magnitude carries that sum and kappas of opposite sign cannot shrink the bound --; x cc 1; x rho0 1.  That is 20; the
fast form has the two-rounding fdiv twice and v_rsq / v_rcp (+ 6).  The rho* term (DfsphRhoAdvPass::pair): the gradient 14, v_i - v_j
1, the three products and two additions 3 (relative to sum_c |dv_c g_c|), V_j x 1: 19.  The PCISPH rho* term (PcisphRhoStarPass::pair):
the difference 1, r^2 3, sqrt 1, q 1, polynomial 4, constant 1, V_j x 1: 12.  All fit nonpressure_terms' budget (36 + N_MAX + 3) u <=
1e-5 with N_MAX = 100 summed terms per row (asserted from the pair list), so its C1 = 1e-5 and C2 = 5e-7 are used unchanged.
The wrench term: the 20 (26) of the correction term, / dt 1 (2), x m0 1 and m0 = V_i rho0 1, the arm 1, the cross product 3: <= 34 <=
WRENCH_TERM = 44 of nonpressure_terms.wrench_bound, used unchanged.

Two additions that follow from the code.  (a) MODE 1 (density solve) subtracts every term from the velocity itself: n_i subtractions
and nothing else, each rounding relative to a partial result of at most |v0| + sum|term|: + (n_i + 1) u (|v0| + sum|term|) per
component (MODE 0: the one addition v0 + dv, 1 u of the same).  (b) The threshold |k_sum| > m_eps dt: k_i + k_j is one rounding, the
f32 product m_eps dt two (the constant's and the product's); a pair with | |k_sum| - m_eps dt | <= 3 u (|k_sum| + m_eps dt) may go
either way and adds its |term| to the bound (`extra`).  At most 1 % of the accepted pairs may be ambiguous (assert_alive_dfsph).
The same holds for the PCISPH rho* and a CURRENT distance within 4 u h of h: the pair's term at the predicted distance need not be
small, so it goes into `extra`."""
import numpy as np

from tests.helpers import _pair_list
from tests.nonpressure_terms import (C1, C2, N_MAX, U, _body_sums, _sum, kernel_grad_scale, kernel_w)

M_EPS = 1e-5   # DFSPH.py:17

CORRECTION_MUTANTS = ("kj_left_out", "rho_i_for_rho_j", "no_threshold", "threshold_on_ki", "rigid_as_fluid", "plus_for_minus",
                      "mode0_from_updated_velocity", "reaction_sign", "reaction_without_dt", "reaction_mj_for_mi",
                      "torque_arm_without_com")
RHO_STAR_MUTANTS = ("no_clamp_at_1", "dt_left_out", "stale_velocity")
PCISPH_MUTANTS = ("neighbours_by_predicted", "rigid_at_predicted", "w_at_current", "no_clamp_at_0")


def _pairs(x, mat, h):
    """directed pairs (i fluid, j fluid or rigid) within the pair list's radius, with R = x_i - x_j and r"""
    _, i, j = _pair_list(x, h)
    keep = (mat[i] == 1) & ((mat[j] == 1) | (mat[j] == 2))
    i, j = i[keep], j[keep]
    R = x[i] - x[j]
    return i, j, R, np.linalg.norm(R, axis=1)


def dfsph_correction_f64(x, kappa, rho, vol, mat, is_dynamic, obj, com, params, mode, mutant=None):
    """correct_divergence_step (DFSPH.py:162-202, mode 0, kappa = kappa_v) / correct_density_error_step (:246-283, mode 1): for fluid i
      fluid j:  if |k_i + k_j| > m_eps dt:  v_i -= V_j grad W_ij (k_i / rho_i + k_j / rho_j) rho0
      rigid j:  if |k_i| > m_eps dt:        v_i -= V_j grad W_ij (k_i / rho_i) rho0, and for a dynamic j the body of j takes
                force_j = V_j grad W_ij (k_i / rho_i) rho0 / dt (V_i rho0), torque_j = (x_j - com_j) x force_j.
    The two modes compute the same dv (mode 0 accumulates it and adds it, mode 1 subtracts term by term from the velocity; neither
    reads a neighbour's velocity): `mode` only names the bound (correction_bound).  Returns dict: dv, mag = sum|term| with |term| =
    |V_j grad W| (|k_i / rho_i| + |k_j / rho_j|) rho0, mag_amp, extra (the ambiguous pairs' |term|) -- (n, 3), rows of non-fluid
    particles zero --, n_terms (accepted + ambiguous), pairs: dict(i, j, fluid_j, accepted, ambiguous, skipped_zero, dynamic_j, term),
    wrench (nonpressure_terms._body_sums)."""
    x = x.astype(np.float64)
    n = len(x)
    h, rho0, dt = params["h"], params["rho0"], params["dt"]
    k, rh, vl = kappa.astype(np.float64), rho.astype(np.float64), vol.astype(np.float64)
    i, j, R, r = _pairs(x, mat, h)
    keep = r <= h
    i, j, R, r = i[keep], j[keep], R[keep], r[keep]
    fl_j = mat[j] == 1
    s, s_amp = kernel_grad_scale(r, h)
    thr = M_EPS * dt
    k_i = k[i]
    k_j = np.where(fl_j, k[j], 0.0)
    rho_j = np.where(fl_j, rh[j], 1.0)
    if mutant == "rigid_as_fluid":   # the reference's dead assignment k_j = k_i (:185, :266) taken at its word: the fluid formula, no reaction
        k_j = np.where(fl_j, k_j, k_i)
        rho_j = np.where(fl_j, rho_j, rh[i])
    k_sum = k_i + k_j
    if mutant == "threshold_on_ki":
        k_sum = k_i
    accepted = np.abs(k_sum) > thr
    if mutant == "no_threshold":
        accepted = np.ones_like(accepted)
    ambiguous = (np.abs(np.abs(k_sum) - thr) <= 3 * U * (np.abs(k_sum) + thr)) & (mutant is None)
    a_i = k_i / rh[i]
    a_j = k_j / (rh[i] if mutant == "rho_i_for_rho_j" else rho_j)
    if mutant == "kj_left_out":
        a_j = 0.0 * a_j
    sign = 1.0 if mutant == "plus_for_minus" else -1.0
    gs = vl[j] * s
    base = (gs * (a_i + a_j) * rho0)[:, None] * R          # V_j grad W (k_i / rho_i + k_j / rho_j) rho0
    term = sign * base
    tmag = (np.abs(gs) * (np.abs(a_i) + np.abs(a_j)) * rho0)[:, None] * np.abs(R)
    tamp = (vl[j] * s_amp * (np.abs(a_i) + np.abs(a_j)) * rho0)[:, None] * np.abs(R)
    acc = accepted[:, None]
    fluid = (mat == 1)[:, None]
    dv = np.where(fluid, _sum(i, n, np.where(acc, term, 0.0)), 0.0)
    mag = _sum(i, n, np.where(acc | ambiguous[:, None], tmag, 0.0))
    mag_amp = _sum(i, n, np.where(acc | ambiguous[:, None], tamp, 0.0))
    extra = _sum(i, n, np.where(ambiguous[:, None], tmag, 0.0))
    # ---- reaction on dynamic bodies (:193-202, :274-283)
    dyn = ~fl_j & (is_dynamic[j] != 0) & accepted & (mutant != "rigid_as_fluid")
    m_i = rho0 * (vl[j[dyn]] if mutant == "reaction_mj_for_mi" else vl[i[dyn]])
    scale = (m_i / (1.0 if mutant == "reaction_without_dt" else dt))[:, None]
    rsign = -1.0 if mutant == "reaction_sign" else 1.0
    f = rsign * base[dyn] * scale
    wrench = _body_sums(obj[j[dyn]], np.asarray(com, np.float64), x[j[dyn]], f, tmag[dyn] * scale, tamp[dyn] * scale,
                        no_com=mutant == "torque_arm_without_com")
    amb_dyn = ~fl_j & (is_dynamic[j] != 0) & ambiguous
    amb_scale = (rho0 * vl[i[amb_dyn]] / dt)[:, None]
    wa = _body_sums(obj[j[amb_dyn]], np.asarray(com, np.float64), x[j[amb_dyn]], 0.0 * tmag[amb_dyn], tmag[amb_dyn] * amb_scale,
                    0.0 * tmag[amb_dyn])
    wrench["force_extra"], wrench["torque_extra"] = wa["force_mag"], wa["torque_mag"]
    skipped_zero = ~accepted & ~ambiguous & (k_i == 0) & (k_j == 0)
    return dict(dv=dv, mag=mag, mag_amp=mag_amp, extra=extra, n_terms=np.bincount(i[accepted | ambiguous], minlength=n),
                n_nbr=np.bincount(i, minlength=n),
                pairs=dict(i=i, j=j, fluid_j=fl_j, accepted=accepted, ambiguous=ambiguous, skipped_zero=skipped_zero, dynamic_j=dyn,
                           term=term), wrench=wrench)


def correction_bound(res, mode, v0):
    """bound of (v1 - v0) against res["dv"], both taken in float64 of the stored f32 velocities (module docstring (a))"""
    n = res["n_terms"].astype(np.float64)[:, None]
    adds = (n + 1.0) if mode == 1 else 1.0
    return C1 * res["mag"] + C2 * res["mag_amp"] + res["extra"] + adds * U * (np.abs(v0.astype(np.float64)) + res["mag"])


def dfsph_rho_star_f64(x, v, rho, vol, mat, params, mutant=None, v_stale=None):
    """compute_density_star (DFSPH.py:105-126): delta_i = sum_j V_j (v_i - v_j) . grad W_ij over every neighbour (fluid and rigid
    alike), rho*_i = max(rho_i / rho0 + dt delta_i, 1) for fluid i.  Returns dict: delta, delta_mag = sum_j sum_c |V_j dv_c grad W_c|,
    delta_amp, rho_star, bound (of rho*: dt (C1 mag + C2 amp) + 4 u (rho_i / rho0 + dt |delta|): the division 1 (2 in the fast build),
    x dt 1, the addition 1; max() is 1-Lipschitz, so a row whose interval straddles the clamp is accepted on either side), n_nbr.
    The sum is also D rho / Dt before its clamp at 0 and the neighbour-count rule (:66-101): bound C1 mag + C2 amp."""
    x = x.astype(np.float64)
    vv = (v_stale if mutant == "stale_velocity" else v).astype(np.float64)
    n = len(x)
    h, rho0, dt = params["h"], params["rho0"], params["dt"]
    i, j, R, r = _pairs(x, mat, h)
    keep = r <= h
    i, j, R, r = i[keep], j[keep], R[keep], r[keep]
    s, s_amp = kernel_grad_scale(r, h)
    vl = vol.astype(np.float64)
    prod = (vv[i] - vv[j]) * R
    delta = _sum(i, n, (vl[j] * s) * prod.sum(axis=1))
    mag = _sum(i, n, (vl[j] * np.abs(s)) * np.abs(prod).sum(axis=1))
    amp = _sum(i, n, (vl[j] * s_amp) * np.abs(prod).sum(axis=1))
    fluid = mat == 1
    base = np.where(fluid, rho.astype(np.float64) / rho0, 1.0)
    raw = base + (1.0 if mutant == "dt_left_out" else dt) * delta
    star = raw if mutant == "no_clamp_at_1" else np.maximum(raw, 1.0)
    bound = dt * (C1 * mag + C2 * amp) + 4 * U * (base + dt * np.abs(delta))
    return dict(delta=delta, delta_mag=mag, delta_amp=amp, raw=raw, rho_star=np.where(fluid, star, 0.0), bound=bound,
                n_nbr=np.bincount(i, minlength=n))


def pcisph_rho_star_f64(x, x_pred, vol, mat, params, mutant=None):
    """compute_density_star (PCISPH.py:33-62): ret_i = sum_j V_j W(|x*_i - y_j|) for fluid i over the neighbours j of the CURRENT
    positions (for_all_neighbors walks particle_positions: |x_i - x_j| < h), y_j = x*_j (predicted) for a fluid j and x_j (current)
    for a rigid j -- no self term --, rho*_i = ret_i rho0, and the error's term max(0, ret_i - 1).  W at the predicted distance may
    see distances beyond h (zero) and misses pairs that come within h only in the prediction.  Returns dict: ret, rho_star, mag, mag_amp,
    extra (pairs whose current distance is within 4 u h of h, at their predicted-distance term), bound (of rho*: rho0 (C1 mag + C2
    mag_amp + extra) + u rho*), n_terms, left (current neighbours at a predicted distance >= h), pairs."""
    x, xp = x.astype(np.float64), x_pred.astype(np.float64)
    n = len(x)
    h, rho0 = params["h"], params["rho0"]
    vl = vol.astype(np.float64)
    y = np.where((mat == 1)[:, None] | (mutant == "rigid_at_predicted"), xp, x)
    src = y if mutant == "neighbours_by_predicted" else x
    i, j, _, r_cur = _pairs(src, mat, h)
    keep = r_cur < h
    edge = (np.abs(r_cur - h) <= 4 * U * h) & (mutant is None)
    keep_any = keep | edge
    i, j, r_cur, keep, edge = i[keep_any], j[keep_any], r_cur[keep_any], keep[keep_any], edge[keep_any]
    rp = r_cur if mutant == "w_at_current" else np.linalg.norm(xp[i] - y[j], axis=1)
    w, w_amp = kernel_w(rp, h)
    t = vl[j] * w
    ret = _sum(i, n, np.where(keep, t, 0.0))
    mag, mag_amp, extra = _sum(i, n, t), _sum(i, n, vl[j] * w_amp), _sum(i, n, np.where(edge, t, 0.0))
    fluid = mat == 1
    star = np.where(fluid, ret * rho0, 0.0)
    bound = rho0 * (C1 * mag + C2 * mag_amp + extra) + U * star
    return dict(ret=ret, rho_star=star, mag=mag, mag_amp=mag_amp, extra=extra, bound=bound, n_terms=np.bincount(i, minlength=n),
                left=int((keep & (rp >= h)).sum()), pairs=dict(i=i, j=j, r_cur=r_cur, r_pred=rp))


def pcisph_entered(x, x_pred, mat, h):
    """pairs (i fluid) that are NO neighbours at the current positions and within h at the predicted ones (rigid j: current)"""
    x, xp = x.astype(np.float64), x_pred.astype(np.float64)
    y = np.where((mat == 1)[:, None], xp, x)
    i, j, _, rp = _pairs(y, mat, h)
    r_cur = np.linalg.norm(x[i] - x[j], axis=1)
    return int(((rp < h) & (r_cur >= h)).sum())


def pcisph_error_f64(res, mat):
    """density_error (PCISPH.py:40-45): mean over the fluid particles of max(0, ret - 1).  Returns (mean, bound): max() is 1-Lipschitz,
    so every row adds at most its bound / rho0 (only rows that can reach 1 at all), and an f32 sum of n values in any order, the
    subtraction and the division add at most (n + 2) u of the sum of the magnitudes."""
    fl = mat == 1
    nf = int(fl.sum())
    rb = res["bound"][fl] / (res["rho_star"][fl] / np.maximum(res["ret"][fl], 1e-300)) + U
    ret = res["ret"][fl]
    e = np.maximum(0.0, ret - 1.0)
    reach = ret + rb > 1.0
    return e.sum() / nf, (rb[reach].sum() + (nf + 2) * U * (e.sum() + rb[reach].sum())) / nf


def pcisph_pressure_f64(p_prev, rho_star, k, rho0, mutant=None, contracted=False):
    """update_pressure (PCISPH.py:66-71): p = max(0, p + k (rho0 - rho*)).  Returns (p, bound): the subtraction, the product and the
    addition are three roundings (an fma saves one): 3 u (|p_prev| + |k (rho0 - rho*)|); max() is 1-Lipschitz.  contracted (the fast
    build, -ffp-contract=fast): PcisphRhoStarPass::finish computes rho* = sum rho0 and rho0 - rho* side by side, and the compiler may
    contract the two into fma(-sum, rho0, rho0): the pressure then comes from the UNROUNDED rho*, which lies within u rho* of the
    stored one -- where rho* is close to rho0 that is far more than 3 u of the difference -- so + |k| u rho* (found by the first GPU
    run of tests/test_hip_pressure_solve.py: 9709 times the three-rounding bound on a row 0.03 kg / m^3 off rho0; the strict build is
    held to the bits instead)."""
    p0, rs = p_prev.astype(np.float64), rho_star.astype(np.float64)
    d = float(k) * (rho0 - rs)
    p = p0 + d
    if mutant != "no_clamp_at_0":
        p = np.maximum(p, 0.0)
    return p, 3 * U * (np.abs(p0) + np.abs(d)) + (abs(float(k)) * U * np.abs(rs) if contracted else 0.0)


def pcisph_k_f64(params):
    """compute_pcisph_k (PCISPH.py:129-151): -0.5 / (dt V0)^2 / (|sum grad W|^2 + sum |grad W|^2) over the lattice of pitch 0.97 diameter
    inside the support radius.  Returns (k, relative bound): each gradient 14 roundings, squared and summed over P points: (2 x 14 + P
    + 6) u, plus the f32 roundings of dt, V0 and the lattice pitch (3 + 3 u, the pitch through the conditioning of |grad W|^2, <= 8)."""
    h, dt, V0, dia = params["h"], params["dt"], params["V0"], params["diameter"]
    pitch = dia * 0.97
    m = int(h / pitch) + 1
    ax = np.arange(-m, m + 1) * pitch
    P = -np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    r = np.linalg.norm(P, axis=1)
    P, r = P[r < h], r[r < h]
    g = kernel_grad_scale(r, h)[0][:, None] * P
    den = (g.sum(axis=0) ** 2).sum() + (g * g).sum()
    return -0.5 / (dt * V0) ** 2 / den, (28 + len(P) + 6 + 6 + 8 * 3) * U


def predicted_f64(x, v0, a_np, a_p, dt):
    """compute_predicted_velocity / _position (PCISPH.py:19-29; init_step :161-162 with a_p = 0): v* = v0 + dt (a_np + a_p) -- the inner
    addition, the product and the outer addition: 3 u (|v0| + dt (|a_np| + |a_p|)) -- and x* = x + dt v* from a GIVEN v*: 2 u (|x| + dt
    |v*|).  Returns (v*, bound) and a function (v*_given) -> (x*, bound)."""
    x, v0, a_np, a_p = (np.asarray(a, np.float64) for a in (x, v0, a_np, a_p))
    vs = v0 + dt * (a_np + a_p)
    vb = 3 * U * (np.abs(v0) + dt * (np.abs(a_np) + np.abs(a_p)))

    def position(v_star):
        v_star = np.asarray(v_star, np.float64)
        return x + dt * v_star, 2 * U * (np.abs(x) + dt * np.abs(v_star))
    return vs, vb, position


# ---- liveness: a scene change must not hollow the checks out

def assert_alive_dfsph(res, star, drho_positive, fl, rigid):
    """`res`: dfsph_correction_f64; `star`: the rho* the kappas came from (or None for the divergence solve); `drho_positive`: rows
    with D rho / Dt > 0 (or None for the density solve)"""
    p = res["pairs"]
    assert res["n_nbr"].max() <= N_MAX, "more summed terms in a row than the derivation of C1 allows"
    if star is not None:
        assert int((star[fl] > 1).sum()) >= 200, "fluid rows with rho* > 1"
    if drho_positive is not None:
        assert int(drho_positive[fl].sum()) >= 200, "fluid rows with D rho / Dt > 0"
    rows_acc = np.zeros(len(fl), bool)
    rows_acc[p["i"][p["accepted"]]] = True
    assert int((p["skipped_zero"] & rows_acc[p["i"]]).sum()) >= 100, "pairs skipped by the threshold next to accepted ones"
    assert int((res["n_nbr"][fl] < 20).sum()) >= 50, "fluid rows with fewer than 20 neighbours"
    assert int(p["ambiguous"].sum()) <= 0.01 * int(p["accepted"].sum()), "pairs the threshold cannot decide: more than 1 % of the accepted"
    if rigid:
        live = p["dynamic_j"] & (np.abs(p["term"]).max(axis=1) > 0)
        assert int(live.sum()) >= 50, "fluid - dynamic rigid pairs with a nonzero term"


def assert_alive_pcisph(res, entered):
    assert res["n_terms"].max() <= N_MAX, "more summed terms in a row than the derivation of C1 allows"
    assert res["left"] >= 50, ("current neighbours at a predicted distance >= h", res["left"])
    assert entered >= 50, ("non-neighbours at a predicted distance < h", entered)


# ---- the scene: nonpressure_terms.scene made to compress -- as it stands its densities stay below rho0 almost everywhere (12 rows with
# rho* > 1), and the PCISPH rho*, which has no self term, never reaches rho0: no kappa, no pressure.  Four times the velocity noise
# (2 m/s), a convergence of 45 / s towards the centre of the block and dt = 1 ms give, measured with the oracle (rigid scene / twin;
# tests/test_pressure_solve_host.py asserts the counts):
#   DFSPH, K = 0: 615 / 592 rows with kappa > 0, 308 / 279 with rho* > 1 after the correction, 481 / 358 with D rho / Dt > 0 after the
#     divergence correction, 9828 / 8402 (1254 / 762) pairs skipped next to accepted ones, 63 / 149 rows below 20 neighbours, 200
#     pairs with the cube.  After one step (K = 1) the compression has filled the edges of the block: 41 rows below 20 neighbours in
#     the rigid scene, fewer than the 50 asked for -- hence K = 0 for DFSPH: the state prepare() leaves.
#   PCISPH, K = 1: 339 / 329 rows with ret > 1 (a pressure) in the first round, 822 / 242 neighbours that leave the support radius in
#     the prediction, 9000 / 8990 pairs that enter it.  At K = 0 no row reaches ret > 1.
K_STEPS = {"dfsph": 0, "pcisph": 1}
NOISE, CONVERGE, DT = 4.0, 45.0, 1e-3


def scene(method, rigid=True, layers=None):
    from tests import nonpressure_terms as T
    sc = T.scene(method, rigid=rigid, noise=NOISE, converge=CONVERGE, dt=DT, layers=layers)
    sc["pd"]["fixed_iterations"] = 1
    return sc


# ---- the comparisons, shared by the CPU tests (oracle) and the GPU tests (library): every array by the same particle order

def _frac(err, bound):
    """worst err / bound; a row with a zero bound has to be exact"""
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(f.max()) if f.size else 0.0


def check_dfsph_solve(sc, s0, s1, wrench, mode, tiny_wrench=0.0):
    """One solve with ONE fixed iteration (rho* / D rho / Dt pass, kappa, one correction, the pass again) from the state s0 (x, v, rho,
    vol, mat, dyn, obj) to s1 (v, `kappa`: the kappa the correction used, `after`: the rho* (mode 1) or D rho / Dt (mode 0) stored
    last), `wrench` = (forces, torques) accumulated over it.  Asserts the liveness of the state and every bound; returns the worst
    fractions."""
    from tests import helpers as H
    from tests import nonpressure_terms as T
    P = sc["params"]
    fl = s0["mat"] == 1
    res = dfsph_correction_f64(s0["x"], s1["kappa"], s0["rho"], s0["vol"], s0["mat"], s0["dyn"], s0["obj"], sc["com"], P, mode)
    assert_alive_dfsph(res, s1["after"] if mode == 1 else None, (s1["after"] > 0) if mode == 0 else None, fl, sc["rigid"])
    if mode == 1:
        assert int((s1["kappa"][fl] > 0).sum()) >= 200, "fluid rows whose rho* before the correction was > 1"
    fr = {}
    got = s1["v"].astype(np.float64) - s0["v"].astype(np.float64)
    fr["dv"] = _frac(np.abs(got - res["dv"])[fl], correction_bound(res, mode, s0["v"])[fl])
    assert fr["dv"] <= 1, fr
    assert np.array_equal(s1["v"][~fl], s0["v"][~fl]), "velocity of a non-fluid row changed"
    if sc["rigid"]:
        w = res["wrench"]
        for part, g in (("force", wrench[0]), ("torque", wrench[1])):
            wb = T.wrench_bound(w, part)[T.BODY] + tiny_wrench + U * np.abs(w[part][T.BODY])
            fr["wrench " + part] = _frac(np.abs(g - w[part])[T.BODY], wb)
            assert fr["wrench " + part] <= 1, (fr, g[T.BODY], w[part][T.BODY])
    rs = dfsph_rho_star_f64(s0["x"], s1["v"], s0["rho"], s0["vol"], s0["mat"], P)
    after = s1["after"].astype(np.float64)
    if mode == 1:
        fr["rho*"] = _frac(np.abs(after - rs["rho_star"])[fl], rs["bound"][fl])
        assert fr["rho*"] <= 1, fr
        assert int(((rs["raw"] < 1) & fl).sum()) >= 100 and int(((rs["raw"] > 1) & fl).sum()) >= 200, "both sides of the clamp at 1"
    else:
        val, mag, n_lo, n_hi = H.dfsph_density_derivative_f64(s0["x"], s1["v"], s0["vol"], s0["mat"], P["h"])
        assert (np.abs(val - rs["delta"]) <= 1e-9 * (mag + 1e-300))[fl].all() and (np.abs(mag - rs["delta_mag"]) <= 1e-9 * mag)[fl].all()
        bound = C1 * rs["delta_mag"] + C2 * rs["delta_amp"]
        low, sure = fl & (n_hi < 20), fl & (n_lo >= 20)
        assert low.sum() >= 50 and (after[low] == 0).all(), "D rho / Dt below 20 neighbours"
        e = np.abs(after - np.maximum(val, 0.0))
        fr["D rho / Dt"] = _frac(e[sure], bound[sure])
        assert fr["D rho / Dt"] <= 1, fr
        either = fl & ~low & ~sure
        assert ((after[either] == 0) | (e[either] <= bound[either])).all()
    return fr


def check_pcisph_init(sc, s0, a_np, s1):
    """init_step (PCISPH.py:154-162): s0 (x, v: the velocity at the start of the step, mat), a_np, s1 (pvel, ppos, prs, pacc)"""
    P = sc["params"]
    fl = s0["mat"] == 1
    vs, vb, position = predicted_f64(s0["x"], s0["v"], a_np, 0.0 * a_np.astype(np.float64), P["dt"])
    fr = {"init v*": _frac(np.abs(s1["pvel"] - vs)[fl], vb[fl])}
    xs, xb = position(s1["pvel"])
    fr["init x*"] = _frac(np.abs(s1["ppos"] - xs)[fl], xb[fl])
    assert max(fr.values()) <= 1, fr
    assert (s1["prs"] == 0).all() and (s1["pacc"] == 0).all()
    return fr


def check_pcisph_round(sc, s0, a_np, ppos_before, prs_before, s1, s2, err, k, strict, tag):
    """One iteration of refine (PCISPH.py:110-118) in its two halves: from the predicted positions `ppos_before` and pressures
    `prs_before` to s1 (star, prs) with the density error `err`, then to s2 (pacc, pvel, ppos).  s0: x, v (start of the step), rho, mass,
    vol, mat.  k: pcisph_k as the f32 the solver holds.  strict: the pressure update bit for bit (no contraction in that build)."""
    from tests import helpers as H
    P = sc["params"]
    fl = s0["mat"] == 1
    fr = {}
    res = pcisph_rho_star_f64(s0["x"], ppos_before, s0["vol"], s0["mat"], P)
    assert_alive_pcisph(res, pcisph_entered(s0["x"], ppos_before, s0["mat"], P["h"]))
    fr[tag + " rho*"] = _frac(np.abs(s1["star"] - res["rho_star"])[fl], res["bound"][fl])
    assert fr[tag + " rho*"] <= 1, fr
    p, pb = pcisph_pressure_f64(prs_before, s1["star"], k, P["rho0"], contracted=not strict)
    fr[tag + " p"] = _frac(np.abs(s1["prs"] - p)[fl], pb[fl])
    assert fr[tag + " p"] <= 1, fr
    if strict:
        k32, r32 = np.float32(k), np.float32(P["rho0"])
        p32 = prs_before[fl] + k32 * (r32 - s1["star"][fl])
        assert p32.dtype == np.float32
        np.testing.assert_array_equal(s1["prs"][fl], np.where(p32 < 0, np.float32(0), p32))
    mean, mb = pcisph_error_f64(res, s0["mat"])
    fr[tag + " error"] = _frac(np.abs(np.float64(err) - mean)[None], np.array([mb]))
    assert fr[tag + " error"] <= 1, (fr, err, mean, mb)
    a_p, mag, mag_amp = H.wcsph_pressure_accel_f64(s0["x"], s0["rho"], s1["prs"], s0["mass"], s0["vol"], s0["mat"], P["h"], P["rho0"])
    fr[tag + " a_p"] = _frac(np.abs(s2["pacc"] - a_p)[fl], (1e-5 * mag + 5e-7 * mag_amp)[fl])
    assert fr[tag + " a_p"] <= 1, fr
    vs, vb, position = predicted_f64(s0["x"], s0["v"], a_np, s2["pacc"], P["dt"])
    fr[tag + " v*"] = _frac(np.abs(s2["pvel"] - vs)[fl], vb[fl])
    xs, xb = position(s2["pvel"])
    fr[tag + " x*"] = _frac(np.abs(s2["ppos"] - xs)[fl], xb[fl])
    assert max(fr.values()) <= 1, fr
    return fr, dict(positive_pressures=int((s1["prs"][fl] > 0).sum()), clamped=int(((s1["prs"] == 0) & fl).sum()),
                    a_p_alive=int((np.abs(a_p[fl]).max(axis=1) > 0).sum()))
