"""The IISPH terms of the reference (SPH/fluid_solvers/IISPH.py) restated in float64 over a KD-tree pair list -- independent of the
oracle and of the device code -- with backward-error bounds in the style of helpers.wcsph_pressure_accel_f64: every pair term of a
sum carries a relative error eps_j = 1e-5 + 5e-7 amp_j in ANY f32 evaluation of it (~12 roundings of the term plus a sum of <= 64
terms, (12 + 64) u = 4.5e-6 < 1e-5; amp_j = |q W'' / W'| is the kernel gradient's conditioning in q = r / h, which ~3 roundings
reach), so |sum_f32 - sum| <= sum_j |term_j| eps_j.  The bounds are relative to sum |terms|, not to |sum|: they hold however badly a
scene cancels.

Rigid neighbours take the library's definition of the one term the reference leaves undefined (IISPH.py:40-44): rho_i^2 in place of
particle_densities_star[p_i]^2."""
import numpy as np

from tests.helpers import _pair_list

U = 2.0 ** -24
OMEGA = 0.2


def _pairs(x, mat, h, rows):
    """Pairs (o, i, j) of fluid particles i (rows: a sample, o = position in rows) with every neighbour j, kernel gradient
    grad W_ij (base_solver.py:81) and the per-term relative error eps of any f32 evaluation of it."""
    x = x.astype(np.float64)
    o, i, j = _pair_list(x, h, rows)
    R = x[i] - x[j]
    r = np.linalg.norm(R, axis=1)
    keep = (mat[i] == 1) & (r > 1e-5) & (r <= h) & ((mat[j] == 1) | (mat[j] == 2))
    o, i, j, R, r = o[keep], i[keep], j[keep], R[keep], r[keep]
    q = r / h
    kg = 6.0 * (8.0 / np.pi) / h ** 3
    sc = np.where(q <= 0.5, kg * q * (3 * q - 2), -kg * (1 - q) ** 2) / (r * h)
    amp = np.where(q <= 0.5, np.abs(6 * q - 2) / np.maximum(np.abs(3 * q - 2), 1e-300), 2 * q / np.maximum(1 - q, 1e-300))
    return o, i, j, sc[:, None] * R, 1e-5 + 5e-7 * amp


def _sum(o, n, t):
    t = np.asarray(t, np.float64)
    if t.ndim == 1:
        return np.bincount(o, t, minlength=n)
    return np.stack([np.bincount(o, t[:, c], minlength=n) for c in range(t.shape[1])], axis=1)


def prepare_terms(x, v, rho, vol, mat, h, rho0, dt, rows=None):
    """compute_dii (IISPH.py:18-44), compute_aii (:47-68), compute_density_star (:71-90) for the fluid particles `rows` (all if
    None).  v: the velocities after the non-pressure update (v*).  Returns dict of values and bounds (rows follow `rows`):
    dii (n,3) / dii_b, aii / aii_b, rho_star / rho_star_b."""
    n = len(x) if rows is None else len(rows)
    o, i, j, g, eps = _pairs(x, mat, h, rows)
    rho = rho.astype(np.float64)
    m0 = rho0 * vol.astype(np.float64)
    fl_j = (mat[j] == 1)[:, None]
    # dii: fluid neighbour -m0_j grad W / rho_j^2 ; rigid neighbour -m0_j grad W / rho_i^2 (the library's definition)
    t_d = -(m0[j] / np.where(fl_j[:, 0], rho[j] ** 2, rho[i] ** 2))[:, None] * g
    dii = _sum(o, n, t_d)
    dii_b = _sum(o, n, np.abs(t_d) * eps[:, None])
    # aii = dt^2 sum_j m0_j (dii_i - m0_i / rho_i^2 grad W) . grad W (rigid and fluid neighbours alike)
    dji = (m0[i] / rho[i] ** 2)[:, None] * g
    dd = dii[o] - dji
    t_a = m0[j] * (dd * g).sum(axis=1)
    aii = dt * dt * _sum(o, n, t_a)
    # error: the pair term's own roundings (relative to sum_c |dd_c g_c|) + the error of dii_i entering every term
    t_a_mag = m0[j] * (np.abs(dd) * np.abs(g)).sum(axis=1)
    aii_b = dt * dt * (_sum(o, n, t_a_mag * 2 * eps) + _sum(o, n, (dii_b[o] * np.abs(g)).sum(axis=1) * m0[j]))
    # rho* = rho_i + dt sum_j m0_j (v_i - v_j) . grad W
    vv = v.astype(np.float64)
    t_r = m0[j] * ((vv[i] - vv[j]) * g).sum(axis=1)
    t_r_mag = m0[j] * (np.abs(vv[i] - vv[j]) * np.abs(g)).sum(axis=1)
    ri = rho if rows is None else rho[np.asarray(rows)]
    rho_star = ri + dt * _sum(o, n, t_r)
    rho_star_b = 2 * U * np.abs(ri) + dt * _sum(o, n, t_r_mag * 2 * eps)
    return dict(dii=dii, dii_b=dii_b, aii=aii, aii_b=aii_b, rho_star=rho_star, rho_star_b=rho_star_b)


def iteration_terms(x, rho, vol, mat, h, rho0, dt, p_prev, dii, dij_pj, rows=None):
    """One iteration of refine from f32 inputs: compute_dij_pj (IISPH.py:125-146) from the pressures p_prev, and compute_sum_i
    (:148-183) from the GIVEN dij_pj (what the evaluation under test stored) with w_j = dii_j p_j + dij_pj_j.  Returns dict:
    dij_pj (n,3) / dij_pj_b, sum_i / sum_i_b."""
    n = len(x) if rows is None else len(rows)
    o, i, j, g, eps = _pairs(x, mat, h, rows)
    rho = rho.astype(np.float64)
    m0 = rho0 * vol.astype(np.float64)
    p = p_prev.astype(np.float64)
    fl_j = mat[j] == 1
    t_d = np.where(fl_j, -m0[j] / rho[j] ** 2 * p[j], 0.0)[:, None] * g
    dpj = _sum(o, n, t_d)
    dpj_b = _sum(o, n, np.abs(t_d) * eps[:, None])
    dij = dij_pj.astype(np.float64)
    w = dii.astype(np.float64) * p[:, None] + dij
    w_b = 2 * U * (np.abs(dii.astype(np.float64) * p[:, None]) + np.abs(dij))   # the f32 product and sum forming w_j
    cp = (m0[i] / rho[i] ** 2 * p[i])[:, None] * g
    tv = np.where(fl_j[:, None], dij[i] - w[j] + cp, dij[i])
    t_s = m0[j] * (tv * g).sum(axis=1)
    t_s_mag = m0[j] * ((np.abs(dij[i]) + np.where(fl_j[:, None], np.abs(w[j]) + np.abs(cp), 0.0)) * np.abs(g)).sum(axis=1)
    t_s_w = m0[j] * (np.where(fl_j[:, None], w_b[j], 0.0) * np.abs(g)).sum(axis=1)
    sum_i = dt * dt * _sum(o, n, t_s)
    sum_i_b = dt * dt * (_sum(o, n, t_s_mag * 2 * eps) + _sum(o, n, t_s_w))
    return dict(dij_pj=dpj, dij_pj_b=dpj_b, sum_i=sum_i, sum_i_b=sum_i_b)


def pressure_update(p_prev, aii, rho_star, sum_i, rho0):
    """update_pressure (IISPH.py:98-123) in float64 from f32 inputs; returns (p, bound, error contribution per particle)."""
    p_prev, aii, rs, si_ = (a.astype(np.float64) for a in (p_prev, aii, rho_star, sum_i))
    si = rho0 - rs
    live = np.abs(aii) > 1e-10
    safe = np.where(live, aii, 1.0)
    raw = (1 - OMEGA) * p_prev + OMEGA / safe * (si - si_)
    p = np.where(live, np.maximum(0.0, raw), 0.0)
    # a handful of roundings of each operand: the subtraction rho0 - rho* is exact in f32 near rho0, the rest is ~6 u
    bound = np.where(live, 8 * U * ((1 - OMEGA) * np.abs(p_prev) + np.abs(OMEGA / safe) * (np.abs(si) + np.abs(si_) + 2 * U * np.abs(rs))), 0.0)
    err = np.where(p > 1e-10, aii * p + si_ - si, 0.0)
    return p, bound, err
