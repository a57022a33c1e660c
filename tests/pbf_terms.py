"""The PBF terms of the reference (SPH/fluid_solvers/PBF.py) restated in float64 -- independent of the device code -- with the
stale-grid neighbour set of base_container.py:550-560: particle j is a candidate of particle i when the cell the step's sort filed j
in lies within one cell of pos_to_index(x_i) (the CURRENT position, truncated like the reference's cast) on every axis and inside
the grid; it is a neighbour when |x_i - x_j| < dh with the current positions of both.

Bounds in the style of tests/iisph_terms.py: every pair term carries a relative error eps = 1e-5 in any f32 evaluation, plus the
conditioning of the spiky gradient in r (|2 r / (h - r)| roundings of r) and of poly6 (|6 r^2 / (h^2 - r^2)|); the bound of a sum
is sum_j |term_j| eps_j, relative to the sum of |terms|, so it holds however badly a sum cancels."""
import numpy as np

POLY6 = 315.0 / 64.0 / np.pi
SPIKY = -45.0 / np.pi
LAMBDA_EPS, CORR_K, CORR_DQ = 100.0, 0.001, 0.3


def cells(x, grid_size):
    """base_container.py:468 pos_to_index: an f32 quotient (as the reference and the device divide), truncated towards zero."""
    q = np.asarray(x, np.float32) / np.float32(grid_size)
    q = np.where(np.isfinite(q), q, -2.0)   # (a non-finite position lies in no cell)
    return np.trunc(np.clip(q, -2.0, 1e9)).astype(np.int64)


def stale_pairs(x, sort_x, h, grid_size, grid_num, rows):
    """(o, i, j, R, r) for every fluid-or-not target i in `rows` (o = position in rows): j != i, |x_i - x_j| < h, j's sort cell
    within one cell of i's current cell and inside the grid."""
    from scipy.spatial import cKDTree
    x = np.asarray(x, np.float64)
    rows = np.asarray(rows)
    gn = np.asarray(grid_num)
    cj = cells(sort_x, grid_size)
    ci = cells(x[rows], grid_size)
    # particles with a non-finite position (the reference's PBF can produce them: a fluid neighbour left with rho = 0 by the last
    # refine divides the next step's viscosity by zero) are nobody's neighbour: their distance test fails
    fin = np.nonzero(np.isfinite(x).all(axis=1))[0]
    lists = cKDTree(x[fin]).query_ball_point(x[rows], h * (1 + 1e-6))
    cnt = np.array([len(l) for l in lists])
    o = np.repeat(np.arange(len(rows)), cnt)
    j = fin[np.concatenate([np.asarray(l, np.int64) for l in lists])] if len(lists) else np.zeros(0, np.int64)
    i = rows[o]
    R = x[i] - x[j]
    r = np.linalg.norm(R, axis=1)
    inside = np.all((cj[j] >= 0) & (cj[j] < gn), axis=1)
    near = np.all(np.abs(cj[j] - ci[o]) <= 1, axis=1)
    keep = (i != j) & (r < h) & inside & near
    return o[keep], i[keep], j[keep], R[keep], r[keep]


def recentred(x, sort_x, grid_size, grid_num, mat):
    """Fluid particles whose current cell differs from their sort cell (or lies outside the grid)."""
    c, s = cells(x, grid_size), cells(sort_x, grid_size)
    inside = np.all((c >= 0) & (c < np.asarray(grid_num)), axis=1)
    return int(np.count_nonzero((mat == 1) & ~(inside & np.all(c == s, axis=1))))


def _w(r, h):
    w = np.where((r > 0) & (r < h), POLY6 * ((h * h - r * r) / h ** 3) ** 3, 0.0)
    amp = np.abs(6 * r * r / np.maximum(h * h - r * r, 1e-300))
    return w, 1e-5 + 1e-6 * amp


def _g(R, r, h):
    s = np.where((r > 0) & (r < h), SPIKY * ((h - r) / h ** 3) ** 2 / np.maximum(r, 1e-300), 0.0)
    amp = np.abs(2 * r / np.maximum(h - r, 1e-300))
    return s[:, None] * R, 1e-5 + 1e-6 * amp


def _sum(o, n, t):
    t = np.asarray(t, np.float64)
    if t.ndim == 1:
        return np.bincount(o, t, minlength=n)
    return np.stack([np.bincount(o, t[:, c], minlength=n) for c in range(t.shape[1])], axis=1)


def density_lambda(x, sort_x, vol, mass, mat, h, grid_size, grid_num, rho0, rows):
    """compute_density (base_solver.py:522, self term V_i W(0) = 0) + compute_lambda (PBF.py:68-102) for the fluid particles
    `rows`.  Returns rho, rho_b (bound), lam, lam_b, pairs (accepted pairs of the walk)."""
    n = len(rows)
    o, i, j, R, r = stale_pairs(x, sort_x, h, grid_size, grid_num, rows)
    vol = np.asarray(vol, np.float64); mass = np.asarray(mass, np.float64)
    w, ew = _w(r, h)
    rho = rho0 * _sum(o, n, vol[j] * w)
    rho_b = rho0 * _sum(o, n, np.abs(vol[j] * w) * ew) + 1e-6 * np.abs(rho)
    g, eg = _g(R, r, h)
    fl = mat[j] == 1
    rg = mat[j] == 2
    coef = np.where(fl, mass[j] / rho0, np.where(rg, vol[j] * rho[o] / rho0, 0.0))
    gg = coef[:, None] * g
    s1 = _sum(o, n, gg)
    s2 = _sum(o, n, (gg * gg).sum(axis=1))
    den = s2 + (s1 * s1).sum(axis=1) + LAMBDA_EPS
    c = rho / rho0 - 1.0
    lam = -c / den
    # error: of the constraint (rho's bound) and of the denominator (relative eps of each squared term, doubled)
    s1_b = _sum(o, n, np.abs(gg) * eg[:, None])
    den_b = _sum(o, n, 2 * (gg * gg).sum(axis=1) * eg) + 2 * (np.abs(s1) * s1_b).sum(axis=1) + 1e-6 * den
    lam_b = (rho_b / rho0) / den + np.abs(c) * den_b / den ** 2 + 1e-6 * np.abs(lam) + 1e-9
    return dict(rho=rho, rho_b=rho_b, lam=lam, lam_b=lam_b, pairs=len(o))


def fix_delta(x, sort_x, lam, vol, mass, mat, h, grid_size, grid_num, rho0, rows):
    """fix_position (PBF.py:104-131), Jacobi: the displacement dx_i of the fluid particles `rows`, with its bound."""
    n = len(rows)
    o, i, j, R, r = stale_pairs(x, sort_x, h, grid_size, grid_num, rows)
    lam = np.asarray(lam, np.float64); vol = np.asarray(vol, np.float64); mass = np.asarray(mass, np.float64)
    g, eg = _g(R, r, h)
    w, ew = _w(r, h)
    wq, _ = _w(np.array([CORR_DQ * h]), h)
    sc = -CORR_K * (w / wq[0]) ** 4
    fl = mat[j] == 1
    rg = mat[j] == 2
    k = np.where(fl, lam[i] + lam[j] + sc, np.where(rg, 2 * lam[i] + sc, 0.0))
    m = np.where(fl, mass[j], np.where(rg, vol[j] * rho0, 0.0))
    t = (k * m)[:, None] * g / rho0
    dx = _sum(o, n, t)
    mag = (np.abs(lam[i]) + np.abs(lam[j]) * fl + np.abs(sc)) * m
    db = _sum(o, n, (mag[:, None] * np.abs(g) / rho0) * (eg + 4 * ew)[:, None]) + 1e-9
    return dict(dx=dx, dx_b=db, pairs=len(o))
