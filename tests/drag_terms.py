"""The air drag of Gissler, Band, Peer, Ihmsen, Teschner 2017 restated in float64 -- written from the formulas of
include/sph_hip.h, independent of the device code -- with forward-error bounds for every stored term, the mutants that every
comparison has to catch, and the test scenes.

Constants (water in air): sigma = 0.0724, mu_l = 0.00102, mu_a = 1.845e-5, C_F = 1/3, C_k = 8, C_d = 5, C_b = 0.5, n_full = 38;
d = 2 r, rho_l = density0, rho_a the air's density:
    L = cbrt(3 / (4 pi)) d;  1/t_d = C_d mu_l / (2 rho_l L^2);  omega^2 = C_k sigma / (rho_l L^3) - 1/t_d^2
    t_max = -2 (atan(sqrt(t_d^2 omega^2)) - pi) / omega;  c_def = 1 - exp(-t_max / t_d) (cos(omega t_max) + sin(omega t_max) / (omega t_d))
    y_coeff = C_F (rho_a L / sigma) c_def / (C_k C_b);  n23 = 2 n_full / 3
Per active fluid particle i, j over its fluid neighbours (r_ij < h, self excluded):
    v_rel = u - v_i;  s2 = |v_rel|^2;  s2 < 1e-6: everything 0
    s = sqrt(s2);  e = v_rel / s;  y = min(s2 y_coeff, 1);  Re = 2 max(rho_a s L / mu_a, 0.1)
    C_sph = Re <= 1000 ? 24 / Re (1 + Re^(2/3) / 6) : 0.424;  C_liu = C_sph (1 + 2.632 y)
    f = min(n23, n_i) / n23;  C_D = (1 - f) C_liu + f;  A_drop = pi (L + C_b L y)^2;  A_un = (1 - f) A_drop + f d^2
    q = max_j e . (x_i - x_j) / |x_i - x_j| (>= 0);  w = clamp(1 - q, 0, 1);  a_drag = k / (2 m_i) rho_a s v_rel C_D w A_un

Bounds.  u = 2^-24 is the unit roundoff of one correctly rounded f32 operation, a constant rounded once from double, or an input
that is exact.  Every quantity carries an ABSOLUTE bound E, propagated to first order through the operations as the formulas are
written (rho = E / |value| where a relative bound is handier), times 1.02 for the second order; FAST = 4 u is what the fast build's
v_rcp_f32 / v_rsq_f32 may add where the strict build has a correctly rounded division or root (1-2 ulp, as the other *_terms.py take
them).  The inputs (positions, velocities, masses) are the device's own f32 values and exact.
    r_c = u_c - v_c            E_r = u |u_c| (the wind's rounding) + u |r_c|
    s2 = sum r_c^2             E = sum 2 |r_c| E_r + 3 u s2 (three products, two additions, all terms positive)
    s = sqrt(s2)               rho_s = rho_s2 / 2 + u
    e_c = r_c / s              E_e = E_r / s + |e_c| (rho_s + u [+ FAST: the walk takes v_rsq])
    y = min(s2 y_coeff, 1)     rho_y = rho_s2 + 2 u (constant, product); the clamp only lowers the error
    Re = 2 max(re_coeff s, .1) rho_Re = rho_s + 2 u
    Re^(1/3)                   rho = rho_Re / 3 + 7 u: the cube root is written out in plain f32 arithmetic (bit seed within 3.5 %, two
                               Halley steps that cube the error to 1.6e-14; what is left is the roundoff of the last step: t^3 with two
                               roundings enters the quotient with weights 1/3 and 2/3 (2 u), two sums, a division, a product, 4 u, + 1 u)
    Re^(2/3) = c c             rho = 2 rho_cbrt + u
    t = 1 + Re^(2/3) / 6       E_t = (Re^(2/3) / 6) (rho + u) + u t
    24 / Re                    rho = rho_Re + u [fast: + FAST + u]
    C_sph                      rho = rho_lead + E_t / t + u;  the constant branch: u.  C_sph is continuous at Re = 1000 and its relative
                               slope there is 0.37 per unit of relative change of Re, no more than inside the lower branch: a comparison
                               that rounding flips is covered by + 0.4 x 2 rho_Re within 2 rho_Re of 1000
    C_liu = C_sph p            p = 1 + 2.632 y: E_p = 2.632 y (rho_y + 2 u) + u p;  rho = rho_Csph + E_p / p + u
    f                          n_i >= n23: exactly 1 (n_i is an integer and n23 = 25.33: no rounding can flip it); else n_i / n23 or
                               n_i (1 / n23): 2 u f either way.  g = 1 - f: E_g = E_f + u g
    C_D = g C_liu + f          E = E_g C_liu + g C_liu (rho_Cliu + u) + E_f + u C_D
    rad = L + C_b L y          E = u L + C_b L y (rho_y + 2 u) + u rad;  A_drop = pi rad^2: rho = 2 rho_rad + 3 u
    A_un = g A_drop + f d^2    E = E_g A_drop + g A_drop (rho_Adrop + u) + E_f d^2 + 2 u f d^2 + u A_un
    q (the walk)               per pair dx_c = x_i,c - x_j,c (u each), dot = sum e_c dx_c (products u, two additions 2 u: 4 u relative to
                               sum |e_c dx_c| <= r), r^2 (2 u of the differences + 3 u: 5 u), its root (2.5 u + u), the quotient u; by
                               Cauchy-Schwarz sum_c E_e,c |dx_c| / r <= |E_e|:  E_q = |E_e| + 4 u + 4.5 u [fast: |E_e| + 4 u + 3.5 u + FAST]
                               -- absolute, for every pair, hence for their maximum.  Host records carry q as an input: E_q = 0.
    w = clamp(1 - q, 0, 1)     E_w = E_q + u + 2^-20: the device stores a w below 2^-20 (= 16 u, what E_q comes to) as 0, so that a
                               fully shielded particle feels no force whatever the rounding of q
    a_c = ((k rho_a / 2) s) ((C_D w) A_un) / m_i r_c
                               with K = a / w:  E_a = |K r_c| E_w + |a_c| (rho_s + rho_CD + rho_Aun + 7 u [+ FAST + u]) + |a_c / r_c| E_r
                               (7: the constant, four products, the division, the product with r_c)
n_i is an integer count and compared exactly.  That needs the same pairs on both sides: neighbour_terms() refuses its input with an
assertion if any fluid pair lies within 1e-5 h of h (the f32 rounding of r^2 and of h could decide it); likewise particle_f64 refuses
a record whose s2 lies within four bounds of the threshold 1e-6.  The scenes' jitter seeds are chosen so that no pair does, which
tests/test_drag_host.py checks on the CPU."""
import numpy as np

from tests.helpers import _pair_list, with_layers

U = 2.0 ** -24
FAST = 4 * U
SECOND_ORDER = 1.02
SIGMA, MU_L, MU_A, C_F, C_K, C_DAMP, C_B, N_FULL = 0.0724, 0.00102, 1.845e-5, 1.0 / 3.0, 8.0, 5.0, 0.5, 38.0
S2_MIN = 1e-6
W_FLUSH = 2.0 ** -20
RHO_AIR = 1.2041
GAP = 1e-5

PARTICLE_MUTANTS = ("vrel_sign", "wind_dropped", "n_full_for_n23", "cliu_without_y", "re_branch_swapped", "adrop_d_for_L",
                    "inv_m_dropped", "threshold_dropped")
WALK_MUTANTS = ("xj_minus_xi", "q_sum", "rigid_counted", "rigid_shielding")
MUTANTS = PARTICLE_MUTANTS + WALK_MUTANTS
RIGID_MUTANTS = ("rigid_counted", "rigid_shielding")   # need a boundary to differ at all
WIND_MUTANTS = ("wind_dropped",)                        # need a wind


def constants(radius, rho_l, rho_a=RHO_AIR):
    """dict(L, inv_td, omega2, t_max, c_def, y_coeff, n23, re_coeff, d)"""
    d = 2.0 * radius
    L = np.cbrt(3.0 / (4.0 * np.pi)) * d
    inv_td = C_DAMP * MU_L / (2.0 * rho_l * L ** 2)
    omega2 = C_K * SIGMA / (rho_l * L ** 3) - inv_td ** 2
    assert omega2 > 0, "omega^2 <= 0: the model does not apply"
    omega, td = np.sqrt(omega2), 1.0 / inv_td
    t_max = -2.0 * (np.arctan(np.sqrt(td ** 2 * omega2)) - np.pi) / omega
    c_def = 1.0 - np.exp(-t_max / td) * (np.cos(omega * t_max) + np.sin(omega * t_max) / (omega * td))
    y_coeff = C_F * (rho_a * L / SIGMA) * c_def / (C_K * C_B)
    return dict(L=L, inv_td=inv_td, omega2=omega2, t_max=t_max, c_def=c_def, y_coeff=y_coeff, n23=2.0 * N_FULL / 3.0,
                re_coeff=rho_a * L / MU_A, d=d)


def c_sphere(re, swapped=False):
    lower = 24.0 / re * (1.0 + re ** (2.0 / 3.0) / 6.0)
    return np.where((re > 1000.0) if swapped else (re <= 1000.0), lower, 0.424)


def particle_f64(v, m, n, q, radius, rho_l, k=1.0, rho_a=RHO_AIR, u=(0.0, 0.0, 0.0), mutant=None, fast=False, e_q=None, e_dir=False):
    """Everything behind the walk for records (v (n, 3), m, n_i, q): dict(a, w, cd, a_un, y, s, e and b_a, b_w, b_cd, b_a_un, b_y, b_e:
    the bounds; on: above the threshold).  e_q: the absolute bound q carries (None: 0, q is an input); e_dir: return only s, e, b_e
    (what the walk needs)."""
    K = constants(radius, rho_l, rho_a)
    v, m, n, q = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(m, np.float64), np.asarray(n, np.float64), np.asarray(q, np.float64)
    wind = np.zeros(3) if mutant == "wind_dropped" else np.asarray(u, np.float64)
    r = wind - v
    if mutant == "vrel_sign":
        r = -r
    E_r = U * np.abs(wind)[None, :] + U * np.abs(r)
    s2 = (r ** 2).sum(axis=1)
    E_s2 = (2 * np.abs(r) * E_r).sum(axis=1) + 3 * U * s2
    on = np.ones(len(s2), bool) if mutant == "threshold_dropped" else s2 >= S2_MIN
    if mutant != "threshold_dropped":
        assert (np.abs(s2 - S2_MIN) > 4 * E_s2).all(), "a record within four bounds of the threshold s2 = 1e-6"
    s2s = np.where(s2 > 0, s2, 1.0)
    rho_s2 = E_s2 / s2s
    s = np.sqrt(s2s)
    rho_s = rho_s2 / 2 + U
    e = r / s[:, None]
    E_e = E_r / s[:, None] + np.abs(e) * (rho_s + U + (FAST if fast else 0.0))[:, None]
    e = np.where(on[:, None], e, 0.0)
    E_e = np.where(on[:, None], E_e, 0.0) * SECOND_ORDER
    if e_dir:
        return dict(s=s, e=e, b_e=E_e, on=on)
    y = np.minimum(s2 * K["y_coeff"], 1.0)
    rho_y = rho_s2 + 2 * U
    E_y = y * rho_y
    re = 2.0 * np.maximum(K["re_coeff"] * s, 0.1)
    rho_re = rho_s + 2 * U
    c_sph = c_sphere(re, mutant == "re_branch_swapped")
    r23 = re ** (2.0 / 3.0)
    rho_r23 = 2 * (rho_re / 3 + 7 * U) + U
    t = 1.0 + r23 / 6.0
    E_t = (r23 / 6.0) * (rho_r23 + U) + U * t
    rho_lead = rho_re + U + ((FAST + U) if fast else 0.0)
    rho_low = rho_lead + E_t / t + U + np.where(np.abs(re - 1000.0) <= 2000.0 * rho_re, 0.8 * rho_re, 0.0)
    rho_csph = np.where(re <= 1000.0 * (1 + 2 * rho_re), rho_low, U)
    p = 1.0 if mutant == "cliu_without_y" else 1.0 + 2.632 * y
    E_p = 2.632 * y * (rho_y + 2 * U) + U * p
    c_liu = c_sph * p
    rho_cliu = rho_csph + E_p / p + U
    n23 = N_FULL if mutant == "n_full_for_n23" else K["n23"]
    f = np.minimum(n23, n) / n23
    E_f = np.where(n >= n23, 0.0, 2 * U * f)
    g = 1.0 - f
    E_g = E_f + U * g
    cd = g * c_liu + f
    E_cd = E_g * c_liu + g * c_liu * (rho_cliu + U) + E_f + U * cd
    length = K["d"] if mutant == "adrop_d_for_L" else K["L"]
    rad = length + C_B * length * y
    E_rad = U * length + C_B * length * y * (rho_y + 2 * U) + U * rad
    a_drop = np.pi * rad ** 2
    rho_adrop = 2 * E_rad / rad + 3 * U
    d2 = K["d"] ** 2
    a_un = g * a_drop + f * d2
    E_aun = E_g * a_drop + g * a_drop * (rho_adrop + U) + E_f * d2 + 2 * U * f * d2 + U * a_un
    w = np.clip(1.0 - q, 0.0, 1.0)
    E_w = (0.0 if e_q is None else e_q) + U + W_FLUSH
    inv_m = 1.0 if mutant == "inv_m_dropped" else 1.0 / m
    Kc = k * 0.5 * inv_m * rho_a * s * cd * a_un          # a = Kc w v_rel
    a = (Kc * w)[:, None] * r
    rho_rest = rho_s + E_cd / cd + E_aun / a_un + 7 * U + ((FAST + U) if fast else 0.0)
    E_a = np.abs(Kc[:, None] * r) * np.asarray(E_w)[..., None] + np.abs(a) * rho_rest[:, None] + np.abs(Kc * w)[:, None] * E_r
    z = lambda arr: np.where(on if arr.ndim == 1 else on[:, None], arr, 0.0)
    so = SECOND_ORDER
    return dict(a=z(a), w=z(w), cd=z(cd), a_un=z(a_un), y=z(y), s=s, e=e, on=on, re=re, f=f,
                b_a=z(E_a) * so, b_w=z(np.broadcast_to(E_w, w.shape)) * so, b_cd=z(E_cd) * so, b_a_un=z(E_aun) * so, b_y=z(E_y) * so, b_e=E_e)


def neighbour_terms(x, mat, h, e, b_e, mutant=None, fast=False):
    """(n_i, q, E_q) of every row from a KD-tree pair list: the count of fluid neighbours within h and the largest e_i . (x_i - x_j) /
    |x_i - x_j| over them (0 without one).  Rows that are not fluid: zero.  Refuses a pair list with a fluid pair within GAP h of h."""
    x = np.asarray(x, np.float64)
    n = len(x)
    _, i, j = _pair_list(x, h * (1 + 2 * GAP))
    R = x[i] - x[j]
    r = np.linalg.norm(R, axis=1)
    both = (mat[i] == 1) & (mat[j] == 1)
    assert (np.abs(r[both] - h) > GAP * h).all(), "a fluid pair within 1e-5 h of h: the count would depend on rounding"
    assert (r > 0).all()
    near = r < h
    count = near & (mat[i] == 1) & ((mat[j] == 1) | (mutant == "rigid_counted"))
    shield = near & (mat[i] == 1) & ((mat[j] == 1) | (mutant == "rigid_shielding"))
    n_i = np.bincount(i[count], minlength=n).astype(np.float64)
    sign = -1.0 if mutant == "xj_minus_xi" else 1.0
    qq = sign * (e[i] * R).sum(axis=1) / r
    q = np.zeros(n)
    if mutant == "q_sum":
        q = np.bincount(i[shield], np.maximum(qq[shield], 0.0), minlength=n)
    else:
        np.maximum.at(q, i[shield], qq[shield])
    E_q = np.linalg.norm(b_e, axis=1) + 4 * U + (3.5 * U + FAST if fast else 4.5 * U)
    return n_i, q, E_q * SECOND_ORDER


def drag_f64(x, v, mass, mat, h, radius, rho_l, k=1.0, rho_a=RHO_AIR, u=(0.0, 0.0, 0.0), mutant=None, fast=False):
    """The walk and everything behind it: particle_f64's dict plus n, q, b_q; rows that are not fluid are zero."""
    fl = np.asarray(mat) == 1
    pm = mutant if mutant in PARTICLE_MUTANTS else None
    wm = mutant if mutant in WALK_MUTANTS else None
    vv = np.where(fl[:, None], np.asarray(v, np.float64), 1.0)     # (rows that are not fluid: any value off the threshold)
    dirs = particle_f64(vv, 1.0, 0.0, 0.0, radius, rho_l, k, rho_a, u, mutant=pm, fast=fast, e_dir=True)
    n_i, q, E_q = neighbour_terms(x, mat, h, dirs["e"], dirs["b_e"], mutant=wm, fast=fast)
    res = particle_f64(vv, np.where(fl, mass, 1.0), n_i, q, radius, rho_l, k, rho_a, u, mutant=pm, fast=fast, e_q=E_q)
    for key in ("a", "w", "cd", "a_un", "y", "b_a", "b_w", "b_cd", "b_a_un", "b_y"):
        res[key] = np.where(fl if res[key].ndim == 1 else fl[:, None], res[key], 0.0)
    res.update(n=np.where(fl, n_i, 0.0), q=np.where(fl, q, 0.0), b_q=E_q, fluid=fl)
    return res


TERMS = ("a", "w", "cd", "a_un", "y")


def misses(got, res, rows=None):
    """{term: worst |got - model| / bound} over the terms that miss their bound (n: 'count'); got: dict(a, n, w, cd, a_un, y)."""
    out = {}
    sel = slice(None) if rows is None else rows
    if "n" in got and not np.array_equal(np.asarray(got["n"], np.float64)[sel], res["n"][sel]):
        out["n"] = float(np.abs(np.asarray(got["n"], np.float64)[sel] - res["n"][sel]).max())
    for t in TERMS:
        err = np.abs(np.asarray(got[t], np.float64) - res[t])[sel]
        b = res["b_" + t][sel]
        bad = err > b
        if bad.any():
            out[t] = float((err[bad] / np.maximum(b[bad], 1e-300)).max())
    return out


def worst(got, res, rows=None):
    """{term: max |got - model| / bound} (0 / 0 = 0), for the log"""
    sel = slice(None) if rows is None else rows
    out = {}
    for t in TERMS:
        err = np.abs(np.asarray(got[t], np.float64) - res[t])[sel]
        b = res["b_" + t][sel]
        out[t] = float(np.where(err > 0, err / np.maximum(b, 1e-300), 0.0).max()) if err.size else 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The scenes.  block_scene: a jittered 7 x 7 x 7 fluid block (343 particles: two workgroups, the second partial) in the form of
# nonpressure_terms.scene / surface_tension_terms.scene (nonpressure_terms.feed inserts it), with random velocities whose speeds
# span 1e-4 ... 12 m / s log-uniformly and every eighth particle at rest.  The kinds "rigid" and "fluid" of micropolar_terms.scene are
# taken with the seed below.
BLOCK_EDGE = 7
BLOCK_SEED, SCENE_SEED = 5, 11
WINDS = ((0.0, 0.0, 0.0), (3.0, -1.0, 0.5))


def block_velocities(n, seed=BLOCK_SEED):
    rng = np.random.default_rng(seed + 1000)
    speed = 10.0 ** rng.uniform(-4.0, np.log10(12.0), n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    vel = speed[:, None] * d
    vel[::8] = 0.0
    return vel.astype(np.float32)


def particles_scene(method, pos, vel, rigid_pos=None, dt=4e-4, viscosity_method="standard", gravity=None, kind="particles", layers=None):
    """A scene of given fluid particles (object 0) and, with rigid_pos, a static rigid object 1, in the form of nonpressure_terms.scene;
    layers: in a domain of that many cell layers in z (tests/helpers.py with_layers)."""
    from sph_project_amd import scene as S
    from sph_project_amd.product import dam_break_scene, scene_particles
    cfg = dam_break_scene(method=method, domain_end=(0.6, 0.52, 0.52), start=(0, 0, 0), end=(0, 0, 0), add_domain_box=False,
                          viscosity=0.01, viscosity_b=0.01, dt=dt, viscosity_method=viscosity_method)
    if layers is not None:
        cfg = with_layers(cfg, layers)
    cfg["FluidBlocks"] = []
    if gravity is not None:
        cfg["Configuration"]["gravitation"] = [float(g) for g in gravity]
    c, geo, batches = scene_particles(cfg)
    sol = S.derive_solver_constants(c)
    k = len(pos)
    batches.append(dict(object_id=0, pos=np.asarray(pos, np.float32), vel=np.asarray(vel, np.float32), density=np.full(k, 1000.0, np.float32),
                        material=np.ones(k, np.int32), is_dynamic=np.ones(k, np.int32)))
    if rigid_pos is not None:
        kr = len(rigid_pos)
        batches.append(dict(object_id=1, pos=np.asarray(rigid_pos, np.float32), vel=np.zeros((kr, 3), np.float32),
                            density=np.full(kr, 2200.0, np.float32), material=np.full(kr, 2, np.int32), is_dynamic=np.zeros(kr, np.int32)))
    total = sum(len(b["pos"]) for b in batches)
    pd = S.params_dict(geo, sol, method, total)
    params = dict(h=pd["support_radius"], rho0=pd["density_0"], diameter=2 * pd["particle_radius"], st=pd["surface_tension"],
                  mu=pd["viscosity"], mu_b=pd["viscosity_b"], g=pd["gravity"], dim=3, dt=float(np.float32(pd["dt"])),
                  padding=pd["padding"], domain=pd["domain_size"], V0=pd["V0"], radius=pd["particle_radius"])
    return dict(cfg=cfg, pd=pd, batches=batches, com=np.zeros((2, 3), np.float32), params=params, rigid=False, kind=kind)


def block_scene(method, seed=BLOCK_SEED, **kw):
    rng = np.random.default_rng(seed)
    d = 0.02
    ax = 0.2 + d * np.arange(BLOCK_EDGE)
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    pts = pts + rng.uniform(-0.2, 0.2, pts.shape) * (0.5 * d)
    sc = particles_scene(method, pts, block_velocities(len(pts), seed), kind="block", **kw)
    assert abs(sc["params"]["diameter"] - d) < 1e-12
    return sc


def scene(method, kind, **kw):
    """kind "block", or "rigid" / "fluid" of micropolar_terms.scene"""
    if kind == "block":
        return block_scene(method, **kw)
    from tests import micropolar_terms as M
    sc = M.scene(method, kind, seed=SCENE_SEED, **kw)
    sc["params"]["radius"] = sc["pd"]["particle_radius"]
    return sc


def host_arrays(sc):
    """(x, v, mat, mass) by insertion order, mass = density V0 for fluid (what the library derives) and 1 elsewhere (unused)"""
    cat = lambda k, dt: np.concatenate([np.asarray(b[k]) for b in sc["batches"]]).astype(dt)
    x, v, mat = cat("pos", np.float32), cat("vel", np.float32), cat("material", np.int32)
    mass = np.where(mat == 1, cat("density", np.float64) * sc["params"]["V0"], 1.0)
    return x, v, mat, mass


def assert_alive(res, wind):
    """A scene change must not hollow the checks out."""
    fl = res["fluid"]
    on = res["on"] & fl
    assert on.sum() > 50 and np.abs(res["a"][on]).max() > 1e-3
    assert res["n"][fl].min() < 20 and res["n"][fl].max() >= 26, "both sides of n23"
    assert (res["w"][on] < 0.05).any() and (res["w"][on] > 0.5).any(), "shielded and exposed particles"
    if not any(wind):
        assert (~res["on"] & fl).any(), "particles below the threshold"
