"""The elastic solids (corotated SPH elasticity per fluid object) restated in float64 -- written from the formulas,
independent of the device code -- with bounds derived from operation counts and magnitudes in the style of tests/micropolar_terms.py,
and the mutants that every comparison has to catch.  Arrays are in ID order (ids = append order); the rows of an object are a
contiguous id range.

    capture:  N0_i = same-object fluid particles j != i with r2 < h2 on the f32 differences (the step's own test), ascending id
              M_i = sum_j V0 x0_ji (x) gradW0_ij;  g0_ij = M_i^-1 gradW0_ij;  q_i = identity
    step:     F_i = sum_j V0 (x_j - x_i) (x) g0_ij;  R_i: ROT_ITERS iterations of Mueller et al. 2016 from the stored q_i
              eps_i = 1/2 (F_i R_i^T + R_i F_i^T) - I;  sig_i = 2 mu eps_i + lambda tr(eps_i) I
              a_el_i = (V0^2 / m_i) sum_j (sig_i R_i g0_ij - sig_j R_j g0_ji)

Bounds (u = 2^-24; every one holds for ANY f32 evaluation of the same sums in list order, fused or not).
  gradW0 in f32 (kernGrad + geom of csrc/sph_device.hpp): the difference 1, r^2 3, sqrt 1, q 1, the polynomial 4, its constant 1,
    1 / (rn h) 2, x dx 1 = 14, fast forms + 4: G_U = 18 u relative, plus the conditioning of the gradient in q, 6 u |s| amp |R|
    (nonpressure_terms.kernel_grad_scale).  Call it dg.
  M is summed in float64 from those f32 gradients: dM = sum V0 |x0_ji| (x) dg.  g0 = M^-1 g in float64, rounded once:
    |d g0| <= 1.001 |M^-1| (dg + dM |g0|) + u |g0|  (first order, 1.001 for the second).
  consistency sum_j V0 x0_ji (x) g0_ij = I, summed in float64 from the device's g0: sum_j V0 |x0_ji| (x) |d g0_ij|.
  F: per entry x_j - x_i 1, V0 x 1, the product 1, K additions: (K + 4) u sum_k |V0 d_a g0_b|.
  q: one iteration rounds om = num / den to (10 num_mag + 8 |om| dot_mag) u / den (num_mag, dot_mag: the sums of the magnitudes of
    the products, which carry the 4 u of each entry of mat(q)), the quaternion by half of that, sin and cos 2 x 2 u, the Hamilton
    product 6 u, the normalisation 4 u: r_t = |d om| / 2 + 14 u.  An error made in iteration t reaches the result through the
    remaining iterations; its gain G_t is measured ON THE MODEL (finite differences of the float64 iteration in four directions,
    summed): |d q| <= sum_t G_t r_t.
  sigma from the device's F and q: mat(q) 6 u per entry; A = F R^T: sum_c |F_ac| (3 u |R_bc| + 6 u); - I, the mean: 2 u (|A| + I);
    that is d eps; sigma: 2 mu d eps + lambda sum d eps_kk + 4 u (|2 mu eps| + 3 |lambda| max|eps_kk|) + 2 u |sigma|
    (the constants mu, lambda 1 u each).
  a_el from the device's q, sigma and table: per entry two matrix-vector products on each side, (K + 20) u sum_k mag_k with
    mag_k = |sig_i| (|R_i| + 6 u J) |g0_ij| + |sig_j| (|R_j| + 6 u J) |g0_ji|, times the coefficient V0^2 / m_i (3 u, inside the 20).
  momentum: |sum_i m_i a_el_i| <= sum_i m_i bound_i (the pair terms cancel exactly in exact arithmetic: g0_ji of row i is g0_ij of
    row j bit for bit)."""
import numpy as np

from tests import nonpressure_terms as T

U = T.U
G_U = 18.0
K_MAX = 64
ROT_ITERS = 10
MIN_EIG_RATIO = 1e-3

MUTANTS = ("g_outer_x", "no_minv", "gji_neg_gij", "plus_neighbour", "ri_in_neighbour", "unsymmetrised", "rtf", "no_lambda",
           "mu_double", "v0_once", "div_mj", "cold_start", "nine_iterations", "foreign_neighbours", "by_slot")


def lame(E, nu, mutant=None):
    mu = E / (1.0 + nu) if mutant == "mu_double" else E / (2.0 * (1.0 + nu))
    lam = 0.0 if mutant == "no_lambda" else E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    return mu, lam


def h2_threshold(h):
    """The library's acceptance threshold (sph_api.hip fill_consts): the smallest f32 t with sqrtf(t) >= f32(h)."""
    hf = np.float32(h)
    t = np.float32(hf * hf)
    while np.sqrt(np.nextafter(t, np.float32(0.0))) >= hf:
        t = np.nextafter(t, np.float32(0.0))
    while np.sqrt(t) < hf:
        t = np.nextafter(t, np.float32(np.inf))
    return t


def _pad(lists, fill=-1):
    k = max(1, max((len(l) for l in lists), default=1))
    out = np.full((len(lists), k), fill, np.int64)
    for r, l in enumerate(lists):
        out[r, :len(l)] = l
    return out


def capture_f64(x0, obj, fluid, target, h, V0, mutant=None):
    """x0 (N, 3) float32, obj (N,), fluid (N,) bool in id order.  dict: ids, id0, nbr (n, K) ids (-1 behind the end), cnt, M, ratio,
    g0_ij, g0_ji, g0_bound (n, K, 3), cons, cons_bound (n, 3, 3), ambiguous (pairs whose acceptance an evaluation order could flip)."""
    x0 = np.asarray(x0, np.float32)
    ids = np.nonzero(np.asarray(obj) == target)[0]
    assert len(ids) and ids[-1] - ids[0] + 1 == len(ids), "the object's ids are one contiguous range"
    id0, n = int(ids[0]), len(ids)
    cand = np.nonzero(fluid)[0] if mutant == "foreign_neighbours" else ids
    h2 = h2_threshold(h)
    xi, xc = x0[ids], x0[cand]
    d = xi[:, None, :] - xc[None, :, :]                       # f32 differences
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]   # f32, as written
    acc = (r2 < h2) & (ids[:, None] != cand[None, :])
    d64 = d.astype(np.float64)
    r2x = (d64 ** 2).sum(-1)
    aligned = (d != 0).sum(-1) <= 1                          # one product: every evaluation order gives fl(dx dx)
    ambiguous = int(((np.abs(r2x - float(h2)) <= 8 * U * float(h2)) & ~aligned & (ids[:, None] != cand[None, :])).sum())
    lists = [cand[acc[r]] for r in range(n)]
    nbr = _pad(lists)
    cnt = np.array([len(l) for l in lists])
    mask = nbr >= 0
    j = np.where(mask, nbr, id0)
    R = (x0[ids][:, None, :].astype(np.float64) - x0[j].astype(np.float64)) * mask[..., None]    # x0_i - x0_j
    r = np.linalg.norm(R, axis=-1)
    s, s_amp = T.kernel_grad_scale(r, h)
    g = s[..., None] * R
    dg = (G_U * U * np.abs(g) + 6 * U * s_amp[..., None] * np.abs(R)) * mask[..., None]
    M = np.einsum("nka,nkb->nab", -V0 * R, g)
    dM = np.einsum("nka,nkb->nab", V0 * np.abs(R), dg)
    ev = np.linalg.eigvalsh(0.5 * (M + M.transpose(0, 2, 1)))
    ratio = np.where((ev[:, -1] > 0) & (cnt >= 3), ev[:, 0] / np.where(ev[:, -1] > 0, ev[:, -1], 1.0), 0.0)
    ok = ratio >= MIN_EIG_RATIO
    Minv = np.zeros_like(M)
    Minv[ok] = np.linalg.inv(M[ok])
    if mutant == "no_minv":
        Minv = np.broadcast_to(np.eye(3), M.shape).copy()
    g0 = np.einsum("nab,nkb->nka", Minv, g)
    g0_bound = 1.001 * np.einsum("nab,nkb->nka", np.abs(Minv), dg + np.einsum("nab,nkb->nka", dM, np.abs(g0))) + U * np.abs(g0)
    g0_bound *= mask[..., None]
    # the partner's entry
    g0_ji = np.zeros_like(g0)
    rows = np.clip(j - id0, 0, n - 1)
    for rr in range(n):
        for k in range(cnt[rr]):
            jj = nbr[rr, k]
            if jj < id0 or jj >= id0 + n:
                continue   # (mutant foreign_neighbours: no partner row)
            back = np.nonzero(nbr[rows[rr, k]] == ids[rr])[0]
            if len(back):
                g0_ji[rr, k] = g0[rows[rr, k], back[0]]
    if mutant == "gji_neg_gij":
        g0_ji = -g0
    cons = np.einsum("nka,nkb->nab", -V0 * R, g0)
    cons_bound = np.einsum("nka,nkb->nab", V0 * np.abs(R), g0_bound)
    return dict(ids=ids, id0=id0, n=n, nbr=nbr, cnt=cnt, M=M, ratio=ratio, g0_ij=g0, g0_ji=g0_ji, g0_bound=g0_bound, cons=cons,
                cons_bound=cons_bound, ambiguous=ambiguous, R0=R)


# ---------------------------------------------------------------------------------------------------------------------------
def quat_matrix(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - w * z); R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y); R[..., 2, 1] = 2 * (y * z + w * x); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def quat_mul(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(-1, keepdims=True)], -1)


def rotation_step(q, F):
    """One iteration; returns (q_new, rounding r_t of this iteration as the docstring derives it)."""
    R = quat_matrix(q)
    num = np.cross(R.transpose(0, 2, 1), F.transpose(0, 2, 1)).sum(1)          # sum_k r_k x f_k (columns)
    num_mag = np.stack([(np.abs(R[:, (a + 1) % 3, :]) * np.abs(F[:, (a + 2) % 3, :]) +
                         np.abs(R[:, (a + 2) % 3, :]) * np.abs(F[:, (a + 1) % 3, :])).sum(-1) for a in range(3)], -1)
    dot = (R * F).sum((1, 2))
    dot_mag = (np.abs(R) * np.abs(F)).sum((1, 2))
    den = np.abs(dot) + 1e-9
    om = num / den[:, None]
    w = np.linalg.norm(om, axis=-1)
    d_om = (10 * np.linalg.norm(num_mag, axis=-1) + 8 * w * dot_mag) * U / den
    live = w >= 1e-9
    ws = np.where(live, w, 1.0)
    dq = np.concatenate([np.sin(0.5 * ws)[:, None] * om / ws[:, None], np.cos(0.5 * ws)[:, None]], -1)
    qn = quat_mul(dq, q)
    qn /= np.linalg.norm(qn, axis=-1, keepdims=True)
    return np.where(live[:, None], qn, q), np.where(live, 0.5 * d_om + 14 * U, 0.0)


def extract_rotation(q, F, iters=ROT_ITERS, with_bound=False):
    q = np.array(q, np.float64)
    hist, rnd = [q], []
    for _ in range(iters):
        q, r = rotation_step(q, F)
        hist.append(q); rnd.append(r)
    if not with_bound:
        return q
    bound = np.zeros(len(q))
    eps = 1e-6
    for t in range(iters):   # an error behind iteration t (in q_{t+1}) passes through iterations t + 1 .. iters - 1
        gain = np.zeros(len(q))
        for a in range(4):
            qp = hist[t + 1].copy()
            qp[:, a] += eps
            qp /= np.linalg.norm(qp, axis=-1, keepdims=True)
            base = hist[t + 1]
            shift = np.linalg.norm(qp - base, axis=-1)
            for _ in range(t + 1, iters):
                qp, _r = rotation_step(qp, F)
            gain += np.linalg.norm(qp - q, axis=-1) / np.maximum(shift, 1e-12)
        bound += np.maximum(gain, 1.0) * rnd[t]
    return q, bound


def stress(F, q, mu, lam, mutant=None):
    """(sigma (n, 6), bound (n, 6)) from F and q: xx xy xz yy yz zz."""
    R = quat_matrix(q)
    A = np.einsum("nca,ncb->nab", R, F) if mutant == "rtf" else np.einsum("nac,nbc->nab", F, R)
    I = np.eye(3)
    eps = A - I if mutant == "unsymmetrised" else 0.5 * (A + A.transpose(0, 2, 1)) - I
    dA = np.einsum("nac,nbc->nab", np.abs(F), 3 * U * np.abs(R) + 6 * U)
    deps = 0.5 * (dA + dA.transpose(0, 2, 1)) + 2 * U * (np.abs(A) + I)
    tr = np.trace(eps, axis1=1, axis2=2)
    sig = 2 * mu * eps + lam * tr[:, None, None] * I
    dsig = (2 * mu * deps + abs(lam) * np.trace(deps, axis1=1, axis2=2)[:, None, None] * I +
            4 * U * (np.abs(2 * mu * eps) + 3 * abs(lam) * np.abs(eps[:, [0, 1, 2], [0, 1, 2]]).max(-1)[:, None, None] * I) + 2 * U * np.abs(sig))
    pick = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])
    return sig[:, pick[0], pick[1]], dsig[:, pick[0], pick[1]]


def sym3(s6):
    m = np.empty(s6.shape[:-1] + (3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        m[..., a, b] = m[..., b, a] = s6[..., k]
    return m


def step_f64(x, cap, q_prev, mass, V0, E, nu, mutant=None, order=None, F_in=None, q_in=None, sig_in=None, g0_ij=None, g0_ji=None):
    """One elastic pass on positions x (N, 3; id order) with the capture `cap`.  q_prev, mass: (N, ...) id order.  The stages can be
    fed with the device's results: F_in (n, 3, 3), q_in (n, 4), sig_in (n, 6) of the object's rows; g0_ij / g0_ji: the device's table.
    order (mutant by_slot): slot -> id of the current order; the mutant reads x_j at SLOT j.
    dict: F, F_bound, q, q_bound, sig, sig_bound, a, a_bound (n rows)."""
    ids, id0, n, nbr = cap["ids"], cap["id0"], cap["n"], cap["nbr"]
    mask = nbr >= 0
    rows_ok = mask & (nbr >= id0) & (nbr < id0 + n)
    j = np.where(mask, nbr, id0)
    gij = np.asarray(cap["g0_ij"] if g0_ij is None else g0_ij, np.float64) * mask[..., None]
    gji = np.asarray(cap["g0_ji"] if g0_ji is None else g0_ji, np.float64) * mask[..., None]
    x = np.asarray(x, np.float64)
    xj = x[np.asarray(order)[j]] if mutant == "by_slot" else x[j]
    d = (xj - x[ids][:, None, :]) * mask[..., None]
    mu, lam = lame(E, nu, mutant)
    if mutant == "g_outer_x":
        F = np.einsum("nka,nkb->nab", gij, V0 * d)
    else:
        F = np.einsum("nka,nkb->nab", V0 * d, gij)
    F_bound = (mask.sum(1) + 4)[:, None, None] * U * np.einsum("nka,nkb->nab", np.abs(V0 * d), np.abs(gij))
    Fq = np.asarray(F if F_in is None else F_in, np.float64)
    q0 = np.asarray(q_prev, np.float64)[ids]
    if mutant == "cold_start":
        q0 = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1))
    iters = ROT_ITERS - 1 if mutant == "nine_iterations" else ROT_ITERS
    if mutant is None:
        q, q_bound = extract_rotation(q0, Fq, iters, with_bound=True)
    else:
        q, q_bound = extract_rotation(q0, Fq, iters), np.zeros(n)
    qs = np.asarray(q if q_in is None else q_in, np.float64)
    sig, sig_bound = stress(Fq, qs, mu, lam, mutant)
    ss = np.asarray(sig if sig_in is None else sig_in, np.float64)
    # pass B: the neighbours' q and sigma by id (rows of the same object)
    R = quat_matrix(qs)
    S = sym3(ss)
    jr = np.clip(j - id0, 0, n - 1)
    Rj, Sj = R[jr], S[jr]
    if mutant == "ri_in_neighbour":
        Rj = np.broadcast_to(R[:, None], Rj.shape)
    ti = np.einsum("nab,nbc,nkc->nka", S, R, gij)
    tj = np.einsum("nkab,nkbc,nkc->nka", Sj, Rj, gji) * rows_ok[..., None]
    terms = ti + tj if mutant == "plus_neighbour" else ti - tj
    J = 6 * U * np.ones((3, 3))
    mag = (np.einsum("nab,nbc,nkc->nka", np.abs(S), np.abs(R) + J, np.abs(gij)) +
           np.einsum("nkab,nkbc,nkc->nka", np.abs(Sj), np.abs(Rj) + J, np.abs(gji)) * rows_ok[..., None])
    m = np.asarray(mass, np.float64)
    if mutant == "div_mj":
        coef = (V0 * V0 / m[j])[..., None] * mask[..., None]
        a = (coef * terms).sum(1)
    else:
        coef = (V0 if mutant == "v0_once" else V0 * V0) / m[ids]
        a = coef[:, None] * terms.sum(1)
    a_bound = (V0 * V0 / m[ids])[:, None] * (mask.sum(1) + 20)[:, None] * U * mag.sum(1)
    return dict(F=F, F_bound=F_bound, q=q, q_bound=q_bound, sig=sig, sig_bound=sig_bound, a=a, a_bound=a_bound)


def quat_dist(a, b):
    """|a - b| up to the sign of the quaternion (q and -q are the same rotation)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.minimum(np.linalg.norm(a - b, axis=-1), np.linalg.norm(a + b, axis=-1))


def worst(err, bound, tiny=0.0):
    """max err / (bound + tiny): <= 1 passes."""
    return float(np.max(np.abs(err) / (np.asarray(bound) + tiny))) if np.size(err) else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# Scenes (host): blocks on the rest lattice of the library's geometry, h = 2 d, V0 = 0.8 d^3.
D = 0.02
H = 2 * D
V0 = float(np.float32(0.8 * D ** 3))


def block(n=(8, 8, 8), origin=(0.2, 0.2, 0.2), jitter=0.0, seed=7):   # (seed 7: the longest list of the jittered 8x8x8 block has 36 entries)
    ax = [D * np.arange(k) for k in n]
    x = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3) + np.asarray(origin)
    if jitter:
        x = x + np.random.default_rng(seed).uniform(-jitter, jitter, x.shape) * D
    return x.astype(np.float32)


def two_blocks(jitter=0.0):
    """An 8x8x8 elastic block (object 0) and a 6x6x6 plain block (object 1) touching it along +x; id order = append order."""
    a = block((8, 8, 8), jitter=jitter)
    b = block((6, 6, 6), origin=(0.2 + 8 * D, 0.2, 0.2), jitter=jitter, seed=4)
    x = np.concatenate([a, b])
    obj = np.concatenate([np.zeros(len(a), np.int32), np.ones(len(b), np.int32)])
    return x, obj


def rotation(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def rotation_quat(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(deg)
    return np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]])


def deform(x0, kind, seed=5):
    """(x, A or None): positions deformed about the block's centre.  affine: a general matrix near the identity; rigid: 40 degrees
    about (1, 2, 3) plus a translation; smooth: a random smooth field (a rotation that varies across the block plus a quadratic
    displacement); stretch: diag(1.05, 1, 1); far: the affine map plus a translation of several cells."""
    x0 = np.asarray(x0, np.float64)
    c = x0.mean(0)
    y = x0 - c
    rng = np.random.default_rng(seed)
    if kind == "rigid":
        A = rotation((1, 2, 3), 40.0)
        return (y @ A.T + c + np.array([0.013, -0.007, 0.021])).astype(np.float32), A
    if kind in ("affine", "far"):
        A = rotation((2, -1, 1), 25.0) @ (np.eye(3) + 0.08 * rng.uniform(-1, 1, (3, 3)))
        t = np.array([0.17, 0.13, 0.21]) if kind == "far" else np.array([0.004, 0.002, -0.003])
        return (y @ A.T + c + t).astype(np.float32), A
    if kind == "stretch":
        A = np.diag([1.05, 1.0, 1.0])
        return (y @ A.T + c).astype(np.float32), A
    assert kind == "smooth"
    ang = 30.0 + 400.0 * y[:, 0]                      # degrees: the rotation about z varies along x
    ca, sa = np.cos(np.radians(ang)), np.sin(np.radians(ang))
    z = np.stack([ca * y[:, 0] - sa * y[:, 1], sa * y[:, 0] + ca * y[:, 1], y[:, 2]], -1)
    z = z + 0.8 * np.stack([y[:, 1] * y[:, 2], y[:, 0] ** 2, -y[:, 0] * y[:, 1]], -1)
    return (z + c).astype(np.float32), None


def warm_start(n, kind="far", seed=9):
    """Warm-start quaternions the tests upload: `far` is 150 degrees away from the rigid scene's rotation, so that ten iterations do
    not converge (the mutants cold_start, nine_iterations and unsymmetrised differ there); `near`: 5 degrees about random axes."""
    rng = np.random.default_rng(seed)
    if kind == "far":
        q = rotation_quat((1, 2, 3), 40.0 - 150.0)
        return np.tile(q, (n, 1)).astype(np.float32)
    ax = rng.normal(size=(n, 3))
    return np.stack([rotation_quat(a, 5.0) for a in ax]).astype(np.float32)
