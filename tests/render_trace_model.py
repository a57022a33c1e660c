"""float64 restatement of the terms of a traced mesh frame (csrc/sph_render_trace.hpp), for checks per term from the
device's own inputs: every function takes what the device recorded for a segment (origin, direction, normal, throughput) and recomputes
one term of it; no error is followed through a chain of bounces.

Bounds.  u = 2^-24 is the unit roundoff of float32; the device evaluates every term below in float32 from float32 inputs, with at most
a dozen rounded operations per term, on magnitudes that the scenes of the tests keep below 4 (coordinates inside and around the unit
box, unit directions and normals, throughputs, F and colours in [0, 1]).
  cosine     the device normalises the recorded direction itself (three divisions by the largest component, a square root, three
             divisions: <= 4 u per component in the strict build) and takes a dot product with the recorded normal (3 u): the cosine
             is within 7 u, say 8 u, of the float64 one.
  k          Snell's discriminant k = 1 - eta^2 (1 - c^2), eta <= ior < 2: its error is <= 2 eta^2 c x 8 u + 3 u of its own two fmas
             <= 32 u, so sqrt(k) is within 32 u / (2 sqrt k) = 16 u / sqrt(k): the error of the inputs, amplified near k = 0, not
             just the root's own rounding.  Segments with |k| < K_TOL = 2^-10 are unsure and left out (there the sign of k itself,
             refraction or total reflection, is open).
  direction  eta d + (eta c - sqrt k) n, normalised: 1.33 x 4 u of d, 1.33 x 8 u of c, 16 u / sqrt(k) of the root, 4 u of the two fmas
             and 4 u of the normalisation: (23 + 16 / sqrt k) u in the strict build.  The fast build divides by a reciprocal and takes
             reciprocal square roots, each within 2.5 ulp where the strict operations are within 0.5: 2 u more at each of the 14
             divisions and roots on the way (two normalisations of seven each): 28 u more.  DIR_TOL(k) = (64 + 16 / sqrt k) u for both.
  F          Schlick: x = 1 - cos <= 1, x^5 by three multiplications, one fma: 5 u of its own; the cosine on the outside is c (8 u) or
             sqrt k (16 u / sqrt k), times the slope 5 x^4 <= 5, and 14 u for the fast build's divisions behind the cosine:
             F_TOL(k) = (64 + 80 / sqrt k) u.
  throughput from the start's throughput, the recorded t and the recorded F: one exp2f (<= 2 ulp of a value <= 1, its argument in error by <= 3 u |arg| with |arg| <= 8 in the tests: 24 u relative) and
             two multiplications: THR_TOL = 32 u.
  position   the next origin is O + t d by one fma per component: <= u (|O| + t |d|) <= 8 u; POS_TOL = 8 u.
  pixel      the byte is floor(255 x + 0.5) of the sum of the recorded contributions; the device adds them in float32 in segment order
             (<= 2 max_depth additions of values <= 1: <= 2 max_depth u <= 2^-17 for max_depth <= 64), so the float64 sum decides the byte
             unless 255 x + 0.5 lies within 255 x 2^-17 < 2^-9 of an integer: there either neighbour is accepted.
Nothing here is fitted to what a device returned."""
import numpy as np

U = 2.0 ** -24
DIR_TOL = 80 * U   # DIR_TOL(1): where k = 1 (a reflection, a ray along the normal)


def dir_tol(k):
    return (64.0 + 16.0 / np.sqrt(np.maximum(np.abs(k), K_TOL))) * U


def f_tol(k):
    return (64.0 + 80.0 / np.sqrt(np.maximum(np.abs(k), K_TOL))) * U


THR_TOL = 32 * U
POS_TOL = 8 * U
K_TOL = 2.0 ** -10
BYTE_EDGE = 2.0 ** -9
FLOOR_ID = -14
W_O, W_D, W_ID, W_T, W_N, W_THR0, W_THR1, W_ADD, W_SHADOW, W_RID, W_F, W_FLAGS = 0, 3, 6, 7, 8, 11, 14, 17, 20, 21, 22, 23
F_USED, F_ENTER, F_TIR, F_INSIDE, F_RSHADOW = 1, 2, 4, 8, 16


def camera(eye, target, up=(0.0, 1.0, 0.0), fov=70.0, W=64, H=64):
    """(E, f, s, u, tx, ty) of sph_render_create, in float64"""
    E = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - E
    f /= np.linalg.norm(f)
    s = np.cross(f, np.asarray(up, np.float64))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    ty = np.tan(0.5 * np.radians(fov))
    return E, f, s, u, ty * W / H, ty


def pixel_rays(cam, W, H):
    """directions (H, W, 3) of the pixel centres' rays, f . d = 1"""
    E, f, s, u, tx, ty = cam
    X = ((2 * np.arange(W) + 1) / W - 1.0) * tx
    Y = (1.0 - (2 * np.arange(H) + 1) / H) * ty
    return X[None, :, None] * s + Y[:, None, None] * u + f


def plane_hit(O, d, y):
    """where rays O + t d meet the plane of height y (points (..., 3); t <= 0 or a parallel ray: nan)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (y - O[..., 1]) / d[..., 1]
    t = np.where(t > 0, t, np.nan)
    return O + t[..., None] * d


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def snell(d, n, eta):
    """(refracted unit direction, reflected unit direction, k, cos_i) of unit d at unit normal n turned against it; k < 0: total internal
    reflection, the refracted direction is nan"""
    d, n = unit(np.asarray(d, np.float64)), np.asarray(n, np.float64)
    ci = -np.sum(d * n, axis=-1)
    k = 1.0 - eta * eta * (1.0 - ci * ci)
    with np.errstate(invalid="ignore"):
        q = eta * ci - np.sqrt(k)
    refr = unit(np.asarray(eta)[..., None] * d + q[..., None] * n)
    refl = unit(d + 2.0 * ci[..., None] * n)
    return refr, refl, k, ci


def schlick(cos_outside, ior):
    f0 = ((ior - 1.0) / (ior + 1.0)) ** 2
    return f0 + (1.0 - f0) * (1.0 - cos_outside) ** 5


def transmittance(rgb, absorb, radius, length):
    """per channel exp2(-absorb (1 - rgb / 255) length / radius)"""
    return np.exp2(-(absorb / radius) * np.asarray(length)[..., None] * (1.0 - np.asarray(rgb, np.float64) / 255.0))


def check_segments(paths, rgb, ids, background, ior, max_depth, truncated, water=None):
    """Every recorded water segment of paths (H, W, depth, 24) against the terms above, from the device's own origin, direction,
    normal and throughput; every pixel's byte from its recorded contributions.  water: (rgb, absorb, radius) of the scene's one water
    colour -- then the throughput of the segments inside the fluid is checked as well.  Returns counts for the caller's report."""
    P = paths.astype(np.float64)
    I = paths.view(np.int32)
    flags = I[..., W_FLAGS]
    used = (flags & F_USED) != 0
    hit_id = I[..., W_ID]
    H, W, D, _ = paths.shape
    assert used[:, :, 0].all()
    # the primary hit is what ids() shows, except where a box line lies in front
    line = ids <= -2
    line &= ids != FLOOR_ID
    assert (hit_id[:, :, 0][~line] == ids[~line]).all()
    # a used segment follows a used segment that handed a throughput on; its origin is the point the last one hit
    for k in range(1, D):
        prev, cur = used[:, :, k - 1], used[:, :, k]
        assert not (cur & ~prev).any()
        hp = P[:, :, k - 1, W_O:W_O + 3] + P[:, :, k - 1, W_T, None] * P[:, :, k - 1, W_D:W_D + 3]
        assert np.abs(hp - P[:, :, k, W_O:W_O + 3])[cur].max(initial=0.0) <= POS_TOL
    n_water = n_unsure = 0
    for k in range(D):
        # water segments: the ones a further segment follows
        nxt = used[:, :, k + 1] if k + 1 < D else np.zeros((H, W), bool)
        m = used[:, :, k] & nxt
        if not m.any():
            continue
        d, n = P[:, :, k, W_D:W_D + 3][m], P[:, :, k, W_N:W_N + 3][m]
        fl = flags[:, :, k][m]
        entering, tir = (fl & F_ENTER) != 0, (fl & F_TIR) != 0
        eta = np.where(entering, 1.0 / ior, ior)
        refr, refl, kk, ci = snell(d, n, eta)
        sure = np.abs(kk) >= K_TOL
        n_water += int(m.sum())
        n_unsure += int((~sure).sum())
        assert (tir[sure] == (kk[sure] < 0)).all()
        want = np.where(tir[:, None], refl, refr)
        got = P[:, :, k + 1, W_D:W_D + 3][m]
        over = np.abs(got - want).max(axis=-1) / np.where(tir, DIR_TOL, dir_tol(kk))
        assert over[sure].max(initial=0.0) <= 1.0, over[sure].max()
        with np.errstate(invalid="ignore"):
            F = np.where(tir, 0.0, schlick(np.where(entering, ci, np.sqrt(kk)), ior))
        over = np.abs(P[:, :, k, W_F][m] - F) / f_tol(kk)
        assert over[sure].max(initial=0.0) <= 1.0, over[sure].max()
        # the throughput handed on: (1 - F) x what reached the hit -- the start's, absorbed along a segment inside the fluid -- with the
        # device's own F (checked above): its error is not followed into this term
        inside = (fl & F_INSIDE) != 0
        t0, t1 = P[:, :, k, W_THR0:W_THR0 + 3][m], P[:, :, k, W_THR1:W_THR1 + 3][m]
        T = np.ones_like(t0)
        if water is not None:
            T = np.where(inside[:, None], transmittance(water[0], water[1], water[2], P[:, :, k, W_T][m]), 1.0)
        ok = sure & (~inside | (water is not None))
        assert np.abs(t1 - t0 * T * (1.0 - P[:, :, k, W_F][m])[:, None])[ok].max(initial=0.0) <= THR_TOL
        # the normal is a unit vector turned against the ray
        assert np.abs(np.linalg.norm(n, axis=-1) - 1.0).max() <= 8 * U and (np.sum(unit(d) * n, axis=-1) <= 8 * U).all()
    # the pixel from its recorded contributions (a cut path adds the background through the last throughput handed on)
    total = P[..., W_ADD:W_ADD + 3].sum(axis=2)
    assert D == max_depth
    cut = used[:, :, D - 1] & (np.abs(P[:, :, D - 1, W_THR1:W_THR1 + 3]).sum(axis=-1) > 0)
    total = total + cut[..., None] * P[:, :, D - 1, W_THR1:W_THR1 + 3] * (np.asarray(background, np.float64) / 255.0)
    assert int(cut.sum()) == truncated, (int(cut.sum()), truncated)
    x = 255.0 * np.clip(total, 0.0, 1.0) + 0.5
    want = np.floor(x)
    edge = np.abs(x - np.round(x)) < BYTE_EDGE
    diff = np.abs(rgb.astype(np.float64) - want)
    diff[line] = 0.0
    assert (diff[~edge] == 0).all(), np.argwhere(diff * ~edge)[:5]
    assert (diff <= 1).all()
    return dict(water_segments=n_water, unsure=n_unsure, edge_bytes=int(edge.sum()))


# --- hits: the winner, t, the normal, the light's visibility and the contribution of a segment, from the device's own ray ----------------
# Bounds (u = 2^-24).  An edge function d . (p x q) evaluated in float32 from p = P - O, q = Q - O: <= 5 u A of its own operations and
# <= 2 u A from the rounding of p and q, A = sum_i |d_i| (|p_j q_k| + |p_k q_j|); the device counts it as inside down to -8 u A
# (trace_edge).  So a triangle whose three float64 edge functions are >= 0 is accepted for SURE, one with a function below -16 u A is
# refused for sure, and what lies between is POSSIBLE.  t = (p0 . N) / (d . N): numerator and denominator are dot products of rounded
# vectors (N: 4 u per component relative to its products), <= 8 u sum |p0_i N_i| and 8 u sum |d_i N_i|, the division u, the clamp into the
# box's slab range moves a sure hit by the slab's rounding, <= 8 u (|O| + t |d|) / |d|:
#   T_TOL = 16 u (sum |p0_i N_i| / |d . N| + |t| sum |d_i N_i| / |d . N|) + 8 u (|O|_max + |t| |d|) / |d|.
# A ray GRAZES when sum |d_i N_i| > 2^8 |d . N| (then T_TOL exceeds 2^-12 |t| and the sign of d . N, enter or leave, is within 2^-16 of
# open): unsure.  The winner rule is that of render_mesh_model.py: with t_sure the smallest t + T_TOL over the sure hits, the candidates
# are the possible hits with t - T_TOL <= t_sure; a segment whose candidates are more than one is AMBIGUOUS (unsure); the device's id must
# be a candidate always.  The floor takes part with t = (y - O_y) / d_y (3 u |t|), sure when the point lies more than 8 u (|O| + |t| |d|)
# inside the rectangle.  Visibility: the same rule along L = light - P over the triangles that block, sure blocked when a sure hit has
# T_TOL < t < 1 - T_TOL, possibly blocked when a possible one has -T_TOL < t < 1 + T_TOL; between the two the shadow ray is a NEAR MISS
# (unsure).  Contribution of a segment that ends on a diffuse surface or the floor: throughput x col / 255 x (ambient + V n.L / |L|
# light_rgb) from the RECORDED normal, t and shadow word: a dot product of a unit vector with L / |L| (8 u), one fma, two multiplications
# on values <= 2: ADD_TOL = 32 u.  The flat normal is N / |N| turned against the ray: 8 u per component.
# The blended normal: sum_k W_k n_k over the three corners, W_k the edge function opposite corner k (the device's weights about the
# ray's origin; their common sign is taken out, so the order of the corners does not matter), normalised.  Each W_k carries 7 u A_k, the
# sum 3 u of its own on |n_k| <= 1, the normalisation 4 u (16 u in the fast build): NORM_TOL = 8 u sum_k A_k |n_k| / |blend| + 24 u.
# The device takes the blend where it lies on the geometric normal's side of the ray ((n . d)(Ng . d) > 0), else Ng / |Ng|; where
# |n . d| < 2^-10 |d| that side is open and the segment is left out of the normal check (counted as grazing).
# The reflection segment: from the hit point along d + 2 c n with the RECORDED normal; its direction is within DIR_TOL of the device's,
# so the point it reaches is within DIR_TOL t_r and n.L / |L| there within 2 DIR_TOL t_r / |L|:
#   REFL_TOL = ADD_TOL + 2 DIR_TOL t_r / |L|  on  throughput x F x colour.
ADD_TOL = 32 * U
FLAT_TOL = 8 * U
SIDE = 2.0 ** -10
GRAZE = 2.0 ** 8
PICK = 2.0 ** -12   # trace_pick: a hit inside only by its error bound yields to a hard one less than 2^-12 t behind it


class Scene:
    """what a traced frame is drawn from, in float64: kept triangles (corners C, global ids gid, water flag, colour, flat flag), floor
    (y, x0, x1, z0, z1, cell) or None, light, ambient, light_rgb, background (0..255), radius, absorb, ior, z_near"""

    def __init__(self, meshes, box=None, floor=True, floor_cell=10.0, light=(2.0, 2.0, 2.0), ambient=0.1, light_rgb=(1.0, 1.0, 1.0),
                 background=(0, 0, 0), radius=0.01, absorb=0.05, ior=1.33, z_near=0.1, shadows=True):
        C, gid, water, col, flat, VN, flip, g0 = [], [], [], [], [], [], [], 0
        for item in meshes:
            v, t, n, rgb = item[:4]
            mat = item[4] if len(item) > 4 else "diffuse"
            inward = bool(item[5]) if len(item) > 5 else False
            v, t = np.asarray(v, np.float32), np.asarray(t, np.int64).reshape(-1, 3)
            ok = ((t >= 0) & (t < len(v))).all(axis=1)
            c = v[np.clip(t, 0, max(len(v) - 1, 0))].astype(np.float64)
            ok &= np.isfinite(c).all(axis=(1, 2))
            with np.errstate(invalid="ignore", over="ignore"):
                ok &= (np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]) != 0).any(axis=1)
            C.append(c[ok]); gid.append(g0 + np.nonzero(ok)[0])
            water.append(np.full(int(ok.sum()), mat == "water")); col.append(np.tile(np.float64(rgb), (int(ok.sum()), 1)))
            flat.append(np.full(int(ok.sum()), n is None))
            flip.append(np.full(int(ok.sum()), inward))
            VN.append(np.zeros((int(ok.sum()), 3, 3)) if n is None else np.asarray(n, np.float32).astype(np.float64)[np.clip(t, 0, max(len(v) - 1, 0))][ok])
            g0 += len(t)
        cat = lambda a, shape: np.concatenate(a) if a else np.zeros(shape)   # noqa: E731
        self.C, self.gid = cat(C, (0, 3, 3)), cat(gid, (0,)).astype(np.int64)
        self.water, self.col, self.flat = cat(water, (0,)).astype(bool), cat(col, (0, 3)), cat(flat, (0,)).astype(bool)
        self.N = np.cross(self.C[:, 1] - self.C[:, 0], self.C[:, 2] - self.C[:, 0])
        self.VN, self.flip = cat(VN, (0, 3, 3)), cat(flip, (0,)).astype(bool)
        self.floor = None
        if box is not None and floor:
            (x0, y0, z0), (x1, _, z1) = np.float32(box[0]).astype(np.float64), np.float32(box[1]).astype(np.float64)
            self.floor = (y0, x0, x1, z0, z1, float(np.float32(floor_cell * radius)))
        self.light, self.amb, self.lrgb = np.float32(light).astype(np.float64), float(np.float32(ambient)), np.float32(light_rgb).astype(np.float64)
        self.bg, self.radius, self.absorb, self.ior, self.zn, self.shadows = np.float64(background), radius, absorb, ior, z_near, shadows

    def hits(self, O, d, tmin, self_id, blockers=False):
        """rays O + t d (S, 3) against every triangle (and, unless blockers, the floor as the last column): t, T_TOL, sure, possible,
        grazing, each (S, T [+ 1]); self_id (S,) is never hit; blockers: only the triangles that block light"""
        p = self.C[None] - O[:, None, None, :]                                   # (S, T, 3, 3)
        dd = d[:, None, :]

        def edge(a, b):
            e = np.sum(dd * np.cross(a, b), axis=-1)
            A = (np.abs(dd[..., 0]) * (np.abs(a[..., 1] * b[..., 2]) + np.abs(a[..., 2] * b[..., 1]))
                 + np.abs(dd[..., 1]) * (np.abs(a[..., 2] * b[..., 0]) + np.abs(a[..., 0] * b[..., 2]))
                 + np.abs(dd[..., 2]) * (np.abs(a[..., 0] * b[..., 1]) + np.abs(a[..., 1] * b[..., 0])))
            return e, 16 * U * A
        e = [edge(p[:, :, 1], p[:, :, 2]), edge(p[:, :, 2], p[:, :, 0]), edge(p[:, :, 0], p[:, :, 1])]
        sure = np.all([x >= 0 for x, _ in e], axis=0) | np.all([x <= 0 for x, _ in e], axis=0)
        poss = np.all([x >= -b for x, b in e], axis=0) | np.all([x <= b for x, b in e], axis=0)
        dn = np.sum(dd * self.N[None], axis=-1)
        sdn = np.sum(np.abs(dd * self.N[None]), axis=-1)
        num = np.sum(p[:, :, 0] * self.N[None], axis=-1)
        snum = np.sum(np.abs(p[:, :, 0] * self.N[None]), axis=-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num / dn
            dl = np.linalg.norm(d, axis=-1)[:, None]
            tol = 16 * U * (snum + np.abs(t) * sdn) / np.abs(dn) + 8 * U * (np.abs(O).max(axis=-1)[:, None] + np.abs(t) * dl) / dl
        graze = sdn > GRAZE * np.abs(dn)
        bad = ~np.isfinite(t) | (self.gid[None] == self_id[:, None])
        if blockers:
            bad |= self.water[None]
        tm = tmin[:, None]
        sure = sure & ~bad & ~graze & (t - tol > tm)
        poss = poss & ~bad & (t + tol > tm)
        if not blockers:
            S = len(O)
            ft, ftol, fs, fp = np.full(S, np.inf), np.zeros(S), np.zeros(S, bool), np.zeros(S, bool)
            if self.floor is not None:
                y, x0, x1, z0, z1, _ = self.floor
                with np.errstate(divide="ignore", invalid="ignore"):
                    ft = (y - O[:, 1]) / d[:, 1]
                ftol = 3 * U * np.abs(ft)
                X, Z = O[:, 0] + ft * d[:, 0], O[:, 2] + ft * d[:, 2]
                m = 8 * U * (np.abs(O).max(axis=-1) + np.abs(ft) * dl[:, 0])
                ok = np.isfinite(ft) & (self_id != FLOOR_ID)
                inner = np.minimum(np.minimum(X - x0, x1 - X), np.minimum(Z - z0, z1 - Z))
                fs = ok & (inner > m) & (ft - ftol > tmin)
                fp = ok & (inner > -m) & (ft + ftol > tmin)
                ft = np.where(np.isfinite(ft), ft, np.inf)
            t, tol = np.concatenate([t, ft[:, None]], axis=1), np.concatenate([tol, ftol[:, None]], axis=1)
            sure, poss = np.concatenate([sure, fs[:, None]], axis=1), np.concatenate([poss, fp[:, None]], axis=1)
            graze = np.concatenate([graze, np.zeros((S, 1), bool)], axis=1)
        return np.where(poss, t, np.inf), np.where(poss, tol, 0.0), sure, poss, graze

    def closest(self, O, d, tmin, self_id):
        """(candidates (S, T + 1), ids of the columns) by the sure / possible rule"""
        t, tol, sure, poss, graze = self.hits(O, d, tmin, self_id)
        t_sure = np.where(sure, t + tol, np.inf).min(axis=1, initial=np.inf)
        cand = poss & (t - tol <= (t_sure + PICK * np.abs(t_sure))[:, None])
        return cand, t, tol, graze, np.concatenate([self.gid, [FLOOR_ID]])

    def blocked(self, P, self_id):
        """(sure blocked, possibly blocked) of the light as seen from P"""
        L = self.light[None] - P
        t, tol, sure, poss, _ = self.hits(P, L, np.zeros(len(P)), self_id, blockers=True)
        return (sure & (t - tol > 0) & (t + tol < 1)).any(axis=1), (poss & (t - tol < 1)).any(axis=1)

    def normal_at(self, tri, O, d, water):
        """(the unit normal the device uses for triangles tri (n,) hit by rays O + t d, its bound, side open): the blend or the face
        normal, turned against the ray; for water the blend only where it lies on the geometric normal's side of the ray"""
        C, vn = self.C[tri], self.VN[tri]
        p = C - O[:, None, :]

        def edge(a, b):
            e = np.sum(d * np.cross(a, b), axis=-1)
            A = (np.abs(d[:, 0]) * (np.abs(a[:, 1] * b[:, 2]) + np.abs(a[:, 2] * b[:, 1])) + np.abs(d[:, 1]) * (np.abs(a[:, 2] * b[:, 0]) + np.abs(a[:, 0] * b[:, 2]))
                 + np.abs(d[:, 2]) * (np.abs(a[:, 0] * b[:, 1]) + np.abs(a[:, 1] * b[:, 0])))
            return e, A
        (w0, a0), (w1, a1), (w2, a2) = edge(p[:, 1], p[:, 2]), edge(p[:, 2], p[:, 0]), edge(p[:, 0], p[:, 1])
        bl = w0[:, None] * vn[:, 0] + w1[:, None] * vn[:, 1] + w2[:, None] * vn[:, 2]
        bl = np.where((w0 + w1 + w2 < 0)[:, None], -bl, bl)
        nb = np.linalg.norm(bl, axis=-1)
        blended = ~self.flat[tri] & (nb > 0)
        face = unit(self.N[tri])
        with np.errstate(divide="ignore", invalid="ignore"):
            ns = np.where(blended[:, None], bl / nb[:, None], face)
            tol = np.where(blended, 8 * U * (a0 * np.linalg.norm(vn[:, 0], axis=-1) + a1 * np.linalg.norm(vn[:, 1], axis=-1)
                                             + a2 * np.linalg.norm(vn[:, 2], axis=-1)) / nb + 24 * U, FLAT_TOL)
        dl = np.linalg.norm(d, axis=-1)
        nd = np.sum(ns * d, axis=-1)
        open_side = blended & (np.abs(nd) < SIDE * dl)
        ng = np.where(self.flip[tri][:, None], -self.N[tri], self.N[tri])
        back = water & blended & ~(nd * np.sum(ng * d, axis=-1) > 0)   # the blend on the far side of the ray: the geometric normal
        ns = np.where(back[:, None], face, ns)
        tol = np.where(back, FLAT_TOL, tol)
        ns = np.where((np.sum(ns * d, axis=-1) > 0)[:, None], -ns, ns)
        return ns, tol, open_side

    def floor_tone(self, P):
        """(tone 0..255, sure) of the checker at floor points P"""
        y, x0, x1, z0, z1, cell = self.floor
        a, b = (P[:, 0] - x0) / cell, (P[:, 2] - z0) / cell
        sure = (np.abs(a - np.round(a)) > 2.0 ** -12) & (np.abs(b - np.round(b)) > 2.0 ** -12)
        return np.where((np.floor(a) + np.floor(b)).astype(np.int64) & 1, 128.0, 204.0), sure


def check_hits(paths, sc, stride=1, chunk=None):
    """Every recorded segment of every stride-th pixel against the scene in float64, from the device's own origin and direction: the
    hit id among the candidates; where the winner is not ambiguous and the ray does not graze: t and the normal (face or blend); where
    the segment ends on a diffuse triangle or the floor: the shadow word against the light's visibility and the contribution; where it
    is a water hit that reflects: the reflection's hit id, shadow flag and colour (_check_reflections).  Returns the counts."""
    chunk = chunk or max(1, 1000000 // max(len(sc.gid), 1))
    sub = np.ascontiguousarray(paths[::stride, ::stride])
    H, W, D, _ = sub.shape
    P, I = sub.astype(np.float64).reshape(-1, D, 24), sub.view(np.int32).reshape(-1, D, 24)
    rep = dict(segments=0, ambiguous=0, grazing=0, near_miss=0, shaded=0, normals=0, blended=0, reflections=0)
    col_of = {int(g): k for k, g in enumerate(sc.gid)}
    for k in range(D):
        use = (I[:, k, W_FLAGS] & F_USED) != 0
        idx = np.nonzero(use)[0]
        for c0 in range(0, len(idx), chunk):
            s = idx[c0:c0 + chunk]
            O, d, hid, trec = P[s, k, 0:3], P[s, k, 3:6], I[s, k, W_ID], P[s, k, W_T]
            self_id = I[s, k - 1, W_ID] if k else np.full(len(s), -99)
            tmin = np.full(len(s), sc.zn if k == 0 else 0.0)
            cand, t, tol, graze, ids = sc.closest(O, d, tmin, self_id)
            n_c = cand.sum(axis=1)
            rep["segments"] += len(s)
            for j in range(len(s)):   # the device's id is a candidate; a miss only where nothing is sure
                if hid[j] == -1:
                    assert not (cand[j] & (t[j] < np.inf)).any() or n_c[j] == 0 or not sc.hits(O[j:j + 1], d[j:j + 1], tmin[j:j + 1], self_id[j:j + 1])[2].any(), (k, int(s[j]))
                else:
                    assert cand[j, ids == hid[j]].any(), (k, int(s[j]), int(hid[j]), ids[cand[j]].tolist())
            col = np.array([np.nonzero(ids == h)[0][0] if h != -1 else 0 for h in hid])
            gz = graze[np.arange(len(s)), col] & (hid != -1)
            amb = (n_c > 1) & ~gz
            rep["ambiguous"] += int(amb.sum()); rep["grazing"] += int(gz.sum())
            clear = (n_c == 1) & ~gz & (hid != -1)
            dt = np.abs(trec - t[np.arange(len(s)), col]) / np.maximum(tol[np.arange(len(s)), col], 1e-300)
            assert dt[clear].max(initial=0.0) <= 1.0, (k, dt[clear].max())
            is_floor = hid == FLOOR_ID
            tri = np.array([col_of.get(int(h), 0) for h in hid])
            # the normal of every clear triangle hit: the blend or the face normal (water: the side rule), turned against the ray
            on_tri = clear & (hid >= 0)
            if on_tri.any():
                q = np.nonzero(on_tri)[0]
                n_want, n_tol, open_side = sc.normal_at(tri[q], O[q], d[q], sc.water[tri[q]])
                rep["grazing"] += int(open_side.sum())
                dn = np.abs(P[s[q], k, W_N:W_N + 3] - n_want).max(axis=-1) / n_tol
                assert dn[~open_side].max(initial=0.0) <= 1.0, (k, "normal", dn[~open_side].max())
                rep["normals"] += int((~open_side).sum()); rep["blended"] += int((~open_side & ~sc.flat[tri[q]]).sum())
                # the reflection segment of a water hit: its hit among the candidates, its colour in the segment's contribution
                fl = I[s[q], k, W_FLAGS]
                wq = sc.water[tri[q]] & ((fl & F_TIR) == 0) & ~open_side & (P[s[q], k, W_F] > 0)
                if wq.any():
                    _check_reflections(sc, P[s[q][wq], k], I[s[q][wq], k], hid[q][wq], k == 0, rep, col_of)
            # segments that end on the floor or a diffuse triangle
            ends = clear & (is_floor | ((hid >= 0) & ~sc.water[tri])) if len(sc.gid) else clear & is_floor
            if not ends.any():
                continue
            e = np.nonzero(ends)[0]
            Pt = O[e] + trec[e, None] * d[e]
            n_rec = P[s[e], k, W_N:W_N + 3]
            fe = is_floor[e]
            up = np.where((d[e][:, 1] > 0)[:, None], np.float64([0.0, -1.0, 0.0]), np.float64([0.0, 1.0, 0.0]))
            assert np.abs(n_rec - up)[fe].max(initial=0.0) <= FLAT_TOL, (k, "floor normal")
            L = sc.light[None] - Pt
            ndl = np.maximum(np.sum(n_rec * L, axis=-1) / np.linalg.norm(L, axis=-1), 0.0)
            sh = I[s[e], k, W_SHADOW]
            sure_b, poss_b = sc.blocked(Pt, hid[e])
            cast = sh >= 0
            near = cast & poss_b & ~sure_b
            rep["near_miss"] += int(near.sum())
            assert not (cast & (sh == 1) & ~poss_b).any(), (k, "a shadow where nothing can block the light")
            assert not (cast & (sh == 0) & sure_b).any(), (k, "no shadow where the light is surely blocked")
            assert (cast == (sc.shadows & (ndl > 8 * U)))[np.abs(ndl) > 16 * U].all() if sc.shadows else not cast.any()
            base = sc.col[tri[e]] / 255.0 if len(sc.gid) else np.zeros((len(e), 3))
            tone_sure = np.ones(len(e), bool)
            if is_floor[e].any():
                tone, ts = sc.floor_tone(Pt)
                base = np.where(is_floor[e, None], tone[:, None] / 255.0, base)
                tone_sure = ~is_floor[e] | ts
            thr = P[s[e], k, W_THR0:W_THR0 + 3]
            ins = (I[s[e], k, W_FLAGS] & F_INSIDE) != 0
            ok = tone_sure & ~ins   # (a segment that ends on a solid inside the fluid: the absorbing colour is not recorded)
            want = thr * base * (sc.amb + np.where(sh == 1, 0.0, ndl)[:, None] * sc.lrgb[None])
            got = P[s[e], k, W_ADD:W_ADD + 3]
            assert np.abs(got - want)[ok].max(initial=0.0) <= ADD_TOL, (k, np.abs(got - want)[ok].max())
            rep["shaded"] += int(ok.sum())
    return rep


def _check_reflections(sc, R, RI, hid, primary, rep, col_of):
    """R (n, 24) records of clear water hits that reflect: the reflection ray from the recorded normal, its hit id (word 21) among the
    candidates, the shadow flag against the visibility, and throughput x F x colour in words 17-19"""
    O, d, t, n, F = R[:, 0:3], R[:, 3:6], R[:, W_T], R[:, W_N:W_N + 3], R[:, W_F]
    Pt = O + t[:, None] * d
    du = unit(d)
    rd = unit(du - 2.0 * np.sum(du * n, axis=-1)[:, None] * n)
    cand, tt, tol, graze, ids = sc.closest(Pt, rd, np.zeros(len(Pt)), hid)
    rid = RI[:, W_RID]
    n_c = cand.sum(axis=1)
    for j in range(len(Pt)):
        if rid[j] == -1:
            assert n_c[j] == 0 or not sc.hits(Pt[j:j + 1], rd[j:j + 1], np.zeros(1), hid[j:j + 1])[2].any(), ("reflection", j)
        else:
            assert cand[j, ids == rid[j]].any(), ("reflection", j, int(rid[j]), ids[cand[j]].tolist())
    col = np.array([np.nonzero(ids == h)[0][0] if h != -1 else 0 for h in rid])
    clear = ((n_c == 1) & (rid != -1) & ~graze[np.arange(len(Pt)), col]) | ((n_c == 0) & (rid == -1))
    tri = np.array([col_of.get(int(h), 0) for h in rid])
    is_floor, on_tri = rid == FLOOR_ID, rid >= 0
    solid = is_floor | (on_tri & ~sc.water[tri]) if len(sc.gid) else is_floor
    tr = np.where(rid != -1, tt[np.arange(len(Pt)), col], 0.0)
    tr = np.where(np.isfinite(tr), tr, 0.0)
    Pr = Pt + tr[:, None] * rd
    nn = np.tile(np.float64([0.0, 1.0, 0.0]), (len(Pt), 1))
    nn = np.where((rd[:, 1] > 0)[:, None], -nn, nn)
    open_side = np.zeros(len(Pt), bool)
    if (on_tri & solid).any():
        g = np.nonzero(on_tri & solid)[0]
        nn[g], _, open_side[g] = sc.normal_at(tri[g], Pt[g], rd[g], np.zeros(len(g), bool))
    L = sc.light[None] - Pr
    Ll = np.linalg.norm(L, axis=-1)
    ndl = np.maximum(np.sum(nn * L, axis=-1) / Ll, 0.0)
    shadowed = (RI[:, W_FLAGS] & F_RSHADOW) != 0
    sure_b, poss_b = sc.blocked(Pr, rid)
    chk = clear & solid & ~open_side
    cast = chk & sc.shadows & (ndl > 64 * U)
    rep["near_miss"] += int((cast & poss_b & ~sure_b).sum())
    assert not (chk & shadowed & ~poss_b).any(), "a reflection in shadow where nothing can block the light"
    assert not (cast & ~shadowed & sure_b).any(), "a lit reflection where the light is surely blocked"
    base = sc.col[tri] / 255.0 if len(sc.gid) else np.zeros((len(Pt), 3))
    tone_sure = np.ones(len(Pt), bool)
    if is_floor.any():
        tone, ts = sc.floor_tone(Pr)
        base = np.where(is_floor[:, None], tone[:, None] / 255.0, base)
        tone_sure = ~is_floor | ts
    C = np.where(solid[:, None], base * (sc.amb + np.where(shadowed, 0.0, ndl)[:, None] * sc.lrgb[None]), sc.bg[None] / 255.0)
    # the throughput at the hit: the start's, absorbed along a segment inside the fluid (the colour of the mesh that is left)
    inside = (RI[:, W_FLAGS] & F_INSIDE) != 0
    length = t * (np.linalg.norm(d, axis=-1) if primary else 1.0)
    acol = sc.col[np.array([col_of.get(int(h), 0) for h in hid])] if len(sc.gid) else np.zeros((len(Pt), 3))
    thr = R[:, W_THR0:W_THR0 + 3] * np.where(inside[:, None], transmittance(np.zeros(3), sc.absorb, sc.radius, length) ** (1.0 - acol / 255.0), 1.0)
    want = thr * F[:, None] * C
    tolr = ADD_TOL + 2.0 * DIR_TOL * tr / np.maximum(Ll, 1e-300) + THR_TOL
    ok = clear & tone_sure & ~open_side & ~(cast & poss_b & ~sure_b)
    over = np.abs(R[:, W_ADD:W_ADD + 3] - want).max(axis=-1) / tolr
    assert over[ok].max(initial=0.0) <= 1.0, ("reflection colour", over[ok].max())
    rep["reflections"] += int(ok.sum())


def trace64(sc, O, d, max_depth, mutant=None, chunk=256):
    """The paths of rays O + t d (S, 3) through the scene in float64, flat normals throughout, as records in the device's layout
    (S, max_depth, 24) float32, with the number of segments and of UNSURE ones: an ambiguous winner, a grazing ray, Snell's discriminant
    within K_TOL of zero, a shadow ray that is a near miss.  mutant: "shadow_uncut" (a shadow ray is not cut at the light) or
    "self_hit" (a path segment may hit the triangle it starts on) -- what a broken device would record."""
    S = len(O)
    rec = np.zeros((S, max_depth, 24))
    ints = np.zeros((S, max_depth, 24), np.int64)
    ints[..., W_ID] = ints[..., W_SHADOW] = ints[..., W_RID] = -1
    O, d = O.astype(np.float64).copy(), d.astype(np.float64).copy()
    thr, alive, inside = np.ones((S, 3)), np.ones(S, bool), np.zeros(S, bool)
    self_id, wcol = np.full(S, -99), np.zeros((S, 3))
    n_seg = n_unsure = 0
    ids = np.concatenate([sc.gid, [FLOOR_ID]])

    def first(Oa, da, tmin, sid):
        out = [[], [], [], []]
        for c0 in range(0, len(Oa), chunk):
            sl = slice(c0, c0 + chunk)
            cand, t, tol, graze, _ = sc.closest(Oa[sl], da[sl], tmin[sl], sid[sl])
            w = np.where(cand, t, np.inf).argmin(axis=1)
            hit = cand.any(axis=1)
            out[0].append(np.where(hit, w, -1)); out[1].append(t[np.arange(len(w)), w])
            out[2].append(cand.sum(axis=1) > 1); out[3].append(graze[np.arange(len(w)), w] & hit)
        return [np.concatenate(x) for x in out]

    def shade(Pa, da, col, hid):
        """(colour (n, 3), normal, shadow word, near miss) of diffuse / floor hits: col is the column of the hit"""
        fl = col == len(sc.gid)
        N = np.where(fl[:, None], np.float64([0.0, 1.0, 0.0]), unit(sc.N[np.minimum(col, max(len(sc.gid) - 1, 0))]) if len(sc.gid) else np.float64([0.0, 1.0, 0.0]))
        N = np.where((np.sum(N * da, axis=-1) > 0)[:, None], -N, N)
        L = sc.light[None] - Pa
        ndl = np.maximum(np.sum(N * L, axis=-1) / np.linalg.norm(L, axis=-1), 0.0)
        sh, near = np.full(len(Pa), -1), np.zeros(len(Pa), bool)
        cast = sc.shadows & (ndl > 0)
        if cast.any():
            if mutant == "shadow_uncut":
                t, tol, sure, poss, _ = sc.hits(Pa[cast], L[cast], np.zeros(int(cast.sum())), hid[cast], blockers=True)
                sb = pb = (sure & (t > 0)).any(axis=1)
            else:
                sb, pb = sc.blocked(Pa[cast], hid[cast])
            sh[cast] = pb.astype(int)
            near[cast] = pb & ~sb
        base = sc.col[np.minimum(col, max(len(sc.gid) - 1, 0))] / 255.0 if len(sc.gid) else np.zeros((len(Pa), 3))
        if fl.any():
            base = np.where(fl[:, None], sc.floor_tone(Pa)[0][:, None] / 255.0, base)
        return base * (sc.amb + np.where(sh == 1, 0.0, ndl)[:, None] * sc.lrgb[None]), N, sh, near

    for k in range(max_depth):
        a = np.nonzero(alive)[0]
        if not len(a):
            break
        tmin = np.full(len(a), sc.zn if k == 0 else 0.0)
        sid = np.full(len(a), -99) if mutant == "self_hit" else self_id[a]
        col, t, amb, gz = first(O[a], d[a], tmin, sid)
        if mutant == "self_hit" and k:   # the triangle the segment starts on, at no distance
            own = np.array([np.nonzero(ids == s)[0][0] if s in ids else -1 for s in self_id[a]])
            col, t = np.where(own >= 0, own, col), np.where(own >= 0, 2.0 ** -20, t)
        n_seg += len(a)
        unsure = amb | gz
        hit = col >= 0
        hid = np.where(hit, ids[np.maximum(col, 0)], -1)
        rec[a, k, 0:3], rec[a, k, 3:6], rec[a, k, W_T] = O[a], d[a], np.where(hit, t, 0.0)
        rec[a, k, W_THR0:W_THR0 + 3] = thr[a]
        ints[a, k, W_ID], ints[a, k, W_FLAGS] = hid, F_USED
        Pt = O[a] + np.where(hit, t, 0.0)[:, None] * d[a]
        is_water = hit & (col < len(sc.gid)) & sc.water[np.minimum(col, max(len(sc.gid) - 1, 0))] if len(sc.gid) else np.zeros(len(a), bool)
        # misses: the background
        miss = ~hit
        rec[a[miss], k, W_ADD:W_ADD + 3] = thr[a[miss]] * sc.bg / 255.0
        # water hits decide inside by the sign of d . Ng
        dng = np.sum(d[a] * sc.N[np.minimum(col, max(len(sc.gid) - 1, 0))], axis=-1) if len(sc.gid) else np.zeros(len(a))
        ins = np.where(is_water, dng >= 0, inside[a])
        acol = np.where(is_water[:, None], sc.col[np.minimum(col, max(len(sc.gid) - 1, 0))] if len(sc.gid) else 0.0, wcol[a])
        length = t * (np.linalg.norm(d[a], axis=-1) if k == 0 else 1.0)
        th = np.where((ins & hit)[:, None], thr[a] * transmittance(np.zeros(3), sc.absorb, sc.radius, np.where(hit, length, 0.0)) ** (1.0 - acol / 255.0), thr[a])
        ints[a, k, W_FLAGS] |= np.where(ins & hit & (is_water | inside[a]), F_INSIDE, 0)
        # diffuse and floor hits end the path
        e = hit & ~is_water
        if e.any():
            C, N, sh, near = shade(Pt[e], d[a][e], col[e], hid[e])
            rec[a[e], k, W_ADD:W_ADD + 3], rec[a[e], k, W_N:W_N + 3], ints[a[e], k, W_SHADOW] = th[e] * C, N, sh
            unsure[e] |= near
        # water: Snell, Schlick, one reflection segment
        w = np.nonzero(is_water)[0]
        if len(w):
            n = unit(sc.N[col[w]])
            entering = dng[w] < 0
            n = np.where(entering[:, None], n, -n)
            eta = np.where(entering, 1.0 / sc.ior, sc.ior)
            refr, refl, kk, ci = snell(d[a][w], n, eta)
            unsure[w] |= np.abs(kk) < K_TOL
            tir = kk < 0
            with np.errstate(invalid="ignore"):
                F = np.where(tir, 0.0, schlick(np.where(entering, ci, np.sqrt(kk)), sc.ior))
            # the reflection
            rcol, rt, ramb, rgz = first(Pt[w], refl, np.zeros(len(w)), hid[w])
            C = np.tile(sc.bg / 255.0, (len(w), 1))
            rs = (rcol >= 0) & ~tir & ~((rcol < len(sc.gid)) & sc.water[np.minimum(rcol, len(sc.gid) - 1)])
            anyhit = (rcol >= 0) & ~tir
            ints[a[w[anyhit]], k, W_RID] = ids[rcol[anyhit]]   # (a reflection that meets water is recorded, and adds the background)
            if rs.any():
                rid = ids[rcol[rs]]
                Cr, _, shr, _ = shade(Pt[w][rs] + rt[rs, None] * refl[rs], refl[rs], rcol[rs], rid)
                C[rs] = Cr
                ints[a[w[rs]], k, W_RID] = rid
                ints[a[w[rs]], k, W_FLAGS] |= np.where(shr == 1, F_RSHADOW, 0)
            rec[a[w], k, W_ADD:W_ADD + 3] = th[w] * F[:, None] * C
            nthr = th[w] * (1.0 - F)[:, None]
            rec[a[w], k, W_N:W_N + 3], rec[a[w], k, W_F], rec[a[w], k, W_THR1:W_THR1 + 3] = n, F, nthr
            ints[a[w], k, W_FLAGS] |= np.where(entering, F_ENTER, 0) | np.where(tir, F_TIR, 0)
            g = a[w]
            thr[g], O[g], d[g] = nthr, Pt[w], np.where(tir[:, None], refl, refr)
            inside[g], wcol[g], self_id[g] = entering | tir, sc.col[col[w]], hid[w]
        n_unsure += int(unsure.sum())
        alive[a[~is_water]] = False
    paths = rec.astype(np.float32)
    pi = paths.view(np.int32)
    for wd in (W_ID, W_SHADOW, W_RID, W_FLAGS):
        pi[..., wd] = ints[..., wd]
    return paths, n_seg, n_unsure
