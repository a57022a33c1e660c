"""Restatement of the thickness mode of the surface frames (include/sph_hip.h sph_render_set_thickness), for the tests.

splat() restates the thickness splat in np.float32, operation for operation (one rounding each, sums from the left, IEEE division and
square root, as the kernel runs them with contraction off), given the particles, the camera and the DEVICE's opaque key plane -- the way
the depth model takes the device's key plane.  Its pixels are a superset of the device's conservative bounds: a pixel outside a sphere's
bounds fails the hit test.  smooth() is integer arithmetic.  Both must agree with the device exactly.

composite() is float64 here and f32 there; `tol` bounds per pixel, in 8-bit steps, how far the device's byte may be from the model's.
The device evaluates, per channel, v = (behind a + lit (1 - a)) + hi from exact integers (Q, T, the base colour, the opaque byte).
  * lit and hi are section 24's two terms and carry section 24's errors (tests/render_surface_model.py, restated in _surface_terms):
    the normal's, dn = SLACK 2^-24 (|a| |b| / |a x b| + 1), once through the Lambert term, shininess times through the highlight, plus
    the log2 / exp2 ulps of the power: e_lit = lmax dn, e_hi = lmax spec dhi.  lit enters with the factor (1 - a) <= 1.
  * a = exp2(-tau), tau = (absorb (1 - base) + scatter) Tr, Tr = max(T, 1) / 256.  tau is built from non-negative terms by six rounded
    operations (the conversion of T, base = byte / 255, 1 - base, the product with absorb, the sum with scatter, the product with Tr;
    the division by 256 is exact), so its relative error is at most 6 2^-24, taken as 8 2^-24.  d(2^-x) = ln 2 2^-x dx: the relative
    error of a is ln 2 tau 8 2^-24, plus the hardware exp2's documented 1 ulp = 2 2^-24 relative; v_exp_f32 flushes a denormal result
    to zero, at most 2^-126 absolute.  da = a (ln 2 tau 8 + 2) 2^-24 + 2^-126.
  * a enters v as a (behind - lit): that error is da |behind - lit|.
  * the remaining roundings (behind = byte / 255, two products, 1 - a, two sums; every value at most 1 + lmax (1 + spec)) : 8 2^-24 vmax.
  * one 8-bit rounding step: floor(255 x + 0.5) of two values dv apart differ by at most floor(255 dv) + 1.
tol = 1 + floor(255 (e_lit (1 - a) + e_hi + da |behind - lit| + 8 2^-24 vmax))."""
from __future__ import annotations

import numpy as np

from tests import render_model as RM
from tests import render_surface_model as SM

SENT = SM.SENT
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
U = SM.U
SLACK = SM.SLACK
DEFAULTS = dict(absorb=0.05, scatter=0.01, iterations=2)
F = np.float32


def device_camera(W, H, eye=(5.5, 2.5, 4.0), target=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=70.0):
    """The f32 camera constants as the host rounds them once: E, f, s, u (3 each), tx, ty."""
    E, f, s, u, tx, ty = RM.camera(eye, target, up, fov, W, H)
    return E.astype(F), f.astype(F), s.astype(F), u.astype(F), F(tx), F(ty)


def pixel_rays32(W, H, tx, ty):
    """render_X / render_Y in f32."""
    X = ((2 * np.arange(W) + 1).astype(F) / F(W) - F(1)) * tx
    Y = (F(1) - (2 * np.arange(H) + 1).astype(F) / F(H)) * ty
    return X, Y


def splat(xyz, okey, radius, zn=0.1, pair_budget=1 << 21, **camera):
    """The summed plane of the surface particles xyz f32[n, 3] in front of the opaque key plane okey u64 (H, W):
    (T uint32 (H, W), dict(adds, clipped, removed))."""
    okey = np.asarray(okey, np.uint64)
    H, W = okey.shape
    E, f, s, u, tx, ty = device_camera(W, H, **camera)
    x = np.asarray(xyz, F).reshape(-1, 3)
    r = F(radius)
    r2 = F(float(radius) * float(radius))
    inv_u = F(256.0 / float(r))
    zn = F(zn)
    Xc, Yr = pixel_rays32(W, H, tx, ty)
    top_all = (okey >> np.uint64(32)).astype(np.uint32).view(F).reshape(-1)
    has_all = (okey != ALL_ONES).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        vx, vy, vz = x[:, 0] - E[0], x[:, 1] - E[1], x[:, 2] - E[2]
        xs = (s[0] * vx + s[1] * vy) + s[2] * vz
        ys = (u[0] * vx + u[1] * vy) + u[2] * vz
        z = (f[0] * vx + f[1] * vy) + f[2] * vz
    assert xs.dtype == F and z.dtype == F
    ok = np.isfinite(x).all(axis=1) & (z + r > zn)
    # pixel bounds in float64 with two pixels of margin (the device takes one beyond its f32 tangents); the whole screen near the eye
    zd, xd, yd, rd = z.astype(np.float64), xs.astype(np.float64), ys.astype(np.float64), float(r)
    full = zd - rd <= float(zn) * 1.001
    with np.errstate(invalid="ignore", divide="ignore"):
        den = zd * zd - rd * rd
        qx, qy = rd * np.sqrt(np.maximum(xd * xd + den, 0)), rd * np.sqrt(np.maximum(yd * yd + den, 0))
        lim = 4.0 * max(W, H)
        c0 = np.clip(((xd * zd - qx) / den / float(tx) + 1) * 0.5 * W - 0.5, -lim, lim)
        c1 = np.clip(((xd * zd + qx) / den / float(tx) + 1) * 0.5 * W - 0.5, -lim, lim)
        r0 = np.clip((1 - (yd * zd + qy) / den / float(ty)) * 0.5 * H - 0.5, -lim, lim)
        r1 = np.clip((1 - (yd * zd - qy) / den / float(ty)) * 0.5 * H - 0.5, -lim, lim)
    c0 = np.where(full, -1, c0); c1 = np.where(full, W, c1); r0 = np.where(full, -1, r0); r1 = np.where(full, H, r1)
    c0, c1, r0, r1 = [np.nan_to_num(a, nan=0.0) for a in (c0, c1, r0, r1)]
    i0 = np.maximum(np.floor(c0).astype(np.int64) - 2, 0); i1 = np.minimum(np.ceil(c1).astype(np.int64) + 2, W - 1)
    j0 = np.maximum(np.floor(r0).astype(np.int64) - 2, 0); j1 = np.minimum(np.ceil(r1).astype(np.int64) + 2, H - 1)
    ok &= (i0 <= i1) & (j0 <= j1)
    idx = np.flatnonzero(ok)
    bw = (i1 - i0 + 1)[idx]
    area = bw * (j1 - j0 + 1)[idx]
    cum = np.cumsum(area)
    T = np.zeros(W * H, np.int64)
    st = dict(adds=0, clipped=0, removed=0)
    start = 0
    while start < len(idx):
        stop = max(start + 1, int(np.searchsorted(cum, (cum[start - 1] if start else 0) + pair_budget, side="right")))
        sel, a = idx[start:stop], area[start:stop]
        k_ = np.repeat(np.arange(len(sel)), a)
        q = np.arange(a.sum()) - np.repeat(np.cumsum(a) - a, a)
        P = sel[k_]
        ii = i0[P] + q % bw[start:stop][k_]
        jj = j0[P] + q // bw[start:stop][k_]
        X, Y = Xc[ii], Yr[jj]
        pxs, pys, pz = xs[P], ys[P], z[P]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            dd = (X * X + Y * Y) + F(1)
            k = ((X * pxs + Y * pys) + pz) / dd
            wx, wy, wz = pxs - k * X, pys - k * Y, pz - k
            h = r2 - ((wx * wx + wy * wy) + wz * wz)
            root = np.sqrt(np.where(h >= 0, h, F(0)) / dd)
            t0, t1 = k - root, k + root
            assert t0.dtype == F
            hit = (h >= 0) & (t0 > zn)
            pix = jj * W + ii
            top = top_all[pix]
            cut = has_all[pix] & (top < t1)
            b = np.where(cut, top, t1)
            add = hit & (b > t0)
            c = ((b - t0) * inv_u).astype(F)
        np.add.at(T, pix[add], c[add].astype(np.int64))
        st["adds"] += int(add.sum())
        st["clipped"] += int((add & cut).sum())
        st["removed"] += int((hit & ~add).sum())
        start = stop
    assert T.max(initial=0) < 1 << 32
    return T.reshape(H, W).astype(np.uint32), st


def smooth_once(T, Q, rnum, rmax):
    """One Jacobi step of the thickness plane T under the depth plane Q (SENT: not a surface pixel): (T', taps visited).  Section 24's
    integer tent with R_i from Q_i; a tap counts when it is in the frame and a surface pixel."""
    Q = np.asarray(Q).astype(np.uint64)
    H, W = Q.shape
    surf = Q != SENT
    R, _ = SM.window(Q, rnum, rmax)
    R = np.where(surf, R, -1)
    rm = int(R.max()) if surf.any() else 0
    padT = np.zeros((H + 2 * rm, W + 2 * rm), np.int64)
    padS = np.zeros((H + 2 * rm, W + 2 * rm), np.int64)
    padT[rm:rm + H, rm:rm + W] = np.asarray(T).astype(np.int64)
    padS[rm:rm + H, rm:rm + W] = surf
    tent = [np.maximum(R + 1 - k, 0) for k in range(rm + 1)]
    num = np.zeros((H, W), np.int64)
    den = np.zeros((H, W), np.int64)
    for dy in range(-rm, rm + 1):
        for dx in range(-rm, rm + 1):
            w = tent[abs(dy)] * tent[abs(dx)] * padS[rm + dy:rm + dy + H, rm + dx:rm + dx + W]
            num += w * padT[rm + dy:rm + dy + H, rm + dx:rm + dx + W]
            den += w
    out = np.asarray(T).astype(np.int64).copy()
    d = den[surf]
    out[surf] = (num[surf] + (d >> 1)) // d
    return out.astype(np.uint32), int(((2 * R[surf] + 1) ** 2).sum())


def smooth(T, Q, iterations, rnum, rmax):
    """All iterations: (T with 0 on non-surface pixels, taps visited)."""
    visited = 0
    T = np.asarray(T, np.uint32)
    for _ in range(iterations):
        T, v = smooth_once(T, Q, rnum, rmax)
        visited += v
    return np.where(np.asarray(Q).astype(np.uint64) != SENT, T, 0).astype(np.uint32), visited


def _surface_terms(q, base_rgb, flag, radius, eye=(5.5, 2.5, 4.0), target=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=70.0,
                   light=(2.0, 2.0, 2.0), light_rgb=(1.0, 1.0, 1.0), ambient=0.1, spec=0.35, shininess=40.0):
    """Section 24's colour stage (render_surface_model.shade restated) split into its two terms: lit (H, W, 3) = base (amb + max(n.L, 0)
    lrgb), hi (H, W, 3) = spec lrgb max(n.h, 0)^shininess, and their error bounds e_lit, e_hi (H, W)."""
    H, W = q.shape
    flag = np.asarray(flag, bool)
    E, f, s, u_, tx, ty = RM.camera(eye, target, up, fov, W, H)
    Xc, Yr = RM.pixel_rays(W, H, tx, ty)
    X, Y = np.broadcast_to(Xc[None, :], (H, W)), np.broadcast_to(Yr[:, None], (H, W))
    Xn = np.broadcast_to(np.append(Xc[1:], Xc[-1])[None, :], (H, W))
    Yn = np.broadcast_to(np.append(Yr[1:], Yr[-1])[:, None], (H, W))
    dX, dY = 2.0 * tx / W, -2.0 * ty / H
    uu = float(F(float(F(radius)) / 256.0))
    lv = np.asarray(light, np.float64) - E
    Lv = np.array([s @ lv, u_ @ lv, f @ lv])
    lrgb = np.asarray(light_rgb, np.float64)
    sx, sy, ql, qr, qu, qd = SM.sides(q)
    qi = np.where(flag, q.astype(np.int64), 1)
    z = qi * uu
    P = np.stack([z * X, z * Y, z], axis=2)
    e = -P / np.linalg.norm(P, axis=2, keepdims=True)
    dzx = np.where(sx > 0, qr - qi, qi - ql) * uu
    zx = np.where(sx > 0, z, ql * uu)
    a = np.stack([dzx * np.where(sx > 0, Xn, X) + zx * dX, dzx * Y, dzx], axis=2)
    dzy = np.where(sy > 0, qd - qi, qi - qu) * uu
    zy = np.where(sy > 0, z, qu * uu)
    b = np.stack([dzy * X, dzy * np.where(sy > 0, Yn, Y) + zy * dY, dzy], axis=2)
    c = np.cross(a, b)
    cl = np.linalg.norm(c, axis=2)
    both = flag & (sx != 0) & (sy != 0) & (cl > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(both[..., None], c / cl[..., None], e)
        n = np.where(((n * P).sum(axis=2) > 0)[..., None] & both[..., None], -n, n)
        dn = np.where(both, SLACK * U * np.linalg.norm(a, axis=2) * np.linalg.norm(b, axis=2) / np.where(both, cl, 1.0), 0.0) + SLACK * U
    Ld = Lv - P
    Ld /= np.linalg.norm(Ld, axis=2, keepdims=True)
    ndl = np.maximum((n * Ld).sum(axis=2), 0.0)
    h = Ld + e
    hl = np.linalg.norm(h, axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        ndh = np.where(hl > 0, np.maximum((n * h).sum(axis=2) / np.where(hl > 0, hl, 1.0), 0.0), 0.0)
        hi = np.where(ndh > 0, ndh ** shininess, 0.0)
        e2 = np.where(ndh > 0, np.abs(shininess * np.log2(np.where(ndh > 0, ndh, 1.0))), 0.0)
        dhi = shininess * np.where(ndh > 0, ndh ** (shininess - 1.0), 0.0) * dn + hi * (4 * U * (e2 + 4))
    base = np.asarray(base_rgb, np.float64) / 255.0
    lit = base * (ambient + ndl[..., None] * lrgb)
    lmax = float(lrgb.max())
    return lit, spec * hi[..., None] * lrgb, lmax * dn, lmax * spec * dhi, lmax


def composite(q, T, base_rgb, flag, opaque_rgb, frame_rgb, radius, absorb=0.05, scatter=0.01, spec=0.35, shininess=40.0, **camera):
    """rgb uint8 (H, W, 3) -- frame_rgb with the flagged pixels composited -- and tol (H, W, 3), the bound of the docstring.  q: the
    final depth plane, T: the smoothed thickness plane, opaque_rgb: the opaque layer's colours."""
    flag = np.asarray(flag, bool)
    lit, hi, e_lit, e_hi, lmax = _surface_terms(np.asarray(q).astype(np.uint64), base_rgb, flag, radius, spec=spec, shininess=shininess, **camera)
    ab, sc = float(F(absorb)), float(F(scatter))
    base = np.asarray(base_rgb, np.float64) / 255.0
    Tr = np.maximum(np.asarray(T).astype(np.float64), 1.0)[..., None] / 256.0
    tau = (ab * (1.0 - base) + sc) * Tr
    a = np.exp2(-tau)
    behind = np.asarray(opaque_rgb, np.float64) / 255.0
    val = (behind * a + lit * (1.0 - a)) + hi
    out = np.floor(255 * np.clip(val, 0, 1) + 0.5)
    da = a * (np.log(2.0) * tau * 8 + 2) * U + 2.0 ** -126
    vmax = 1.0 + lmax * (1.0 + spec)
    err = e_lit[..., None] * (1.0 - a) + e_hi[..., None] + da * np.abs(behind - lit) + 8 * U * vmax
    rgb = np.where(flag[..., None], out, np.asarray(frame_rgb, np.float64)).astype(np.uint8)
    tol = np.where(flag[..., None], 1 + np.floor(255.0 * err), 0).astype(np.int64)
    return rgb, tol
