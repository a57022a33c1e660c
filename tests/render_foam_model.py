"""Restatement of the diffuse particles in the surface frames (include/sph_hip.h sph_render_set_surface_foam), for the tests.

splat() restates the splat in np.float32, operation for operation (one rounding each, sums from the left, IEEE division and square root,
as the kernel runs them with contraction off), given the diffuse particles, the camera and the DEVICE's planes of the foam-free frame:
its key plane key0, its surface flags and, thickness mode, its opaque key plane.  The three integer planes and the four counters must
agree with the device exactly.  front_depth() draws a key plane of spheres with the same sequence, for the host tests and for choosing
seeds without a device.

The colour stage is float64 here and f32 there; the bounds are per pixel and channel, in 8-bit steps.  U = 2^-24.

I(F) = 1 - exp2(-x), x = density (F / 256).  The conversion of F rounds once above 2^24, the division by 256 is exact, the product
rounds once: x carries a relative error of at most 2 U.  d(2^-x) = ln 2 2^-x dx, the hardware exp2 is documented to 1 ulp = 2 U relative
and flushes a denormal result to zero (2^-126 absolute), and the subtraction from 1 rounds once more (the result is at most 1):
    dI = e (ln 2 x 2 + 2) U + 2^-126 + U,   e = 2^-x.

Over layer, v = cur' (1 - I) + f I with cur' = cur / 255 and f = rgb / 255 from exact bytes.  I enters as I (f - cur'): dI |f - cur'|.
The remaining roundings (two divisions by 255, 1 - I, two products, one sum; every value at most 1) are 6 U, taken as 8 U.  One 8-bit
rounding step: floor(255 x + 0.5) of two values dv apart differ by at most floor(255 dv) + 1.
    tol_over = 1 + floor(255 (dI |f - cur'| + 8 U)).
Where the pixel was recomputed by the under layer just before, the byte `cur` itself may differ from the model's by tol_under; it
enters with the factor (1 - I): tol = tol_over + ceil(tol_under (1 - I)).

Under layer, v = (lit (1 - a1) + a1 (f Iu + (1 - Iu) (lit (1 - a2) + a2 behind))) + hi.  lit and hi are section 24's two terms with section
24's errors e_lit and e_hi as tests/render_thickness_model.py states them; lit enters with the factor (1 - a1) + a1 (1 - Iu) (1 - a2) <= 1.
a_k = exp2(-(k T_k)) with k T_k built by six rounded operations from non-negative terms, as section 25's tau: da_k = a_k (ln 2 k T_k 8 + 2) U
+ 2^-126.  a1 enters as a1 (mid - lit), a2 as a1 (1 - Iu) a2 (behind - lit), Iu as a1 Iu (f - deep), with mid and deep the two brackets:
    err = e_lit + e_hi + da1 |mid - lit| + da2 a1 (1 - Iu) |behind - lit| + dIu a1 |f - deep| + 16 U vmax,
the last term for the sixteen remaining roundings of values of at most vmax = 1 + lmax (1 + spec).
    tol_under = 1 + floor(255 err)."""
from __future__ import annotations

import numpy as np

from tests import render_thickness_model as TM

F = np.float32
U = 2.0 ** -24
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
NONE32 = np.uint32(0xFFFFFFFF)
DEFAULTS = dict(radius_scale=0.5, density=1.0, depth_bias=1.0, rgb=(255, 255, 255), raw_spheres=True)


def _pairs(xyz, rad, W, H, zn, camera, pair_budget=1 << 21):
    """Yields, chunk by chunk, the (sphere, pixel) pairs of spheres of radius `rad` (a float64; the device rounds it and its square to
    f32 once each) over a superset of the device's conservative bounds: (sphere index, pixel index, t0, t1, hit), t0 / t1 in f32."""
    E, f, s, u, tx, ty = TM.device_camera(W, H, **camera)
    x = np.asarray(xyz, F).reshape(-1, 3)
    r, r2 = F(rad), F(float(rad) * float(rad))
    zn = F(zn)
    Xc, Yr = TM.pixel_rays32(W, H, tx, ty)
    with np.errstate(invalid="ignore", over="ignore"):
        vx, vy, vz = x[:, 0] - E[0], x[:, 1] - E[1], x[:, 2] - E[2]
        xs = (s[0] * vx + s[1] * vy) + s[2] * vz
        ys = (u[0] * vx + u[1] * vy) + u[2] * vz
        z = (f[0] * vx + f[1] * vy) + f[2] * vz
    assert xs.dtype == F and z.dtype == F
    ok = np.isfinite(x).all(axis=1) & (z + r > zn)
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
        yield P, jj * W + ii, t0, t1, hit
        start = stop


def front_depth(xyz, radius, W, H, zn=0.1, **camera):
    """The key plane u64 (H, W) of spheres at xyz: float_bits(t0) << 32 | sphere index of the nearest hit, all ones where none."""
    key = np.full(W * H, ALL_ONES, np.uint64)
    for P, pix, t0, t1, hit in _pairs(xyz, float(F(radius)), W, H, zn, camera):
        k = (t0[hit].view(np.uint32).astype(np.uint64) << np.uint64(32)) | P[hit].astype(np.uint64)
        np.minimum.at(key, pix[hit], k)
    return key.reshape(H, W)


def key_depth(key):
    """(t f32, present bool), flat, of a key plane."""
    key = np.asarray(key, np.uint64).reshape(-1)
    return (key >> np.uint64(32)).astype(np.uint32).view(F), key != ALL_ONES


def splat(xyz, radius, key0, flag, okey=None, radius_scale=0.5, depth_bias=1.0, zn=0.1, **camera):
    """The planes of the diffuse particles xyz f32[n, 3] on the foam-free frame's key plane key0 u64 (H, W) and surface flags
    flag bool (H, W); okey: the opaque layer's key plane in thickness mode, None in the opaque surface mode.
    (fo, fu, du uint32 (H, W), dict(adds_over, adds_under, clipped, removed))."""
    key0 = np.asarray(key0, np.uint64)
    H, W = key0.shape
    r = F(radius)
    inv_u = F(256.0 / float(r))
    bias = F(float(depth_bias) * float(r))
    tw_all, has_w = key_depth(key0)
    thick = okey is not None
    top_all, has_all = key_depth(okey) if thick else (tw_all, has_w)
    flag = np.asarray(flag, bool).reshape(-1)
    fo, fu = np.zeros(W * H, np.int64), np.zeros(W * H, np.int64)
    du = np.full(W * H, int(NONE32), np.int64)
    st = dict(adds_over=0, adds_under=0, clipped=0, removed=0)
    for P, pix, t0, t1, hit in _pairs(xyz, float(radius_scale) * float(radius), W, H, zn, camera):
        with np.errstate(invalid="ignore", over="ignore"):
            top = top_all[pix]
            cut = has_all[pix] & (top < t1)
            b = np.where(cut, top, t1)
            add = hit & (b > t0)
            c = ((b - t0) * inv_u).astype(F)
            tw = tw_all[pix]
            under = add & thick & flag[pix] & (t0 >= tw + bias)
            dq = ((t0 - tw) * inv_u).astype(F)
        over = add & ~under
        np.add.at(fo, pix[over], c[over].astype(np.int64))
        np.add.at(fu, pix[under], c[under].astype(np.int64))
        np.minimum.at(du, pix[under], dq[under].astype(np.int64))
        st["adds_over"] += int(over.sum())
        st["adds_under"] += int(under.sum())
        st["clipped"] += int((add & cut).sum())
        st["removed"] += int((hit & ~add).sum())
    assert max(fo.max(initial=0), fu.max(initial=0)) < 1 << 32
    return fo.reshape(H, W).astype(np.uint32), fu.reshape(H, W).astype(np.uint32), du.reshape(H, W).astype(np.uint32), st


def intensity(Fsum, density):
    """I(F) in float64, density as the device holds it (f32)."""
    return 1.0 - np.exp2(-(float(F(density)) * (np.asarray(Fsum).astype(np.float64) / 256.0)))


def intensity32(Fsum, density):
    """I(F) in f32 with the device's operation order (numpy's exp2 in place of the hardware's)."""
    x = F(density) * (np.asarray(Fsum).astype(F) / F(256))
    return F(1) - np.exp2(-x).astype(F)


def _d_intensity(Fsum, density):
    x = float(F(density)) * (np.asarray(Fsum).astype(np.float64) / 256.0)
    e = np.exp2(-x)
    return e * (np.log(2.0) * x * 2 + 2) * U + 2.0 ** -126 + U


def render_byte(v):
    """floor(255 clamp(v, 0, 1) + 0.5), float64."""
    return np.floor(255 * np.clip(v, 0, 1) + 0.5)


def over(cur_rgb, fo, rgb=(255, 255, 255), density=1.0):
    """The over layer on the bytes cur_rgb uint8 (H, W, 3): (rgb uint8, tol int (H, W, 3)); pixels with fo == 0 or I == 0 keep their
    bytes with tol 0."""
    fo = np.asarray(fo)
    I = intensity(fo, density)[..., None]
    I32 = intensity32(fo, density)
    on = ((fo > 0) & (I32 != 0))[..., None]
    cur = np.asarray(cur_rgb, np.float64) / 255.0
    f = np.asarray(rgb, np.float64) / 255.0
    out = render_byte(cur * (1.0 - I) + f * I)
    err = _d_intensity(fo, density)[..., None] * np.abs(f - cur) + 8 * U
    res = np.where(on, out, np.asarray(cur_rgb, np.float64)).astype(np.uint8)
    tol = np.where(on, 1 + np.floor(255.0 * err), 0).astype(np.int64)
    return res, tol


def under_value(lit, hi, behind, f, kc, T, du, Iu):
    """The under expression in float64 from its terms (arrays that broadcast): the value before render_byte, and mid, deep, a1, a2,
    kT1, kT2."""
    Tm = np.maximum(np.asarray(T).astype(np.float64), 1.0)
    m = np.minimum(Tm, np.asarray(du).astype(np.float64))
    T1, T2 = m / 256.0, (Tm - m) / 256.0
    a1, a2 = np.exp2(-(kc * T1)), np.exp2(-(kc * T2))
    deep = lit * (1.0 - a2) + a2 * behind
    mid = f * Iu + (1.0 - Iu) * deep
    return (lit * (1.0 - a1) + a1 * mid) + hi, mid, deep, a1, a2, kc * T1, kc * T2


def under(surface_rgb, q, T, base_rgb, flag, opaque_rgb, fu, du, radius, absorb=0.05, scatter=0.01, rgb=(255, 255, 255), density=1.0,
          spec=0.35, shininess=40.0, **camera):
    """The under layer: surface_rgb with the flagged pixels of fu > 0 recomputed, and tol (H, W, 3) (0 where nothing was recomputed)."""
    flag = np.asarray(flag, bool)
    fu = np.asarray(fu)
    lit, hi, e_lit, e_hi, lmax = TM._surface_terms(np.asarray(q).astype(np.uint64), base_rgb, flag, radius, spec=spec, shininess=shininess, **camera)
    base = np.asarray(base_rgb, np.float64) / 255.0
    kc = float(F(absorb)) * (1.0 - base) + float(F(scatter))
    behind = np.asarray(opaque_rgb, np.float64) / 255.0
    f = np.asarray(rgb, np.float64) / 255.0
    Iu = intensity(fu, density)[..., None]
    on = (flag & (fu > 0) & (intensity32(fu, density) != 0))[..., None]
    val, mid, deep, a1, a2, x1, x2 = under_value(lit, hi, behind, f, kc, np.asarray(T)[..., None], np.asarray(du)[..., None], Iu)
    da1 = a1 * (np.log(2.0) * x1 * 8 + 2) * U + 2.0 ** -126
    da2 = a2 * (np.log(2.0) * x2 * 8 + 2) * U + 2.0 ** -126
    vmax = 1.0 + lmax * (1.0 + spec)
    err = (e_lit[..., None] + e_hi[..., None] + da1 * np.abs(mid - lit) + da2 * a1 * (1.0 - Iu) * np.abs(behind - lit) +
           _d_intensity(fu, density)[..., None] * a1 * np.abs(f - deep) + 16 * U * vmax)
    res = np.where(on, render_byte(val), np.asarray(surface_rgb, np.float64)).astype(np.uint8)
    tol = np.where(on, 1 + np.floor(255.0 * err), 0).astype(np.int64)
    return res, tol


def composite(surface_rgb, fo, fu=None, du=None, thick=None, rgb=(255, 255, 255), density=1.0):
    """The frame sph_render_surface leaves: surface_rgb -- the foam-free surface frame's bytes, the device's -- with the under layer
    (thick: dict(q, T, base_rgb, flag, opaque_rgb, radius, absorb, scatter, spec, shininess, camera...) in thickness mode, else None)
    and then the over layer.  (rgb uint8 (H, W, 3), tol int (H, W, 3))."""
    cur, tol_u = np.asarray(surface_rgb, np.uint8), 0
    if thick is not None:
        cur, tol_u = under(cur, fu=fu, du=du, rgb=rgb, density=density, **thick)
    out, tol_o = over(cur, fo, rgb=rgb, density=density)
    carried = np.ceil(tol_u * (1.0 - intensity(fo, density))[..., None]).astype(np.int64) if thick is not None else 0
    return out, np.where(tol_o > 0, tol_o + carried, tol_u)
