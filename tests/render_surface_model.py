"""Restatement of the screen-space surface mode (include/sph_hip.h sph_render_set_surface), for the tests.

The depth stage -- quantise, the Jacobi smoothing, the choice of the neighbour a normal is taken from -- is integer arithmetic (uint64 /
int64 here, u32 / u64 on the device) and must agree with the device exactly.  The colour stage is float64 here and f32 there; `rgb_tol`
bounds, in 8-bit steps, how far the device may be from the model: one step of rounding plus 255 times the error of the lit value.  That
error comes from the normal -- the cross product c = a x b of two differences whose f32 evaluation carries a few roundings each, so
|dn| <= SLACK 2^-24 |a| |b| / |c| -- which enters the Lambert term once and the highlight shininess times (d x^s = s x^(s-1) dx), plus the
hardware log2 / exp2 of the highlight (1 ulp each, the exponent's error times ln 2)."""
from __future__ import annotations

import numpy as np

from tests import render_model as RM

SENT = 0xFFFFFFFF
QMAX = (1 << 24) - 1
U = 2.0 ** -24
SLACK = 16
DEFAULTS = dict(iterations=3, sigma=1.5, range=2.0, rmax=12, spec=0.35, shininess=40.0)


def constants(radius, H, fov, sigma=1.5, range=2.0):
    """(inv_u f32, u f32, Rnum, dq) as the host computes them once."""
    r = float(np.float32(radius))
    inv_u = np.float32(256.0 / r)
    u = np.float32(r / 256.0)
    ty = np.tan(0.5 * np.radians(fov))
    return inv_u, u, int(np.round(256.0 * sigma * H / (2.0 * ty))), int(np.round(256.0 * range))


def make_key(t, ids):
    """u64 key plane of depths t (f32) and ids; id < 0: nothing drawn."""
    t = np.asarray(t, np.float32)
    ids = np.asarray(ids, np.int64)
    key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ids & 0xFFFFFFFF).astype(np.uint64)
    return np.where(ids < 0, np.uint64(0xFFFFFFFFFFFFFFFF), key)


def quantise(key, flag, inv_u):
    """q = min((u32)(t * inv_u), 2^24 - 1) on flagged pixels, SENT elsewhere (uint64 array)."""
    t = (np.asarray(key, np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (t * np.float32(inv_u)).astype(np.float32)
        big = ~(v < np.float32(QMAX))
        q = np.where(big, QMAX, np.where(big, 0, v).astype(np.int64)).astype(np.uint64)
    return np.where(np.asarray(flag, bool), q, np.uint64(SENT))


def window(q, rnum, rmax):
    """(R, clamped) per pixel: R = clamp(Rnum / q, 1, rmax), rmax where q = 0; meaningless on SENT pixels."""
    q = q.astype(np.int64)
    raw = np.where(q > 0, rnum // np.maximum(q, 1), rmax + 1)
    return np.clip(raw, 1, rmax), raw > rmax


def smooth_once(q, rnum, dq, rmax):
    """One Jacobi step; returns (q', taps visited, taps accepted, pixels clamped at rmax)."""
    H, W = q.shape
    surf = q != SENT
    qi = q.astype(np.int64)
    R, clamped = window(q, rnum, rmax)
    R = np.where(surf, R, -1)   # (weights of a non-surface centre are all zero)
    rm = int(R.max()) if surf.any() else 0
    # the sentinel and every out-of-frame cell: 2^32 - 1, further than dq (at most 2^24) from any depth (below 2^24)
    pad = np.full((H + 2 * rm, W + 2 * rm), SENT, np.int64)
    pad[rm:rm + H, rm:rm + W] = qi
    tent = [np.maximum(R + 1 - k, 0) for k in range(rm + 1)]   # tent[|d|]: zero outside the pixel's own window
    num = np.zeros((H, W), np.int64)
    den = np.zeros((H, W), np.int64)
    acc = np.zeros((H, W), np.int64)
    for dy in range(-rm, rm + 1):
        for dx in range(-rm, rm + 1):
            qj = pad[rm + dy:rm + dy + H, rm + dx:rm + dx + W]
            w = tent[abs(dy)] * tent[abs(dx)] * (np.abs(qj - qi) <= dq)
            num += w * qj
            den += w
            acc += w > 0
    out = q.copy()
    d = den[surf]
    out[surf] = ((num[surf] + (d >> 1)) // d).astype(np.uint64)
    visited = int(((2 * R[surf] + 1) ** 2).sum())
    return out, visited, int(acc[surf].sum()), int((clamped & surf).sum())


def smooth(q, iterations, rnum, dq, rmax):
    """All iterations; returns (q, stats dict, list of every iterate)."""
    steps = [q]
    st = dict(surface_pixels=int((q != SENT).sum()), iterations=iterations, taps_visited=0, taps_accepted=0, clamped_rmax=0)
    for it in range(iterations):
        q, v, a, c = smooth_once(q, rnum, dq, rmax)
        st["taps_visited"] += v
        st["taps_accepted"] += a
        if it == 0:
            st["clamped_rmax"] = c
        steps.append(q)
    return q, st, steps


def _side(qi, qm, qp):
    """+1: the neighbour at index + 1, -1: the one before, 0: none (the smaller |dq|, a tie to the + side)."""
    vm, vp = qm != SENT, qp != SENT
    dm, dp = np.abs(qm - qi), np.abs(qp - qi)
    plus = vp & (~vm | (dp <= dm))
    return np.where(plus, 1, np.where(vm, -1, 0))


def sides(q):
    """(sx, sy, ql, qr, qu, qd) int64 planes of the normal's neighbour choice."""
    H, W = q.shape
    qi = q.astype(np.int64)
    pad = np.full((H + 2, W + 2), SENT, np.int64)
    pad[1:-1, 1:-1] = qi
    ql, qr, qu, qd = pad[1:-1, :-2], pad[1:-1, 2:], pad[:-2, 1:-1], pad[2:, 1:-1]
    return _side(qi, ql, qr), _side(qi, qu, qd), ql, qr, qu, qd


def shade(q, base_rgb, flag, frame_rgb, radius, eye=(5.5, 2.5, 4.0), target=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=70.0,
          light=(2.0, 2.0, 2.0), light_rgb=(1.0, 1.0, 1.0), ambient=0.1, spec=0.35, shininess=40.0):
    """rgb uint8 (H, W, 3) -- frame_rgb with the flagged pixels lit -- rgb_tol (H, W) and the normals (H, W, 3) in (s, u, f) coordinates."""
    H, W = q.shape
    flag = np.asarray(flag, bool)
    E, f, s, u_, tx, ty = RM.camera(eye, target, up, fov, W, H)
    Xc, Yr = RM.pixel_rays(W, H, tx, ty)
    X, Y = np.broadcast_to(Xc[None, :], (H, W)), np.broadcast_to(Yr[:, None], (H, W))
    Xn = np.broadcast_to(np.append(Xc[1:], Xc[-1])[None, :], (H, W))   # X of the next column (unused on the last)
    Yn = np.broadcast_to(np.append(Yr[1:], Yr[-1])[:, None], (H, W))
    dX, dY = 2.0 * tx / W, -2.0 * ty / H
    uu = float(np.float32(float(np.float32(radius)) / 256.0))
    lv = np.asarray(light, np.float64) - E
    Lv = np.array([s @ lv, u_ @ lv, f @ lv])
    lrgb = np.asarray(light_rgb, np.float64)
    sx, sy, ql, qr, qu, qd = sides(q)
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
        # the highlight's error: through the normal, and through log2 / exp2 (exponent e2 = shininess log2 ndh, a few ulp of it times ln 2)
        e2 = np.where(ndh > 0, np.abs(shininess * np.log2(np.where(ndh > 0, ndh, 1.0))), 0.0)
        dhi = shininess * np.where(ndh > 0, ndh ** (shininess - 1.0), 0.0) * dn + hi * (4 * U * (e2 + 4))
    base = np.asarray(base_rgb, np.float64) / 255.0
    val = base * (ambient + ndl[..., None] * lrgb) + spec * hi[..., None] * lrgb
    lit = np.floor(255 * np.clip(val, 0, 1) + 0.5)
    err = 255.0 * float(lrgb.max()) * (dn + spec * dhi)
    rgb = np.where(flag[..., None], lit, np.asarray(frame_rgb, np.float64)).astype(np.uint8)
    rgb_tol = np.where(flag, 1 + np.floor(err), 0).astype(np.int64)
    return rgb, rgb_tol, n


def surface(key, flag, base_rgb, frame_rgb, radius, fov=70.0, iterations=3, sigma=1.5, range=2.0, rmax=12, spec=0.35, shininess=40.0,
            **camera):
    """The whole mode from a key plane: dict(q, stats, rgb, rgb_tol, normal, R) -- R the window half-width of the first iteration."""
    H, W = np.asarray(key).shape
    inv_u, _, rnum, dq = constants(radius, H, fov, sigma, range)
    q0 = quantise(key, flag, inv_u)
    q, st, _ = smooth(q0, iterations, rnum, dq, rmax)
    rgb, tol, n = shade(q, base_rgb, flag, frame_rgb, radius, fov=fov, spec=spec, shininess=shininess, **camera)
    return dict(q=q.astype(np.uint32), q0=q0.astype(np.uint32), stats=st, rgb=rgb, rgb_tol=tol, normal=n, R=window(q0, rnum, rmax)[0])
