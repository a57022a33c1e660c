"""Float64 restatement of the particle image (include/sph_hip.h sph_render_create), for the tests.

render() returns the winner ids, the rgb, and per pixel an `ambiguous` flag: f32 rounding may change the winner there.  A pixel is
ambiguous when a sphere that could win passes within `tol_len` of its silhouette (|w| ~ r, disc ~ 0) or of the near plane, when its two
best depths are closer than their error bounds, or when a box line's minor-axis coordinate lies that close to a pixel edge.  The bounds
come from the f32 evaluation on the device: every length there carries a few roundings of |c - E| + |E| (view transform, ray, the
projection w of c - E across the ray), bounded by SLACK * 2^-24 (|c - E| + |E| + r).  `rgb_tol` bounds, in 8-bit steps, how far the
device's colour may be from the model's: one step of rounding plus 255 times the normal's error (which grows like tol / sqrt(disc) near
the silhouette).
Vectorised and chunked by (particle, pixel) pairs, so C2 at 1024^2 stays within memory."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
SLACK = 16
LINE_ID0 = 0xFFFFFFF0
BOX_RGB = (252, 173, 71)
# box_lines_indices of the reference's run_simulation.py; anchor a has x from bit 1, y from bit 0, z from bit 2
EDGES = [(0, 1), (0, 2), (1, 3), (2, 3), (4, 5), (4, 6), (5, 7), (6, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
REFERENCE_CAMERA = dict(eye=(5.5, 2.5, 4.0), target=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=70.0)


def camera(eye, target, up, fov, W, H):
    E = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - E
    f /= np.linalg.norm(f)
    s = np.cross(f, np.asarray(up, np.float64))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    ty = np.tan(0.5 * np.radians(fov))
    return E, f, s, u, ty * W / H, ty


def pixel_rays(W, H, tx, ty):
    """X (per column) and Y (per row) of d = f + X s + Y u."""
    return (2 * (np.arange(W) + 0.5) / W - 1) * tx, (1 - 2 * (np.arange(H) + 0.5) / H) * ty


def box_anchors(lo, hi):
    return np.array([[hi[0] if a & 2 else lo[0], hi[1] if a & 1 else lo[1], hi[2] if a & 4 else lo[2]] for a in range(8)], np.float64)


def line_steps(A, B, E, f, s, u, tx, ty, W, H, zn):
    """Pixels (i, j), depths t and an ambiguity flag of one box edge: clipped at zn, one step per pixel of the screen major axis,
    nearest pixel on the minor one, 1/z linear on the screen.  The clipped, projected end points are rounded to f32 as the device
    receives them."""
    P = np.array([A - E, B - E], np.float64)
    z = P @ f
    if z[0] <= zn and z[1] <= zn:
        return None
    for q in (0, 1):
        if z[q] < zn:
            w = (zn - z[q]) / (z[1 - q] - z[q])
            P[q] = P[q] + w * (P[1 - q] - P[q])
            z[q] = zn
    px = (P @ s / z / tx + 1) * 0.5 * W
    py = (1 - P @ u / z / ty) * 0.5 * H
    ax = 0 if abs(px[1] - px[0]) >= abs(py[1] - py[0]) else 1
    ma, mi = (px, py) if ax == 0 else (py, px)
    nmaj = W if ax == 0 else H
    if not abs(ma[1] - ma[0]) > 1e-9:
        return None
    k0 = max(np.ceil(min(ma) - 0.5), 0.0)
    k1 = min(np.floor(max(ma) - 0.5), nmaj - 1.0)
    if k0 > k1:
        return None
    g = np.array([ma[0], mi[0], ma[1], mi[1], 1 / z[0], 1 / z[1]], np.float32).astype(np.float64)
    k = np.arange(int(k0), int(k1) + 1, dtype=np.float64)
    sp = (k + 0.5 - g[0]) / (g[2] - g[0])
    m = g[1] + sp * (g[3] - g[1])
    t = 1.0 / (g[4] + sp * (g[5] - g[4]))
    tol = 1e-3 + 16 * U * np.abs(g[:4]).max()
    frac = m - np.floor(m)
    amb = (frac < tol) | (frac > 1 - tol)
    mj = np.floor(m).astype(np.int64)
    kk = k.astype(np.int64)
    i, j = (kk, mj) if ax == 0 else (mj, kk)
    keep = (i >= 0) & (i < W) & (j >= 0) & (j < H) & (t > zn)
    amb_t = np.abs(t - zn) < 64 * U * t
    m = keep | amb_t
    return ax, i[m], j[m], t[m], amb[m] | amb_t[m], keep[m]


class _Best:
    """Per pixel: the best (t, particle index or line id, tolerance) and the second (t, tolerance); min t of near-silhouette passes."""

    def __init__(self, npx):
        self.t = np.full((npx, 2), np.inf)
        self.tol = np.zeros((npx, 2))
        self.who = np.full(npx, -1, np.int64)
        self.sil = np.full(npx, np.inf)
        self.amb = np.zeros(npx, bool)

    def add(self, p, t, tol, who):
        if len(p) == 0:
            return
        o = np.lexsort((t, p))
        p, t, tol, who = p[o], t[o], tol[o], who[o]
        first = np.ones(len(p), bool)
        first[1:] = p[1:] != p[:-1]
        f_idx = np.flatnonzero(first)
        sec = f_idx + 1
        has2 = sec < len(p)
        has2[has2] = ~first[sec[has2]]
        up = p[f_idx]
        c_t = np.stack([self.t[up, 0], self.t[up, 1], t[f_idx], np.where(has2, t[np.minimum(sec, len(p) - 1)], np.inf)], axis=1)
        c_tol = np.stack([self.tol[up, 0], self.tol[up, 1], tol[f_idx], np.where(has2, tol[np.minimum(sec, len(p) - 1)], 0.0)], axis=1)
        c_who = np.stack([self.who[up], np.full(len(up), -1), who[f_idx], np.full(len(up), -1)], axis=1)
        ordr = np.argsort(c_t, axis=1, kind="stable")[:, :2]
        r = np.arange(len(up))[:, None]
        self.t[up] = c_t[r, ordr]
        self.tol[up] = c_tol[r, ordr]
        self.who[up] = c_who[np.arange(len(up)), ordr[:, 0]]


def render(xyz, radius, colors=None, ids=None, W=1024, H=1024, eye=(5.5, 2.5, 4.0), target=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0),
           fov=70.0, zn=0.1, light=(2.0, 2.0, 2.0), light_rgb=(1.0, 1.0, 1.0), ambient=0.1, background=(0, 0, 0), box=None,
           box_rgb=BOX_RGB, pair_budget=1 << 21):
    x = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(x)
    col = np.full((n, 3), 255, np.int64) if colors is None else np.asarray(colors).astype(np.int64).reshape(-1, 3)
    pid = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids).astype(np.int64).reshape(-1)
    r = float(np.float32(radius))
    E, f, s, u, tx, ty = camera(eye, target, up, fov, W, H)
    Xc, Yr = pixel_rays(W, H, tx, ty)
    best = _Best(W * H)
    finite = np.isfinite(x).all(axis=1)
    v = x - E
    xs, ys, z = v @ s, v @ u, v @ f
    # conservative bounds: two pixels of margin (the device takes one beyond its own f32 tangents)
    full = z - r <= zn
    ok = finite & (z + r > zn)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = z * z - r * r
        qx, qy = r * np.sqrt(np.maximum(xs * xs + den, 0)), r * np.sqrt(np.maximum(ys * ys + den, 0))
        xl, xh = (xs * z - qx) / den, (xs * z + qx) / den
        yl, yh = (ys * z - qy) / den, (ys * z + qy) / den
        lim = 4.0 * max(W, H)
        c0 = np.clip((xl / tx + 1) * 0.5 * W - 0.5, -lim, lim)
        c1 = np.clip((xh / tx + 1) * 0.5 * W - 0.5, -lim, lim)
        r0 = np.clip((1 - yh / ty) * 0.5 * H - 0.5, -lim, lim)
        r1 = np.clip((1 - yl / ty) * 0.5 * H - 0.5, -lim, lim)
    c0 = np.where(full, -1, c0); c1 = np.where(full, W, c1); r0 = np.where(full, -1, r0); r1 = np.where(full, H, r1)
    c0, c1, r0, r1 = [np.nan_to_num(a, nan=0.0) for a in (c0, c1, r0, r1)]
    i0 = np.maximum(np.floor(c0).astype(np.int64) - 2, 0); i1 = np.minimum(np.ceil(c1).astype(np.int64) + 2, W - 1)
    j0 = np.maximum(np.floor(r0).astype(np.int64) - 2, 0); j1 = np.minimum(np.ceil(r1).astype(np.int64) + 2, H - 1)
    ok &= (i0 <= i1) & (j0 <= j1)
    idx = np.flatnonzero(ok)
    bw = (i1 - i0 + 1)[idx]
    area = bw * (j1 - j0 + 1)[idx]
    tol_len = SLACK * U * (np.linalg.norm(v, axis=1) + np.linalg.norm(E) + r)
    cum = np.cumsum(area)
    start = 0
    while start < len(idx):
        stop = max(start + 1, int(np.searchsorted(cum, (cum[start - 1] if start else 0) + pair_budget, side="right")))
        sel = idx[start:stop]
        a = area[start:stop]
        k = np.repeat(np.arange(len(sel)), a)
        q = np.arange(a.sum()) - np.repeat(np.cumsum(a) - a, a)
        P = sel[k]
        ii = i0[P] + q % bw[start:stop][k]
        jj = j0[P] + q // bw[start:stop][k]
        X, Y = Xc[ii], Yr[jj]
        dd = X * X + Y * Y + 1
        kk = (X * xs[P] + Y * ys[P] + z[P]) / dd
        wx, wy, wz = xs[P] - kk * X, ys[P] - kk * Y, z[P] - kk
        w2 = wx * wx + wy * wy + wz * wz
        h = r * r - w2
        t = kk - np.sqrt(np.maximum(h, 0) / dd)
        tl = tol_len[P]
        hit = (h >= 0) & (t > zn)
        near = (np.abs(np.sqrt(w2) - r) < tl) | ((h >= 0) & (np.abs(t - zn) < tl))
        # depth error: the f32 lengths plus the square root's amplification of the error of h ~ 2 r tl near the silhouette
        tol_t = tl + 2 * r * tl / np.sqrt(np.maximum(h, 2 * r * tl) * dd)
        pix = jj * W + ii
        best.add(pix[hit], t[hit], tol_t[hit], P[hit])
        np.minimum.at(best.sil, pix[near], kk[near] - tl[near])
        start = stop
    if box is not None:
        A = box_anchors(np.asarray(box[0], np.float64), np.asarray(box[1], np.float64))
        for e, (a0, a1) in enumerate(EDGES):
            st = line_steps(A[a0], A[a1], E, f, s, u, tx, ty, W, H, zn)
            if st is None:
                continue
            ax, li, lj, lt, lamb, keep = st
            inb = (li >= 0) & (li < W) & (lj >= 0) & (lj < H)
            lp = lj * W + li
            best.amb[lp[lamb & inb]] = True
            # the neighbouring minor pixel may be the one drawn instead
            for dm in (-1, 1):
                ni, nj = (li, lj + dm) if ax == 0 else (li + dm, lj)
                m = lamb & (ni >= 0) & (ni < W) & (nj >= 0) & (nj < H)
                best.amb[(nj * W + ni)[m]] = True
            m = keep & inb
            best.add(lp[m], lt[m], 64 * U * lt[m], np.full(m.sum(), -2 - e, np.int64))
    bt, b2 = best.t[:, 0], best.t[:, 1]
    with np.errstate(invalid="ignore"):
        ambiguous = best.amb | (b2 - bt <= best.tol[:, 0] + best.tol[:, 1]) | (np.isfinite(best.sil) & (best.sil <= bt + best.tol[:, 0]))
    who = best.who
    out_ids = np.full(W * H, -1, np.int64)
    sph = who >= 0
    out_ids[sph] = pid[who[sph]]
    out_ids[who <= -2] = who[who <= -2]
    rgb = np.empty((W * H, 3), np.float64)
    rgb[:] = np.asarray(background, np.float64)
    rgb[who <= -2] = np.asarray(box_rgb, np.float64)
    rgb_tol = np.ones(W * H, np.int64)
    p = np.flatnonzero(sph)
    if len(p):
        c = who[p]
        jj, ii = p // W, p % W
        d = np.stack([Xc[ii], Yr[jj], np.ones(len(p))], axis=1) @ np.stack([s, u, f])   # world-frame ray
        t = bt[p]
        P = E + t[:, None] * d
        nrm = (P - x[c]) / r
        L = np.asarray(light, np.float64) - P
        L /= np.linalg.norm(L, axis=1, keepdims=True)
        ndl = np.maximum((nrm * L).sum(axis=1), 0.0)
        val = col[c] / 255.0 * (ambient + ndl[:, None] * np.asarray(light_rgb, np.float64))
        rgb[p] = np.floor(255 * np.clip(val, 0, 1) + 0.5)
        # error of the colour: 255 |dn| with |dn| <= (|dt| |d| + tl) / r, plus the rounding of the exact value near a half step
        dn = (best.tol[p, 0] * np.linalg.norm(d, axis=1) + tol_len[c]) / r
        rgb_tol[p] = 1 + np.floor(255 * dn * max(1.0, float(np.max(light_rgb))))   # 8-bit steps: the rounding plus the colour's error
    return dict(ids=out_ids.reshape(H, W).astype(np.int64), rgb=rgb.reshape(H, W, 3).astype(np.uint8),
                ambiguous=ambiguous.reshape(H, W), rgb_tol=rgb_tol.reshape(H, W), covered=int(sph.sum()))
