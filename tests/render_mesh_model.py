"""Float64 restatement of the mesh image (include/sph_hip.h sph_render_mesh_begin), for the tests.

render(meshes, ...) takes the list FrameRenderer.from_meshes takes, with host arrays: (vertices, triangles, normals or None, rgb).  It
returns per pixel the winner (global triangle index, -1 background, -2 - edge a box line), its colour, an `ambiguous` flag, the colour
bound `rgb_tol` in 8-bit steps, and for the ambiguous pixels the set of ids the device may show (`candidates(p)`).

Error bounds (u = 2^-24; nothing here is fitted to the device's output):
  vertex   a vertex reaches the device's view frame as fl(R fl(x - E)): one rounding of x - E, the f32 camera (E and the rows of R, each
           relative u) and three roundings of the fma chain, each at most u (|x - E| + |E|) -- under delta = SLACK u (|x - E| + |E|) with
           the SLACK = 16 of section 15 (tests/render_model.py).
  edge     e = d . (p x q), evaluated as fma(X, m_x, fma(Y, m_y, m_z)), m = fl(p x q) by one product and one fma per component.  Moving p by
           delta changes e by at most delta |q x d| (and q: delta |p x d|); m_x carries u (|p_y q_z| + |p_z q_y|) and likewise m_y, m_z;
           X and Y carry 4 u relative; the two fma of the dot product 2 u (|X m_x| + |Y m_y| + |m_z|).  tol_e is the sum.  A pixel centre
           is surely inside when all three edge functions clear their tol_e with one sign, possibly inside when none contradicts by more.
  depth    t = (a . N) / (d . N), N = e1 x e2 of the edge vectors.  dN = 2 delta (|e1| + |e2|) + 4 u |e1| |e2| bounds the error of N
           (both edge vectors move by up to 2 delta; two roundings per component).  A hit point lies within the longest edge L of the
           vertex a the device measures from, so the plane's tilt moves it by L dN / |d . N|, the vertex error by delta |N| / |d . N|, the
           roundings of a . N and d . N by 3 u (|a| + t |d|) |N| / |d . N|, the division by u t:
           tol_t = (delta |N| + L dN + 3 u (|a| + t |d|) |N|) / |d . N| + 2 u t.  A triangle seen so edge-on that |d . N| is within
           |d| dN + 3 u |d| |N| of zero is never `sure`.
  colour   one 8-bit step for the rounding plus 255 times the normal's error: dN / |N| for a flat normal, the edge tolerances over
           |d . N| for a blend (its weights are the edge functions, which sum to d . N), plus the light direction's tol_t |d| / |L|.  Where
           the normal is within that error of perpendicular to the ray, the two-sided flip may go either way: the bound is 255 there.
A pixel is ambiguous unless exactly one id can win it and that one is sure: the candidates are the possible hits whose t - tol_t does not
exceed the smallest t + tol_t of the sure ones, plus the background when no hit is sure; box lines take part with the depth bound and
the minor-axis flag of tests/render_model.py (the neighbouring pixel is then a candidate too)."""
from __future__ import annotations

import numpy as np

from tests import render_model as RM

U = RM.U
SLACK = RM.SLACK


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _norm(a):
    return np.sqrt((a * a).sum(axis=-1))


def _edge(p, q, dp, dq, D, X, Y):
    """e = d . (p x q) and its bound for pairs (rows of p, q: view coordinates; D = (X, Y, 1))."""
    m = _cross(p, q)
    e = X * m[:, 0] + Y * m[:, 1] + m[:, 2]
    mag = np.stack([np.abs(p[:, 1] * q[:, 2]) + np.abs(p[:, 2] * q[:, 1]), np.abs(p[:, 2] * q[:, 0]) + np.abs(p[:, 0] * q[:, 2]),
                    np.abs(p[:, 0] * q[:, 1]) + np.abs(p[:, 1] * q[:, 0])], axis=1)
    tol = dp * _norm(_cross(q, D)) + dq * _norm(_cross(p, D))
    tol = tol + U * (np.abs(X) * mag[:, 0] + np.abs(Y) * mag[:, 1] + mag[:, 2])
    tol = tol + 6 * U * (np.abs(X * m[:, 0]) + np.abs(Y * m[:, 1]) + np.abs(m[:, 2]))
    return e, tol


class Result(dict):
    def candidates(self, j, i):
        """ids the device may show at pixel (row j, column i)."""
        p = j * self["W"] + i
        lo, hi = np.searchsorted(self["_cpix"], [p, p + 1])
        out = set(int(v) for v in self["_cid"][lo:hi])
        if self["_bg"][p]:
            out.add(-1)
        return out


def render(meshes, W=1024, H=1024, eye=(5.5, 2.5, 4.0), target=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=70.0, zn=0.1,
           light=(2.0, 2.0, 2.0), light_rgb=(1.0, 1.0, 1.0), ambient=0.1, background=(0, 0, 0), box=None, box_rgb=RM.BOX_RGB,
           pair_budget=1 << 21):
    E, f, s, u, tx, ty = RM.camera(eye, target, up, fov, W, H)
    R = np.stack([s, u, f])
    Xc, Yr = RM.pixel_rays(W, H, tx, ty)
    zn = float(np.float32(zn))
    # the list, concatenated; triangles with a bad index, a non-finite vertex or N = 0 are skipped and counted
    V, NV, T, TM = [], [], [], []
    cols, smooth = [], []
    v0 = 0
    skipped = dict(bad_index=0, skipped_nonfinite=0, skipped_degenerate=0)
    for k, (v, t, n, rgb) in enumerate(meshes):
        v = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 3)
        t = np.asarray(t, np.int64).reshape(-1, 3)
        V.append(v)
        NV.append(np.zeros_like(v) if n is None else np.asarray(n, np.float32).astype(np.float64).reshape(-1, 3))
        ok = ((t >= 0) & (t < len(v))).all(axis=1)
        skipped["bad_index"] += int((~ok).sum())
        T.append(np.where(ok[:, None], t + v0, -1))
        TM.append(np.full(len(t), k))
        cols.append(np.asarray(rgb, np.float64).reshape(3))
        smooth.append(n is not None)
        v0 += len(v)
    V = np.concatenate(V) if V else np.zeros((0, 3))
    NV = np.concatenate(NV) if NV else np.zeros((0, 3))
    T = np.concatenate(T) if T else np.zeros((0, 3), np.int64)
    TM = np.concatenate(TM) if TM else np.zeros(0, np.int64)
    cols = np.array(cols).reshape(-1, 3)
    smooth = np.array(smooth, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        PV = (V - E) @ R.T                                     # view coordinates (s, u, f)
        dV = SLACK * U * (_norm(V - E) + np.linalg.norm(E))
    valid = T[:, 0] >= 0
    Ti = np.where(T < 0, 0, T)
    fin = np.isfinite(V).all(axis=1)[Ti].all(axis=1) if len(V) else np.zeros(len(T), bool)
    skipped["skipped_nonfinite"] += int((valid & ~fin).sum())
    valid &= fin
    A, B, Cc = (np.where(valid[:, None], PV[Ti[:, k]], 0.0) for k in range(3)) if len(V) else (np.zeros((len(T), 3)),) * 3
    e1, e2 = B - A, Cc - A
    N = _cross(e1, e2)
    # the device's N is an f32 cross product of f32 differences: zero exactly when the f32 vertices are collinear enough for that; the
    # cases keep to triangles that are degenerate exactly (two equal vertices) or not at all
    deg = valid & (_norm(N) == 0)
    skipped["skipped_degenerate"] += int(deg.sum())
    valid &= ~deg
    dA, dB, dC = (dV[Ti[:, k]] if len(V) else np.zeros(len(T)) for k in range(3))
    dmax = np.maximum(dA, np.maximum(dB, dC))
    l1, l2 = _norm(e1), _norm(e2)
    Lmax = np.maximum(np.maximum(l1, l2), _norm(Cc - B))
    dN = 2 * dmax * (l1 + l2) + 4 * U * l1 * l2
    Nn = _norm(N)
    amax = np.maximum(_norm(A), np.maximum(_norm(B), _norm(Cc)))
    # bounds in pixels
    Z = np.stack([A[:, 2], B[:, 2], Cc[:, 2]], axis=1)
    valid &= Z.max(axis=1) + dmax > zn
    full = Z.min(axis=1) <= 2 * zn
    with np.errstate(invalid="ignore", divide="ignore"):
        col = np.stack([(P[:, 0] / P[:, 2] / tx + 1) * 0.5 * W - 0.5 for P in (A, B, Cc)], axis=1)
        row = np.stack([(1 - P[:, 1] / P[:, 2] / ty) * 0.5 * H - 0.5 for P in (A, B, Cc)], axis=1)
    lim = 4.0 * max(W, H)
    c0 = np.where(full, -1, np.clip(np.nan_to_num(col.min(axis=1)), -lim, lim)); c1 = np.where(full, W, np.clip(np.nan_to_num(col.max(axis=1)), -lim, lim))
    r0 = np.where(full, -1, np.clip(np.nan_to_num(row.min(axis=1)), -lim, lim)); r1 = np.where(full, H, np.clip(np.nan_to_num(row.max(axis=1)), -lim, lim))
    i0 = np.maximum(np.floor(c0).astype(np.int64) - 2, 0); i1 = np.minimum(np.ceil(c1).astype(np.int64) + 2, W - 1)
    j0 = np.maximum(np.floor(r0).astype(np.int64) - 2, 0); j1 = np.minimum(np.ceil(r1).astype(np.int64) + 2, H - 1)
    valid &= (i0 <= i1) & (j0 <= j1)
    idx = np.flatnonzero(valid)
    bw = (i1 - i0 + 1)[idx]
    area = bw * (j1 - j0 + 1)[idx]
    cum = np.cumsum(area)
    out = dict(pix=[], tid=[], t=[], tol=[], sure=[], hit=[], ntol=[], flip=[])
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
        D = np.stack([X, Y, np.ones(len(X))], axis=1)
        eA, tA = _edge(B[P], Cc[P], dB[P], dC[P], D, X, Y)
        eB, tB = _edge(Cc[P], A[P], dC[P], dA[P], D, X, Y)
        eC, tC = _edge(A[P], B[P], dA[P], dB[P], D, X, Y)
        poss = ((eA >= -tA) & (eB >= -tB) & (eC >= -tC)) | ((eA <= tA) & (eB <= tB) & (eC <= tC))
        m = np.flatnonzero(poss)
        if len(m) == 0:
            start = stop
            continue
        P, ii, jj, X, Y, D = P[m], ii[m], jj[m], X[m], Y[m], D[m]
        eA, eB, eC, tA, tB, tC = eA[m], eB[m], eC[m], tA[m], tB[m], tC[m]
        inside = ((eA > tA) & (eB > tB) & (eC > tC)) | ((eA < -tA) & (eB < -tB) & (eC < -tC))
        exact = ((eA >= 0) & (eB >= 0) & (eC >= 0)) | ((eA <= 0) & (eB <= 0) & (eC <= 0))
        dn = (D * N[P]).sum(axis=1)
        dl = _norm(D)
        den_tol = dl * dN[P] + 3 * U * dl * Nn[P]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (A[P] * N[P]).sum(axis=1) / dn
            tol = (dmax[P] * Nn[P] + Lmax[P] * dN[P] + 3 * U * (amax[P] + np.abs(t) * dl) * Nn[P]) / np.abs(dn) + 2 * U * np.abs(t)
        edge_on = ~(np.abs(dn) > 2 * den_tol) | ~np.isfinite(t)
        t = np.where(edge_on, 0.0, t)
        tol = np.where(edge_on, np.inf, tol)
        keep = edge_on | (t + tol > zn)
        sure = inside & ~edge_on & (t - tol > zn)
        hit = exact & ~edge_on & (t > zn)
        # the normal and its bound
        nf = N[P] / Nn[P][:, None]
        ntol = dN[P] / Nn[P]
        sm = smooth[TM[P]]
        if sm.any():
            blend = eA[:, None] * NV[Ti[P, 0]] + eB[:, None] * NV[Ti[P, 1]] + eC[:, None] * NV[Ti[P, 2]]
            blend = blend @ R.T
            bl = _norm(blend)
            good = sm & np.isfinite(bl) & (bl > 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                nb = blend / bl[:, None]
                wn = np.maximum(_norm(NV[Ti[P, 0]]), np.maximum(_norm(NV[Ti[P, 1]]), _norm(NV[Ti[P, 2]])))
                btol = 2 * (tA + tB + tC + 8 * U * (np.abs(eA) + np.abs(eB) + np.abs(eC))) * wn / bl + 8 * U
            nf = np.where(good[:, None], nb, nf)
            ntol = np.where(good, btol, ntol)
        nd = (nf * D).sum(axis=1)
        flip_unsure = np.abs(nd) <= 2 * ntol * dl
        nf = np.where((nd > 0)[:, None], -nf, nf)
        kk = np.flatnonzero(keep)
        out["pix"].append((jj * W + ii)[kk]); out["tid"].append(P[kk]); out["t"].append(t[kk]); out["tol"].append(tol[kk])
        out["sure"].append(sure[kk]); out["hit"].append(hit[kk]); out["ntol"].append(ntol[kk]); out["flip"].append(flip_unsure[kk])
        out.setdefault("n", []).append(nf[kk])
        start = stop
    cat = lambda key, dt: np.concatenate(out[key]) if out[key] else np.zeros(0, dt)
    pix, tid, t, tol = cat("pix", np.int64), cat("tid", np.int64), cat("t", np.float64), cat("tol", np.float64)
    sure, hit, ntol, flip = cat("sure", bool), cat("hit", bool), cat("ntol", np.float64), cat("flip", bool)
    nrm = np.concatenate(out["n"]) if out.get("n") else np.zeros((0, 3))
    npx = W * H
    amb_line = np.zeros(npx, bool)
    l_pix, l_id, l_t, l_tol, l_sure, l_hit = [], [], [], [], [], []
    if box is not None:
        Abox = RM.box_anchors(np.asarray(box[0], np.float64), np.asarray(box[1], np.float64))
        for e, (a0, a1) in enumerate(RM.EDGES):
            st = RM.line_steps(Abox[a0], Abox[a1], E, f, s, u, tx, ty, W, H, zn)
            if st is None:
                continue
            ax, li, lj, lt, lamb, keep = st
            inb = (li >= 0) & (li < W) & (lj >= 0) & (lj < H)
            for dm in (0, -1, 1):
                ni, nj = (li, lj + dm) if ax == 0 else (li + dm, lj)
                m = inb & (ni >= 0) & (ni < W) & (nj >= 0) & (nj < H) & (lamb if dm else np.ones(len(li), bool))
                l_pix.append((nj * W + ni)[m]); l_id.append(np.full(m.sum(), -2 - e, np.int64)); l_t.append(lt[m]); l_tol.append(64 * U * lt[m])
                l_sure.append((keep & ~lamb)[m] if dm == 0 else np.zeros(m.sum(), bool))
                l_hit.append(keep[m] if dm == 0 else np.zeros(m.sum(), bool))
    if l_pix:
        pix = np.concatenate([pix] + l_pix); tid = np.concatenate([tid] + l_id); t = np.concatenate([t] + l_t)
        tol = np.concatenate([tol] + l_tol); sure = np.concatenate([sure] + l_sure); hit = np.concatenate([hit] + l_hit)
        nl = len(pix) - len(ntol)
        ntol = np.concatenate([ntol, np.zeros(nl)]); flip = np.concatenate([flip, np.zeros(nl, bool)]); nrm = np.concatenate([nrm, np.zeros((nl, 3))])
    # candidates: possible hits not surely behind the nearest sure one
    t_up = np.full(npx, np.inf)
    np.minimum.at(t_up, pix[sure], (t + tol)[sure])
    cand = (t - tol) <= t_up[pix]
    ncand = np.bincount(pix[cand], minlength=npx)
    nsure = np.bincount(pix[cand & sure], minlength=npx)
    bg_cand = ~np.isfinite(t_up)
    ambiguous = ((ncand > 0) & bg_cand) | (ncand > 1) | ((ncand == 1) & (nsure == 0))
    # the model's own winner: the smallest (t, id) of the exact hits
    ids = np.full(npx, -1, np.int64)
    rgb = np.empty((npx, 3), np.float64)
    rgb[:] = np.asarray(background, np.float64)
    rgb_tol = np.ones(npx, np.int64)
    depth = np.full(npx, np.inf)
    h = np.flatnonzero(hit)
    if len(h):
        key_id = np.where(tid[h] < 0, RM.LINE_ID0 + (-2 - tid[h]), tid[h])
        o = np.lexsort((key_id, t[h], pix[h]))
        hs = h[o]
        first = np.ones(len(hs), bool)
        first[1:] = pix[hs][1:] != pix[hs][:-1]
        w = hs[first]
        ids[pix[w]] = tid[w]
        depth[pix[w]] = t[w]
        lw = w[tid[w] < 0]
        rgb[pix[lw]] = np.asarray(box_rgb, np.float64)
        tw = w[tid[w] >= 0]
        if len(tw):
            p = pix[tw]
            jj, ii = p // W, p % W
            D = np.stack([Xc[ii], Yr[jj], np.ones(len(p))], axis=1)
            Pv = t[tw][:, None] * D
            Lv = R @ (np.asarray(light, np.float64) - E) - Pv
            ll = _norm(Lv)
            ndl = np.maximum((nrm[tw] * Lv).sum(axis=1) / ll, 0.0)
            val = cols[TM[tid[tw]]] / 255.0 * (ambient + ndl[:, None] * np.asarray(light_rgb, np.float64))
            rgb[p] = np.floor(255 * np.clip(val, 0, 1) + 0.5)
            err = ntol[tw] + 8 * U + np.where(np.isfinite(tol[tw]), tol[tw], 0.0) * _norm(D) / ll
            rgb_tol[p] = np.where(flip[tw], 255, 1 + np.floor(255 * err * max(1.0, float(np.max(light_rgb)))))
    o = np.argsort(pix[cand], kind="stable")
    res = Result(ids=ids.reshape(H, W), rgb=rgb.reshape(H, W, 3).astype(np.uint8), ambiguous=ambiguous.reshape(H, W),
                 rgb_tol=rgb_tol.reshape(H, W), depth=depth.reshape(H, W), covered=int((ids >= 0).sum()), W=W, H=H,
                 _cpix=pix[cand][o], _cid=tid[cand][o], _bg=bg_cand, triangles=len(T), **skipped)
    return res
