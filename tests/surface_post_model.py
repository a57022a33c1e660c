"""Numpy restatement of the surface post-processing: the vertex adjacency, the smoothing weights in float64, and the
Laplacian and normal smoothing in float32 with the library's order of operations (so the strict build must match it bit for bit).
Used by tests/test_surface_post_host.py (CPU) and tests/test_hip_surface_post.py."""
from __future__ import annotations

import numpy as np

F1 = np.float32(1.0)


def adjacency(n_vertices, triangles):
    """(offsets i64[nv + 1], neighbours i64[E]): per vertex the vertices j != i that share a triangle with it, ascending, unique."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    a = np.concatenate([t[:, 0], t[:, 0], t[:, 1], t[:, 1], t[:, 2], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 2], t[:, 0], t[:, 0], t[:, 1]])
    keep = a != b
    key = np.unique(a[keep] * max(n_vertices, 1) + b[keep])
    src, dst = key // max(n_vertices, 1), key % max(n_vertices, 1)
    off = np.zeros(n_vertices + 1, dtype=np.int64)
    np.add.at(off, src + 1, 1)
    return np.cumsum(off), dst


def particle_counts(x, h):
    """c_j = sum over k != j with |x_j - x_k| < h of (1 - |x_j - x_k|^2 / h^2), float64; also the longest such sum."""
    from scipy.spatial import cKDTree
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    tree = cKDTree(x)
    c = np.zeros(len(x))
    n_max = 0
    for j, nb in enumerate(tree.query_ball_point(x, h)):
        nb = np.array([k for k in nb if k != j], dtype=np.int64)
        if len(nb):
            d2 = ((x[nb] - x[j]) ** 2).sum(axis=1)
            d2 = d2[d2 < h * h]
            c[j] = (1.0 - d2 / (h * h)).sum()
            n_max = max(n_max, len(d2))
    return c, n_max


def vertex_max_counts(vertices, x, c, radius):
    """max c_j over the particles with |v - x_j| < radius (0 when there are none), float64."""
    from scipy.spatial import cKDTree
    tree = cKDTree(np.asarray(x, dtype=np.float64).reshape(-1, 3))
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(v))
    for i, nb in enumerate(tree.query_ball_point(v, radius)):
        if nb:
            nb = np.array(nb, dtype=np.int64)
            d2 = ((tree.data[nb] - v[i]) ** 2).sum(axis=1)
            sel = nb[d2 < radius * radius]
            out[i] = c[sel].max() if len(sel) else 0.0
    return out


def weights(vertices, x, h, normalization=13.0, radius=None):
    """w_i = min(1, N_i / normalization), N_i = max c_j over the particles within h of vertex i (within `radius` if given), float64."""
    c, _ = particle_counts(x, h)
    return np.minimum(1.0, vertex_max_counts(vertices, x, c, h if radius is None else radius) / normalization)


def _neighbour_sum(a, off, nb, s):
    """s += a[j] for the neighbours j of every vertex, in ascending order, in float32 (one add per neighbour, as the device adds)."""
    deg = np.diff(off)
    start = off[:-1]
    for k in range(int(deg.max()) if len(deg) else 0):
        m = deg > k
        s[m] += a[nb[start[m] + k]]
    return s


def smooth(vertices, off, nb, w=None, iters=25):
    """iters Jacobi iterations P' = (1 - w) P + w m, m = (sum_{j ascending} P_j) / |N(i)| (IEEE divide), float32; a vertex without
    neighbours stays.  w None: 1."""
    P = np.array(vertices, dtype=np.float32).reshape(-1, 3)
    off = np.asarray(off, dtype=np.int64)
    nb = np.asarray(nb, dtype=np.int64)
    deg = np.diff(off)
    has = deg > 0
    degf = np.where(has, deg, 1).astype(np.float32)[:, None]
    w = np.ones(len(P), np.float32) if w is None else np.asarray(w, dtype=np.float32)
    wi, wo = w[:, None], (F1 - w)[:, None]
    for _ in range(iters):
        s = _neighbour_sum(P, off, nb, np.zeros_like(P))
        m = s / degf
        P = np.where(has[:, None], wo * P + wi * m, P)
    return P


def smooth_normals(normals, off, nb, iters=10):
    """iters iterations n' = s / sqrt(s.s), s = n_i + sum_{j ascending} n_j, float32; s.s = 0: s stays."""
    n = np.array(normals, dtype=np.float32).reshape(-1, 3)
    off = np.asarray(off, dtype=np.int64)
    nb = np.asarray(nb, dtype=np.int64)
    for _ in range(iters):
        s = _neighbour_sum(n, off, nb, n.copy())
        ln = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        pos = ln > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.where(pos[:, None], s / np.where(pos, ln, F1)[:, None], s)
    return n
