"""Float64 numpy restatement of the surface reconstruction with anisotropic kernels: brute force over particles.  The
grid, bricks, case table and emit order are those of tests/surface_model.py (its reconstruct() runs here with this module's field).
Used by tests/test_surface_aniso_host.py (CPU) and tests/test_hip_surface_aniso.py.

    python tests/surface_aniso_model.py      prints the table of DESIGN.md 29 (surface offsets of thin shapes, in particle radii)

`mutant` (a name of MUTANTS) breaks the method in one place; the host tests show that each one is caught."""
from __future__ import annotations

import numpy as np

from tests import surface_model as SM

DEFAULTS = dict(max_ratio=2.0, min_neighbours=25, sparse_scale=0.5)
MUTANTS = ("cov_about_xi", "no_det", "grad_A", "clamp_l3_only", "count_le", "iso_V")
SWEEPS = 12   # cyclic Jacobi in float64: converged to the last bit well before


def eig_sym3(C):
    """(lambda[n,3], v[n,3,3] with the eigenvectors in the columns) of symmetric C[n,3,3]: cyclic Jacobi, SWEEPS sweeps over (0,1), (0,2),
    (1,2), the rotation of the library's routine (csrc/sph_surface_aniso_eig.hpp).  Unordered."""
    a = np.array(C, dtype=np.float64).reshape(-1, 3, 3).copy()
    v = np.broadcast_to(np.eye(3), a.shape).copy()
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[:, p, q]
            on = apq != 0.0
            safe = np.where(on, apq, 1.0)
            with np.errstate(over="ignore"):
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * safe)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            t = np.where(on, t, 0.0)
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            J = np.broadcast_to(np.eye(3), a.shape).copy()
            J[:, p, p] = c
            J[:, q, q] = c
            J[:, p, q] = s
            J[:, q, p] = -s
            a = np.einsum("nji,njk,nkl->nil", J, a, J)
            a[:, p, q] = np.where(on, 0.0, a[:, p, q])
            a[:, q, p] = a[:, p, q]
            v = np.einsum("nij,njk->nik", v, J)
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), v


def kernel_matrix(C, N, max_ratio=2.0, min_neighbours=25, sparse_scale=0.5, mutant=None):
    """(A[n,3,3], det[n], sparse[n] bool, clamped[n] bool) from covariances C[n,3,3] and neighbour counts N[n] (steps 4 and 5)."""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 3, 3)
    N = np.asarray(N).reshape(-1)
    lam, v = eig_sym3(C)
    l1 = lam.max(axis=1)
    sparse = (N < min_neighbours) | ~(l1 > 0.0)
    ratio = lam / np.where(sparse, 1.0, l1)[:, None]
    lo = np.full_like(ratio, 1.0 / max_ratio)
    if mutant == "clamp_l3_only":   # only the smallest eigenvalue is clamped
        lo = np.where(ratio <= ratio.min(axis=1, keepdims=True), lo, 1e-12)
    a = 1.0 / np.maximum(ratio, lo)
    clamped = (ratio < 1.0 / max_ratio).any(axis=1) & ~sparse
    a[sparse] = 1.0 / sparse_scale
    A = np.einsum("nk,nik,njk->nij", a, v, v)
    same = (a[:, 0] == a[:, 1]) & (a[:, 1] == a[:, 2])   # a I: the sum over an orthonormal basis, without its rounding
    A[same] = a[same, 0][:, None, None] * np.eye(3)
    return A, a.prod(axis=1), sparse, clamped


def sym6(M):
    """(xx, xy, xz, yy, yz, zz) of symmetric M[n,3,3]: the library's layout."""
    M = np.asarray(M)
    return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], axis=1)


def from6(A6):
    A6 = np.asarray(A6, dtype=np.float64).reshape(-1, 6)
    return A6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def matrix_set(max_ratio=2.0, min_neighbours=25, seed=29):
    """(C6 f32[n,6], N i32[n]): 4000 random covariances V diag(lambda) V^T (random rotations, ratios log-uniform over six decades or uniform in [0.4, 1], scales
    from 1e-8 to 1e2) and the hard ones: all lambda equal, rank 2, rank 1, zero, ratios exactly at 1 / max_ratio, diagonal and
    nearly diagonal matrices, and neighbour counts at min_neighbours - 1 and min_neighbours."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(4000, 3, 3)))
    lam = 10.0 ** rng.uniform(-6.0, 0.0, size=(4000, 3))
    lam[3000:] = rng.uniform(0.4, 1.0, size=(1000, 3))   # the last thousand: ratios around and inside the clamp
    lam[:, 0] = 1.0
    lam *= 10.0 ** rng.uniform(-8.0, 2.0, size=(4000, 1))
    C = [np.einsum("nik,nk,njk->nij", q, lam, q)]
    R = q[:64]
    for l in ((1.0, 1.0, 1.0), (1.0, 0.3, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0 / max_ratio, 1.0 / max_ratio),
              (1.0, 1.0, 1.0 / max_ratio), (1.0, 0.5 + 1e-7, 0.5 - 1e-7), (1.0, 1.0 - 1e-7, 1e-30)):
        C.append(np.einsum("nik,k,njk->nij", R, np.array(l) * 4.9e-4, R))
        C.append(np.diag(np.array(l) * 4.9e-4)[None])
        C.append(np.diag(np.array(l)[::-1] * 4.9e-4)[None])
    near = np.diag([1.0, 0.7, 0.2])[None] + 1e-9 * (R[:8] + R[:8].transpose(0, 2, 1))
    C.append(near)
    C = np.concatenate(C)
    N = np.full(len(C), 60, dtype=np.int32)
    N[1::7] = min_neighbours
    N[3::7] = min_neighbours - 1
    return sym6(C).astype(np.float32), N


# The f32 routine against this model on matrix_set(): the largest ||A_f32 - A_model||_F measured, and the bound the tests allow -- 8 times
# that, because the set is a sample and not a proof (profiles/surface_aniso_bounds.txt)
A_F32_MEASURED = 1.7e-6
A_F32_BOUND = 8.0 * A_F32_MEASURED


class AnisoField:
    """phi(x) = sum_j V_j w_j(x), w_j(x) = det A_j W(|A_j (x - x_j)|), V_j = 1 / sum_k w_k(x_j); the interface of surface_model.Field."""

    def __init__(self, xyz, h, max_ratio=2.0, min_neighbours=25, sparse_scale=0.5, mutant=None):
        self.x = x = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.h, self.mutant = h, mutant
        n = len(x)
        self.N = np.zeros(n, dtype=np.int64)
        self.C = np.zeros((n, 3, 3))
        for a in range(0, n, 256):
            d = x[None, :, :] - x[a:a + 256, None, :]          # x_k - x_i
            r = np.linalg.norm(d, axis=2)
            near = (r <= h) if mutant == "count_le" else (r < h)
            self.N[a:a + 256] = near.sum(axis=1) - 1           # k != i
            w = np.where(near, 1.0 - (r / h) ** 3, 0.0)
            sw = w.sum(axis=1)
            mean = np.einsum("ik,ika->ia", w, d) / sw[:, None]
            dd = d if mutant == "cov_about_xi" else d - mean[:, None, :]
            self.C[a:a + 256] = np.einsum("ik,ika,ikb->iab", w, dd, dd) / sw[:, None, None]
        self.A, self.det, self.sparse, self.clamped = kernel_matrix(self.C, self.N, max_ratio, min_neighbours, sparse_scale, mutant)
        if mutant == "no_det":
            self.det = np.ones(n)
        self.V = np.ones(n)
        if mutant == "iso_V":
            self.V = SM.Field(x, h).V
        else:
            dens = np.zeros(n)
            for a in range(0, n, 256):
                dens[a:a + 256] = self._w(x[a:a + 256], np.arange(n))[0].sum(axis=1)
            self.V = 1.0 / dens
        self.n_max = 0
        self.k_max = 0.0

    def _w(self, pts, near):
        """(w_j(pts)[m, len(near)] without V_j, y = A_j (pts - x_j), |y|)"""
        d = pts[:, None, :] - self.x[near][None, :, :]
        y = np.einsum("kab,mkb->mka", self.A[near], d)
        q = np.linalg.norm(y, axis=2)
        return self.det[near][None, :] * SM.kernel_w(q, self.h), y, q

    def phi(self, pts):
        return self.phi_near(pts, np.arange(len(self.x)))

    def phi_near(self, pts, near):
        """phi at pts from the particles `near` (which must hold every particle within h of every point): surface_model.Field's loop,
        operation for operation, with y = A_j d in the place of d and det A_j V_j in the place of V_j."""
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        near = np.asarray(near)
        xs, A, Vd = self.x[near], self.A[near], self.det[near] * self.V[near]
        out = np.zeros(len(pts))
        for a in range(0, len(pts), 1024):
            q = pts[a:a + 1024]
            d = [q[:, None, c] - xs[None, :, c] for c in range(3)]
            d2 = (d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
            i, j = np.nonzero(d2 < self.h * self.h)       # |y| >= |d|: nothing outside contributes
            dx, dy, dz = d[0][i, j], d[1][i, j], d[2][i, j]
            y = [A[j, c, 0] * dx + A[j, c, 1] * dy + A[j, c, 2] * dz for c in range(3)]
            ql = np.sqrt(y[0] ** 2 + y[1] ** 2 + y[2] ** 2)
            np.add.at(out, a + i, SM.kernel_w(ql, self.h) * Vd[j])
            self.n_max = max(self.n_max, int(np.bincount(i).max()) if len(i) else 0)
            if len(i):   # the largest K of sens() over everything evaluated so far
                K = np.bincount(i, weights=Vd[j] * (3.0 * SM.kernel_w(ql, self.h) + np.abs(SM.kernel_dw(ql, self.h)) * np.sqrt(d2[i, j])))
                self.k_max = max(self.k_max, float(K.max()))
        return out

    def sens(self, pts):
        """(K, G) at pts: how far errors of the kernel matrices can move phi and grad phi.  With every |dA_j|_2 <= eps (and so every
        eigenvalue a_k >= 1 of A_j within eps, det A_j within 3 eps det A_j, |y| within eps |d|): |d phi| <= eps K, |d grad phi| <= eps G,
          K = sum_j V_j det_j (3 W(|y|) + |W'(|y|)| |d|),
          G = sum_j V_j det_j (3 |psi| |A y| + psi1 |d| |A y| + |psi| (|y| + |A_j|_2 |d|)),   psi = W'(|y|) / |y|, |psi'| <= psi1 = 18 k / h^4
        (grad w_j = det psi A y; psi' = 3 kG / h^2 for q <= 1/2 and kG (1 - q^2) / (q^2 h^2) <= that beyond, kG = 6 k / h), V_j held fixed."""
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        psi1 = 18.0 * 8.0 / (np.pi * self.h ** 3) / self.h ** 4 * self.h   # 3 kG / h^2
        every = np.arange(len(self.x))
        norm2 = np.abs(np.linalg.eigvalsh(self.A)).max(axis=1)
        K, G = np.zeros(len(pts)), np.zeros(len(pts))
        for a in range(0, len(pts), 256):
            p = pts[a:a + 256]
            w, y, q = self._w(p, every)
            dl = np.linalg.norm(p[:, None, :] - self.x[None, :, :], axis=2)
            inside = q < self.h
            dw = np.abs(SM.kernel_dw(q, self.h))
            psi = np.where(q > 1e-12, dw / np.maximum(q, 1e-300), 0.0)
            Ay = np.linalg.norm(np.einsum("kab,mkb->mka", self.A, y), axis=2)
            Vd = (self.V * self.det)[None, :]
            K[a:a + 256] = (self.V[None, :] * (3.0 * w + self.det[None, :] * dw * dl)).sum(axis=1)
            G[a:a + 256] = (Vd * inside * (3.0 * psi * Ay + psi1 * dl * Ay + psi * (q + norm2[None, :] * dl))).sum(axis=1)
        return K, G

    def grad(self, pts):
        """(grad phi, sum_j V_j |grad w_j|) at pts: grad w_j = det A_j W'(|y|) / |y| A_j y."""
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        g = np.zeros((len(pts), 3))
        ga = np.zeros(len(pts))
        every = np.arange(len(self.x))
        for a in range(0, len(pts), 256):
            _, y, q = self._w(pts[a:a + 256], every)
            s = np.where(q > 1e-12, SM.kernel_dw(q, self.h) / np.maximum(q, 1e-300), 0.0) * (self.V * self.det)[None, :]
            Ay = y if self.mutant == "grad_A" else np.einsum("kab,mkb->mka", self.A, y)
            g[a:a + 256] = (s[:, :, None] * Ay).sum(axis=1)
            ga[a:a + 256] = (np.abs(s) * np.linalg.norm(Ay, axis=2)).sum(axis=1)
        return g, ga


def reconstruct(xyz, radius, smoothing_length=3.5, cube_size=0.5, iso=0.6, normals=True, **aniso):
    """surface_model.reconstruct with the anisotropic field (aniso: max_ratio, min_neighbours, sparse_scale, mutant).  The result's
    "field" is the AnisoField (N, C, A, det, V, sparse, clamped per input particle)."""
    prm = dict(DEFAULTS, **aniso)
    iso_field = SM.Field
    SM.Field = lambda x, h: AnisoField(x, h, **prm)   # the one place where reconstruct() builds its field
    try:
        return SM.reconstruct(xyz, radius, smoothing_length, cube_size, iso, normals)
    finally:
        SM.Field = iso_field


# --- surface offsets of thin shapes (the table of DESIGN.md 29) ---------------------------------------------------------------------

def lattice(n, spacing, lo=(0.0, 0.0, 0.0)):
    g = [np.arange(k) * spacing for k in n]
    return np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(lo)


def offset_along(field, origins, direction, iso=0.6, radius=0.01, reach=4.0):
    """Mean over the rays origin + s direction of the s (multiples of the radius) at which phi falls through iso for the last time: phi
    sampled every 0.05, the crossing interpolated linearly between the last sample inside and the next."""
    s = np.arange(0.0, reach + 1e-9, 0.05)
    out = []
    for o in np.asarray(origins, dtype=np.float64).reshape(-1, 3):
        phi = field.phi(o[None, :] + s[:, None] * radius * np.asarray(direction, dtype=np.float64)[None, :])
        inside = np.nonzero(phi > iso)[0]
        if len(inside) == 0 or inside[-1] + 1 >= len(s):
            out.append(0.0 if len(inside) == 0 else s[-1])
            continue
        k = inside[-1]
        out.append(s[k] + 0.05 * (phi[k] - iso) / (phi[k] - phi[k + 1]))
    return float(np.mean(out))


def _rays_over_cell(centre, spacing, axes=(0, 1)):
    """9 ray origins over one lattice cell next to `centre`: on the particle, over the edge middles, over the cell's middle."""
    out = []
    for u in (0.0, 0.25, 0.5):
        for v in (0.0, 0.25, 0.5):
            o = np.array(centre, dtype=np.float64)
            o[axes[0]] += u * spacing
            o[axes[1]] += v * spacing
            out.append(o)
    return np.array(out)


def shape_table(make_field, radius=0.01, spacing=0.02, iso=0.6):
    """{row: offset in r} for the five shapes; make_field(xyz, h) -> a field with phi()."""
    h = 2.0 * 3.5 * radius
    rows = {}
    for name, nz in (("single layer 12x12x1", 1), ("double layer 12x12x2", 2)):
        x = lattice((12, 12, nz), spacing)
        top = np.array([5 * spacing, 5 * spacing, (nz - 1) * spacing])
        rows[name] = offset_along(make_field(x, h), _rays_over_cell(top, spacing), (0, 0, 1), iso, radius)
        if nz == 2:   # in the plane, outward from the middle of an edge, at the height of a layer and between the two
            F = make_field(x, h)
            rim = np.array([[11 * spacing, 5 * spacing, 0.0], [11 * spacing, 5.5 * spacing, 0.0], [11 * spacing, 5 * spacing, 0.5 * spacing],
                            [11 * spacing, 5.5 * spacing, 0.5 * spacing]])
            rows["rim of the double layer"] = offset_along(F, rim, (1, 0, 0), iso, radius)
    x = SM.jittered_block((0.0, 0.0, 0.0), (12, 12, 3), spacing, 0.3, 3).astype(np.float64)
    F = make_field(x, h)
    mid = [i for i in range(len(x)) if 3 * spacing < x[i, 0] < 8 * spacing and 3 * spacing < x[i, 1] < 8 * spacing and x[i, 2] > 1.5 * spacing]
    rows["3 jittered layers 12x12x3"] = offset_along(F, x[mid], (0, 0, 1), iso, radius)   # above each top-layer centre
    x = lattice((8, 8, 8), spacing)
    rows["face of an 8x8x8 block"] = offset_along(make_field(x, h), _rays_over_cell((3 * spacing, 3 * spacing, 7 * spacing), spacing),
                                                  (0, 0, 1), iso, radius)
    return rows


def lone_radius(make_field, radius=0.01, iso=0.6):
    """Radius (in r) at which one particle alone is meshed."""
    return offset_along(make_field(np.zeros((1, 3)), 2.0 * 3.5 * radius), np.zeros((1, 3)), (1, 0, 0), iso, radius)


if __name__ == "__main__":
    iso_t = shape_table(lambda x, h: SM.Field(x, h))
    ani_t = shape_table(lambda x, h: AnisoField(x, h, **DEFAULTS))
    print("| shape | isotropic | anisotropic, ratio 2 |\n|---|---|---|")
    for k in iso_t:
        print(f"| {k} | {iso_t[k]:.2f} r | {ani_t[k]:.2f} r |")
    print(f"| one particle alone (radius) | {lone_radius(lambda x, h: SM.Field(x, h)):.2f} r | "
          f"{lone_radius(lambda x, h: AnisoField(x, h, **DEFAULTS)):.2f} r |")
