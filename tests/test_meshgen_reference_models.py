"""Known-answer tests of the mesh -> particles path on the reference's OWN models
(its data/models/{cube,sphere,torus,icosphere,cone}.obj, stored unchanged under tests/golden/models/), placed the way its scene files place them
(final_scene1.json: sphere.obj scale 0.6; test.json: cube.obj scale 1; particleRadius 0.01 -> pitch 0.02).

trimesh is absent, so `mesh.voxelized(pitch).fill().points` (base_container.py:641-642) and `mesh.contains` (:686-694)
cannot be run; what CAN be checked without them, and independently of the numpy twin of tests/test_meshgen.py:

  * containment against a brute-force GENERALISED WINDING NUMBER (sum of the signed solid angles of all triangles, Van
    Oosterom & Strackee 1983) evaluated at every lattice point -- a different algorithm from the ray-crossing parity the
    product uses; agreement is asserted for every point of the np.arange lattice, selected or not;
  * closed-form volumes: the cube's edge^3, 4/3 pi r^3, 2 pi^2 R r^2 (radii read off the model's bounds), against
    count * pitch^3 within a surface-layer tolerance (area * pitch);
  * the voxel set of `voxel_points`: on integer multiples of the pitch, unique, x-major order; contains every lattice point
    whose winding number says "inside" (the fill is complete); every other voxel is within half a voxel diagonal of the
    surface (brute-force point-triangle distance: nothing but surface voxels was added); every mesh vertex falls into an
    occupied voxel (trimesh's subdivision voxeliser samples exactly the vertices of the subdivided mesh, the original ones
    among them); point symmetry about the origin for the centrally symmetric models (round() is odd, so the set of
    round(v / pitch) is symmetric when the triangulated model is: exactly for the cube, up to grazed voxels for the rest);
  * the torus keeps its hole through the fill."""
import os

import numpy as np
import pytest

from sph_project_amd import meshgen as M

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")
PITCH = 0.02   # particle diameter of every reference scene that loads a mesh (particleRadius 0.01)


def load(name, scale=1.0, translation=(0.0, 0.0, 0.0)):
    mesh = M.load_obj(os.path.join(MODELS, name))
    return M.place(mesh, [scale] * 3, 0.0, [0, 1, 0], translation)


def winding_number(mesh, pts, chunk=2048):
    """Generalised winding number of the closed triangle mesh about every point (1 inside, 0 outside)."""
    tri = mesh.vertices[mesh.faces]
    out = np.empty(len(pts))
    for s in range(0, len(pts), chunk):
        p = pts[s:s + chunk, None, None, :].astype(np.float64)
        a, b, c = (tri[None, :, k, :] - p[:, :, 0, :] for k in range(3))
        la, lb, lc = (np.linalg.norm(v, axis=-1) for v in (a, b, c))
        num = np.einsum("pfi,pfi->pf", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("pfi,pfi->pf", a, b) * lc + np.einsum("pfi,pfi->pf", b, c) * la + np.einsum("pfi,pfi->pf", c, a) * lb
        out[s:s + chunk] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
    return out


def orientation(mesh):
    """+1 if the faces are wound outward (positive signed volume), -1 otherwise."""
    t = mesh.vertices[mesh.faces]
    return np.sign(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum())


def mesh_volume_area(mesh):
    t = mesh.vertices[mesh.faces]
    vol = abs(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum()) / 6.0
    area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum()
    return vol, area


def dist_to_surface(mesh, pts, chunk=512):
    """Brute-force distance of every point to the triangle soup (closest point on each triangle, Ericson 5.1.5)."""
    tri = mesh.vertices[mesh.faces]
    A, B, C = tri[:, 0][None], tri[:, 1][None], tri[:, 2][None]
    ab, ac = B - A, C - A
    out = np.empty(len(pts))
    for s in range(0, len(pts), chunk):
        p = pts[s:s + chunk, None, :].astype(np.float64)
        ap = p - A
        d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
        bp = p - B
        d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
        cp = p - C
        d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
        va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
        with np.errstate(divide="ignore", invalid="ignore"):
            den = va + vb + vc
            v, w = vb / den, vc / den
            q = A + ab * v[..., None] + ac * w[..., None]                    # interior
            t_ab = d1 / (d1 - d3)
            t_ac = d2 / (d2 - d6)
            t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], A + ab * t_ab[..., None], q)
        q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], A + ac * t_ac[..., None], q)
        q = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], B + (C - B) * t_bc[..., None], q)
        q = np.where(((d1 <= 0) & (d2 <= 0))[..., None], A + 0 * q, q)
        q = np.where(((d3 >= 0) & (d4 <= d3))[..., None], B + 0 * q, q)
        q = np.where(((d6 >= 0) & (d5 <= d6))[..., None], C + 0 * q, q)
        out[s:s + chunk] = np.linalg.norm(p - q, axis=-1).min(axis=1)
    return out


CASES = {
    # name: (file, scale, translation of a scene that uses it or a lattice-generic one)
    "cube": ("cube.obj", 1.0, (1.0, 2.3, 1.0)),            # test.json
    "sphere": ("sphere.obj", 0.6, (0.3, 2.4, 1.25)),       # final_scene1.json
    "torus": ("torus.obj", 1.0, (0.813, 0.407, 0.611)),
    "icosphere": ("icosphere.obj", 0.3, (0.5, 0.5, 0.5)),
    "cone": ("cone.obj", 0.3, (0.411, 0.523, 0.637)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_models_are_closed_and_winding_number_is_an_indicator(name):
    """Premise of everything below: the model is a closed surface, so the winding number is 0 or +-1 away from it."""
    f, s, t = CASES[name]
    mesh = load(f, s, t)
    edges = np.sort(np.concatenate([mesh.faces[:, [0, 1]], mesh.faces[:, [1, 2]], mesh.faces[:, [2, 0]]]), axis=1)
    # OBJ files repeat vertices along texture seams: weld by position before counting edge uses
    _, inv = np.unique(np.round(mesh.vertices, 9), axis=0, return_inverse=True)
    we = np.sort(inv.reshape(-1)[edges], axis=1)
    we = we[we[:, 0] != we[:, 1]]
    _, cnt = np.unique(we, axis=0, return_counts=True)
    assert np.all(cnt == 2), (name, np.bincount(cnt))
    rng = np.random.default_rng(3)
    lo, hi = mesh.bounds
    p = rng.uniform(lo - 0.1, hi + 0.1, (400, 3))
    w = winding_number(mesh, p) * orientation(mesh)
    assert np.all((np.abs(w) < 1e-6) | (np.abs(w - 1) < 1e-6)), (name, w[(np.abs(w) > 1e-6) & (np.abs(w - 1) > 1e-6)])


@pytest.mark.parametrize("name", list(CASES))
def test_fluid_points_equal_the_winding_number_selection(name):
    """load_fluid_body (:676-694): every point of the np.arange lattice over the bounds is selected iff it is inside."""
    f, s, t = CASES[name]
    mesh = load(f, s, t)
    pts = M.fluid_points(mesh, PITCH)
    lo, hi = mesh.bounds
    axes = [np.arange(lo[k], hi[k], PITCH) for k in range(3)]
    lattice = np.array(np.meshgrid(*axes, sparse=False, indexing="ij"), dtype=np.float32).reshape(3, -1).T
    w = winding_number(mesh, lattice) * orientation(mesh)
    inside = w > 0.5
    # points ON the surface (the lattice starts on the bounding box: cube faces, poles) have no defined side
    clear = dist_to_surface(mesh, lattice) > 1e-6
    sel = np.zeros(len(lattice), bool)
    key = {tuple(r) for r in pts.tolist()}
    sel[[i for i, r in enumerate(lattice.tolist()) if tuple(r) in key]] = True
    assert sel.sum() == len(pts)                       # every returned point is a lattice point, none twice
    assert np.array_equal(sel[clear], inside[clear]), (name, int((sel != inside)[clear].sum()))
    # meshgrid 'ij' order (z fastest), as base_container.py:689-693 leaves it
    assert np.all(np.lexsort((pts[:, 2], pts[:, 1], pts[:, 0])) == np.arange(len(pts)))
    vol, area = mesh_volume_area(mesh)
    assert abs(len(pts) * PITCH ** 3 - vol) <= 0.75 * area * PITCH, (name, len(pts) * PITCH ** 3, vol)


def test_closed_form_volumes():
    cube = load(*CASES["cube"][:1], CASES["cube"][1], CASES["cube"][2])
    edge = np.ptp(cube.vertices, axis=0)
    assert np.allclose(edge, edge[0])
    n = M.fluid_points(cube, PITCH)
    # the lattice starts ON the lower faces (np.arange from the bounds' minimum): containment is half-open, [lo, hi), like np.arange
    # itself, so a box-shaped body gets its full k^3 block (round 4: 14 of the 225 points of the lower z face used to be lost to a
    # crossing computed 1 ulp above the lattice's own z)
    k = len(np.arange(0.0, edge[0], PITCH))
    assert len(n) == k ** 3, (len(n), k)
    sph = load("sphere.obj", 0.6, (0.3, 2.4, 1.25))
    r = 0.5 * np.ptp(sph.vertices, axis=0)
    assert np.allclose(r, r[0], rtol=2e-3)
    npts = len(M.fluid_points(sph, PITCH))
    exact = 4.0 / 3.0 * np.pi * r[0] ** 3
    # the polyhedron (32 x 16 facets) is smaller than its sphere by ~1.2 %; the lattice count scatters by a surface layer
    assert -0.03 < (npts * PITCH ** 3 - exact) / exact < 0.005, (npts * PITCH ** 3, exact)
    tor = load("torus.obj", 2.0, CASES["torus"][2])    # tube radius = 6 pitches
    ext = np.sort(np.ptp(tor.vertices, axis=0))
    rr = 0.5 * ext[0]                                   # tube radius = half the extent along the axis
    RR = 0.5 * ext[2] - rr
    exact = 2.0 * np.pi ** 2 * RR * rr ** 2
    poly, area = mesh_volume_area(tor)
    # 24 x 12 inscribed facets: the polyhedron holds (12 / 2 pi) sin(2 pi / 12) = 95.5 % of the tube's cross-section
    assert -0.06 < (poly - exact) / exact < 0.0, (poly, exact)
    npts = len(M.fluid_points(tor, PITCH))
    assert abs(npts * PITCH ** 3 - poly) / poly < 0.02, (npts * PITCH ** 3, poly)


@pytest.mark.parametrize("name", list(CASES))
def test_voxel_points_are_surface_voxels_plus_a_complete_fill(name):
    """load_rigid_body (:641-642)."""
    f, s, t = CASES[name]
    mesh = load(f, s, t)
    vox = M.voxel_points(mesh, PITCH)
    assert vox.dtype == np.float32 and vox.ndim == 2 and vox.shape[1] == 3
    idx = np.round(vox.astype(np.float64) / PITCH).astype(np.int64)
    assert np.allclose(idx * PITCH, vox, atol=1e-6)                                  # centres = integer multiples of the pitch
    assert len(np.unique(idx, axis=0)) == len(idx)
    assert np.all(np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0])) == np.arange(len(idx)))   # x-major (np.argwhere order of the dense grid)
    occupied = {tuple(r) for r in idx.tolist()}
    # (1) every vertex of the model sits in an occupied voxel
    vidx = np.round(mesh.vertices / PITCH).astype(np.int64)
    assert all(tuple(r) in occupied for r in vidx.tolist())
    # (2) the fill is complete: every lattice point strictly inside the model is a voxel
    lo = np.floor(mesh.bounds[0] / PITCH).astype(int) - 1
    hi = np.ceil(mesh.bounds[1] / PITCH).astype(int) + 1
    grid = np.stack(np.meshgrid(*[np.arange(lo[k], hi[k] + 1) for k in range(3)], indexing="ij"), -1).reshape(-1, 3)
    w = winding_number(mesh, grid * PITCH) * orientation(mesh)
    inside = w > 0.5
    in_set = np.array([tuple(r) in occupied for r in grid.tolist()])
    missing = inside & ~in_set
    assert not missing.any(), (name, int(missing.sum()))
    # (3) nothing but surface voxels was added: a voxel outside the model holds a piece of the surface, i.e. its centre is no
    #     further from it than half the voxel's diagonal
    extra = grid[in_set & ~inside]
    d = dist_to_surface(mesh, extra * PITCH) if len(extra) else np.zeros(1)
    assert d.max() <= 0.5 * np.sqrt(3.0) * PITCH * (1 + 1e-9), (name, d.max() / PITCH)
    # (4) volume: model + at most a shell one voxel thick
    vol, area = mesh_volume_area(mesh)
    assert vol - 0.5 * area * PITCH <= len(vox) * PITCH ** 3 <= vol + 1.0 * area * PITCH, (name, len(vox) * PITCH ** 3, vol, area * PITCH)


@pytest.mark.parametrize("name", ["cube", "sphere", "torus"])
def test_voxel_set_has_the_models_point_symmetry(name):
    """The three models are symmetric under x -> -x about their own centre (the origin of the file); np.round is odd, so the
    occupied index set of the untranslated model is symmetric too -- exactly, voxel for voxel."""
    mesh = load(CASES[name][0], CASES[name][1])
    v = mesh.vertices
    # premise: the vertex set itself is centrally symmetric (to the 6 digits the file keeps)
    a = np.unique(np.round(v, 5), axis=0)
    b = np.unique(np.round(-v, 5), axis=0)
    if a.shape != b.shape or not np.allclose(a, b, atol=2e-5):
        pytest.skip("model is not centrally symmetric")
    idx = np.round(M.voxel_points(mesh, PITCH).astype(np.float64) / PITCH).astype(np.int64)
    s0 = {tuple(r) for r in idx.tolist()}
    s1 = {tuple(r) for r in (-idx).tolist()}
    # exact for the cube; the sphere's and the torus' quads are non-planar and the file's triangulation picks one diagonal, whose
    # mirror image is the OTHER diagonal: the two surfaces differ by less than the facet sagitta, i.e. in voxels they merely graze
    limit = 0 if name == "cube" else 0.02 * len(s0)
    assert len(s0 ^ s1) <= limit, (name, len(s0 ^ s1), len(s0))


def test_torus_keeps_its_hole():
    tor = load("torus.obj", 1.0)
    ext = np.ptp(tor.vertices, axis=0)
    axis = int(np.argmin(ext))                         # the torus' axis = its thinnest extent
    rr = 0.5 * ext[axis]
    RR = 0.5 * np.max(ext) - rr
    vox = M.voxel_points(tor, PITCH)
    radial = np.linalg.norm(np.delete(vox, axis, axis=1), axis=1)
    assert radial.min() > RR - rr - PITCH                                            # nothing in the hole
    assert radial.max() < RR + rr + PITCH
    fl = M.fluid_points(tor, PITCH)
    radial = np.linalg.norm(np.delete(fl, axis, axis=1), axis=1)
    assert radial.min() > RR - rr - 1e-6 and radial.max() < RR + rr + 1e-6
