"""GPU: traced mesh frames (csrc/sph_render_trace.hpp): the invariants of the hierarchy built on the device, culling that
changes nothing (the frame traced through the hierarchy against the frame in which every ray tests every triangle, byte for byte, in both
builds and on a repeat), every recorded water segment against the float64 terms of tests/render_trace_model.py, known answers (a
shadow, a water slab, total internal reflection, paths cut at max_depth, the reconstructor's winding) and the plumbing."""
import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd.render import FrameRenderer, RenderError
from sph_project_amd.surface import SurfaceReconstructor
from tests import render_trace_model as TM
from tests.test_hip_render_mesh import BLOCK_CAMERA, UNIT_BOX, backdrop, block_surface, golden_meshes

pytestmark = pytest.mark.gpu

RADIUS = 0.01
WATER = (60, 140, 220)


def box_mesh(lo, hi):
    """a closed box wound outwards: 8 corners, 12 triangles"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    v = np.array([[(hi if (a >> k) & 1 else lo)[k] for k in range(3)] for a in range(8)], np.float32)   # corner a: bit k picks hi on axis k
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # -z, +z, -y, +y, -x, +x seen from outside
    t = np.array([[a, b, c] for a, b, c, d in q] + [[a, c, d] for a, b, c, d in q], np.int32)
    return v, t


def kept(meshes):
    """global indices and float32 corners (n, 3, 3) of the triangles the set-up keeps: valid indices, finite corners, no two corners
    equal and a non-zero cross product"""
    out_g, out_c, g0 = [np.zeros(0, np.int64)], [np.zeros((0, 3, 3), np.float32)], 0
    for v, t, *_ in meshes:
        v, t = np.asarray(v, np.float32), np.asarray(t, np.int64)
        ok = ((t >= 0) & (t < len(v))).all(axis=1)
        c = v[np.clip(t, 0, max(len(v) - 1, 0))]
        ok &= np.isfinite(c).all(axis=(1, 2))
        with np.errstate(invalid="ignore", over="ignore"):
            n = np.cross(c[:, 1].astype(np.float64) - c[:, 0], c[:, 2].astype(np.float64) - c[:, 0])
        ok &= (n != 0).any(axis=1)
        out_g.append(g0 + np.nonzero(ok)[0])
        out_c.append(c[ok])
        g0 += len(t)
    return np.concatenate(out_g), np.concatenate(out_c)


def check_tree(r, meshes, label):
    st = r.trace_stats()
    g, c = kept(meshes)
    n = len(g)
    assert st["triangles"] == n and st["nodes"] == max(2 * n - 1, 0) and st["aborted_rays"] == 0, (label, st, n)
    b = r.trace_bvh()
    assert sorted(b["leaf_triangle"].tolist()) == g.tolist(), label   # every kept triangle is exactly one leaf
    if n == 0:
        return st
    left, right, boxes = b["left"], b["right"], b["boxes"]
    assert len(left) == len(right) == n - 1 and boxes.shape == (2 * n - 1, 6)
    kids = np.concatenate([left, right])
    assert ((kids >= 1) & (kids < 2 * n - 1)).all() and len(np.unique(kids)) == 2 * n - 2, label   # one parent each, the root has none
    # no node is reachable twice, every node is reached, the depth is within the bound of the 64-bit keys
    seen = np.zeros(2 * n - 1, bool)
    level = np.array([0])
    depth = -1
    while len(level):
        assert not seen[level].any(), label
        seen[level] = True
        depth += 1
        inner = level[level < n - 1]
        level = np.concatenate([left[inner], right[inner]])
    assert seen.all() and depth == st["depth"] and depth <= 64, (label, depth, st["depth"])
    # boxes: bit for bit the union of the corners (leaves) and of the children (inner nodes)
    corner = dict(zip(g.tolist(), c))
    lc = np.stack([corner[int(t)] for t in b["leaf_triangle"]])
    want = np.concatenate([lc.min(axis=1), lc.max(axis=1)], axis=1)
    assert boxes[n - 1:].tobytes() == want.tobytes(), label
    if n > 1:
        u = np.concatenate([np.minimum(boxes[left, :3], boxes[right, :3]), np.maximum(boxes[left, 3:], boxes[right, 3:])], axis=1)
        assert boxes[:n - 1].tobytes() == u.tobytes(), label
    return st


def renderer(fast=False, size=64, **kw):
    base = dict(width=size, height=size, box=UNIT_BOX, camera_position=(0.5, 1.3, 2.4), camera_lookat=(0.5, 0.25, 0.5), fov=45.0)
    base.update(kw)
    return FrameRenderer(RADIUS, fast_math=fast, **base)


def trace_both(r, meshes, **kw):
    """the frame through the hierarchy, once more, and with every ray testing every triangle: the same bytes; returns the first"""
    out = []
    for bvh in (True, True, False):
        r.set_trace(bvh=bvh, record=True, **kw)
        rgb = r.from_meshes(meshes)
        st = r.trace_stats()
        assert st["aborted_rays"] == 0
        out.append((rgb, r.ids(), r.trace_paths(), st))
    a = out[0]
    for b in out[1:]:
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        for k in ("triangles", "rays_primary", "rays_path", "rays_reflect", "rays_shadow", "truncated"):
            assert a[3][k] == b[3][k], k
    assert out[2][3]["node_visits"] == 0 and a[3]["node_visits"] > 0 or a[3]["triangles"] == 0
    return a


def hits(paths, meshes, label, stride=1, **scene):
    """the winner, t, flat normals, shadow words and contributions of the recorded segments against the scene in float64; the unsure
    segments (ambiguous winner, grazing ray, near-miss shadow ray) stay under 1 %"""
    rep = TM.check_hits(paths, TM.Scene(meshes, radius=RADIUS, **scene), stride=stride)
    print(label, "hits", rep)
    assert rep["segments"] > 0 and rep["ambiguous"] + rep["grazing"] + rep["near_miss"] < 0.01 * rep["segments"], (label, rep)
    return rep


def golden_scene():
    m = golden_meshes(smooth_icosphere=True)
    return [m[0] + ("water",), m[1], m[2]]


# --- 1. the hierarchy ----------------------------------------------------------------------------------------------------------------------
def line_of_triangles(n):
    """n copies of one small triangle whose centroids lie on one line"""
    base = np.float32([[0.0, 0.0, 0.0], [0.004, 0.0, 0.001], [0.001, 0.004, 0.0]])
    off = np.float32([0.1, 0.3, 0.5]) + np.arange(n, dtype=np.float32)[:, None] * np.float32([0.8 / n, 0.0, 0.0])
    v = (base[None] + off[:, None]).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3), None, (200, 200, 200)


@pytest.mark.parametrize("fast", [False, True])
def test_tree_invariants_on_the_smallest_shapes_that_can_break_a_build(gpu, fast):
    r = renderer(fast)
    r.set_trace()
    tri = (np.float32([[0.2, 0.3, 0.5], [0.8, 0.3, 0.4], [0.5, 0.7, 0.6]]), np.int32([[0, 1, 2]]), None, (255, 0, 0))
    two = (tri[0], np.int32([[0, 1, 2], [2, 1, 0]]), None, (255, 0, 0))
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, (1, 2, 3))
    gm = golden_meshes()
    cases = {"none": [], "empty mesh": [empty], "one": [tri], "two coincident": [two], "twice": [gm[1], gm[1]], "golden": gm,
             "line": [line_of_triangles(4097)]}
    for label, meshes in cases.items():
        r.from_meshes(meshes)
        st = check_tree(r, meshes, label)
        print(label, {k: st[k] for k in ("triangles", "depth", "node_visits", "triangle_tests")})
        ids = r.ids()
        if label in ("none", "empty mesh"):   # the floor alone
            assert st["triangles"] == 0 and (ids == L.RENDER_TRACE_FLOOR_ID).sum() > 500 and not (ids >= 0).any()
        if label == "two coincident":         # an exact tie goes to the smaller index
            assert set(np.unique(ids[ids >= 0])) == {0}
        if label == "twice":
            assert set(np.unique(r.mesh_of(ids)[ids >= 0])) == {0}
    # skipped triangles: counted, and the rest of the frame unchanged
    clean = r.from_meshes(gm).tobytes()
    clean_ids = r.ids().tobytes()
    tv, tt, _, tcol = gm[2]
    nl = len(tv)
    dirty_v = np.concatenate([tv, np.float32([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5]])])
    extra = np.array([[0, 1, nl], [nl + 1, 2, 3], [4, 4, 5], [6, 7, 7]], np.int32)
    dirty = [gm[0], gm[1], (dirty_v, np.concatenate([tt, extra]), None, tcol)]
    assert r.from_meshes(dirty).tobytes() == clean and r.ids().tobytes() == clean_ids
    st = check_tree(r, dirty, "dirty")
    r.clear_trace()   # the raster frame of the same list counts the same triangles out
    r.from_meshes(dirty)
    ms = r.mesh_stats()
    assert (ms["skipped_nonfinite"], ms["skipped_degenerate"], ms["bad_index"]) == (2, 2, 0)
    r.set_trace()
    assert (st["skipped_nonfinite"], st["skipped_degenerate"], st["bad_index"]) == (2, 2, 0)
    worse = [gm[0], gm[1], (tv, np.concatenate([tt, np.array([[0, 1, nl], [-1, 2, 3], [0, 1, 2 ** 30]], np.int32)]), None, tcol)]
    with pytest.raises(RenderError) as e:
        r.from_meshes(worse)
    assert e.value.code == -1
    assert r.trace_stats()["bad_index"] == 3 and r.mesh_stats()["bad_index"] == 3
    assert r.last_rgb().tobytes() == clean and r.ids().tobytes() == clean_ids
    check_tree(r, worse, "bad index")


# --- 2. and 3. culling changes nothing; every segment against the model --------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True])
def test_golden_scene_is_the_same_with_and_without_the_hierarchy_and_matches_the_terms(gpu, fast):
    r = renderer(fast, size=96)
    rgb, ids, paths, st = trace_both(r, golden_scene(), absorb=0.05)
    assert st["truncated"] < 0.01 * 96 * 96 and st["rays_shadow"] > 1000 and st["rays_reflect"] > 100 and st["rays_path"] > 200
    assert {0, 1, 2} <= set(np.unique(r.mesh_of(ids)[ids >= 0])) and (ids == L.RENDER_TRACE_FLOOR_ID).sum() > 500 and (ids <= -2).any()
    rep = TM.check_segments(paths, rgb, ids, (0, 0, 0), 1.33, 6, st["truncated"], water=((230, 60, 40), 0.05, RADIUS))
    print("golden", fast, st, rep)
    assert rep["water_segments"] > 200 and rep["unsure"] < 0.01 * rep["water_segments"]
    hr = hits(paths, golden_scene(), "golden", box=UNIT_BOX)
    assert hr["shaded"] > 1000 and hr["blended"] > 200 and hr["reflections"] > 100
    # the water sphere does not block the light, the torus and the cube do: some floor pixels are in shadow, at the ambient level
    I = paths.view(np.int32)
    floor = ids == L.RENDER_TRACE_FLOOR_ID
    shadowed = floor & (I[:, :, 0, TM.W_SHADOW] == 1)
    assert shadowed.sum() > 50 and (rgb[shadowed] <= 21).all() and (rgb[floor & (I[:, :, 0, TM.W_SHADOW] == 0)] > 21).all()


@pytest.mark.parametrize("fast", [False, True])
def test_smoothed_surface_in_front_of_a_backdrop(gpu, fast):
    container, solver, recon, (v, t, n) = block_surface(fast)
    state = [container.engine.download(f).tobytes() for f in (L.F_POSITION, L.F_VELOCITY, L.F_PARTICLE_ID)]
    r = FrameRenderer(RADIUS, width=96, height=96, fast_math=fast, **BLOCK_CAMERA)
    meshes = [backdrop(), (v, t, n, WATER, "water")]
    rgb, ids, paths, st = trace_both(r, meshes, absorb=0.05)
    check_tree(r, meshes, "surface")
    rep = TM.check_segments(paths, rgb, ids, (0, 0, 0), 1.33, 6, st["truncated"], water=(WATER, 0.05, RADIUS))
    print("surface", fast, st, rep)
    hr = hits(paths, meshes, "surface", stride=8)
    assert hr["blended"] > 50 and hr["reflections"] > 20   # the blend of the surface's own normals, the backdrop seen in the water
    assert (ids >= 2).sum() > 800 and (ids == -1).sum() == 0 and rep["unsure"] < 0.01 * rep["water_segments"]
    # the device copy of the surface gives the same frame, and the surface object and the simulation are untouched
    r.set_trace(record=True, absorb=0.05)
    again = r.from_meshes([backdrop(), (recon, WATER, "water")])
    assert again.tobytes() == rgb.tobytes() and r.ids().tobytes() == ids.tobytes()
    v2, t2, n2 = recon._download()
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes() and n2.tobytes() == n.tobytes()
    assert [container.engine.download(f).tobytes() for f in (L.F_POSITION, L.F_VELOCITY, L.F_PARTICLE_ID)] == state


# --- 4. known answers ----------------------------------------------------------------------------------------------------------------------
def test_a_quad_between_the_light_and_the_floor_casts_its_shadow(gpu):
    light = np.float64([0.5, 2.0, 0.5])
    quad = (np.float32([[0.35, 0.5, 0.35], [0.65, 0.5, 0.35], [0.65, 0.5, 0.65], [0.35, 0.5, 0.65]]), np.int32([[0, 1, 2], [0, 2, 3]]), None,
            (255, 255, 255))
    cam = dict(camera_position=(0.5, 1.6, 2.2), camera_lookat=(0.5, 0.0, 0.5), fov=40.0)
    r = renderer(size=96, light_position=tuple(light), **cam)
    rgb, ids, paths, st = trace_both(r, [quad], floor_cell=1000.0)   # (one checker cell: the floor has one tone, 204)
    # the analytic shadow: the quad projected from the light onto y = 0, a square about (0.5, 0.5) of half width 0.15 x 2 / 1.5 = 0.2
    c = TM.camera(cam["camera_position"], cam["camera_lookat"], fov=cam["fov"], W=96, H=96)
    d = TM.pixel_rays(c, 96, 96)
    # a pixel is well inside (outside) when its centre and the centres of its eight neighbours are: the shape shrunk (grown) by a pixel
    P = TM.plane_hit(c[0], d, 0.0)
    cheb = np.maximum(np.abs(P[..., 0] - 0.5), np.abs(P[..., 2] - 0.5))
    pad = np.pad(cheb, 1, mode="edge")
    near = np.stack([pad[1 + a:97 + a, 1 + b:97 + b] for a in (-1, 0, 1) for b in (-1, 0, 1)])
    floor = ids == L.RENDER_TRACE_FLOOR_ID
    inside, outside = floor & (near.max(axis=0) < 0.2), floor & (near.min(axis=0) > 0.2)
    ambient = int(np.floor(255.0 * (204.0 / 255.0 * 0.1) + 0.5))
    assert hits(paths, [quad], "shadow", box=UNIT_BOX, floor_cell=1000.0, light=light)["shaded"] > 2000
    print("shadow: floor", int(floor.sum()), "inside", int(inside.sum()), "outside", int(outside.sum()))
    assert inside.sum() > 100 and outside.sum() > 1000
    assert (rgb[inside] == ambient).all() and (rgb[outside] > ambient).all()
    r.set_trace(shadows=False, floor_cell=1000.0)
    assert (r.from_meshes([quad])[inside] > ambient).all()


SLAB = ((0.1, 0.2, 0.1), (0.9, 0.4, 0.9))
SLAB_CAMERA = dict(camera_position=(0.5, 1.5, 1.6), camera_lookat=(0.5, 0.3, 0.5), fov=20.0)


def test_a_water_slab_moves_the_floor_behind_it_where_snell_puts_it(gpu):
    """Tolerance: three segments (air, water, air), each end point O + t d with a direction known to DIR_TOL and positions below 2:
    per segment <= length x DIR_TOL + POS_TOL, lengths <= 2: the recorded floor point lies within 3 (2 DIR_TOL + POS_TOL) = 504 u of
    the float64 one; 512 u is asserted."""
    v, t = box_mesh(*SLAB)
    r = renderer(size=64, **SLAB_CAMERA)
    rgb, ids, paths, st = trace_both(r, [(v, t, None, WATER, "water")], absorb=0.05)
    rep = TM.check_segments(paths, rgb, ids, (0, 0, 0), 1.33, 6, st["truncated"], water=(WATER, 0.05, RADIUS))
    hits(paths, [(v, t, None, WATER, "water")], "slab", box=UNIT_BOX)
    c = TM.camera(SLAB_CAMERA["camera_position"], SLAB_CAMERA["camera_lookat"], fov=SLAB_CAMERA["fov"], W=64, H=64)
    d = TM.unit(TM.pixel_rays(c, 64, 64)[24:40, 24:40])
    up = np.float64([0.0, 1.0, 0.0])
    P1 = TM.plane_hit(c[0], d, 0.4)
    d2 = TM.snell(d, up, 1.0 / 1.33)[0]
    P2 = TM.plane_hit(P1, d2, 0.2)
    d3 = TM.snell(d2, up, 1.33)[0]
    P3 = TM.plane_hit(P2, d3, 0.0)
    assert np.abs(d3 - d).max() < 1e-12   # (parallel faces: the ray leaves as it came, moved sideways)
    I = paths.view(np.int32)[24:40, 24:40]
    Q = paths[24:40, 24:40].astype(np.float64)
    assert (I[:, :, 0, TM.W_ID] >= 0).all() and (I[:, :, 1, TM.W_ID] >= 0).all() and (I[:, :, 2, TM.W_ID] == L.RENDER_TRACE_FLOOR_ID).all()
    assert ((I[:, :, 0, TM.W_FLAGS] & TM.F_ENTER) != 0).all() and ((I[:, :, 1, TM.W_FLAGS] & (TM.F_ENTER | TM.F_INSIDE)) == TM.F_INSIDE).all()
    got = Q[:, :, 2, :3] + Q[:, :, 2, TM.W_T, None] * Q[:, :, 2, 3:6]
    err = np.abs(got - P3).max()
    straight = np.abs(TM.plane_hit(c[0], d, 0.0) - P3).max()
    print("slab: floor point error", err, "bound", 512 * TM.U, "moved by the slab", straight, rep)
    assert err <= 512 * TM.U and straight > 0.02
    # absorption: the throughput at the exit is (1 - F) exp2(-absorb (1 - rgb / 255) l / radius) of the entry's
    T = TM.transmittance(WATER, 0.05, RADIUS, np.linalg.norm(P2 - P1, axis=-1))
    F = TM.schlick(-np.sum(d * up, axis=-1), 1.33)
    assert np.abs(Q[:, :, 1, TM.W_THR1:TM.W_THR1 + 3] - ((1 - F) ** 2)[..., None] * T).max() <= 4 * TM.THR_TOL


def test_from_inside_beyond_the_critical_angle_the_path_reflects(gpu):
    v, t = box_mesh((-2.0, -1.0, -2.0), (3.0, 0.6, 3.0))
    # the camera under the surface y = 0.6, looking up at 20 degrees above the horizontal: 70 degrees from the normal, beyond 48.8
    cam = dict(camera_position=(0.5, 0.3, 2.0), camera_lookat=(0.5, 0.3 + np.tan(np.radians(20.0)), 1.0), fov=10.0)
    r = renderer(size=64, box=None, **cam)
    rgb, ids, paths, st = trace_both(r, [(v, t, None, WATER, "water")], absorb=0.0)
    I, Q = paths.view(np.int32), paths.astype(np.float64)
    fl = I[:, :, 0, TM.W_FLAGS]
    assert ((fl & TM.F_TIR) != 0).all() and ((fl & TM.F_ENTER) == 0).all() and (Q[:, :, 0, TM.W_F] == 0).all()
    assert (Q[:, :, 0, TM.W_THR1:TM.W_THR1 + 3] == 1.0).all()
    d0 = TM.unit(Q[:, :, 0, 3:6])
    assert np.abs(Q[:, :, 1, 3:6] - d0 * np.float64([1.0, -1.0, 1.0])).max() <= TM.DIR_TOL
    TM.check_segments(paths, rgb, ids, (0, 0, 0), 1.33, 6, st["truncated"])
    hits(paths, [(v, t, None, WATER, "water")], "inside", absorb=0.0)


def test_paths_through_more_interfaces_than_max_depth_are_cut_and_counted(gpu):
    a, b = box_mesh((-5.0, 0.6, -5.0), (6.0, 0.7, 6.0)), box_mesh((-5.0, 0.3, -5.0), (6.0, 0.4, 6.0))
    meshes = [(a[0], a[1], None, WATER, "water"), (b[0], b[1], None, WATER, "water")]
    # (looking straight down, a little off the middle: no pixel centre lies on the diagonal edge of a face, where a path would start
    # on the edge shared with the face's other triangle -- DESIGN.md 30, what is not done)
    cam = dict(camera_position=(0.513, 2.0, 0.507), camera_lookat=(0.513, 0.0, 0.507), camera_up=(0.0, 0.0, -1.0), fov=30.0)
    r = renderer(size=64, background=(10, 200, 30), **cam)
    rgb, ids, paths, st = trace_both(r, meshes, max_depth=3, floor=False)
    assert st["truncated"] == 64 * 64   # four interfaces along every ray, three segments
    TM.check_segments(paths, rgb, ids, (10, 200, 30), 1.33, 3, st["truncated"])
    hits(paths, meshes, "nested", box=UNIT_BOX, floor=False, background=(10, 200, 30))
    rgb, ids, paths, st = trace_both(r, meshes, max_depth=5, floor=False)
    assert st["truncated"] == 0
    TM.check_segments(paths, rgb, ids, (10, 200, 30), 1.33, 5, 0)


def test_the_reconstructor_winds_its_triangles_outwards(gpu):
    g = np.arange(-6, 7) * (2 * RADIUS)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    centre = np.float64([0.5, 0.5, 0.5])
    p = (p[np.linalg.norm(p, axis=1) <= 0.12] + centre).astype(np.float32)
    recon = SurfaceReconstructor(RADIUS)
    v, t, n = recon.from_points(p)
    c = v[t].astype(np.float64)
    N = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    s = np.sum(N * (c.mean(axis=1) - centre), axis=1)
    print("winding: triangles", len(t), "outwards", int((s > 0).sum()), "inwards", int((s < 0).sum()))
    assert len(t) > 500 and (s > 0).all()
    # so a ray from outside enters at its first hit and leaves at its second; with the flag set for an inward-wound copy of the mesh too
    # (a camera off the lattice's planes of symmetry: no pixel centre's ray runs through an edge of the mesh; and close by: the
    # band about an edge in which a hit is only possible grows with the square of the distance over the edge's length, and from 1.5
    # away it made 3.6 % of these small triangles' segments ambiguous)
    r = renderer(size=64, box=None, camera_position=(0.5745, 0.547, 0.839), camera_lookat=(0.5, 0.5, 0.5), fov=14.0)
    for mesh in [(v, t, n, WATER, "water"), (v, t[:, ::-1].copy(), n, WATER, "water", True)]:
        r.set_trace(record=True)
        r.from_meshes([mesh])
        hr = hits(r.trace_paths(), [mesh], "ball", stride=8)   # (the blend of the reconstructor's normals; the inward copy by its flag)
        assert hr["blended"] > 100
        I = r.trace_paths().view(np.int32)
        print("winding: second segments that do not leave", int(((I[:, :, 1, TM.W_FLAGS] & (TM.F_ENTER | TM.F_INSIDE)) != TM.F_INSIDE).sum()))
        assert ((I[:, :, 0, TM.W_FLAGS] & TM.F_ENTER) != 0).all() and ((I[:, :, 1, TM.W_FLAGS] & (TM.F_ENTER | TM.F_INSIDE)) == TM.F_INSIDE).all()


# --- 5. plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_mode_off_after_on_gives_the_raster_frame_again_and_refuses_the_trace_calls(gpu):
    meshes = golden_meshes()
    r = renderer(size=96)
    raster = r.from_meshes(meshes).tobytes()
    raster_ids = r.ids().tobytes()
    r.set_trace()
    scene = [meshes[0] + ("water",), meshes[1], meshes[2]]
    traced = r.from_meshes(scene)
    assert traced.tobytes() != raster and r.trace_stats()["triangles"] == sum(len(m[1]) for m in meshes)
    assert r.from_meshes(meshes, download=False) is None and r.last_rgb().tobytes() != raster   # the traced frame stays on the device
    r.clear_trace()
    for call in (r.trace_stats, r.trace_bvh, r.trace_paths):
        with pytest.raises(RenderError) as e:
            call()
        assert e.value.code == -1
    assert r.from_meshes(scene).tobytes() == raster and r.ids().tobytes() == raster_ids   # materials are ignored by the raster frame
    r.set_trace()
    with pytest.raises(RenderError):
        r.trace_stats()   # no traced frame is held yet
    with pytest.raises(RenderError):
        r.set_trace(max_depth=0)
    with pytest.raises(RenderError):
        r.set_trace(ior=0.5)
    h = r._native(UNIT_BOX)
    assert r.lib.sph_render_mesh_material(h, 1, 0) == -1   # no mesh added
    with pytest.raises(ValueError):
        r.from_meshes([meshes[0] + ("glass",)])


def test_particle_frames_are_untouched_by_the_mode(gpu):
    x = np.random.default_rng(5).uniform(0.2, 0.8, (500, 3)).astype(np.float32)
    r = renderer(size=96)
    before = r.from_points(x).tobytes()
    r.set_trace()
    r.from_meshes(golden_scene())
    assert r.from_points(x).tobytes() == before
    with pytest.raises(RenderError):
        r.trace_stats()   # the frame held is a particle frame


def test_driver_and_command_line_tool_write_the_same_traced_png(gpu, tmp_path):
    import json
    import os

    from sph_project_amd import product as P
    from sph_project_amd import render_meshes, run_simulation
    from sph_project_amd.video import decode_png
    cfg = P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2))
    cfg["Configuration"].update(exportPly=True, outputInterval=3)
    f = tmp_path / "fluid.json"
    f.write_text(json.dumps(cfg))
    out, plain = tmp_path / "out", tmp_path / "plain"
    flags = ["--render_size", "160", "120", "--camera_position", "1.2", "0.8", "1.4", "--camera_lookat", "0.2", "0.2", "0.2"]
    common = ["--scene_file", str(f), "--max_steps", "4", "--reconstruct", "--render_meshes", "--mesh_smoothing_iters", "5",
              "--normals_smoothing_iters", "3"] + flags
    trace = ["--raytrace", "--trace_depth", "5", "--trace_absorb", "0.1"]
    run_simulation.main(common + ["--output_dir", str(out), "--video"] + trace)
    run_simulation.main(common + ["--output_dir", str(plain)])
    frames = sorted(d for d in os.listdir(out) if (out / d).is_dir())
    assert frames == ["000000", "000003"] and (out / "render.avi").stat().st_size > 1000
    want = {d: (out / d / "render.png").read_bytes() for d in frames}
    assert render_meshes.main(["--input_dir", str(out), "--scene_file", str(f), "--rendered_image_name", "again.png"] + flags + trace) == 2
    assert render_meshes.main(["--input_dir", str(out), "--scene_file", str(f), "--rendered_image_name", "device.png", "--png_device"]
                              + flags + trace) == 2
    for d in frames:
        assert (out / d / "again.png").read_bytes() == want[d], d
        img = decode_png(want[d])
        assert (decode_png((out / d / "device.png").read_bytes()) == img).all()
        raster = decode_png((plain / d / "render.png").read_bytes())
        assert img.shape == (120, 160, 3) and (img != raster).any(axis=2).sum() > 1000   # a floor, shadows and water: another picture


def test_driver_traces_a_scene_with_a_rigid_cube(gpu, tmp_path):
    import json
    import os

    from sph_project_amd import run_simulation
    from tests.test_hip_render_mesh import _scene_with_cube
    from sph_project_amd.video import decode_png
    f = tmp_path / "cube.json"
    f.write_text(json.dumps(_scene_with_cube()))
    out = tmp_path / "out"
    cam = ["--camera_position", "1.6", "1.0", "1.9", "--camera_lookat", "0.4", "0.3", "0.4"]
    run_simulation.main(["--scene_file", str(f), "--max_steps", "3", "--output_dir", str(out), "--render_meshes", "--raytrace", "--png_device",
                         "--render_size", "160", "120"] + cam)
    frames = sorted(d for d in os.listdir(out) if (out / d).is_dir())
    assert frames == ["000000", "000002"]
    for d in frames:
        px = decode_png((out / d / "render.png").read_bytes()).reshape(-1, 3).astype(np.int64)
        # the yellow cube (255, 200, 0) is diffuse: Lambert keeps its channel ratios; the floor is grey
        cube = (px[:, 0] >= 20) & (px[:, 2] == 0) & (np.abs(255 * px[:, 1] - 200 * px[:, 0]) <= 2 * 255)
        grey = (px[:, 0] >= 10) & (px[:, 0] == px[:, 1]) & (px[:, 1] == px[:, 2])
        assert cube.sum() > 15 and grey.sum() > 500, (d, int(cube.sum()), int(grey.sum()))
