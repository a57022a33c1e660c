"""GPU: mesh rendering (csrc/sph_render_mesh.hpp) against the float64 restatement in tests/render_mesh_model.py --
watertightness included --, exact ties, repeatability, the device path of a surface against its host copy, skipped triangles, the surface
object and the simulation left untouched, and the render.png frames of the driver and of render_meshes.py."""
import json
import os

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import meshgen
from sph_project_amd import product as P
from sph_project_amd.render import FrameRenderer, RenderError
from sph_project_amd.surface import SurfaceReconstructor
from tests import helpers as H
from tests import render_mesh_model as MM
from tests.test_render_host import decode_png

pytestmark = pytest.mark.gpu

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")
UNIT_BOX = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _model(name, scale, angle, axis, translation):
    m = meshgen.place(meshgen.load_obj(os.path.join(MODELS, name)), (scale,) * 3, angle, axis, translation)
    return np.asarray(m.vertices, np.float32), np.asarray(m.faces, np.int32)


def golden_meshes(smooth_icosphere=False):
    """icosphere, torus and cube of tests/golden/models inside the unit box, apart from each other"""
    iv, it = _model("icosphere.obj", 1.4, 0.3, (0, 1, 0), (0.32, 0.36, 0.62))
    tv, tt = _model("torus.obj", 0.8, 0.9, (1, 0, 1), (0.68, 0.62, 0.35))
    cv, ct = _model("cube.obj", 0.9, 0.5, (1, 2, 3), (0.72, 0.2, 0.75))
    n = None
    if smooth_icosphere:   # the analytic normals of a sphere about its centre
        c = iv.astype(np.float64).mean(axis=0)
        n = (iv - c) / np.linalg.norm(iv - c, axis=1, keepdims=True)
        n = n.astype(np.float32)
    return [(iv, it, n, (230, 60, 40)), (tv, tt, None, (60, 200, 90)), (cv, ct, None, (70, 90, 240))]


CLOSE_UP = dict(camera_position=(0.72, 0.27, 1.02), camera_lookat=(0.72, 0.2, 0.75), fov=70.0)


def _kw(model=False, close=False, size=None):
    """renderer (or model) keywords of the reference camera / the close-up"""
    kw = {}
    if size:
        kw.update(dict(W=size, H=size) if model else dict(width=size, height=size))
    if close:
        c = CLOSE_UP
        kw.update(dict(eye=c["camera_position"], target=c["camera_lookat"], fov=c["fov"]) if model else c)
    return kw


def compare(r, m, rgb, label):
    """The rule of tests/test_hip_render.py with the candidates added: ids equal on every non-ambiguous pixel and rgb within the model's
    bound there; on an ambiguous pixel the device's id is one of the model's candidates (an interior edge may show either triangle,
    never what lies behind); ambiguous pixels under 0.5 % of the covered ones."""
    ids = r.ids()
    amb = m["ambiguous"]
    covered = int((m["ids"] >= 0).sum())
    assert covered > 0, label
    print(f"{label}: covered {covered}, ambiguous {int(amb.sum())} ({100.0 * amb.sum() / covered:.3f} %), "
          f"ids differ on {int((ids != m['ids']).sum())} pixel(s)")
    bad = (ids != m["ids"]) & ~amb
    assert not bad.any(), (label, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    for j, i in np.argwhere(amb & (ids != m["ids"])):
        assert int(ids[j, i]) in m.candidates(int(j), int(i)), (label, int(j), int(i), int(ids[j, i]), m.candidates(int(j), int(i)))
    assert amb.sum() < 0.005 * covered, (label, int(amb.sum()), covered)
    agree = (ids == m["ids"]) & ~amb
    diff = np.abs(rgb.astype(np.int64) - m["rgb"].astype(np.int64)).max(axis=2)
    print(f"{label}: largest rgb difference {int(diff[agree].max())}, largest bound {int(m['rgb_tol'][agree].max())}, "
          f"bound of one step on {100.0 * (m['rgb_tol'][m['ids'] >= 0] == 1).mean():.2f} % of the covered pixels")
    over = agree & (diff > m["rgb_tol"])
    assert not over.any(), (label, int(over.sum()), np.argwhere(over)[:5].tolist())
    assert (m["rgb_tol"][m["ids"] >= 0] <= 2).mean() > 0.9, label
    st = r.mesh_stats()
    assert abs(st["covered_pixels"] - covered) <= amb.sum(), (label, st["covered_pixels"], covered)
    return st


def backdrop(z=0.02):
    v = np.array([[-0.5, -0.5, z], [1.5, -0.5, z], [1.5, 1.5, z], [-0.5, 1.5, z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), None, (255, 255, 255)


BLOCK_CAMERA = dict(camera_position=(0.36, 0.42, 0.95), camera_lookat=(0.3, 0.28, 0.3), fov=50.0)


def block_surface(fast):
    """the reconstructed, smoothed surface of a small dam-break block"""
    container, solver = H.build_product(P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2), translation=(0.2, 0.2, 0.2)), fast_math=int(fast))
    solver.prepare()
    solver.advance(3)
    recon = SurfaceReconstructor(container.dx, fast_math=fast)
    recon.set_postprocess(mesh_smoothing_iters=25, mesh_smoothing_weights=True, weights_normalization=13.0, normals_smoothing_iters=10)
    v, t, n = recon.from_container(container, 0)
    return container, solver, recon, (v, t, n)


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("label", ["reference_flat", "reference_smooth", "close_up"])
def test_golden_models_match_the_model(gpu, label, fast):
    meshes = golden_meshes(smooth_icosphere=label == "reference_smooth")
    close = label == "close_up"
    r = FrameRenderer(0.01, fast_math=fast, box=UNIT_BOX, **_kw(close=close, size=512 if close else None))
    rgb = r.from_meshes(meshes)
    m = MM.render(meshes, box=UNIT_BOX, **_kw(model=True, close=close, size=512 if close else None))
    st = compare(r, m, rgb, label)
    nt = sum(len(x[1]) for x in meshes)
    assert (st["meshes"], st["triangles"], st["vertices"]) == (3, nt, sum(len(x[0]) for x in meshes))
    assert st["skipped_nonfinite"] == st["skipped_degenerate"] == st["bad_index"] == 0
    assert set(np.unique(r.mesh_of(r.ids()))) >= {0, 1, 2} or close
    if close:   # the cube's faces fill the frame and cross the near plane
        assert st["large"] >= 2 and (m["depth"][m["ids"] >= 0].min() < 0.11)
    else:
        assert (m["ids"] <= -2).sum() > 300 and st["large"] == 0


@pytest.mark.parametrize("fast", [False, True])
def test_smoothed_surface_in_front_of_a_backdrop_matches_the_model(gpu, fast):
    container, solver, recon, (v, t, n) = block_surface(fast)
    meshes = [backdrop(), (v, t, n, (50, 100, 200))]
    r = FrameRenderer(0.01, fast_math=fast, **BLOCK_CAMERA)
    rgb = r.from_meshes(meshes)
    m = MM.render(meshes, eye=BLOCK_CAMERA["camera_position"], target=BLOCK_CAMERA["camera_lookat"], fov=BLOCK_CAMERA["fov"])
    compare(r, m, rgb, "surface")
    ids = r.ids()
    assert (ids >= 2).sum() > 50000 and (ids == -1).sum() == 0   # the backdrop fills the frame behind the surface


@pytest.mark.parametrize("fast", [False, True])
def test_exact_ties_go_to_the_smaller_global_index(gpu, fast):
    tri = np.array([[0.2, 0.2, 0.5], [0.8, 0.25, 0.4], [0.45, 0.8, 0.6]], np.float32)
    r = FrameRenderer(0.01, width=512, height=512, fast_math=fast, camera_position=(0.5, 0.5, 2.0), camera_lookat=(0.5, 0.5, 0.0), fov=40.0)
    # two coincident triangles of one mesh (the second with its corners turned and its winding reversed)
    r.from_meshes([(tri, np.array([[0, 1, 2], [2, 1, 0]], np.int32), None, (255, 0, 0))])
    ids = r.ids()
    assert set(np.unique(ids)) == {-1, 0} and (ids == 0).sum() > 10000
    # two meshes sharing a face: a tetrahedron on either side of it, mesh 1 with vertices of its own at the same positions
    # behind the face as seen from the camera, so that the shared face is what the camera sees of both
    apex_a, apex_b = np.float32([0.5, 0.45, -0.3]), np.float32([0.4, 0.5, -0.6])
    va, vb = np.concatenate([apex_a[None], tri]), np.concatenate([tri[::-1], apex_b[None]])
    ta = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 2, 3]], np.int32)   # the shared face is mesh 0's last triangle: global 3
    tb = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)   # ... and mesh 1's first: global 4
    rgb = r.from_meshes([(va, ta, None, (255, 0, 0)), (vb, tb, None, (0, 255, 0))])
    ids = r.ids()
    assert set(np.unique(ids)) == {-1, 3} and (rgb[ids == 3][:, 1] == 0).all() and (ids == 3).sum() > 10000
    rgb = r.from_meshes([(vb, tb, None, (0, 255, 0)), (va, ta, None, (255, 0, 0))])
    ids = r.ids()
    assert set(np.unique(ids)) == {-1, 0} and (rgb[ids == 0][:, 0] == 0).all()


def test_repeat_and_host_copy_of_a_surface_give_the_same_bytes(gpu):
    container, solver, recon, (v, t, n) = block_surface(False)
    r = FrameRenderer(0.01, box=UNIT_BOX, **BLOCK_CAMERA)
    a = r.from_meshes([(recon, (50, 100, 200))])
    ia = r.ids()
    st = r.mesh_stats()
    assert st["triangles"] == len(t) and st["vertices"] == len(v) and (ia >= 0).sum() > 50000
    b = r.from_meshes([(v, t, n, (50, 100, 200))])
    assert a.tobytes() == b.tobytes() and ia.tobytes() == r.ids().tobytes()
    c = r.from_meshes([(recon, (50, 100, 200))])
    assert a.tobytes() == c.tobytes() and ia.tobytes() == r.ids().tobytes()
    # the surface object is untouched: a second download equals the first
    v2, t2, n2 = recon._download()
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes() and n2.tobytes() == n.tobytes()
    # the same surface twice in one list: the first copy wins every pixel
    r.from_meshes([(recon, (50, 100, 200)), (recon, (200, 100, 50))])
    ids = r.ids()
    assert set(np.unique(r.mesh_of(ids)[ids >= 0])) == {0}


def test_skipped_triangles_are_counted_and_the_rest_of_the_frame_is_unchanged(gpu):
    meshes = golden_meshes()
    r = FrameRenderer(0.01, width=512, height=512, box=UNIT_BOX)
    clean = r.from_meshes(meshes).tobytes()
    clean_ids = r.ids()
    iv, it, _, col = meshes[0]
    # two non-finite, two with a repeated corner: appended at the end of the LAST mesh, so every other triangle keeps its global index
    tv, tt, _, tcol = meshes[2]
    last_v = np.concatenate([tv, np.float32([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5]])])
    nl = len(tv)
    extra = np.array([[0, 1, nl], [nl + 1, 2, 3], [4, 4, 5], [6, 7, 7]], np.int32)
    dirty = [meshes[0], meshes[1], (last_v, np.concatenate([tt, extra]), None, tcol)]
    assert r.from_meshes(dirty).tobytes() == clean
    assert r.ids().tobytes() == clean_ids.tobytes()
    st = r.mesh_stats()
    assert (st["skipped_nonfinite"], st["skipped_degenerate"], st["bad_index"]) == (2, 2, 0)
    # indices outside the mesh: skipped, counted, SPH_ERR_INVALID after the frame is drawn
    worse = [meshes[0], meshes[1], (tv, np.concatenate([tt, np.array([[0, 1, nl], [-1, 2, 3], [0, 1, 2 ** 30]], np.int32)]), None, tcol)]
    with pytest.raises(RenderError) as e:
        r.from_meshes(worse)
    assert e.value.code == -1
    assert r.mesh_stats()["bad_index"] == 3
    assert r.last_rgb().tobytes() == clean and r.ids().tobytes() == clean_ids.tobytes()
    # add / end without begin
    h = r._native(UNIT_BOX)
    assert r.lib.sph_render_mesh_end(h) == -1
    assert r.lib.sph_render_mesh_add(h, iv.ctypes.data, None, it.ctypes.data, len(iv), len(it), np.zeros(3, np.uint8).ctypes.data) == -1
    assert r.lib.sph_render_mesh_begin(h) == 0
    assert r.lib.sph_render_mesh_add(h, None, None, it.ctypes.data, 5, len(it), np.zeros(3, np.uint8).ctypes.data) == -1
    assert r.lib.sph_render_mesh_add(h, iv.ctypes.data, None, it.ctypes.data, -1, 0, np.zeros(3, np.uint8).ctypes.data) == -1
    # an empty list is a frame of background and box
    r.from_meshes([])
    assert set(np.unique(r.ids())) <= set(range(-13, 0)) and r.mesh_stats()["triangles"] == 0


def test_mesh_frames_leave_the_simulation_and_particle_frames_untouched(gpu):
    def run(render):
        container, solver = H.build_product(P.dam_break_scene(method="dfsph", end=(0.2, 0.2, 0.2), dt=6e-4))
        solver.prepare()
        r = FrameRenderer(container.dx, width=256, height=256) if render else None
        recon = SurfaceReconstructor(container.dx) if render else None
        for k in range(6):
            solver.step()
            if r is not None and k % 2 == 0:
                recon.from_container(container, 0)
                r.from_meshes([(recon, (50, 100, 200))])
                r.ids()
        solver.advance(5)
        eng = container.engine
        eng.synchronize()
        return (eng.download(L.F_POSITION), eng.download(L.F_VELOCITY), eng.download(L.F_PARTICLE_ID), solver.stats()), container, r
    a, _, _ = run(False)
    b, container, r = run(True)
    for u, w in zip(a[:3], b[:3]):
        assert u.tobytes() == w.tobytes()
    assert a[3] == b[3]
    # a particle frame after a mesh frame on the same renderer equals one from a fresh renderer
    after = r.from_container(container)
    after_ids = r.ids()
    fresh = FrameRenderer(container.dx, width=256, height=256)
    assert fresh.from_container(container).tobytes() == after.tobytes() and fresh.ids().tobytes() == after_ids.tobytes()
    assert r.stats()["drawn"] > 0


def _scene_with_cube():
    cfg = P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2), translation=(0.15, 0.1, 0.15))
    cfg["Configuration"].update(exportPly=True, outputInterval=2)
    cfg["RigidBodies"] = [{
        "objectId": 1, "geometryFile": os.path.join(MODELS, "cube.obj"), "translation": [0.6, 0.5, 0.6], "rotationAxis": [0, 0, 1],
        "rotationAngle": 30, "scale": [0.8, 0.8, 0.8], "velocity": [0.0, 0.0, 0.0], "density": 900.0, "color": [255, 200, 0],
        "isDynamic": True, "entryTime": -1.0}]
    return cfg


def test_driver_writes_render_png_with_both_objects(gpu, tmp_path):
    from sph_project_amd import run_simulation
    f = tmp_path / "cube.json"
    f.write_text(json.dumps(_scene_with_cube()))
    out = tmp_path / "out"
    cam = ["--camera_position", "1.6", "1.0", "1.9", "--camera_lookat", "0.4", "0.3", "0.4"]
    run_simulation.main(["--scene_file", str(f), "--max_steps", "5", "--output_dir", str(out), "--render_meshes", "--render_size", "320", "240"] + cam)
    frames = sorted(d for d in os.listdir(out) if (out / d).is_dir())
    assert frames == ["000000", "000002", "000004"]
    for d in frames:
        assert "render.png" in os.listdir(out / d)
        img = decode_png((out / d / "render.png").read_bytes())
        assert img.shape == (240, 320, 3)
        px = img.reshape(-1, 3).astype(np.int64)
        # Lambert shading keeps a colour's channel ratios (up to rounding): blue-ish fluid (50, 100, 200), yellow cube (255, 200, 0)
        # (down to the ambient term alone, 0.1 of the colour).  The 0.2 block, about 2.2 from the eye, spans about
        # 0.2 / (2 * 2.2 * tan 35 deg) * 240 = 16 rows: one face is some 250 pixels, so 100 of its colour must be there
        fluid = (px[:, 2] >= 15) & (np.abs(px[:, 2] - 4 * px[:, 0]) <= 4) & (np.abs(px[:, 2] - 2 * px[:, 1]) <= 3)
        cube = (px[:, 0] >= 20) & (px[:, 2] == 0) & (np.abs(255 * px[:, 1] - 200 * px[:, 0]) <= 2 * 255)
        assert fluid.sum() > 100 and cube.sum() > 100, (d, int(fluid.sum()), int(cube.sum()))
    # without the flag nothing of it is written
    out2 = tmp_path / "plain"
    run_simulation.main(["--scene_file", str(f), "--max_steps", "5", "--output_dir", str(out2)])
    assert all("render.png" not in os.listdir(out2 / d) for d in os.listdir(out2))


def test_cli_reproduces_the_drivers_png_from_the_written_objs(gpu, tmp_path):
    from sph_project_amd import render_meshes, run_simulation
    cfg = P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2))
    cfg["Configuration"].update(exportPly=True, outputInterval=3)
    f = tmp_path / "fluid.json"
    f.write_text(json.dumps(cfg))
    out = tmp_path / "out"
    flags = ["--render_size", "400", "300", "--camera_position", "1.2", "0.8", "1.4", "--camera_lookat", "0.2", "0.2", "0.2"]
    run_simulation.main(["--scene_file", str(f), "--max_steps", "4", "--output_dir", str(out), "--reconstruct", "--render_meshes",
                         "--mesh_smoothing_iters", "5", "--mesh_smoothing_weights", "--normals_smoothing_iters", "3"] + flags)
    frames = sorted(os.listdir(out))
    assert frames == ["000000", "000003"]
    want = {d: (out / d / "render.png").read_bytes() for d in frames}
    assert render_meshes.main(["--input_dir", str(out), "--scene_file", str(f), "--rendered_image_name", "again.png"] + flags) == 2
    for d in frames:
        assert (out / d / "again.png").read_bytes() == want[d], d
        img = decode_png(want[d])
        assert (img.reshape(-1, 3)[:, 2] > 60).sum() > 500   # the fluid is in the picture


def _sphere(radius, centre, scale=1.0):
    """the golden icosphere with analytic normals"""
    v, t = _model("icosphere.obj", scale, 0.0, (0, 1, 0), centre)
    c = v.astype(np.float64).mean(axis=0)
    n = ((v - c) / np.linalg.norm(v - c, axis=1, keepdims=True)).astype(np.float32)
    return v, t, n


def test_normals_survive_flat_meshes_between_smooth_ones_and_a_reused_renderer(gpu):
    """The normals buffer holds a slot per vertex of the frame but grows for smooth meshes only: a flat mesh larger than everything
    before it, between two smooth ones, and a second frame whose flat prefix is larger than the previous frame's normals, must draw what a
    fresh renderer draws and what the model says."""
    tv, tt = _model("torus.obj", 0.8, 0.9, (1, 0, 1), (0.5, 0.5, 0.5))   # 576 vertices, flat
    a, b = _sphere(0.2, (0.2, 0.3, 0.6)), _sphere(0.2, (0.8, 0.7, 0.4))  # 42 vertices each, smooth
    frames = [[(a[0], a[1], a[2], (230, 60, 40))],                                                              # small normals buffer
              [(a[0], a[1], a[2], (230, 60, 40)), (tv, tt, None, (60, 200, 90)), (b[0], b[1], b[2], (70, 90, 240))],
              [(tv, tt, None, (60, 200, 90)), (tv + np.float32([0, 0, -0.3]), tt, None, (9, 200, 90)), (b[0], b[1], b[2], (70, 90, 240))]]
    kw = dict(width=384, height=384, camera_position=(0.5, 0.6, 2.2), camera_lookat=(0.5, 0.5, 0.5), fov=40.0)
    reused = FrameRenderer(0.01, **kw)
    for k, meshes in enumerate(frames):
        got = reused.from_meshes(meshes)
        got_ids = reused.ids()
        fresh = FrameRenderer(0.01, **kw)
        assert fresh.from_meshes(meshes).tobytes() == got.tobytes() and fresh.ids().tobytes() == got_ids.tobytes(), k
        m = MM.render(meshes, W=384, H=384, eye=kw["camera_position"], target=kw["camera_lookat"], fov=40.0)
        compare(reused, m, got, f"growth frame {k}")
        seen = set(np.unique(reused.mesh_of(got_ids)[got_ids >= 0]))
        assert seen == set(range(len(meshes))), (k, seen)


def test_mesh_queries_need_a_mesh_frame(gpu):
    r = FrameRenderer(0.05, width=64, height=64)
    for call in (r.mesh_stats, lambda: r.mesh_of(np.zeros(3, np.int64))):
        with pytest.raises(RenderError):
            call()
    r.from_points(np.float32([[0, 0, 0]]))
    with pytest.raises(RenderError):
        r.mesh_stats()
    with pytest.raises(RenderError):
        r.mesh_of(r.ids())
    r.from_meshes([])
    assert r.mesh_stats()["triangles"] == 0
    with pytest.raises(RenderError):
        r.stats()


def test_driver_draws_the_rigid_body_where_it_is_now(gpu, tmp_path):
    """A cube thrown downwards at 2 m/s: after 100 steps of 4e-4 s it has fallen 0.08 m and more, about 0.08 / (2 * 1.9 * tan 35 deg)
    * 240 = 7 rows at the camera below; its pixels in render.png must have moved down by 3 rows at least."""
    from sph_project_amd import run_simulation
    cfg = _scene_with_cube()
    cfg["Configuration"].update(exportPly=False, outputInterval=100)
    cfg["RigidBodies"][0].update(velocity=[0.0, -2.0, 0.0], translation=[0.6, 0.7, 0.6])
    f = tmp_path / "fall.json"
    f.write_text(json.dumps(cfg))
    out = tmp_path / "out"
    run_simulation.main(["--scene_file", str(f), "--max_steps", "101", "--output_dir", str(out), "--render_meshes", "--render_size", "320", "240",
                         "--camera_position", "1.6", "1.0", "1.9", "--camera_lookat", "0.4", "0.3", "0.4"])
    assert sorted(os.listdir(out)) == ["000000", "000100"]
    rows = []
    for d in ("000000", "000100"):
        assert os.listdir(out / d) == ["render.png"]   # the flag alone: no PLY, no OBJ
        px = decode_png((out / d / "render.png").read_bytes()).astype(np.int64)
        cube = (px[..., 0] >= 20) & (px[..., 2] == 0) & (np.abs(255 * px[..., 1] - 200 * px[..., 0]) <= 2 * 255)
        assert cube.sum() > 100, (d, int(cube.sum()))
        rows.append(np.nonzero(cube)[0].mean())
    print("cube rows", rows)
    assert rows[1] - rows[0] >= 3.0, rows


def test_c2_full_size_from_rest_matches_the_model_on_256x256(gpu):
    """C2 (1,231,200 particles) from rest, reference settings 25 / on / 13 / 10, reference camera, 256 x 256, against the whole float64
    model (its run time is printed).  The triangles (edge about 0.005) are several times smaller than a pixel here (0.028 at the
    block's distance), so by the model's derived bounds most covered pixels have more than one triangle within rounding of the pixel
    centre: the share of ambiguous pixels is printed, not capped -- the 0.5 % cap belongs to the cases whose placement the tests choose.
    What is asserted on EVERY pixel: an unambiguous pixel has the model's id and its colour within the model's bound; an ambiguous
    pixel shows one of the model's candidates for it, i.e. a triangle within the derived tolerance of that pixel centre and of the front
    depth -- never the background where a triangle surely covers the pixel, never a triangle where none can, never the block's far side.
    Measured on an MI355X (strict build): 2,384,632 triangles, the model takes 34 s; 11,387 covered pixels (device 11,388), 1,359 of them
    ambiguous (11.9 %) with a median of 3 candidates (67 at most); ids differ on 65 pixels, all ambiguous; on the 64,177 unambiguous
    pixels the largest colour difference is one 8-bit step."""
    import time
    container, solver = H.build_product(P.c2_scene())
    solver.prepare()
    recon = SurfaceReconstructor(container.dx)
    recon.set_postprocess(mesh_smoothing_iters=25, mesh_smoothing_weights=True, weights_normalization=13.0, normals_smoothing_iters=10)
    v, t, n = recon.from_container(container, 0)
    assert recon.stats()["particles"] == 1231200 and len(t) > 2000000
    dom = np.asarray(container.domain_end, np.float64)
    r = FrameRenderer(container.dx, width=256, height=256, box=(np.zeros(3), dom))
    rgb = r.from_meshes([(recon, (50, 100, 200))])
    ids = r.ids()
    st = r.mesh_stats()
    assert st["triangles"] == len(t) and st["skipped_nonfinite"] == st["skipped_degenerate"] == st["bad_index"] == 0
    t0 = time.perf_counter()
    m = MM.render([(v, t, n, (50, 100, 200))], W=256, H=256, box=(np.zeros(3), dom))
    secs = time.perf_counter() - t0
    amb = m["ambiguous"]
    covered = int((m["ids"] >= 0).sum())
    print(f"c2: {len(t)} triangles, model {secs:.1f} s, covered {covered}, device covered {st['covered_pixels']}, ambiguous {int(amb.sum())} "
          f"({100.0 * amb.sum() / max(covered, 1):.2f} % of covered), ids differ on {int((ids != m['ids']).sum())} pixel(s)")
    assert covered > 5000
    # measured 11.9 %: sub-pixel triangles make many pixels ambiguous by the derived bounds, but a share beyond 15 % would mean the
    # bounds (or the mesh) have drifted
    assert amb.sum() < 0.15 * covered, (int(amb.sum()), covered)
    bad = (ids != m["ids"]) & ~amb
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    sizes = []
    for j, i in np.argwhere(amb):
        c = m.candidates(int(j), int(i))
        sizes.append(len(c))
        assert int(ids[j, i]) in c, (int(j), int(i), int(ids[j, i]), sorted(c)[:8])
    print(f"c2: candidates per ambiguous pixel: median {int(np.median(sizes)) if sizes else 0}, largest {max(sizes) if sizes else 0}")
    agree = (ids == m["ids"]) & ~amb
    diff = np.abs(rgb.astype(np.int64) - m["rgb"].astype(np.int64)).max(axis=2)
    over = agree & (diff > m["rgb_tol"])
    print(f"c2: unambiguous pixels {int(agree.sum())}, largest rgb difference there {int(diff[agree].max())}")
    assert not over.any(), (int(over.sum()), np.argwhere(over)[:5].tolist())
    # where the model sees a triangle in front, the device almost always does too (the exceptions are ambiguous pixels with the
    # background among their candidates, checked above)
    assert (ids[m["ids"] >= 0] != -1).mean() > 0.99


def test_two_fluid_objects_driver_with_both_flags_equals_the_cli_over_the_objs(gpu, tmp_path):
    """Two fluid blocks of different colours, --reconstruct and --render_meshes together: one reconstructor serves the OBJ export and the
    mesh frame in turn, and every object must appear with its own surface in its own colour -- the PNG equals what render_meshes.py draws
    from the written OBJ files, and both colours are in it."""
    from sph_project_amd import render_meshes, run_simulation
    cfg = P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2), translation=(0.1, 0.1, 0.1))
    second = dict(cfg["FluidBlocks"][0])
    second.update(objectId=1, translation=[0.6, 0.1, 0.5], end=[0.15, 0.3, 0.15], color=[220, 60, 30])
    cfg["FluidBlocks"].append(second)
    cfg["Configuration"].update(exportPly=True, outputInterval=3)
    f = tmp_path / "two.json"
    f.write_text(json.dumps(cfg))
    out = tmp_path / "out"
    flags = ["--render_size", "400", "300", "--camera_position", "1.4", "0.9", "1.6", "--camera_lookat", "0.4", "0.2", "0.4"]
    run_simulation.main(["--scene_file", str(f), "--max_steps", "4", "--output_dir", str(out), "--reconstruct", "--render_meshes",
                         "--mesh_smoothing_iters", "5", "--normals_smoothing_iters", "3"] + flags)
    frames = sorted(os.listdir(out))
    assert frames == ["000000", "000003"]
    for d in frames:
        assert {"particle_object_0.obj", "particle_object_1.obj", "render.png"} <= set(os.listdir(out / d))
    assert render_meshes.main(["--input_dir", str(out), "--scene_file", str(f), "--rendered_image_name", "again.png"] + flags) == 2
    for d in frames:
        assert (out / d / "again.png").read_bytes() == (out / d / "render.png").read_bytes(), d
        px = decode_png((out / d / "render.png").read_bytes()).reshape(-1, 3).astype(np.int64)
        blue = (px[:, 2] >= 15) & (np.abs(px[:, 2] - 4 * px[:, 0]) <= 4) & (np.abs(px[:, 2] - 2 * px[:, 1]) <= 3)      # (50, 100, 200)
        red = (px[:, 0] >= 15) & (np.abs(60 * px[:, 0] - 220 * px[:, 1]) <= 2 * 220) & (np.abs(30 * px[:, 0] - 220 * px[:, 2]) <= 2 * 220)  # (220, 60, 30)
        assert blue.sum() > 100 and red.sum() > 100, (d, int(blue.sum()), int(red.sum()))
