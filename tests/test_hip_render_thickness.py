"""GPU: the thickness mode of the surface frames (csrc/sph_render_thickness.hpp) against tests/render_thickness_model.py --
the opaque layer against an ordinary draw of the opaque particles, the summed and the smoothed plane exactly, the composite within the
model's bound, the two identities, the same bytes and planes from both builds / a repeat / another particle order, the handle path
against the points path with the rigid body showing through, the refusals, and the driver's flags."""
import os

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd.render import FrameRenderer, RenderError, SURFACE_SENTINEL
from sph_project_amd.video import decode_png as decode_any_png
from tests import helpers as H
from tests import render_model as RM
from tests import render_surface_model as SM
from tests import render_thickness_model as TM
from tests.test_hip_render_surface import MODELS, _driver_scene, _random_particles, _sheet
from tests.test_render_host import decode_png
from tests.test_video_host import avi_frames

pytestmark = pytest.mark.gpu


def _reference():
    """(a) 3000 random particles in the reference view, every other one a surface particle"""
    x, c, ids = _random_particles(3000, 0.0, 2.0, 1)
    return x, c, ids, np.arange(len(x)) % 2 == 0


def _sheet_all():
    """(b) the two-layer lattice sheet of the surface tests (seen head-on, as there: that is what puts it on all four borders)"""
    return _sheet(0)


def _large():
    """(c) the reference view at radius 0.12.  A surface sphere 0.25 in front of the eye fills half the frame (the large path) with 400
    small surface particles behind it; an opaque sphere intersects it, so the opaque depth falls inside its chords; off to one corner a
    surface sphere lies wholly behind an opaque one; towards another a surface sphere holds the near plane between its two hits on every
    ray that meets it (the tangent from the eye is shorter than z_near)."""
    E, f, s, u, tx, ty = RM.camera(**RM.REFERENCE_CAMERA, W=256, H=256)
    at = lambda depth, X=0.0, Y=0.0: E + depth * (f + X * s + Y * u)
    rng = np.random.default_rng(11)
    cloud = np.stack([at(d, X, Y) for d, X, Y in zip(rng.uniform(1.0, 3.0, 400), rng.uniform(-0.6, 0.6, 400), rng.uniform(-0.6, 0.6, 400))])
    special = np.stack([at(0.25), at(0.35, 0.12, 0.05), at(1.0, 0.55, 0.55), at(1.5, 0.55, 0.55), at(0.11, -0.55, -0.55)])
    x = np.concatenate([cloud, special]).astype(np.float32)
    c = rng.integers(0, 256, (len(x), 3), dtype=np.uint8)
    ids = np.concatenate([rng.permutation(np.arange(4000, dtype=np.uint32))[:400], [5000, 5001, 5002, 5003, 5004]]).astype(np.uint32)
    surf = np.ones(len(x), bool)
    surf[[401, 402]] = False   # the intersecting sphere and the one in front of 5003
    return x, c, ids, surf


SCENES = {
    # label: (particles, radius, renderer keywords)
    "reference": (_reference, 0.02, dict(box=((0, 0, 0), (2, 2, 2)))),
    "sheet": (_sheet_all, 0.06, dict(camera_position=(0.0, 0.0, 2.0), camera_lookat=(0.0, 0.0, 0.0), fov=60.0)),
    "large": (_large, 0.12, dict(box=((0, 0, 0), (2, 2, 2)))),
}
CASES = [("reference", 97, 61, 12), ("reference", 128, 128, 12), ("sheet", 128, 128, 12), ("large", 256, 256, 16)]   # scene, W, H, rmax
CASE_IDS = [f"{c[0]}-{c[1]}x{c[2]}" for c in CASES]
_cache = {}


def _camera(rkw):
    k = dict(fov=rkw.get("fov", 70.0))
    if "camera_position" in rkw:
        k.update(eye=rkw["camera_position"], target=rkw["camera_lookat"])
    return k


def _case(case, fast=False):
    """The frame of a case drawn once per build with the mode on (thickness iterations 0), the device's planes and the model's raw plane
    on the device's opaque keys, shared by the tests."""
    if (case, fast) in _cache:
        return _cache[(case, fast)]
    scene, W, Hh, rmax = case
    make, radius, rkw = SCENES[scene]
    x, c, ids, surf = make()
    r = FrameRenderer(radius, width=W, height=Hh, fast_math=fast, **rkw)
    r.set_surface(rmax=rmax)
    r.set_thickness(iterations=0)
    plain = r.from_points(x, c, ids, surface=surf)
    stats = r.stats()
    won = r.ids()
    key, _ = r.layer()
    okey, orgb = r.surface_opaque()
    first = r.surface()
    raw, q, tst = r.surface_thickness(raw=True), r.surface_depth(), r.thickness_stats()
    order = np.argsort(ids)
    at = np.searchsorted(ids[order], np.where(won >= 0, won, ids[order][0]).astype(np.uint32))
    who = order[np.minimum(at, len(ids) - 1)]
    flag = (won >= 0) & surf[who]
    base = np.where(flag[..., None], c[who], 0)
    cam = _camera(rkw)
    m_raw, m_st = TM.splat(x[surf], okey, radius, **cam)
    _, _, rnum, _ = SM.constants(radius, Hh, rkw.get("fov", 70.0))
    out = dict(r=r, x=x, c=c, ids=ids, surf=surf, plain=plain, won=won, key=key, okey=okey, orgb=orgb, first=first, raw=raw, q=q, tst=tst,
               flag=flag, base=base, cam=cam, m_raw=m_raw, m_st=m_st, rnum=rnum, rmax=rmax, radius=radius, rkw=rkw, W=W, H=Hh, stats=stats)
    _cache[(case, fast)] = out
    return out


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=[CASE_IDS[0], CASE_IDS[1], CASE_IDS[3]])
def test_opaque_layer_is_the_ordinary_frame_of_the_opaque_particles(gpu, case, fast):
    k = _case(case, fast)
    o = FrameRenderer(k["radius"], width=k["W"], height=k["H"], fast_math=fast, **k["rkw"])   # the mode off, the same parameters
    keep = ~k["surf"]
    frame = o.from_points(k["x"][keep], k["c"][keep], k["ids"][keep])
    key, rgb = o.layer()
    assert (key != np.uint64(0xFFFFFFFFFFFFFFFF)).sum() > 100 and ((key & np.uint64(0xFFFFFFFF)) >= np.uint64(RM.LINE_ID0)).sum() > 50
    assert np.array_equal(k["okey"], key) and np.array_equal(k["orgb"], rgb) and np.array_equal(rgb, frame)
    assert np.array_equal(k["r"].layer()[0], k["key"]) and np.array_equal(k["r"].ids(), k["won"])   # the frame's own planes are untouched
    o.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_raw_thickness_and_counters_equal_the_model(gpu, case):
    k = _case(case)
    flag, raw, tst = k["flag"], k["raw"], k["tst"]
    assert flag.sum() > 50
    diff = raw != k["m_raw"]
    print(case, "raw differences", int(diff.sum()), "adds", tst["adds"], "clipped", tst["clipped"], "removed", tst["removed"],
          "max", int(raw.max()), "empty", tst["empty_pixels"])
    assert not diff.any(), (case, int(diff.sum()), np.argwhere(diff)[:5].tolist(), raw[diff][:5], k["m_raw"][diff][:5])
    assert {a: tst[a] for a in ("adds", "clipped", "removed")} == k["m_st"], (tst, k["m_st"])
    assert tst["adds"] > flag.sum() and not raw[~flag].any()   # behind an opaque winner nothing is left of any chord
    assert tst["empty_pixels"] == int((raw[flag] == 0).sum()) and tst["max_thickness"] == int(raw[flag].max())
    if case[0] == "sheet":
        assert flag[0].all() and flag[-1].all() and flag[:, 0].all() and flag[:, -1].all()
        assert tst["clipped"] == 0 and tst["removed"] == 0
    if case[0] == "reference":
        assert tst["removed"] > 0 and (k["won"] <= -2).sum() > 50   # (spheres below a pixel: hidden ones, none cut inside its chord)
    if case[0] == "large":
        x, surf = k["x"], k["surf"]
        assert k["stats"]["large"] >= 3 and (k["won"] == 5000).mean() > 0.25
        nothing = np.full(raw.shape, 0xFFFFFFFFFFFFFFFF, np.uint64)
        assert TM.splat(x[404:405], nothing, k["radius"], **k["cam"])[1] == dict(adds=0, clipped=0, removed=0)   # across the near plane
        hidden = TM.splat(x[403:404], k["okey"], k["radius"], **k["cam"])[1]
        assert hidden["adds"] == 0 and hidden["removed"] > 50                                                    # wholly behind 5002
        free = TM.splat(x[400:401], nothing, k["radius"], **k["cam"])[0]
        cutp = TM.splat(x[400:401], k["okey"], k["radius"], **k["cam"])[0]
        inside = (cutp > 0) & (cutp < free)
        assert inside.sum() > 500, int(inside.sum())                                                             # the clip inside a chord


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_smoothed_thickness_equals_the_model_on_the_device_planes(gpu, case):
    k = _case(case)
    r, flag = k["r"], k["flag"]
    for n in (0, 1, 3):
        r.set_thickness(iterations=n)
        r.surface()
        T, q = r.surface_thickness(), r.surface_depth()
        assert np.array_equal(q, k["q"]) and np.array_equal(r.surface_thickness(raw=True), k["raw"])   # a repeat starts from the same planes
        want, visited = TM.smooth(k["raw"], q, n, k["rnum"], k["rmax"])
        diff = T != want
        print(case, n, "smoothed differences", int(diff.sum()))
        assert not diff.any(), (case, n, int(diff.sum()), np.argwhere(diff)[:5].tolist())
        st = r.thickness_stats()
        assert st["iterations"] == n and st["taps_visited"] == visited and st["max_thickness"] == int(T.max(initial=0)), (st, visited)
        assert not T[~flag].any() and ((q == SURFACE_SENTINEL) == ~flag).all()
    if n and k["rmax"] == 16:
        R = SM.window(k["q"].astype(np.uint64), k["rnum"], 16)[0]
        assert (R[flag] > 12).any()   # the case that reaches beyond the default rmax


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_colour_is_within_the_models_bound(gpu, case):
    k = _case(case)
    r, flag = k["r"], k["flag"]
    worst = 0
    for kw in (dict(TM.DEFAULTS), dict(absorb=0.5, scatter=0.0, iterations=1), dict(absorb=0.0, scatter=0.2, iterations=0)):
        r.set_thickness(**kw)
        rgb = r.surface()
        T, q = r.surface_thickness(), r.surface_depth()
        m_rgb, tol = TM.composite(q, T, k["base"], flag, k["orgb"], k["plain"], k["radius"], absorb=kw["absorb"], scatter=kw["scatter"], **k["cam"])
        d = np.abs(rgb.astype(np.int64) - m_rgb.astype(np.int64))
        print(case, kw, "max colour difference", int(d.max()), "largest bound", int(tol.max()), "share of bound 1:", float((tol[flag] == 1).mean()))
        over = d > tol
        assert not over.any(), (case, kw, int(over.sum()), int(d.max()), np.argwhere(over)[:5].tolist())
        assert (tol[flag] == 1).mean() > 0.5
        assert np.array_equal(rgb[~flag], k["plain"][~flag])
        worst = max(worst, int(d.max()))
    assert worst <= 2


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_two_identities_are_exact(gpu, case, fast):
    k = _case(case, fast)
    r, flag = k["r"], k["flag"]
    skw = dict(rmax=k["rmax"])
    r.clear_thickness()
    r.from_points(k["x"], k["c"], k["ids"], surface=k["surf"])
    opaque_surface = r.surface()   # the thickness mode off
    r.set_thickness(scatter=1e6)
    r.from_points(k["x"], k["c"], k["ids"], surface=k["surf"])
    assert r.surface().tobytes() == opaque_surface.tobytes()
    r.set_surface(spec=0.0, **skw)
    r.set_thickness(absorb=0.0, scatter=0.0)
    r.from_points(k["x"], k["c"], k["ids"], surface=k["surf"])
    clear = r.surface()
    assert np.array_equal(clear[flag], k["orgb"][flag]) and np.array_equal(clear[~flag], k["plain"][~flag])
    r.set_surface(**skw)
    r.set_thickness(iterations=0)


def test_both_builds_a_repeat_and_another_order_give_the_same_bytes_and_planes(gpu):
    """The frame's bytes, both thickness planes and the opaque colours are the same everywhere.  Two planes are by definition the build's
    own and are compared within each build: the opaque KEY plane is the ordinary frame's of the build in use (its depths may differ in
    the last bits between the builds, as layer()'s do), and the depth plane Q is section 24's quantisation of that build's key plane (on
    the large scene the truncation falls on the other side in a few pixels of the fast build; the count is printed)."""
    for case in (CASES[0], CASES[3]):
        a, b = _case(case, False), _case(case, True)
        out, own = [], []
        for k in (a, b):
            r = k["r"]
            r.set_thickness()
            def planes():
                return (r.surface().tobytes(), r.surface_thickness().tobytes(), r.surface_thickness(raw=True).tobytes(),
                        r.surface_opaque()[1].tobytes())
            def build_planes():
                return (r.surface_opaque()[0].tobytes(), r.surface_depth().tobytes())
            r.from_points(k["x"], k["c"], k["ids"], surface=k["surf"])
            out.append(planes())
            out.append(planes())   # once more on the same frame
            own.append([build_planes()])
            perm = np.random.default_rng(9).permutation(len(k["x"]))
            r.from_points(k["x"][perm], k["c"][perm], k["ids"][perm], surface=k["surf"][perm])
            out.append(planes())
            own[-1].append(build_planes())
            r.set_thickness(iterations=0)
        print(case, "depth plane pixels that differ between the builds:",
              int((np.frombuffer(own[0][0][1], np.uint32) != np.frombuffer(own[1][0][1], np.uint32)).sum()))
        assert all(o == out[0] for o in out), (case, [[u == w for u, w in zip(o, out[0])] for o in out])
        assert all(o[0] == o[1] for o in own), case


def _mixed_scene():
    """the mixed scene of the surface tests with the cube moved behind the fluid block as the camera below sees it: partly covered"""
    cfg = P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2), translation=(0.15, 0.1, 0.15), add_domain_box=False)
    cfg["RigidBodies"] = [{
        "objectId": 1, "geometryFile": os.path.join(MODELS, "cube.obj"), "translation": [0.3, 0.25, 0.55], "rotationAxis": [0, 0, 1],
        "rotationAngle": 30, "scale": [0.8, 0.8, 0.8], "velocity": [0.0, 0.0, 0.0], "density": 900.0, "color": [255, 200, 0],
        "isDynamic": True, "entryTime": -1.0}]
    return cfg


CAM = dict(width=256, height=192, camera_position=(0.25, 0.3, -0.5), camera_lookat=(0.28, 0.22, 0.5))


@pytest.mark.parametrize("fast", [False, True])
def test_handle_path_equals_points_path_and_the_cube_shows_through(gpu, fast):
    container, solver = H.build_product(_mixed_scene(), fast_math=int(fast))
    solver.prepare()
    for _ in range(3):
        solver.step()
    eng = container.engine
    dom = np.asarray(container.domain_end, np.float64)
    r = FrameRenderer(container.dx, box=((0, 0, 0), dom), fast_math=fast, **CAM)
    plain = r.from_container(container)
    r.set_surface()
    r.from_container(container)
    ids, key = r.ids(), r.layer()[0]
    solid = r.surface()   # the opaque surface
    r.set_thickness()
    assert r.from_container(container).tobytes() == plain.tobytes()   # the mode leaves the particle frame alone
    a = r.surface()
    planes = (r.surface_thickness(), r.surface_thickness(raw=True), r.surface_depth()) + r.surface_opaque()
    assert r.ids().tobytes() == ids.tobytes() and r.layer()[0].tobytes() == key.tobytes()
    pid = eng.download(L.F_PARTICLE_ID)
    mat = eng.download(L.F_MATERIAL)
    flag = np.isin(ids, pid[mat == 1]) & (ids >= 0)
    assert flag.sum() > 300 and ((ids >= 0) & ~flag).sum() > 300 and (ids <= -2).sum() > 100
    assert np.array_equal(a[~flag], plain[~flag])   # every flag-0 pixel keeps its bytes
    okey = planes[3]
    behind = np.isin((okey & np.uint64(0xFFFFFFFF)).astype(np.int64), pid[mat != 1]) & (okey != np.uint64(0xFFFFFFFFFFFFFFFF))
    through = flag & behind & (a != solid).any(axis=2)
    print("surface pixels", int(flag.sum()), "with the cube behind", int((flag & behind).sum()), "changed", int(through.sum()))
    assert through.sum() > 50   # the rigid body shows through the fluid
    st = r.thickness_stats()
    assert st["adds"] > flag.sum() and st["clipped"] == 0 and st["removed"] == 0   # (the cube lies behind every chord in front of it)
    # the same visible particles through the points path, the fluid ones flagged
    x = eng.download(L.F_POSITION)
    col = eng.download(L.F_COLOR).astype(np.uint8)
    assert r.from_points(x, col, pid.astype(np.uint32), surface=mat == 1).tobytes() == plain.tobytes()
    assert r.surface().tobytes() == a.tobytes()
    again = (r.surface_thickness(), r.surface_thickness(raw=True), r.surface_depth()) + r.surface_opaque()
    assert all(u.tobytes() == w.tobytes() for u, w in zip(planes, again))
    r.clear_thickness()
    r.from_container(container)
    assert r.surface().tobytes() == solid.tobytes()
    r.clear_surface()
    assert r.from_container(container).tobytes() == plain.tobytes()


def test_the_thickness_mode_leaves_the_simulation_bit_identical(gpu):
    def run(render):
        container, solver = H.build_product(_mixed_scene())
        solver.prepare()
        r = FrameRenderer(container.dx, width=128, height=128) if render else None
        if r is not None:
            r.set_surface()
            r.set_thickness()
        for k in range(6):
            solver.step()
            if r is not None and k % 2 == 0:
                r.from_container(container)
                r.surface()
                r.surface_thickness()
        solver.advance(5)
        eng = container.engine
        eng.synchronize()
        return eng.download(L.F_POSITION), eng.download(L.F_VELOCITY), eng.download(L.F_PARTICLE_ID), solver.stats()
    a, b = run(False), run(True)
    for u, w in zip(a[:3], b[:3]):
        assert u.tobytes() == w.tobytes()
    assert a[3] == b[3]


def test_refusals_are_errors_with_messages(gpu):
    x, c, ids = _random_particles(200, 0.0, 2.0, 7)
    r = FrameRenderer(0.05, width=64, height=48)
    with pytest.raises(RenderError, match="surface mode is off") as e:
        r.set_thickness()
    assert e.value.code == L.ERR_INVALID
    r.set_surface()
    for bad, word in ((dict(absorb=-0.1), "absorb"), (dict(absorb=float("nan")), "absorb"), (dict(scatter=-1.0), "scatter"),
                      (dict(scatter=float("inf")), "scatter"), (dict(iterations=-1), "iterations"), (dict(iterations=65), "iterations")):
        with pytest.raises(RenderError, match=word) as e:
            r.set_thickness(**bad)
        assert e.value.code == L.ERR_INVALID, bad
    r.set_thickness()
    for call in (r.surface_thickness, lambda: r.surface_thickness(raw=True), r.surface_opaque):
        with pytest.raises(RenderError, match="no surface frame with thickness"):
            call()
    r.from_points(x, c, ids)
    assert r.surface_opaque()[0].shape == (48, 64)
    with pytest.raises(RenderError, match="no surface frame with thickness"):
        r.surface_thickness()   # drawn, not yet composited
    assert r.surface().shape == (48, 64, 3) and r.surface_thickness().shape == (48, 64)
    key, rgb = r.layer()
    r.merge_layer(key, rgb)
    with pytest.raises(RenderError, match="sph_render_layer_merge") as e:
        r.surface()
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(RenderError, match="no surface frame with thickness"):
        r.surface_thickness()
    r.clear_thickness()
    r.from_points(x, c, ids)
    r.set_thickness()   # switched on after the frame was drawn: that frame has no opaque layer
    with pytest.raises(RenderError, match="before the thickness mode was switched on"):
        r.surface()
    r.from_points(x, c, ids)
    assert r.surface().shape == (48, 64, 3)
    many = np.zeros(((1 << 23) + 1, 3), np.float32)   # more contributions than a pixel's u32 is sure to hold
    with pytest.raises(RenderError, match="8388609 particles") as e:
        r.from_points(many)
    assert e.value.code == L.ERR_UNSUPPORTED
    r.from_points(x, c, ids)
    assert r.surface().shape == (48, 64, 3)
    r.clear_surface()   # switches the thickness mode off too
    r.set_surface()
    r.from_points(x, c, ids)
    r.surface()
    with pytest.raises(RenderError, match="no surface frame with thickness"):
        r.surface_thickness()


def test_driver_writes_translucent_surface_views(gpu, tmp_path):
    from sph_project_amd import run_simulation
    cfg, f = _driver_scene(tmp_path)
    base = ["--scene_file", str(f), "--max_steps", "5", "--render_size", "320", "240",
            "--camera_position", "1.2", "0.7", "1.3", "--camera_lookat", "0.1", "0.1", "0.1"]
    thick = ["--render_surface", "--surface_thickness", "--surface_absorb", "0.2"]
    out, dev, solid, raw = tmp_path / "out", tmp_path / "dev", tmp_path / "solid", tmp_path / "raw"
    run_simulation.main(base + ["--output_dir", str(out), "--render", "--video"] + thick)
    run_simulation.main(base + ["--output_dir", str(dev), "--render", "--png_device"] + thick)
    run_simulation.main(base + ["--output_dir", str(solid), "--render", "--render_surface"])
    run_simulation.main(base + ["--output_dir", str(raw), "--render"])
    frames = sorted(d for d in os.listdir(out) if (out / d).is_dir())
    assert frames == ["000000", "000002", "000004"]
    assert sorted(os.listdir(out)) == frames + ["raw_view.avi", "surface_view.avi"]
    container, solver = H.build_product(cfg)
    solver.prepare()
    r = FrameRenderer(container.dx, width=320, height=240, camera_position=(1.2, 0.7, 1.3), camera_lookat=(0.1, 0.1, 0.1))
    r.set_surface()
    done = 0
    for d in frames:
        assert sorted(os.listdir(out / d)) == ["raw_view.png", "surface_view.png"]
        solver.advance(int(d) + 1 - done)
        done = int(d) + 1
        r.set_thickness(absorb=0.2)
        plain = r.from_container(container)
        want = r.surface()
        r.clear_thickness()
        r.from_container(container)
        opaque_surface = r.surface()
        img = decode_png((out / d / "surface_view.png").read_bytes())
        assert img.shape == (240, 320, 3) and img.tobytes() == want.tobytes(), d
        assert decode_any_png((dev / d / "surface_view.png").read_bytes()).tobytes() == want.tobytes()
        # without the new flags nothing moved: the surface frame and the particle frame are the parent's
        solid_png = (solid / d / "surface_view.png").read_bytes()
        assert decode_png(solid_png).tobytes() == opaque_surface.tobytes() and solid_png != (out / d / "surface_view.png").read_bytes()
        assert (want != opaque_surface).any()
        for other in (out, solid):
            assert (other / d / "raw_view.png").read_bytes() == (raw / d / "raw_view.png").read_bytes()
        assert decode_png((raw / d / "raw_view.png").read_bytes()).tobytes() == plain.tobytes()
    for name in ("raw_view.avi", "surface_view.avi"):
        jpegs, info = avi_frames((out / name).read_bytes())
        assert len(jpegs) == len(frames), name
    a, _ = avi_frames((out / "raw_view.avi").read_bytes())
    b, _ = avi_frames((out / "surface_view.avi").read_bytes())
    assert a[0] != b[0]
