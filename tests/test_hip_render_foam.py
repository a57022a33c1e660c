"""GPU: diffuse particles in the surface frames (csrc/sph_render_foam.hpp) against tests/render_foam_model.py, all through the
handle path -- the three integer planes and the counters exactly, the colours within the model's derived bounds, the identities, the same
bytes and planes from both builds (wherever the builds' own foam-free planes agree: see that test) / a repeat / a second surface() /
another seeding order, the refusals, and the driver's flags.

The fluid is a resting dam-break block; the diffuse set is placed with DiffuseParticles.seed and never stepped.  The model takes the
foam-free frame's planes (key plane, surface flags and base colours, opaque layer, depth and thickness planes, surface frame) from a second
renderer without the mode on the same container: the renderer is deterministic, so these are the planes the renderer under test worked on,
which every case asserts first.

The largest colour bounds and differences of a run are recorded in profiles/render_surface_foam_gpu_tests.txt."""
import json
import os

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd.foam import DiffuseParticles
from sph_project_amd.render import FrameRenderer, RenderError
from sph_project_amd.video import decode_png as decode_any_png
from tests import helpers as H
from tests import render_foam_model as FM
from tests.test_render_host import decode_png

pytestmark = pytest.mark.gpu

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
# the block of dam_break_scene(end=(0.3, 0.16, 0.3)) at its default translation: particle centres from LO to HI, radius 0.01
LO, HI, RAD = np.array([0.1, 0.1, 0.1]), np.array([0.4, 0.24, 0.4]), 0.01
CUBE_AT = np.array([0.3, 0.25, 0.55])
CAM_A = dict(camera_position=(0.75, 0.65, 0.8), camera_lookat=(0.25, 0.2, 0.25), fov=40.0)     # down onto the top face and two sides
CAM_B = dict(camera_position=(0.25, 0.3, -0.5), camera_lookat=(0.28, 0.22, 0.5), fov=40.0)     # the cube behind the block
CAM_C = dict(camera_position=(0.25, 0.3, -0.5), camera_lookat=(0.28, 0.22, 0.5), fov=30.0)


def seeds_a(seed=21):
    """400 points: a third above the block, a third within one radius of its top face, a third inside it"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(LO, HI, (400, 3))
    top = HI[1] + RAD
    x[:134, 1] = top + rng.uniform(0.03, 0.12, 134)
    x[134:267, 1] = top + rng.uniform(-RAD, RAD, 133)
    x[267:, 1] = rng.uniform(LO[1], HI[1] - 3 * RAD, 133)
    return x.astype(np.float32)


def seeds_b():
    """(a)'s points and 120 around the cube: in front of it, straddling its faces and the box lines' depth, inside it"""
    rng = np.random.default_rng(22)
    return np.concatenate([seeds_a(), (CUBE_AT + rng.uniform(-0.16, 0.16, (120, 3))).astype(np.float32)])


def seeds_c():
    """for radius_scale 4: six spheres in front of the block near enough for the large path, sixty ordinary ones, one across the near
    plane and one wholly behind the cube"""
    eye, at = np.array(CAM_C["camera_position"]), np.array(CAM_C["camera_lookat"])
    f = (at - eye) / np.linalg.norm(at - eye)
    rng = np.random.default_rng(23)
    big = np.array([[0.12, 0.30, -0.05], [0.36, 0.32, 0.0], [0.25, 0.12, -0.08], [0.30, 0.40, -0.1], [0.2, 0.2, 0.02], [0.4, 0.15, -0.02]])
    cloud = rng.uniform(LO - 0.05, HI + 0.05, (60, 3))
    near = eye + 0.1 * f
    hidden = CUBE_AT + np.array([0.06, -0.03, 0.25])
    return np.concatenate([big, cloud, [near], [hidden]]).astype(np.float32)


def _mixed_scene():
    """the mixed scene of the thickness tests with this file's block: the rigid cube behind part of it as CAM_B sees it"""
    cfg = P.dam_break_scene(method="wcsph", end=(0.3, 0.16, 0.3), add_domain_box=False)
    cfg["RigidBodies"] = [{
        "objectId": 1, "geometryFile": os.path.join(MODELS, "cube.obj"), "translation": [float(v) for v in CUBE_AT], "rotationAxis": [0, 0, 1],
        "rotationAngle": 30, "scale": [0.8, 0.8, 0.8], "velocity": [0.0, 0.0, 0.0], "density": 900.0, "color": [255, 200, 0],
        "isDynamic": True, "entryTime": -1.0}]
    return cfg


SCENES = {
    # label: (scene, seeds, camera, box lines, set_surface_foam keywords)
    "a": (lambda: P.dam_break_scene(method="dfsph", end=(0.3, 0.16, 0.3), dt=6e-4), seeds_a, CAM_A, False, dict()),
    "b": (_mixed_scene, seeds_b, CAM_B, True, dict()),
    "c": (_mixed_scene, seeds_c, CAM_C, True, dict(radius_scale=4.0)),
}
CASES = [("a", 97, 61), ("a", 128, 128), ("b", 128, 128), ("c", 256, 256)]
CASE_IDS = [f"{c[0]}-{c[1]}x{c[2]}" for c in CASES]
_scene_cache, _cache = {}, {}


def _scene(label, fast=False):
    """the resting container of a scene and its diffuse set, once per build"""
    if (label, fast) not in _scene_cache:
        make, seeds = SCENES[label][:2]
        container, solver = H.build_product(make(), fast_math=int(fast))
        solver.prepare()
        eng = container.engine
        x = eng.download(L.F_POSITION)
        mat = eng.download(L.F_MATERIAL)
        assert np.abs(x[mat == 1].min(0) - LO).max() < 1e-3 and np.abs(x[mat == 1].max(0) - HI).max() < 1e-3   # the block the seeds were laid out for
        sx = seeds()
        d = DiffuseParticles(container.dx, container.domain_start, container.domain_end, max_diffuse=2000, fast_math=fast)
        d.seed(sx, np.zeros_like(sx), np.full(len(sx), 3.0))
        _scene_cache[(label, fast)] = (container, d, sx)
    return _scene_cache[(label, fast)]


def _renderer(label, W, Hh, fast, container):
    cam, box = SCENES[label][2], SCENES[label][3]
    return FrameRenderer(container.dx, width=W, height=Hh, fast_math=fast, box=None if box else False, **cam)


def _model_camera(label):
    cam = SCENES[label][2]
    return dict(eye=cam["camera_position"], target=cam["camera_lookat"], fov=cam["fov"])


def _case(case, thick, fast=False):
    """A case drawn once per mode and build: the foam-free planes of a second renderer, the planes and frames of the renderer under test
    (raw_spheres off, so that its particle frame is the foam-free one too), and the model's planes on them."""
    key = (case, thick, fast)
    if key in _cache:
        return _cache[key]
    label, W, Hh = case
    container, d, sx = _scene(label, fast)
    fkw = SCENES[label][4]
    eng = container.engine
    pid, mat, col = eng.download(L.F_PARTICLE_ID), eng.download(L.F_MATERIAL), eng.download(L.F_COLOR).astype(np.uint8)
    ref = _renderer(label, W, Hh, fast, container)
    ref.set_surface()
    if thick:
        ref.set_thickness()
    plain = ref.from_container(container).copy()
    ids = ref.ids()
    key0 = ref.layer()[0]
    okey, orgb = ref.surface_opaque() if thick else (None, None)
    surf_rgb = ref.surface().copy()
    q = ref.surface_depth()
    T = ref.surface_thickness() if thick else None
    order = np.argsort(pid)
    who = order[np.minimum(np.searchsorted(pid[order], np.where(ids >= 0, ids, pid[order][0])), len(pid) - 1)]
    flag = (ids >= 0) & (mat[who] == 1)
    base = np.where(flag[..., None], col[who], 0)
    r = _renderer(label, W, Hh, fast, container)
    r.set_surface()
    if thick:
        r.set_thickness()
    r.set_surface_foam(d, raw_spheres=False, **fkw)
    frame = r.from_container(container).copy()
    planes = r.surface_foam_planes()
    out = r.surface().copy()
    st = r.surface_foam_stats()
    # the planes the model takes from `ref` are the ones `r` worked on
    assert frame.tobytes() == plain.tobytes() and r.layer()[0].tobytes() == key0.tobytes() and np.array_equal(r.ids(), ids)
    assert r.surface_depth().tobytes() == q.tobytes()
    if thick:
        assert all(u.tobytes() == w.tobytes() for u, w in zip(r.surface_opaque(), (okey, orgb))) and r.surface_thickness().tobytes() == T.tobytes()
    got = d.download(sort=False)["x"]
    assert got.tobytes() == sx.tobytes()
    cam = _model_camera(label)
    m_fo, m_fu, m_du, m_st = FM.splat(got, container.dx, key0, flag, okey, radius_scale=fkw.get("radius_scale", 0.5), **cam)
    k = dict(container=container, d=d, sx=sx, ref=ref, r=r, plain=plain, ids=ids, key0=key0, okey=okey, orgb=orgb, surf_rgb=surf_rgb, q=q, T=T,
             flag=flag, base=base, planes=planes, out=out, st=st, cam=cam, fkw=fkw, model=(m_fo, m_fu, m_du), m_st=m_st, W=W, H=Hh, label=label,
             thick=thick, fast=fast)
    _cache[key] = k
    return k


def _thick_terms(k, **over):
    return dict(q=k["q"], T=k["T"], base_rgb=k["base"], flag=k["flag"], opaque_rgb=k["orgb"], radius=k["container"].dx,
                **dict(dict(absorb=0.05, scatter=0.01), **over), **k["cam"])


@pytest.mark.parametrize("thick", [False, True], ids=["opaque", "thickness"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_planes_and_counters_equal_the_model(gpu, case, thick):
    k = _case(case, thick)
    st, m_st = k["st"], k["m_st"]
    for name, got, want in zip(("fo", "fu", "du"), k["planes"], k["model"]):
        diff = got != want
        print(case, thick, name, "differences", int(diff.sum()), "set", int((got != (FM.NONE32 if name == "du" else 0)).sum()))
        assert not diff.any(), (case, thick, name, int(diff.sum()), np.argwhere(diff)[:5].tolist(), got[diff][:5], want[diff][:5])
    print(case, thick, st)
    assert {a: st[a] for a in m_st} == m_st, (st, m_st)
    fo, fu, du = k["planes"]
    assert st["diffuse"] == len(k["sx"]) and st["pixels_over"] == int((fo > 0).sum()) and st["pixels_under"] == int((fu > 0).sum())
    assert ((du != FM.NONE32) == (fu > 0)).all() and not fu[~k["flag"]].any()
    if not thick:
        assert st["adds_under"] == 0 and not fu.any()
    if case[0] == "a" and thick:
        assert (fo > 0).sum() >= 30 and (fu > 0).sum() >= 30 and (du != FM.NONE32).sum() >= 30
    if case[0] == "b":
        assert st["clipped"] > 0 and st["removed"] > 0
        assert (k["ids"] <= -2).sum() > 50 and ((k["ids"] >= 0) & ~k["flag"]).sum() > 100   # box lines and the cube are in the frame
    if case[0] == "c":
        assert st["large"] >= 3, st
        nothing = np.full(fo.shape, ALL_ONES, np.uint64)
        none = np.zeros(fo.shape, bool)
        one = lambda i, key: FM.splat(k["sx"][i:i + 1], k["container"].dx, key, none, None, radius_scale=4.0, **k["cam"])[3]
        assert one(66, nothing) == dict(adds_over=0, adds_under=0, clipped=0, removed=0)        # across the near plane
        limit = k["okey"] if thick else k["key0"]
        hidden = one(67, limit)
        assert hidden["adds_over"] == 0 and hidden["removed"] > 50                               # wholly behind the cube


@pytest.mark.parametrize("thick", [False, True], ids=["opaque", "thickness"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_colour_is_within_the_models_bound(gpu, case, thick):
    k = _case(case, thick)
    r, (fo, fu, du) = k["r"], k["planes"]
    worst_d = worst_tol = 0
    for kw in (dict(), dict(density=0.25, rgb=(200, 230, 255)), dict(density=8.0, depth_bias=1.0)):
        r.set_surface_foam(k["d"], raw_spheres=False, **dict(k["fkw"], **kw))
        r.from_container(k["container"])
        rgb = r.surface()
        assert all(u.tobytes() == w.tobytes() for u, w in zip(r.surface_foam_planes(), k["planes"]))   # (colour parameters only)
        m_rgb, tol = FM.composite(k["surf_rgb"], fo, fu, du, _thick_terms(k) if thick else None, rgb=kw.get("rgb", (255, 255, 255)),
                                  density=kw.get("density", 1.0))
        diff = np.abs(rgb.astype(np.int64) - m_rgb.astype(np.int64))
        touched = (fo > 0) | (fu > 0)
        print(case, thick, kw, "max colour difference", int(diff.max()), "largest bound", int(tol.max()), "pixels", int(touched.sum()),
              "share of bound 1:", float((tol[touched] <= 1).mean()) if touched.any() else 1.0)
        over = diff > tol
        assert not over.any(), (case, thick, kw, int(over.sum()), int(diff.max()), np.argwhere(over)[:5].tolist())
        assert np.array_equal(rgb[~touched], k["surf_rgb"][~touched])
        assert (rgb[touched] != k["surf_rgb"][touched]).any()
        worst_d, worst_tol = max(worst_d, int(diff.max())), max(worst_tol, int(tol.max()))
    assert worst_d <= 2, (worst_d, worst_tol)
    r.set_surface_foam(k["d"], raw_spheres=False, **k["fkw"])


@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fast"])
@pytest.mark.parametrize("thick", [False, True], ids=["opaque", "thickness"])
def test_identities_are_exact(gpu, thick, fast):
    k = _case(CASES[1], thick, fast)
    r, ref, d, container = k["r"], k["ref"], k["d"], k["container"]
    fo, fu, du = k["planes"]
    # density 0: the surface frame without the mode
    r.set_surface_foam(d, density=0.0, raw_spheres=False)
    r.from_container(container)
    assert r.surface().tobytes() == k["surf_rgb"].tobytes()
    # defaults: untouched pixels keep the foam-free surface frame's bytes; the depth and thickness planes are the foam-free ones
    r.set_surface_foam(d)
    raw = r.from_container(container).copy()
    raw_ids, raw_layer = r.ids().copy(), r.layer()
    out = r.surface()
    touched = (fo > 0) | (fu > 0)
    assert np.array_equal(out[~touched], k["surf_rgb"][~touched]) and touched.sum() > 60
    assert r.surface_depth().tobytes() == k["q"].tobytes()
    if thick:
        assert r.surface_thickness().tobytes() == k["T"].tobytes() and r.surface_thickness(raw=True).tobytes() == ref.surface_thickness(raw=True).tobytes()
    assert all(u.tobytes() == w.tobytes() for u, w in zip(r.surface_foam_planes(), k["planes"]))   # raw_spheres does not move the planes
    assert out.tobytes() == k["out"].tobytes()
    # raw_spheres: the particle frame, ids and layer are those of a plain renderer with set_foam
    p = _renderer(k["label"], k["W"], k["H"], fast, container)
    p.set_foam(d)
    want = p.from_container(container)
    assert raw.tobytes() == want.tobytes() and (raw != k["plain"]).any()
    assert np.array_equal(raw_ids, p.ids()) and (raw_ids < -17).sum() > 30
    assert all(u.tobytes() == w.tobytes() for u, w in zip(raw_layer, p.layer()))
    # a saturated layer: the centre pixel of a diffuse sphere in front of everything holds rgb exactly
    r.set_surface_foam(d, density=1e6, rgb=(12, 200, 77), raw_spheres=False)
    r.from_container(container)
    sat = r.surface()
    covered = fo >= 128   # more than a quarter of a diffuse diameter of chord in front of the limit
    assert covered.sum() > 20 and (sat[covered] == np.array([12, 200, 77], np.uint8)).all()
    r.set_surface_foam(d, raw_spheres=False)


def test_builds_repeats_and_seeding_orders_give_the_same_bytes_and_planes(gpu):
    for case, thick in ((CASES[0], True), (CASES[2], True), (CASES[3], False)):
        a, b = _case(case, thick, False), _case(case, thick, True)
        # What the mode reads is by definition the build's own: t_w is the upper half of the frame's key plane, t_op of the opaque layer's,
        # Q the quantised key plane, cur the surface frame's byte -- and the ordinary splat that writes the keys contracts in the fast
        # build (their depths differ in the last bits, as layer()'s do; tests/test_hip_render_thickness.py compares them within each build
        # for the same reason, and those kernels are not this mode's to change).  Wherever the two builds hold the same inputs the planes
        # are the same integers and the frame the same bytes; where a limit differs in its last bits a chord cut by it (or du, measured
        # from it) may truncate to the next unit, and a byte computed from it may round to the next step.  Measured (MI355X,
        # profiles/render_surface_foam_gpu_tests.txt): limits differ on 429 / 2,326 / 15,645 pixels of the three cases; planes differ on
        # 0 / 2 (du) / 15 (fo) of them, each by one unit; bytes on 0 / 0 / 4.
        same = a["key0"] == b["key0"]
        if thick:
            same &= a["okey"] == b["okey"]
        differ = [u != w for u, w in zip(a["planes"], b["planes"])]
        for name, m in zip(("fo", "fu", "du"), differ):
            assert not (m & same).any(), (case, "builds", name, int((m & same).sum()))
        inputs = same & ~differ[0] & ~differ[1] & ~differ[2] & (a["surf_rgb"] == b["surf_rgb"]).all(axis=2)
        qsame = np.pad(a["q"] == b["q"], 1, constant_values=True)   # the under layer's normal reads the four neighbours' depths
        inputs &= qsame[1:-1, 1:-1] & qsame[:-2, 1:-1] & qsame[2:, 1:-1] & qsame[1:-1, :-2] & qsame[1:-1, 2:]
        if thick:
            inputs &= a["T"] == b["T"]
        bytes_differ = (a["out"] != b["out"]).any(axis=2)
        print(case, "pixels whose limits differ between the builds:", int((~same).sum()), "plane pixels that differ: fo / fu / du",
              [int(m.sum()) for m in differ], "largest difference", [int(np.abs(u.astype(np.int64) - w.astype(np.int64)).max())
                                                                      for u, w in zip(a["planes"], b["planes"])],
              "pixels whose inputs differ:", int((~inputs).sum()), "pixels whose bytes differ:", int(bytes_differ.sum()))
        assert not (bytes_differ & inputs).any(), (case, "builds", int((bytes_differ & inputs).sum()))
        r, container = a["r"], a["container"]
        r.from_container(container)
        first = r.surface().copy()
        second = r.surface().copy()            # a second call on the same frame
        r.from_container(container)
        third = r.surface().copy()             # a repeat
        assert first.tobytes() == second.tobytes() == third.tobytes() == a["out"].tobytes(), case
        assert all(u.tobytes() == w.tobytes() for u, w in zip(r.surface_foam_planes(), a["planes"]))
        perm = np.random.default_rng(4).permutation(len(a["sx"]))
        d2 = DiffuseParticles(container.dx, container.domain_start, container.domain_end, max_diffuse=2000)
        d2.seed(a["sx"][perm], np.zeros_like(a["sx"]), np.full(len(perm), 3.0))
        for raw_spheres in (False, True):
            r.set_surface_foam(d2, raw_spheres=raw_spheres, **a["fkw"])
            r.from_container(container)
            assert r.surface().tobytes() == a["out"].tobytes(), (case, "order", raw_spheres)
            assert r.surface().tobytes() == a["out"].tobytes(), (case, "order, second call", raw_spheres)
            assert all(u.tobytes() == w.tobytes() for u, w in zip(r.surface_foam_planes(), a["planes"]))
        r.set_surface_foam(a["d"], raw_spheres=False, **a["fkw"])


def test_refusals_are_errors_with_messages_and_leave_the_simulation_alone(gpu):
    def run(render):
        container, solver = H.build_product(P.dam_break_scene(method="dfsph", end=(0.2, 0.2, 0.2), dt=6e-4))
        solver.prepare()
        if render:
            refusals(container)
        for _ in range(4):
            solver.step()
        eng = container.engine
        eng.synchronize()
        return eng.download(L.F_POSITION), eng.download(L.F_VELOCITY), eng.download(L.F_PARTICLE_ID)

    def refusals(container):
        d = DiffuseParticles(container.dx, container.domain_start, container.domain_end, max_diffuse=1000)
        d.seed([[0.2, 0.35, 0.2]], [[0, 0, 0]], [1.0])
        r = FrameRenderer(container.dx, width=64, height=48, camera_position=(0.9, 0.6, 1.0), camera_lookat=(0.2, 0.2, 0.2))
        with pytest.raises(RenderError, match="surface mode is off") as e:
            r.set_surface_foam(d)
        assert e.value.code == L.ERR_INVALID
        r.set_surface()
        for bad, word in ((dict(radius_scale=0.0), "radius_scale"), (dict(radius_scale=float("nan")), "radius_scale"),
                          (dict(radius_scale=float("inf")), "radius_scale"), (dict(density=-1.0), "density"), (dict(density=float("nan")), "density"),
                          (dict(depth_bias=-0.5), "depth_bias"), (dict(depth_bias=float("inf")), "depth_bias")):
            with pytest.raises(RenderError, match=word) as e:
                r.set_surface_foam(d, **bad)
            assert e.value.code == L.ERR_INVALID, bad
        with pytest.raises(RenderError, match="surface mode is on") as e:   # set_foam under the surface mode is still refused
            r.set_foam(d)
        assert e.value.code == L.ERR_UNSUPPORTED
        # set_foam set at the same time
        s = FrameRenderer(container.dx, width=64, height=48)
        s.set_foam(d)
        lib = L.load()
        h = s._native(None)
        import ctypes as C
        sp = L.SphRenderSurfaceParams()
        sp.iterations, sp.rmax, sp.sigma, sp.range, sp.spec, sp.shininess, sp.object_mask = 3, 12, 1.5, 2.0, 0.35, 40.0, -1
        assert lib.sph_render_set_surface(h, C.byref(sp)) == 0
        assert lib.sph_render_set_surface_foam(h, d.h, None) == L.ERR_UNSUPPORTED
        assert b"sph_render_set_foam" in lib.sph_render_last_error(h)
        s.close()
        if lib.sph_device_count() > 1:
            other = DiffuseParticles(container.dx, container.domain_start, container.domain_end, max_diffuse=10, device=1)
            with pytest.raises(RenderError, match="device") as e:
                r.set_surface_foam(other)
            assert e.value.code == L.ERR_INVALID
        # a frame drawn before the mode was switched on
        r.from_container(container)
        r.set_surface_foam(d)
        with pytest.raises(RenderError, match="before the diffuse particles were set") as e:
            r.surface()
        assert e.value.code == L.ERR_INVALID
        with pytest.raises(RenderError, match="no frame with diffuse particles"):
            r.surface_foam_planes()
        r.from_container(container)
        assert r.surface().shape == (48, 64, 3) and r.surface_foam_planes()[0].shape == (48, 64)
        r.set_thickness()   # the planes of the frame held were summed against the other limits
        with pytest.raises(RenderError, match="thickness"):
            r.surface()
        r.from_container(container)
        assert r.surface().shape == (48, 64, 3)
        # the points path ignores the mode
        x = container.engine.download(L.F_POSITION)
        r.clear_thickness()
        r.from_points(x)
        a = r.surface()
        r.clear_surface_foam()
        r.from_points(x)
        assert r.surface().tobytes() == a.tobytes()
        # a diffuse count whose chords could overflow a pixel's u32: refused before any launch
        r.set_surface_foam(d, radius_scale=1e7)
        with pytest.raises(RenderError, match="2\\^32") as e:
            r.from_container(container)
        assert e.value.code == L.ERR_UNSUPPORTED
        # switching the surface mode off switches this mode off
        r.set_surface_foam(d)
        r.clear_surface()
        r.set_surface()
        r.from_container(container)
        r.surface()
        with pytest.raises(RenderError, match="no frame with diffuse particles"):
            r.surface_foam_planes()
        # (a sharded handle: the guard is the first statement of the handle-side check, as sph_foam_step_handle's; a two-rank fixture is
        # not cheap)

    a, b = run(False), run(True)
    for u, w in zip(a, b):
        assert u.tobytes() == w.tobytes()


def test_driver_writes_white_water_into_surface_views(gpu, tmp_path):
    from sph_project_amd import run_simulation
    cfg = P.dam_break_scene(method="wcsph", end=(0.36, 0.36, 0.36), velocity=(2.5, 0.0, 0.0))
    cfg["Configuration"].update(exportFrame=True, exportPly=True, outputInterval=50,
                                foam=dict(e_min=0.2, e_max=3.0, ta_min=0.5, ta_max=5.0, wc_min=0.2, wc_max=2.0))
    f = tmp_path / "scene.json"
    f.write_text(json.dumps(cfg))
    size = ["--render_size", "320", "240", "--camera_position", "1.6", "0.9", "1.8", "--camera_lookat", "0.3", "0.2", "0.3"]
    common = ["--scene_file", str(f), "--max_steps", "160"] + size
    new, dev, foam, nofoam, surf = (tmp_path / n for n in ("new", "dev", "foam", "nofoam", "surf"))
    run_simulation.main(common + ["--output_dir", str(new), "--render", "--foam", "--render_surface", "--surface_foam"])
    run_simulation.main(common + ["--output_dir", str(dev), "--render", "--foam", "--render_surface", "--surface_foam", "--png_device"])
    run_simulation.main(common + ["--output_dir", str(foam), "--render", "--foam"])
    run_simulation.main(common + ["--output_dir", str(nofoam), "--render", "--render_surface"])
    frames = sorted(os.listdir(foam))
    assert frames == ["000000", "000050", "000100", "000150"] == sorted(os.listdir(new)) == sorted(os.listdir(nofoam))
    differ = 0
    for fr in frames:
        assert sorted(os.listdir(new / fr)) == ["diffuse_particles.ply", "particle_object_0.ply", "raw_view.png", "surface_view.png"]
        assert sorted(os.listdir(nofoam / fr)) == ["particle_object_0.ply", "raw_view.png", "surface_view.png"]   # nothing new without the flags
        for name in ("raw_view.png", "particle_object_0.ply", "diffuse_particles.ply"):
            assert (new / fr / name).read_bytes() == (foam / fr / name).read_bytes(), (fr, name)
        a, b = decode_png((new / fr / "surface_view.png").read_bytes()), decode_png((nofoam / fr / "surface_view.png").read_bytes())
        differ += int((a != b).any())
        assert decode_any_png((dev / fr / "surface_view.png").read_bytes()).tobytes() == a.tobytes(), fr
    assert differ >= 1
    # the last frame through the Python interface
    container, solver = H.build_product(cfg)
    solver.prepare()
    args = run_simulation.parse_args(["--scene_file", str(f), "--foam"])
    d = run_simulation.make_foam(container, solver, run_simulation.SimConfig(scene_file_path=str(f)), args)
    run_simulation.FoamStepper(solver, container, d, 4, float(solver.dt[None])).advance(151)
    r = FrameRenderer(container.dx, width=320, height=240, camera_position=(1.6, 0.9, 1.8), camera_lookat=(0.3, 0.2, 0.3))
    r.set_surface()
    r.set_surface_foam(d)
    r.from_container(container)
    want = r.surface()
    assert decode_png((new / "000150" / "surface_view.png").read_bytes()).tobytes() == want.tobytes()
    assert r.surface_foam_stats()["pixels_over"] > 0
