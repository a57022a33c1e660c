"""CPU: the screen-space surface mode without a GPU -- properties of the integer model (tests/render_surface_model.py) on
hand-made key planes, the C-ABI mirror, and the driver's argument errors."""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from sph_project_amd import _lib as L
from tests import render_surface_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS, FOV = 0.02, 70.0


def _plane(t, flag=None, H=None):
    """quantised depth of a plane of f32 depths (every pixel a surface pixel unless flag says otherwise)"""
    t = np.asarray(t, np.float32)
    ids = np.arange(t.size, dtype=np.int64).reshape(t.shape)
    flag = np.ones(t.shape, bool) if flag is None else flag
    inv_u, u, rnum, dq = SM.constants(RADIUS, H or t.shape[0], FOV)
    return SM.quantise(SM.make_key(t, ids), flag, inv_u), rnum, dq


def test_quantise_is_one_f32_multiply_and_a_truncation():
    t = np.array([[0.1, 1.0, 2.5, 1e9, 3.9999]], np.float32)
    inv_u, u, _, _ = SM.constants(RADIUS, 64, FOV)
    q, _, _ = _plane(t)
    want = [int(np.float32(v) * inv_u) for v in t[0]]
    want[3] = SM.QMAX
    assert q[0].tolist() == want
    assert inv_u == np.float32(256.0 / float(np.float32(RADIUS))) and u == np.float32(RADIUS) / np.float32(256.0)
    q2, _, _ = _plane(t, flag=np.array([[1, 0, 1, 1, 0]], bool))
    assert q2[0, 1] == SM.SENT and q2[0, 4] == SM.SENT and q2[0, 0] == q[0, 0]


def test_a_flat_sheet_is_a_fixed_point():
    q, rnum, dq = _plane(np.full((40, 52), 2.0, np.float32))
    out, st, steps = SM.smooth(q, 4, rnum, dq, 12)
    assert all(np.array_equal(s, q) for s in steps)
    assert st["surface_pixels"] == 40 * 52 and st["taps_accepted"] < st["taps_visited"]   # the border windows leave the frame


def test_a_bumpy_sheet_never_widens():
    rng = np.random.default_rng(5)
    t = (2.0 + 0.01 * rng.standard_normal((48, 48))).astype(np.float32)
    q, rnum, dq = _plane(t)
    _, _, steps = SM.smooth(q, 5, rnum, dq, 12)
    spread = [int(s.max()) - int(s.min()) for s in steps]
    assert spread[0] > 0 and all(b <= a for a, b in zip(spread, spread[1:])), spread
    assert spread[-1] < spread[0]
    for a, b in zip(steps, steps[1:]):   # convex combinations: every value stays inside the range of the previous iterate
        assert b.min() >= a.min() and b.max() <= a.max()


def test_two_sheets_further_apart_than_dq_never_mix():
    rng = np.random.default_rng(6)
    H = W = 48
    front = np.zeros((H, W), bool)
    front[10:30, 8:40] = True
    t = np.where(front, 2.0, 2.5).astype(np.float32) + (0.004 * rng.standard_normal((H, W))).astype(np.float32)
    q, rnum, dq = _plane(t)
    f0 = q[front].astype(np.int64)
    assert int(q[~front].min()) - int(f0.max()) > dq + (f0.max() - f0.min())
    _, _, steps = SM.smooth(q, 5, rnum, dq, 12)
    for s in steps:
        assert s[front].min() >= f0.min() and s[front].max() <= f0.max()
    # ... and the front sheet smooths as if the back one were not there
    alone, _, _ = SM.smooth(np.where(front, q, np.uint64(SM.SENT)), 5, rnum, dq, 12)
    assert np.array_equal(alone[front], steps[-1][front])


def test_a_lone_pixel_is_unchanged_and_faces_the_eye():
    H = W = 33
    flag = np.zeros((H, W), bool)
    flag[11, 20] = True
    q, rnum, dq = _plane(np.full((H, W), 1.7, np.float32), flag)
    out, st, _ = SM.smooth(q, 3, rnum, dq, 12)
    assert np.array_equal(out, q) and st["taps_accepted"] == 3 and st["surface_pixels"] == 1
    sx, sy = SM.sides(out)[:2]
    assert sx[11, 20] == 0 and sy[11, 20] == 0
    cam = dict(eye=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
    base = np.full((H, W, 3), 200, np.uint8)
    frame = np.full((H, W, 3), 7, np.uint8)
    rgb, tol, n = SM.shade(out, base, flag, frame, RADIUS, fov=FOV, **cam)
    from tests import render_model as RM
    E, f, s, u, tx, ty = RM.camera(cam["eye"], cam["target"], cam["up"], FOV, W, H)
    X, Y = RM.pixel_rays(W, H, tx, ty)
    d = np.array([X[20], Y[11], 1.0])
    assert np.allclose(n[11, 20], -d / np.linalg.norm(d), atol=1e-12)
    assert (rgb[~flag] == 7).all() and (tol[~flag] == 0).all() and tol[11, 20] == 1


def test_window_follows_the_depth_and_clamps_at_both_ends():
    inv_u, u, rnum, dq = SM.constants(RADIUS, 256, FOV)
    q = np.array([[0, 1, rnum // 13, rnum // 12, rnum // 2, rnum, rnum + 1, SM.QMAX]], np.uint64)
    R, clamped = SM.window(q, rnum, 12)
    assert R[0].tolist() == [12, 12, 12, 12, 2, 1, 1, 1]
    assert clamped[0].tolist() == [True, True, True, False, False, False, False, False]


def test_normal_of_a_tilted_plane_and_the_tie_rule():
    # a plane z = z0 + k x in view space, sampled along the pixel rays: every difference gives the same normal
    H = W = 64
    cam = dict(eye=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
    from tests import render_model as RM
    E, f, s, u, tx, ty = RM.camera(cam["eye"], cam["target"], cam["up"], FOV, W, H)
    X, Y = RM.pixel_rays(W, H, tx, ty)
    k, z0 = 0.5, 2.0
    z = z0 / (1.0 - k * X)[None, :] * np.ones((H, 1))   # z = z0 + k z X
    q, rnum, dq = _plane(z.astype(np.float32))
    sx, sy, *_ = SM.sides(q)
    assert (sy[1:-1] == 1).all() and (sy[0] == 1).all() and (sy[-1] == -1).all()   # equal |dq| up and down: the + side
    assert (sx[:, -1] == -1).all()
    rgb, tol, n = SM.shade(q, np.full((H, W, 3), 255, np.uint8), np.ones((H, W), bool), np.zeros((H, W, 3), np.uint8), RADIUS, fov=FOV, **cam)
    want = np.array([k, 0.0, -1.0]) / np.hypot(k, 1.0)
    assert np.abs(n[4:-4, 4:-4] - want).max() < 2e-2   # (the depth is quantised to r / 256 and the pixels are 0.03 wide)
    assert (tol == 1).mean() > 0.5


# --- C-ABI -----------------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["sph_render_set_surface", "sph_render_points_surface_mask", "sph_render_surface", "sph_render_surface_download_depth",
               "sph_render_surface_stats"]


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header and name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    from sph_project_amd import render as R
    assert R.SURFACE_SENTINEL == SM.SENT and "SPH_RENDER_SURFACE_SENTINEL 0xFFFFFFFFu" in header


@pytest.mark.parametrize("struct_name", ["SphRenderSurfaceParams", "SphRenderSurfaceStats", "SphRenderStats"])
def test_surface_structs_match_the_header(struct_name):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None
    cls = getattr(L, struct_name)
    names = [n for n, _ in cls._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"sph_hip.h\"\nint main(void){\n"
    src += "".join(f'printf("%zu\\n", offsetof({struct_name}, {n}));\n' for n in names)
    src += f'printf("%zu\\n", sizeof({struct_name})); return 0; }}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "o.c"), os.path.join(d, "o")
        open(c, "w").write(src)
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    assert [getattr(cls, n).offset for n in names] == vals[:-1]
    assert ctypes.sizeof(cls) == vals[-1]


def test_null_renderer_is_refused_without_a_device():
    lib = L.load()
    p = L.SphRenderSurfaceParams()
    assert lib.sph_render_set_surface(None, ctypes.byref(p)) == L.ERR_INVALID
    assert lib.sph_render_surface(None) == L.ERR_INVALID
    assert lib.sph_render_surface_stats(None, None) == L.ERR_INVALID


# --- driver ----------------------------------------------------------------------------------------------------------------------

def _scene(tmp_path):
    from sph_project_amd import product as P
    cfg = P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2))
    cfg["Configuration"].update(exportFrame=True, outputInterval=2)
    f = tmp_path / "frames.json"
    f.write_text(json.dumps(cfg))
    return f


def _driver(args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # no GPU may be opened for these answers
    return subprocess.run([sys.executable, os.path.join(ROOT, "sph_project_amd", "run_simulation.py")] + args, capture_output=True,
                          text=True, env=env, cwd=ROOT, timeout=120)


def test_driver_refuses_render_surface_on_several_gpus_before_opening_one(tmp_path):
    f = _scene(tmp_path)
    r = _driver(["--scene_file", str(f), "--output_dir", str(tmp_path / "o"), "--render_surface", "--gpus", "2"])
    assert r.returncode == 2 and "--render_surface" in r.stderr and "--gpus 2" in r.stderr, r.stderr
    assert not (tmp_path / "o").exists()


@pytest.mark.parametrize("flag,value", [("--surface_iters", "2"), ("--surface_sigma", "1.0"), ("--surface_range", "3.0")])
def test_driver_refuses_surface_parameters_without_the_mode(tmp_path, flag, value):
    f = _scene(tmp_path)
    r = _driver(["--scene_file", str(f), "--output_dir", str(tmp_path / "o"), "--render", flag, value])
    assert r.returncode == 2 and flag in r.stderr and "--render_surface" in r.stderr, r.stderr
    assert not (tmp_path / "o").exists()


def test_driver_lists_the_surface_flags():
    r = _driver(["--help"])
    assert r.returncode == 0
    for flag in ("--render_surface", "--surface_iters", "--surface_sigma", "--surface_range"):
        assert flag in r.stdout
