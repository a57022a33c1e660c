"""CPU: the model of the diffuse particles in the surface frames (tests/render_foam_model.py) against a float64 brute-force
restatement on hand-placed spheres, the properties of its colour stage, the ABI of the new entry points and the driver's argument errors."""
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
from tests import render_foam_model as FM
from tests import render_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, R, ZN = 96, 64, 0.05, 0.1
CAM = dict(eye=(0.0, 0.0, 2.0), target=(0.0, 0.0, 0.0), fov=60.0)
F = np.float32


def _at(depth, X=0.0, Y=0.0):
    E, f, s, u, tx, ty = RM.camera(**CAM, up=(0.0, 1.0, 0.0), W=W, H=H)
    return E + depth * (f + X * s + Y * u)


# a wall of fluid spheres at view depth 1.0 over the left two thirds of the frame, an opaque sphere behind its middle, and a dozen diffuse
# spheres (radius 0.5 R) placed by hand; every one is named by what must happen to it
WALL = np.array([_at(1.0, X, Y) for X in np.arange(-0.55, 0.2, 0.06) for Y in np.arange(-0.35, 0.36, 0.06)], np.float32)
OPAQUE = np.array([_at(1.3, -0.2, 0.0)], np.float32)
DIFFUSE = {
    "front": _at(0.7, -0.3, 0.1), "front2": _at(0.5, -0.1, -0.2), "front_free": _at(0.8, 0.45, 0.2),
    "behind": _at(1.15, -0.45, 0.25), "behind2": _at(1.2, 0.05, -0.25), "behind_free": _at(1.5, 0.45, -0.2),
    "straddle_bias": _at(1.0 - R + R + 0.5 * R + 0.001, -0.3, -0.1),   # t0 about one radius behind the wall's front: both sides of t_w + bias
    "straddle_wall": _at(1.0 - R, -0.5, -0.25),                         # its chord begins in front of the wall's depth and ends behind it
    "cut": _at(1.3 - R - 0.01, -0.2, 0.0),                              # reaches into the opaque sphere: cut by L in thickness mode
    "removed": _at(1.3, -0.2, 0.0),                                     # inside the opaque sphere: removed by L
    "near": _at(ZN, 0.02, 0.01),                                        # across the near plane: t0 <= z_near on every ray
    "far_corner": _at(0.9, 0.55, 0.33),
}
DX = np.array(list(DIFFUSE.values()), np.float32)


def _planes():
    key_w = FM.front_depth(WALL, R, W, H, ZN, **CAM)
    key_o = FM.front_depth(OPAQUE, R, W, H, ZN, **CAM)
    okey = np.where(key_o != FM.ALL_ONES, key_o | np.uint64(0x40000000), key_o)   # (ids of their own)
    key0 = np.minimum(key_w, okey)
    flag = (key0 == key_w) & (key_w != FM.ALL_ONES)
    return key0, flag, okey


def _brute(thick, radius_scale=0.5, bias_radii=1.0):
    """float64, pair by pair: per pixel the sum of the chords in units of u over and under, the smallest (t0 - t_w) / u of an under
    chord, the number of pairs, and whether a pair lies within 1e-5 of one of the decisions (hit, near plane, limit, bias)."""
    key0, flag, okey = _planes()
    tw, has_w = FM.key_depth(key0)
    top, has_l = FM.key_depth(okey) if thick else (tw, has_w)
    tw, top = tw.astype(np.float64).reshape(H, W), top.astype(np.float64).reshape(H, W)
    has_l = has_l.reshape(H, W)
    E, f, s, u, tx, ty = RM.camera(**CAM, up=(0.0, 1.0, 0.0), W=W, H=H)
    Xc, Yr = RM.pixel_rays(W, H, tx, ty)
    X, Y = np.meshgrid(Xc, Yr)
    r, rf = float(F(R)), radius_scale * R
    inv_u, bias = 256.0 / r, bias_radii * r
    eps = 1e-5
    fo, fu = np.zeros((H, W)), np.zeros((H, W))
    du = np.full((H, W), np.inf)
    pairs, near = np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    what = {}
    for name, c in zip(DIFFUSE, DX.astype(np.float64)):
        v = c - E
        xs, ys, z = v @ s, v @ u, v @ f
        dd = X * X + Y * Y + 1
        k = (X * xs + Y * ys + z) / dd
        h = rf * rf - ((xs - k * X) ** 2 + (ys - k * Y) ** 2 + (z - k) ** 2)
        root = np.sqrt(np.maximum(h, 0) / dd)
        t0, t1 = k - root, k + root
        hit = (h >= 0) & (t0 > ZN)
        near |= (np.abs(h) < eps * rf) | ((h >= 0) & (np.abs(t0 - ZN) < eps))
        b = np.where(has_l & (top < t1), top, t1)
        add = hit & (b > t0)
        near |= hit & ((np.abs(b - t0) < eps) | (has_l & (np.abs(top - t1) < eps)))
        under = add & thick & flag & (t0 >= tw + bias)
        near |= add & thick & flag & (np.abs(t0 - (tw + bias)) < eps)
        over = add & ~under
        fo += np.where(over, (b - t0) * inv_u, 0)
        fu += np.where(under, (b - t0) * inv_u, 0)
        du = np.where(under, np.minimum(du, (t0 - tw) * inv_u), du)
        pairs += add
        what[name] = dict(hit=int(hit.sum()), over=int(over.sum()), under=int(under.sum()), cut=int((add & has_l & (top < t1)).sum()),
                          removed=int((hit & ~add).sum()))
    return fo, fu, du, pairs, near, what


@pytest.mark.parametrize("thick", [False, True])
def test_model_planes_match_a_float64_brute_force(thick):
    key0, flag, okey = _planes()
    fo, fu, du, st = FM.splat(DX, R, key0, flag, okey if thick else None, zn=ZN, **CAM)
    bfo, bfu, bdu, pairs, near, what = _brute(thick)
    clear = ~near
    assert clear.mean() > 0.98
    # every pair truncates once and its f32 chord is within a few 1e-6 of the float64 one: at most one unit per pair
    assert (np.abs(fo.astype(np.float64) - bfo)[clear] <= pairs[clear] + 1e-3).all()
    assert (np.abs(fu.astype(np.float64) - bfu)[clear] <= pairs[clear] + 1e-3).all()
    has = np.isfinite(bdu)
    assert np.array_equal((du != FM.NONE32)[clear], has[clear])
    assert (np.abs(du.astype(np.float64) - bdu)[clear & has] <= 1.0 + 1e-3).all()
    assert ((fo > 0) | (fu > 0))[clear].sum() == (pairs > 0)[clear].sum() > 40
    # the hand-placed spheres do what their names say
    assert what["front"]["over"] > 3 and what["front"]["under"] == 0 and what["front2"]["over"] > 3
    assert what["front_free"]["over"] > 3 and what["behind_free"]["over"] > 0 and what["behind_free"]["under"] == 0   # no surface there
    assert what["near"]["hit"] == 0 and what["near"]["over"] == 0
    if thick:
        assert what["behind"]["under"] > 0 and what["behind"]["over"] == 0 and what["behind2"]["under"] > 0
        assert what["straddle_wall"]["over"] > 0 and what["straddle_wall"]["cut"] == 0
        assert what["cut"]["cut"] > 0 and what["removed"]["removed"] > 0 and what["removed"]["over"] + what["removed"]["under"] == 0
        assert st["adds_under"] > 0 and (fu > 0).sum() > 5 and ((du != FM.NONE32) == (fu > 0)).all()
    else:
        assert what["behind"]["removed"] > 0 and what["behind"]["over"] == 0          # the frame is opaque: behind the wall nothing is left
        assert what["straddle_wall"]["cut"] > 0                                        # cut by the wall's own depth
        assert st["adds_under"] == 0 and not fu.any() and (du == FM.NONE32).all()
    assert st["clipped"] > 0 and st["removed"] > 0
    total = {k: sum(w[k] for w in what.values()) for k in ("over", "under", "cut", "removed")}
    # counters: the two statements may differ on the pairs that sit on a decision
    slack = int(near.sum()) * len(DIFFUSE)
    assert abs(st["adds_over"] - total["over"]) <= slack and abs(st["adds_under"] - total["under"]) <= slack
    assert abs(st["clipped"] - total["cut"]) <= slack and abs(st["removed"] - total["removed"]) <= slack


def test_bias_decides_over_or_under():
    key0, flag, okey = _planes()
    one = DX[list(DIFFUSE).index("straddle_bias")][None]
    lo = FM.splat(one, R, key0, flag, okey, depth_bias=0.0, zn=ZN, **CAM)[3]
    hi = FM.splat(one, R, key0, flag, okey, depth_bias=3.0, zn=ZN, **CAM)[3]
    mid = FM.splat(one, R, key0, flag, okey, depth_bias=1.0, zn=ZN, **CAM)[3]
    assert lo["adds_under"] > 0 and lo["adds_over"] == 0 and hi["adds_under"] == 0 and hi["adds_over"] == lo["adds_under"]
    assert mid["adds_over"] + mid["adds_under"] == lo["adds_under"]


def test_intensity_is_monotone_and_zero_at_zero():
    Fs = np.concatenate([np.arange(0, 4096), 2 ** np.arange(12, 32, dtype=np.int64) - 1])
    for density in (0.0, 1e-3, 1.0, 7.5, 1e6):
        I, I32 = FM.intensity(Fs, density), FM.intensity32(Fs, density)
        assert I[0] == 0.0 and I32[0] == 0.0 and I32.dtype == np.float32
        assert (np.diff(I) >= 0).all() and (np.diff(I32) >= 0).all() and I.max() <= 1.0 and I32.max() <= 1.0
    assert not FM.intensity32(Fs, 0.0).any()
    assert FM.intensity32(np.array([256]), 1e6)[0] == 1.0


def test_over_composite_stays_between_the_pixel_and_the_foam_colour():
    rng = np.random.default_rng(5)
    cur = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    fo = rng.integers(0, 3000, (40, 50)).astype(np.uint32)
    fo[::3] = 0
    for rgb in ((255, 255, 255), (10, 200, 90)):
        out, tol = FM.over(cur, fo, rgb=rgb, density=1.0)
        lo, hi = np.minimum(cur, np.asarray(rgb, np.uint8)), np.maximum(cur, np.asarray(rgb, np.uint8))
        assert ((out >= lo) & (out <= hi)).all()
        assert np.array_equal(out[fo == 0], cur[fo == 0]) and not tol[fo == 0].any() and (tol[fo > 0] == 1).all()
    out, _ = FM.over(cur, fo, density=0.0)
    assert np.array_equal(out, cur)
    out, _ = FM.over(cur, np.full((40, 50), 256, np.uint32), rgb=(1, 2, 3), density=1e6)
    assert (out == np.array([1, 2, 3], np.uint8)).all()


def test_render_byte_gives_every_byte_back():
    b = np.arange(256)
    assert np.array_equal(FM.render_byte(b / 255.0), b)
    b32 = np.arange(256, dtype=np.float32)
    assert np.array_equal(np.floor(np.float32(255) * (b32 / np.float32(255)) + np.float32(0.5)), b32)   # in f32, as the device divides


def test_a_saturated_under_layer_hides_what_is_behind():
    rng = np.random.default_rng(6)
    lit, hi, f = rng.uniform(0, 1, (30, 3)), rng.uniform(0, 0.3, (30, 3)), np.array([1.0, 0.9, 0.8])
    kc, T, du = rng.uniform(0.01, 0.1, (30, 3)), rng.integers(1, 5000, (30, 1)), rng.integers(0, 3000, (30, 1))
    a = FM.under_value(lit, hi, rng.uniform(0, 1, (30, 3)), f, kc, T, du, 1.0)[0]
    b = FM.under_value(lit, hi, rng.uniform(0, 1, (30, 3)), f, kc, T, du, 1.0)[0]
    assert np.array_equal(a, b)
    c = FM.under_value(lit, hi, np.zeros((30, 3)), f, kc, T, du, 0.5)[0]
    d = FM.under_value(lit, hi, np.ones((30, 3)), f, kc, T, du, 0.5)[0]
    assert (d > c).all()
    # without foam the two columns multiply back to section 25's single transmittance
    behind = rng.uniform(0, 1, (30, 3))
    v0 = FM.under_value(lit, hi, behind, f, kc, T, du, 0.0)[0]
    a_all = np.exp2(-(kc * np.maximum(T, 1) / 256.0))
    assert np.allclose(v0, (behind * a_all + lit * (1 - a_all)) + hi, rtol=0, atol=1e-12)


def test_defaults_are_the_documented_ones():
    import inspect
    from sph_project_amd.render import FrameRenderer
    sig = inspect.signature(FrameRenderer.set_surface_foam).parameters
    for k, v in FM.DEFAULTS.items():
        assert sig[k].default == v, k
    assert FM.DEFAULTS == dict(radius_scale=0.5, density=1.0, depth_bias=1.0, rgb=(255, 255, 255), raw_spheres=True)


def test_abi_symbols_are_declared_and_exported():
    names = ("sph_render_set_surface_foam", "sph_render_surface_download_foam", "sph_render_surface_foam_stats")
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    for n in names:
        assert n in L.EXPORTED_SYMBOLS and f"int {n}(" in header
    for method in ("set_surface_foam", "clear_surface_foam", "surface_foam_planes", "surface_foam_stats"):
        from sph_project_amd.render import FrameRenderer
        assert callable(getattr(FrameRenderer, method))


@pytest.mark.parametrize("struct_name", ["SphRenderSurfaceFoamParams", "SphRenderSurfaceFoamStats"])
def test_structs_match_the_header(struct_name):
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


def _driver(args, tmp_path):
    from sph_project_amd import product as P
    cfg = P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2))
    cfg["Configuration"].update(exportFrame=True, outputInterval=2)
    f = tmp_path / "frames.json"
    f.write_text(json.dumps(cfg))
    # no GPU may be opened and no library loaded for these answers
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", SPH_HIP_LIB=str(tmp_path / "no_such_library.so"))
    return subprocess.run([sys.executable, os.path.join(ROOT, "sph_project_amd", "run_simulation.py"), "--scene_file", str(f),
                           "--output_dir", str(tmp_path / "o")] + args, capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)


@pytest.mark.parametrize("args,words", [
    (["--surface_foam", "--render_surface"], ("--surface_foam", "--foam")),
    (["--surface_foam", "--foam", "--render"], ("--surface_foam", "--render_surface")),
    (["--foam", "--render_surface", "--surface_foam_density", "2.0"], ("--surface_foam_density", "--surface_foam")),
    (["--foam", "--render_surface", "--surface_foam_bias", "0.5"], ("--surface_foam_bias", "--surface_foam")),
    (["--foam", "--render", "--render_surface"], ("--foam", "--render_surface", "--surface_foam")),   # still refused; the hint names the flag
])
def test_driver_refuses_bad_surface_foam_arguments(tmp_path, args, words):
    r = _driver(args, tmp_path)
    assert r.returncode == 2, r.stderr
    for word in words:
        assert word in r.stderr, r.stderr
    assert not (tmp_path / "o").exists()


def test_driver_lists_the_surface_foam_flags(tmp_path):
    r = _driver(["--help"], tmp_path)
    assert r.returncode == 0
    for flag in ("--surface_foam", "--surface_foam_density", "--surface_foam_bias"):
        assert flag in r.stdout
