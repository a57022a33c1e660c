"""CPU: particle rendering without a GPU -- the PNG writer, the geometry of the float64 model (tests/render_model.py), the
C-ABI mirror, parameter checks before any device is touched, and the driver's flags."""
import ctypes
import os
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import render as R
from tests import render_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        out.append((tag, body))
        pos += 12 + n
    return out


def decode_png(data):
    """uint8 (H, W, 3) of an 8-bit RGB PNG whose rows all use filter 0 (what write_png writes)."""
    ch = _chunks(data)
    assert ch[0][0] == b"IHDR" and ch[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", ch[0][1])
    assert (depth, ctype, comp, filt, inter) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in ch if t == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def test_png_writer_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    p = tmp_path / "f.png"
    R.write_png(str(p), img)
    data = p.read_bytes()
    ch = _chunks(data)
    assert [t for t, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">II", ch[0][1][:8]) == (53, 37)
    assert np.array_equal(decode_png(data), img)
    with pytest.raises(ValueError):
        R.encode_png(np.zeros((4, 4), np.uint8))


# --- the model's geometry --------------------------------------------------------------------------------------------------------

CAM = dict(eye=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=60.0)


def _centroid(m):
    j, i = np.nonzero(m["ids"] >= 0)
    return i.mean(), j.mean(), len(i)


def test_model_right_is_plus_s_and_up_is_plus_u():
    W = H = 128
    E, f, s, u, tx, ty = RM.camera(CAM["eye"], CAM["target"], CAM["up"], CAM["fov"], W, H)
    assert np.allclose(s, [1, 0, 0]) and np.allclose(u, [0, 1, 0]) and np.allclose(f, [0, 0, -1])
    ci, cj, _ = _centroid(RM.render([[0.5, 0, 0]], 0.05, W=W, H=H, **CAM))
    assert ci > W / 2 + 5 and abs(cj - (H - 1) / 2) < 0.5
    ci, cj, _ = _centroid(RM.render([[0, 0.5, 0]], 0.05, W=W, H=H, **CAM))
    assert cj < H / 2 - 5 and abs(ci - (W - 1) / 2) < 0.5   # above the centre: smaller row index (rows from the top)


def test_model_disc_has_the_analytic_radius_and_t_is_the_view_depth():
    W = H = 512
    r, D = 0.2, 3.0
    m = RM.render([[0, 0, 0]], r, W=W, H=H, **CAM)
    _, _, npx = _centroid(m)
    # the sphere's silhouette is a circle of angular radius asin(r / D): on the image plane tan(asin(r/D)) = r / sqrt(D^2 - r^2)
    rad_px = r / np.sqrt(D * D - r * r) / np.tan(np.radians(CAM["fov"] / 2)) * (H / 2)
    assert abs(npx - np.pi * rad_px ** 2) < 2 * np.pi * rad_px * 1.0, (npx, np.pi * rad_px ** 2)
    # t at the centre pixel pair is the view depth of the front of the sphere: D - r (f . d = 1)
    E, f, s, u, tx, ty = RM.camera(CAM["eye"], CAM["target"], CAM["up"], CAM["fov"], W, H)
    X, Y = RM.pixel_rays(W, H, tx, ty)
    d = f + X[W // 2] * s + Y[H // 2] * u
    c = np.zeros(3)
    b = d @ (c - E)
    disc = b * b - (d @ d) * ((c - E) @ (c - E) - r * r)
    t = (b - np.sqrt(disc)) / (d @ d)
    P = E + t * d
    assert abs((P - E) @ f - t) < 1e-12 and abs(t - (D - r)) < 1e-3
    assert abs(np.linalg.norm(P - c) - r) < 1e-12


def test_model_nearer_sphere_wins_and_ids_break_nothing():
    W = H = 64
    x = np.array([[0, 0, 0], [0, 0, 0.5]], np.float32)
    m = RM.render(x, 0.3, ids=[7, 3], W=W, H=H, **CAM)
    assert m["ids"][H // 2, W // 2] == 3
    m2 = RM.render(x[::-1], 0.3, ids=[3, 7], W=W, H=H, **CAM)
    assert np.array_equal(m["ids"], m2["ids"]) and np.array_equal(m["rgb"], m2["rgb"])


def test_model_box_lines_and_non_finite_particles():
    W = H = 96
    m = RM.render(np.array([[np.nan, 0, 0], [0, 0, 0]], np.float32), 0.1, W=W, H=H, box=((-1, -1, -1), (1, 1, 1)), **CAM)
    ids = m["ids"]
    assert set(np.unique(ids[ids <= -2])) <= set(range(-13, -1)) and (ids <= -2).sum() > 4 * W
    assert (ids >= 0).sum() > 0 and set(np.unique(ids[ids >= 0])) == {1}
    assert (m["rgb"][ids <= -2] == RM.BOX_RGB).all() and (m["rgb"][ids == -1] == 0).all()


# --- C-ABI -----------------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["sph_render_create", "sph_render_destroy", "sph_render_last_error", "sph_render_points", "sph_render_handle",
               "sph_render_download", "sph_render_stats"]


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header and name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("struct_name", ["SphRenderParams", "SphRenderStats"])
def test_render_structs_match_the_header(struct_name):
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


def test_create_refuses_bad_parameters_before_touching_a_device():
    lib = L.load()
    h = ctypes.c_void_p()
    bads = (dict(width=0), dict(height=-3), dict(width=16385), dict(width=16384, height=8192), dict(fov_deg=0.0), dict(fov_deg=180.0),
            dict(z_near=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(ambient=-0.1), dict(eye=(-1.0, 0.0, 0.0)),
            dict(up=(6.5, 2.5, 4.0)), dict(background_rgb=(0, 256, 0)), dict(box_rgb=(-1, 0, 0)), dict(reserved=1),
            dict(draw_box=1, box_hi=(float("inf"), 1.0, 1.0)))
    for bad in bads:
        kw = dict(width=64, height=48, eye=(5.5, 2.5, 4.0), target=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=70.0, z_near=0.1,
                  radius=0.01, light_pos=(2.0, 2.0, 2.0), light_rgb=(1.0, 1.0, 1.0), ambient=0.1, background_rgb=(0, 0, 0), draw_box=0,
                  box_lo=(0.0, 0.0, 0.0), box_hi=(1.0, 1.0, 1.0), box_rgb=(252, 173, 71), fast_math=0, device=-1, reserved=0)
        kw.update(bad)
        p = L.SphRenderParams()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        assert lib.sph_render_create(ctypes.byref(p), ctypes.byref(h)) == -1, bad   # SPH_ERR_INVALID
        assert not h.value
        assert lib.sph_render_last_error(None)


def test_driver_has_the_render_flags():
    from sph_project_amd import run_simulation
    src = open(run_simulation.__file__).read()
    for flag in ('"--render"', '"--render_size"', '"--camera_position"', '"--camera_lookat"', '"--camera_fov"'):
        assert flag in src, flag
    assert "raw_view.png" in src
