"""GPU: the PNG encoder in coding="dynamic" (csrc/sph_png.hpp, DESIGN.md 21 'Dynamic blocks') against the test-owned encoder of
tests/png_dynamic_model.py, byte for byte, in both builds, with its counters; repeat; own pictures for the branches; a 1024 x 1024
picture checked by decoding and against the fixed coding's file; set_coding back and forth; a renderer's frame read in place; the
drivers' --png_coding."""
import ctypes
import json
import os

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd.png import PngEncoder, PngError, bound
from sph_project_amd.render import encode_png
from sph_project_amd.video import decode_png
from tests import png_dynamic_model as D
from tests import png_model as M
from tests.test_hip_video import _mesh_renderer, _particle_renderer
from tests.test_png_dynamic_host import dcase
from tests.test_png_host import case, kind_for
from tests.test_video_host import picture

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (37, 53), (86, 7)]   # width, height; (37, 53): two segments, the code-length limit in both; (86, 7): rows of 259 bytes
COUNTERS = ["raw_bytes", "zlib_bytes", "file_bytes", "segments", "stored_segments", "literals", "matches", "filter_rows",
            "dynamic_segments", "dynamic_header_bits"]


def same_counters(st, info):
    assert {k: st[k] for k in COUNTERS} == {k: info[k] for k in COUNTERS}


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("filt", ["adaptive", 0, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bytes_equal_the_model(gpu, size, filt, fast):
    img, want, info = dcase(kind_for(*size), size[0], size[1], filt)
    v = PngEncoder(size[0], size[1], filter=filt, coding="dynamic", fast_math=fast)
    got = v.encode(img)
    st = v.stats()
    print(f"{size} filter {filt} fast={fast}: {len(got)} bytes (model {len(want)}), modes {info['_modes']}, stats {st}")
    same_counters(st, info)
    assert got == want
    assert v.encode(img) == got   # a repeated call


@pytest.mark.parametrize("kind,width,height,filters", [("stripes", 100, 45, ("adaptive", 0)), ("black", 64, 64, ("adaptive", 0)),
                                                       ("flat", 256, 256, ("adaptive", 0)), ("period5", 2000, 1, (0,))])
def test_own_pictures_equal_the_model(gpu, kind, width, height, filters):
    """dynamic and stored segments in one file; matches of 258 with a single distance code; five literal values and no distance code"""
    for filt in filters:
        img, want, info = dcase(kind, width, height, filt)
        v = PngEncoder(width, height, filter=filt, coding="dynamic")
        got = v.encode(img)
        print(f"{kind} filter {filt}: {len(got)} bytes (model {len(want)}), modes {info['_modes']}, notes {info['_notes']}")
        assert got == want, (kind, filt)
        same_counters(v.stats(), info)


@pytest.mark.parametrize("fast", [False, True])
def test_mixed_640_has_all_three_modes(gpu, fast):
    img, want, info = dcase("mixed", 640, 480, "adaptive")
    modes = info["_modes"]
    assert info["segments"] == 226 and min(modes.count(m) for m in (0, 1, 2)) > 0
    v = PngEncoder(640, 480, coding="dynamic", fast_math=fast)
    got = v.encode(img)
    st = v.stats()
    print(f"mixed 640 x 480 fast={fast}: {len(got)} bytes (model {len(want)}, fixed {len(case('mixed', 640, 480, 'adaptive')[1])}), stats {st}")
    assert st["dynamic_segments"] == info["dynamic_segments"] == modes.count(2)
    same_counters(st, info)
    assert got == want


def test_discs_at_1024_decode_exactly_and_are_smaller_than_fixed(gpu):
    img = picture("discs", 1024, 1024, seed=2048)
    v = PngEncoder(1024, 1024, coding="dynamic")
    data = v.encode(img)
    st = v.stats()
    fixed = PngEncoder(1024, 1024).encode(img)
    print(f"discs 1024 x 1024: dynamic {len(data)} bytes, fixed {len(fixed)}, bound {bound(1024, 1024)}, host encoder {len(encode_png(img))}, stats {st}")
    M.check_file(data, img)   # zlib's own decoder, the Adler-32, every chunk CRC, the pixels
    assert len(data) == st["file_bytes"] <= bound(1024, 1024)
    assert len(data) < len(fixed)
    assert st["segments"] == 769 and 0 < st["dynamic_segments"] <= 769 and st["dynamic_header_bits"] > 0
    assert PngEncoder(1024, 1024, coding="dynamic", fast_math=True).encode(img) == data


def test_set_coding_switches_one_object_back_and_forth(gpu):
    img, want_dyn, info = dcase("mixed", 37, 53, "adaptive")
    _, want_fixed, info_fixed = case("mixed", 37, 53, "adaptive")
    v = PngEncoder(37, 53)
    assert v.coding == "fixed" and v.encode(img) == want_fixed
    st = v.stats()
    assert st["dynamic_segments"] == 0 and st["dynamic_header_bits"] == 0
    v.set_coding("dynamic")
    assert v.coding == "dynamic" and v.encode(img) == want_dyn
    same_counters(v.stats(), info)
    v.set_coding("fixed")
    assert v.encode(img) == want_fixed
    st = v.stats()
    assert st["dynamic_segments"] == 0 and {k: st[k] for k in ("literals", "matches", "stored_segments", "file_bytes")} == \
        {k: info_fixed[k] for k in ("literals", "matches", "stored_segments", "file_bytes")}
    with pytest.raises(ValueError):
        v.set_coding("best")
    assert v.lib.sph_png_set_coding(v.h, ctypes.c_int32(2)) == L.ERR_INVALID      # the library refuses it too, with a message
    assert b"coding" in v.lib.sph_png_last_error(v.h)
    assert v.encode(img) == want_fixed                                            # and the coding is what it was
    v.close()
    with pytest.raises(PngError, match="closed"):
        v.set_coding("dynamic")


@pytest.mark.parametrize("make", [_particle_renderer, _mesh_renderer], ids=["particles", "meshes"])
def test_encode_last_reads_the_renderers_frame_in_place(gpu, make):
    r = make()
    rgb, ids = r.last_rgb(), r.ids()
    assert (ids >= 0).sum() > 500
    v = PngEncoder(320, 240, coding="dynamic")
    a = v.encode_last(r)
    assert a == v.encode(rgb)
    info = {}
    assert a == D.encode(rgb, "adaptive", info)
    same_counters(v.stats(), info)
    M.check_file(a, rgb)
    assert info["dynamic_segments"] > 0 and len(a) < len(PngEncoder(320, 240).encode_last(r))
    assert r.last_rgb().tobytes() == rgb.tobytes() and r.ids().tobytes() == ids.tobytes()


def test_drivers_png_coding(gpu, tmp_path):
    from sph_project_amd import render_meshes, run_simulation
    cfg = P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2))
    cfg["Configuration"].update(exportFrame=True, exportPly=True, outputInterval=3)
    f = tmp_path / "frames.json"
    f.write_text(json.dumps(cfg))
    dyn, fix = tmp_path / "dyn", tmp_path / "fix"
    cam = ["--render_size", "320", "240", "--camera_position", "1.2", "0.8", "1.4", "--camera_lookat", "0.2", "0.2", "0.2"]
    common = ["--scene_file", str(f), "--max_steps", "4", "--render", "--render_meshes", "--reconstruct", "--video", "--png_device"] + cam
    c1, _ = run_simulation.main(common + ["--output_dir", str(dyn), "--png_coding", "dynamic"])
    c2, _ = run_simulation.main(common + ["--output_dir", str(fix)])
    for field in (L.F_POSITION, L.F_VELOCITY, L.F_PARTICLE_ID):
        assert c1.engine.download(field).tobytes() == c2.engine.download(field).tobytes()
    frames = sorted(d for d in os.listdir(fix) if (fix / d).is_dir())
    assert frames == ["000000", "000003"] and sorted(os.listdir(dyn)) == sorted(os.listdir(fix))
    for d in frames:
        for name in ("raw_view.png", "render.png"):
            a, b = (dyn / d / name).read_bytes(), (fix / d / name).read_bytes()
            px = decode_png(b)
            assert px.shape == (240, 320, 3) and px.any()
            M.check_file(a, px)                              # the same pixels from a valid file
            assert b == M.encode(px)                         # without --png_coding: the fixed coding's bytes, as before
            assert a == D.encode(px) and len(a) <= len(b)
    for name in ("raw_view.avi", "render.avi"):
        assert (dyn / name).read_bytes() == (fix / name).read_bytes(), name
    assert render_meshes.main(["--input_dir", str(dyn), "--scene_file", str(f), "--rendered_image_name", "again.png", "--png_device",
                               "--png_coding", "dynamic"] + cam) == 2
    for d in frames:
        assert (dyn / d / "again.png").read_bytes() == (dyn / d / "render.png").read_bytes(), d
