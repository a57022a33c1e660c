"""CPU: the PNG stream without a GPU -- the test-owned encoder of tests/png_model.py read back by zlib, PIL and
video.decode_png with every checksum redone, every branch of the stream shown to be taken on the model's own counters, the size caps,
and the library's host side: symbols, struct layout, sph_png_bound, parameter checks before any device is touched, the command lines."""
import ctypes
import functools
import io
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import png as PNG
from sph_project_amd.render import encode_png
from tests import png_model as M
from tests.test_video_host import picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flat(width, height, colour=(0, 0, 0)):
    return np.broadcast_to(np.asarray(colour, np.uint8), (height, width, 3)).copy()


def stripes(width, height):
    """Own picture: a flat top (rows of zeros after Up: matches of 258), vertical stripes of period 2 pixels (distance 6 under filter 0),
    noise at the bottom (literals, a stored segment)."""
    img = np.zeros((height, width, 3), np.uint8)
    img[: height // 3] = (30, 60, 90)
    img[height // 3: 2 * height // 3, ::2] = (200, 10, 10)
    img[height // 3: 2 * height // 3, 1::2] = (10, 200, 10)
    img[2 * height // 3:] = np.random.default_rng(5).integers(0, 256, (height - 2 * height // 3, width, 3), dtype=np.uint8)
    return img


def make_picture(kind, width, height):
    if kind == "flat":
        return flat(width, height, (77, 77, 77))
    if kind == "black":
        return flat(width, height)
    if kind == "stripes":
        return stripes(width, height)
    return picture(kind, width, height, seed=width + height)


def kind_for(width, height):
    return "noise" if width * height < 10 else "lines" if height < 10 else "mixed"


@functools.lru_cache(maxsize=None)
def case(kind, width, height, filt):
    """picture, the model's file, the model's counters (computed once, shared with tests/test_hip_png.py; treat as read-only)"""
    img = make_picture(kind, width, height)
    info = {}
    data = M.encode(img, filt, info)
    img.setflags(write=False)
    return img, data, info


CASES = [("noise", 1, 1), ("noise", 3, 2), ("mixed", 37, 53), ("lines", 86, 7), ("stripes", 100, 45), ("black", 64, 64),
         ("flat", 256, 256), ("mixed", 640, 480)]
FILTERS = ["adaptive", 0, 1, 2, 3, 4]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("kind,width,height", CASES[:-1])
def test_model_files_decode_exactly_and_their_checksums_hold(kind, width, height, filt):
    img, data, info = case(kind, width, height, filt)
    raw = M.check_file(data, img)   # zlib, Adler-32, every chunk CRC, video.decode_png
    assert info["raw_bytes"] == len(raw) == height * (1 + 3 * width)
    assert info["file_bytes"] == len(data) <= M.bound(width, height)
    assert sum(info["filter_rows"]) == height
    if filt != "adaptive":
        assert info["filter_rows"][filt] == height and set(raw[:: 1 + 3 * width]) == {filt}
    ch = M.chunks(data)
    assert len(ch) == info["segments"] + 3 and info["zlib_bytes"] == sum(len(c[1]) for c in ch[1:-1])
    Image = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), img)


def test_the_large_mixed_picture_decodes_and_takes_every_branch():
    img, data, info = case("mixed", 640, 480, "adaptive")
    M.check_file(data, img)
    assert all(n > 0 for n in info["filter_rows"]), info["filter_rows"]                  # every filter type wins a row
    assert 0 < info["stored_segments"] < info["segments"] == 226                          # fixed and stored in one picture
    assert info["_longest"] == 258 and info["_first_last"]
    assert info["literals"] > 0 and info["matches"] > 0
    assert len(data) <= M.bound(640, 480)


def test_small_pictures_take_the_branches_too():
    _, _, info = case("mixed", 37, 53, "adaptive")      # a row of 112 bytes: no multiple of anything
    assert all(n > 0 for n in info["filter_rows"]) and info["segments"] == 2
    _, _, info = case("mixed", 37, 53, 0)
    assert info["stored_segments"] == 1 and info["segments"] == 2
    _, _, info = case("black", 64, 64, "adaptive")      # all zeros: literal, then matches of 258 from byte 1 to the segment's last byte
    assert info["_longest"] == 258 and info["_first_last"] and info["literals"] == info["segments"] == 4
    assert info["filter_rows"] == [64, 0, 0, 0, 0]      # all costs are 0: the lowest type
    _, _, info = case("lines", 86, 7, 0)                # a filtered row of 259 bytes, one past the longest match
    assert info["raw_bytes"] == 7 * 259
    _, _, info = case("noise", 1, 1, "adaptive")
    assert (info["segments"], info["literals"], info["matches"]) == (1, 4, 0)


def test_the_token_rule_on_a_hand_made_stream():
    """DESIGN.md 21 on bytes small enough to parse by hand."""
    b = np.array([5, 5, 5, 5, 5, 9, 1, 2, 3, 1, 2, 3, 1, 2, 7, 7], np.uint8)
    ln, ds = M.match_lengths(b)
    assert (ln[1], ds[1]) == (4, 1)             # 5 5 5 5 behind the first 5
    assert (ln[9], ds[9]) == (5, 3)             # 1 2 3 1 2 repeats at distance 3 (and at 6 from position 12 on: shorter)
    assert ln[0] == 0 and ln[5] == 0 and ln[14] == 0 and ln[15] == 0   # 7 7: a run of 1 is below the minimum
    long = np.zeros(600, np.uint8)
    ln, ds = M.match_lengths(long)
    assert ln[1] == 258 and ds[1] == 1 and ln[341] == 258 and ln[342] == 258 and ln[343] == 257 and ln[599] == 0 and ln[597] == 3
    two = np.zeros(M.SEG + 10, np.uint8)
    ln, _ = M.match_lengths(two)
    assert ln[M.SEG] == 0 and ln[M.SEG - 3] == 3 and ln[M.SEG - 2] == 0 and ln[M.SEG + 1] == 9   # nothing crosses a segment's start


def test_size_caps():
    for kind, w, h in CASES:
        for filt in ("adaptive", 0, 2):
            _, data, _ = case(kind, w, h, filt)
            assert len(data) <= M.bound(w, h) == PNG.bound(w, h), (kind, w, h, filt)
    img, data, info = case("flat", 256, 256, "adaptive")
    print(f"256 x 256 of one colour: {len(data)} bytes (cap {196864 // 32}, the host encoder {len(encode_png(img))})")
    assert info["raw_bytes"] == 196864 and len(data) <= 196864 // 32
    # noise cannot be compressed: every full segment is stored, and the file stays between the raw size and the bound
    rnd = picture("noise", 200, 41, seed=3)
    info = {}
    data = M.encode(rnd, 0, info)
    assert info["stored_segments"] >= info["segments"] - 1 == 6 and info["raw_bytes"] < len(data) <= M.bound(200, 41)


# --- the library, without a device ---------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["sph_png_create", "sph_png_destroy", "sph_png_last_error", "sph_png_bound", "sph_png_encode_rgb", "sph_png_encode_render",
               "sph_png_size", "sph_png_download", "sph_png_stats"]


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header and name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("struct_name", ["SphPngParams", "SphPngStats"])
def test_png_structs_match_the_header(struct_name):
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


def test_bound_is_the_documented_formula():
    lib = L.load()
    for w, h in ((1, 1), (3, 2), (37, 53), (86, 7), (640, 480), (1024, 1024), (16384, 4096), (4096, 16384)):
        raw = h * (1 + 3 * w)
        want = 8 + 25 + 17 * -(-raw // 4096) + raw + 2 + 16 + 12
        n = ctypes.c_int64()
        p = L.SphPngParams(width=w, height=h, filter=-1, fast_math=0, device=-1, reserved=0)
        assert lib.sph_png_bound(ctypes.byref(p), ctypes.byref(n)) == 0
        assert n.value == want == M.bound(w, h) == PNG.bound(w, h), (w, h)
    p = L.SphPngParams(width=0, height=4, filter=-1, fast_math=0, device=-1, reserved=0)
    assert lib.sph_png_bound(ctypes.byref(p), ctypes.byref(n)) == -1 and lib.sph_png_last_error(None)


def test_create_refuses_bad_parameters_before_touching_a_device():
    lib = L.load()
    h = ctypes.c_void_p()
    for bad in (dict(width=0), dict(height=-1), dict(width=16385), dict(width=16384, height=8192), dict(filter=-2), dict(filter=5),
                dict(reserved=1)):
        kw = dict(width=64, height=48, filter=-1, fast_math=0, device=-1, reserved=0)
        kw.update(bad)
        p = L.SphPngParams(**kw)
        assert lib.sph_png_create(ctypes.byref(p), ctypes.byref(h)) == -1, bad   # SPH_ERR_INVALID
        assert not h.value
        assert lib.sph_png_last_error(None)
    for bad in ("best", 5, -1, 1.5):
        with pytest.raises(ValueError):
            PNG.PngEncoder.__init__(object.__new__(PNG.PngEncoder), 8, 8, filter=bad)
    assert lib.sph_png_encode_rgb(None, None) == -1 and lib.sph_png_size(None, None) == -1 and lib.sph_png_download(None, None) == -1


def test_both_command_lines_carry_the_flag():
    from sph_project_amd import render_meshes, run_simulation
    a = run_simulation.parse_args(["--scene_file", "x.json", "--render", "--png_device"])
    assert a.png_device and not run_simulation.parse_args(["--scene_file", "x.json", "--render"]).png_device
    with pytest.raises(SystemExit):   # the flag needs a renderer whose frames it compresses
        run_simulation.parse_args(["--scene_file", "x.json", "--png_device"])
    assert render_meshes.parse_args(["--input_dir", "d", "--scene_file", "s.json", "--png_device"]).png_device
    assert not render_meshes.parse_args(["--input_dir", "d", "--scene_file", "s.json"]).png_device
