"""CPU: the video stream without a GPU -- the test-owned encoder and decoder of tests/jpeg_model.py against the float64
transform (the coefficient bound), against PIL where it is installed, the library's fixed headers against the model's, the AVI muxer
read back by a RIFF parser, the PNG reader, the C-ABI mirror, parameter checks before any device is touched, and both command lines."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import video as V
from sph_project_amd.render import encode_png
from tests import jpeg_model as JM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# DESIGN.md 18, "the error bound": with A = 2 sqrt 2 the largest absolute row sum of the DCT matrix, e_s the sample error of the integer
# colour matrix (255 x its largest row error / 2^16, + 2^-17 for the 4:2:0 mean), samples below 128, row-pass values below 128 A:
#   delta <= A^2 e_s + A (8 x 128 x 2^-21 + 2^-17) + 8 x 128 A x 2^-21 + 2^-17  =  0.0230 + 0.0014 + 0.0014  <  0.03
DELTA = 0.03


def picture(kind, width, height, seed=0):
    """Synthetic uint8 (height, width, 3): 'discs' shaded discs on black with a one-pixel box line (a particle frame), 'lines'
    one-pixel lines, 'gradient', 'noise', 'mixed' (a quarter of each)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    if kind == "noise":
        return rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    if kind == "gradient":
        return np.stack([x * 255 // max(width - 1, 1), y * 255 // max(height - 1, 1), (x + y) * 255 // max(width + height - 2, 1)], axis=2).astype(np.uint8)
    img = np.zeros((height, width, 3), np.uint8)
    if kind == "lines":
        img[:, ::7] = (252, 173, 71)
        img[::5, :] = (40, 200, 255)
        d = np.arange(min(width, height))
        img[d, d] = (255, 255, 255)
        return img
    if kind == "discs":
        n = max(3, width * height // 600)
        r = max(2.0, min(width, height) / 90)
        for cx, cy, col in zip(rng.uniform(0, width, n), rng.uniform(0.3 * height, height, n), rng.integers(40, 256, (n, 3))):
            x0, x1, y0, y1 = int(max(cx - r, 0)), int(min(cx + r + 1, width)), int(max(cy - r, 0)), int(min(cy + r + 1, height))
            if x0 >= x1 or y0 >= y1:
                continue
            d2 = ((x[y0:y1, x0:x1] - cx) ** 2 + (y[y0:y1, x0:x1] - cy) ** 2) / (r * r)
            shade = np.sqrt(np.clip(1.0 - d2, 0.0, 1.0))[..., None]
            patch = img[y0:y1, x0:x1]
            patch[...] = np.where(d2[..., None] < 1.0, (0.1 + 0.9 * shade) * col, patch).astype(np.uint8)
        img[height // 8, :] = (252, 173, 71)
        return img
    assert kind == "mixed"
    h2, w2 = height // 2, width // 2
    img[:h2, :w2] = picture("discs", w2, h2, seed)
    img[:h2, w2:] = picture("lines", width - w2, h2, seed)
    img[h2:, :w2] = picture("gradient", w2, height - h2, seed)
    img[h2:, w2:] = picture("noise", width - w2, height - h2, seed)
    return img


KINDS = ["discs", "lines", "gradient", "noise"]


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def test_delta_is_what_the_formats_give():
    exact = np.array([[0.299, 0.587, 0.114], [-0.299 / 1.772, -0.587 / 1.772, 0.5], [0.5, -0.587 / 1.402, -0.114 / 1.402]]) * 65536
    e_s = 255 * np.abs(exact - JM.COLOUR).sum(axis=1).max() / 65536 + 2.0 ** -17
    c = JM.dct_matrix_float()
    A = np.abs(c).sum(axis=1).max()
    assert abs(A - 2 * np.sqrt(2)) < 1e-12
    assert np.abs(c * (1 << JM.COS_BITS) - JM.DCT_INT).max() <= 0.5 and JM.COS_BITS == 20 and JM.SAMPLE_BITS == 16
    bound = A * A * e_s + A * (8 * 128 * 2.0 ** -21 + 2.0 ** -17) + 8 * 128 * A * 2.0 ** -21 + 2.0 ** -17
    print(f"e_s = {e_s:.6f}, derived bound = {bound:.5f}, DELTA = {DELTA}")
    assert bound <= DELTA < 0.5
    assert JM.COLOUR.sum(axis=1).tolist() == [65536, 0, 0]


@pytest.mark.parametrize("chroma", ["420", "444"])
@pytest.mark.parametrize("quality", [50, 90, 100])
def test_decoded_coefficients_are_within_half_a_step_of_the_float_transform(quality, chroma):
    worst = -1.0
    for kind in KINDS:
        img = picture(kind, 53, 37, seed=quality)
        info = {}
        data = JM.encode(img, quality, chroma, info)
        d = JM.decode(data)
        assert (d["width"], d["height"], d["chroma"], d["restart_interval"]) == (53, 37, chroma, JM.RESTART_MCUS)
        assert d["intervals"] == info["restart_intervals"]
        ref = JM.reference_coefficients(img, chroma)
        for c in range(3):
            assert d["coef"][c].shape == ref[c].shape
            excess = np.abs(d["coef"][c] - ref[c]) - d["quant"][c] / 2
            worst = max(worst, float(excess.max()))
            assert (excess <= DELTA).all(), (kind, c, float(excess.max()))
        assert d["rgb"].shape == img.shape
    print(f"q{quality} {chroma}: largest |dequantised - float DCT| - q/2 = {worst:.5f} (DELTA {DELTA})")


def test_stuffing_restart_wrap_and_sizes_in_the_model():
    img = picture("noise", 160, 96, seed=1)
    info = {}
    data = JM.encode(img, 100, "444", info)
    assert info["stuffed_bytes"] > 0 and info["restart_intervals"] == 30 and info["blocks"] == 20 * 12 * 3
    scan = data[len(JM.header(160, 96, 100, "444")):-2]
    assert len(scan) == info["scan_bytes"] and scan.count(b"\xff\x00") == info["stuffed_bytes"]
    assert np.array_equal(JM.decode(data)["rgb"].shape, img.shape)
    for w, h in ((1, 1), (8, 8), (17, 9)):
        d = JM.decode(JM.encode(picture("noise", w, h), 90, "420"))
        assert d["rgb"].shape == (h, w, 3)


@pytest.mark.parametrize("chroma", ["420", "444"])
@pytest.mark.parametrize("quality", [50, 90, 100])
def test_pil_decodes_every_stream_and_the_psnr_matches_its_own_encoder(quality, chroma):
    Image = pytest.importorskip("PIL.Image")
    for kind in KINDS:
        img = picture(kind, 96, 80, seed=3)
        data = JM.encode(img, quality, chroma)
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (96, 80) and im.mode == "RGB" and im.format == "JPEG"
        ours = _psnr(np.asarray(im), img)
        bio = io.BytesIO()
        Image.fromarray(img).save(bio, "JPEG", quality=quality, subsampling={"420": 2, "444": 0}[chroma])
        theirs = _psnr(np.asarray(Image.open(io.BytesIO(bio.getvalue()))), img)
        print(f"{kind} q{quality} {chroma}: PSNR of PIL's decode of our stream {ours:.2f} dB, of PIL's own encode {theirs:.2f} dB")
        assert ours >= theirs - 0.5, (kind, ours, theirs)
        # PIL's tables at this quality are the model's (the IJG rule on Annex K)
        pil_q = Image.open(io.BytesIO(bio.getvalue())).quantization
        for k, t in enumerate(JM.quant_tables(quality)):
            assert sorted(pil_q[k]) == sorted(int(v) for v in t)


def test_library_header_equals_the_model_header():
    lib = L.load()
    for w, h, q, chroma in ((1024, 1024, 90, "420"), (37, 53, 50, "444"), (1, 1, 100, "420"), (16384, 4096, 1, "444")):
        p = L.SphVideoParams(width=w, height=h, quality=q, chroma=int(chroma), fast_math=0, device=-1, reserved=0)
        n = ctypes.c_int64()
        assert lib.sph_video_header(ctypes.byref(p), None, ctypes.byref(n)) == 0
        buf = ctypes.create_string_buffer(n.value)
        assert lib.sph_video_header(ctypes.byref(p), buf, ctypes.byref(n)) == 0
        assert buf.raw == JM.header(w, h, q, chroma)


# --- AVI ---------------------------------------------------------------------------------------------------------------------------

def _riff(data, pos, end):
    """[(tag, list type or None, payload offset, payload size, children)]"""
    out = []
    while pos < end:
        tag, n = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        assert pos + 8 + n <= end, (tag, pos, n, end)
        if tag in (b"RIFF", b"LIST"):
            out.append((tag, data[pos + 8:pos + 12], pos + 12, n - 4, _riff(data, pos + 12, pos + 8 + n)))
        else:
            out.append((tag, None, pos + 8, n, []))
        pos += 8 + n + (n & 1)
    assert pos == end or pos == end + 1
    return out


def avi_frames(data):
    """The frames of a Motion-JPEG AVI and its header fields, with every structural check of the container."""
    top = _riff(data, 0, len(data))
    assert len(top) == 1 and top[0][0] == b"RIFF" and top[0][1] == b"AVI " and top[0][3] + 12 == len(data)
    kids = top[0][4]
    assert [(k[0], k[1]) for k in kids] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl, movi, idx1 = kids
    assert [(k[0], k[1]) for k in hdrl[4]] == [(b"avih", None), (b"LIST", b"strl")]
    avih = struct.unpack("<14I", data[hdrl[4][0][2]:hdrl[4][0][2] + hdrl[4][0][3]])
    strl = hdrl[4][1][4]
    assert [k[0] for k in strl] == [b"strh", b"strf"]
    strh = struct.unpack("<4s4sIHHIIIIIIII4H", data[strl[0][2]:strl[0][2] + strl[0][3]])
    strf = struct.unpack("<IiiHH4sIiiII", data[strl[1][2]:strl[1][2] + strl[1][3]])
    assert strh[0] == b"vids" and strh[1] == b"MJPG" and strf[5] == b"MJPG" and strf[0] == 40 and strf[4] == 24
    frames = []
    for k in movi[4]:
        assert k[0] == b"00dc"
        frames.append(data[k[2]:k[2] + k[3]])
        assert k[2] % 2 == 0, "chunks start on even offsets"
    n = len(frames)
    assert avih[4] == n and strh[9] == n and avih[6] == 1 and avih[3] & 0x10
    assert idx1[3] == 16 * n
    movi_tag = movi[2] - 4
    for i in range(n):
        tag, flags, off, size = struct.unpack("<4sIII", data[idx1[2] + 16 * i:idx1[2] + 16 * i + 16])
        at = movi_tag + off
        assert tag == b"00dc" and flags & 0x10 and data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == size
        payload = data[at + 8:at + 8 + size]
        assert payload == frames[i] and payload[:2] == b"\xff\xd8" and payload[-2:] == b"\xff\xd9"
    biggest = max((len(f) for f in frames), default=0)
    assert avih[7] >= biggest and strh[10] >= biggest
    return frames, dict(usec_per_frame=avih[0], width=avih[8], height=avih[9], scale=strh[6], rate=strh[7], strf_size=(strf[1], strf[2]),
                        frame_rect=strh[-2:])


def test_avi_round_trip_tree_sizes_index_and_padding(tmp_path):
    streams = [JM.encode(picture("noise", 8, 8, seed=k), 90, "444") for k in range(1, 12)]
    even = next(x for x in streams if len(x) % 2 == 0)
    odd = next(x for x in streams if len(x) % 2 == 1)
    payloads = [even, odd, odd, even]   # both parities: odd chunks are padded
    assert {len(p) % 2 for p in payloads} == {0, 1}
    path = tmp_path / "t.avi"
    with V.AviWriter(str(path), 8, 8, 25) as w:
        for p in payloads:
            w.add(p)
    data = path.read_bytes()
    frames, info = avi_frames(data)
    assert frames == payloads
    assert info == dict(usec_per_frame=40000, width=8, height=8, scale=1, rate=25, strf_size=(8, 8), frame_rect=(8, 8))
    assert len(data) % 2 == 0
    # an empty file is still a well-formed AVI
    with V.AviWriter(str(tmp_path / "e.avi"), 8, 8, 20):
        pass
    assert avi_frames((tmp_path / "e.avi").read_bytes())[0] == []
    with pytest.raises(ValueError):
        V.AviWriter(str(tmp_path / "bad.avi"), 8, 8, 0)


def test_avi_refuses_to_pass_two_gib(tmp_path):
    assert V.AVI_LIMIT == 2 ** 31 - 1
    jpg = JM.encode(picture("noise", 8, 8), 90, "444")
    path = tmp_path / "limit.avi"
    w = V.AviWriter(str(path), 8, 8, 20, limit=V.AVI_LIMIT)
    w.add(jpg)
    w.size = V.AVI_LIMIT - len(jpg) - 20   # as if 2 GiB of frames had been written already
    with pytest.raises(V.VideoError, match="classic AVI"):
        w.add(jpg)
    assert w.frames == 1
    w.close()
    small = V.AviWriter(str(tmp_path / "s.avi"), 8, 8, 20, limit=2000)
    small.add(jpg)
    with pytest.raises(V.VideoError):
        for _ in range(5):
            small.add(jpg)
    small.close()
    got, _ = avi_frames((tmp_path / "s.avi").read_bytes())
    assert got and all(f == jpg for f in got) and os.path.getsize(tmp_path / "s.avi") <= 2000


# --- PNG reader ----------------------------------------------------------------------------------------------------------------------

def test_decode_png_reads_what_encode_png_writes():
    img = picture("mixed", 53, 37, seed=4)
    assert np.array_equal(V.decode_png(encode_png(img)), img)
    with pytest.raises(ValueError, match="not a PNG"):
        V.decode_png(b"\xff\xd8 no png")
    bad = bytearray(encode_png(img))
    bad[40] ^= 1
    with pytest.raises(ValueError, match="CRC"):
        V.decode_png(bytes(bad))


def test_decode_png_against_pil_files():
    Image = pytest.importorskip("PIL.Image")
    img = picture("mixed", 61, 45, seed=5)

    def save(im, **kw):
        bio = io.BytesIO()
        im.save(bio, "PNG", **kw)
        return bio.getvalue()
    rgb_png = save(Image.fromarray(img), optimize=True)   # adaptive row filters
    raw = np.frombuffer(__import__("zlib").decompress(b"".join(b for t, b in V._png_chunks(rgb_png) if t == b"IDAT")), np.uint8)
    assert len(set(raw.reshape(45, 1 + 3 * 61)[:, 0].tolist())) > 1, "PIL chose one filter only: the adaptive case is not exercised"
    assert np.array_equal(V.decode_png(rgb_png), img)
    rgba = np.dstack([img, np.full(img.shape[:2], 77, np.uint8)])
    assert np.array_equal(V.decode_png(save(Image.fromarray(rgba, "RGBA"))), img)
    grey = img[:, :, 1]
    assert np.array_equal(V.decode_png(save(Image.fromarray(grey, "L"))), np.repeat(grey[:, :, None], 3, axis=2))
    # every filter type, written by hand: PIL's choice above need not contain all five
    for ft in range(5):
        assert np.array_equal(V.decode_png(_png_with_filter(img, ft)), img), ft
    with pytest.raises(ValueError, match="palette"):
        V.decode_png(save(Image.fromarray(img).convert("P")))
    with pytest.raises(ValueError, match="bit depth 16"):
        V.decode_png(save(Image.fromarray(grey.astype(np.uint16) * 257)))
    with pytest.raises(ValueError, match="interlace"):
        V.decode_png(_interlaced(rgb_png))


def _png_with_filter(img, ft):
    """An RGB PNG whose rows all use filter type ft (written from the PNG specification's definitions)."""
    from sph_project_amd.render import _chunk
    h, w = img.shape[:2]
    a = img.reshape(h, 3 * w).astype(np.int64)
    rows = []
    for y in range(h):
        cur = a[y]
        up = a[y - 1] if y else np.zeros_like(cur)
        left = np.concatenate([np.zeros(3, np.int64), cur[:-3]])
        upleft = np.concatenate([np.zeros(3, np.int64), up[:-3]])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) // 2
        else:
            p = left + up - upleft
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        rows.append(bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes())
    import zlib
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(b"".join(rows)))
            + _chunk(b"IEND", b""))


def _interlaced(png):
    """The same file with the IHDR interlace byte set (and its CRC redone): must be refused by name, whatever the data."""
    from sph_project_amd.render import _chunk
    body = bytearray(png[16:29])
    body[12] = 1
    return png[:8] + _chunk(b"IHDR", bytes(body)) + png[33:]


# --- C-ABI and command lines ---------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["sph_video_create", "sph_video_destroy", "sph_video_last_error", "sph_video_header", "sph_video_encode_rgb",
               "sph_video_encode_render", "sph_video_size", "sph_video_download", "sph_video_stats"]


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header and name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("struct_name", ["SphVideoParams", "SphVideoStats"])
def test_video_structs_match_the_header(struct_name):
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
    for bad in (dict(width=0), dict(height=-1), dict(width=16385), dict(width=16384, height=8192), dict(quality=0), dict(quality=101),
                dict(chroma=422), dict(chroma=0), dict(reserved=1)):
        kw = dict(width=64, height=48, quality=90, chroma=420, fast_math=0, device=-1, reserved=0)
        kw.update(bad)
        p = L.SphVideoParams(**kw)
        assert lib.sph_video_create(ctypes.byref(p), ctypes.byref(h)) == -1, bad   # SPH_ERR_INVALID
        assert not h.value
        assert lib.sph_video_last_error(None)
    with pytest.raises(ValueError):
        V.VideoEncoder.__init__(object.__new__(V.VideoEncoder), 8, 8, chroma="422")


def test_both_command_lines_carry_their_flags(tmp_path):
    from sph_project_amd import make_video, run_simulation
    src = open(run_simulation.__file__).read()
    for flag in ('"--video"', '"--video_fps"', '"--video_quality"', '"--video_chroma"'):
        assert flag in src, flag
    assert "raw_view.avi" in src and "render.avi" in src
    a = run_simulation.parse_args(["--scene_file", "x.json", "--render", "--video"])
    assert a.video and a.video_fps == 20 and a.video_chroma == "420"
    with pytest.raises(SystemExit):   # --video needs a renderer to take its frames from
        run_simulation.parse_args(["--scene_file", "x.json", "--video"])
    m = make_video.parse_args(["--input_dir", "d", "--output_path", "o.avi"])
    assert (m.image_name, m.fps, m.chroma) == ("raw_view.png", 20, "420") and 1 <= m.quality <= 100
    with pytest.raises(SystemExit):
        make_video.parse_args(["--output_path", "o.avi"])
    with pytest.raises(SystemExit) as e:
        make_video.main(["--input_dir", str(tmp_path), "--output_path", str(tmp_path / "o.mp4")])
    assert "avi" in str(e.value).lower() and not (tmp_path / "o.mp4").exists()
    # frame directories in integer order; everything else in the directory is left alone
    for name in ("10", "9", "000002", "notes", "raw_view.avi"):
        (tmp_path / name).mkdir()
    assert make_video.frame_directories(str(tmp_path)) == ["000002", "9", "10"]
