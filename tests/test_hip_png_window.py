"""GPU: the PNG encoder in coding="window" (csrc/sph_png.hpp, DESIGN.md 21 'Window matches') against the test-owned encoder of
tests/png_window_model.py: the candidates of the whole stream exactly, the file byte for byte with its counters, in both builds; the
other codings' bytes unchanged beside a window encoder and on one encoder switched back and forth; a 1024 x 1024 picture checked by
decoding and against the dynamic coding's file; the driver's --png_coding window."""
import json
import os

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd.png import NO_CANDIDATE, PngEncoder, PngError, bound
from sph_project_amd.video import decode_png
from tests import png_dynamic_model as D
from tests import png_model as M
from tests import png_window_model as W
from tests.test_png_dynamic_host import dcase
from tests.test_png_host import case
from tests.test_png_window_host import CASES, COUNTERS, FILTERS, make_picture, wcase

pytestmark = pytest.mark.gpu


def same_counters(st, info):
    assert {k: st[k] for k in COUNTERS} == {k: info[k] for k in COUNTERS}


# all keys equal; a stream of 38,528 bytes (more than window plus segment, no multiple of anything); the repeats at 32768 / 32769; a
# stream shorter than one sort tile; 8195 bytes: two sort tiles of 4096 keys and one key more
CANDIDATE_CASES = [("flat", 64, 64, 0), ("noise", 100, 128, 0), ("far", 16384, 1, 0), ("noise", 3, 2, "adaptive"), ("alphabet4", 546, 5, 0),
                   ("noise", 1, 1, 0)]


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("kind,width,height,filt", CANDIDATE_CASES, ids=lambda v: str(v))
def test_candidates_equal_the_definition(gpu, kind, width, height, filt, fast):
    img = make_picture(kind, width, height)
    want = W.candidates(M.filtered(img, M.filter_setting(filt))[0].reshape(-1))
    v = PngEncoder(width, height, filter=filt, coding="window", fast_math=fast)
    data = v.encode(img)
    got = v.candidates()
    print(f"{kind} {width} x {height}: {len(want)} positions, {(want != W.NONE).sum()} with a candidate, file {len(data)} bytes")
    assert NO_CANDIDATE == W.NONE and got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert np.array_equal(decode_png(data), img)
    assert np.array_equal(v.candidates(), want)                      # a second download; and after a second encode
    assert v.encode(img) == data and np.array_equal(v.candidates(), want)


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("kind,width,height", CASES, ids=lambda v: str(v))
def test_bytes_and_counters_equal_the_model(gpu, kind, width, height, filt, fast):
    img, want, info = wcase(kind, width, height, filt)
    v = PngEncoder(width, height, filter=filt, coding="window", fast_math=fast)
    got = v.encode(img)
    st = v.stats()
    print(f"{kind} {width} x {height} filter {filt} fast={fast}: {len(got)} bytes (model {len(want)}), modes {info['_modes']}, stats {st}")
    assert np.array_equal(v.candidates(), info["_prev"])
    same_counters(st, info)
    assert got == want
    assert v.encode(img) == got and st["ms_candidates"] > 0


@pytest.mark.parametrize("kind,filt", [("discs", "adaptive"), ("discs", 0), ("onecolour", "adaptive")])
def test_640_pictures_equal_the_model(gpu, kind, filt):
    """discs: the window block wins some segments and loses others; one-colour discs: it wins them all, with all 30 distance symbols"""
    img, want, info = wcase(kind, 640, 480, filt)
    v = PngEncoder(640, 480, filter=filt, coding="window")
    got = v.encode(img)
    st = v.stats()
    print(f"{kind} 640 x 480 filter {filt}: {len(got)} bytes (model {len(want)}), window segments {st['window_segments']} of {st['segments']}, stats {st}")
    same_counters(st, info)
    assert got == want
    assert PngEncoder(640, 480, filter=filt, coding="window", fast_math=True).encode(img) == want


def test_the_other_codings_keep_their_bytes_beside_a_window_encoder(gpu):
    img, want_win, info = wcase("mixed", 37, 53, "adaptive")
    _, want_dyn, info_dyn = dcase("mixed", 37, 53, "adaptive")
    _, want_fixed, _ = case("mixed", 37, 53, "adaptive")
    w = PngEncoder(37, 53, coding="window")
    assert w.encode(img) == want_win
    assert PngEncoder(37, 53).encode(img) == want_fixed                 # new encoders after a window encoder has run
    assert PngEncoder(37, 53, coding="dynamic").encode(img) == want_dyn
    v = PngEncoder(37, 53)                                              # one encoder, back and forth
    for coding, want in (("fixed", want_fixed), ("window", want_win), ("dynamic", want_dyn), ("window", want_win), ("fixed", want_fixed),
                         ("dynamic", want_dyn)):
        v.set_coding(coding)
        assert v.coding == coding and v.encode(img) == want, coding
        st = v.stats()
        assert (st["window_segments"] > 0) == (coding == "window") and (st["ms_candidates"] > 0) == (coding == "window")
        if coding == "window":
            same_counters(st, info)
            assert np.array_equal(v.candidates(), info["_prev"])
        else:
            assert st["window_matches"] == st["window_far_matches"] == st["window_header_bits"] == 0
            with pytest.raises(PngError, match="window"):
                v.candidates()
    assert {k: st[k] for k in ("literals", "matches", "dynamic_segments", "file_bytes")} == \
        {k: info_dyn[k] for k in ("literals", "matches", "dynamic_segments", "file_bytes")}
    assert w.encode(img) == want_win


def test_one_colour_discs_at_1024_decode_exactly_and_are_smaller_than_dynamic(gpu):
    img = W.one_colour_discs(1024, 1024)
    v = PngEncoder(1024, 1024, coding="window")
    data = v.encode(img)
    st = v.stats()
    dyn = PngEncoder(1024, 1024, coding="dynamic").encode(img)
    print(f"one-colour discs 1024 x 1024: window {len(data)} bytes, dynamic {len(dyn)}, ratio {len(data) / len(dyn):.3f}, stats {st}")
    M.check_file(data, img)   # zlib's own decoder, the Adler-32, every chunk CRC, the pixels
    assert len(data) == st["file_bytes"] <= bound(1024, 1024)
    assert len(data) < len(dyn)
    assert st["segments"] == 769 and 0 < st["window_segments"] <= 769 and 0 < st["window_far_matches"] <= st["matches"]
    prev = v.candidates()
    b = M.filtered(img, -1)[0].reshape(-1)
    assert np.array_equal(prev, W.candidates(b))
    assert PngEncoder(1024, 1024, coding="window", fast_math=True).encode(img) == data


def test_driver_png_coding_window(gpu, tmp_path):
    from sph_project_amd import run_simulation
    cfg = P.dam_break_scene(method="wcsph", end=(0.2, 0.2, 0.2))
    cfg["Configuration"].update(exportFrame=True, exportPly=True, outputInterval=3)
    f = tmp_path / "frames.json"
    f.write_text(json.dumps(cfg))
    win, plain = tmp_path / "win", tmp_path / "plain"
    cam = ["--render_size", "320", "240", "--camera_position", "1.2", "0.8", "1.4", "--camera_lookat", "0.2", "0.2", "0.2"]
    common = ["--scene_file", str(f), "--max_steps", "4", "--render"] + cam
    run_simulation.main(common + ["--output_dir", str(win), "--png_device", "--png_coding", "window"])
    run_simulation.main(common + ["--output_dir", str(plain)])            # the default path: the host's encoder
    frames = sorted(d for d in os.listdir(plain) if (plain / d).is_dir())
    assert frames == ["000000", "000003"]
    for d in frames:
        a, b = (win / d / "raw_view.png").read_bytes(), (plain / d / "raw_view.png").read_bytes()
        px = decode_png(b)
        assert px.shape == (240, 320, 3) and px.any()
        M.check_file(a, px)                                               # the same pixels from a valid file
        assert a == W.encode(px) and len(a) <= len(D.encode(px))
    with pytest.raises(SystemExit) as e:                                  # the coding belongs to the device encoder
        run_simulation.main(common + ["--output_dir", str(win), "--png_coding", "window"])
    assert e.value.code == 2
