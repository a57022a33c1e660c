"""CPU: the dynamic coding of the PNG stream ('Dynamic blocks') without a GPU -- the test-owned encoder of
tests/png_dynamic_model.py read back by zlib, PIL and video.decode_png with every checksum redone, never longer than the fixed model's
file or the bound, every branch shown taken on the model's notes, the length rules on hand-made histograms, and the library's host side:
the new symbol, the struct layout, the refusals, the command lines."""
import ctypes
import functools
import io
import itertools
import os

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import png as PNG
from tests import png_dynamic_model as D
from tests import png_model as M
from tests import test_png_host as H

ROOT = H.ROOT


def make_picture(kind, width, height):
    return D.period5(width) if kind == "period5" else H.make_picture(kind, width, height)


@functools.lru_cache(maxsize=None)
def dcase(kind, width, height, filt):
    """picture, the dynamic model's file, its counters and notes (computed once, shared with tests/test_hip_png_dynamic.py; read-only)"""
    img = make_picture(kind, width, height)
    info = {}
    data = D.encode(img, filt, info)
    img.setflags(write=False)
    return img, data, info


@functools.lru_cache(maxsize=None)
def fixed_file(kind, width, height, filt):
    return M.encode(make_picture(kind, width, height), filt)


CASES = [("noise", 1, 1), ("noise", 3, 2), ("mixed", 37, 53), ("lines", 86, 7), ("stripes", 100, 45), ("black", 64, 64),
         ("flat", 256, 256), ("period5", 2000, 1)]


def first_block_bits(data):
    """the three header bits (BFINAL, BTYPE) of the block every segment's chunk starts with"""
    bodies = [c[1] for c in M.chunks(data)[1:-2]]
    return [(b[2] if k == 0 else b[0]) & 7 for k, b in enumerate(bodies)]


@pytest.mark.parametrize("filt", ["adaptive", 0, 2, 4])
@pytest.mark.parametrize("kind,width,height", CASES)
def test_model_files_decode_and_are_no_longer_than_fixed(kind, width, height, filt):
    img, data, info = dcase(kind, width, height, filt)
    raw = M.check_file(data, img)   # zlib, Adler-32, every chunk CRC, video.decode_png
    assert info["raw_bytes"] == len(raw)
    assert info["file_bytes"] == len(data) <= len(fixed_file(kind, width, height, filt)) <= M.bound(width, height) == PNG.bound(width, height)
    modes = info["_modes"]
    assert len(modes) == info["segments"] and modes.count(2) == info["dynamic_segments"] and modes.count(0) == info["stored_segments"]
    assert (info["dynamic_header_bits"] > 0) == (info["dynamic_segments"] > 0)
    assert first_block_bits(data) == [{0: 0, 1: 2, 2: 4}[m] | (k == len(modes) - 1) for k, m in enumerate(modes)]
    ch = M.chunks(data)
    assert len(ch) == info["segments"] + 3 and info["zlib_bytes"] == sum(len(c[1]) for c in ch[1:-1])
    Image = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), img)


def test_every_branch_is_taken():
    img, data, info = dcase("mixed", 640, 480, "adaptive")          # all three modes in one picture
    M.check_file(data, img)
    modes = info["_modes"]
    assert info["segments"] == 226 and min(modes.count(m) for m in (0, 1, 2)) > 0, [modes.count(m) for m in (0, 1, 2)]
    assert len(data) < len(H.case("mixed", 640, 480, "adaptive")[1]) <= M.bound(640, 480)
    assert info["_notes"]["cl_limit"] > 0 and info["_notes"]["hlit286"] > 0 and info["_notes"]["overlong"] == 0
    assert info["_notes"]["longest_code"] <= 15
    _, _, info = dcase("mixed", 37, 53, "adaptive")                 # the code-length limit in both segments; a dynamic first segment
    assert info["_modes"] == [2, 2] and info["_notes"]["cl_limit"] == 2   # behind the zlib header, a dynamic last one with BFINAL
    _, _, info = dcase("period5", 2000, 1, 0)                       # five byte values with period 5: literals only, no distance code
    assert info["_modes"] == [2, 2] and info["_notes"]["no_dist"] == 2 and info["matches"] == 0 and info["literals"] == 6001
    _, _, info = dcase("black", 64, 64, "adaptive")                 # one literal, matches of 258 at distance 1: a single distance code
    assert info["_notes"]["one_dist"] == 4 and info["_modes"] == [2, 2, 2, 1]   # (the short last segment stays fixed)
    _, _, info = dcase("stripes", 100, 45, 0)                       # dynamic and stored in one file
    assert info["_modes"] == [2, 2, 2, 0]


def test_where_dynamic_never_wins_the_bytes_are_the_fixed_models():
    for kind, w, h in (("noise", 1, 1), ("noise", 3, 2)):           # the header outweighs any gain
        for filt in ("adaptive", 0):
            _, data, info = dcase(kind, w, h, filt)
            assert info["dynamic_segments"] == 0 and info["dynamic_header_bits"] == 0
            assert data == H.case(kind, w, h, filt)[1]
            assert {k: info[k] for k in ("literals", "matches", "stored_segments")} == {k: H.case(kind, w, h, filt)[2][k] for k in ("literals", "matches", "stored_segments")}
    _, data, info = dcase("black", 64, 64, "adaptive")              # here it wins: three full segments of 17 tokens each
    assert info["dynamic_segments"] == 3 and len(data) < len(H.case("black", 64, 64, "adaptive")[1])


# --- the length rules on hand-made histograms -----------------------------------------------------------------------------------------

def cost(hist, lengths):
    return sum(int(c) * ln for c, ln in zip(hist, lengths))


def best_cost_under(hist, limit):
    """the least cost of any complete prefix code with lengths <= limit, by trying every sorted length profile"""
    w = sorted((int(c) for c in hist if c > 0), reverse=True)
    best = None
    for prof in itertools.combinations_with_replacement(range(1, limit + 1), len(w)):   # non-decreasing: the heaviest gets the shortest
        if sum(1 << (limit - ln) for ln in prof) == 1 << limit:
            c = sum(a * b for a, b in zip(w, prof))
            best = c if best is None else min(best, c)
    return best


def test_two_symbols_and_single_symbols():
    for rule in (D.huffman_lengths, lambda h: D.limited_lengths(h, 7)):
        assert rule([0, 7, 0, 1]) == [0, 1, 0, 1]
        assert rule([0, 0, 5, 0, 0]) == [0, 0, 1, 0, 0]             # one used (distance) symbol: length 1, an incomplete code
        assert rule([0, 0, 0]) == [0, 0, 0]
    assert D.limited_lengths([0, 0, 0, 0, 9], D.DIST_LIMIT) == [0, 0, 0, 0, 1]


def test_equal_counts_break_ties_as_stated():
    # five leaves a..e of weight 3 in symbol order.  Two queues: a + b = 6, c + d = 6 (leaves before the node of 6), e + (a b) = 9 (the
    # leaf, then the older node), (c d) + (e a b) = 15: a, b at depth 3, the rest at 2.  Package-merge: the first 8 items of list 4 are
    # a b c d e (a b) (c d) (e (a b)): the same lengths.
    assert D.huffman_lengths([3] * 5) == [3, 3, 2, 2, 2]
    assert D.limited_lengths([3] * 5, 4) == [3, 3, 2, 2, 2]
    assert D.huffman_lengths([4] * 8) == [3] * 8 and D.limited_lengths([4] * 8, 7) == [3] * 8
    ll = D.huffman_lengths([14] * 286)                              # 286 = 2 x 256 - 226: 226 codes of 8 bits, 60 of 9
    assert D.kraft(ll, 15) == 1 << 15 and sorted(set(ll)) == [8, 9] and ll.count(9) == 60
    assert ll[:60] == [9] * 60                                      # the first leaves are joined first and end up deepest
    # a leaf before an internal node of equal weight: (1 1) = 2 waits while the leaves 2, 2 are joined, then 2 + 4 (the node first
    # would give 3 3 2 1 at the same cost: the stated preference keeps the tree shallow)
    assert D.huffman_lengths([1, 1, 2, 2]) == [2, 2, 2, 2]
    assert D.huffman_lengths([1, 1, 2]) == [2, 2, 1]


def test_fibonacci_counts_reach_15_and_the_next_step_is_refused():
    fib = [1, 1]
    while fib[-1] < 987:
        fib.append(fib[-1] + fib[-2])
    assert len(fib) == 16 and sum(fib) == 2583
    ll = D.huffman_lengths(fib)
    assert max(ll) == 15 == D.LL_LIMIT and D.kraft(ll, 15) == 1 << 15
    assert ll == [15, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    deeper = D.huffman_lengths(fib + [1597])                        # 4180 symbols: more than a segment's 4097
    assert max(deeper) == 16 and sum(fib) + 1597 > M.SEG + 1
    # the guard itself: a block whose lit/len code passes 15 is not offered
    notes = dict(cl_limit=0, no_dist=0, one_dist=0, hlit286=0, overlong=0, longest_code=0)
    b = np.repeat(np.arange(16, dtype=np.uint8), fib[1:] + [1597])    # 4179 literals; the end of block is the other count of 1
    assert D.dynamic_block(b, np.zeros(len(b), np.int64), np.zeros(len(b), np.int64), True, notes) is None and notes["overlong"] == 1


@pytest.mark.parametrize("hist", [
    [1, 1, 2, 4, 8, 16, 32, 64, 128, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],        # plain Huffman: depth 8
    [1, 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 0, 0, 0, 0, 0, 1, 1, 1],         # Fibonacci with ties
    [40, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 300],          # all 19 used
])
def test_the_code_length_code_keeps_its_limit_at_the_least_cost(hist):
    plain = D.huffman_lengths(hist)
    got = D.limited_lengths(hist, D.CL_LIMIT)
    assert max(got) <= 7 and D.kraft(got, 7) == 1 << 7
    assert [ln > 0 for ln in got] == [c > 0 for c in hist]
    assert cost(hist, got) == best_cost_under(hist, 7) >= cost(hist, plain)
    if max(plain) <= 7:
        assert cost(hist, got) == cost(hist, plain)
    else:
        assert cost(hist, got) > cost(hist, plain)
    # ties: of two symbols with equal counts the one with the smaller number is never the shorter
    for a, b in itertools.combinations(range(19), 2):
        if hist[a] == hist[b] and hist[a]:
            assert got[a] >= got[b], (a, b)


def test_the_header_rule_on_hand_made_lengths():
    assert D.run_length([0] * 150) == [(18, 127, 7), (18, 1, 7)]                 # 138 + 12
    assert D.run_length([0] * 148) == [(18, 127, 7), (17, 7, 3)]                 # 138 + 10
    assert D.run_length([0] * 140) == [(18, 127, 7), (0, 0, 0), (0, 0, 0)]
    assert D.run_length([5] * 8) == [(5, 0, 0), (16, 3, 2), (5, 0, 0)]           # 1 + 6 + 1
    assert D.run_length([5] * 10) == [(5, 0, 0), (16, 3, 2), (16, 0, 2)]         # 1 + 6 + 3
    assert D.run_length([3, 3, 3, 0, 0, 0, 4]) == [(3, 0, 0), (3, 0, 0), (3, 0, 0), (17, 0, 3), (4, 0, 0)]
    assert D.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]   # RFC 1951 3.2.2's example


# --- the library, without a device ---------------------------------------------------------------------------------------------------

def test_set_coding_is_declared_exported_and_refuses():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    lib = L.load()
    assert "sph_png_set_coding(" in header and "sph_png_set_coding" in L.EXPORTED_SYMBOLS and lib.sph_png_set_coding is not None
    assert "#define SPH_PNG_CODING_FIXED 0" in header and "#define SPH_PNG_CODING_DYNAMIC 1" in header
    assert (L.PNG_CODING_FIXED, L.PNG_CODING_DYNAMIC) == (0, 1)
    for coding in (0, 1, 2, -1):
        assert lib.sph_png_set_coding(None, coding) == -1
    assert b"sph_png_set_coding" in lib.sph_png_last_error(None)
    for bad in ("best", 1, None, "Dynamic"):
        with pytest.raises(ValueError):
            PNG.PngEncoder.__init__(object.__new__(PNG.PngEncoder), 8, 8, coding=bad)   # before any device is touched
    # reserved is still refused
    p = L.SphPngParams(width=8, height=8, filter=-1, fast_math=0, device=-1, reserved=1)
    h = ctypes.c_void_p()
    assert lib.sph_png_create(ctypes.byref(p), ctypes.byref(h)) == -1 and not h.value


def test_struct_layouts_match_the_header_with_the_new_fields_last():
    names = [n for n, _ in L.SphPngStats._fields_]
    assert names[-2:] == ["dynamic_segments", "dynamic_header_bits"] and names[-3] == "ms_total"
    assert L.SphPngStats.dynamic_segments.offset == 8 * 18                        # 12 int64 and 6 doubles before it, as before
    assert [n for n, _ in L.SphPngParams._fields_] == ["width", "height", "filter", "fast_math", "device", "reserved"]
    for struct_name in ("SphPngParams", "SphPngStats"):
        H.test_png_structs_match_the_header(struct_name)                          # offsetof / sizeof from the compiled header


def test_both_command_lines_carry_png_coding():
    from sph_project_amd import render_meshes, run_simulation
    base = ["--scene_file", "x.json", "--render", "--png_device"]
    assert run_simulation.parse_args(base).png_coding == "fixed"
    assert run_simulation.parse_args(base + ["--png_coding", "dynamic"]).png_coding == "dynamic"
    for bad in (["--scene_file", "x.json", "--render", "--png_coding", "dynamic"], ["--scene_file", "x.json", "--render", "--png_coding", "fixed"],
                base + ["--png_coding", "best"]):
        with pytest.raises(SystemExit):
            run_simulation.parse_args(bad)
    rm = ["--input_dir", "d", "--scene_file", "s.json"]
    assert render_meshes.parse_args(rm + ["--png_device"]).png_coding == "fixed"
    assert render_meshes.parse_args(rm + ["--png_device", "--png_coding", "dynamic"]).png_coding == "dynamic"
    with pytest.raises(SystemExit):
        render_meshes.parse_args(rm + ["--png_coding", "dynamic"])
