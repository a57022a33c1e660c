"""Host: the diffuse-particle model's known answers (tests/foam_model.py) -- the hash, analytic potentials and normals, the
three classes, death -- the condition the GPU tests put on their inputs, the new C symbols and struct layouts, and the driver's argument
errors.  No GPU."""
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
from tests import foam_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, H = M.R0, 4 * M.R0
DOM = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
OPEN = dict(ta_min=0.0, ta_max=1.0, wc_min=0.0, wc_max=1.0, e_min=0.0, e_max=1.0, k_ta=0.0, k_wc=0.0, max_diffuse=1000)


def model(**over):
    return M.FoamModel(R, *DOM, **dict(OPEN, **over))


def w(r):
    return 1.0 - r / H


def test_hash_known_answers():
    assert int(M.hash_u32(0, 0, 0, 0, 0)) == 0x4C727AF3
    assert int(M.hash_u32(12345, 7, 3, 2, 1)) == 0xBC2A8D0E
    assert np.allclose(M.rand(0, np.arange(3), 0, 0, 0), [0.29862177, 0.29656154, 0.32629389], atol=1e-8)
    # a negative id is its 32-bit pattern; the seed's upper half matters
    assert int(M.hash_u32(0, -1, 0, 0, 0)) == int(M.hash_u32(0, 0xFFFFFFFF, 0, 0, 0))
    assert int(M.hash_u32(1 << 32, 0, 0, 0, 0)) != int(M.hash_u32(0, 0, 0, 0, 0))
    assert int(M.make_key(3, 5, 2)) == (3 << 40) | (5 << 8) | 2


def test_hash_streams_are_uniform_and_below_one():
    pid = np.arange(1 << 16)
    for stream in range(5):
        u = M.rand(2024, pid, 7, 1, stream)
        assert abs(u.mean() - 0.5) < 0.01 and u.max() < 1.0 and u.min() >= 0.0
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)   # float32 holds every value
    a, b = M.rand(2024, pid, 7, 1, 1), M.rand(2024, pid, 7, 1, 2)
    assert abs(np.corrcoef(a, b)[0, 1]) < 0.02


def test_phi_at_below_and_above_its_limits():
    I = np.array([-1.0, 0.0, 2.0, 3.5, 5.0, 7.0])
    assert np.allclose(M.phi(I, 2.0, 5.0), [0.0, 0.0, 0.0, 0.5, 1.0, 1.0])


def test_a_uniform_velocity_lattice_traps_no_air_and_its_interior_has_no_normal():
    x = M.lattice(6, 6, 6, (0.4, 0.4, 0.4))
    v = np.tile([1.5, -0.5, 2.0], (len(x), 1))
    r = model().step(x, v, np.arange(len(x)), 1e-3)
    assert not r["ta"].any()
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    interior = ((g >= 2) & (g <= 3)).all(1)
    assert interior.sum() == 8 and not r["has_normal"][interior].any() and not r["normal"][interior].any()
    assert r["has_normal"][(g == 0).all(1)].all()   # a corner has one
    assert np.allclose(r["e"], 0.5 * (1.5 ** 2 + 0.5 ** 2 + 2.0 ** 2))


def test_a_flat_free_surface_has_axis_normals_and_no_crest():
    x = M.lattice(9, 4, 9, (0.3, 0.3, 0.3))
    g = np.stack(np.meshgrid(np.arange(9), np.arange(4), np.arange(9), indexing="ij"), -1).reshape(-1, 3)
    v = np.tile([0.0, 1.0, 0.0], (len(x), 1))
    r = model().step(x, v, np.arange(len(x)), 1e-3)
    centre = np.flatnonzero((g == (4, 3, 4)).all(1))[0]
    assert r["has_normal"][centre] and r["gate"][centre]
    assert np.abs(r["normal"][centre] - [0.0, 1.0, 0.0]).max() < 1e-6
    assert abs(r["wc"][centre]) < 1e-6
    below = np.flatnonzero((g == (4, 2, 4)).all(1))[0]
    assert not r["has_normal"][below]   # only the layer at distance h is missing above it, and that one weighs nothing


def test_two_particles_head_on():
    s, d = 3.0, 0.025
    x = np.array([[0.5, 0.5, 0.5], [0.5 + d, 0.5, 0.5]])
    v = np.array([[s, 0.0, 0.0], [-s, 0.0, 0.0]])
    r = model().step(x, v, [0, 1], 1e-3)
    want = 2 * s * 2 * w(float(np.float32(0.5 + d)) - 0.5)   # (the model takes float32 positions, as the device does)
    assert np.allclose(r["ta"], [want, want], rtol=1e-12)
    # flying apart: nothing
    assert np.allclose(model().step(x, -v, [0, 1], 1e-3)["ta"], 0.0, atol=1e-12)


def cluster(n, centre, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(centre) + rng.uniform(-0.2 * H, 0.2 * H, (n, 3))


def test_zero_ten_and_thirty_neighbours_take_the_three_branches():
    dt, g = 2e-3, np.array([0.0, -9.81, 0.0])
    seeds = np.array([[0.2, 0.5, 0.5], [0.5, 0.5, 0.5], [0.8, 0.5, 0.5]])
    x = np.concatenate([cluster(10, seeds[1], 1), cluster(30, seeds[2], 2)])
    v = np.concatenate([np.tile([0.3, 0.1, 0.0], (10, 1)), np.tile([0.0, 0.2, -0.1], (30, 1))])
    v0 = np.array([[0.1, 0.2, 0.3]] * 3)
    m = model(k_b=2.0, k_d=0.8, n_spray=6, n_bubble=20)
    m.seed(seeds, v0, [1.0, 1.0, 1.0])
    r = m.step(x, v, np.arange(40), dt)
    assert r["adv_N"].tolist() == [0, 10, 30] and r["adv_cls"].tolist() == [M.SPRAY, M.FOAM, M.BUBBLE] and not r["adv_und"].any()
    s = m.sorted()
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    assert np.allclose(s["v"][0], f32(v0[0]) + f32(dt) * f32(g), atol=1e-12) and s["life"][0] == 1.0
    assert np.allclose(s["v"][1], f32([0.3, 0.1, 0.0]), atol=1e-12) and np.isclose(s["life"][1], 1.0 - f32(dt), atol=1e-12)
    want = f32(v0[2]) - 2.0 * f32(dt) * f32(g) + 0.8 * (f32([0.0, 0.2, -0.1]) - f32(v0[2]))
    assert np.allclose(s["v"][2], want, atol=1e-12) and s["life"][2] == 1.0
    assert np.allclose(s["x"], f32(seeds) + f32(dt) * s["v"], atol=1e-12)
    assert s["cls"].tolist() == [M.SPRAY, M.FOAM, M.BUBBLE]


def test_a_foam_particle_dies_in_the_step_where_its_life_crosses_zero():
    dt = 2e-3
    x = cluster(10, (0.5, 0.5, 0.5), 4)
    m = model()
    m.seed([[0.5, 0.5, 0.5]], [[0.0, 0.0, 0.0]], [2.5 * dt])
    alive = []
    for _ in range(4):
        m.step(x, np.zeros_like(x), np.arange(10), dt)
        alive.append(len(m.key))
    assert alive == [1, 1, 0, 0]
    # ... and leaving the clamp box deletes whatever the life
    m = model()
    m.seed([[0.5, 0.0401, 0.5]], [[0.0, -1.0, 0.0]], [5.0])
    m.step(x, np.zeros_like(x), np.arange(10), dt)
    assert len(m.key) == 0


def test_children_beyond_the_capacity_are_dropped_in_scan_order():
    x, v, ids = M.input_a()
    big, small = M.FoamModel(R, *DOM, **M.PARAMS_A), M.FoamModel(R, *DOM, **dict(M.PARAMS_A, max_diffuse=64))
    a, b = big.step(x, v, ids, M.DT_FOAM), small.step(x, v, ids, M.DT_FOAM)
    assert a["born"] > 64 and b["born"] == 64 and small.dropped == a["born"] - 64 and big.dropped == 0
    assert np.array_equal(b["child_key"], a["child_key"][:64])


@pytest.mark.parametrize("case", ["A", "B"])
def test_the_gpu_inputs_meet_the_cap_on_undecided_sources(case):
    """the condition of tests/test_hip_foam.py, on the float64 model alone: at most 2 % of the source particles with n_d > 0 are
    undecided (an input that misses it gets another jitter seed, never a wider cap), and enough children are born for the comparison
    to mean something"""
    inp, prm, least = {"A": (M.input_a, M.PARAMS_A, 200), "B": (M.input_b, M.PARAMS_B, 50)}[case]
    x, v, ids = inp()
    r = M.FoamModel(R, *DOM, **prm).step(x, v, ids, M.DT_FOAM)
    sources = r["nd"] > 0
    assert sources.sum() >= 40
    assert (r["und_gen"] & sources).sum() <= 0.02 * sources.sum(), (int((r["und_gen"] & sources).sum()), int(sources.sum()))
    decided_children = (~r["und_gen"][r["child_src"]]).sum()
    assert decided_children >= least
    if case == "B":
        assert prm["k_ta"] == 0.0 and not r["ta"].any()   # every child of B comes from the wave crest alone


# --- ABI -------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["sph_foam_create", "sph_foam_destroy", "sph_foam_last_error", "sph_foam_step_handle", "sph_foam_step_points", "sph_foam_seed",
               "sph_foam_count", "sph_foam_download", "sph_foam_download_potentials", "sph_foam_clear", "sph_foam_stats", "sph_render_set_foam"]


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header and name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert lib.sph_foam_stats(None, None) == L.ERR_INVALID
    assert lib.sph_foam_count(None, None) == L.ERR_INVALID
    assert lib.sph_foam_step_points(None, None, None, None, 0, 1e-3) == L.ERR_INVALID
    assert lib.sph_render_set_foam(None, None, 0.5, None, None, None) == L.ERR_INVALID
    # a bad parameter is refused before any device is looked for
    p = L.SphFoamParams()
    h = ctypes.c_void_p()
    assert lib.sph_foam_create(ctypes.byref(p), ctypes.byref(h)) == L.ERR_INVALID and not h.value
    assert b"radius" in lib.sph_foam_last_error(None)


@pytest.mark.parametrize("struct_name", ["SphFoamParams", "SphFoamStats"])
def test_foam_structs_match_the_header(struct_name):
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


def test_python_and_model_defaults_are_the_documented_ones():
    from sph_project_amd import foam
    for k, v in M.DEFAULTS.items():
        assert foam.DEFAULTS[k] == v, k
    assert (foam.DEFAULTS["ta_min"], foam.DEFAULTS["ta_max"], foam.DEFAULTS["wc_min"], foam.DEFAULTS["wc_max"]) == (5.0, 20.0, 2.0, 8.0)
    assert (foam.DEFAULTS["n_spray"], foam.DEFAULTS["n_bubble"], foam.DEFAULTS["max_per_particle"]) == (6, 20, 8)


# --- driver ----------------------------------------------------------------------------------------------------------------------
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
    (["--foam_every", "2"], ("--foam_every", "--foam")),
    (["--foam_max", "1000"], ("--foam_max", "--foam")),
    (["--foam", "--gpus", "2"], ("--foam", "--gpus")),
    (["--foam", "--render", "--render_surface"], ("--foam", "--render_surface")),
    (["--foam", "--foam_every", "0"], ("--foam_every",)),
])
def test_driver_refuses_bad_foam_arguments(tmp_path, args, words):
    r = _driver(args, tmp_path)
    assert r.returncode == 2, r.stderr
    for word in words:
        assert word in r.stderr, r.stderr
    assert not (tmp_path / "o").exists()


def test_driver_lists_the_foam_flags(tmp_path):
    r = _driver(["--help"], tmp_path)
    assert r.returncode == 0
    for flag in ("--foam", "--foam_every", "--foam_max"):
        assert flag in r.stdout
