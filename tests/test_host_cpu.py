"""CPU-only checks (no GPU): the C-ABI library loads and exports every symbol include/sph_hip.h declares,
the product path fails loudly without a device, scene arithmetic, analytic known answers of the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import ref as oracle_ref
from sph_project_amd import _lib as L
from sph_project_amd import scene
from sph_project_amd.SPH.utils import SimConfig
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        return hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    except OSError:
        return False


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    declared = set(re.findall(r"\b(sph_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = L.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in sph_hip.h but not exported by libsph_hip.so"
    assert declared == set(L.EXPORTED_SYMBOLS), declared ^ set(L.EXPORTED_SYMBOLS)


def test_struct_layout_matches_header(tmp_path):
    """ctypes mirrors of SphParams / SphStats / SphGridLayout have the size and field offsets the C compiler gives the header, and the
    table ids are the header's."""
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "sph_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(SphParams), offsetof(SphParams, grid_num), offsetof(SphParams, gravity),
         offsetof(SphParams, dt), offsetof(SphParams, particle_max_num), offsetof(SphParams, deterministic), sizeof(SphStats));
  printf("%zu %zu\\n", offsetof(SphStats, err_divergence), offsetof(SphStats, total_time));
  printf("%zu %zu %zu %zu %zu\\n", sizeof(SphGridLayout), offsetof(SphGridLayout, scan_tile), offsetof(SphGridLayout, axis_map),
         offsetof(SphGridLayout, cell_size), offsetof(SphGridLayout, tiles_valid));
  printf("%d %d %d %d\\n", SPH_GRID_CELL_START, SPH_GRID_TILE_HEADER, SPH_GRID_LANE_PERM, SPH_GRID_CELL_WORD);
  return 0; }''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    got = [ctypes.sizeof(L.SphParams), L.SphParams.grid_num.offset, L.SphParams.gravity.offset, L.SphParams.dt.offset,
           L.SphParams.particle_max_num.offset, L.SphParams.deterministic.offset, ctypes.sizeof(L.SphStats),
           L.SphStats.err_divergence.offset, L.SphStats.total_time.offset,
           ctypes.sizeof(L.SphGridLayout), L.SphGridLayout.scan_tile.offset, L.SphGridLayout.axis_map.offset,
           L.SphGridLayout.cell_size.offset, L.SphGridLayout.tiles_valid.offset,
           L.GRID_CELL_START, L.GRID_TILE_HEADER, L.GRID_LANE_PERM, L.GRID_CELL_WORD]
    assert [int(x) for x in out] == got


# runtime switches retired with the alternatives they selected: neither library may still read them
RETIRED_SWITCHES = (
    "SPH_XCD_CHUNK", "SPH_RUN_GROUPING", "SPH_SCAN_ALL_TILES", "SPH_NO_MASK_REUSE", "SPH_NO_LANE_PERM", "SPH_NO_LOOP_PUBLISH",
    "SPH_SLOW_SYNC", "SPH_STEP_COPIES_STATS", "SPH_NO_LOOP_HINT", "SPH_NO_FUSED_FORCES", "SPH_NO_SLAB_FUSED_FIELDS",
    "SPH_NO_SLAB_PRESEND", "SPH_NO_SLAB_OVERLAP", "SPH_NO_NEXT_HASH", "SPH_FIXED_KEEP_RESIDUAL", "SPH_NO_DFSPH_FUSED_DIV",
    "SPH_NO_CG_SPLIT", "SPH_CG_SPLIT_WAYS", "SPH_NO_CG_FUSED_P", "SPH_CG_COMBINE", "SPH_NO_SCAN_FOLD", "SPH_SCAN_FOLD_SLAB",
    "SPH_SORT_MOVE_ALL", "SPH_NO_LIST_GRID", "SPH_DEBUG_EXTRA_LDS", "SPH_AXIS_ORDER")


def test_test_hooks_live_in_their_own_library():
    """the pre-round-5 single halo header (a protocol with a known race), the consumer stall, the injected step failure and
    the rank that cannot set the push transport up, and the two switches of the implicit-viscosity launch forms are compiled into libsph_hip_testhooks.so only (-DSPH_TEST_HOOKS); the production
    library does not even contain the switches' names.  Nor does it contain the name of any retired switch."""
    here = os.path.join(ROOT, "sph_project_amd")
    prod = open(os.path.join(here, "libsph_hip.so"), "rb").read()
    hooks = open(os.path.join(here, "libsph_hip_testhooks.so"), "rb").read()
    for name in (b"SPH_TEST_SINGLE_HEADER", b"SPH_TEST_HALO_DELAY_US", b"SPH_TEST_FAIL_STEP", b"SPH_COMM_TEST_FAIL_PUSH_RANK",
                 b"SPH_TEST_CG_SPLIT_LIMIT", b"SPH_TEST_CG_SEPARATE_P"):
        assert name not in prod and name in hooks, name
    for name in RETIRED_SWITCHES:
        word = re.compile(re.escape(name.encode()) + rb"(?![A-Z0-9_])")   # the whole name, not a prefix of a longer one
        assert not word.search(prod) and not word.search(hooks), name


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a machine without a GPU")
def test_no_cpu_fallback():
    with pytest.raises(L.SphError, match="no HIP device"):
        H.build_product(H.dam_break_scene(end=(0.1, 0.1, 0.1)))


def test_scene_counts_of_baseline_configs():
    """particle counts verified with the reference's own np.arange arithmetic."""
    assert scene.cube_particle_num([0.0] * 3, [0.4] * 3, 0.02) == 8000
    assert scene.cube_particle_num([0.09, 0.2, 0.2], [1.7, 4.0, 1.8], 0.02) == 1231200
    assert scene.cube_particle_num([0.1, 0.1, 0.08], [2.1, 5.1, 3.28], 0.02) == 4000000
    from sph_project_amd import product as bench
    cfg = SimConfig(config=bench.c2_scene())
    geo = scene.derive_geometry(cfg)
    assert list(geo.grid_num) == [213, 200, 50] and abs(geo.V0 - 0.8 * 0.02 ** 3) < 1e-18


def test_simconfig_contract(tmp_path):
    import json
    p = tmp_path / "s.json"
    p.write_text(json.dumps(H.dam_break_scene()))
    c = SimConfig(scene_file_path=str(p))
    assert c.get_cfg("particleRadius") == 0.01 and c.get_cfg("nope") is None
    assert c.get_rigid_bodies() == [] and len(c.get_fluid_blocks()) == 1
    with pytest.raises(AssertionError):
        c.get_cfg("nope", enforce_exist=True)


# ---------------------------------------------------------------- analytic known answers (oracle)
def _lattice_sim(n=12, spacing=0.02):
    cfg = H.dam_break_scene(end=(n * spacing - 1e-9,) * 3, translation=(0.2, 0.2, 0.2))
    sim = H.build_oracle(cfg)
    sim.call("prepare_neighborhood_search")
    return sim


def test_kernel_normalisation_and_lattice_density():
    """sum_j V W(r_ij) on an interior lattice node ~ 0.8 (V0 = 0.8 d^3, base_container.py:49): rho = 0.8 rho0."""
    sim = _lattice_sim()
    sim.call("compute_density")
    rho = sim.field("particle_densities")
    pos = sim.field("particle_positions")
    inner = np.all((pos > 0.2 + 0.045) & (pos < 0.2 + 12 * 0.02 - 0.065), axis=1)
    assert inner.sum() > 50
    assert np.allclose(rho[inner], rho[inner][0], rtol=1e-5)
    # W integrates to 1: lattice quadrature of the cubic spline with cell volume d^3 (error of the quadrature < 1 %)
    assert abs(rho[inner][0] / 1000.0 / 0.8 - 1.0) < 0.01


def test_counting_sort_is_a_stable_permutation():
    cfg = H.dam_break_scene(end=(0.2, 0.2, 0.2))
    sim = H.build_oracle(cfg, jitter=0.006, seed=3)
    ids0 = H.oracle_ids(sim)
    pos0 = sim.field("particle_positions").copy()
    sim.call("prepare_neighborhood_search")
    ids = H.oracle_ids(sim)
    assert sorted(ids) == sorted(ids0)
    np.testing.assert_array_equal(sim.field("particle_positions"), pos0[ids])
    gid = sim.field("grid_ids")
    assert np.all(np.diff(gid) >= 0)
    for g in np.unique(gid)[:50]:
        assert np.all(np.diff(ids[gid == g]) > 0)  # stable: insertion order kept inside a cell
    cnt = sim.field("grid_num_particles")
    assert cnt[-1] == sim.particle_num and np.all(np.diff(cnt) >= 0)  # inclusive scan


def test_pressure_force_conserves_momentum():
    """Fluid-only symmetric pair forces: sum_i m_i a_i = 0 for the pressure acceleration."""
    cfg = H.dam_break_scene(end=(0.198, 0.198, 0.198), particleSpacing=0.018)
    sim = H.build_oracle(cfg, jitter=0.002, seed=4)
    sim.call("prepare_neighborhood_search")
    sim.call("compute_density")
    sim.call("wcsph_compute_pressure")
    sim.call("compute_pressure_acceleration")
    a = sim.field("particle_accelerations").astype(np.float64)
    m = sim.field("particle_masses").astype(np.float64)
    assert np.abs(sim.field("particle_pressures")).max() > 1e3
    total = (a * m[:, None]).sum(0)
    assert np.abs(total).max() < 1e-6 * np.abs(a * m[:, None]).sum()


def test_oracle_pair_metric_counts_four_wcsph_passes():
    sim = H.build_oracle(H.dam_break_scene(end=(0.12, 0.12, 0.12)), jitter=0.004, seed=8)
    sim.prepare()
    pos = sim.field("particle_positions").copy()
    diff = pos[:, None, :] - pos[None, :, :]
    r = np.sqrt((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2])  # f32, same order
    brute = int(((r < np.float32(0.04)) & ~np.eye(len(pos), dtype=bool)).sum())
    before = sim.last_pairs
    sim.call("compute_density")
    assert sim.last_pairs - before == brute
    # a WCSPH step = 4 neighbour passes over (almost) the same pairs
    sim.step(1)
    assert abs(sim.last_pairs - 4 * brute) <= 0.01 * 4 * brute


@pytest.mark.parametrize("native", [True, False], ids=["c-abi", "python"])
def test_ply_writer_layout(tmp_path, monkeypatch, native):
    """The bytes `ti.tools.PLYWriter(num_vertices=n).add_vertex_pos(x, y, z).export_ascii(path)` writes (run_simulation.py:139-144),
    restated from Taichi's python/taichi/tools/ply.py (print_header + export_ascii; default comment "created by PLYWriter"; every
    value is `str(np.float32)` followed by one blank).  Taichi is not installed here: the expected text below is that restatement
    written out by hand, not the output of a Taichi run.  Two writers produce it: sph_write_ply_ascii (C++ behind the C-ABI, the
    default: 0.3 s per 1.23 M-particle frame) and the numpy one (SPH_PLY_PYTHON=1, ~5 s)."""
    from sph_project_amd.run_simulation import read_ply_ascii, write_ply_ascii
    if native:
        monkeypatch.delenv("SPH_PLY_PYTHON", raising=False)
    else:
        monkeypatch.setenv("SPH_PLY_PYTHON", "1")
    p = tmp_path / "a.ply"
    pos = np.array([[0.0, 1.0, 2.5], [0.1, -3.0e-5, 123456.7], [1.0 / 3.0, 1e16, -0.0]], dtype=np.float32)
    write_ply_ascii(str(p), pos)
    expected = ("ply\nformat ascii 1.0\ncomment created by PLYWriter\nelement vertex 3\n"
                "property float x\nproperty float y\nproperty float z\nend_header\n"
                "0.0 1.0 2.5 \n0.1 -3e-05 123456.7 \n0.33333334 1e+16 -0.0 \n")
    assert p.read_text() == expected
    # the body is what export_ascii's python loop produces, value by value
    body = "".join("".join(str(v) + " " for v in row) + "\n" for row in pos)
    assert p.read_text().endswith("end_header\n" + body)
    # shortest round-trip digits: reading the file back gives the float32 values bit for bit
    rng = np.random.default_rng(5)
    big = np.concatenate([rng.uniform(-8, 8, (40000, 3)), rng.uniform(-1e-6, 1e-6, (50, 3)), rng.uniform(-1e9, 1e9, (50, 3))]).astype(np.float32)
    write_ply_ascii(str(p), big)   # (> 1 MiB of text: the native writer flushes its buffer in between)
    back = read_ply_ascii(str(p))
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), big.view(np.uint32))
    lines = p.read_text().splitlines()
    assert lines[lines.index("end_header") + 7] == "".join(str(v) + " " for v in big[6])
    write_ply_ascii(str(p), np.zeros((0, 3), np.float32))     # an object that has not entered yet
    assert p.read_text().endswith("element vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    assert read_ply_ascii(str(p)).shape == (0, 3)


def test_native_number_format_is_numpys(tmp_path):
    """sph_format_f32 (csrc/sph_export.hpp: std::to_chars shortest digits laid out by numpy's rule -- positional with one digit behind
    the point for 0 and 1e-4 <= |v| < 1e16, else scientific with a two-digit exponent) against `str(np.float32)` on 250 k values: uniform,
    tiny, over the whole exponent range, arbitrary bit patterns (subnormals, NaNs, infinities), and the edges of the two notations."""
    import ctypes as C
    from sph_project_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1)
    with np.errstate(over="ignore"):
        vals = np.concatenate([
            rng.uniform(-10, 10, 60000), rng.uniform(-1e-3, 1e-3, 40000), 10.0 ** rng.uniform(-45, 38, 60000) * rng.choice([-1, 1], 60000),
            [0.0, -0.0, 1.0, 0.1, 1e-4, 9.99999e-5, 1e16, 9.9999e15, 1e-5, 123456792.0, np.inf, -np.inf, np.nan, 1.17549435e-38, 1e-45,
             3.4028235e38, 0.0001234, 100.0, 1e15]]).astype(np.float32)
    vals = np.concatenate([vals, rng.integers(0, 2 ** 32, 90000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    buf = C.create_string_buffer(64)
    ref = vals.astype(str).tolist()
    bad = []
    for v, r in zip(vals.tolist(), ref):
        n = lib.sph_format_f32(C.c_float(v), buf)
        if buf.raw[:n].decode() != r:
            bad.append((v, buf.raw[:n], r))
    assert not bad, bad[:5]
    assert ref[vals.tolist().index(100.0)] == "100.0" and "1e-05" in ref and "1e+16" in ref


def test_bench_secondary_bound_is_recomputable_from_the_committed_profile():
    """bench.py attaches PMC-derived figures (HBM traffic, VALU issue, parked wave-cycles, LDS, effective clock) to its roofline object
    from profiles/pmc_derived.json.  Every one of them must follow from the counters printed in the summary file it names, by the
    formulas of tools/prof_summary.py ("a reader can recompute every number in the line")."""
    import json
    import re
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import prof_summary as ps
    doc = json.load(open(os.path.join(root, "profiles", "pmc_derived.json")))
    checked = 0
    # one summary file per configuration since round 5 (C2, C3 and C5 are separate rocprofv3 runs); every kernel entry of every configuration
    for config in [k for k in doc if not k.startswith("_")]:
        txt = open(os.path.join(root, doc[config].get("_source") or doc["_source"])).read()
        trace = {m.group(1): float(m.group(3)) * 1e3 for m in re.finditer(r"^(\S+)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)$", txt, re.M)}
        block = txt.split("== PMC counters, average per launch ==")[1].split("== derived")[0]
        ctr, cur = {}, None
        for line in block.splitlines():
            if line and not line.startswith(" "):
                cur = line.strip(); ctr[cur] = {}
            elif line.strip():
                a, b = line.split(); ctr[cur][a] = float(b)
        kernel_of = {v: "nbr_pass<%s>" % k for k, v in ps.KERNEL_ID.items()}
        for kid, entry in doc[config].items():
            if kid.startswith("_"):
                continue
            kernel = kernel_of[kid]
            d = ps.derive(trace[kernel], ctr[kernel])
            for key, val in entry.items():
                if key == "avg_us":
                    assert abs(val - trace[kernel] / 1e3) < 0.06, (config, kid, val, trace[kernel])
                else:
                    # (the summary prints the duration to 0.1 us: 2e-3 for the ~100 us walks of C2 / C3, more for the 13-30 us ones of C5)
                    tol = 2e-3 + 0.06 / max(trace[kernel] / 1e3, 1.0)
                    assert abs(d[key] - val) <= tol * abs(val) + 1e-9, (config, kid, key, d[key], val)
                checked += 1
    assert set(doc) >= {"c2", "c3", "c5"} and "density" in doc["c2"] and "wcsph_forces" in doc["c2"] and "cg_ap" in doc["c5"]
    assert checked >= 14


def test_run_record_stable_rank_model():
    """The deterministic sort of round 5 (csrc/sph_device.hpp k_scatter_index / k_scatter<true>) as a numpy model, against a stable argsort:
    the histogram hands every RUN (consecutive source particles of a wave with the same cell -- and, for the records, consecutive SLOTS) a
    block of its cell's slots in whatever order the atomics land; the stable rank of a particle is (lengths of the cell's runs that start at a
    lower source index) + (its position inside its run).  Includes what broke the first version on the GPU: particles that took their slots one
    by one (the arrivals a slab step appends) and happen to sit next to each other in the source order."""
    rng = np.random.default_rng(5)
    for trial in range(40):
        n_cells = int(rng.integers(3, 40))
        n_old = int(rng.integers(1, 600))
        n_new = int(rng.integers(0, 80))                      # arrivals: appended behind, one atomic each
        # last step's sorted order with a few particles that changed cell
        cell = np.sort(rng.integers(0, n_cells, n_old))
        move = rng.random(n_old) < 0.15
        cell[move] = np.clip(cell[move] + rng.integers(-1, 2, move.sum()), 0, n_cells - 1)
        cell = np.concatenate([cell, rng.integers(0, n_cells, n_new)]).astype(np.int64)
        n = n_old + n_new
        # k_hash_count: runs of equal cell inside waves of 64 source particles (old particles only), one "atomic" per run, in a random order
        wave = np.arange(n) // 64
        head_hash = np.ones(n, bool)
        head_hash[1:n_old] = (cell[1:n_old] != cell[:n_old - 1]) | (wave[1:n_old] != wave[:n_old - 1])
        heads = np.nonzero(head_hash[:n_old])[0]
        lens = np.diff(np.concatenate([heads, [n_old]]))
        count = np.zeros(n_cells, np.int64)
        slot = np.zeros(n, np.int64)
        for k in rng.permutation(len(heads)):                 # the order the atomics are served in
            h, L = heads[k], lens[k]
            slot[h:h + L] = count[cell[h]] + np.arange(L)
            count[cell[h]] += L
        for i in rng.permutation(np.arange(n_old, n)):        # k_halo_unpack2: the arrivals, one atomic each, after the hash
            slot[i] = count[cell[i]]; count[cell[i]] += 1
        start = np.concatenate([[0], np.cumsum(count)])
        # k_scatter_index: a record (first index, length) per run, filed at the run's first slot; runs must be contiguous in cell AND slot
        head = np.ones(n, bool)
        head[1:] = (cell[1:] != cell[:-1]) | (slot[1:] != slot[:-1] + 1) | (wave[1:] != wave[:-1])
        hs = np.nonzero(head)[0]
        ls = np.diff(np.concatenate([hs, [n]]))
        rec = {}
        for h, L in zip(hs, ls):
            rec[start[cell[h]] + slot[h]] = (h, L)
        # k_scatter<true>: the head walks its cell's records by jumping over their lengths
        dest = np.empty(n, np.int64)
        for h, L in zip(hs, ls):
            c = cell[h]
            r0, p = 0, start[c]
            while p < start[c + 1]:
                assert p in rec, "the walk must land on run starts only"
                first, length = rec[p]
                if first < h:
                    r0 += length
                p += length
            dest[h:h + L] = start[c] + r0 + np.arange(L)
        want = np.empty(n, np.int64)
        want[np.argsort(cell, kind="stable")] = np.arange(n)
        np.testing.assert_array_equal(dest, want)


def test_run_list_stable_rank_model():
    """The deterministic sort by per-cell RUN LISTS (round 6: csrc/sph_device.hpp run_list_file / k_sort_rank / k_gather_prep) as a numpy
    model, against a stable argsort.  Whoever hashes a run (consecutive source particles of a wave with the same cell) takes one histogram
    "atomic" for it -- served in any order -- and links it into its cell's list: the run whose atomic returned 0 (the cell's first arrival)
    stores (first particle, length) into first[cell] without another atomic, every later arrival exchanges head[cell] = (epoch, first
    particle) and keeps what it found (if of this epoch) as its `next`.  Stale heads and stale first[] entries of earlier sorts must not
    matter.  k_sort_rank: dest = cell_start + (lengths of the cell's runs that start at a lower source index) + (position inside the
    run), written as the inverse map the gather reads."""
    rng = np.random.default_rng(6)
    n_cells = 48
    head = np.zeros(n_cells, np.int64)          # (epoch << 32) | first particle; never reset
    first = np.full((n_cells, 2), -7, np.int64)  # never reset either
    epoch = 0
    for trial in range(60):
        epoch += 1
        n = int(rng.integers(1, 700))
        cell = np.sort(rng.integers(0, n_cells, n))
        move = rng.random(n) < (0.0 if trial % 5 == 0 else 0.2)    # every fifth trial: a rest lattice (every run is its cell, up to wave seams)
        cell[move] = np.clip(cell[move] + rng.integers(-2, 3, move.sum()), 0, n_cells - 1)
        wave = np.arange(n) // 64
        is_head = np.ones(n, bool)
        is_head[1:] = (cell[1:] != cell[:-1]) | (wave[1:] != wave[:-1])
        heads = np.nonzero(is_head)[0]
        lens = np.diff(np.concatenate([heads, [n]]))
        count = np.zeros(n_cells, np.int64)
        rec = {}
        for k in rng.permutation(len(heads)):                 # the order the atomics are served in
            h, L, c = int(heads[k]), int(lens[k]), int(cell[heads[k]])
            base = count[c]; count[c] += L
            if base == 0:
                first[c] = (h, L)
            else:
                old = head[c]; head[c] = (epoch << 32) | h
                rec[h] = (int(old & 0xffffffff) if (old >> 32) == epoch else -1, L)
        start = np.concatenate([[0], np.cumsum(count)])
        inv = np.full(n, -1, np.int64)
        for h, L in zip(heads, lens):
            c = cell[h]
            r0 = 0
            if start[c + 1] - start[c] != L:
                f0, fl = first[c]
                r0 = fl if f0 < h else 0
                p = int(head[c] & 0xffffffff) if (head[c] >> 32) == epoch else -1
                hops = 0
                while p >= 0:
                    nxt, length = rec[p]
                    if p < h:
                        r0 += length
                    p = nxt
                    hops += 1
                    assert hops <= start[c + 1] - start[c]
            d = start[c] + r0 + np.arange(L)
            assert (inv[d] == -1).all()
            inv[d] = h + np.arange(L)
        np.testing.assert_array_equal(inv, np.argsort(cell, kind="stable"))


def test_bench_dump_reorders_by_id_and_samples_above_the_limit():
    """bench.py --dump-outputs (dump_arrays): rows go to particle-id order as float32; above the byte limit the rows of an ascending
    sample of ids are kept, within the limit and the same from call to call; ids that are not a permutation are refused."""
    import bench
    rng = np.random.default_rng(5)
    n = 1000
    ids = rng.permutation(n).astype(np.int32)
    fields = {"position": rng.random((n, 3), dtype=np.float32), "density": rng.random(n, dtype=np.float32)}
    full = bench.dump_arrays(ids, fields)
    for name, a in fields.items():
        assert full[name].dtype == np.float32
        np.testing.assert_array_equal(full[name][ids], a)
    limit = 4000                                   # 16 B per particle: 250 of the 1000
    s1, s2 = bench.dump_arrays(ids, fields, limit), bench.dump_arrays(ids, fields, limit)
    assert len(s1["density"]) == 250 and sum(a.nbytes for a in s1.values()) <= limit
    for name in fields:
        np.testing.assert_array_equal(s1[name], s2[name])
    keep = np.array([np.flatnonzero((full["position"] == row).all(axis=1))[0] for row in s1["position"]])
    assert np.all(np.diff(keep) > 0)
    np.testing.assert_array_equal(s1["density"], full["density"][keep])
    bad = ids.copy()
    bad[0] = bad[1]
    with pytest.raises(RuntimeError):
        bench.dump_arrays(bad, fields)


def test_bench_measures_beyond_the_headline_only_with_full():
    """A plain `bench.py --gpus 1 --steps N --warmup W` is the headline alone; --full (off by default) turns on what takes runs of its own."""
    import bench
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False and plain.steps == 20 and plain.warmup == 5
    assert bench.parse_args(["--full"]).full is True
