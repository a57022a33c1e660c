"""CPU only: the host model of the grid tables (tests/grid_model.py) against the oracle's grid build on three small scenes, in the
identity axis order and in a permuted one, and the checker against tables that are right except for one planted fault each (what a
mutation run on the GPU would show, without running a wrong kernel there)."""
import copy

import numpy as np
import pytest

from tests import grid_model as GM
from tests import helpers as H

AXIS_ORDERS = [(0, 1, 2), (2, 0, 1)]


def _permuted(cfg, axis_map):
    """the scene as the library sees it: library axis k = scene axis axis_map[k]"""
    out = copy.deepcopy(cfg)
    p = lambda v: [v[a] for a in axis_map]
    c = out["Configuration"]
    c["domainStart"], c["domainEnd"], c["gravitation"] = p(c["domainStart"]), p(c["domainEnd"]), p(c["gravitation"])
    for b in out["FluidBlocks"]:
        for k in ("start", "end", "translation", "velocity", "scale"):
            b[k] = p(b[k])
    return out


def _to_scene(pos_lib, axis_map):
    out = np.empty_like(pos_lib)
    out[:, list(axis_map)] = pos_lib
    return out


def _scene(late=False):
    """a 10 x 8 x 9 block thrown at the corner of a 0.30 x 0.42 x 0.50 domain: 8 x 11 x 13 cells of 0.04, no two axes alike"""
    cfg = H.dam_break_scene(domain_end=(0.30, 0.42, 0.50), end=(0.2 - 1e-9, 0.16 - 1e-9, 0.18 - 1e-9), translation=(0.05, 0.21, 0.06),
                            velocity=(1.5, -1.0, 2.0))
    if late:
        cfg["FluidBlocks"].append({"objectId": 1, "start": [0.0, 0.0, 0.0], "end": [0.08 - 1e-9] * 3, "translation": [0.05, 0.05, 0.36],
                                   "scale": [1, 1, 1], "velocity": [0.0, 0.0, -1.0], "density": 1000.0, "color": [7, 8, 9],
                                   "entryTime": 3.5 * 4e-4})
    return cfg


def _check_sort(sim, axis_map, pos_before, ids_before):
    """the oracle has just sorted `pos_before` (its own frame = the library's, in the order `ids_before`)"""
    gn_lib = [int(g) for g in sim.params["grid_num"]]
    gn_scene = [0, 0, 0]
    for k, a in enumerate(axis_map):
        gn_scene[a] = gn_lib[k]
    n = len(ids_before)
    lay = GM.make_layout(gn_scene, sim.params["support_radius"], n, axis_map)
    assert [lay["nx"], lay["ny"], lay["nz"]] == gn_lib
    m = GM.GridModel(GM.to_library(_to_scene(pos_before, axis_map), axis_map), ids_before, lay)
    np.testing.assert_array_equal(m.cell_start[1:], sim.field("grid_num_particles"))   # the reference's table is the inclusive scan
    np.testing.assert_array_equal(m.ids, H.oracle_ids(sim)[:n])
    np.testing.assert_array_equal(m.lin, sim.field("grid_ids")[:n])
    assert GM.check_tables(m.tables(), m) == []
    return m


@pytest.mark.parametrize("axis_map", AXIS_ORDERS, ids=["xyz", "zxy"])
def test_model_matches_the_oracle_on_a_jittered_block_and_after_30_steps(axis_map):
    sim = H.build_oracle(_permuted(_scene(), axis_map), jitter=0.006, seed=2)
    pos, ids = sim.field("particle_positions").copy(), H.oracle_ids(sim)
    sim.prepare()
    m0 = _check_sort(sim, axis_map, pos, ids)
    assert not np.array_equal(m0.ids, ids)          # the jitter did put particles out of lattice order
    moved = 0
    for _ in range(30):
        pos, ids = sim.field("particle_positions").copy(), H.oracle_ids(sim)
        sim.step(1)                                  # WCSPH sorts first: the sort saw the positions of the step before
        m = _check_sort(sim, axis_map, pos, ids)
        moved += int((m.order != np.arange(m.n)).sum())
    assert moved > 100                               # particles did change cell on the way


@pytest.mark.parametrize("axis_map", AXIS_ORDERS, ids=["xyz", "zxy"])
def test_model_matches_the_oracle_with_a_late_entry_object(axis_map):
    sim = H.build_oracle(_permuted(_scene(late=True), axis_map), jitter=0.004, seed=3)
    pos, ids = sim.field("particle_positions").copy(), H.oracle_ids(sim)
    sim.prepare()
    _check_sort(sim, axis_map, pos, ids)
    counts = []
    for _ in range(8):
        pos, ids = sim.field("particle_positions").copy(), H.oracle_ids(sim)
        H.oracle_step(sim)                           # the object enters in the middle of the fifth step, behind that step's sort
        _check_sort(sim, axis_map, pos, ids)
        counts.append(sim.particle_num)
    assert counts[0] == 720 and counts[-1] == 720 + 64 and counts[2] == 720 and counts[4] == 784, counts


# ---------------------------------------------------------------- the checker has teeth
@pytest.fixture(scope="module")
def planted():
    """16 x 16 x 32 cells = 4 scan tiles: a block of 300 particles in the lowest cells and one of 250 in the highest (it holds cell G - 1
    and sits at cx = nx - 1), tiles 1 and 2 empty with 300 particles before them; 550 particles = two full tiles of 256 and one of 38"""
    rng = np.random.default_rng(7)
    cell = 0.04
    lay = GM.make_layout((16, 16, 32), cell, 550)
    lo = rng.uniform(0.0, 0.079, (300, 3))
    hi = np.array([0.64, 0.64, 1.28]) - rng.uniform(0.0005, 0.079, (250, 3))
    hi[0] = np.array([0.64, 0.64, 1.28]) - 0.001        # cell G - 1
    pos = np.concatenate([lo, hi]).astype(np.float32)
    ids = rng.permutation(550)
    pos = pos[rng.permutation(550)]
    m = GM.GridModel(pos, ids, lay)
    assert m.counts[2048:6144].sum() == 0 and m.lin[-1] == lay["G"] - 1 and m.cell_start[2048] == 300
    assert GM.check_tables(m.tables(), m) == [] and GM.check_tables(m.tables(), m, deterministic=False) == []
    return m


def _only(viol, *words):
    assert len(viol) == 1, viol
    for w in words:
        assert w in viol[0], (w, viol[0])


def test_checker_reports_a_stale_empty_tile(planted):
    t = planted.tables()
    t["cell_start"][4096:6144] = 0                      # the count before the tile at an earlier sort
    _only(GM.check_tables(t, planted), "scan tile 2 ", "empty", "300 particles before it", "2048 entries differ")


def test_checker_reports_an_off_by_one_total(planted):
    t = planted.tables()
    t["cell_start"][-1] -= 1
    _only(GM.check_tables(t, planted), "cell_start[G = 8192]", "got 549", "want n = 550")


def test_checker_reports_a_stability_violation(planted):
    m = planted
    t = m.tables()
    c = int(np.flatnonzero(m.counts >= 2)[0])
    s = int(m.cell_start[c])
    t["ids"][[s, s + 1]] = t["ids"][[s + 1, s]]         # two particles of one cell swapped
    _only(GM.check_tables(t, m), "order: 2 slots differ", "a permutation of the same ids", "first at slot %d (cell %d)" % (s, c))
    assert GM.check_tables(t, m, deterministic=False) == []     # the cells still hold the same particles
    assert m.lin[-1] != c
    t["ids"][[s, -1]] = t["ids"][[-1, s]]               # ... but not after a swap with a particle of another cell
    _only(GM.check_tables(t, m, deterministic=False), "the cells do not hold the model's particles")


def test_checker_reports_a_run_length_taken_before_the_clamp(planted):
    m = planted
    G, ny, nz = m.layout["G"], m.layout["ny"], m.layout["nz"]
    t = m.tables()
    tile, k = m.tiles - 1, 4                            # the last tile ends in cell G - 1: its own window reaches one cell past the grid
    hi = int(m.headers[tile, 1]) + (k // 3 - 1) * ny * nz + (k % 3 - 1) * nz + 1
    assert hi == G
    beyond = 0                                          # what lies behind cell_start[G] in the zero-filled allocation
    t["headers"][tile, 11 + k] = beyond - int(m.headers[tile, 2 + k])
    _only(GM.check_tables(t, m), "tile header %d" % tile, "run length k=4")


def test_checker_reports_a_repeated_lane(planted):
    t = planted.tables()
    t["lane_perm"][1, 17] = 16
    _only(GM.check_tables(t, planted), "tile 1", "no bijection", "byte 16 occurs 2 times")
    t = planted.tables()
    t["lane_perm"][2, [3, 200]] = t["lane_perm"][2, [200, 3]]   # still a bijection, but a slot past n among the live ones
    _only(GM.check_tables(t, planted), "last tile", "does not come last")


def test_checker_reports_a_wrong_domain_bit_at_the_high_wall(planted):
    m = planted
    t = m.tables()
    s = int(np.flatnonzero(m.cx == m.layout["nx"] - 1)[0])
    assert not (int(m.cell_word[s]) >> 11) & 0b111000000        # no column at cx + 1
    t["cell_word"][s] |= np.uint32(1 << (11 + 7))               # (ox, oy) = (+1, 0) claimed to exist
    _only(GM.check_tables(t, m), "column-exists bits", "first at slot %d" % s, "cell (15,")
