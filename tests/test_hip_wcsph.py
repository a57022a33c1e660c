"""GPU parity tests of the WCSPH hot path: libsph_hip (through the C-ABI, driven by the SPH
package exactly as run_simulation.py drives the reference) against the CPU oracle."""
import numpy as np
import pytest

from sph_project_amd import _lib as L
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _state(container):
    e = container.engine
    ids = e.download(L.F_PARTICLE_ID)
    return {k: H.by_id(ids, e.download(f)) for k, f in
            dict(x=L.F_POSITION, v=L.F_VELOCITY, a=L.F_ACCELERATION, rho=L.F_DENSITY, p=L.F_PRESSURE,
                 V=L.F_REST_VOLUME, m=L.F_MASS).items()}


def _ref_state(ref):
    ids = H.oracle_ids(ref)
    names = dict(x="particle_positions", v="particle_velocities", a="particle_accelerations",
                 rho="particle_densities", p="particle_pressures", V="particle_rest_volumes", m="particle_masses")
    return {k: H.by_id(ids, ref.field(n).copy()) for k, n in names.items()}


def test_sort_matches_reference_order(gpu):
    """After prepare(): same permutation as the serial counting sort (base_container.py:506)."""
    cfg = H.dam_break_scene(end=(0.2, 0.24, 0.16))
    container, solver = H.build_product(cfg, jitter=0.004, seed=3)
    solver.prepare()
    ref = H.build_oracle(cfg, jitter=0.004, seed=3)
    ref.prepare()
    e = container.engine
    np.testing.assert_array_equal(e.download(L.F_PARTICLE_ID), H.oracle_ids(ref))
    np.testing.assert_array_equal(e.download(L.F_POSITION), ref.field("particle_positions"))
    np.testing.assert_array_equal(e.download(L.F_GRID_ID), ref.field("grid_ids"))
    g = e.download(L.F_GRID_ID)
    assert np.all(np.diff(g) >= 0)


@pytest.mark.parametrize("jitter", [0.0, 0.003])
def test_one_step_fields(gpu, jitter):
    cfg = H.dam_break_scene(end=(0.2, 0.2, 0.2))
    container, solver = H.build_product(cfg, jitter=jitter, seed=1)
    solver.prepare()
    solver.step()
    ref = H.build_oracle(cfg, jitter=jitter, seed=1)
    ref.prepare()
    ref.step(1)
    a, b = _state(container), _ref_state(ref)
    assert solver.stats()["pair_interactions"] == ref.last_pairs
    np.testing.assert_allclose(a["rho"], b["rho"], rtol=2e-6)
    np.testing.assert_allclose(a["p"], b["p"], rtol=1e-4, atol=1e-2)
    scale = np.abs(b["a"]).max()
    np.testing.assert_allclose(a["a"], b["a"], rtol=1e-4, atol=1e-5 * scale)
    np.testing.assert_allclose(a["v"], b["v"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(a["x"], b["x"], rtol=1e-6, atol=1e-8)


def test_drift_100_steps_8k(gpu):
    """C1 (8000-particle cube, WCSPH, dt 4e-4), N = 100 steps, drift <= 1e-4."""
    cfg = H.dam_break_scene()
    container, solver = H.build_product(cfg)
    solver.prepare()
    for _ in range(100):
        solver.step()
    ref = H.build_oracle(cfg)
    ref.prepare()
    ref.step(100)
    a, b = _state(container), _ref_state(ref)
    d = H.drift(a["x"], b["x"], container.dh)
    print("drift max %.3e p99 %.3e" % (d.max(), np.percentile(d, 99)))
    assert d.max() <= 1e-4


@pytest.mark.parametrize("fast_math", [0, 1])
def test_drift_compressed_block(gpu, fast_math):
    """Lattice packed 10 % tighter than rest spacing: rho > rho0 from step 0, so the Tait pressure force (which
    a rest lattice never triggers: rho = 0.8 rho0 is clamped to rho0, p = 0) dominates the motion."""
    cfg = H.dam_break_scene(end=(0.36, 0.36, 0.36), particleSpacing=0.018, velocity=(0.0, -0.5, 0.0))
    container, solver = H.build_product(cfg, jitter=0.002, seed=9, fast_math=fast_math)
    solver.prepare()
    ref = H.build_oracle(cfg, jitter=0.002, seed=9)
    ref.prepare()
    for _ in range(60):
        solver.step()
    ref.step(60)
    a, b = _state(container), _ref_state(ref)
    assert np.abs(b["p"]).max() > 1e3
    d = H.drift(a["x"], b["x"], container.dh)
    print("compressed drift (fast=%d) max %.3e p99 %.3e, n=%d" % (fast_math, d.max(), np.percentile(d, 99), len(d)))
    assert d.max() <= 1e-4


def test_fast_math_drift(gpu):
    cfg = H.dam_break_scene()
    container, solver = H.build_product(cfg, fast_math=1)
    solver.prepare()
    for _ in range(100):
        solver.step()
    ref = H.build_oracle(cfg)
    ref.prepare()
    ref.step(100)
    d = H.drift(_state(container)["x"], _ref_state(ref)["x"], container.dh)
    print("fast-math drift max %.3e p99 %.3e" % (d.max(), np.percentile(d, 99)))
    assert d.max() <= 1e-4


def test_lds_tile_equals_global_path(gpu):
    """The LDS cell-tile path and the direct-from-L2 fallback visit the same pairs in the same order."""
    cfg = H.dam_break_scene(end=(0.3, 0.3, 0.3))
    out = []
    for fg in (0, 1):
        container, solver = H.build_product(cfg, jitter=0.003, seed=7, force_global=fg)
        solver.prepare()
        for _ in range(5):
            solver.step()
        out.append((_state(container), solver.stats()))
    for k in ("x", "v", "rho", "p", "a"):
        np.testing.assert_array_equal(out[0][0][k], out[1][0][k])
    assert out[0][1]["pair_interactions"] == out[1][1]["pair_interactions"]
    assert out[0][1]["lds_fallback_blocks"] < out[1][1]["lds_fallback_blocks"]


@pytest.mark.parametrize("spacing,label", [(0.0185, "runs of ~30 candidates: some second mask words"),
                                           (0.0165, "runs of ~43 candidates: every wave takes the 64-bit merged loop"),
                                           (0.0140, "runs of ~70 candidates: beyond two mask words, ordered path")])
def test_all_neighbour_paths_agree(gpu, spacing, label):
    """The merged loop (one or two mask words per run, lane permutation), the ordered LDS path (mode 4) and the
    chunk path of oversized runs (mode 1: every run) visit the same pairs in the same order: bitwise identical states and pair counts,
    whatever the number of candidates per run.  Against the oracle: pair counts identical, drift within tolerance."""
    cfg = H.dam_break_scene(end=(0.2, 0.2, 0.2), particleSpacing=spacing, dt=1e-4)
    out = []
    dh = None
    for fg in (0, 4, 1):
        container, solver = H.build_product(cfg, jitter=0.002, seed=11, force_global=fg)
        solver.prepare()
        for _ in range(3):
            solver.step()
        out.append((_state(container), solver.stats()))
        dh = container.dh
    for other in out[1:]:
        for k in ("x", "v", "rho", "p", "a"):
            np.testing.assert_array_equal(out[0][0][k], other[0][k])
        assert out[0][1]["pair_interactions"] == other[1]["pair_interactions"]
    ref = H.build_oracle(cfg, jitter=0.002, seed=11)
    ref.prepare()
    ref.step(3)
    assert out[0][1]["pair_interactions"] == ref.last_pairs
    d = H.drift(out[0][0]["x"], _ref_state(ref)["x"], dh)
    print(label, "drift max %.3e" % d.max())
    assert d.max() <= 1e-5


OVERSIZED = [("dfsph", 0.0060), ("dfsph", 0.0064), ("pcisph", 0.0060), ("wcsph", 0.0060)]


def oversized_scene(method, spacing):
    """(scene, jitter, seed) of test_oversized_runs_through_the_tile_in_chunks (tests/test_hip_tall_grid.py runs its tall twin)"""
    return H.dam_break_scene(method=method, end=(0.118, 0.118, 0.118), particleSpacing=spacing, dt=1e-5), 0.3 * spacing, 5


@pytest.mark.parametrize("method,spacing", OVERSIZED)
def test_oversized_runs_through_the_tile_in_chunks(gpu, method, spacing):
    """A run longer than a functor's tile goes through the tile in chunks (process_chunk), and tiles differ between functors (1280 slots
    for the payload-free passes, ~1064 for the 32-36-byte records, in between for the solver walks): the pass that STORES the
    acceptance masks may take the chunk path for a run that a later pass reads out of its larger tile with those stored masks, and
    the other way round.  ~300 particles per cell puts the run lengths right across those capacities.  One step (the block is far
    too dense to be stepped further), default paths against debug mode 1 (every run through the chunk path, every mask recomputed):
    bitwise the same state and the same number of pairs."""
    cfg, jitter, seed = oversized_scene(method, spacing)
    out = []
    for fg in (0, 1):
        container, solver = H.build_product(cfg, jitter=jitter, seed=seed, force_global=fg, fixed_iterations=2)
        solver.prepare()
        solver.step()
        out.append((_state(container), solver.stats()))
    assert out[0][1]["lds_fallback_blocks"] > 0    # some runs did overflow a tile in the default build
    for k in ("x", "v", "rho"):
        np.testing.assert_array_equal(out[0][0][k], out[1][0][k])
    assert out[0][1]["pair_interactions"] == out[1][1]["pair_interactions"]


PILED_UP = [(0.0080, "125 particles per cell: a group's three runs exceed the tile -> staged in rounds"),
            (0.0058, "~330 per cell: single runs exceed the tile -> through the tile in chunks")]


def piled_up_scene(spacing):
    """(scene, jitter, seed) of test_piled_up_cells_density (tests/test_hip_tall_grid.py runs its tall twin)"""
    return H.dam_break_scene(end=(0.118, 0.118, 0.118), particleSpacing=spacing), 0.3 * spacing, 4


@pytest.mark.parametrize("spacing,label", PILED_UP)
def test_piled_up_cells_density(gpu, spacing, label):
    """Extreme pile-ups (the domain clamp of the reference parks particles in the boundary cells): the density pass alone -- a
    full step would blow such a block apart -- through every path: default (rounds / chunks as the tile allows), ordered LDS
    walk (mode 4), every run in chunks (mode 1); bitwise the same densities and pair counts, and the oracle's."""
    cfg, jitter, seed = piled_up_scene(spacing)
    out = []
    for fg in (0, 4, 1):
        container, solver = H.build_product(cfg, jitter=jitter, seed=seed, force_global=fg)
        solver.prepare()
        e = container.engine
        e.run_phase(L.PH_DENSITY)
        ids = e.download(L.F_PARTICLE_ID)
        out.append((H.by_id(ids, e.download(L.F_DENSITY)), solver.stats()))
    for rho, st in out[1:]:
        np.testing.assert_array_equal(out[0][0], rho)
        assert st["pair_interactions"] == out[0][1]["pair_interactions"]
    ref = H.build_oracle(cfg, jitter=jitter, seed=seed)
    ref.prepare()
    ref.call("compute_density")
    rho_ref = H.by_id(H.oracle_ids(ref), ref.field("particle_densities").copy())
    n = len(rho_ref)
    print(label, ": n = %d, max rho / rho0 = %.0f, pairs per particle %.0f, runs walked from L2 %d (default) / %d (forced)" % (
        n, rho_ref.max() / 1000.0, out[0][1]["pair_interactions"] / n, out[0][1]["lds_fallback_blocks"], out[2][1]["lds_fallback_blocks"]))
    np.testing.assert_allclose(out[0][0], rho_ref, rtol=3e-6)   # (a density that matches to 3e-6 has the oracle's neighbours)
    assert rho_ref.max() > 10 * 1000.0


def test_static_domain_box(gpu):
    """addDomainBox: static rigid boundary particles (base_container.py:192, base_solver.py:106)."""
    cfg = H.dam_break_scene(domain_end=(0.6, 0.6, 0.6), end=(0.2, 0.2, 0.2), translation=(0.06, 0.06, 0.06),
                            add_domain_box=True)
    container, solver = H.build_product(cfg)
    solver.prepare()
    ref = H.build_oracle(cfg)
    ref.prepare()
    a, b = _state(container), _ref_state(ref)
    np.testing.assert_allclose(a["V"], b["V"], rtol=2e-6)
    np.testing.assert_allclose(a["m"], b["m"], rtol=2e-6)
    for _ in range(20):
        solver.step()
    ref.step(20)
    a, b = _state(container), _ref_state(ref)
    assert solver.stats()["pair_interactions"] == ref.last_pairs
    d = H.drift(a["x"], b["x"], container.dh)
    print("box drift max %.3e" % d.max())
    assert d.max() <= 1e-4


def test_non_deterministic_sort_still_within_tolerance(gpu):
    cfg = H.dam_break_scene(end=(0.2, 0.2, 0.2))
    container, solver = H.build_product(cfg, deterministic=0)
    solver.prepare()
    for _ in range(50):
        solver.step()
    ref = H.build_oracle(cfg)
    ref.prepare()
    ref.step(50)
    d = H.drift(_state(container)["x"], _ref_state(ref)["x"], container.dh)
    assert d.max() <= 1e-4


def test_edge_cases(gpu):
    # single particle: no neighbours, free fall + boundary clamp
    cfg = H.dam_break_scene(end=(0.01, 0.01, 0.01))
    container, solver = H.build_product(cfg)
    assert container.particle_max_num == 1
    solver.prepare()
    ref = H.build_oracle(cfg)
    ref.prepare()
    for _ in range(400):
        solver.step()
    ref.step(400)
    np.testing.assert_allclose(container.engine.download(L.F_POSITION), ref.field("particle_positions"), rtol=1e-6)
    np.testing.assert_allclose(container.engine.download(L.F_VELOCITY), ref.field("particle_velocities"), rtol=1e-5, atol=1e-7)
    # capacity and argument errors surface as exceptions, not aborts
    with pytest.raises(L.SphError):
        container.engine.append_particles(0, np.zeros((1, 3)), np.zeros((1, 3)), np.ones(1), np.zeros(1),
                                          np.ones(1), np.ones(1), np.zeros((1, 3)))
    with pytest.raises(L.SphError):
        container.engine.download(L.F_DFSPH_ALPHA)


def test_c2_full_size_20_steps(gpu):
    """the headline configuration C2 (1,231,200 particles, bench.py's workload, fast build) against the
    oracle for N = 20 steps, THROUGH THE PATH bench.py TIMES: one solver.advance(20) = sph_step_async(20), in which the
    force pass of every step but the last is also the next step's init_grid (NextHash, base_container.py:496-546) --
    asserted from the library's own counters, not assumed.  Plus size-independent checks at full size: accepted-pair
    counts identical to the oracle's, the sort is a permutation (every id once), positions stay inside the clamped
    domain, no NaNs; and ids / positions / velocities bit-equal to the same scene stepped one call at a time (the
    path every fixture test takes: k_hash_count launched every step)."""
    from sph_project_amd import product as bench
    cfg = bench.c2_scene()
    container, solver = H.build_product(cfg, fast_math=1)
    solver.prepare()
    ref = H.build_oracle(cfg)
    ref.prepare()
    h0, p0, l0 = solver.stats()["hash_launches"], solver.stats()["prehashed_sorts"], solver.stats()["list_sorts"]
    solver.advance(20)
    ref.step(20)
    e = container.engine
    st = solver.stats()
    assert st["steps"] == 20
    assert st["prehashed_sorts"] - p0 == 19 and st["hash_launches"] - h0 == 1, (st["hash_launches"], st["prehashed_sorts"])
    assert st["list_sorts"] - l0 == 20, st   # ... and every sort ranked the particles from the run lists those hashers filed (k_sort_rank + k_gather_prep)
    ids = e.download(L.F_PARTICLE_ID)
    assert np.array_equal(np.sort(ids), np.arange(1231200))
    x_sorted, v_sorted = e.download(L.F_POSITION), e.download(L.F_VELOCITY)
    x = H.by_id(ids, x_sorted)
    xr = H.by_id(H.oracle_ids(ref), ref.field("particle_positions").copy())
    assert np.isfinite(x).all()
    pad = container.padding
    assert (x >= np.float32(pad)).all() and (x <= (container.domain_size - pad).astype(np.float32)).all()
    d = H.drift(x, xr, container.dh)
    print("C2 full size through advance(20): drift max %.3e p99 %.3e; pairs/step %d; hash launches %d, prehashed sorts %d" % (
        d.max(), np.percentile(d, 99), st["pair_interactions"], st["hash_launches"] - h0, st["prehashed_sorts"] - p0))
    assert d.max() <= 1e-4
    assert st["pair_interactions"] == ref.last_pairs
    ref.close()
    # the same scene, one call per step: no NextHash anywhere
    c1, s1 = H.build_product(cfg, fast_math=1)
    s1.prepare()
    h1 = s1.stats()["hash_launches"]
    for _ in range(20):
        s1.step()
    st1 = s1.stats()
    assert st1["prehashed_sorts"] == 0 and st1["hash_launches"] - h1 == 20
    assert np.array_equal(c1.engine.download(L.F_PARTICLE_ID), ids)
    assert np.array_equal(c1.engine.download(L.F_POSITION), x_sorted)
    assert np.array_equal(c1.engine.download(L.F_VELOCITY), v_sorted)
    assert st1["pair_interactions"] == st["pair_interactions"]


@pytest.mark.parametrize("fast_math", [1, 0])
def test_c2_full_size_in_motion_vs_oracle(gpu, fast_math, from_step=2500):
    """The state `value_in_motion` of bench.py is quoted on: C2 (1,231,200 particles) advanced to step 2500 -- the column has collapsed,
    39 neighbours per particle instead of 29, cells of up to several dozen particles at the bottom and along the walls: second mask words,
    staging rounds that do not fit the tile, the chunked walk (`lds_fallback_blocks`), particles resting on the domain faces -- none of which
    the rest lattice of the 20-step test ever takes at this size.  The oracle is seeded with the product's state at that step (positions /
    velocities bit for bit, in the product's order), both advance 5 steps -- the product through ONE advance(5), the path the bench times --
    and must agree: drift <= 1e-5 by particle id (measured 1.5e-7), the accepted-pair counts of the last step equal up to the handful of
    pairs that sit within an ulp of r = h (each counts 4: one density + three force sums), and the sort order equal except where a particle
    sits within an ulp of a cell face at sort time (it then files into the neighbouring cell on one side only: a few hundred slots of
    1.23 M shift by one; measured 0-612).  Neither build is bit-identical to the oracle in this state (1,916 positions differ by an ulp
    after the first step in the strict build): the equalities of the rest-lattice test would be luck here."""
    from sph_project_amd import product as bench
    cfg = bench.c2_scene()
    container, solver = H.build_product(cfg, fast_math=fast_math)
    solver.prepare()
    solver.advance(from_step)
    e = container.engine
    ids0, x0, v0 = (e.download(f) for f in (L.F_PARTICLE_ID, L.F_POSITION, L.F_VELOCITY))
    assert np.array_equal(np.sort(ids0), np.arange(1231200)) and np.isfinite(x0).all() and np.isfinite(v0).all()
    st0 = solver.stats()
    nbrs = st0["pair_evaluations"] / 2.0 / 1231200
    assert nbrs > 35.0, nbrs   # (the rest lattice holds 29: this IS another regime)
    ref = H.oracle_from_state(cfg, x0, v0, ids0)
    ref.prepare()
    p0 = st0["prehashed_sorts"]
    solver.advance(5)
    ref.step(5)
    st = solver.stats()
    assert st["prehashed_sorts"] - p0 == 4, (p0, st["prehashed_sorts"])
    ids, oid = e.download(L.F_PARTICLE_ID), H.oracle_ids(ref)
    assert np.array_equal(np.sort(ids), np.arange(1231200))
    moved = int((ids != oid).sum())
    x, xr = H.by_id(ids, e.download(L.F_POSITION)), H.by_id(oid, ref.field("particle_positions").copy())
    d = H.drift(x, xr, container.dh)
    dv = np.abs(H.by_id(ids, e.download(L.F_VELOCITY)).astype(np.float64) - H.by_id(oid, ref.field("particle_velocities").copy())).max()
    print("C2 in motion (steps %d..%d, %s build): %.1f neighbours per particle, drift max %.3e p99 %.3e, max |dv| %.3e m/s, pairs/step %d "
          "(oracle %+d), slots in another order %d, ordered-walk rounds in the last step %d" % (
              from_step, from_step + 5, "fast" if fast_math else "strict", nbrs, d.max(), np.percentile(d, 99), dv, st["pair_interactions"],
              ref.last_pairs - st["pair_interactions"], moved, st["lds_fallback_blocks"]))
    assert d.max() <= 1e-5
    assert abs(st["pair_interactions"] - ref.last_pairs) <= 4 * 64, (st["pair_interactions"], ref.last_pairs)
    assert moved <= 1231200 // 100, moved
    ref.close()


@pytest.mark.parametrize("fast_math", [0, 1])
def test_next_hash_changes_nothing(gpu, fast_math):
    """NextHash A/B: a collapsing block advanced with sph_step_async(n) in calls of several lengths (the force
    pass hashes for the next sort inside a call, k_hash_count runs at the head of every call) against the same scene with
    no NextHash at all (one step per call): ids, positions, velocities, densities and pair counts array_equal after
    every call, and the counters say which path ran.  The block is perturbed and moving, so cells change population every step
    (runs of equal cells break up: the histogram atomics of the epilogue and of k_hash_count hand out different slots -- the
    stable rank must not care)."""
    cfg = H.dam_break_scene(end=(0.3, 0.4, 0.3), velocity=(0.4, -1.5, 0.3))
    out = []
    for mode in ("calls", "single"):
        container, solver = H.build_product(cfg, fast_math=fast_math, jitter=0.003, seed=11)
        e = container.engine
        solver.prepare()
        st0 = solver.stats()
        snaps = []
        for n in (1, 7, 2, 30):
            if mode == "calls":
                e.step_async(n)
            else:
                for _ in range(n):
                    e.step_async(1)
            st = solver.stats()
            snaps.append((e.download(L.F_PARTICLE_ID), e.download(L.F_POSITION), e.download(L.F_VELOCITY), e.download(L.F_DENSITY),
                          st["pair_interactions"]))
        st = solver.stats()
        assert st["prehashed_sorts"] == (0 + 6 + 1 + 29 if mode == "calls" else 0), st
        assert (st["hash_launches"] - st0["hash_launches"]) + st["prehashed_sorts"] == 40, (st0, st)
        out.append(snaps)
    for a, b in zip(*out):
        for u, v in zip(a[:4], b[:4]):
            assert np.array_equal(u, v)
        assert a[4] == b[4]


@pytest.mark.parametrize("fast_math", [0, 1])
def test_list_sort_equals_record_sort(gpu, fast_math, monkeypatch):
    """The deterministic sort by per-cell RUN LISTS (filed by whoever hashes: k_hash_count / the force pass; then k_sort_rank +
    k_gather_prep, which also prepares the tiles for the neighbour passes) against the sort by run records (k_scatter_index +
    k_scatter<true> + k_block_prep; SPH_NO_RUN_LISTS=1): a perturbed, collapsing block whose cells change population every step,
    advanced in calls of several lengths -- ids, positions, velocities, densities and pair counts array_equal after every call
    (= same order, same tile headers / cell words / lane permutation as far as any result depends on them), and the counters say
    which sort ran.  reorder_particles: base_container.py:506-515."""
    cfg = H.dam_break_scene(end=(0.3, 0.4, 0.3), velocity=(0.4, -1.5, 0.3))
    out = []
    for lists in (True, False):
        if not lists:
            monkeypatch.setenv("SPH_NO_RUN_LISTS", "1")
        container, solver = H.build_product(cfg, fast_math=fast_math, jitter=0.003, seed=11)
        e = container.engine
        solver.prepare()
        snaps = []
        for n in (1, 7, 2, 30):
            e.step_async(n)
            st = solver.stats()
            snaps.append((e.download(L.F_PARTICLE_ID), e.download(L.F_POSITION), e.download(L.F_VELOCITY), e.download(L.F_DENSITY),
                          st["pair_interactions"]))
        st = solver.stats()
        sorts = st["hash_launches"] + st["prehashed_sorts"]
        assert st["list_sorts"] == (sorts if lists else 0), st
        out.append(snaps)
    for a, b in zip(*out):
        for u, v in zip(a[:4], b[:4]):
            assert np.array_equal(u, v)
        assert a[4] == b[4]


def test_list_sort_leaves_colours_at_home_and_densities_to_the_next_pass(gpu):
    """What the sort's gather does NOT move (k_gather_prep: the colours stay keyed by the particle id while the ids are the append
    order; an all-fluid WCSPH step does not carry the density its next pass recomputes): two blocks of different colour thrown at
    each other plus one that enters late, advanced through list sorts -- every particle still has the colour it was appended
    with (downloaded in sorted order, looked up by id), the density download is the pass's own (finite, ~rho0), and the colours
    keep travelling with the particles once ids set from outside have ended the shortcut."""
    cfg = H.dam_break_scene(end=(0.2, 0.3, 0.3), translation=(0.1, 0.1, 0.1), velocity=(1.0, 0.0, 0.0))
    cfg["FluidBlocks"][0]["color"] = [10, 20, 30]
    cfg["FluidBlocks"].append({"objectId": 1, "start": [0.0, 0.0, 0.0], "end": [0.2, 0.3, 0.3], "translation": [0.5, 0.1, 0.1],
                               "scale": [1, 1, 1], "velocity": [-1.0, 0.0, 0.0], "density": 1000.0, "color": [200, 100, 50],
                               "entryTime": -1.0})
    cfg["FluidBlocks"].append({"objectId": 2, "start": [0.0, 0.0, 0.0], "end": [0.1, 0.1, 0.1], "translation": [0.35, 0.6, 0.2],
                               "scale": [1, 1, 1], "velocity": [0.0, -1.0, 0.0], "density": 1000.0, "color": [7, 8, 9],
                               "entryTime": 20.5 * 4e-4})
    container, solver = H.build_product(cfg, fast_math=1)
    solver.prepare()
    e = container.engine
    ids0, col0 = e.download(L.F_PARTICLE_ID), e.download(L.F_COLOR)
    home = np.zeros((container.particle_max_num, 3), np.int32)
    home[ids0] = col0
    n0 = len(ids0)
    for _ in range(30):
        solver.step()
    solver.advance(30)
    st = solver.stats()
    assert st["list_sorts"] >= 60, st
    ids, col, rho = e.download(L.F_PARTICLE_ID), e.download(L.F_COLOR), e.download(L.F_DENSITY)
    assert len(ids) > n0 and np.array_equal(np.sort(ids), np.arange(len(ids)))      # the late block came in
    late = ids >= n0
    assert (col[late] == np.array([7, 8, 9])).all()
    assert np.array_equal(col[~late], home[ids[~late]])
    assert set(map(tuple, col0)) == {(10, 20, 30), (200, 100, 50)}
    assert np.isfinite(rho).all() and rho.min() >= 999.0 and rho.max() < 2000.0
    # ids from outside end the shortcut: the colours are materialised and travel with the particles again
    e.upload(L.F_PARTICLE_ID, (ids + 1000000).astype(np.int32))
    solver.advance(5)
    ids2, col2 = e.download(L.F_PARTICLE_ID), e.download(L.F_COLOR)
    lut = np.zeros((len(ids), 3), np.int32)
    lut[ids] = col
    assert np.array_equal(col2, lut[ids2 - 1000000])


def test_list_sort_with_boundary_particles(gpu, monkeypatch):
    """The same A/B where the scene is not all fluid (sampled domain box: the gather also flags the tiles that hold fluid, and
    k_hash_count -- not the force pass -- files the runs every step)."""
    cfg = H.dam_break_scene(domain_end=(0.6, 0.6, 0.6), end=(0.2, 0.2, 0.2), translation=(0.06, 0.06, 0.06),
                            add_domain_box=True)
    out = []
    for lists in (True, False):
        if not lists:
            monkeypatch.setenv("SPH_NO_RUN_LISTS", "1")
        container, solver = H.build_product(cfg)
        solver.prepare()
        for _ in range(10):
            solver.step()
        solver.advance(5)
        st = solver.stats()
        assert (st["list_sorts"] > 0) == lists, st
        out.append((_state(container), st))
    for k in ("x", "v", "rho", "p", "a", "V"):
        np.testing.assert_array_equal(out[0][0][k], out[1][0][k])
    assert out[0][1]["pair_interactions"] == out[1][1]["pair_interactions"]


def test_fluid_workgroup_list_changes_nothing(gpu, monkeypatch):
    """With a sampled domain box most workgroups hold no fluid; fluid-only functors launch the listed ones only.
    Same particles, same order of operations: bitwise the same state as with every workgroup launched."""
    cfg = H.dam_break_scene(domain_end=(0.6, 0.6, 0.6), end=(0.2, 0.2, 0.2), translation=(0.06, 0.06, 0.06),
                            add_domain_box=True)
    out = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("SPH_NO_BLOCK_LIST", "1")
        container, solver = H.build_product(cfg)
        solver.prepare()
        for _ in range(10):
            solver.step()
        out.append((_state(container), solver.stats()))
    for k in ("x", "v", "rho", "p", "a", "V"):
        np.testing.assert_array_equal(out[0][0][k], out[1][0][k])
    assert out[0][1]["pair_interactions"] == out[1][1]["pair_interactions"]


def test_bench_line_contract(gpu):
    """bench.py prints ONE JSON line with the fields the driver and the judge read (small configuration)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "c1", "--steps", "5", "--warmup", "2",
                        "--cpu-steps", "1", "--full"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert "workload" in d["config"] and "model" not in d["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"], k
    assert d["roofline"]["bound"] == "hbm" and abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-12
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert d["cpu_baseline"]["kind"] == "port" and d["value"] > d["cpu_baseline"]["value"] > 0


def test_bench_plain_run_is_the_headline_only(gpu):
    """Without --full bench.py times its steps and prints the line, and runs nothing of its own after them: no CPU baseline, no solo
    per-kernel event passes, no copy-rate measurement, no in-motion window, no extra scenes."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "c1", "--steps", "5", "--warmup", "2"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "particle-updates/sec" and d["unit"] == "particle-updates/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 5 and d["value"] > 0 and d["ms_per_step"] == d["repeat_ms_per_step"][0] > 0
    assert d["config"]["state"] == "steps 7..12 from the initial lattice", d["config"]["state"]   # warm-up 2 + pre-pass 5
    assert d["cpu_baseline"] is None and d["in_motion"] is None and "extras" not in d
    ro = d["roofline"]
    assert ro["achieved"] > 0 and ro["launches"] >= 5 and abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-12
    assert ro["measured_copy_gbs"] is None and ro["all_kernels"] is None and ro["runner_up"] is None


def _run_fast(cfg, steps, jitter=0.003, seed=2):
    container, solver = H.build_product(cfg, jitter=jitter, seed=seed, fast_math=1)
    solver.prepare()
    for _ in range(steps):
        solver.step()
    e = container.engine
    return e.download(L.F_PARTICLE_ID), e.download(L.F_POSITION), e.download(L.F_VELOCITY), e.download(L.F_DENSITY)


def test_uniform_mass_force_pass_is_the_generic_one_bit_for_bit(gpu, monkeypatch):
    """A scene with ONE fluid mass runs WcsphForcePass<true, true> in the fast build (the products with the mass hoisted out of the pair
    loop): the same roundings in the same order, so every field must be bit-identical to the generic instantiation (SPH_NO_UNIFORM_MASS)."""
    cfg = H.dam_break_scene(end=(0.3, 0.26, 0.22), translation=(0.13, 0.11, 0.07))
    monkeypatch.delenv("SPH_NO_UNIFORM_MASS", raising=False)
    a = _run_fast(cfg, 40)
    monkeypatch.setenv("SPH_NO_UNIFORM_MASS", "1")
    b = _run_fast(cfg, 40)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("with_plate", [False, True], ids=["fluid", "rigid"])
def test_force_pass_that_counts_its_own_pairs(gpu, monkeypatch, fast_math, with_plate):
    """the fused force pass leaves its pair statistics to the density pass whose masks it walks (State::density_books_forces).
    A launch that the density pass did not book for must count itself (WcsphForcePass<AF, false, true>, chosen by l_wcsph_forces):
    SPH_FORCES_COUNT_OWN makes wcsph_step take that road -- same state bit for bit, same pair_interactions, and the oracle's count."""
    cfg = H.dam_break_scene(end=(0.3, 0.26, 0.22), translation=(0.13, 0.11, 0.07), add_domain_box=with_plate)
    out = []
    for own in (False, True):
        if own:
            monkeypatch.setenv("SPH_FORCES_COUNT_OWN", "1")
        else:
            monkeypatch.delenv("SPH_FORCES_COUNT_OWN", raising=False)
        container, solver = H.build_product(cfg, fast_math=fast_math)
        solver.prepare()
        for _ in range(5):
            solver.step()
        e = container.engine
        out.append((e.download(L.F_PARTICLE_ID), e.download(L.F_POSITION), e.download(L.F_VELOCITY), solver.stats()))
    for k in range(3):
        np.testing.assert_array_equal(out[0][k], out[1][k])
    assert out[0][3]["pair_interactions"] == out[1][3]["pair_interactions"] > 0
    assert out[0][3]["pair_evaluations"] == out[1][3]["pair_evaluations"]
    ref = H.build_oracle(cfg)
    ref.prepare()
    ref.step(5)
    if not fast_math:
        assert out[1][3]["pair_interactions"] == ref.last_pairs


@pytest.mark.parametrize("fast_math", [0, 1])
def test_two_fluid_masses_against_the_oracle(gpu, fast_math):
    """Two touching fluid blocks of different density (masses 8e-3 and 5.6e-3): m_ij = (m_i + m_j) / 2 and the neighbour's mass in every
    pair term matter (base_solver.py:136-240) -- the uniform-mass instantiation would be wrong here and must not be chosen."""
    cfg = H.dam_break_scene(end=(0.16, 0.2, 0.16), translation=(0.1, 0.1, 0.1), velocity=(0.2, 0.0, 0.0))
    second = dict(cfg["FluidBlocks"][0], objectId=1, translation=[0.27, 0.107, 0.093], density=700.0, velocity=[-0.2, 0.0, 0.0], color=[200, 100, 50])
    cfg["FluidBlocks"].append(second)
    container, solver = H.build_product(cfg, fast_math=fast_math)   # (no jitter: the helpers perturb a multi-block scene block by block / all at once)
    solver.prepare()
    ref = H.build_oracle(cfg)
    ref.prepare()
    np.testing.assert_array_equal(container.engine.download(L.F_POSITION), ref.field("particle_positions"))
    m = container.engine.download(L.F_MASS)
    assert len(np.unique(m)) == 2
    solver.step()
    ref.step(1)
    assert solver.stats()["pair_interactions"] == ref.last_pairs     # (later, pairs at the edge of the support flip with the last bits)
    for _ in range(9):
        solver.step()
    ref.step(9)
    a, b = _state(container), _ref_state(ref)
    assert abs(solver.stats()["pair_interactions"] - ref.last_pairs) <= 1e-3 * ref.last_pairs
    d = H.drift(a["x"], b["x"], container.dh)
    assert d.max() <= 1e-5, d.max()
    np.testing.assert_allclose(a["v"], b["v"], rtol=0, atol=5e-5 * float(np.abs(b["v"]).max()))



def test_a_failed_step_drops_the_hash_made_for_its_successor(gpu, tmp_path):
    """NextHash relies on every failure path clearing `prehashed` / `cell_count_clean`.  The test-hook library fails step 4 of a
    sph_step_async(10) between its halves -- after the force pass has hashed for step 5 -- once; the call reports the error, the next call
    steps on, and the state after 10 steps' worth of device work equals that of an undisturbed run bit for bit (ids, positions, velocities):
    the abandoned histogram was cleared, the next sort hashed for itself."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = os.path.join(root, "sph_project_amd", "libsph_hip_testhooks.so")
    out = {}
    for tag, env in (("plain", {}), ("failed", {"SPH_TEST_FAIL_STEP": "4"})):
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "failed_step_probe.py"), "wcsph", str(tmp_path / (tag + ".npz"))],
                           env=dict(os.environ, SPH_HIP_LIB=hooks, **env), capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        out[tag] = (json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]), np.load(tmp_path / (tag + ".npz")))
    print(out["plain"][0], out["failed"][0])
    assert out["plain"][0]["failed"] == "" and "injected failure" in out["failed"][0]["failed"]
    assert out["failed"][0]["steps_after_failure"] == 4
    # one hash kernel more than the undisturbed run's two calls need: the sort after the failure could not use the abandoned hash
    assert out["failed"][0]["hash_launches"] == out["plain"][0]["hash_launches"] + 1, (out["plain"][0], out["failed"][0])
    for k in ("ids", "pos", "vel"):
        np.testing.assert_array_equal(out["plain"][1][k], out["failed"][1][k])
    assert out["plain"][0]["pairs"] == out["failed"][0]["pairs"]
