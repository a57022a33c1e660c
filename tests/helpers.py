"""Shared scene builders for the tests: one JSON-like scene dict feeds both the product containers
(HIP) and the oracle (CPU), so the comparison reads like `reference scene in -> state out`."""
import copy

import numpy as np

from oracle import ref as oracle_ref
from sph_project_amd import scene
from sph_project_amd.product import dam_break_scene, scene_particles  # noqa: F401 (shared with bench.py / smoke())
from sph_project_amd import product as _product
from sph_project_amd import _lib as _L
from sph_project_amd.SPH.utils import SimConfig  # noqa: F401 (re-exported for tests)


# Cell layers in z from which the fast build mixes the outer candidate runs of a neighbour walk's staging groups (sph_api.hip
# refresh_counts: run_grouping = fast_math && !slab_active && nz >= 40; sph_device.hpp run_of).
MIXED_RUN_LAYERS = 40


def with_layers(cfg_dict, layers):
    """A copy of the scene whose domain has `layers` cell layers in z and is otherwise the same.  The cell index is (cx ny + cy) nz + cz,
    lexicographic in (cx, cy, cz) whatever nz is: the same particles keep their sorted order, their 256-particle tiles and their
    neighbours, so between two heights only what depends on nz itself changes -- the staging groups (MIXED_RUN_LAYERS) and the chain
    staging of thin grids.  grid_num = ceil(size / cell) (scene.derive_geometry) gives `layers` for every extent in (layers - 1, layers]
    cells; the interval is open below, so the extent taken is its middle, layers - 1/2 cells: one cell less is again a middle."""
    cfg = copy.deepcopy(cfg_dict)
    geo = scene.derive_geometry(SimConfig(config=cfg))
    assert geo.dim == 3
    cfg["Configuration"]["domainEnd"][2] = float(geo.domain_start[2] + (layers - 0.5) * geo.grid_size)
    tall = scene.derive_geometry(SimConfig(config=cfg))
    assert int(tall.grid_num[2]) == layers and (tall.grid_num[:2] == geo.grid_num[:2]).all(), (tall.grid_num, layers)
    return cfg


def perturb(pos, amplitude, seed=0):
    rng = np.random.default_rng(seed)
    return (pos + rng.uniform(-amplitude, amplitude, pos.shape)).astype(np.float32)


def _oracle_insert(sim, b, jitter=0.0, seed=0):
    n = b["pos"].shape[0]
    pos = perturb(b["pos"], jitter, seed) if (jitter > 0 and b["material"][0] == 1) else b["pos"]
    color = np.zeros((n, 3), np.int32)
    color[:, 0] = np.arange(sim._next_id, sim._next_id + n)
    sim._next_id += n
    if b["object_id"] >= 0:
        sim.set_object(b["object_id"], int(b["material"][0]), 0)
    sim.add_particles(b["object_id"], pos, b["vel"], b["density"], np.zeros(n, np.float32), b["material"],
                      b["is_dynamic"], color)


def build_oracle(cfg_dict, jitter=0.0, seed=0, fixed_iterations=0):
    """Oracle fed like BaseSolver.prepare() feeds the reference: objects whose entryTime has come at t = 0 are inserted
    now, the others wait in sim._pending for oracle_step() (base_container.py:218-221)."""
    cfg, geo, batches = scene_particles(cfg_dict)
    sol = scene.derive_solver_constants(cfg)
    total = sum(b["pos"].shape[0] for b in batches)
    pd = scene.params_dict(geo, sol, cfg.get_cfg("simulationMethod"), total, fixed_iterations=fixed_iterations)
    sim = oracle_ref.RefSim(pd)
    sim._next_id = 0
    sim._pending = []
    sim._time = 0.0
    sim._dt = float(np.float32(sol.dt))   # solver.dt[None] is an f32 field (base_solver.py:35-36)
    for b in batches:
        if b["entry_time"] > sim._time:
            sim._pending.append(b)
        else:
            _oracle_insert(sim, b, jitter, seed)
    return sim


class ArraysAsEngine:
    """The part of the product engine's interface oracle_from_product reads (download / particle_num / fluid_particle_num), served
    from host arrays keyed by the engine's field ids.  Lets the seeding be fed from anything with the product's layout: the state
    arrays of oracle_from_state's callers, or another oracle's fields (oracle_as_engine) for the CPU tests of the seeding itself."""

    def __init__(self, fields, fluid_particle_num):
        self.fields = fields
        self.particle_num = len(fields[_L.F_PARTICLE_ID])
        self.fluid_particle_num = int(fluid_particle_num)

    def download(self, fid):
        return np.array(self.fields[fid], copy=True)


def oracle_as_engine(sim):
    """An oracle's per-particle state as the engine would download it: slot order, ids from the colour word, cg_x slot-indexed."""
    names = {_L.F_POSITION: "particle_positions", _L.F_VELOCITY: "particle_velocities", _L.F_DENSITY: "particle_densities",
             _L.F_REST_VOLUME: "particle_rest_volumes", _L.F_MASS: "particle_masses", _L.F_MATERIAL: "particle_materials",
             _L.F_OBJECT_ID: "particle_object_ids", _L.F_IS_DYNAMIC: "particle_is_dynamic", _L.F_CG_X: "cg_x"}
    fields = {fid: sim.field(name).copy() for fid, name in names.items()}
    fields[_L.F_PARTICLE_ID] = oracle_ids(sim)
    return ArraysAsEngine(fields, sim.fluid_particle_num)


def oracle_from_product(cfg_dict, engine, fixed_iterations=0):
    """An oracle holding the particles of `engine` (the product's, or anything with its download interface) in its current slot
    order -- the stable counting sorts of both sides then keep them aligned -- with every per-particle value the reference carries
    from one step to the next (oracle/sph_ref.c): positions, velocities, ids (colour word, like build_oracle), object ids, is_dynamic,
    densities, rest volumes, masses, materials, and the CG warm start.  For comparisons that start from a state the PRODUCT has reached
    (a collapsed column at step 2500, the emitter scene in the state bench.py times), which the oracle could only reach by itself in
    hours.  What is recomputed rather than carried: prepare() re-sorts (a no-op permutation on a sorted state), recomputes the rest
    volumes of boundary particles at or below gravitationUpper and, for DFSPH, density and alpha -- exactly what the end of the
    previous step left (base_solver.py:696, DFSPH.py:316-321).  Refused: late blocks (entryTime > 0: their insertion time is host
    state) and rigid bodies (their pose is)."""
    cfg, geo, batches = scene_particles(cfg_dict)
    assert not (cfg.get_rigid_bodies() or cfg.get_rigid_blocks()), "oracle_from_product: rigid bodies carry a pose the seeding does not copy"
    assert all(b["entry_time"] <= 0 for b in batches), "oracle_from_product: a late block would need the host's insertion time"
    fluid_objects = sorted({int(b["object_id"]) for b in batches if b["material"][0] == 1})
    sol = scene.derive_solver_constants(cfg)
    get = engine.download
    ids, x, v, rho = get(_L.F_PARTICLE_ID), get(_L.F_POSITION), get(_L.F_VELOCITY), get(_L.F_DENSITY)
    vol, mass, mat, obj, dyn = get(_L.F_REST_VOLUME), get(_L.F_MASS), get(_L.F_MATERIAL), get(_L.F_OBJECT_ID), get(_L.F_IS_DYNAMIC)
    n = len(ids)
    assert n == engine.particle_num and np.array_equal(np.sort(ids), np.arange(n))
    assert set(np.unique(obj).tolist()) <= {-1, *fluid_objects}, np.unique(obj)
    g_upper = np.float32(sol.g_upper)
    # Emitter-frozen fluid: material 2 in a fluid object, above gravitationUpper (base_solver.py:670).  The reference counts a particle
    # as fluid only when it is ADDED with material 1 (sph_ref.c sphref_add_particles, base_container.py:797): add it as fluid, freeze it
    # afterwards -- fluid_particle_num, the denominator of PCISPH's stop test, counts it.
    frozen = (mat == 2) & np.isin(obj, fluid_objects)
    assert (x[frozen, 1] > g_upper).all(), "a frozen fluid particle at or below gravitationUpper"
    # ... and no ACTIVE fluid above it, so the prepare_emitter() of prepare() changes nothing
    assert not (x[mat == 1, 1] > g_upper).any(), "an active fluid particle above gravitationUpper"
    sim = oracle_ref.RefSim(scene.params_dict(geo, sol, cfg.get_cfg("simulationMethod"), n, fixed_iterations=fixed_iterations))
    sim._next_id = n
    sim._pending = []
    sim._time = 0.0   # only late blocks read it (oracle_step), and there are none
    sim._dt = float(np.float32(sol.dt))
    for o in fluid_objects:   # object materials decide who the emitter may move (base_solver.py:660-666)
        sim.set_object(o, 1, 0)
    color = np.zeros((n, 3), np.int32)
    color[:, 0] = ids
    sim.add_particles(-1, x, v, rho, np.zeros(n, np.float32), np.where(frozen, 1, mat), dyn, color)
    sim.field("particle_materials")[:] = mat
    sim.field("particle_object_ids")[:] = obj
    # add_particles sets rest volume V0 and mass V0 x density; the product's carry what the reference's boundary-volume pass and the
    # insertion left (fluid: V0 and V0 rho0, also for fluid the emitter released -- frozen particles sit above gravitationUpper, where
    # that pass skips them, so none ever gets a boundary volume; boundary particles: 1 / sum W)
    sim.field("particle_rest_volumes")[:] = vol
    sim.field("particle_masses")[:] = mass
    if cfg.get_cfg("viscosityMethod") == "implicit":
        # CG warm start x - v of the last solve (base_solver.py:440): slot-indexed, NOT reordered by the sort (sph_ref.c prepare_cg1)
        sim.field("cg_x")[:] = get(_L.F_CG_X)
    assert sim.fluid_particle_num == engine.fluid_particle_num, (sim.fluid_particle_num, engine.fluid_particle_num)
    return sim


def oracle_from_state(cfg_dict, x, v, ids, fixed_iterations=0):
    """oracle_from_product for a ONE-fluid-block scene from positions / velocities / ids alone: every particle is active fluid of
    that block with the block's is_dynamic (base_solver.py:139 / :555 look at is_dynamic of FLUID particles too), rest volume V0 and
    the mass the reference derives from the block's rest density at insertion (base_container.py:404-438); the current density is
    recomputed every step."""
    cfg, geo, batches = scene_particles(cfg_dict)
    assert len(batches) == 1 and batches[0]["material"][0] == 1
    b = batches[0]
    n = len(ids)
    v0 = np.float32(geo.V0)
    fields = {_L.F_PARTICLE_ID: ids, _L.F_POSITION: x, _L.F_VELOCITY: v, _L.F_DENSITY: np.full(n, b["density"][0], np.float32),
              _L.F_REST_VOLUME: np.full(n, v0, np.float32), _L.F_MASS: np.full(n, v0 * np.float32(b["density"][0]), np.float32),
              _L.F_MATERIAL: np.full(n, 1, np.int32), _L.F_OBJECT_ID: np.full(n, b["object_id"], np.int32),
              _L.F_IS_DYNAMIC: np.full(n, b["is_dynamic"][0], np.int32), _L.F_CG_X: np.zeros((n, 3), np.float32)}
    return oracle_from_product(cfg_dict, ArraysAsEngine(fields, n), fixed_iterations=fixed_iterations)


def oracle_step(sim, n=1):
    """solver.step() of the reference with its host part: _step() inserts the objects that are due in the middle of the
    step (WCSPH.py:41, DFSPH.py:307, PCISPH.py:181), then total_time advances (base_solver.py:694)."""
    for _ in range(n):
        if not sim._pending:
            sim.step(1)
        else:
            sim.step_begin()
            due = [b for b in sim._pending if not (b["entry_time"] > sim._time)]
            sim._pending = [b for b in sim._pending if b["entry_time"] > sim._time]
            for b in due:
                _oracle_insert(sim, b)
            sim.step_end()
        sim._time += sim._dt


def oracle_ids(sim):
    return sim.field("particle_colors")[:, 0].copy()


def build_product(cfg_dict, jitter=0.0, seed=0, **engine_opts):
    """Product containers driven exactly like run_simulation.py drives the reference (sph_project_amd.product), plus the
    tests' seeded perturbation of the fluid lattice."""
    container, solver = _product.build_product(cfg_dict, **engine_opts)
    if jitter > 0:
        # same perturbed fluid lattice as build_oracle: insert, then overwrite positions before prepare()
        container.insert_object()
        solver.rigid_solver.insert_rigid_object()
        from sph_project_amd import _lib as L
        pos = container.engine.download(L.F_POSITION)
        mat = container.engine.download(L.F_MATERIAL)
        fl = mat == 1
        pos[fl] = perturb(pos[fl], jitter, seed)
        container.engine.upload(L.F_POSITION, pos)
    return container, solver


def by_id(ids, arr):
    """Reorder `arr` (current sorted order) into particle-id order."""
    out = np.empty_like(arr)
    out[ids] = arr
    return out


def drift(x, x_ref, dh):
    """SURVEY 8(c) parity metric: |x - x_ref| / max(|x_ref|, dh), per particle."""
    num = np.linalg.norm(x.astype(np.float64) - x_ref.astype(np.float64), axis=1)
    den = np.maximum(np.linalg.norm(x_ref.astype(np.float64), axis=1), dh)
    return num / den


def _pair_list(x, h, rows=None):
    """Directed pairs (o, i, j) with |x_i - x_j| <= h (1 + 1e-6), i != j, from a KD-tree: i over every particle (o = i), or only over
    `rows` (o = position in `rows`) -- a sample of a 1.23 M state is queried without building its whole pair list."""
    from scipy.spatial import cKDTree
    tree = cKDTree(x)
    if rows is None:
        pairs = tree.query_pairs(h * (1 + 1e-6), output_type="ndarray")
        i = np.concatenate([pairs[:, 0], pairs[:, 1]])
        return i, i, np.concatenate([pairs[:, 1], pairs[:, 0]])
    rows = np.asarray(rows)
    lists = tree.query_ball_point(x[rows], h * (1 + 1e-6))
    cnt = np.array([len(l) for l in lists])
    o = np.repeat(np.arange(len(rows)), cnt)
    i = rows[o]
    j = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if len(lists) else np.zeros(0, np.int64)
    keep = i != j
    return o[keep], i[keep], j[keep]


def wcsph_pressure_accel_f64(x, rho, prs, mass, vol, mat, h, rho0, rows=None, pair_terms=False):
    """The reference's pressure acceleration (base_solver.py:136-178 with the cubic kernel gradient of base_solver.py:41-58)
    restated in float64 over a KD-tree pair list -- an independent evaluation, not the oracle: a_i = -sum_j m_j (p_i / rho_i^2 +
    p_j / rho_j^2) grad W_ij over fluid neighbours, -rho0 V_j p_i / rho_i^2 grad W_ij over boundary neighbours.
    Returns per particle and component (rows of non-fluid particles are zero): the sum, sum_j |term_j|, and sum_j |term_j| amp_j with
    amp_j = |q W'' / W'| the factor by which a relative error of q = r / h shows up in the term: 2 q / (1 - q) on the outer branch
    ((1 - q)^2 cancels towards the edge of the support), |6 q - 2| / |3 q - 2| <= 2 on the inner one.
    `rows`: evaluate only these particles (rows of the result follow `rows`); their neighbours come from the whole state.
    `pair_terms`: a fourth result, the pair terms themselves -- dict(o, i, j, t, t_amp) with t the (pairs, 3) terms of the sum and t_amp
    their |term| amp -- for the reaction onto rigid bodies (tests/nonpressure_terms.py pressure_wrench_f64)."""
    x = x.astype(np.float64)
    o, i, j = _pair_list(x, h, rows)
    n = len(x) if rows is None else len(rows)
    R = x[i] - x[j]
    r = np.linalg.norm(R, axis=1)
    keep = (mat[i] == 1) & (r > 1e-5) & (r <= h)
    o, i, j, R, r = o[keep], i[keep], j[keep], R[keep], r[keep]
    q = r / h
    kg = 6.0 * (8.0 / np.pi) / h ** 3
    s = np.where(q <= 0.5, kg * q * (3 * q - 2), -kg * (1 - q) ** 2) / (r * h)
    s_amp = np.where(q <= 0.5, kg * q * np.abs(6 * q - 2), kg * 2 * q * (1 - q)) / (r * h)   # |s| amp, finite at q = 1
    pt = prs.astype(np.float64) / rho.astype(np.float64) ** 2
    coef = np.where(mat[j] == 1, mass[j].astype(np.float64) * (pt[i] + pt[j]), rho0 * vol[j].astype(np.float64) * pt[i])
    t = -(coef * s)[:, None] * R
    a, mag, mag_amp = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    np.add.at(a, o, t)
    np.add.at(mag, o, np.abs(t))
    t_amp = np.abs((coef * s_amp)[:, None] * R)
    np.add.at(mag_amp, o, t_amp)
    if pair_terms:
        return a, mag, mag_amp, dict(o=o, i=i, j=j, t=t, t_amp=t_amp)
    return a, mag, mag_amp


def dfsph_alpha_f64(x, vol, mat, h):
    """DFSPH.py:23-62 restated in float64 over a KD-tree pair list (independent of the oracle): with g_ij = V_j grad W_ij,
    S_i = sum_{j fluid} |g_ij|^2 + |sum_{j all} g_ij|^2 and alpha_i = 1 / S_i if S_i > 1e-5, else 0 (fluid particles; other rows 0).
    Returns (S, B): B bounds |S_f32 - S| for ANY f32 evaluation of the same sums in any order (backward error, the pressure helper's
    model): every component of g_ij carries a relative error eps_j = 1e-5 + 5e-7 amp_j -- ~12 roundings of the term (difference, r,
    q, the polynomial, V_j x, the division by r h; v_rsq / v_rcp 1 ulp each in the fast build) plus a sum of <= 64 terms, (12 + 64) u =
    4.5e-6 < 1e-5, and the ~3 roundings that reach q = r / h times the kernel gradient's conditioning in q, amp_j = |q W'' / W'|
    (2 q / (1 - q) on the outer branch: a neighbour near the edge of the support carries the cancellation 1 - q) -- so
      |d sum_j |g_ij|^2| <= sum_j |g_ij|^2 (2 eps_j + 3 u)                       (each square: two factors, three roundings)
      |d s_c| <= E_c = sum_j |g_ij,c| eps_j,   s = sum_j g_ij                      (the vector sum)
      |d |s|^2| <= sum_c (2 |s_c| E_c + E_c^2) + 3 u |s|^2
    B is the sum of the two.  Then 1 / S_f32 lies in [1 / (S + B), 1 / (S - B)] widened by the division's rounding (the fast build's
    v_rcp: 1 ulp) where S - B > 0."""
    x = x.astype(np.float64)
    n = len(x)
    _, i, j = _pair_list(x, h)
    R = x[i] - x[j]
    r = np.linalg.norm(R, axis=1)
    keep = (mat[i] == 1) & (r > 1e-5) & (r <= h) & ((mat[j] == 1) | (mat[j] == 2))
    i, j, R, r = i[keep], j[keep], R[keep], r[keep]
    q = r / h
    kg = 6.0 * (8.0 / np.pi) / h ** 3
    sc = np.where(q <= 0.5, kg * q * (3 * q - 2), -kg * (1 - q) ** 2) / (r * h)
    amp = np.where(q <= 0.5, np.abs(6 * q - 2) / np.maximum(np.abs(3 * q - 2), 1e-300), 2 * q / np.maximum(1 - q, 1e-300))
    g = (vol[j].astype(np.float64) * sc)[:, None] * R
    u = 2.0 ** -24
    eps = 1e-5 + 5e-7 * amp
    fl_j = mat[j] == 1
    g2 = np.where(fl_j, (g * g).sum(axis=1), 0.0)
    sq = np.bincount(i, g2, minlength=n)
    sq_err = np.bincount(i, g2 * (2 * eps + 3 * u), minlength=n)
    s = np.stack([np.bincount(i, g[:, c], minlength=n) for c in range(3)], axis=1)
    E = np.stack([np.bincount(i, np.abs(g[:, c]) * eps, minlength=n) for c in range(3)], axis=1)
    s2 = (s * s).sum(axis=1)
    S = sq + s2
    B = sq_err + (2 * np.abs(s) * E + E * E).sum(axis=1) + 3 * u * s2
    fl = mat == 1
    return np.where(fl, S, 0.0), np.where(fl, B, 0.0)


def dfsph_density_derivative_f64(x, v, vol, mat, h):
    """DFSPH.py:66-98 restated in float64 over a KD-tree pair list (independent of the oracle): (D rho / Dt) / rho0 of particle i =
    max(sum_j V_j (v_i - v_j) . grad W_ij, 0), zero where the particle has fewer than 20 neighbours.  Returns (value before the
    neighbour-count rule, sum_j sum_c |V_j (v_i - v_j)_c grad W_c|, neighbour count with the support radius shrunk / grown by 1e-6):
    the two counts bracket what an f32 `r < h` can decide for pairs that sit exactly one support radius apart (lattices)."""
    from scipy.spatial import cKDTree
    x, v = x.astype(np.float64), v.astype(np.float64)
    n = len(x)
    pairs = cKDTree(x).query_pairs(h * (1 + 1e-6), output_type="ndarray")
    i = np.concatenate([pairs[:, 0], pairs[:, 1]])
    j = np.concatenate([pairs[:, 1], pairs[:, 0]])
    keep = mat[i] == 1
    i, j = i[keep], j[keep]
    R = x[i] - x[j]
    r = np.linalg.norm(R, axis=1)
    n_hi = np.bincount(i, minlength=n)
    n_lo = np.bincount(i[r < h * (1 - 1e-6)], minlength=n)
    q = r / h
    kg = 6.0 * (8.0 / np.pi) / h ** 3
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(q <= 0.5, kg * q * (3 * q - 2), -kg * (1 - q) ** 2) / (r * h)
    s = np.where((r > 1e-5) & (q <= 1.0), s, 0.0)
    prod = (v[i] - v[j]) * R * (vol[j].astype(np.float64) * s)[:, None]
    return np.bincount(i, prod.sum(axis=1), minlength=n), np.bincount(i, np.abs(prod).sum(axis=1), minlength=n), n_lo, n_hi
