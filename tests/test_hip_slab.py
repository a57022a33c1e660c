"""GPU: z-slab sharding.  Several ranks (one process each) share this box's single GPU.  Control plane: the shared-memory
segment (RCCL refuses two ranks on one device).  Data plane, both tested against the undecomposed CPU oracle:
  * "shm+ipc": the PUSH transport -- the production data plane: halo records and field messages are written by the sending
    rank's kernels straight into the neighbour's inbox (hipIpc mapping), headers / message numbers / waits on the device,
    WCSPH steps fully asynchronous (device-resident counts, launches from bounds);
  * "shm": host-staged mailboxes (the older test rig; same classify / unpack / table kernels as the RCCL send/recv fallback)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sph_project_amd import _lib as L
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


TRANSPORT = ["shm+ipc"]   # set by the fixture below for the running test
LAYOUT = [""]             # SPH_SLAB_LAYOUT of the running test ("": default, slabs along the fastest axis of the cell order)


@pytest.fixture(autouse=True, params=["shm+ipc", "shm"])
def transport(request):
    TRANSPORT[0] = request.param
    return request.param


def _pairs_agree(got, want):
    """Accepted-pair counts of a sharded run against the undecomposed oracle.  A sharded library works in a frame whose axes are a
    permutation of the scene's (the slab axis is its slowest sort axis: csrc/sph_api.hip set_axis_order), so r^2 = dx^2 + dy^2 + dz^2 is
    summed in another order and a pair within an ulp of the support radius can fall on the other side: a few in 10^6, not one more."""
    assert abs(int(got) - int(want)) <= max(2, 2e-5 * int(want)), (got, want)


# Worker processes of one run.  The test process has the GPU open as well, and a GPU shared with other users takes at most six processes
# at once: more ranks than this share processes (rank r runs in process r % MAX_PROCS, in a thread of its own; no two neighbours share one).
MAX_PROCS = 4


def _run_ranks(cfg, nranks, steps, tmp_path, jitter=0.0, seed=0, fixed_iterations=0, rebalance=0, advance=False, extra_env=None, timeout=None):
    tmp_path.mkdir(parents=True, exist_ok=True)
    scene_path = tmp_path / "scene.json"
    scene_path.write_text(json.dumps(cfg))
    uid = os.urandom(128).hex()
    env = dict(os.environ, SPH_COMM_TRANSPORT=TRANSPORT[0], SPH_FIXED_ITERATIONS=str(fixed_iterations), SPH_SLAB_REBALANCE=str(rebalance),
               SPH_WORKER_ADVANCE="1" if advance else "0", SPH_COMM_TIMEOUT_S="40")
    if LAYOUT[0]:
        env["SPH_SLAB_LAYOUT"] = LAYOUT[0]
    env.update(extra_env or {})
    nprocs = min(nranks, MAX_PROCS)
    groups = [list(range(i, nranks, nprocs)) for i in range(nprocs)]
    procs = []
    for g in groups:
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "slab_worker.py"), ",".join(map(str, g)), str(nranks), uid,
                                       str(scene_path), str(steps), str(tmp_path / "rank{rank}.npz"), str(jitter), str(seed)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    plogs = []
    for p in procs:
        o, _ = p.communicate(timeout=timeout or int(os.environ.get("SPH_TEST_RANK_TIMEOUT", "300")))
        plogs.append(o.decode())
    if any(p.returncode != 0 for p in procs):   # (the rank that reports "a neighbour failed" is rarely the one that says why)
        raise AssertionError("\n".join(f"---- ranks {g} (exit {p.returncode}):\n{plogs[i][-1500:]}" for i, (g, p) in enumerate(zip(groups, procs))))
    logs = [plogs[r % nprocs] for r in range(nranks)]   # (the log of the process that ran the rank)
    outs = [np.load(tmp_path / f"rank{r}.npz") for r in range(nranks)]
    if extra_env and "SPH_COMM_TRANSPORT" in extra_env:
        return outs, logs
    want = "ipc-push+shm" if TRANSPORT[0] == "shm+ipc" else "shm"
    assert all(str(o["transport"]) == want for o in outs), [str(o["transport"]) for o in outs]   # no silent fall-back in the tests
    return outs, logs


@pytest.fixture
def slow_layout(transport):
    """SPH_SLAB_LAYOUT=slow for the ranks of this test: the scene's z is mapped onto the library's x (its slowest sort axis, library axes =
    scene z, x, y at the C-ABI boundary), WCSPH passes run boundary tiles first and the halo messages go out behind them (round 4; measured
    slower than the default layout on thin slabs, kept as an option: DESIGN.md).  The overlap rides on the push transport; over the
    mailboxes the same permuted frame runs without it."""
    LAYOUT[0] = "slow"
    yield
    LAYOUT[0] = ""


@pytest.mark.parametrize("nranks", [2, 3])
def test_slow_axis_layout_with_overlap_matches_oracle(gpu, tmp_path, nranks, slow_layout):
    """The same scene and limits as test_slab_sharding_matches_oracle[advance] in the other layout: every vector crosses the ABI through
    the axis permutation, the step message of step k + 1 is started behind the boundary tiles of step k's force pass, the field message
    behind the boundary tiles of the density pass."""
    test_slab_sharding_matches_oracle(gpu, tmp_path, nranks, True)


def test_slow_axis_layout_dfsph_and_a_dynamic_rigid_body(gpu, tmp_path, slow_layout):
    """Solver loops (exact launches, no overlap) and the rigid hook in the permuted frame: pose in, wrench out, with the sign of the
    axial vectors (angular velocity, torque) under the permutation."""
    test_dfsph_slab_sharding_matches_oracle(gpu, tmp_path, 2, 3)
    test_dynamic_rigid_body_under_slab_sharding(gpu, tmp_path)


@pytest.mark.parametrize("advance", [False, True], ids=["step", "advance"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_slab_sharding_matches_oracle(gpu, tmp_path, nranks, advance):
    """advance: all 40 steps handed to the device in ONE call -- over the push transport they run without a single host
    read-back (device-resident counts, launch bounds from the pinned mirror); step: one call and one settle per step."""
    # a block that spans the domain in z and falls / spreads for 40 steps: particles migrate across slab faces
    cfg = H.dam_break_scene(domain_end=(1.0, 1.0, 1.2), start=(0.1, 0.1, 0.08), end=(0.4, 0.4, 1.12), translation=(0, 0, 0),
                            velocity=(0.0, -0.3, 2.5), particleSpacing=0.019)
    steps = 40
    outs, logs = _run_ranks(cfg, nranks, steps, tmp_path, jitter=0.002, seed=3, advance=advance)
    # the undecomposed CPU oracle on the same seeded scene is the reference (not a single-rank run of the same library)
    ref = H.build_oracle(cfg, jitter=0.002, seed=3)
    ref.prepare()
    ref.step(steps)
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    rho_ref = H.by_id(ids, ref.field("particle_densities").copy())
    _, geo, _b = H.scene_particles(cfg)
    dh, nz = geo.dh, int(geo.grid_num[2])
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids), "every particle owned by exactly one rank"
    x = np.empty_like(x_ref)
    rho = np.empty_like(rho_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]
        rho[o["ids"]] = o["rho"]
        assert int(o["n_ghost"]) > 0
    d = H.drift(x, x_ref, dh)
    print("slab x%d drift max %.3e; owned per rank %s" % (nranks, d.max(), [len(o["ids"]) for o in outs]))
    assert d.max() <= 1e-5
    np.testing.assert_allclose(rho, rho_ref, rtol=2e-5)
    # ownership follows the particles: somebody changed slab during the run
    cuts = outs[0]["cuts"]
    from sph_project_amd import slab
    cz0 = slab.cell_layer(_b[0]["pos"][:, 2], dh, nz)
    cz1 = slab.cell_layer(x[:, 2], dh, nz)
    assert (slab.owner_of(cz0, cuts) != slab.owner_of(cz1, cuts)).sum() > 0
    _pairs_agree(sum(int(o["pairs"]) for o in outs), ref.last_pairs)


@pytest.mark.parametrize("nranks,fixed", [(2, 3), (3, 3), (2, 0), (3, 0)])
def test_pcisph_slab_sharding_matches_oracle(gpu, tmp_path, nranks, fixed):
    """PCISPH under z-slab sharding: per refine iteration the ghosts' p / rho^2 goes out between the rho* pass and the
    pressure-acceleration pass and their predicted positions after it; the density error is all-reduced (PCISPH.py:110-125)."""
    cfg = H.dam_break_scene(method="pcisph", domain_end=(1.0, 1.0, 1.2), start=(0.1, 0.1, 0.08), end=(0.34, 0.34, 1.1),
                            translation=(0, 0, 0), velocity=(0.0, -0.3, 1.5), particleSpacing=0.0165, dt=4e-4)
    # measured iterations: stop before the column reaches the lid -- there the reference's loop runs into its 1000-iteration
    # cap without converging (oracle and HIP agree on that, step for step) and amplifies f32 rounding differences
    steps = 20 if fixed else 8
    outs, logs = _run_ranks(cfg, nranks, steps, tmp_path, jitter=0.0015, seed=6, fixed_iterations=fixed)
    ref = H.build_oracle(cfg, jitter=0.0015, seed=6, fixed_iterations=fixed)
    ref.prepare()
    hist_ref = []
    for _ in range(steps):
        ref.step(1)
        hist_ref.append((int(ref.scalar("last_iter_pci")), ref.scalar("last_err_pci")))
    print("per step (iterations, error): oracle", hist_ref)
    print("per step (iterations, error): rank 0", [(int(r[0]), float("%.4e" % r[1])) for r in outs[0]["hist"]])
    if not fixed:
        assert max(h[0] for h in hist_ref) < 1000 and max(h[0] for h in hist_ref) >= 10
        # (the all-reduced sum is added up in another order than the oracle's: a step whose error passes the threshold by less
        #  than that rounding may stop one iteration apart -- SURVEY 8c; none does in this scene, +-1 keeps the test from flaking)
        assert max(abs(int(r[0]) - h[0]) for r, h in zip(outs[0]["hist"], hist_ref)) <= 1
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    prs_ref = H.by_id(ids, ref.field("particle_pressures").copy())
    _, geo, _b = H.scene_particles(cfg)
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids)
    x, prs = np.empty_like(x_ref), np.empty_like(prs_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]; prs[o["ids"]] = o["prs"]
        assert int(o["n_ghost"]) > 0
    d = H.drift(x, x_ref, geo.dh)
    it_ref = int(ref.scalar("last_iter_pci"))
    print("pcisph slab x%d fixed=%d: drift max %.3e, iterations per rank %s (err %s), oracle %d (err %.3e), max p %.1f" % (
        nranks, fixed, d.max(), [int(o["iter_pcisph"]) for o in outs], ["%.3e" % float(o["err_pcisph"]) for o in outs], it_ref,
        ref.scalar("last_err_pci"), prs_ref.max()))
    assert prs_ref.max() > 0, "the pressure solver has work to do in this scene"
    if fixed:
        assert d.max() <= 1e-5
        np.testing.assert_allclose(prs, prs_ref, rtol=0, atol=1e-3 * float(prs_ref.max()))   # regression guard (PCISPH's p accumulates k (rho0 - rho*) over the iterations; fitted, re-fitted when the sharded frame changed its summation order)
        _pairs_agree(sum(int(o["pairs"]) for o in outs), ref.last_pairs)
    else:
        assert d.max() <= 1e-5


@pytest.mark.parametrize("method,nranks", [("wcsph", 2), ("wcsph", 3), ("dfsph", 2), ("pcisph", 2)])
def test_implicit_viscosity_slab_sharding_matches_oracle(gpu, tmp_path, method, nranks):
    """Implicit viscosity under z-slab sharding (base_solver.py:445-517): the ghosts' search direction goes out before every
    A p pass, the dot products are all-reduced, the solved velocities of the ghosts follow the loop.  The reference keeps
    last step's solution as the initial guess WITHOUT reordering it with the particles (slot-indexed), so a sharded run starts
    its solves from a slightly different guess than an undecomposed one: both run the reference's stop test (|r| <= 1e-6),
    take the same number of iterations (+-1) and agree to the solver's tolerance, not to rounding."""
    cfg = H.dam_break_scene(method=method, domain_end=(1.0, 1.0, 1.2), start=(0.1, 0.1, 0.08), end=(0.36, 0.36, 1.12),
                            translation=(0, 0, 0), velocity=(0.0, -0.3, 2.0), particleSpacing=0.019, dt=4e-4,
                            viscosity=50.0, viscosity_method="implicit")
    steps = 12
    outs, logs = _run_ranks(cfg, nranks, steps, tmp_path, jitter=0.002, seed=8, fixed_iterations=0)
    ref = H.build_oracle(cfg, jitter=0.002, seed=8)
    ref.prepare()
    it_ref = []
    for _ in range(steps):
        ref.step(1)
        it_ref.append(int(ref.scalar("last_iter_cg")))
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    v_ref = H.by_id(ids, ref.field("particle_velocities").copy())
    _, geo, _b = H.scene_particles(cfg)
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids)
    x, v = np.empty_like(x_ref), np.empty_like(v_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]; v[o["ids"]] = o["vel"]
        assert int(o["n_ghost"]) > 0
    it = [[int(r[2]) for r in o["hist"]] for o in outs]
    d = H.drift(x, x_ref, geo.dh)
    dv = np.abs(v - v_ref).max() / np.abs(v_ref).max()
    print("implicit %s slab x%d: drift max %.3e, |dv|/vmax %.3e, CG iterations per step %s, oracle %s" % (method, nranks, d.max(), dv, it[0], it_ref))
    assert all(i == it[0] for i in it), "every rank runs the same number of iterations"
    assert max(it_ref) >= 5, "the solver has work to do in this scene"
    # (the warm start is slot-indexed; ghost slots are zeroed after a solve so that no neighbour-rank velocity is taken for a guess)
    assert max(abs(a - b) for a, b in zip(it[0], it_ref)) <= 1
    assert d.max() <= 1e-6 and dv <= 1e-5


@pytest.mark.parametrize("nranks,fixed", [(2, 3), (3, 3), (2, 0)])
def test_dfsph_slab_sharding_matches_oracle(gpu, tmp_path, nranks, fixed):
    """DFSPH under z-slab sharding: per solver iteration the ghosts' kappa goes out before the correction
    pass and their velocities after it, the residual is all-reduced over the ranks (DFSPH.py:139-159, :225-243).
    fixed > 0: both sides do exactly that many iterations (bitwise-comparable work); fixed = 0: the reference's own
    stop tests on the all-reduced residual (the sum order differs from a single rank's, so +-1 iteration is allowed)."""
    cfg = H.dam_break_scene(method="dfsph", domain_end=(1.0, 1.0, 1.2), start=(0.1, 0.1, 0.08), end=(0.36, 0.36, 1.12),
                            translation=(0, 0, 0), velocity=(0.0, -0.3, 2.0), particleSpacing=0.019, dt=6e-4)
    steps = 25
    outs, logs = _run_ranks(cfg, nranks, steps, tmp_path, jitter=0.002, seed=5, fixed_iterations=fixed)
    ref = H.build_oracle(cfg, jitter=0.002, seed=5, fixed_iterations=fixed)
    ref.prepare()
    ref.step(steps)
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    v_ref = H.by_id(ids, ref.field("particle_velocities").copy())
    rho_ref = H.by_id(ids, ref.field("particle_densities").copy())
    _, geo, _b = H.scene_particles(cfg)
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids), "every particle owned by exactly one rank"
    x, v, rho = np.empty_like(x_ref), np.empty_like(v_ref), np.empty_like(rho_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]; v[o["ids"]] = o["vel"]; rho[o["ids"]] = o["rho"]
        assert int(o["n_ghost"]) > 0
    d = H.drift(x, x_ref, geo.dh)
    it = [(int(o["iter_density"]), int(o["iter_divergence"])) for o in outs]
    print("dfsph slab x%d fixed=%d: drift max %.3e; iterations per rank %s, oracle (%d, %d)" %
          (nranks, fixed, d.max(), it, int(ref.scalar("last_iter_den")), int(ref.scalar("last_iter_div"))))
    assert len(set(it)) == 1, "every rank sees the same all-reduced residual"
    if fixed:
        assert d.max() <= 1e-5
        np.testing.assert_allclose(rho, rho_ref, rtol=3e-5)
        np.testing.assert_allclose(v, v_ref, rtol=0, atol=3e-5 * float(np.abs(v_ref).max()))
        _pairs_agree(sum(int(o["pairs"]) for o in outs), ref.last_pairs)
    else:
        assert abs(it[0][0] - int(ref.scalar("last_iter_den"))) <= 1 and abs(it[0][1] - int(ref.scalar("last_iter_div"))) <= 1
        assert d.max() <= 1e-4


def test_slab_cuts_follow_the_fluid(gpu, tmp_path):
    """Rebalancing (cuts from a per-z-layer histogram): a block that flies along +z leaves the lower slabs
    empty unless the cuts follow it.  With re-planning every 4 steps (one layer per event) the result is still the
    undecomposed oracle's, every particle has exactly one owner, and the cuts have moved with the fluid."""
    cfg = H.dam_break_scene(domain_end=(0.6, 0.6, 2.4), start=(0.1, 0.1, 0.1), end=(0.3, 0.3, 0.9), translation=(0, 0, 0),
                            velocity=(0.0, 0.0, 8.0), particleSpacing=0.019, gravitation=[0.0, 0.0, 0.0])
    steps, nranks = 100, 3
    outs, logs = _run_ranks(cfg, nranks, steps, tmp_path, jitter=0.002, seed=7, rebalance=4)
    ref = H.build_oracle(cfg, jitter=0.002, seed=7)
    ref.prepare()
    ref.step(steps)
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    _, geo, _b = H.scene_particles(cfg)
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids)
    x = np.empty_like(x_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]
    d = H.drift(x, x_ref, geo.dh)
    cuts0 = [int(v) for v in outs[0]["cuts"]]
    cuts1 = [int(outs[0]["z_lo"])] + [int(o["z_hi"]) for o in outs]
    owned = [len(o["ids"]) for o in outs]
    print("rebalance: cuts %s -> %s, owned %s, drift %.2e" % (cuts0, cuts1, owned, d.max()))
    assert d.max() <= 1e-5
    _pairs_agree(sum(int(o["pairs"]) for o in outs), ref.last_pairs)
    assert all(cuts1[k + 1] == int(outs[k + 1]["z_lo"]) for k in range(nranks - 1)), "neighbours agree on their common face"
    assert cuts1[1] > cuts0[1] and cuts1[2] > cuts0[2], "the fluid moved up by 8 layers, the cuts followed"
    assert max(owned) <= 1.6 * min(owned), "still balanced"


def test_a_cut_that_moves_hands_over_a_layer_larger_than_the_async_margin(gpu, tmp_path):
    """after a rebalance moved a cut, the gaining rank receives a whole cell layer in ONE step message.  With fewer
    than 16 layers per rank that is more than the margin of an asynchronous launch bound (max(16384, n / 16)), SLAB_ST_BOUND was raised
    and the run died at the next settle -- the only rebalance test had 5 k particles and stayed under the floor.  Here a layer holds
    ~19 k particles (> 16384 and > n / 16 = 8.3 k at 7 layers per rank), the steps go to the device in ONE advance() call, and the cuts
    move: the step right after a cut moved runs with exact launches (sph_comm_api.hpp slab_neighbor_search)."""
    cfg = H.dam_break_scene(domain_end=(2.2, 2.1, 1.4), start=(0.1, 0.1, 0.1), end=(2.08, 1.98, 0.66), translation=(0, 0, 0),
                            velocity=(0.0, 0.0, 8.0), particleSpacing=0.02, gravitation=[0.0, 0.0, 0.0])
    steps, nranks = 40, 2
    outs, logs = _run_ranks(cfg, nranks, steps, tmp_path, jitter=0.002, seed=9, rebalance=4, advance=True)
    ref = H.build_oracle(cfg, jitter=0.002, seed=9)
    ref.prepare()
    ref.step(steps)
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    _, geo, _b = H.scene_particles(cfg)
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids)
    x = np.empty_like(x_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]
    d = H.drift(x, x_ref, geo.dh)
    cuts0 = [int(v) for v in outs[0]["cuts"]]
    cuts1 = [int(outs[0]["z_lo"])] + [int(o["z_hi"]) for o in outs]
    nz = int(geo.grid_num[2])
    layer = np.bincount(np.clip((x_ref[:, 2] / geo.dh).astype(int), 0, nz - 1), minlength=nz).max()
    print("big-layer rebalance: n %d, fullest layer %d, cuts %s -> %s, drift %.2e" % (len(ids), layer, cuts0, cuts1, d.max()))
    assert layer > max(16384, len(ids) // nranks // 16)
    assert cuts1[1] > cuts0[1], "the fluid moved up, the cut followed"
    assert d.max() <= 1e-5
    _pairs_agree(sum(int(o["pairs"]) for o in outs), ref.last_pairs)


@pytest.mark.parametrize("method", ["wcsph", "dfsph"])
def test_late_entry_under_slab_sharding(gpu, tmp_path, method):
    """a block with a late entryTime enters a sharded run (base_container.py:218-221).  Every rank
    appends the part of the block inside its slab, ids are global insertion indices, DFSPH's residual means keep dividing
    by the whole scene's particle count."""
    dt = 6e-4 if method == "dfsph" else 4e-4
    cfg = H.dam_break_scene(method=method, domain_end=(0.6, 0.8, 1.2), start=(0.1, 0.1, 0.1), end=(0.3, 0.26, 1.06),
                            translation=(0, 0, 0), velocity=(0.0, -0.5, 0.5), particleSpacing=0.019, dt=dt)
    cfg["FluidBlocks"].append({"objectId": 1, "start": [0.0, 0.0, 0.0], "end": [0.13, 0.09, 0.75], "translation": [0.12, 0.28, 0.21],
                               "scale": [1, 1, 1], "velocity": [0.0, -1.5, 0.0], "density": 1000.0, "color": [1, 2, 3],
                               "entryTime": 3.5 * dt})
    steps, fixed = 12, (3 if method == "dfsph" else 0)
    outs, logs = _run_ranks(cfg, 2, steps, tmp_path, fixed_iterations=fixed)
    ref = H.build_oracle(cfg, fixed_iterations=fixed)
    ref.prepare()
    n0 = ref.particle_num
    H.oracle_step(ref, steps)
    assert ref.particle_num > n0, "the late block is in"
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    rho_ref = H.by_id(ids, ref.field("particle_densities").copy())
    _, geo, _b = H.scene_particles(cfg)
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids)
    x, rho = np.empty_like(x_ref), np.empty_like(rho_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]; rho[o["ids"]] = o["rho"]
        assert (o["ids"] >= n0).any(), "both slabs got a share of the late block"
    d = H.drift(x, x_ref, geo.dh)
    print("late entry under slab (%s): n %d -> %d, drift %.2e" % (method, n0, ref.particle_num, d.max()))
    assert d.max() <= 1e-5
    np.testing.assert_allclose(rho, rho_ref, rtol=3e-5)
    _pairs_agree(sum(int(o["pairs"]) for o in outs), ref.last_pairs)


def test_emitter_under_slab_sharding(gpu, tmp_path):
    """The emitter hack (gravitationUpper, base_solver.py:18-23, :660-677) under sharding: frozen "rigid" fluid above the
    threshold is released step by step on whichever rank owns it; ghosts carry the material they have on their owner."""
    cfg = H.dam_break_scene(domain_end=(0.6, 0.8, 1.2), start=(0.1, 0.2, 0.1), end=(0.26, 0.5, 1.06), translation=(0, 0, 0),
                            velocity=(0.0, -2.5, 0.3), particleSpacing=0.019, gravitationUpper=0.34)
    steps = 40
    outs, logs = _run_ranks(cfg, 2, steps, tmp_path)
    ref = H.build_oracle(cfg)
    ref.prepare()
    ref.step(steps)
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    _, geo, _b = H.scene_particles(cfg)
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids)
    x = np.empty_like(x_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]
    d = H.drift(x, x_ref, geo.dh)
    released = int((ref.field("particle_materials") == 1).sum())
    print("emitter under slab: %d of %d particles fluid after %d steps, drift %.2e" % (released, len(ids), steps, d.max()))
    assert d.max() <= 1e-5 and 0 < released < len(ids)
    _pairs_agree(sum(int(o["pairs"]) for o in outs), ref.last_pairs)


_CUBE_OBJ = "v -0.05 -0.05 -0.05\nv 0.05 -0.05 -0.05\nv 0.05 0.05 -0.05\nv -0.05 0.05 -0.05\nv -0.05 -0.05 0.05\nv 0.05 -0.05 0.05\nv 0.05 0.05 0.05\nv -0.05 0.05 0.05\n" \
            "f 1 3 2\nf 1 4 3\nf 5 6 7\nf 5 7 8\nf 1 2 6\nf 1 6 5\nf 2 3 7\nf 2 7 6\nf 3 4 8\nf 3 8 7\nf 4 1 5\nf 4 5 8\n"


def test_dynamic_rigid_body_under_slab_sharding(gpu, tmp_path):
    """SURVEY 8e "rigid coupling under sharding": a dynamic body that straddles the slab face and drifts across it while it
    falls into the fluid.  Its particles take their rest positions along when they change owner (64-byte records), every
    rank sums the wrench of its own fluid particles and sph_get_rigid_wrench all-reduces it, every rank's host rigid solver
    integrates the same body with the same numbers.  Reference: a single-GPU run of the same product (the oracle has no
    rigid integrator; wrench and pose are pinned to the reference by the rigid_* fixtures)."""
    (tmp_path / "cube.obj").write_text(_CUBE_OBJ)
    cfg = H.dam_break_scene(domain_end=(0.6, 0.8, 0.64), end=(0.3, 0.16, 0.4), translation=(0.12, 0.06, 0.12), dt=4e-4, viscosity_b=0.5)
    cfg["RigidBodies"] = [{"objectId": 1, "geometryFile": str(tmp_path / "cube.obj"), "isDynamic": True, "entryTime": -1.0,
                           "density": 600.0, "color": [200, 50, 50], "velocity": [0.0, -1.0, 0.9], "translation": [0.27, 0.27, 0.30],
                           "scale": [1, 1, 1], "rotationAngle": 20.0, "rotationAxis": [0, 1, 0]}]
    steps = 150
    outs, logs = _run_ranks(cfg, 2, steps, tmp_path)
    container, solver = H.build_product(cfg)
    solver.prepare()
    for _ in range(steps):
        solver.step()
    e = container.engine
    ids = e.download(L.F_PARTICLE_ID)
    x_ref = H.by_id(ids, e.download(L.F_POSITION))
    mat = H.by_id(ids, e.download(L.F_MATERIAL))
    body = solver.rigid_solver.bodies[1]
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids), "every particle owned by exactly one rank"
    x = np.empty_like(x_ref)
    owner = np.empty(len(ids), np.int32)
    for r, o in enumerate(outs):
        x[o["ids"]] = o["pos"]; owner[o["ids"]] = r
    rigid = mat == 2
    d = H.drift(x, x_ref, container.dh)
    # the body started with its centre 1.5 cells below the cut and moved ~5 cm in z: its particles sit on both ranks
    print("dynamic rigid under slab: drift fluid %.3e rigid %.3e, rigid particles per rank %s, body com %s" % (
        d[~rigid].max(), d[rigid].max(), np.bincount(owner[rigid], minlength=2), body.com))
    assert np.bincount(owner[rigid], minlength=2).min() > 0, "the body straddles the face"
    assert body.com[1] < 0.27 - 0.03, "it fell"
    assert d[rigid].max() <= 1e-5 and d[~rigid].max() <= 1e-4


def test_dead_neighbour_is_an_error_not_a_hang(gpu, tmp_path):
    """A rank that disappears must not leave its neighbour waiting for ever -- neither in a kernel (the device-side waits of
    the push transport are bounded and raise SLAB_ST_TIMEOUT) nor on the host (bounded stream waits / mailbox waits): the
    survivor's call returns an error within the time-out.  Plain library use, no launcher that could kill it."""
    import time
    cfg = H.dam_break_scene(domain_end=(1.0, 1.0, 1.2), start=(0.1, 0.1, 0.08), end=(0.3, 0.3, 1.12), translation=(0, 0, 0))
    scene_path = tmp_path / "scene.json"
    scene_path.write_text(json.dumps(cfg))
    uid = os.urandom(128).hex()
    env = dict(os.environ, SPH_COMM_TRANSPORT=TRANSPORT[0], SPH_COMM_TIMEOUT_S="6", SPH_WORKER_DIE_RANK="1", SPH_WORKER_ADVANCE="1")
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "slab_worker.py"), str(r), "2", uid, str(scene_path), "5",
                               str(tmp_path / f"rank{r}.npz")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=200)[0].decode() for p in procs]
    assert procs[1].returncode == 3
    assert procs[0].returncode not in (0, None), logs[0][-2000:]
    assert "SphError" in logs[0] and ("did not arrive in time" in logs[0] or "timed out" in logs[0] or "no answer" in logs[0]), logs[0][-2000:]
    assert time.time() - t0 < 150


def test_push_transport_is_all_ranks_or_none_under_the_hook_library(gpu, tmp_path, transport):
    """The push data plane is used by every rank or by none: a rank that cannot set it up (test-hook library; on a real node: no peer mapping, no
    coherent memory, a failed self-test) takes all ranks to the control plane's own transport at set-up, and the run is still right."""
    cfg = H.dam_break_scene(domain_end=(1.0, 1.0, 1.2), start=(0.1, 0.1, 0.08), end=(0.3, 0.3, 1.12), translation=(0, 0, 0),
                            velocity=(0.0, -0.3, 2.0), particleSpacing=0.019)
    steps = 12
    outs, logs = _run_ranks(cfg, 3, steps, tmp_path, advance=True, extra_env={"SPH_COMM_TRANSPORT": "shm+auto", "SPH_COMM_TEST_FAIL_PUSH_RANK": "1",
                                                                           "SPH_HIP_LIB": HOOKS_LIB})
    assert [str(o["transport"]) for o in outs] == ["shm", "shm", "shm"], [str(o["transport"]) for o in outs]
    assert any("push transport not available" in l for l in logs)
    ref = H.build_oracle(cfg)
    ref.prepare()
    ref.step(steps)
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    x = np.empty_like(x_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]
    _, geo, _b = H.scene_particles(cfg)
    assert H.drift(x, x_ref, geo.dh).max() <= 1e-5
    # and without the hook the same command line comes up with the push transport -- unless the mailboxes are asked for by name
    request, want = ("shm+auto", "ipc-push+shm") if transport == "shm+ipc" else ("shm", "shm")
    outs2, _ = _run_ranks(cfg, 2, 3, tmp_path, extra_env={"SPH_COMM_TRANSPORT": request})
    assert [str(o["transport"]) for o in outs2] == [want] * 2


def test_exact_launch_flavour_of_the_push_transport(gpu, tmp_path, transport):
    """SPH_SLAB_ASYNC=0: WCSPH steps over the push transport with the counts read back once per step and exact launch grids (what the
    iterative solvers always use) -- same particles, same pairs as the asynchronous flavour.  The mailbox transport always runs exact
    launches: there the switch must change nothing at all."""
    cfg = H.dam_break_scene(domain_end=(1.0, 1.0, 1.2), start=(0.1, 0.1, 0.08), end=(0.3, 0.3, 1.12), translation=(0, 0, 0),
                            velocity=(0.0, -0.3, 2.0), particleSpacing=0.019)
    (tmp_path / "a").mkdir(); (tmp_path / "s").mkdir()
    outs_a, _ = _run_ranks(cfg, 2, 15, tmp_path / "a", advance=True)
    outs_s, _ = _run_ranks(cfg, 2, 15, tmp_path / "s", advance=True, extra_env={"SPH_SLAB_ASYNC": "0", "SPH_COMM_TRANSPORT": transport})
    for a, b in zip(outs_a, outs_s):
        assert str(b["transport"]) == ("ipc-push+shm" if transport == "shm+ipc" else "shm")
        oa, ob = np.argsort(a["ids"]), np.argsort(b["ids"])
        np.testing.assert_array_equal(a["ids"][oa], b["ids"][ob])
        np.testing.assert_array_equal(a["pos"][oa], b["pos"][ob])     # the same kernels in the same order: bit-identical
        assert int(a["pairs"]) == int(b["pairs"])


HOOKS_LIB = os.path.join(ROOT, "sph_project_amd", "libsph_hip_testhooks.so")


def _owned_state(outs):
    ids = np.concatenate([o["ids"] for o in outs])
    order = np.argsort(ids, kind="stable")
    return ids[order], np.concatenate([o["pos"] for o in outs])[order], np.concatenate([o["rho"] for o in outs])[order]


def test_stalled_consumer_exposes_the_single_header_race_and_only_that(gpu, tmp_path, transport):
    """The mechanism of round 5's halo race, reproduced on demand (model: tests/test_halo_protocol_model.py).  The test-hook library
    (libsph_hip_testhooks.so, -DSPH_TEST_HOOKS: the production library has neither switch) stalls rank 1's k_halo_unpack2 between its own
    announce and its poll for 0.3 s -- what time slicing of eight ranks on one GPU did at random.  Between sph_prepare's step message
    and the first step's there is no field message, so rank 0 runs ahead and announces message 2 while rank 1 still has to read message
    1's header:
      * header per message parity (the protocol in the tree): nothing changes -- bit-identical to the run without the stall, equal to
        the oracle;
      * SPH_TEST_SINGLE_HEADER (pre-round-5): rank 1 takes message 2's record count for message 1's payload -- the run fails or
        ends in a different particle set.  If it ever passes, the stall no longer reaches the seam and this test says so.
    The mailbox transport has no shared header (every message carries its own count): there the stall and the single-header switch
    change nothing."""
    assert os.path.exists(HOOKS_LIB), "build() makes libsph_hip_testhooks.so"
    # The two messages of the seam must DIFFER for the mix-up to show (same positions -> same records -> same count, and a header taken
    # from the wrong message is then harmless).  They differ when particles change owner in prepare's exchange: the lattice (spacing 0.02
    # from z = 0.08) has a particle layer exactly ON every cell face, the seeded jitter puts half of the layer on the slab cut below the
    # cut: ~110 migrants in message 1, which come back as ordinary boundary copies in message 2.  (C4 with jitter has 12.5 k of them per
    # face -- the 12.5 k garbage records / 2.5 k lost arrivals of profiles/r05_halo_header_race_ab.txt: a fifth of a 62.5 k message's tail.)
    cfg = H.dam_break_scene(domain_end=(1.0, 1.0, 1.2), start=(0.1, 0.1, 0.08), end=(0.4, 0.4, 1.12), translation=(0, 0, 0),
                            velocity=(0.0, -0.3, 2.5))
    steps = 6
    hooks = {"SPH_HIP_LIB": HOOKS_LIB}
    stall = dict(hooks, SPH_TEST_HALO_DELAY_US="300000", SPH_WORKER_DELAY_RANK="1")
    plain, _ = _run_ranks(cfg, 2, steps, tmp_path / "plain", jitter=0.002, seed=3, advance=True, extra_env=hooks)
    good, _ = _run_ranks(cfg, 2, steps, tmp_path / "good", jitter=0.002, seed=3, advance=True, extra_env=stall)
    a, b = _owned_state(plain), _owned_state(good)
    # the stall changes nothing under the two-header protocol.  (Not bit for bit: the order of the records inside a message is the
    # order in which the sender's waves took their slots, the arrivals' order in their cells follows it, and with it the order of a
    # few pair sums -- two sharded runs differ in the last bit of a few positions whenever the timing differs.)
    np.testing.assert_array_equal(a[0], b[0])
    _, geo, _b = H.scene_particles(cfg)
    assert H.drift(b[1], a[1], geo.dh).max() <= 1e-6
    ref = H.build_oracle(cfg, jitter=0.002, seed=3)
    ref.prepare()
    ref.step(steps)
    ids = H.oracle_ids(ref)
    assert np.array_equal(b[0], np.arange(len(ids)))
    assert H.drift(b[1], H.by_id(ids, ref.field("particle_positions").copy()), geo.dh).max() <= 1e-5
    if transport != "shm+ipc":
        bad, _ = _run_ranks(cfg, 2, steps, tmp_path / "bad", jitter=0.002, seed=3, advance=True, extra_env=dict(stall, SPH_TEST_SINGLE_HEADER="1"))
        c = _owned_state(bad)
        np.testing.assert_array_equal(c[0], a[0])
        assert H.drift(c[1], a[1], geo.dh).max() <= 1e-6
        return
    fired = False
    try:
        bad, _ = _run_ranks(cfg, 2, steps, tmp_path / "bad", jitter=0.002, seed=3, advance=True, extra_env=dict(stall, SPH_TEST_SINGLE_HEADER="1"))
        c = _owned_state(bad)
        same_set = len(c[0]) == len(a[0]) and np.array_equal(c[0], a[0])
        fired = not (same_set and H.drift(c[1], a[1], geo.dh).max() <= 1e-5)
        what = "owned particles %d (expected %d), same id set: %s" % (len(c[0]), len(a[0]), same_set)
    except AssertionError as e:      # a rank reported the damage itself (capacity, peer status, non-finite state)
        fired, what = True, "a rank failed: " + str(e)[-300:].replace("\n", " ")
    print("single header + stalled consumer:", what)
    assert fired, "the stall did not expose the single-header race: does it still reach the prepare -> first-step seam?"


def test_stalled_consumers_everywhere_change_nothing(gpu, tmp_path, transport):
    """Stress of the rest of the protocol (header-less field messages under presend + fused field send, SlabDyn / halo_counts banks): every
    waiting workgroup of every rank stalls 0.1-0.4 ms before it polls -- workgroup 0 between its announce and its poll, the others
    staggered -- in three ranks over 12 asynchronous steps.  Same particles, same state (to the last bit or two) as without stalls.  (Over
    the mailbox transport nothing waits on the device: the same comparison holds trivially and guards the hooks' reach.)"""
    cfg = H.dam_break_scene(domain_end=(1.0, 1.0, 1.2), start=(0.1, 0.1, 0.08), end=(0.4, 0.4, 1.12), translation=(0, 0, 0),
                            velocity=(0.0, -0.3, 2.5), particleSpacing=0.019)
    hooks = {"SPH_HIP_LIB": HOOKS_LIB}
    plain, _ = _run_ranks(cfg, 3, 12, tmp_path / "plain", jitter=0.002, seed=5, advance=True, extra_env=hooks)
    slow, _ = _run_ranks(cfg, 3, 12, tmp_path / "slow", jitter=0.002, seed=5, advance=True,
                         extra_env=dict(hooks, SPH_TEST_HALO_DELAY_US="400", SPH_WORKER_DELAY_RANK="all"))
    a, b = _owned_state(plain), _owned_state(slow)
    np.testing.assert_array_equal(a[0], b[0])
    _, geo, _b = H.scene_particles(cfg)
    assert H.drift(b[1], a[1], geo.dh).max() <= 1e-6      # (not bit for bit: see the test above)
    np.testing.assert_allclose(b[2], a[2], rtol=2e-6)


def _eight_way(cfg, steps, tmp_path, jitter, seed, exact_pairs, build="strict"):
    """8 ranks on this box's single GPU (two per worker process, see MAX_PROCS), all `steps` in ONE advance() call, against the undecomposed
    CPU oracle, over the transport of the running test (the push transport is the production data plane).
    build = "fast": the kernels `bench.py --gpus N` runs (v_rcp / v_rsq, FMA, the presend / fused-field-send force and density passes of
    the fast object) -- the sharded path that is TIMED is the one compared with the oracle."""
    nranks = 8
    env = {"SPH_COMM_TIMEOUT_S": "120", "SPH_FAST": "1" if build == "fast" else "0"}
    if build == "stalled":   # strict kernels of the test-hook library, every waiting workgroup of every rank stalled 50-200 us before its poll
        env.update(SPH_HIP_LIB=HOOKS_LIB, SPH_TEST_HALO_DELAY_US="200", SPH_WORKER_DELAY_RANK="all")
    outs, logs = _run_ranks(cfg, nranks, steps, tmp_path, jitter=jitter, seed=seed, advance=True, timeout=600, extra_env=env)
    ref = H.build_oracle(cfg, jitter=jitter, seed=seed)
    ref.prepare()
    ref.step(steps)
    ids = H.oracle_ids(ref)
    x_ref = H.by_id(ids, ref.field("particle_positions").copy())
    rho_ref = H.by_id(ids, ref.field("particle_densities").copy())
    _, geo, _b = H.scene_particles(cfg)
    dh, nz = geo.dh, int(geo.grid_num[2])
    all_ids = np.concatenate([o["ids"] for o in outs])
    if not (len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids)):   # say which rank holds what before failing
        for r, o in enumerate(outs):
            u, cnt = np.unique(o["ids"], return_counts=True)
            print("rank %d: %d owned, %d distinct ids, most repeated id %d x%d, ids == 0: %d, non-finite positions %d" % (
                r, len(o["ids"]), len(u), int(u[cnt.argmax()]), int(cnt.max()), int((o["ids"] == 0).sum()), int((~np.isfinite(o["pos"])).any(1).sum())))
    assert len(all_ids) == len(ids) and len(np.unique(all_ids)) == len(ids), "every particle owned by exactly one rank"
    x, rho = np.empty_like(x_ref), np.empty_like(rho_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]; rho[o["ids"]] = o["rho"]
    ghosts = [int(o["n_ghost"]) for o in outs]
    assert min(ghosts) > 0, ghosts            # two edge ranks (one neighbour) and six interior ones (two)
    assert min(ghosts[1:-1]) > max(ghosts[0], ghosts[-1]) * 1.2, ghosts
    d = H.drift(x, x_ref, dh)
    cuts = [int(v) for v in outs[0]["cuts"]]
    from sph_project_amd import slab
    x0 = np.concatenate([b["pos"] for b in _b])
    if jitter > 0:
        x0 = H.perturb(x0, jitter, seed)
    moved = int((slab.owner_of(slab.cell_layer(x0[:, 2], dh, nz), cuts) != slab.owner_of(slab.cell_layer(x[:, 2], dh, nz), cuts)).sum())
    got, want = sum(int(o["pairs"]) for o in outs), int(ref.last_pairs)
    print("8 ranks on one GPU: n %d, cuts %s (layers per rank %s), owned %s, ghosts %s, changed owner %d, drift max %.3e, pairs %d vs oracle %d" % (
        len(ids), cuts, list(np.diff(cuts)), [len(o["ids"]) for o in outs], ghosts, moved, d.max(), got, want))
    assert d.max() <= 1e-5                     # (north star 1e-4; measured 0 on the rest lattice, 7e-8 in motion)
    np.testing.assert_allclose(rho, rho_ref, rtol=2e-5)
    if exact_pairs:
        assert got == want, (got, want)
    else:
        _pairs_agree(got, want)
    return moved


@pytest.mark.parametrize("build", ["strict", "fast"])
@pytest.mark.parametrize("variant", ["as_written", "jitter_vz"])
def test_c4_sharded_over_8_ranks_matches_oracle(gpu, tmp_path, transport, variant, build):
    """BASELINE configs[3] in its own mode as far as one GPU allows: the 4,000,000-particle dam break z-slab sharded over EIGHT ranks
    (0.5 M particles, 10-12 cell layers each) over the push transport, 5 asynchronous steps, against the undecomposed oracle.
    as_written: the scene of SURVEY 8d C4 (rest lattice, v = (0, -0.5, 0): nobody crosses a z face in 5 steps).  jitter_vz: the same
    block on a seeded perturbed lattice with a z velocity, so that particles migrate across all seven faces."""
    from sph_project_amd import product as P
    cfg = P.c4_scene()
    if variant == "as_written":
        _eight_way(cfg, 5, tmp_path, 0.0, 0, exact_pairs=build == "strict", build=build)
    else:
        cfg["FluidBlocks"][0]["velocity"] = [0.0, -0.5, 1.5]
        moved = _eight_way(cfg, 5, tmp_path, 0.002, 11, exact_pairs=build == "strict", build=build)
        assert moved >= 1000, moved


@pytest.mark.parametrize("build", ["strict", "fast", "stalled"])
def test_c2_scene_sharded_over_8_ranks_matches_oracle(gpu, tmp_path, transport, build):
    """The 1.23 M scene of configs[1] split eight ways: five cell layers of ~31 k particles per rank -- the thin-slab regime (one staged
    stretch per x-offset group, sph_device.hpp nbr_plan "chain") where a whole layer is a fifth of a rank.  Perturbed lattice + z velocity:
    migration across every face, 5 asynchronous steps."""
    from sph_project_amd import product as P
    cfg = P.c2_scene()
    cfg["FluidBlocks"][0]["velocity"] = [0.0, -0.5, 1.5]
    moved = _eight_way(cfg, 5, tmp_path, 0.002, 12, exact_pairs=build != "fast", build=build)
    assert moved >= 500, moved


@pytest.mark.parametrize("build", ["fast"])
def test_c2_in_motion_state_sharded_over_8_ranks_matches_oracle(gpu, tmp_path, transport, build, from_step=2500):
    """What `bench.py --gpus 8` runs through on its way to `in_motion`, checked: the 1.23 M scene in the state of step 2500 (collapsed column,
    39 neighbours per particle, pile-ups along the floor and the z walls that every slab face cuts through) split over eight ranks.  The
    undecomposed product produces the state, the ranks are seeded with it (tests/slab_worker.py SPH_WORKER_STATE: slab membership and cuts
    from these positions), so is the oracle (H.oracle_from_state); 5 asynchronous steps over the push transport; by particle id against
    the oracle."""
    from sph_project_amd import product as P
    cfg = P.c2_scene()
    container, solver = H.build_product(cfg, fast_math=1)
    solver.prepare()
    solver.advance(from_step)
    e = container.engine
    x0, v0 = e.download(L.F_POSITION), e.download(L.F_VELOCITY)
    n = len(x0)
    e.close()
    tmp_path.mkdir(parents=True, exist_ok=True)
    np.savez(tmp_path / "state.npz", x=x0, v=v0)
    steps = 5
    env = {"SPH_COMM_TIMEOUT_S": "120", "SPH_FAST": "1" if build == "fast" else "0", "SPH_WORKER_STATE": str(tmp_path / "state.npz")}
    outs, logs = _run_ranks(cfg, 8, steps, tmp_path, advance=True, timeout=600, extra_env=env)
    ref = H.oracle_from_state(cfg, x0, v0, np.arange(n, dtype=np.int32))
    ref.prepare()
    ref.step(steps)
    oid = H.oracle_ids(ref)
    x_ref, rho_ref = H.by_id(oid, ref.field("particle_positions").copy()), H.by_id(oid, ref.field("particle_densities").copy())
    all_ids = np.concatenate([o["ids"] for o in outs])
    assert len(all_ids) == n and len(np.unique(all_ids)) == n, "every particle owned by exactly one rank"
    x, rho = np.empty_like(x_ref), np.empty_like(rho_ref)
    for o in outs:
        x[o["ids"]] = o["pos"]; rho[o["ids"]] = o["rho"]
    _, geo, _b = H.scene_particles(cfg)
    from sph_project_amd import slab
    cuts = [int(v) for v in outs[0]["cuts"]]
    nz = int(geo.grid_num[2])
    moved = int((slab.owner_of(slab.cell_layer(x0[:, 2], geo.dh, nz), cuts) != slab.owner_of(slab.cell_layer(x[:, 2], geo.dh, nz), cuts)).sum())
    d = H.drift(x, x_ref, geo.dh)
    got, want = sum(int(o["pairs"]) for o in outs), int(ref.last_pairs)
    print("8 ranks on one GPU from the state of step %d: cuts %s, owned %s, ghosts %s, changed owner %d, drift max %.3e, pairs %d vs oracle %d" % (
        from_step, cuts, [len(o["ids"]) for o in outs], [int(o["n_ghost"]) for o in outs], moved, d.max(), got, want))
    assert d.max() <= 1e-5
    np.testing.assert_allclose(rho, rho_ref, rtol=2e-5)
    _pairs_agree(got, want)
    ref.close()
