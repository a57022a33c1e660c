"""The sort's velocity, meta and id arrays carried under the density pass (SortCarry): where the launch behind a list sort of an
all-fluid scene is a density pass over every tile (the WCSPH, PCISPH and IISPH steps), k_gather_prep leaves those three arrays behind and
the prologue of that pass moves them.  Every case runs twice in fresh child processes (tests/sort_carry_probe.py), once as built and once
with SPH_NO_SORT_CARRY=1: after every call position, velocity, density, particle id and the parts of the meta word must be array_equal,
and SphStats::carried_sorts says which path ran."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "sort_carry_probe.py")
CASES = ("c1_fast", "c1_strict", "small216", "small512", "pcisph", "iisph", "boundary", "dfsph", "begin_end")
FIELDS = ("x", "v", "rho", "id", "mat", "obj", "dyn")


def _probe(out, cases, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("SPH_NO_SORT_CARRY", "SPH_TEST_DROP_CARRY")}
    e.update(env)
    r = subprocess.run([sys.executable, PROBE, str(out)] + list(cases), env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(str(out))


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """every case once with the carry and once without: two child processes for the whole module"""
    d = tmp_path_factory.mktemp("sort_carry")
    return _probe(d / "carry.npz", CASES), _probe(d / "plain.npz", CASES, SPH_NO_SORT_CARRY="1")


def _same_state(runs, case, calls):
    a, b = runs
    assert int(a[case + "/calls"]) == int(b[case + "/calls"]) == calls
    for k in range(calls):
        for f in FIELDS:
            u, v = a["%s/%d/%s" % (case, k, f)], b["%s/%d/%s" % (case, k, f)]
            assert np.array_equal(u, v), (case, k, f, int((u != v).sum()))
    n = len(a[case + "/0/id"])
    for r in (a, b):   # the ids are still the particles' own, the meta words still fluid: nothing was left behind or moved twice
        last = "%s/%d/" % (case, calls - 1)
        assert np.array_equal(np.sort(r[last + "id"]), np.arange(n))
        assert np.isfinite(r[last + "v"]).all() and np.isfinite(r[last + "x"]).all() and np.isfinite(r[last + "rho"]).all()
    return int(a[case + "/carried_sorts"]), int(b[case + "/carried_sorts"]), int(a[case + "/list_sorts"])


@pytest.mark.parametrize("case", ["c1_fast", "c1_strict"])
def test_wcsph_c1_300_steps(runs, case):
    """C1 (8,000 particles: 31 full tiles and one of 64), a collapsing perturbed block, 300 steps as step_async(1), step_async(7) and
    step(1) calls, fast and strict builds: the same state after each of the 102 calls, and the sort of every step carried (prepare()'s
    is followed by no density pass and moves everything itself)."""
    on, off, lists = _same_state(runs, case, 102)
    assert off == 0 and on == 300 and lists >= 300, (on, off, lists)
    a = runs[0]
    moved = a[case + "/101/x"] - a[case + "/0/x"]
    assert np.abs(moved).max() > 0.02   # more than a cell: the particles did change cell


@pytest.mark.parametrize("case,n", [("small216", 216), ("small512", 512)])
def test_one_partial_tile_and_no_partial_tile(runs, case, n):
    """a block of fewer than 256 particles (a single partial tile: the lanes past n do nothing) and one of exactly 512 (no partial tile)"""
    on, off, _ = _same_state(runs, case, 20)
    assert len(runs[0][case + "/0/id"]) == n
    assert off == 0 and on == 20, (on, off)


@pytest.mark.parametrize("case", ["pcisph", "iisph"])
def test_pcisph_and_iisph_carry_too(runs, case):
    """their first walk behind the sort is DensityPass<true, false>: C1, 20 steps"""
    on, off, _ = _same_state(runs, case, 20)
    assert off == 0 and on == 20, (on, off)


@pytest.mark.parametrize("case", ["boundary", "dfsph"])
def test_the_option_does_not_leak(runs, case):
    """a scene with boundary particles (not all fluid) and a DFSPH scene (its first walk reads the candidates' velocities): nothing is
    carried, and the state is that of the run with the option switched off"""
    on, off, lists = _same_state(runs, case, 5)
    assert on == 0 and off == 0 and lists >= 5, (on, off, lists)


def test_host_sees_the_sorted_arrays_whole(runs):
    """velocities, ids and meta words downloaded right after prepare() and between sph_step_begin and sph_step_end, 10 steps: whole in
    both runs (checked for every snapshot, not only the last)"""
    on, off, _ = _same_state(runs, "begin_end", 21)
    assert off == 0 and on == 10, (on, off)
    a = runs[0]
    n = len(a["begin_end/0/id"])
    for k in range(21):
        assert np.array_equal(np.sort(a["begin_end/%d/id" % k]), np.arange(n)), k
        assert np.isfinite(a["begin_end/%d/v" % k]).all() and (a["begin_end/%d/mat" % k] == 1).all(), k


def test_a_broken_promise_is_poisoned_in_the_hooks_build(gpu, tmp_path):
    """The test-hook library fills the velocities, meta words and ids that the gather left behind with 0xFF bytes (l_scatter_impl).  One
    strict-build step of C1 in child processes: as built the density pass moves them (the state of the production library's step); with
    SPH_TEST_DROP_CARRY=1 (hook library only) that pass is launched without its carry, as a step would that made the promise and did not
    keep it, and ends with NaN velocities and ids of -1."""
    hooks = os.path.join(ROOT, "sph_project_amd", "libsph_hip_testhooks.so")
    prod = _probe(tmp_path / "prod.npz", ["one_strict_step"])
    kept = _probe(tmp_path / "kept.npz", ["one_strict_step"], SPH_HIP_LIB=hooks)
    broken = _probe(tmp_path / "broken.npz", ["one_strict_step"], SPH_HIP_LIB=hooks, SPH_TEST_DROP_CARRY="1")
    assert int(prod["one_strict_step/carried_sorts"]) == 1 and int(kept["one_strict_step/carried_sorts"]) == 1
    assert int(broken["one_strict_step/carried_sorts"]) == 0
    for f in ("v", "id"):
        assert np.array_equal(prod["one_strict_step/0/" + f], kept["one_strict_step/0/" + f]), f
    assert np.isnan(broken["one_strict_step/0/v"]).all()
    assert (broken["one_strict_step/0/id"] == -1).all()
