"""Child process of tests/test_sort_carry.py: `sort_carry_probe.py OUT.npz CASE [CASE ...]` runs the named cases with whatever library and
switches its environment selects (SPH_NO_SORT_CARRY, SPH_HIP_LIB, SPH_TEST_DROP_CARRY) and saves, per case, the state after every call
-- position, velocity, density, particle id and the three parts of the meta word (material, object id, is_dynamic), all in sorted order
-- and the number of sorts whose velocities, meta words and ids the density pass moved (SphStats::carried_sorts) and of list sorts."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sph_project_amd import _lib as L  # noqa: E402
from sph_project_amd import product as P  # noqa: E402
from tests import helpers as H  # noqa: E402

FIELDS = (("x", L.F_POSITION), ("v", L.F_VELOCITY), ("rho", L.F_DENSITY), ("id", L.F_PARTICLE_ID),
          ("mat", L.F_MATERIAL), ("obj", L.F_OBJECT_ID), ("dyn", L.F_IS_DYNAMIC))
MOVING = dict(velocity=(0.4, -1.5, 0.3))   # the collapsing block of test_list_sort_equals_record_sort: cells change population every step


def snap(e, names=None):
    return {k: e.download(f) for k, f in FIELDS if names is None or k in names}


def run_calls(cfg, calls, fast_math, jitter=0.003):
    container, solver = H.build_product(cfg, fast_math=fast_math, jitter=jitter, seed=11)
    solver.prepare()
    e = container.engine
    snaps = []
    for kind, n in calls:
        if kind == "async":
            e.step_async(n)
            e.synchronize()
        else:
            e.step(n)
        snaps.append(snap(e))
    return snaps, solver.stats()


def case_c1(fast_math):
    """C1, WCSPH, 300 steps: step_async(1) (its sort hashes for itself), step_async(7) (six sorts hashed by the force pass in front of
    them, NextHash) and step(1), 33 times over and three more."""
    calls = [("async", 1), ("async", 7), ("sync", 1)] * 33 + [("sync", 1)] * 3
    assert sum(n for _, n in calls) == 300
    return run_calls(P.dam_break_scene(**MOVING), calls, fast_math)


def case_small(end, want_n):
    """one fluid block of want_n particles, 20 steps"""
    cfg = P.dam_break_scene(end=(end, end, end), **MOVING)
    snaps, st = run_calls(cfg, [("sync", 1)] * 20, 1)
    assert len(snaps[0]["id"]) == want_n, len(snaps[0]["id"])
    return snaps, st


def case_method(method, steps, **scene):
    return run_calls(P.dam_break_scene(method=method, **MOVING, **scene), [("sync", 1)] * steps, 1)


def case_boundary():
    """the scene of test_static_domain_box: static boundary particles, so not all fluid"""
    cfg = P.dam_break_scene(domain_end=(0.6, 0.6, 0.6), end=(0.2, 0.2, 0.2), translation=(0.06, 0.06, 0.06), add_domain_box=True)
    snaps, st = run_calls(cfg, [("sync", 1)] * 5, 1, jitter=0.0)
    assert (snaps[0]["mat"] != 1).any()
    return snaps, st


def case_begin_end():
    """wherever the host may look: right after prepare(), and between sph_step_begin and sph_step_end"""
    container, solver = H.build_product(P.dam_break_scene(**MOVING), fast_math=1, jitter=0.003, seed=11)
    solver.prepare()
    e = container.engine
    snaps = [snap(e)]
    for _ in range(10):
        e.step_begin()
        snaps.append(snap(e))
        e.step_end()
        snaps.append(snap(e))
    return snaps, solver.stats()


def case_one_strict_step():
    """one step of C1, strict build (the test-hook library has no other): velocities and ids only"""
    container, solver = H.build_product(P.dam_break_scene(**MOVING), fast_math=0, jitter=0.003, seed=11)
    solver.prepare()
    e = container.engine
    e.step(1)
    return [snap(e, ("v", "id"))], solver.stats()


CASES = {
    "c1_fast": lambda: case_c1(1), "c1_strict": lambda: case_c1(0),
    "small216": lambda: case_small(0.11, 216), "small512": lambda: case_small(0.15, 512),
    "pcisph": lambda: case_method("pcisph", 20), "iisph": lambda: case_method("iisph", 20),
    "boundary": case_boundary, "dfsph": lambda: case_method("dfsph", 5, dt=6e-4),
    "begin_end": case_begin_end, "one_strict_step": case_one_strict_step,
}

if __name__ == "__main__":
    out = {}
    for name in sys.argv[2:]:
        snaps, st = CASES[name]()
        out[name + "/calls"] = np.int64(len(snaps))
        out[name + "/carried_sorts"] = np.int64(st["carried_sorts"])
        out[name + "/list_sorts"] = np.int64(st["list_sorts"])
        for k, s in enumerate(snaps):
            for f, a in s.items():
                out["%s/%d/%s" % (name, k, f)] = a
    np.savez(sys.argv[1], **out)
    print("sort_carry_probe: wrote", len(out), "arrays")
