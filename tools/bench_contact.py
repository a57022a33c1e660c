"""ms/step of product.coupling_scene() (the reference's final_scene1 with cube / sphere meshes) with the native and the contact rigid
backends, alternated in one process; one JSON line per round and a summary line.  --backend X --rounds 1 times one backend only (for a
kernel trace).  The contact pass's own share comes from the HIP-event profiler (kernel id 25, rigid_contact)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import _lib as L  # noqa: E402
from sph_project_amd import product as P  # noqa: E402


def run(backend, steps, warmup):
    os.environ["SPH_RIGID_BACKEND"] = backend
    os.environ["SPH_RIGID_NATIVE_OK"] = "1"
    container, solver = P.build_product(P.coupling_scene())
    solver.prepare()
    e = container.engine
    for _ in range(warmup):
        solver.step()
    e.synchronize()
    e.profile_enable(L.K_RIGID_CONTACT, True); e.profile_reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        solver.step()
    e.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    launches, kms = e.profile_read(L.K_RIGID_CONTACT)
    out = dict(backend=backend, particles=e.particle_num, steps=steps, ms_per_step=round(ms, 4),
               contact_pass_us_per_step=round(1e3 * kms / steps, 2) if launches else 0.0,
               contact_pairs_last=e.get_rigid_contact_pairs() if backend == "contact" else 0)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--backend", default=None, choices=["native", "contact"])
    a = ap.parse_args()
    order = [a.backend] if a.backend else ["native", "contact"]
    res = {b: [] for b in order}
    for _ in range(a.rounds):
        for b in order:
            r = run(b, a.steps, a.warmup)
            res[b].append(r)
            print(json.dumps(r), flush=True)
    print(json.dumps({"summary": {b: min(r["ms_per_step"] for r in rs) for b, rs in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
