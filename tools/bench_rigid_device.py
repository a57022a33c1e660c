"""ms/step of product.coupling_scene() (the reference's final_scene1 with cube / sphere meshes; DFSPH, strict build) with the native and
the device rigid backends, alternated in one process, under tools/bench_contact.py's protocol: `warmup` steps, then `steps` timed steps
(10 and 60: steps 10-70), a fresh scene per measurement.  The steps go through solver.advance(), the driver's path: n round trips
through the host with the native backend, one device call with the device backend.  Per measurement one JSON line with
  ms_per_step        wall clock around advance(steps) + synchronize
  event_ms_per_step  the same steps once more with the HIP-event profiler on every kernel id: the sum of the launches' own times
  integrate_us_per_step  the device backend's launch (kernel id 26) from that second pass
and a summary line (minimum and spread over the rounds).  --backend X --rounds 1 times one backend only (for a kernel trace)."""
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
    solver.advance(warmup)
    e.synchronize()
    t0 = time.perf_counter()
    solver.advance(steps)
    e.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    e.profile_enable(-1, True); e.profile_reset()
    solver.advance(steps)
    e.synchronize()
    per_kernel = {}
    for k in range(64):
        name = e.lib.sph_kernel_name(k).decode()
        if name == "?":
            break
        launches, kms = e.profile_read(k)
        if launches:
            per_kernel[name] = kms
    out = dict(backend=backend, particles=e.particle_num, steps=steps, ms_per_step=round(ms, 4),
               event_ms_per_step=round(sum(per_kernel.values()) / steps, 4),
               integrate_us_per_step=round(1e3 * per_kernel.get("rigid_integrate", 0.0) / steps, 2))
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--backend", default=None, choices=["native", "device"])
    a = ap.parse_args()
    order = [a.backend] if a.backend else ["native", "device"]
    res = {b: [] for b in order}
    for _ in range(a.rounds):
        for b in order:
            r = run(b, a.steps, a.warmup)
            res[b].append(r["ms_per_step"])
            print(json.dumps(r), flush=True)
    print(json.dumps({"summary": {b: dict(min=min(v), max=max(v)) for b, v in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
