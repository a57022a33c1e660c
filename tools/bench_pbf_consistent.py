"""The consistent PBF variant at the C2 geometry (the final_scene0.json block, 1,231,200 particles, dt 4e-4),
fast build, from rest and after --moved steps: ms/step (synchronous steps: the stop test reads back), iterations per step,
microseconds per iteration and per walk (pbfc_density_lambda, pbfc_delta) from sph_profile_*; next to them, measured in the same
run, a PCISPH iteration (pcisph_rho_star + pcisph_pressure_accel) in the same two states and an iteration of the reference variant
in its step 1 (pbf_density_lambda + pbf_fix_position; tools/bench_pbf.py says why only step 1), and the consistent variant once more
with pbfMinIterations = --min_iterations (under the default keys the C2 column comes apart at its impact on the floor, DESIGN.md 27:
the second row times that state).  The wall time and the per-kernel
times come from two fresh containers that run the same steps.  Kernel times are divided by the iterations that ran: launches past a
solve's stop return at their first instruction and add their few microseconds to the sum.
    python tools/bench_pbf_consistent.py [--steps 20] [--moved 1000] [--min_iterations 8] [--out profiles/pbf_consistent_bench_c2.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WALKS = {"pbf consistent": ("pbfc_density_lambda", "pbfc_delta"), "pcisph": ("pcisph_rho_star", "pcisph_pressure_accel"),
         "pbf reference": ("pbf_density_lambda", "pbf_fix_position")}


def scene(which, keys):
    from sph_project_amd import product as P
    cfg = P.c2_scene("pcisph" if which == "pcisph" else "pbf")
    if which == "pbf consistent":
        cfg["Configuration"]["pbfVariant"] = "consistent"
        cfg["Configuration"].update(keys)
    return cfg


def iterations_of(which, solver):
    if which == "pcisph":
        return solver.stats()["iter_pcisph"]
    return solver.iterations


def measure(which, steps, moved, **keys):
    """ms/step, iterations/step, us per walk of `steps` steps behind `moved` steps; keys: scene keys of the consistent variant."""
    from sph_project_amd import product as P

    def fresh():
        c, s = P.build_product(scene(which, keys), fast_math=1)
        s.prepare()
        s.advance(moved)
        c.engine.synchronize()
        return c, s

    c, s = fresh()
    t0 = time.perf_counter()
    s.advance(steps)
    c.engine.synchronize()
    wall = (time.perf_counter() - t0) / steps
    c.engine.close()
    c, s = fresh()
    eng = c.engine
    names = {eng.lib.sph_kernel_name(k).decode(): k for k in range(30)}
    eng.profile_enable(-1, True)
    eng.profile_reset()
    iters = 0
    for _ in range(steps):
        s.step()
        iters += iterations_of(which, s)
    eng.synchronize()
    ms = {k: eng.profile_read(names[k])[1] for k in WALKS[which]}
    n = int(c.particle_num[None])
    eng.close()
    label = which + "".join(f" {k} {v}" for k, v in keys.items())
    return dict(which=label, moved=moved, particles=n, ms_per_step=1e3 * wall, iterations_per_step=iters / steps,
                us_per_walk={k: 1e3 * v / max(iters, 1) for k, v in ms.items()}, us_per_iteration=1e3 * sum(ms.values()) / max(iters, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--moved", type=int, default=1000)
    ap.add_argument("--min_iterations", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pbf_consistent_bench_c2.txt"))
    args = ap.parse_args()
    rows = [measure("pbf consistent", args.steps, 0), measure("pbf consistent", args.steps, args.moved),
            measure("pbf consistent", args.steps, 0, pbfMinIterations=args.min_iterations),
            measure("pbf consistent", args.steps, args.moved, pbfMinIterations=args.min_iterations),
            measure("pcisph", args.steps, 0), measure("pcisph", args.steps, args.moved), measure("pbf reference", 1, 0)]
    lines = [f"C2 ({rows[0]['particles']} particles), fast build, {args.steps} timed steps per row (pbf reference: its step 1 only)",
             f"{'solver':<34}{'state':<20}{'ms/step':>10}{'iter/step':>11}{'us/iter':>10}  us per walk"]
    for r in rows:
        state = "from rest" if r["moved"] == 0 else f"after {r['moved']} steps"
        walks = ", ".join(f"{k} {v:.1f}" for k, v in r["us_per_walk"].items())
        lines.append(f"{r['which']:<34}{state:<20}{r['ms_per_step']:>10.3f}{r['iterations_per_step']:>11.2f}{r['us_per_iteration']:>10.1f}  {walks}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
