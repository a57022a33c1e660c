"""What the adaptive time stepping costs and what it buys, three parts:
  overhead   product.c2_scene("wcsph") in motion, both builds: one handle with the mode off against one with the mode pinned
             (cflMin = cflMax = timeStepSize: the same trajectory, so the difference is the reduce launch plus its read-back), timed
             ALTERNATING --repeats times in windows of --steps synchronous steps (sph_step(h, n): the pinned handle cannot step
             asynchronously, so neither does the other); then HIP events (sph_profile_*) around SPH_K_CFL on the pinned handle.
  buys       product.c2_scene("dfsph") (C3: its own stop tests) run to --scene-time seconds: the scene's step size against the mode with
             cflMax at --factors times it (cflFactor 0.5, cflMin = timeStepSize / 64); wall time, steps, and the solver iterations of
             the last step of every twentieth of the run (a sample, not a mean over all steps).
  dam_break  a small DFSPH dam break (product.dam_break_scene) to --dam-time seconds under the scene's step size and under
             cflMax = 4 x it, one step per call: steps, mean iterations, the largest density ratio, finiteness, containment.
--default-path LABEL=FILE...: appends the medians of `bench.py --repeats` result lines (parent and this tree) to --out.
    python tools/bench_cfl.py [--parts overhead,buys,dam_break] [--steps 50] [--repeats 5] [--scene-time 1.0] [--out profiles/cfl_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEAD_BENCH = (
    "Adaptive time stepping (DESIGN.md 39), tools/bench_cfl.py.  overhead: product.c2_scene(\"wcsph\") after steps_before_timing steps,\n"
    "mode off against mode pinned (cflMin = cflMax = timeStepSize), windows of steps_per_window synchronous steps ALTERNATING; ms per\n"
    "step, median and every repeat; reduce_us_per_launch: HIP events (sph_profile_*, kernel id 37) around k_cfl_speed on the pinned\n"
    "handle (k_outflow_mark loads the same 20 bytes per particle and was recorded at 11 us per launch at a million particles: a\n"
    "comparison, not a bound).  buys: product.c2_scene(\"dfsph\") to scene_time seconds, the scene's step against cflMax at the listed\n"
    "multiples; wall seconds, steps, sampled iterations.  dam_break: the small DFSPH dam break, fixed against cflMax = 4 x the step.\n"
    "Not measured: the reduce with rigid particles in the scene, any grid cap other than 1024 workgroups, one thread per particle\n"
    "against the strided grid, an LDS reduction, PCISPH / IISPH, scenes whose speed brings the step under the scene's own.\n")
HEAD_DEFAULT = (
    "\nThe default path: result lines of `bench.py --gpus 1 --steps 200 --warmup 20 --repeats 5` of the labelled trees, run alternating\n"
    "in one session on one device; ms per step of every run (the bench's median window), their median, and the windows of every run.\n")


def timed(eng, steps):
    eng.synchronize()
    t0 = time.perf_counter()
    eng.step(steps)
    return 1e3 * (time.perf_counter() - t0) / steps


def overhead(fast_math, steps, repeats, before):
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    handles = {}
    for mode in ("off", "pinned"):
        cfg = P.c2_scene("wcsph")
        if mode == "pinned":
            dt = cfg["Configuration"]["timeStepSize"]
            cfg["Configuration"].update(cflMethod="velocity", cflMinTimeStepSize=dt, cflMaxTimeStepSize=dt)
        container, solver = P.build_product(cfg, fast_math=fast_math)
        solver.prepare()
        container.engine.step(before)
        handles[mode] = container
    ms = {m: [] for m in handles}
    for _ in range(repeats):
        for mode, container in handles.items():
            ms[mode].append(timed(container.engine, steps))
    out = {"part": "overhead", "build": "fast" if fast_math else "strict", "particles": int(handles["off"].engine.particle_num),
           "steps_before_timing": before, "steps_per_window": steps}
    for mode in ms:
        out[mode] = {"ms_per_step_median": round(statistics.median(ms[mode]), 4), "ms_per_step_repeats": [round(v, 4) for v in ms[mode]]}
    out["overhead_us_per_step"] = round(1e3 * (out["pinned"]["ms_per_step_median"] - out["off"]["ms_per_step_median"]), 2)
    e = handles["pinned"].engine
    e.profile_enable(L.K_CFL, True)
    e.profile_reset()
    e.step(steps)
    n, total = e.profile_read(L.K_CFL)
    out["reduce_launches"], out["reduce_us_per_launch"] = int(n), round(1e3 * total / max(1, n), 2)
    out["finite"] = bool(np.isfinite(e.download(L.F_POSITION)).all())
    for container in handles.values():
        container.engine.close()
    return out


def buys(factor, scene_time):
    from sph_project_amd import product as P
    cfg = P.c2_scene("dfsph")
    dt = cfg["Configuration"]["timeStepSize"]
    if factor:
        cfg["Configuration"].update(cflMethod="velocity", cflFactor=0.5, cflMaxTimeStepSize=factor * dt)
    container, solver = P.build_product(cfg, fast_math=1)
    solver.prepare()
    e = container.engine
    e.synchronize()
    its, steps = [], 0
    t0 = time.perf_counter()
    for q in range(1, 21):
        if factor:
            steps += solver.advance_to(scene_time * q / 20)
        else:
            n = int(round(scene_time * q / 20 / dt)) - steps
            solver.advance(n)
            steps += n
        st = solver.stats()
        its.append(st["iter_density"] + st["iter_divergence"])
    e.synchronize()
    wall = time.perf_counter() - t0
    from sph_project_amd import _lib as L
    x = e.download(L.F_POSITION)
    out = {"part": "buys", "scene": "c2_scene(dfsph)", "particles": int(e.particle_num), "timeStepSize": dt, "cflMax_over_dt": factor or None,
           "scene_time": round(float(e.time_state()["time"]), 6), "steps": steps, "wall_s": round(wall, 3),
           "ms_per_step": round(1e3 * wall / max(1, steps), 4), "sampled_iterations_per_step": round(statistics.mean(its), 2),
           "sampled_iterations": its, "finite": bool(np.isfinite(x).all())}
    e.close()
    return out


def dam_break(factor, scene_time):
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    cfg = P.dam_break_scene(method="dfsph", viscosity=0.05)
    dt = cfg["Configuration"]["timeStepSize"]
    if factor:
        cfg["Configuration"].update(cflMethod="velocity", cflFactor=0.5, cflMaxTimeStepSize=factor * dt)
    container, solver = P.build_product(cfg, fast_math=0)
    solver.prepare()
    e = container.engine
    its, ratio, steps = [], 0.0, 0
    if factor:
        e.set_time_target(scene_time)
    while scene_time - e.time_state()["time"] > dt / 1048576.0 and steps < 100000:
        e.step(1)
        steps += 1
        st = e.stats()
        its.append(st["iter_density"] + st["iter_divergence"])
        if steps % 10 == 0:
            ratio = max(ratio, float(e.download(L.F_DENSITY).max()) / 1000.0)
    x = e.download(L.F_POSITION)
    lo, hi = np.zeros(3), np.asarray(cfg["Configuration"]["domainEnd"], dtype=np.float64)
    out = {"part": "dam_break", "particles": int(e.particle_num), "timeStepSize": dt, "cflMax_over_dt": factor or None,
           "scene_time": round(float(e.time_state()["time"]), 9), "steps": steps, "mean_iterations_per_step": round(statistics.mean(its), 3),
           "largest_density_ratio": round(ratio, 5), "finite": bool(np.isfinite(x).all()),
           "inside_the_box": bool(((x >= lo) & (x <= hi)).all())}
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", default="overhead,buys,dam_break")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--before", type=int, default=200)
    ap.add_argument("--scene-time", type=float, default=1.0)
    ap.add_argument("--factors", default="0,2,4")
    ap.add_argument("--dam-time", type=float, default=0.2)
    ap.add_argument("--default-path", nargs="*", default=None, help="files of bench.py result lines: label=path")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dam-out", default=None, help="the dam_break lines go here as well (profiles/cfl_dam_break.txt)")
    args = ap.parse_args()
    lines, dam_lines = [], []
    head = HEAD_BENCH
    if args.default_path is not None:
        head = HEAD_DEFAULT
        for item in args.default_path:
            label, path = item.split("=", 1)
            vals, spreads = [], []
            for line in open(path):
                line = line.strip()
                if line.startswith("{"):
                    r = json.loads(line)
                    vals.append(r.get("ms_per_step", r.get("value")))
                    if "repeat_ms_per_step" in r:
                        spreads.append(r["repeat_ms_per_step"])
            lines.append(json.dumps({"default_path": label, "runs": len(vals), "median_ms_per_step": statistics.median(vals) if vals else None,
                                     "runs_ms_per_step": vals, "windows_ms_per_step": spreads}))
    else:
        parts = args.parts.split(",")
        if "overhead" in parts:
            for fast in (0, 1):
                lines.append(json.dumps(overhead(fast, args.steps, args.repeats, args.before)))
                print(lines[-1], flush=True)
        if "buys" in parts:
            for f in args.factors.split(","):
                lines.append(json.dumps(buys(float(f), args.scene_time)))
                print(lines[-1], flush=True)
        if "dam_break" in parts:
            for f in (0.0, 4.0):
                dam_lines.append(json.dumps(dam_break(f, args.dam_time)))
                print(dam_lines[-1], flush=True)
    text = head + "\n".join(lines + dam_lines) + "\n"
    if args.default_path is not None:
        sys.stdout.write(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)
    if args.dam_out and dam_lines:
        with open(args.dam_out, "a") as f:
            f.write("A small DFSPH dam break (product.dam_break_scene, 8000 particles) to the same scene time under the scene's step size and\n"
                    "under cflMethod \"velocity\" with cflMax = 4 x it (tools/bench_cfl.py --parts dam_break): recorded, not asserted beyond\n"
                    "finiteness, containment and fewer steps (tests/test_hip_cfl.py).\n" + "\n".join(dam_lines) + "\n")


if __name__ == "__main__":
    main()
