"""What the fluid emitters cost: product.faucet_scene with a NOZZLE x NOZZLE nozzle and no sampled box (an all-fluid scene,
so the pre-hashed sort of the WCSPH step is in play), WCSPH, both builds.  Two handles on one device are brought to the same step count
-- "running": the emitter goes on (hold 2), "ended": the same emitter with `end` at that count, so the same particle state with nothing
born and nothing held afterwards -- and timed ALTERNATING --repeats times in windows of --steps steps (the median of each and every
repeat are reported; other people's work shares the host; the running handle grows by a layer every spacing / (speed dt) steps, its
count is recorded with every window).  Then, in a run of its own, HIP events around the launches (sph_profile_*, kernel id 34): the
time per launch of k_emit from a handle with hold 0 (nothing else under the id), and of the hold pass from the running handle (its
total less its emit launches at that time).  lost_prehash: the share of the timed steps whose sort had to hash for itself.
--faucet: faucet_scene((4, 4), basin=3) three diameters above the pool at 2 m/s and one diameter above it at 8 m/s, for 300 steps under DFSPH (its own stop tests) and WCSPH with hold 0 and 2: largest density
ratio, the share of the emitter's particles behind the nozzle plane, solver iterations per step.  Recorded, not asserted.
--default-path LABEL=FILE...: appends the medians of `bench.py --repeats` result lines (parent and this tree) to --out.
    python tools/bench_emitter.py [--nozzle 100] [--layers 100] [--speed 4.0] [--steps 20] [--repeats 5] [--out profiles/emitter_bench.txt]
    python tools/bench_emitter.py --faucet [--out profiles/emitter_faucet.txt]
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
    "Fluid emitters (DESIGN.md 35), tools/bench_emitter.py: product.faucet_scene((N, N), method=\"wcsph\", addDomainBox=False), two handles of\n"
    "one device at the same step count: `running` (the emitter goes on, hold 2) and `ended` (the same emitter with `end` at that count: same\n"
    "particle state, nothing born, nothing held), windows of steps_per_window steps ALTERNATING; ms per step, median and every repeat, and\n"
    "the particle count at the start of every window.  emit_us_per_launch: HIP events (sph_profile_*, kernel id 34) around k_emit on a handle\n"
    "with hold 0; hold_us_per_launch: the running handle's id-34 time less its emit launches at that figure, per hold launch.  lost_prehash:\n"
    "share of the timed steps whose sort hashed for itself (hash_launches / sorts).\n")
HEAD_DEFAULT = (
    "\nThe default path: result lines of `bench.py --gpus 1 --steps 200 --warmup 20 --repeats 5` of the labelled trees, run alternating\n"
    "in one session on one device; ms per step of every run (the bench's median window), their median, and the windows of every run.\n")
HEAD_FAUCET = (
    "product.faucet_scene((4, 4), basin=3) (a 4 x 4 nozzle under the lid of a sampled box over a pool three layers deep) in two arrangements:\n"
    "`above` (speed 2, height 16: the nozzle three particle diameters above the pool) and `touching` (speed 8, height 14: one diameter above\n"
    "it, so the jet meets resistance from its second layer on), 300 steps\n"
    "of 4e-4 s, tools/bench_emitter.py --faucet, fast build: largest density / density0 over the fluid at the end and over the sampled steps\n"
    "(every 10th), the share of the emitter's particles behind the nozzle plane at the end (and the largest share seen), mean solver\n"
    "iterations per step.  Recorded, not asserted against a number: tests/test_hip_emitter.py asserts the count, finiteness, the domain and\n"
    "the held layers' positions.\n")


def timed(eng, solver, steps):
    eng.synchronize()
    t0 = time.perf_counter()
    solver.advance(steps)
    eng.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def fill_scene(nozzle, layers, speed, hold, end=None):
    from sph_project_amd import product as P
    cfg = P.faucet_scene((nozzle, nozzle), speed=speed, hold=hold, basin=0, method="wcsph", side=nozzle + 30, height=nozzle + 20,
                         max_layers=layers + 40, addDomainBox=False)
    cfg["Emitters"][0]["end"] = end
    return cfg


def run_bench(fast_math, nozzle, layers, speed, steps, repeats):
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    dt, d = float(np.float32(4e-4)), 0.02
    k0 = int(layers * d / (speed * dt))                   # the step count at which about `layers` layers are alive
    end = (k0 + 0.5) * dt
    handles = {}
    for mode, cfg in (("running", fill_scene(nozzle, layers, speed, 2)), ("ended", fill_scene(nozzle, layers, speed, 2, end=end))):
        container, solver = P.build_product(cfg, fast_math=fast_math)
        solver.prepare()
        solver.advance(k0 + 10)                           # ten steps past `end`: the ended handle's last held layers are long released
        handles[mode] = (container, solver)
    out = {"build": "fast" if fast_math else "strict", "nozzle": nozzle, "layer_particles": nozzle * nozzle, "speed": speed,
           "steps_per_layer": round(d / (speed * dt), 3), "steps_before_timing": k0 + 10, "steps_per_window": steps}
    ms = {"running": [], "ended": []}
    counts = {"running": [], "ended": []}
    st0 = {m: handles[m][0].engine.stats() for m in handles}
    for _ in range(repeats):
        for mode in ("running", "ended"):
            container, solver = handles[mode]
            counts[mode].append(int(container.engine.particle_num))
            ms[mode].append(timed(container.engine, solver, steps))
    for mode in ms:
        st = handles[mode][0].engine.stats()
        sorts = (st["hash_launches"] - st0[mode]["hash_launches"]) + (st["prehashed_sorts"] - st0[mode]["prehashed_sorts"])
        out[mode] = {"ms_per_step_median": round(statistics.median(ms[mode]), 4), "ms_per_step_repeats": [round(v, 4) for v in ms[mode]],
                     "particles_at_window_start": counts[mode],
                     "lost_prehash": round((st["hash_launches"] - st0[mode]["hash_launches"]) / max(1, sorts), 3)}
    # per launch, a run of its own: k_emit alone on a small handle with hold 0 (its threads are the layer's, whatever is alive) ...
    container, solver = P.build_product(fill_scene(nozzle, 8, speed, 0), fast_math=fast_math)
    solver.prepare()
    e = container.engine
    e.profile_enable(L.K_EMIT, True)
    solver.advance(int(6 * d / (speed * dt)))
    e.synchronize()
    n_emit, ms_emit = e.profile_read(L.K_EMIT)
    out["emit_launches"], out["emit_us_per_launch"] = int(n_emit), round(1e3 * ms_emit / max(1, n_emit), 2)
    e.close()
    # ... and the hold pass on the running handle (one id load per live particle)
    container, solver = handles["running"]
    e = container.engine
    layers0 = solver.emitters[0].layers
    e.profile_enable(L.K_EMIT, True)
    e.profile_reset()
    solver.advance(steps)
    e.synchronize()
    n_all, ms_all = e.profile_read(L.K_EMIT)
    emits = solver.emitters[0].layers - layers0
    holds = int(n_all) - emits
    out["hold_launches"], out["hold_us_per_launch"] = holds, round(1e3 * (ms_all - emits * 1e-3 * out["emit_us_per_launch"]) / max(1, holds), 2)
    out["hold_share_of_step"] = round(1e-3 * out["hold_us_per_launch"] / out["running"]["ms_per_step_median"], 4)
    out["particles_at_the_end"] = int(e.particle_num)
    out["finite"] = bool(np.isfinite(e.download(L.F_POSITION)).all())
    return out


FAUCETS = {"above": dict(speed=2.0, height=16), "touching": dict(speed=8.0, height=14)}


def run_faucet(method, hold, which):
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    cfg = P.faucet_scene((4, 4), hold=hold, basin=3, method=method, max_layers=130, **FAUCETS[which])
    container, solver = P.build_product(cfg, fast_math=1)
    solver.prepare()
    e = container.engine
    em = cfg["Emitters"][0]
    pos0, dirn = np.asarray(em["position"], np.float64), np.asarray(em["direction"], np.float64)
    rho0 = float(cfg["Configuration"]["density0"])
    worst_rho = worst_behind = 0.0
    iters = {"iter_density": [], "iter_divergence": []}
    for _ in range(30):
        for _ in range(10):
            solver.step()
            st = solver.stats()
            for key in iters:
                iters[key].append(st[key])
        mat, obj = e.download(L.F_MATERIAL), e.download(L.F_OBJECT_ID)
        rho, x = e.download(L.F_DENSITY), e.download(L.F_POSITION).astype(np.float64)
        ratio = float(rho[mat == 1].max()) / rho0
        mine = obj == em["objectId"]
        behind = float((((x[mine] - pos0) @ dirn) < 0.0).mean()) if mine.any() else 0.0
        worst_rho, worst_behind = max(worst_rho, ratio), max(worst_behind, behind)
    out = {"scene": which, **FAUCETS[which], "method": method, "hold": hold, "particles": int(e.particle_num), "emitted": int(solver.emitters[0].emitted),
           "density_ratio_end": round(ratio, 4), "density_ratio_largest": round(worst_rho, 4),
           "behind_the_plane_end": round(behind, 4), "behind_the_plane_largest": round(worst_behind, 4), "finite": bool(np.isfinite(x).all())}
    if method == "dfsph":
        out["iterations_per_step"] = {k: round(float(np.mean(v)), 2) for k, v in iters.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nozzle", type=int, default=100)
    ap.add_argument("--layers", type=int, default=100)
    ap.add_argument("--speed", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--faucet", action="store_true")
    ap.add_argument("--default-path", nargs="*", default=None, help="files of bench.py result lines: label=path")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
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
    elif args.faucet:
        head = HEAD_FAUCET
        for which in FAUCETS:
            for method in ("dfsph", "wcsph"):
                for hold in (0, 2):
                    lines.append(json.dumps(run_faucet(method, hold, which)))
    else:
        for fast in (0, 1):
            lines.append(json.dumps(run_bench(fast, args.nozzle, args.layers, args.speed, args.steps, args.repeats)))
    text = head + "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
