"""What the outflow volumes cost: product.channel_scene with a NOZZLE x NOZZLE nozzle, no sampled box (an all-fluid scene, so
the pre-hashed sort of the WCSPH step is in play) and no gravity, WCSPH, both builds.  Three handles on one device are brought to the
same step count, at which the jet's head has reached the place of the kill box and about --layers layers are alive:
  "none"    the emitter ends there, no volume: a fixed particle count, asynchronous steps, pre-hashed sorts
  "far"     the same with a volume where no particle is: the mark pass, the lost pre-hashed sort and the per-step count read-back alone
  "steady"  the emitter goes on and the kill box removes about a layer per emission
and timed ALTERNATING --repeats times in windows of --steps steps (the median and every repeat are reported; other people's work shares
the host).  Then, in runs of their own, HIP events around the launches (sph_profile_*): SPH_K_OUTFLOW per launch on the steady handle,
and the three sort ids (hash, scan, scatter) per one-step call there: a call whose slot removed something runs a second sort, by the
graveyard route, before it returns; a call whose slot removed nothing runs the step's list sort alone.
--default-path LABEL=FILE...: appends the medians of `bench.py --repeats` result lines (parent and this tree) to --out.
    python tools/bench_outflow.py [--nozzle 100] [--layers 100] [--speed 4.0] [--steps 20] [--repeats 5] [--out profiles/outflow_bench.txt]
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
    "Outflow volumes (DESIGN.md 37), tools/bench_outflow.py: product.channel_scene((N, N), method=\"wcsph\", addDomainBox=False, gravity=0),\n"
    "three handles of one device at the same step count: `none` (the emitter ended, no volume), `far` (the same with a volume where no\n"
    "particle is) and `steady` (the emitter goes on, the kill box removes about a layer per emission), windows of steps_per_window steps\n"
    "ALTERNATING; ms per step, median and every repeat, the particle count at the start of every window, lost_prehash (the share of the\n"
    "timed steps whose sort hashed for itself).  mark_us_per_launch: HIP events (sph_profile_*, kernel id 36) around k_outflow_mark on the\n"
    "steady handle (k_emit_hold, the nearest existing elementwise pass, was recorded at 7-8 us per launch at this size: a comparison, not\n"
    "a bound).  sort_us: hash + scan + scatter (ids 0, 1, 2) per one-step call: `list` on the far handle (the step's own sort, by run\n"
    "lists, hashing for itself), `list_plus_graveyard` a call of the steady handle whose slot removed something (the same plus the\n"
    "sort that drops the dead before the call returns), `graveyard` their difference.\n"
    "Not measured: more than one volume, spheres, the strict build's isolated pieces against the fast build's (both are listed, neither\n"
    "is compared), removal by id (sph_remove_particles: a host path with two downloads), anything under DFSPH / PCISPH / IISPH.\n")
HEAD_DEFAULT = (
    "\nThe default path: result lines of `bench.py --gpus 1 --steps 200 --warmup 20 --repeats 5` of the labelled trees, run alternating\n"
    "in one session on one device; ms per step of every run (the bench's median window), their median, and the windows of every run.\n")


def timed(eng, solver, steps):
    eng.synchronize()
    t0 = time.perf_counter()
    solver.advance(steps)
    eng.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def scene_of(mode, nozzle, layers, speed, k0):
    from sph_project_amd import product as P
    dt = float(np.float32(4e-4))
    # (the two handles whose emitter ends get a longer channel: their jet flies on through the timed windows and must not reach the end)
    cfg = P.channel_scene((nozzle, nozzle), speed=speed, length=layers + 13 + (0 if mode == "steady" else 40), method="wcsph", side=nozzle + 30,
                          max_layers=layers + 140, gravity=0.0, addDomainBox=False)
    if mode != "steady":
        cfg["Emitters"][0]["end"] = (k0 + 0.5) * dt
    if mode == "none":
        cfg.pop("Outflows")
    elif mode == "far":
        w = cfg["Configuration"]["domainEnd"][1]
        cfg["Outflows"][0].update(min=[0.0, w - 0.04, 0.0], max=[0.04, w, 0.04])   # a corner the jet never reaches
    return cfg


def run_bench(fast_math, nozzle, layers, speed, steps, repeats):
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    dt, d = float(np.float32(4e-4)), 0.02
    k0 = int(layers * d / (speed * dt))   # the head is `layers` spacings from the nozzle: at the kill box's first face
    handles = {}
    for mode in ("none", "far", "steady"):
        container, solver = P.build_product(scene_of(mode, nozzle, layers, speed, k0), fast_math=fast_math)
        solver.prepare()
        solver.advance(k0 + 10)
        handles[mode] = (container, solver)
    out = {"build": "fast" if fast_math else "strict", "nozzle": nozzle, "layer_particles": nozzle * nozzle, "speed": speed,
           "steps_per_layer": round(d / (speed * dt), 3), "steps_before_timing": k0 + 10, "steps_per_window": steps}
    ms = {m: [] for m in handles}
    counts = {m: [] for m in handles}
    st0 = {m: handles[m][0].engine.stats() for m in handles}
    removed0 = handles["steady"][1].outflows[0].removed
    for _ in range(repeats):
        for mode in handles:
            container, solver = handles[mode]
            counts[mode].append(int(container.engine.particle_num))
            ms[mode].append(timed(container.engine, solver, steps))
    for mode in ms:
        st = handles[mode][0].engine.stats()
        sorts = (st["hash_launches"] - st0[mode]["hash_launches"]) + (st["prehashed_sorts"] - st0[mode]["prehashed_sorts"])
        out[mode] = {"ms_per_step_median": round(statistics.median(ms[mode]), 4), "ms_per_step_repeats": [round(v, 4) for v in ms[mode]],
                     "particles_at_window_start": counts[mode],
                     "lost_prehash": round((st["hash_launches"] - st0[mode]["hash_launches"]) / max(1, sorts), 3)}
    out["steady"]["removed_in_the_windows"] = int(handles["steady"][1].outflows[0].removed - removed0)
    out["overhead_far_vs_none"] = round(out["far"]["ms_per_step_median"] / out["none"]["ms_per_step_median"] - 1.0, 4)
    # the isolated pieces, runs of their own: one-step calls on the far handle (every call: the step's own sort, by run lists) and on the
    # steady handle (a call whose slot removed something sorts a second time, by the graveyard route, before it returns)
    ids = tuple(L.KERNEL_IDS.index(name) for name in ("hash_count", "scan", "scatter")) + (L.K_OUTFLOW,)
    sort_ms = {"far": {True: [], False: []}, "steady": {True: [], False: []}}
    for mode in ("far", "steady"):
        container, solver = handles[mode]
        e = container.engine
        for k in ids:
            e.profile_enable(k, True)
        e.profile_reset()
        last = 0.0
        for _ in range(2 * steps):
            e.step(1)
            now = sum(e.profile_read(k)[1] for k in ids[:3])
            sort_ms[mode][solver.outflows[0].removed_last_step > 0].append(now - last)
            last = now
    n_mark, ms_mark = e.profile_read(L.K_OUTFLOW)
    out["mark_launches"], out["mark_us_per_launch"] = int(n_mark), round(1e3 * ms_mark / max(1, n_mark), 2)
    med = lambda v: statistics.median(v) if v else None
    us = lambda v: None if v is None else round(1e3 * v, 2)
    lst, lst_steady, both = med(sort_ms["far"][False]), med(sort_ms["steady"][False]), med(sort_ms["steady"][True])
    out["sort_us"] = {"list": us(lst), "list_on_the_steady_handle": us(lst_steady), "list_plus_graveyard": us(both),
                      "graveyard": None if lst is None or both is None else us(both - lst),
                      "calls": {"far": len(sort_ms["far"][False]), "steady_without_removal": len(sort_ms["steady"][False]),
                                "steady_with_removal": len(sort_ms["steady"][True])}}
    out["particles_at_the_end"] = int(e.particle_num)
    out["finite"] = bool(np.isfinite(e.download(L.F_POSITION)).all())
    for container, _ in handles.values():
        container.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nozzle", type=int, default=100)
    ap.add_argument("--layers", type=int, default=100)
    ap.add_argument("--speed", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
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
