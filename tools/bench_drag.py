"""What the air drag costs at C2 (1,231,200 particles, WCSPH, dt 4e-4) in motion (after --moved steps run
with the mode off), both builds: ms/step with the mode off (density + the fused force pass) and on (density, the drag walk,
non-pressure, v += dt a_drag, pressure + integration), the two modes ALTERNATING --repeats times on one handle (the median of each
and every repeat are reported; other people's work shares the host), the per-kernel times from sph_profile_* (HIP events; a run of
its own behind the timed windows) -- the walk is kernel id 35, the apply is the growth of "misc" (16) between the two modes -- and
the walk's algorithmic traffic (64 B per particle: posv 16 + velm 16 read, two float4 written) as a share of the 8 TB/s HBM peak.
--default-path FILE...: appends the medians of `bench.py --repeats` result lines (parent and this tree) to --out.
--wind-jet: wind_jet_scene for 300 steps in both builds, three twins (drag off, drag on in still air, drag on in a wind along +x).
    python tools/bench_drag.py [--steps 100] [--warmup 10] [--moved 2500] [--repeats 5] [--out profiles/drag_bench_c2.txt]
    python tools/bench_drag.py --wind-jet [--out profiles/drag_jet.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = {"density": 3, "non_pressure": 4, "pressure_integrate": 5, "wcsph_forces": 18, "drag": 35, "misc": 16}
WALK_BYTES = 64          # per particle: R posv 16 + velm 16 -> W dr_acc 16 + dr_terms 16
HBM_PEAK = 8.0e12        # bytes / s


def timed(eng, solver, steps):
    eng.synchronize()
    t0 = time.perf_counter()
    solver.advance(steps)
    eng.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def profiled(eng, solver, steps):
    eng.profile_enable(-1, True)
    eng.profile_reset()
    for _ in range(steps):
        solver.step()
    eng.synchronize()
    out = {k: round(1e3 * eng.profile_read(i)[1] / steps, 2) for k, i in KERNELS.items() if eng.profile_read(i)[0] > 0}
    eng.profile_enable(-1, False)
    return out


def run_c2(fast_math, moved, steps, warmup, repeats, k, wind):
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    container, solver = P.build_product(P.c2_scene("wcsph"), fast_math=fast_math)
    solver.prepare()
    eng = container.engine
    solver.advance(moved)
    n = int(container.particle_num[None])
    out = {"build": "fast" if fast_math else "strict", "moved_steps": moved, "particles": n, "steps_per_window": steps, "k": k,
           "air_velocity": list(wind)}
    ms = {"off": [], "on": []}
    for _ in range(repeats):
        for mode in ("off", "on"):
            eng.set_drag("gissler" if mode == "on" else "none", k, 1.2041, wind)
            solver.advance(warmup)
            ms[mode].append(round(timed(eng, solver, steps), 4))
    for mode in ("off", "on"):
        eng.set_drag("gissler" if mode == "on" else "none", k, 1.2041, wind)
        solver.advance(warmup)
        out[mode] = dict(ms_per_step_median=statistics.median(ms[mode]), ms_per_step_repeats=ms[mode],
                         kernels_us_per_step=profiled(eng, solver, min(steps, 20)))
    walk_us = out["on"]["kernels_us_per_step"].get("drag")
    out["walk_us"] = walk_us
    out["apply_us_misc_on_minus_off"] = round(out["on"]["kernels_us_per_step"].get("misc", 0.0) - out["off"]["kernels_us_per_step"].get("misc", 0.0), 2)
    if walk_us:
        rate = WALK_BYTES * n / (walk_us * 1e-6)
        out["walk_bytes_per_particle"] = WALK_BYTES
        out["walk_TB_per_s"] = round(rate / 1e12, 3)
        out["walk_share_of_hbm_peak"] = round(rate / HBM_PEAK, 4)
    t = eng.download(L.F_DRAG_TERMS)
    fl = eng.download(L.F_MATERIAL) == 1
    out["terms_finite"] = bool(np.isfinite(t).all() and np.isfinite(eng.download(L.F_DRAG_ACCEL)).all())
    out["mean_n_i"] = float(t[fl, 0].mean())
    out["exposed_share_w_above_half"] = float((t[fl, 1] > 0.5).mean())
    eng.close()
    return out


def run_wind_jet(fast_math, steps=300):
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    out = {"build": "fast" if fast_math else "strict", "steps": steps}
    for how, keys in (("off", dict(drag_method=None)), ("drag", dict(wind=(0.0, 0.0, 0.0))), ("wind", dict(wind=(5.0, 0.0, 0.0)))):
        container, solver = P.build_product(P.wind_jet_scene(**keys), fast_math=fast_math)
        solver.prepare()
        solver.advance(steps)
        eng = container.engine
        x, v = eng.download(L.F_POSITION).astype(np.float64), eng.download(L.F_VELOCITY).astype(np.float64)
        jet = (eng.download(L.F_OBJECT_ID) == 0) & (eng.download(L.F_MATERIAL) == 1)
        out[how] = {"particles": int(jet.sum()), "mean_x": float(x[jet, 0].mean()), "mean_y": float(x[jet, 1].mean()),
                    "mean_downward_speed": float(-v[jet, 1].mean()), "mean_vx": float(v[jet, 0].mean()),
                    "finite": bool(np.isfinite(x).all() and np.isfinite(v).all())}
        eng.close()
    out["shift_x_wind_minus_off"] = out["wind"]["mean_x"] - out["off"]["mean_x"]
    out["downward_speed_drag_minus_off"] = out["drag"]["mean_downward_speed"] - out["off"]["mean_downward_speed"]
    return out


def default_path_lines(files):
    """One line per bench.py result file: its label (the file's name), the median ms/step and the repeats bench.py reports."""
    lines = []
    for path in files:
        with open(path) as f:
            res = [json.loads(l) for l in f if l.lstrip().startswith("{")][-1]
        lines.append(json.dumps({"default_path": os.path.basename(path), "ms_per_step": res.get("ms_per_step"),
                                 "repeat_ms_per_step": res.get("repeat_ms_per_step")}))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--moved", type=int, default=2500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k", type=float, default=1.0)
    ap.add_argument("--wind", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--wind-jet", action="store_true")
    ap.add_argument("--default-path", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["# " + " ".join(["python", "tools/bench_drag.py"] + sys.argv[1:])]
    if args.wind_jet:
        lines.append("# wind_jet_scene(): WCSPH, a 4 x 4 nozzle at 3 m / s pointing down under the lid of a tall closed box, 300 steps; the emitter's "
                     "particles with the drag off, on in still air and on in a wind of 5 m / s along +x -- recorded, not asserted")
        for fast_math in (0, 1):
            lines.append(json.dumps(run_wind_jet(fast_math)))
            print(lines[-1], flush=True)
    elif args.default_path:
        lines.append("# bench.py --gpus 1 --steps 200 --warmup 20 --repeats 5, parent tree and this tree alternating in one session")
        lines += default_path_lines(args.default_path)
        print("\n".join(lines), flush=True)
    else:
        for fast_math in (1, 0):
            lines.append(json.dumps(run_c2(fast_math, args.moved, args.steps, args.warmup, args.repeats, args.k, tuple(args.wind))))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.default_path else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
