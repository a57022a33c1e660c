"""What the micropolar vorticity model costs at C2 (1,231,200 particles, WCSPH, dt 4e-4) in motion (after
--moved steps run with the mode off), both builds: ms/step with the mode off (density + the fused force pass) and on (density, the
gather + walk, non-pressure, v += dt a_mp, pressure + integration), the two modes ALTERNATING --repeats times on one handle (the
median of each and every repeat are reported; other people's work shares the host), the per-kernel times from sph_profile_* (HIP
events; a run of its own behind the timed windows), the tile capacity of the walk and the group-overflow fallbacks of the last
timed step.  --default-path FILE...: appends the medians of `bench.py --repeats` result lines (parent and this tree) to --out.
--stirred-tank: stirred_tank_scene(10) for 300 steps in both builds, kinetic energy and sum |w|^2 every 25 steps.
    python tools/bench_micropolar.py [--steps 100] [--warmup 10] [--moved 2500] [--repeats 5] [--out profiles/micropolar_bench_c2.txt]
    python tools/bench_micropolar.py --stirred-tank [--out profiles/micropolar_stirred_tank.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = {"density": 3, "non_pressure": 4, "pressure_integrate": 5, "wcsph_forces": 18, "micropolar": 32, "misc": 16}
TANK_NU_T, TANK_THETA_INV = 0.2, 0.5   # (the values tests/test_hip_micropolar.py stirs the tank with)
# nbr_tile_cap (sph_device.hpp) of a heavy mask-reusing pass: (40960 - 9 x 128 x 2 - 1536) / bytes per slot - 40, down to a multiple of 8
TILE_CAP = {bytes_: ((40960 - 9 * 128 * 2 - 1536) // bytes_ - 40) // 8 * 8 for bytes_ in (32, 36, 48)}


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


def run_c2(fast_math, moved, steps, warmup, repeats, nu_t, zeta, theta_inv):
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    container, solver = P.build_product(P.c2_scene("wcsph"), fast_math=fast_math)
    solver.prepare()
    eng = container.engine
    solver.advance(moved)
    out = {"build": "fast" if fast_math else "strict", "moved_steps": moved, "particles": int(container.particle_num[None]),
           "steps_per_window": steps, "nu_t": nu_t, "zeta": zeta, "theta_inv": theta_inv}
    ms = {"off": [], "on": []}
    last = {}
    for _ in range(repeats):
        for mode in ("off", "on"):
            eng.set_micropolar("micropolar" if mode == "on" else "none", nu_t, zeta, theta_inv)
            solver.advance(warmup)
            ms[mode].append(round(timed(eng, solver, steps), 4))
            st = eng.stats()
            last[mode] = {"lds_fallback_blocks_last_step": int(st["lds_fallback_blocks"]), "pair_evaluations_last_step": int(st["pair_evaluations"])}
    for mode in ("off", "on"):
        eng.set_micropolar("micropolar" if mode == "on" else "none", nu_t, zeta, theta_inv)
        solver.advance(warmup)
        out[mode] = dict(ms_per_step_median=statistics.median(ms[mode]), ms_per_step_repeats=ms[mode],
                         kernels_us_per_step=profiled(eng, solver, min(steps, 20)), **last[mode])
    w = eng.download(L.F_ANGULAR_VELOCITY)
    out["w_finite"] = bool(np.isfinite(w).all())
    out["w_rms"] = float(np.sqrt((w.astype(np.float64) ** 2).sum(axis=1).mean()))
    eng.close()
    return out


def run_stirred_tank(fast_math, omega, nu_t, theta_inv, steps=300, chunk=25, mode_on=True):
    """mode_on = False: the same block without the vorticity keys (the kinetic energy to compare with; no w)"""
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    cfg = (P.stirred_tank_scene(10, omega=omega, vorticity=nu_t, inertiaInverse=theta_inv) if mode_on
           else P.stirred_tank_scene(10, omega=omega, vorticity_method=None))
    container, solver = P.build_product(cfg, fast_math=fast_math)
    solver.prepare()
    eng = container.engine

    def row(k):
        fl = eng.download(L.F_MATERIAL) == 1
        v, m = eng.download(L.F_VELOCITY).astype(np.float64)[fl], eng.download(L.F_MASS).astype(np.float64)[fl]
        w2 = float((eng.download(L.F_ANGULAR_VELOCITY).astype(np.float64)[fl] ** 2).sum()) if mode_on else None
        return [k, float(0.5 * (m * (v ** 2).sum(axis=1)).sum()), w2]
    traj = [row(0)]
    for k in range(chunk, steps + 1, chunk):
        solver.advance(chunk)
        traj.append(row(k))
    finite = bool(np.isfinite(eng.download(L.F_POSITION)).all())
    eng.close()
    return {"build": "fast" if fast_math else "strict", "vorticityMethod": "micropolar" if mode_on else "none", "omega": omega,
            "nu_t": nu_t, "zeta": 0.1, "theta_inv": theta_inv, "finite": finite,
            "trajectory_step_kinetic_energy_sum_w2": traj}


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
    ap.add_argument("--nu_t", type=float, default=0.01)
    ap.add_argument("--zeta", type=float, default=0.1)
    ap.add_argument("--theta_inv", type=float, default=0.5)
    ap.add_argument("--omega", type=float, default=5.0)
    ap.add_argument("--stirred-tank", action="store_true")
    ap.add_argument("--default-path", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["# " + " ".join(["python", "tools/bench_micropolar.py"] + sys.argv[1:])]
    if args.stirred_tank:
        lines.append("# stirred_tank_scene(10): WCSPH, zero gravity, 1000 fluid particles in rigid rotation about +y in a closed box; "
                     "kinetic energy (J) and sum |w|^2 (1 / s^2) of the fluid every 25 steps -- recorded, not asserted")
        for fast_math, mode_on in ((0, True), (1, True), (0, False)):
            lines.append(json.dumps(run_stirred_tank(fast_math, args.omega, TANK_NU_T, TANK_THETA_INV, mode_on=mode_on)))
            print(lines[-1], flush=True)
    elif args.default_path:
        lines.append("# bench.py --gpus 1 --steps 200 --warmup 20 --repeats 5, parent tree and this tree alternating in one session")
        lines += default_path_lines(args.default_path)
        print("\n".join(lines), flush=True)
    else:
        lines.append("# tile capacity (slots per staging group) by bytes per slot: " + json.dumps(TILE_CAP) +
                     " -- NonPressurePass 32, WcsphForcePass 36, MicropolarPass 48")
        for fast_math in (1, 0):
            lines.append(json.dumps(run_c2(fast_math, args.moved, args.steps, args.warmup, args.repeats, args.nu_t, args.zeta, args.theta_inv)))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.default_path else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
