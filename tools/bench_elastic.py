"""What the elastic solids cost: product.jelly_scene with about one million elastic particles (edge 100: 1,000,000 in
the cube, the sampled box around it), WCSPH, both builds.  Two handles on one device -- the cube with the key "elasticity" and the
same cube as plain fluid (an object cannot be unmarked) -- timed ALTERNATING --repeats times (the median of each and every repeat
are reported; other people's work shares the host), then, in a run of its own, the per-kernel times in microseconds per step from sph_profile_* (HIP events):
id 33 is the scatter + pass A + pass B, id 16 (misc) holds v += dt a_el.  prepare_ms is the host clock around prepare() of each
handle (allocation, upload, first sort; with the key also the capture): recorded, but their difference is inside the noise of the
rest and is NOT a measurement of the capture.  Every mode writes a heading in front of its records, so --out files are what this
tool wrote and nothing else.  --default-path LABEL=FILE...: appends the medians of `bench.py --repeats` result lines (parent and this tree) to --out.
--jelly: jelly_scene(8) under DFSPH for 300 steps with and without the key: largest stretch over the rest pairs and the heights.
    python tools/bench_elastic.py [--edge 100] [--steps 100] [--warmup 10] [--repeats 5] [--out profiles/elastic_bench.txt]
    python tools/bench_elastic.py --jelly [--out profiles/elastic_jelly.txt]
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
    "Elastic solids (DESIGN.md 34), tools/bench_elastic.py: product.jelly_scene(EDGE, method=\"wcsph\"), the cube with the key\n"
    "\"elasticity\" (present) and the same cube as plain fluid (absent) on two handles of one device, windows of steps_per_window\n"
    "steps ALTERNATING; ms per step, median and every repeat.  kernels_us_per_step: HIP events around the launches (sph_profile_*), a run\n"
    "of its own behind the timed windows, microseconds per step: `elastic` (kernel id 33) is the scatter + pass A + pass B together,\n"
    "`misc` (id 16) holds v += dt a_el; the four launches are not timed one by one.  prepare_ms: host clock around prepare(), once;\n"
    "the difference of the two is inside its noise and does not measure the capture.\n")
HEAD_DEFAULT = (
    "\nThe default path: result lines of `bench.py --gpus 1 --steps 200 --warmup 20 --repeats 5` of the labelled trees, run alternating\n"
    "in one session on one device; ms per step of every run (the bench's median window), their median, and the windows of every run.\n")
HEAD_JELLY = (
    "product.jelly_scene(8) (an 8x8x8 cube dropped two particle diameters onto the floor of a sampled box), DFSPH, 300 steps of 2.5e-4 s,\n"
    "tools/bench_elastic.py --jelly: with the key \"elasticity\" {youngsModulus 2e4, poissonRatio 0.3} and without.  Stretch = |x_ij| / |x0_ij|\n"
    "over the pairs of the captured rest lists; y in metres (the floor's first free plane is at 0.08).  Recorded, not asserted against a\n"
    "number: tests/test_hip_elastic.py asserts only that the largest stretch is smaller with the key.\n")

KERNELS = {"density": 3, "non_pressure": 4, "pressure_integrate": 5, "wcsph_forces": 18, "elastic": 33, "misc": 16}


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


def run_bench(fast_math, edge, steps, warmup, repeats, young, poisson):
    from sph_project_amd import product as P
    handles, prepare_ms = {}, {}
    for mode, y in (("absent", None), ("present", young)):
        container, solver = P.build_product(P.jelly_scene(edge, young=y, poisson=poisson, method="wcsph"), fast_math=fast_math)
        t0 = time.perf_counter()
        solver.prepare()
        container.engine.synchronize()
        prepare_ms[mode] = round(1e3 * (time.perf_counter() - t0), 1)
        solver.advance(warmup)
        handles[mode] = (container, solver)
    info = handles["present"][0].engine.get_elastic_object(0)
    out = {"build": "fast" if fast_math else "strict", "particles": int(handles["present"][0].particle_num[None]),
           "elastic_particles": info["count"], "longest_list": info["longest_list"], "steps_per_window": steps,
           "youngs_modulus": young, "poisson_ratio": poisson, "prepare_ms": prepare_ms}
    ms = {"absent": [], "present": []}
    for _ in range(repeats):
        for mode in ("absent", "present"):
            container, solver = handles[mode]
            ms[mode].append(timed(container.engine, solver, steps))
    for mode in ms:
        out[f"ms_per_step_{mode}"] = {"median": round(statistics.median(ms[mode]), 4), "repeats": [round(v, 4) for v in ms[mode]]}
    for mode in ms:
        container, solver = handles[mode]
        out[f"kernels_us_per_step_{mode}"] = profiled(container.engine, solver, min(steps, 50))
    from sph_project_amd import _lib as L
    x = handles["present"][0].engine.download(L.F_POSITION)
    out["finite"] = bool(np.isfinite(x).all())
    return out


def run_jelly(fast_math):
    from sph_project_amd import _lib as L
    from sph_project_amd import product as P
    res, pairs = {}, None
    for young in (2.0e4, None):
        container, solver = P.build_product(P.jelly_scene(8, young=young), fast_math=fast_math)
        solver.prepare()
        eng = container.engine
        by_id = lambda f: (lambda ids, a: a[np.argsort(ids)])(eng.download(L.F_PARTICLE_ID), eng.download(f))
        x0, obj = by_id(L.F_POSITION), by_id(L.F_OBJECT_ID)
        if young is not None:
            pairs = (eng.get_elastic_rest(0)[0], eng.get_elastic_object(0)["first_id"])
        solver.advance(300)
        x = by_id(L.F_POSITION)
        nbr, id0 = pairs
        rows = np.arange(nbr.shape[0])[:, None] + id0
        ok = nbr >= 0
        j = np.where(ok, nbr, id0)
        stretch = np.linalg.norm(x[j] - x[rows], axis=-1) / np.maximum(np.linalg.norm(x0[j] - x0[rows], axis=-1), 1e-12)
        y = x[obj == 0][:, 1]
        res["with the key" if young is not None else "without"] = {
            "largest_stretch": round(float(stretch[ok].max()), 4), "smallest_stretch": round(float(stretch[ok].min()), 4),
            "lowest_y": round(float(y.min()), 4), "highest_y": round(float(y.max()), 4), "mean_y": round(float(y.mean()), 4)}
    return {"build": "fast" if fast_math else "strict", "scene": "jelly_scene(8), dfsph, 300 steps of 2.5e-4 s", **res}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--edge", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--young", type=float, default=2.0e4)
    ap.add_argument("--poisson", type=float, default=0.3)
    ap.add_argument("--jelly", action="store_true")
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
    elif args.jelly:
        head = HEAD_JELLY
        for fast in (0, 1):
            lines.append(json.dumps(run_jelly(fast)))
    else:
        for fast in (0, 1):
            lines.append(json.dumps(run_bench(fast, args.edge, args.steps, args.warmup, args.repeats, args.young, args.poisson)))
    text = head + "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
