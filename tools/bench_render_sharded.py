#!/usr/bin/env python
"""Composite cost of sharded frames: product.c2_scene() at rest, reference camera, 1024 x 1024, over 1 (unsharded), 2, 4
and 8 ranks that share ONE GPU (SPH_COMM_TRANSPORT=shm+ipc: the layers travel through the host-staged mailboxes, so the hop cost here is
an upper bound of what RCCL send / recv between devices would show).  Ranks are grouped into at most four worker processes, rank r in
process r % 4, a thread each, never two neighbours in one process.  Per rank count: medians over --frames frames of ms_composite (HIP
events, first send or receive to the end of the last merge; rank 0's and the largest of any rank) and of the whole from_container call
on rank 0 (host clock, frame left on the device).  One JSON line per rank count, appended to --out.

    python tools/bench_render_sharded.py [--ranks 1 2 4 8] [--frames 20] [--out profiles/render_sharded_bench_c2.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_PROCS = 4


def median(v):
    v = sorted(v)
    return 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])


def run_rank(rank, nranks, uid, frames, size, out_dir):
    from sph_project_amd import launch, product as P
    from sph_project_amd.render import FrameRenderer
    cfg = P.c2_scene()
    opts = {}
    if nranks > 1:
        opts["slab"] = dict(rank=rank, nranks=nranks, unique_id=uid, cuts=launch.plan_scene_cuts(cfg, nranks))
    container, solver = P.build_product(cfg, **opts)
    solver.prepare()
    r = FrameRenderer(container.dx, width=size, height=size)
    r.from_container(container, download=False)   # warm-up: buffers, first launches
    wall, comp = [], []
    for _ in range(frames):
        if nranks > 1:
            container.engine.comm_barrier()
        t0 = time.perf_counter()
        r.from_container(container, download=False)
        wall.append(1e3 * (time.perf_counter() - t0))
        cs = r.composite_stats()
        comp.append(cs["ms_composite"])
    res = dict(rank=rank, wall_ms=median(wall), composite_ms=median(comp), hops=cs["hops"], pieces_sent=cs["pieces_sent"],
               bytes_sent=cs["bytes_sent"], drawn_global=cs["drawn_global"], transport=container.engine.comm_transport() if nranks > 1 else "none")
    if rank == 0:
        st = r.stats()
        res.update(ms_render_own=st["ms_total"], covered_pixels=st["covered_pixels"], particles_own=int(st["particles"]))
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)


def worker(args):
    ranks = [int(r) for r in args.worker.split(",")]
    uid = bytes.fromhex(args.uid) if args.uid else None
    if len(ranks) == 1:
        return run_rank(ranks[0], args.nranks, uid, args.frames, args.size, args.dir)
    # the library fills its table of launchers when the first handle of the process is created: before the threads
    from sph_project_amd import product as P
    c, _ = P.build_product(P.dam_break_scene(end=(0.04, 0.04, 0.04)))
    c.engine.close()
    failed = []

    def guarded(rank):
        try:
            run_rank(rank, args.nranks, uid, args.frames, args.size, args.dir)
        except BaseException:  # noqa: BLE001  (reported below; the process exits non-zero)
            import traceback
            traceback.print_exc()
            failed.append(rank)

    threads = [threading.Thread(target=guarded, args=(r,)) for r in ranks]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if failed:
        raise SystemExit(f"ranks {failed} failed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_sharded_bench_c2.txt"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--nranks", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--uid", default="", help=argparse.SUPPRESS)
    ap.add_argument("--dir", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker is not None:
        return worker(args)
    import tempfile
    env = dict(os.environ, SPH_COMM_TRANSPORT="shm+ipc", SPH_COMM_TIMEOUT_S="40")
    with open(args.out, "a") as out:
        out.write(f"python tools/bench_render_sharded.py --frames {args.frames}   (product.c2_scene() at rest, reference camera, "
                  f"{args.size} x {args.size}; ranks share one GPU over shm+ipc; medians of {args.frames} frames, ms)\n")
        for n in args.ranks:
            with tempfile.TemporaryDirectory() as d:
                nprocs = min(n, MAX_PROCS)
                groups = [list(range(i, n, nprocs)) for i in range(nprocs)]
                uid = os.urandom(128).hex()
                procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", ",".join(map(str, g)), "--nranks", str(n),
                                           "--uid", uid, "--dir", d, "--frames", str(args.frames), "--size", str(args.size)], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for g in groups]
                logs = [p.communicate(timeout=900)[0].decode() for p in procs]
                if any(p.returncode for p in procs):
                    raise SystemExit("\n".join(f"---- ranks {g} (exit {p.returncode}):\n{log[-1500:]}" for g, p, log in zip(groups, procs, logs)))
                res = [json.load(open(os.path.join(d, f"rank{r}.json"))) for r in range(n)]
            line = dict(ranks=n, processes=nprocs, transport=res[0]["transport"], frames=args.frames, width=args.size, height=args.size,
                        from_container_ms_rank0=round(res[0]["wall_ms"], 3), ms_composite_rank0=round(res[0]["composite_ms"], 3),
                        ms_composite_max=round(max(r["composite_ms"] for r in res), 3), ms_render_own_rank0=round(res[0]["ms_render_own"], 3),
                        layer_bytes=args.size * args.size * 11, pieces_per_hop=res[-1]["pieces_sent"] if n > 1 else 0,
                        drawn_global=res[0]["drawn_global"], covered_pixels=res[0]["covered_pixels"])
            print(json.dumps(line))
            out.write(json.dumps(line) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
