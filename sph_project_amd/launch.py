"""Ranks of a sharded driver run: what `run_simulation.py --gpus N` needs to start N processes of itself, hand them one communicator id
and cut the scene into z-slabs (sph_project_amd/slab.py).  The pattern is bench.py's own launcher; nothing here opens a GPU.

    spawn_ranks(argv, n)          n fresh child processes of the driver (never exec), rank 0's output relayed, the rest stopped as soon
                                  as one of them exits non-zero
    exchange_unique_id(lib, rank) the 128-byte id of sph_comm_unique_id from rank 0 to the others, through a file
    plan_scene_cuts(cfg, nranks)  slab cuts from the z histogram of the scene's initial particles
"""
from __future__ import annotations

import os
import subprocess
import sys
import threading
import time

import numpy as np

ENV_RANK, ENV_WORLD, ENV_RDV = "SPH_DRIVER_RANK", "SPH_DRIVER_WORLD", "SPH_DRIVER_RDV"


def rank_of_this_process():
    """(rank, world) of a process started by spawn_ranks, or None in any other process."""
    if ENV_RANK not in os.environ:
        return None
    return int(os.environ[ENV_RANK]), int(os.environ[ENV_WORLD])


def spawn_ranks(argv, n, script=None, poll_s=0.05):
    """Start n ranks of `script` (default: the running script) with the arguments argv and wait for them.  Rank 0 writes to this
    process's stdout; the other ranks' stdout is dropped, every rank's stderr is passed through.  A rank that dies leaves its neighbours
    waiting for it: they are stopped (these children, by handle) as soon as any rank exits non-zero.  Returns the exit codes."""
    script = script or os.path.abspath(sys.argv[0])
    rdv = f"/dev/shm/sph_driver_{os.getpid()}_{int(time.time() * 1e6)}.id"
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({ENV_RANK: str(r), ENV_WORLD: str(n), ENV_RDV: rdv})
        procs.append(subprocess.Popen([sys.executable, script] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))

    def relay():
        for line in iter(procs[0].stdout.readline, b""):
            sys.stdout.write(line.decode(errors="replace"))
            sys.stdout.flush()

    reader = threading.Thread(target=relay, daemon=True)
    reader.start()
    try:
        while True:
            rcs = [p.poll() for p in procs]
            if all(rc is not None for rc in rcs):
                break
            if any(rc not in (None, 0) for rc in rcs):
                for p in procs:
                    if p.poll() is None:
                        p.kill()
            time.sleep(poll_s)
    finally:
        for p in procs:   # (an interrupt of the parent leaves nothing running)
            if p.poll() is None:
                p.kill()
        rcs = [p.wait() for p in procs]
        reader.join(timeout=10)
        for path in (rdv, rdv + ".tmp"):
            try:
                os.unlink(path)
            except OSError:
                pass
    return rcs


def exchange_unique_id(lib, rank, timeout_s=120.0):
    """The communicator id of this run: rank 0 makes it (sph_comm_unique_id) and leaves it in the rendezvous file, the others read it."""
    import ctypes
    path = os.environ[ENV_RDV]
    if rank == 0:
        buf = ctypes.create_string_buffer(128)
        if lib.sph_comm_unique_id(buf) != 0:
            raise RuntimeError("sph_comm_unique_id failed")
        with open(path + ".tmp", "wb") as f:
            f.write(buf.raw)
        os.rename(path + ".tmp", path)
        return buf.raw
    t0 = time.time()
    while True:
        try:
            with open(path, "rb") as f:
                data = f.read()
            if len(data) == 128:
                return data
        except OSError:
            pass
        if time.time() - t0 > timeout_s:
            raise RuntimeError(f"rank {rank}: no unique id at {path} after {timeout_s:.0f} s")
        time.sleep(0.01)


def scene_layer_histogram(cfg):
    """Particles per global z cell layer of the domain box and the fluid blocks at their lattice positions (product.scene_particles:
    mesh bodies are not counted; the cuts then follow the fluid as it moves, by the library's rebalancing)."""
    from . import slab
    from .product import scene_particles
    _, geo, batches = scene_particles(cfg)
    nz = int(geo.grid_num[2])
    hist = np.zeros(nz, np.int64)
    for b in batches:
        if len(b["pos"]):
            hist += np.bincount(slab.cell_layer(b["pos"][:, 2], geo.dh, nz), minlength=nz)
    return hist


def plan_scene_cuts(cfg, nranks):
    """Slab cuts (nranks + 1 layer indices, 0 first, nz last) that balance the scene's initial particles: slab.plan_slabs of
    scene_layer_histogram.  ValueError when the grid has too few layers for nranks slabs of two layers."""
    from . import slab
    return [int(k) for k in slab.plan_slabs(scene_layer_histogram(cfg), int(nranks))]
