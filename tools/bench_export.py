"""ms per frame of the text exports on C2 (product.c2_scene(), 1.23 M particles), strict build, from rest and again after
the in-motion steps of the bench line (2500).  Per state the PLY of the fluid object and the OBJ of its reconstructed surface (the
reference's splashsurf settings with smoothing), one untimed frame of each path and then --frames timed frames on which the two paths
alternate, writing to the same directory:
  host    PLY: container.dump (position and object-id download, numpy mask) + sph_write_ply_ascii
          OBJ: the mesh download (sph_surface_download) + sph_write_obj_ascii
  device  PLY: TextExporter.ply_object + write          OBJ: TextExporter.obj_surface + write (the mesh stays on the device)
Reported per state and file type: the medians with the spread (min, max) of both paths' frame times (host clock around the whole
path), the stage times of SphTextStats (HIP events; ms_file: host clock in fwrite), the file's bytes and bytes per second, and once per
state that the two files are identical.  One JSON line per state and file type; with --out also written to that file
(profiles/export_bench_c2.txt)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.run_simulation import write_ply_ascii  # noqa: E402
from sph_project_amd.surface import SurfaceReconstructor  # noqa: E402
from sph_project_amd.text import TextExporter  # noqa: E402


def _ms(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def measure(kind, host, device, exporter, paths, frames, label, step):
    host_path, device_path = paths
    host()
    device()   # untimed: allocations, pinned buffers, first touch
    same = open(host_path, "rb").read() == open(device_path, "rb").read()
    rows = []
    for _ in range(frames):
        h = _ms(host)
        d = _ms(device)
        rows.append(dict(host_ms=h, device_ms=d, **{k: v for k, v in exporter.stats().items() if k.startswith("ms_")}))
    st = exporter.stats()
    med = lambda key: round(float(np.median([r[key] for r in rows])), 3)  # noqa: E731
    out = dict(state=label, step=step, file=kind, frames=frames, identical=same, file_bytes=st["bytes"], rows=st["rows"], values=st["values"],
               pieces=st["pieces"], longest_row=st["longest_row"])
    for key in rows[0]:
        out[key] = med(key)
    for key in ("host_ms", "device_ms"):
        out[key.replace("_ms", "_min_ms")] = round(min(r[key] for r in rows), 3)
        out[key.replace("_ms", "_max_ms")] = round(max(r[key] for r in rows), 3)
    out["host_MB_per_s"] = round(st["bytes"] / out["host_ms"] / 1e3, 1)
    out["device_MB_per_s"] = round(st["bytes"] / out["device_ms"] / 1e3, 1)
    out["speedup"] = round(out["host_ms"] / out["device_ms"], 2)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--no-obj", action="store_true", help="PLY only")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    exporter = TextExporter()
    recon = None
    if not a.no_obj:
        recon = SurfaceReconstructor(container.dx)
        recon.set_postprocess(mesh_smoothing_iters=25, mesh_smoothing_weights=True, weights_normalization=13.0, normals_smoothing_iters=10)
    lines = []
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        def state(label, step):
            ply = (os.path.join(d, "host.ply"), os.path.join(d, "device.ply"))
            lines.append(measure("ply", lambda: write_ply_ascii(ply[0], container.dump(0)["position"]),
                                 lambda: exporter.ply_object(container, 0).write(ply[1]), exporter, ply, a.frames, label, step))
            if recon is not None:
                obj = (os.path.join(d, "host.obj"), os.path.join(d, "device.obj"))
                recon.from_container(container, 0, download=False)

                def host_obj():
                    recon._download()
                    recon.write_obj(obj[0])
                    recon.mesh = None   # (the next frame downloads again, as a driver's frame would)
                lines.append(measure("obj", host_obj, lambda: exporter.obj_surface(recon).write(obj[1]), exporter, obj, a.frames, label, step))

        state("rest", 0)
        if a.motion_step > 0:
            container.engine.step(a.motion_step)
            container.engine.synchronize()
            state("in_motion", a.motion_step)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_export.py: medians over %d frames per state, host and device path alternating on the same frames; times in ms\n"
                    "# (host_ms / device_ms: host clock around the whole path; ms_*: SphTextStats of the device path)\n" % a.frames)
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
