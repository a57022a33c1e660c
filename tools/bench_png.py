"""ms per frame of the PNG encoder on C2 (product.c2_scene(), 1.23 M particles) at the reference's camera and 1024^2,
strict build, from rest and again after the in-motion steps of the bench line (2500).  Per state a particle frame (raw_view.png) and,
with --render_meshes, a mesh frame of the reconstructed surface (render.png): one untimed frame, then --frames timed frames.  Per frame:
the GPU encode by stage (HIP events) and around the call (host clock), the download of the file, and in the same run what storing the
same frame costs on the parent's path: the raw download of the frame (sph_render_download) plus encode_png on the host.  Sizes: the
device's file against encode_png (zlib level 6) and against the same filter-0 stream at zlib level 1.  The device's file is decoded
once per state and compared with the pixels.  --coding fixed | dynamic | window | both | all: which coding the encoder uses; `both`
(fixed, dynamic) and `all` (fixed, dynamic, window) encode every timed frame with one encoder per coding in alternation (the same frame,
the same host reference) and report per coding the stage times, the file bytes, size_vs_host, dynamic_segments and the dynamic headers'
bytes, and for window the candidates' stage, window_segments and the far matches.  One JSON line per state, frame kind and coding; with
--out also written to that file (profiles/png_bench_c2.txt, profiles/png_dynamic_bench_c2.txt, profiles/png_window_bench_c2.txt)."""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.png import PngEncoder  # noqa: E402
from sph_project_amd.render import FrameRenderer, encode_png  # noqa: E402
from sph_project_amd.surface import SurfaceReconstructor  # noqa: E402
from sph_project_amd.video import decode_png  # noqa: E402


def _ms(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def measure(r, encoders, draw, frames, label, step, kind):
    """encoders: {coding: PngEncoder}; every timed frame is encoded by each of them in turn"""
    draw()   # untimed: allocations, first touch
    for v in encoders.values():
        assert np.array_equal(decode_png(v.encode_last(r)), r.last_rgb())   # every coding's file decodes to the frame's pixels
    rows = {c: [] for c in encoders}
    for _ in range(frames):
        draw()
        raw_host, rgb = _ms(r.last_rgb)
        png_host, png = _ms(lambda: encode_png(rgb))
        for coding, v in encoders.items():
            enc_host, _ = _ms(lambda: v._chk(v.lib.sph_png_encode_render(v.h, r._last), "sph_png_encode_render"))
            st = v.stats()
            dl_host, png_dev = _ms(v._download)
            rows[coding].append(dict(encode_ms=st["ms_total"], filter_ms=st["ms_filter"], candidates_ms=st["ms_candidates"], count_ms=st["ms_count"], scan_ms=st["ms_scan"],
                                     write_ms=st["ms_write"], encode_host_ms=enc_host, file_download_host_ms=dl_host,
                                     raw_download_host_ms=raw_host, png_encode_host_ms=png_host,
                                     gpu_path_host_ms=enc_host + dl_host, host_path_host_ms=raw_host + png_host,
                                     device_png_bytes=len(png_dev), host_png_bytes=len(png), stored_segments=st["stored_segments"],
                                     dynamic_segments=st["dynamic_segments"], dynamic_header_bytes=(st["dynamic_header_bits"] + 7) // 8,
                                     window_segments=st["window_segments"], window_matches=st["window_matches"],
                                     window_far_matches=st["window_far_matches"], window_header_bytes=(st["window_header_bits"] + 7) // 8,
                                     segments=st["segments"], literals=st["literals"], matches=st["matches"], filter_rows=st["filter_rows"]))
    raw = np.zeros((r.height, 1 + 3 * r.width), np.uint8)
    raw[:, 1:] = rgb.reshape(r.height, 3 * r.width)
    zlib1 = len(zlib.compress(raw.tobytes(), 1)) + len(png) - len(zlib.compress(raw.tobytes(), 6))
    return [summary(rows[c], r, frames, label, step, kind, c, zlib1) for c in encoders]


def summary(rows, r, frames, label, step, kind, coding, zlib1):
    med = lambda key: round(float(np.median([row[key] for row in rows])), 3)  # noqa: E731
    out = dict(state=label, kind=kind, coding=coding, step=step, frames=frames, width=r.width, height=r.height)
    out.update({k: med(k) for k in rows[0] if k.endswith("_ms")})
    out.update({k: rows[0][k] for k in rows[0] if not k.endswith("_ms")})
    host = [row["host_path_host_ms"] for row in rows]
    out["host_path_min_ms"], out["host_path_max_ms"] = round(min(host), 3), round(max(host), 3)
    out["gpu_path_max_ms"] = round(max(row["gpu_path_host_ms"] for row in rows), 3)
    out["encode_min_ms"], out["encode_max_ms"] = round(min(row["encode_ms"] for row in rows), 3), round(max(row["encode_ms"] for row in rows), 3)
    out["speedup"] = round(out["host_path_host_ms"] / out["gpu_path_host_ms"], 1)
    out["zlib1_png_bytes"] = zlib1
    out["size_vs_host"] = round(out["device_png_bytes"] / out["host_png_bytes"], 3)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--render_meshes", action="store_true", help="also a mesh frame of the reconstructed fluid surface per state")
    ap.add_argument("--filter", default="adaptive")
    ap.add_argument("--coding", default="fixed", choices=["fixed", "dynamic", "window", "both", "all"],
                    help="both / all: every timed frame is encoded with a fixed and a dynamic (and a window) encoder in alternation")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    r = FrameRenderer(container.dx)
    filt = a.filter if a.filter == "adaptive" else int(a.filter)
    encoders = {c: PngEncoder(r.width, r.height, filter=filt, coding=c) for c in {"both": ("fixed", "dynamic"), "all": ("fixed", "dynamic", "window")}.get(a.coding, (a.coding,))}
    rm = recon = None
    if a.render_meshes:
        rm = FrameRenderer(container.dx, box=(np.zeros(3), np.asarray(container.domain_end, dtype=np.float64)))
        recon = SurfaceReconstructor(container.dx)
        recon.set_postprocess(mesh_smoothing_iters=25, mesh_smoothing_weights=True, weights_normalization=13.0, normals_smoothing_iters=10)
    lines = []

    def state(label, step):
        lines.extend(measure(r, encoders, lambda: r.from_container(container, download=False), a.frames, label, step, "particles"))
        if rm is not None:
            recon.from_container(container, 0)
            lines.extend(measure(rm, encoders, lambda: rm.from_meshes([(recon, (50, 100, 200))], download=False), a.frames, label, step, "meshes"))

    state("rest", 0)
    if a.motion_step > 0:
        container.engine.step(a.motion_step)
        container.engine.synchronize()
        state("in_motion", a.motion_step)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_png.py: medians over %d frames per state, times in ms (host clock where the name says host, else HIP events)\n" % a.frames)
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
