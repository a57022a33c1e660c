"""ms per frame of the video encoder on C2 (product.c2_scene(), 1.23 M particles) at the reference's camera and 1024^2,
strict build, from rest and again after the in-motion steps of the bench line (2500).  Per state: one untimed frame, then --frames
timed frames.  Per frame: the render (HIP events), the GPU encode by stage (HIP events) and around the call (host clock), the
compressed size, and the download of those bytes (host clock around sph_video_size + sph_video_download).  Beside them, in the same
run, what storing the same frame costs without the encoder: the raw download of the frame (sph_render_download) plus encode_png on the
host.  One JSON line per state; with --out also written to that file (profiles/video_bench_c2.txt)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.render import FrameRenderer, encode_png  # noqa: E402
from sph_project_amd.video import VideoEncoder  # noqa: E402


def _ms(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def measure(r, v, container, frames, label, step):
    r.from_container(container)   # untimed: allocations, first touch
    v.encode_last(r)
    rows = []
    for _ in range(frames):
        container.engine.synchronize()
        r.from_container(container)
        render = r.stats()
        enc_host, _ = _ms(lambda: v._chk(v.lib.sph_video_encode_render(v.h, r._last), "sph_video_encode_render"))
        st = v.stats()
        dl_host, jpg = _ms(v._download)
        raw_host, rgb = _ms(r.last_rgb)
        png_host, png = _ms(lambda: encode_png(rgb))
        rows.append(dict(render_ms=render["ms_total"], encode_ms=st["ms_total"], count_ms=st["ms_count"], scan_ms=st["ms_scan"],
                         write_ms=st["ms_write"], encode_host_ms=enc_host, jpeg_download_host_ms=dl_host, jpeg_bytes=len(jpg),
                         raw_download_host_ms=raw_host, png_encode_host_ms=png_host, png_bytes=len(png),
                         scan_bytes=st["scan_bytes"], stuffed_bytes=st["stuffed_bytes"], restart_intervals=st["restart_intervals"]))
    med = lambda key: round(float(np.median([row[key] for row in rows])), 3)  # noqa: E731
    out = dict(state=label, step=step, frames=frames, width=r.width, height=r.height, quality=v.quality, chroma=v.chroma,
               particles=int(container.particle_num[None]))
    out.update({k: med(k) for k in rows[0] if k.endswith("_ms")})
    out.update({k: rows[0][k] for k in rows[0] if not k.endswith("_ms")})
    out["gpu_path_ms"] = round(out["encode_host_ms"] + out["jpeg_download_host_ms"], 3)       # after the render: encode + fetch the file
    out["host_path_ms"] = round(out["raw_download_host_ms"] + out["png_encode_host_ms"], 3)   # after the render: fetch the pixels + PNG
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--chroma", default="420")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    r = FrameRenderer(container.dx)
    v = VideoEncoder(r.width, r.height, quality=a.quality, chroma=a.chroma)
    lines = [measure(r, v, container, a.frames, "rest", 0)]
    if a.motion_step > 0:
        container.engine.step(a.motion_step)
        container.engine.synchronize()
        lines.append(measure(r, v, container, a.frames, "in_motion", a.motion_step))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_video.py: medians over %d frames per state, times in ms (host clock where the name says host, else HIP events)\n" % a.frames)
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
