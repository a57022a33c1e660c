"""ms per frame of the particle renderer on C2 (product.c2_scene(), 1.23 M particles) at the reference's camera and
1024^2, from rest and again after the in-motion steps of the bench line (bench.py --motion-step, 2500).  Per state: one untimed frame,
then --frames timed frames, each from the live handle (sph_render_handle, synchronous).  Reports the stage times from HIP events, the
host clock around the call, drawn particles, covered pixels, the 64-bit atomics issued (per drawn particle and per covered pixel), and the
PNG encode of the frame (stdlib zlib, on the host) measured apart.  One JSON line per state."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sph_project_amd import product as P  # noqa: E402
from sph_project_amd.render import FrameRenderer, encode_png  # noqa: E402


def measure(r, container, frames, label, step):
    eng = container.engine
    rgb = r.from_container(container)   # untimed: allocations, first touch
    h = r._last
    mask = C.c_uint32(sum(1 << o for o in range(len(container.object_visibility)) if container.object_visibility[o] == 1))
    host, stats = [], []
    for _ in range(frames):
        eng.synchronize()
        t0 = time.perf_counter()
        rc = r.lib.sph_render_handle(h, eng.h, mask)
        host.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0, rc
        stats.append(r.stats())
    t0 = time.perf_counter()
    png = encode_png(rgb)
    png_ms = 1e3 * (time.perf_counter() - t0)
    best = min(range(frames), key=lambda k: stats[k]["ms_total"])
    st = stats[best]
    med = lambda key: round(sorted(s[key] for s in stats)[frames // 2], 3)  # noqa: E731
    out = dict(state=label, step=step, particles=st["particles"], drawn=st["drawn"], frames=frames, width=r.width, height=r.height,
               ms_per_frame_events=round(st["ms_total"], 3), ms_per_frame_events_median=med("ms_total"),
               ms_per_frame_host=round(min(host), 3), ms_per_frame_host_median=round(sorted(host)[frames // 2], 3),
               ms_input=round(st["ms_input"], 3), ms_splat=round(st["ms_splat"], 3), ms_splat_median=med("ms_splat"),
               ms_shade=round(st["ms_shade"], 3), large=st["large"], skipped_nonfinite=st["skipped_nonfinite"],
               covered_pixels=st["covered_pixels"], atomics=st["atomics"],
               atomics_per_drawn=round(st["atomics"] / max(st["drawn"], 1), 3),
               atomics_per_covered_pixel=round(st["atomics"] / max(st["covered_pixels"], 1), 3),
               png_encode_ms=round(png_ms, 1), png_bytes=len(png),
               atomics_min=min(s["atomics"] for s in stats), atomics_max=max(s["atomics"] for s in stats),
               identical_covered=all(s["covered_pixels"] == st["covered_pixels"] for s in stats))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--motion-step", type=int, default=2500, help="0: from rest only")
    ap.add_argument("--fast-math", action="store_true")
    a = ap.parse_args()
    container, solver = P.build_product(P.c2_scene())
    solver.prepare()
    r = FrameRenderer(container.dx, fast_math=a.fast_math)
    measure(r, container, a.frames, "rest", 0)
    if a.motion_step > 0:
        container.engine.step(a.motion_step)
        container.engine.synchronize()
        measure(r, container, a.frames, "in_motion", a.motion_step)


if __name__ == "__main__":
    main()
