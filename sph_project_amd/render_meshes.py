#!/usr/bin/env python
"""Mesh frames from a directory of OBJ files, with the command line of the reference's render.py (:8-45):

    python sph_project_amd/render_meshes.py --input_dir scene_output --scene_file scene.json [--rendered_image_name render.png]

For every frame directory of --input_dir, every *.obj in it (particle_object_{id}.obj of --reconstruct, mesh_object_{id}.obj of exportObj)
is drawn in the colour its object id has in the scene file, with the domain box, into {frame}/{rendered_image_name} -- on the GPU by
FrameRenderer.from_meshes (Lambert-shaded triangles, not Blender's path tracer).  --scene_file is the simulation's JSON
(the reference passes a .blend scene, which this project cannot read); --num_workers and --device_type are accepted and ignored."""
import argparse
import json
import os
import re
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(_HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(_HERE))

import numpy as np  # noqa: E402


def read_obj(path):
    """(vertices f32[nv, 3], triangles i32[nt, 3], normals f32[nv, 3] or None) of an OBJ with `v`, `vn` and triangular `f a b c` /
    `f a//a b//b c//c` / `f a/t/n ...` records (1-based, or negative = from the end; polygons are fan-triangulated).  Numbers are
    parsed to the nearest f32, so a file written by sph_write_obj_ascii (shortest round-trip digits) comes back bit for bit.  Normals
    are returned when there is one `vn` per vertex and every corner names the normal of its own vertex (what that writer emits)."""
    v, vn, tri = [], [], []
    own = True
    with open(path) as fh:
        for line in fh:
            if line.startswith("v "):
                v.append(line.split()[1:4])
            elif line.startswith("vn "):
                vn.append(line.split()[1:4])
            elif line.startswith("f "):
                idx = []
                for tok in line.split()[1:]:
                    part = tok.split("/")
                    k = int(part[0])
                    k = k - 1 if k > 0 else len(v) + k
                    if len(part) == 3 and part[2]:
                        kn = int(part[2])
                        own = own and (kn - 1 if kn > 0 else len(vn) + kn) == k
                    else:
                        own = own and not vn
                    idx.append(k)
                for a in range(1, len(idx) - 1):
                    tri.append((idx[0], idx[a], idx[a + 1]))
    vert = np.array(v, dtype=np.float32).reshape(-1, 3)   # (via double: exact for shortest round-trip digits of an f32)
    nrm = np.array(vn, dtype=np.float32).reshape(-1, 3) if vn and own and len(vn) == len(v) else None
    return vert, np.array(tri, dtype=np.int32).reshape(-1, 3), nrm


def scene_colours(cfg):
    """object id -> (r, g, b) of every block and body of a scene JSON."""
    out = {}
    for key in ("FluidBlocks", "FluidBodies", "RigidBodies", "RigidBlocks"):
        for obj in cfg.get(key, []) or []:
            if "objectId" in obj and "color" in obj:
                out[int(obj["objectId"])] = tuple(int(c) for c in obj["color"])
    return out


def frame_meshes(frame_dir, colours, water=False):
    """The mesh list of one frame directory: its OBJ files in object-id order (the driver's order), each in its object's colour.
    water: particle_object_*.obj carry the water material of the traced frames (mesh_object_*.obj stay diffuse)."""
    items = []
    for name in os.listdir(frame_dir):
        m = re.fullmatch(r".*_object_(\d+)\.obj", name)
        if m:
            items.append((int(m.group(1)), name))
    out = []
    for oid, name in sorted(items):
        v, t, n = read_obj(os.path.join(frame_dir, name))
        item = (v, t, n, colours.get(oid, (255, 255, 255)))
        out.append(item + ("water",) if water and name.startswith("particle_object_") else item)
    return out


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--input_dir", type=str, required=True)
    parser.add_argument("--scene_file", type=str, required=True, help="the simulation's scene JSON (colours, domain box)")
    parser.add_argument("--rendered_image_name", type=str, default="render.png")
    parser.add_argument("--num_workers", type=int, default=1, help="ignored (one GPU draws a frame in milliseconds)")
    parser.add_argument("--device_type", type=str, default="HIP", help="ignored")
    parser.add_argument("--render_size", type=int, nargs=2, default=(1024, 1024), metavar=("W", "H"))
    parser.add_argument("--camera_position", type=float, nargs=3, default=(5.5, 2.5, 4.0))
    parser.add_argument("--camera_lookat", type=float, nargs=3, default=(-1.0, 0.0, 0.0))
    parser.add_argument("--camera_fov", type=float, default=70.0, help="vertical, degrees")
    parser.add_argument("--png_device", action="store_true",
                        help="compress the PNG files on the GPU from the device image (DESIGN.md 21), as run_simulation.py --png_device does")
    parser.add_argument("--png_coding", default=None, choices=["fixed", "dynamic", "window"],
                        help="with --png_device: fixed (the default), dynamic Huffman blocks or window matches, as run_simulation.py --png_coding")
    parser.add_argument("--raytrace", action="store_true",
                        help="trace the frames instead of rasterising them (DESIGN.md 30), as run_simulation.py --render_meshes --raytrace does")
    parser.add_argument("--trace_depth", type=int, default=None)
    parser.add_argument("--trace_ior", type=float, default=None)
    parser.add_argument("--trace_absorb", type=float, default=None)
    parser.add_argument("--trace_no_shadows", action="store_true")
    parser.add_argument("--trace_no_floor", action="store_true")
    args = parser.parse_args(argv)
    for flag in ("trace_depth", "trace_ior", "trace_absorb", "trace_no_shadows", "trace_no_floor"):
        if getattr(args, flag) not in (None, False) and not args.raytrace:
            parser.error(f"--{flag} sets a parameter of the traced frames: give --raytrace as well")
    if args.png_coding is not None and not args.png_device:
        parser.error("--png_coding chooses the device encoder's code: give --png_device as well")
    args.png_coding = args.png_coding or "fixed"
    return args


def main(argv=None):
    args = parse_args(argv)
    from sph_project_amd.render import FrameRenderer, store_png
    with open(args.scene_file) as fh:
        cfg = json.load(fh)
    colours = scene_colours(cfg)
    dom = np.asarray(cfg["Configuration"]["domainEnd"], dtype=np.float64)
    renderer = FrameRenderer(float(cfg["Configuration"].get("particleRadius", 0.01)), width=args.render_size[0], height=args.render_size[1],
                             camera_position=args.camera_position, camera_lookat=args.camera_lookat, fov=args.camera_fov,
                             box=(np.zeros(3), dom))
    if args.raytrace:
        chosen = dict(max_depth=args.trace_depth, ior=args.trace_ior, absorb=args.trace_absorb)
        renderer.set_trace(shadows=not args.trace_no_shadows, floor=not args.trace_no_floor, **{k: v for k, v in chosen.items() if v is not None})
    encoder = None
    if args.png_device:
        from sph_project_amd.png import PngEncoder
        encoder = PngEncoder(renderer.width, renderer.height, coding=args.png_coding)
    done = 0
    for frame in sorted(os.listdir(args.input_dir)):
        d = os.path.join(args.input_dir, frame)
        if not os.path.isdir(d):
            continue
        meshes = frame_meshes(d, colours, water=args.raytrace)
        if not meshes:
            continue
        store_png(os.path.join(d, args.rendered_image_name), renderer, lambda dl: renderer.from_meshes(meshes, download=dl), encoder)
        done += 1
    print(f"Rendered {done} frame(s) of {args.input_dir}")
    return done


if __name__ == "__main__":
    main()
