#!/usr/bin/env python
"""GGUI-free driver with the command line, loop arithmetic and on-disk outputs of the reference's
run_simulation.py (:13-44 argument + interval arithmetic, :116-155 loop, :137-144 PLY export).

    python sph_project_amd/run_simulation.py --scene_file data/scenes/high_fluid_wcsph.json [--max_steps N]

Frames go to {scene_name}_output/{cnt:06}/particle_object_{id}.ply (ASCII PLY, x y z per vertex -- the
layout Taichi's PLYWriter.export_ascii produces and surface_reconstruction.py / splashsurf consume).
Rigid bodies: mesh_object_{id}.obj per frame with exportObj (:146-150).  PNG frames (exportFrame, :131-134) come from the GPU
renderer of render.py with --render (its own image, not GGUI's: DESIGN.md 15); without --render none is written.  --render_meshes
writes {cnt:06}/render.png, the frame's meshes drawn on the GPU, where the reference's render.py needs Blender.  --video
adds {out}/raw_view.avi / {out}/render.avi, the same frames as Motion-JPEG compressed on the GPU (make_video.py).
--render_surface writes {cnt:06}/surface_view.png: the particle frame with the fluid drawn as a smoothed, lit surface in screen space
(DESIGN.md 24), at the cost of a particle frame where --render_meshes pays for a reconstruction.  --surface_thickness makes that
surface translucent: the fluid's thickness along every ray lets rigid bodies and the box show through.
--foam --render_surface --surface_foam draws the diffuse particles into surface_view.png as white water, over the surface and, with
--surface_thickness, under it.
--png_device writes the PNG files from the device image as well: no pixel is downloaded, no zlib runs on the host;
--png_coding dynamic makes those files smaller (dynamic Huffman blocks) for a slower encode, --png_coding window smaller again (matches from
the 32 KB before a position).
--gpus N shards the scene over N ranks (z-slabs, one process each, started by launch.py): the frames are composited over the ranks
 and written by rank 0, the PLY of a fluid object is written in rank order, one part per rank."""
import argparse
import math
import os
import sys
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)  # makes `import SPH` resolve to sph_project_amd/SPH (drop-in)

import numpy as np  # noqa: E402
from SPH.utils import SimConfig  # noqa: E402
from SPH.containers import DFSPHContainer, WCSPHContainer, PCISPHContainer, IISPHContainer, PBFContainer  # noqa: E402
from SPH.fluid_solvers import DFSPHSolver, WCSPHSolver, PCISPHSolver, IISPHSolver, PBFSolver  # noqa: E402


PLY_COMMENT = "created by PLYWriter"   # taichi.tools.PLYWriter's default `comment`


def write_ply_ascii(path, pos):
    """What `PLYWriter(num_vertices=n); add_vertex_pos(x, y, z); export_ascii(path)` leaves on disk (run_simulation.py:139-144).
    Layout restated from Taichi's python/taichi/tools/ply.py (>= 1.6; the package is absent here, so the layout is NOT compared with
    a Taichi run): `print_header` writes "ply", "format ascii 1.0", "comment created by PLYWriter", "element vertex N", one
    "property float x|y|z" line per channel (`add_vertex_pos` registers the three channels as "float" and casts the data to
    np.float32) and "end_header"; `export_ascii` then appends one line per vertex, every value as `str(np.float32)` -- the shortest
    digits that round-trip -- FOLLOWED by a blank, i.e. "x y z \n".  `ndarray.astype(str)` produces exactly those strings."""
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    if not os.environ.get("SPH_PLY_PYTHON"):
        # the same bytes from C++ behind the C-ABI (csrc/sph_export.hpp): 0.2 s instead of ~5 s for the 1.23 M particles of a frame
        from sph_project_amd import _lib
        rc = _lib.load().sph_write_ply_ascii(os.fsencode(path), pos.ctypes.data, pos.shape[0])
        if rc != 0:
            raise OSError(f"sph_write_ply_ascii({path!r}) failed ({rc})")
        return
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\ncomment {PLY_COMMENT}\n")
        f.write(f"element vertex {pos.shape[0]}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        if pos.shape[0]:
            f.write(" \n".join(map(" ".join, pos.astype(str).tolist())) + " \n")


def write_ply_ascii_part(path, pos, n_total, first):
    """One part of the file write_ply_ascii makes of the concatenated parts: first truncates and writes the header for n_total
    vertices, then (either way) this part's rows are appended."""
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    if not os.environ.get("SPH_PLY_PYTHON"):
        from sph_project_amd import _lib
        rc = _lib.load().sph_write_ply_ascii_part(os.fsencode(path), pos.ctypes.data, pos.shape[0], int(n_total), int(bool(first)))
        if rc != 0:
            raise OSError(f"sph_write_ply_ascii_part({path!r}) failed ({rc})")
        return
    with open(path, "w" if first else "a") as f:
        if first:
            f.write(f"ply\nformat ascii 1.0\ncomment {PLY_COMMENT}\n")
            f.write(f"element vertex {int(n_total)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        if pos.shape[0]:
            f.write(" \n".join(map(" ".join, pos.astype(str).tolist())) + " \n")


def read_ply_ascii(path):
    """Vertex positions of an ASCII PLY as (n, 3) float32 (what surface_reconstruction.py / splashsurf read back)."""
    with open(path) as f:
        assert f.readline().strip() == "ply"
        n, props = None, []
        for line in f:
            tok = line.split()
            if tok[:2] == ["element", "vertex"]:
                n = int(tok[2])
            elif tok[:1] == ["property"]:
                props.append(tok[-1])
            elif tok[:1] == ["end_header"]:
                break
        data = np.loadtxt(f, dtype=np.float32, ndmin=2) if n else np.zeros((0, len(props)), np.float32)
    assert data.shape == (n, len(props)), (data.shape, n, props)
    return data[:, [props.index(k) for k in ("x", "y", "z")]]


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--scene_file", default="", help="scene file")
    parser.add_argument("--max_steps", type=int, default=None, help="stop early (not in the reference)")
    parser.add_argument("--output_dir", default=None, help="default: {scene_name}_output in the cwd (reference behaviour)")
    parser.add_argument("--rigid_backend", default=None, choices=["native", "contact", "device", "device_contact", "pybullet"],
                        help="rigid-body backend (default: SPH_RIGID_BACKEND, else native); 'contact' adds body-body contact, "
                             "'device' runs the native integrator on the GPU, 'device_contact' the contact solve as well")
    parser.add_argument("--reconstruct", action="store_true",
                        help="with every PLY frame also write particle_object_{id}.obj: the fluid object's surface, reconstructed on the "
                             "GPU from the device state (surface_reconstruction.py's defaults; not in the reference)")
    parser.add_argument("--mesh_smoothing_iters", type=int, default=0, help="with --reconstruct: Laplacian smoothing iterations (DESIGN.md 16)")
    parser.add_argument("--mesh_smoothing_weights", action="store_true", help="with --reconstruct: keep isolated particles' meshes unsmoothed")
    parser.add_argument("--normals_smoothing_iters", type=int, default=0, help="with --reconstruct: normal smoothing iterations")
    parser.add_argument("--anisotropic", action="store_true",
                        help="with --reconstruct / --render_meshes: anisotropic kernels (DESIGN.md 29) -- thin sheets, rims and droplets "
                             "are meshed about one particle radius outside their outermost centres where the isotropic kernel adds two")
    parser.add_argument("--aniso_ratio", type=float, default=None, help="with --anisotropic: the most a kernel shrinks along a direction, >= 1 (2)")
    parser.add_argument("--aniso_min_neighbours", type=int, default=None,
                        help="with --anisotropic: below this many neighbours a particle gets the isolated rule (25)")
    parser.add_argument("--aniso_sparse_scale", type=float, default=None,
                        help="with --anisotropic: the isolated rule's support in multiples of h, in (0, 1] (0.5)")
    parser.add_argument("--render", action="store_true",
                        help="on scenes with exportFrame write {out}/{cnt:06}/raw_view.png at the reference's cadence, rendered on the GPU "
                             "from the device state (DESIGN.md 15; not GGUI's image)")
    parser.add_argument("--render_meshes", action="store_true",
                        help="at every output frame write {out}/{cnt:06}/render.png (render.py's default --rendered_image_name): the visible "
                             "fluid objects reconstructed with the --reconstruct settings, the visible rigid bodies' meshes at their current "
                             "pose and the domain box, drawn on the GPU (DESIGN.md 17; not Blender's image)")
    parser.add_argument("--render_surface", action="store_true",
                        help="at every output frame write {out}/{cnt:06}/surface_view.png: the particle frame of raw_view.png with the "
                             "visible fluid objects drawn as a surface -- sphere depths smoothed in screen space, normals off the smoothed "
                             "depth, Lambert and a highlight (DESIGN.md 24; no mesh is reconstructed); needs --gpus 1")
    parser.add_argument("--surface_iters", type=int, default=None, help="with --render_surface: smoothing iterations, 0..64 (3)")
    parser.add_argument("--surface_sigma", type=float, default=None, help="with --render_surface: smoothing half-width in particle radii (1.5)")
    parser.add_argument("--surface_range", type=float, default=None, help="with --render_surface: depth range of a tap in particle radii (2.0)")
    parser.add_argument("--surface_thickness", action="store_true",
                        help="with --render_surface: draw the surface translucent -- the fluid's thickness along every pixel's ray, summed "
                             "from the particles, lets what lies behind (rigid bodies, the box) show through (DESIGN.md 25)")
    parser.add_argument("--raytrace", action="store_true",
                        help="with --render_meshes: trace the mesh frames instead of rasterising them (DESIGN.md 30) -- hard shadows, the "
                             "fluid as refracting, absorbing water, the bottom of the domain box as a checkered floor")
    parser.add_argument("--trace_depth", type=int, default=None, help="with --raytrace: segments of a path (default 6)")
    parser.add_argument("--trace_ior", type=float, default=None, help="with --raytrace: the fluid's index of refraction (default 1.33)")
    parser.add_argument("--trace_absorb", type=float, default=None,
                        help="with --raytrace: absorption per particle radius of path in the fluid, tinted by the fluid's colour (default 0.05)")
    parser.add_argument("--trace_no_shadows", action="store_true", help="with --raytrace: no shadow rays")
    parser.add_argument("--trace_no_floor", action="store_true", help="with --raytrace: no floor")
    parser.add_argument("--surface_absorb", type=float, default=None,
                        help="with --surface_thickness: absorption per particle radius of fluid, scaled by 1 - base colour (0.05)")
    parser.add_argument("--surface_scatter", type=float, default=None,
                        help="with --surface_thickness: scattering per particle radius of fluid, every channel alike (0.01)")
    parser.add_argument("--surface_thickness_iters", type=int, default=None,
                        help="with --surface_thickness: smoothing iterations of the thickness plane, 0..64 (2)")
    parser.add_argument("--render_size", type=int, nargs=2, default=(1024, 1024), metavar=("W", "H"))
    parser.add_argument("--camera_position", type=float, nargs=3, default=(5.5, 2.5, 4.0))
    parser.add_argument("--camera_lookat", type=float, nargs=3, default=(-1.0, 0.0, 0.0))
    parser.add_argument("--camera_fov", type=float, default=70.0, help="vertical, degrees")
    parser.add_argument("--video", action="store_true",
                        help="with --render also write {out}/raw_view.avi, with --render_meshes {out}/render.avi: one Motion-JPEG frame per "
                             "output frame, compressed on the GPU from the device image the PNG is written from (DESIGN.md 18; what "
                             "make_video.py makes of the directory afterwards)")
    parser.add_argument("--video_fps", type=int, default=20, help="make_video.py's --fps")
    parser.add_argument("--video_quality", type=int, default=90, help="JPEG quality 1..100")
    parser.add_argument("--video_chroma", default="420", choices=["420", "444"])
    parser.add_argument("--png_device", action="store_true",
                        help="compress raw_view.png / render.png on the GPU from the renderer's device image (DESIGN.md 21: lossless, the "
                             "same pixels, other bytes than the host's zlib) where the default downloads the frame and runs zlib on it")
    parser.add_argument("--png_coding", default=None, choices=["fixed", "dynamic", "window"],
                        help="with --png_device: the entropy coding of the files (DESIGN.md 21).  fixed (the default): the fixed Huffman "
                             "code; dynamic: per segment a dynamic Huffman block where it is shorter -- smaller files, a slower encode; window: "
                             "also matches from the 32 KB before a position -- smaller files again, a slower encode again")
    parser.add_argument("--export_device", action="store_true",
                        help="format particle_object_{id}.ply (and with --reconstruct particle_object_{id}.obj) on the GPU from the device "
                             "state (DESIGN.md 23: the same bytes as the host writers, no position or mesh download); needs a scene with "
                             "exportPly and --gpus 1")
    parser.add_argument("--foam", action="store_true",
                        help="generate diffuse particles -- spray, foam and bubbles -- from the fluid on the GPU (DESIGN.md 26): "
                             "{frame}/diffuse_particles.ply at every output frame, and with --render drawn into raw_view.png; the "
                             "fluid is not affected.  Parameters: the scene's optional Configuration.foam dict")
    parser.add_argument("--surface_foam", action="store_true",
                        help="with --foam and --render_surface: draw the diffuse particles into surface_view.png as white water -- the "
                             "summed chords of their spheres along every pixel's ray, over the surface and, with --surface_thickness, "
                             "under it, dimmed by the water in front (DESIGN.md 28); with --render raw_view.png shows them as spheres")
    parser.add_argument("--surface_foam_density", type=float, default=None,
                        help="with --surface_foam: whiteness per particle radius of diffuse chord (1.0)")
    parser.add_argument("--surface_foam_bias", type=float, default=None,
                        help="with --surface_foam: particle radii behind the surface from which a diffuse particle counts as under it (1.0)")
    parser.add_argument("--foam_every", type=int, default=None,
                        help="simulation steps per diffuse-particle step, default 4 (its dt is that many time steps)")
    parser.add_argument("--foam_max", type=int, default=None,
                        help="capacity of the diffuse set, default twice the scene's particle capacity")
    parser.add_argument("--gpus", type=int, default=1,
                        help="shard the scene over this many ranks, one process and (unless SPH_COMM_TRANSPORT names a shared-memory "
                             "transport) one GPU each; frames are composited on rank 0 (DESIGN.md 22)")
    args = parser.parse_args(argv)
    if args.gpus < 1:
        parser.error(f"--gpus {args.gpus}: at least one rank is needed")
    for flag in ("foam_every", "foam_max"):
        if getattr(args, flag) is not None and not args.foam:
            parser.error(f"--{flag} sets a parameter of the diffuse particles: give --foam as well")
    if args.surface_foam and not args.foam:
        parser.error("--surface_foam draws the diffuse particles into the surface frames: give --foam as well")
    if args.surface_foam and not args.render_surface:
        parser.error("--surface_foam draws the diffuse particles into the surface frames: give --render_surface as well")
    for flag in ("surface_foam_density", "surface_foam_bias"):
        if getattr(args, flag) is not None and not args.surface_foam:
            parser.error(f"--{flag} sets a parameter of the diffuse particles in the surface frames: give --surface_foam as well")
    if args.foam:
        if args.gpus > 1:
            parser.error(f"--gpus {args.gpus}: --foam reads the whole fluid on one device (sharded scenes are not supported); run it "
                         "with --gpus 1")
        if args.render_surface and not args.surface_foam:
            parser.error("--foam draws the diffuse particles into particle frames only: not with --render_surface (DESIGN.md 26) "
                         "unless --surface_foam draws them into the surface frames")
        if args.foam_every is not None and args.foam_every < 1:
            parser.error(f"--foam_every {args.foam_every}: at least one simulation step per diffuse-particle step")
        if args.foam_max is not None and args.foam_max < 1:
            parser.error(f"--foam_max {args.foam_max}: room for at least one diffuse particle")
    args.foam_every = args.foam_every or 4
    if args.export_device:
        if args.gpus > 1:
            parser.error(f"--gpus {args.gpus}: --export_device formats one device's particles (a sharded scene writes each rank's part "
                         "on the host); run it with --gpus 1")
        if not SimConfig(scene_file_path=args.scene_file).get_cfg("exportPly"):
            parser.error("--export_device formats the PLY frames of a scene with exportPly; this scene exports none")
    if args.anisotropic and not (args.reconstruct or args.render_meshes):
        parser.error("--anisotropic chooses the kernels of the surface reconstruction: give --reconstruct and / or --render_meshes as well")
    for flag in ("aniso_ratio", "aniso_min_neighbours", "aniso_sparse_scale"):
        if getattr(args, flag) is not None and not args.anisotropic:
            parser.error(f"--{flag} sets a parameter of the anisotropic kernels: give --anisotropic as well")
    if args.anisotropic:
        why = anisotropy_error(args.aniso_ratio, args.aniso_min_neighbours, args.aniso_sparse_scale)
        if why:
            parser.error(why)
    if args.render_surface and args.gpus > 1:
        parser.error(f"--gpus {args.gpus}: --render_surface needs the base colour and surface flag of every pixel, which the layers "
                     "composited between ranks do not carry (DESIGN.md 24); run it with --gpus 1")
    for flag in ("surface_iters", "surface_sigma", "surface_range"):
        if getattr(args, flag) is not None and not args.render_surface:
            parser.error(f"--{flag} sets a parameter of the surface frames: give --render_surface as well")
    if args.surface_thickness and not args.render_surface:
        parser.error("--surface_thickness makes the surface frames translucent: give --render_surface as well")
    for flag in ("surface_absorb", "surface_scatter", "surface_thickness_iters"):
        if getattr(args, flag) is not None and not args.surface_thickness:
            parser.error(f"--{flag} sets a parameter of the thickness mode: give --surface_thickness as well")
    if args.gpus > 1:
        check_sharded_args(parser, args)
    if args.raytrace and not args.render_meshes:
        parser.error("--raytrace traces the mesh frames: give --render_meshes as well")
    for flag in ("trace_depth", "trace_ior", "trace_absorb", "trace_no_shadows", "trace_no_floor"):
        if getattr(args, flag) not in (None, False) and not args.raytrace:
            parser.error(f"--{flag} sets a parameter of the traced mesh frames: give --raytrace as well")
    if args.png_device and not (args.render or args.render_meshes or args.render_surface):
        parser.error("--png_device compresses a renderer's frames: give --render, --render_meshes and / or --render_surface as well")
    if args.png_coding is not None and not args.png_device:
        parser.error("--png_coding chooses the device encoder's code: give --png_device as well")
    args.png_coding = args.png_coding or "fixed"
    if args.video and not (args.render or args.render_meshes or args.render_surface):
        parser.error("--video takes its frames from a renderer: give --render, --render_meshes and / or --render_surface as well")
    return args


def check_sharded_args(parser, args):
    """What --gpus N > 1 cannot do, said before any rank is started (no GPU is opened here)."""
    n = args.gpus
    if args.reconstruct or args.render_meshes:
        parser.error(f"--gpus {n}: --reconstruct / --render_meshes need the whole fluid on one device (surface reconstruction of a "
                     "sharded scene is not supported); run them with --gpus 1")
    backend = args.rigid_backend or os.environ.get("SPH_RIGID_BACKEND") or "native"
    if backend in ("device", "device_contact", "pybullet"):
        parser.error(f"--gpus {n}: --rigid_backend {backend} integrates the bodies from one device's particles; sharded scenes run the "
                     "native or contact backend")
    config = SimConfig(scene_file_path=args.scene_file)
    method = config.get_cfg("simulationMethod")
    if method in ("iisph", "pbf"):
        parser.error(f"--gpus {n}: the {method} solver is not sharded (sph_prepare refuses it on a slab); run it with --gpus 1")
    if config.get_cfg("surfaceTensionMethod") == "akinci":
        parser.error(f"--gpus {n}: surfaceTensionMethod \"akinci\" is not sharded (the normals of the ghost particles would need an "
                     "exchange of their own; sph_set_surface_tension refuses a slab); run it with --gpus 1")
    if config.get_cfg("vorticityMethod") == "micropolar":
        parser.error(f"--gpus {n}: vorticityMethod \"micropolar\" is not sharded (the angular velocities of the ghost particles would "
                     "need an exchange of their own; sph_set_micropolar refuses a slab); run it with --gpus 1")
    if config.get_cfg("dragMethod") == "gissler":
        parser.error(f"--gpus {n}: dragMethod \"gissler\" is not sharded (not done, although the walk would need the ghosts' positions "
                     "only; sph_set_drag refuses a slab); run it with --gpus 1")
    if config.get_cfg("thermalMethod") == "conduction":
        parser.error(f"--gpus {n}: thermalMethod \"conduction\" is not sharded (the temperatures of the ghost particles would need an "
                     "exchange of their own; sph_set_thermal refuses a slab); run it with --gpus 1")
    elastic = [e.get("objectId") for e in list(config.get_fluid_blocks()) + list(config.get_fluid_bodies()) if e.get("elasticity") is not None]
    if elastic:
        parser.error(f"--gpus {n}: object {elastic[0]} carries the key \"elasticity\": elastic solids are not sharded (a rest list names "
                     "particles by id across every slab; sph_set_elastic_object refuses a slab); run it with --gpus 1")
    if config.get_emitters():
        parser.error(f"--gpus {n}: the scene has Emitters: fluid emitters are not sharded (their schedule knows one particle count; "
                     "sph_set_emitter refuses a slab); run it with --gpus 1")
    if config.get_outflows():
        parser.error(f"--gpus {n}: the scene has Outflows: outflow volumes are not sharded (a slab rank's graveyard cells are its halo "
                     "exchange's; sph_set_outflow refuses a slab); run it with --gpus 1")
    if config.get_cfg("cflMethod") in ("velocity", 1):
        parser.error(f"--gpus {n}: cflMethod \"velocity\" is not sharded (every rank would need the same largest speed at every step; "
                     "sph_set_cfl refuses a slab); run it with --gpus 1")
    from sph_project_amd import launch
    try:
        launch.plan_scene_cuts(config.config, n)
    except ValueError as e:
        parser.error(f"--gpus {n}: {e}")


def anisotropy_error(ratio, min_neighbours, sparse_scale):
    """Why sph_surface_set_anisotropy would refuse these values (None: not given), or None: said before a GPU is opened."""
    if ratio is not None and not (math.isfinite(ratio) and ratio >= 1.0):
        return f"--aniso_ratio {ratio}: a finite ratio of at least 1"
    if min_neighbours is not None and min_neighbours < 0:
        return f"--aniso_min_neighbours {min_neighbours}: not negative"
    if sparse_scale is not None and not (math.isfinite(sparse_scale) and 0.0 < sparse_scale <= 1.0):
        return f"--aniso_sparse_scale {sparse_scale}: in (0, 1]"
    return None


def surface_anisotropy(args):
    """set_anisotropy keywords of the --aniso_* flags that were given (the others keep the library's defaults)."""
    chosen = dict(max_ratio=args.aniso_ratio, min_neighbours=args.aniso_min_neighbours, sparse_scale=args.aniso_sparse_scale)
    return {k: v for k, v in chosen.items() if v is not None}


def surface_postprocess(args):
    """set_postprocess keywords of the smoothing flags (normalization 13), or None when none of them is set."""
    if not (args.mesh_smoothing_iters or args.mesh_smoothing_weights or args.normals_smoothing_iters):
        return None
    return dict(mesh_smoothing_iters=args.mesh_smoothing_iters, mesh_smoothing_weights=bool(args.mesh_smoothing_weights),
                weights_normalization=13.0, normals_smoothing_iters=args.normals_smoothing_iters)


def trace_keywords(args):
    """set_trace keywords of the --trace_* flags (the renderer's defaults where a flag is not given)."""
    chosen = dict(max_depth=args.trace_depth, ior=args.trace_ior, absorb=args.trace_absorb)
    kw = {k: v for k, v in chosen.items() if v is not None}
    kw.update(shadows=not args.trace_no_shadows, floor=not args.trace_no_floor)
    return kw


def frame_meshes(container, solver, recon, reconstructed=(), water=False):
    """The mesh list of one render.png, in object-id order: every visible fluid object reconstructed in situ (the list item is the
    reconstructor itself: FrameRenderer.from_meshes copies its mesh on the device before the generator reconstructs the next object;
    `reconstructed` names the object whose mesh the reconstructor holds on entry, valid until the first reconstruction here), every visible rigid body's mesh at its current pose, flat
    shaded, each in its scene colour.  water: the fluid meshes carry the material of the traced frames."""
    for oid in sorted(container.object_id_fluid_body | container.object_id_rigid_body):
        if container.object_visibility[oid] != 1:
            continue
        colour = tuple(int(c) for c in container.object_collection[oid]["color"])
        if oid in container.object_id_fluid_body:
            if oid not in reconstructed:
                recon.from_container(container, oid)
                reconstructed = ()   # the reconstructor holds this object's mesh now, no longer the one it was handed with
            yield (recon, colour, "water") if water else (recon, colour)
        else:
            posed = solver.posed_mesh_vertices(oid)
            if posed is not None:
                yield (posed, np.asarray(container.object_collection[oid]["mesh"].faces), None, colour)


METHODS = {"dfsph": (DFSPHContainer, DFSPHSolver), "wcsph": (WCSPHContainer, WCSPHSolver), "pcisph": (PCISPHContainer, PCISPHSolver),
           "iisph": (IISPHContainer, IISPHSolver), "pbf": (PBFContainer, PBFSolver)}


class Schedule:
    """The reference's interval arithmetic (run_simulation.py:13-44) over a scene's configuration: a frame at every step count that is a
    multiple of output_interval, `limit` steps in all (--max_steps stops early), what a frame holds and where the frames go."""

    def __init__(self, config, args):
        fps = config.get_cfg("fps")
        if fps is None:
            fps = 60
        frame_time = 1.0 / fps
        self.output_interval = int(frame_time / config.get_cfg("timeStepSize"))
        total_time = config.get_cfg("totalTime")
        if total_time is None:
            total_time = 10.0
        total_rounds = int(total_time / config.get_cfg("timeStepSize"))
        if config.get_cfg("outputInterval"):
            self.output_interval = config.get_cfg("outputInterval")
        self.limit = total_rounds if args.max_steps is None else min(total_rounds, args.max_steps)
        self.limit = max(self.limit, 1)   # the reference's loop steps once before it looks at the round count
        self.time_step, self.total_time = float(config.get_cfg("timeStepSize")), float(total_time)   # (run_loop_timed goes by scene time)
        self.output_ply = config.get_cfg("exportPly")
        self.output_obj = config.get_cfg("exportObj")
        self.output_frames = config.get_cfg("exportFrame") and args.render
        scene_name = args.scene_file.split("/")[-1].split(".")[0]
        self.out_dir = args.output_dir or f"{scene_name}_output"


def frame_dir(out_dir, cnt):
    """{out_dir}/{cnt:06}, there from the first time a frame asks for it."""
    d = f"{out_dir}/{cnt:06}"
    os.makedirs(d, exist_ok=True)
    return d


def run_loop(solver, engine, sched, wants_frame, write_frame, avi_writers=()):
    """run_simulation.py:126-153 steps once, writes a frame if the count of steps BEFORE this one is a multiple of the interval, then
    counts.  Same frames here -- write_frame(cnt) writes one and returns whether anything was written -- but the steps between two frames
    go to the device in one call.  Returns the step count, the seconds spent in write_frame and the number of frames written; an
    exception still leaves well-formed videos of the frames written so far."""
    cnt, limit, interval = 0, sched.limit, sched.output_interval
    t_export, frames = 0.0, 0
    try:
        while cnt < limit:
            nxt = cnt if cnt % interval == 0 else cnt + interval - cnt % interval   # next count that gets a frame
            if not wants_frame or nxt >= limit:
                solver.advance(limit - cnt)
                cnt = limit
                break
            solver.advance(nxt - cnt + 1)
            cnt = nxt
            engine.synchronize()
            te = time.perf_counter()
            frames += 1 if write_frame(cnt) else 0
            t_export += time.perf_counter() - te
            cnt += 1
        engine.synchronize()
    finally:
        for writer in avi_writers:
            writer.close()
    return cnt, t_export, frames


def run_loop_timed(solver, engine, sched, wants_frame, write_frame, avi_writers=(), max_steps=None):
    """run_loop for a scene with adaptive time stepping (Configuration.cflMethod "velocity"): the loop goes by scene time.
    Frames fall at the instants j * output_interval * timeStepSize, j = 0, 1, ... -- where the fixed-step run writes them --, each frame
    interval is one solver.advance_to, and the run ends at totalTime (sched.total_time) or after max_steps steps.  write_frame gets
    the frame's index j * output_interval, the step count the fixed-step run would name it by.  Returns the steps taken, the seconds spent
    in write_frame and the number of frames written."""
    t_frame = sched.output_interval * sched.time_step
    t_end = sched.total_time
    budget = None if max_steps is None else max(int(max_steps), 1)   # (run_loop steps once before it looks, too)
    cnt, t_export, frames, j = 0, 0.0, 0, 0
    try:
        while budget is None or cnt < budget:   # (like run_loop, no frame at the count the run ends with)
            t_j = j * t_frame
            if not wants_frame or t_j >= t_end:
                cnt += solver.advance_to(t_end, max_steps=None if budget is None else budget - cnt)
                break
            if j > 0:
                cnt += solver.advance_to(t_j, max_steps=None if budget is None else budget - cnt)
                if budget is not None and cnt >= budget:
                    break
            engine.synchronize()
            te = time.perf_counter()
            frames += 1 if write_frame(j * sched.output_interval) else 0
            t_export += time.perf_counter() - te
            j += 1
        engine.synchronize()
    finally:
        for writer in avi_writers:
            writer.close()
    return cnt, t_export, frames


def report(cnt, particles, t0, t_export, frames):
    # frame export (ASCII PLY of every fluid particle, OBJ of every rigid mesh: run_simulation.py:137-150) is host file I/O and can
    # dwarf the simulation -- 1.3 s per frame for the 1.23 M particles of final_scene0.json -- so it is reported apart from the steps
    dt = time.perf_counter() - t0
    print(f"Simulation Finished: {cnt} steps, {particles}, {1e3 * (dt - t_export) / cnt:.3f} ms/step "
          f"(+ {t_export:.2f} s writing {frames} frame(s): {1e3 * dt / cnt:.3f} ms/step all in)")


class FoamStepper:
    """The solver as run_loop drives it, with one diffuse-particle step of every * dt behind every `every` simulation steps: the steps
    of one advance() go to the device in pieces that end where a diffuse step is due.  Under run_loop_timed (advance_to) the diffuse
    step takes the scene time that has passed since the last one."""

    def __init__(self, solver, container, diffuse, every, dt):
        self.solver, self.container, self.diffuse, self.every, self.dt = solver, container, diffuse, every, dt
        self.since = 0
        self.t_last = float(container.total_time)

    def advance_to(self, t, max_steps=None):
        done = 0
        while max_steps is None or done < max_steps:
            k = self.every - self.since
            got = self.solver.advance_to(t, max_steps=k if max_steps is None else min(k, max_steps - done))
            done += got
            self.since += got
            if self.since == self.every:
                now = float(self.container.total_time)
                self.diffuse.step(self.container, now - self.t_last)
                self.since, self.t_last = 0, now
            if got < k:
                break
        return done

    def advance(self, n):
        while n > 0:
            k = min(n, self.every - self.since)
            self.solver.advance(k)
            n -= k
            self.since += k
            if self.since == self.every:
                self.diffuse.step(self.container, self.every * self.dt)
                self.since = 0


def make_foam(container, solver, config, args):
    """The diffuse set of --foam: the scene's domain, radius and gravity, Configuration.foam over the defaults (keys that are no
    parameter are ignored, as the reference ignores keys), --foam_max or twice the particle capacity."""
    from sph_project_amd.foam import DEFAULTS, DiffuseParticles
    given = config.get_cfg("foam") or {}
    params = {k: v for k, v in given.items() if k in DEFAULTS and k not in ("device", "max_diffuse")}
    params["max_diffuse"] = args.foam_max or 2 * int(container.particle_max_num)
    params.setdefault("padding", float(container.padding))
    lo = np.zeros(3)
    lo[:len(container.domain_start)] = container.domain_start
    hi = np.asarray(container.domain_end, dtype=np.float64)
    return DiffuseParticles(container.dx, lo, hi, gravity=[float(g) for g in solver.g], **params)


def make_renderer(container, args, **kw):
    """run_simulation.py:70-108: the window's camera, light and particle radius dx"""
    from sph_project_amd.render import FrameRenderer
    return FrameRenderer(container.dx, width=args.render_size[0], height=args.render_size[1], camera_position=args.camera_position,
                         camera_lookat=args.camera_lookat, fov=args.camera_fov, **kw)


class ImageOutput:
    """One image per frame, {frame}/{png_name}, of what `renderer` holds when store() is called; with --png_device the file is compressed
    on the device, with --video the same device image is also a frame of {out_dir}/{avi_name}."""

    def __init__(self, png_name, avi_name, renderer, args, out_dir, device=-1):
        self.png_name, self.renderer = png_name, renderer
        self.png = self.video = self.avi = None
        if args.png_device:
            from sph_project_amd.png import PngEncoder
            self.png = PngEncoder(renderer.width, renderer.height, coding=args.png_coding, device=device)
        if args.video:
            from sph_project_amd.video import AviWriter, VideoEncoder
            self.video = VideoEncoder(renderer.width, renderer.height, quality=args.video_quality, chroma=args.video_chroma, device=device)
            self.avi = AviWriter(f"{out_dir}/{avi_name}", renderer.width, renderer.height, args.video_fps)

    def store(self, frame_dir, draw):
        """draw(download) renders the frame"""
        from sph_project_amd.render import store_png
        store_png(f"{frame_dir}/{self.png_name}", self.renderer, draw, self.png)
        if self.avi is not None:
            self.avi.add(self.video.encode_last(self.renderer))


def main_sharded(args, rank, world):
    """One rank of --gpus N: the scene's z-slab of this rank, the loop of main(), collective output frames."""
    from sph_project_amd import _lib, launch
    config = SimConfig(scene_file_path=args.scene_file)
    sched = Schedule(config, args)
    os.makedirs(sched.out_dir, exist_ok=True)

    lib = _lib.load()
    ndev = lib.sph_device_count()
    if ndev < 1:
        raise SystemExit("run_simulation: no HIP device visible")
    if os.environ.get("SPH_COMM_TRANSPORT", "").startswith("shm"):
        device = rank % ndev   # the shared-memory transports let several ranks share a GPU
    elif world > ndev:
        if rank == 0:
            print(f"run_simulation: --gpus {world} needs one GPU per rank, {ndev} visible (SPH_COMM_TRANSPORT=shm+ipc lets ranks share "
                  "one)", file=sys.stderr)
        raise SystemExit(2)
    else:
        device = rank
    uid = launch.exchange_unique_id(lib, rank)
    cuts = launch.plan_scene_cuts(config.config, world)
    method = config.get_cfg("simulationMethod")
    container = METHODS[method][0](config, GGUI=False, rigid_backend=args.rigid_backend, device=device,
                                   slab=dict(rank=rank, nranks=world, unique_id=uid, cuts=cuts))
    solver = METHODS[method][1](container)
    engine = container.engine
    if rank == 0:
        print(f"Simulation method: {method} on {world} ranks ({engine.comm_transport()}), slab cuts {cuts}")
    solver.prepare()

    renderer = raw = None
    if sched.output_frames:   # every rank draws its slab; the frame is composited on rank 0
        renderer = make_renderer(container, args, device=device)
        if rank == 0:
            raw = ImageOutput("raw_view.png", "raw_view.avi", renderer, args, sched.out_dir, device)

    def write_frame(cnt):
        d = frame_dir(sched.out_dir, cnt)
        if raw is not None:   # collective: every rank draws, rank 0 holds the frame
            raw.store(d, lambda dl: renderer.from_container(container, download=dl))
        elif renderer is not None:
            renderer.from_container(container)
        if sched.output_ply:   # one file per fluid object: the ranks' owned particles, appended in rank order
            obj = engine.download(_lib.F_OBJECT_ID)
            own = engine.download(_lib.F_GHOST) == 0   # (container.dump does not filter the ghosts)
            pos = engine.download(_lib.F_POSITION)
            fluid_ids = sorted(container.object_id_fluid_body)
            totals = engine.comm_allreduce([float(((obj == i) & own).sum()) for i in fluid_ids]) if fluid_ids else []
            for i, total in zip(fluid_ids, totals):
                for r in range(world):
                    if r == rank:
                        write_ply_ascii_part(f"{d}/particle_object_{i}.ply", pos[(obj == i) & own], int(round(total)), r == 0)
                    engine.comm_barrier()
        if sched.output_obj and rank == 0:
            for r_body_id in container.object_id_rigid_body:
                if "mesh" not in container.object_collection[r_body_id]:
                    continue
                with open(f"{d}/mesh_object_{r_body_id}.obj", "w") as f:
                    f.write(container.object_collection[r_body_id]["mesh"].export(file_type="obj"))
        return True

    t0 = time.perf_counter()
    cnt, t_export, frames = run_loop(solver, engine, sched, sched.output_ply or sched.output_obj or sched.output_frames, write_frame,
                                     [raw.avi] if raw is not None and raw.avi is not None else [])
    n_global = int(round(engine.comm_allreduce([engine.comm_get_slab()["n_owned"]])[0]))
    if rank == 0:
        report(cnt, f"{n_global} particles on {world} ranks", t0, t_export, frames)
    return container, solver


def main(argv=None):
    args = parse_args(argv)
    if args.gpus > 1:
        from sph_project_amd import launch
        me = launch.rank_of_this_process()
        if me is None:   # the parent: starts the ranks, opens no GPU
            rcs = launch.spawn_ranks(sys.argv[1:] if argv is None else list(argv), args.gpus, script=os.path.abspath(__file__))
            if any(rcs):
                print(f"run_simulation: rank exit codes {rcs}", file=sys.stderr)
                raise SystemExit(1)
            return None
        return main_sharded(args, me[0], me[1])
    config = SimConfig(scene_file_path=args.scene_file)
    sched = Schedule(config, args)
    out_dir = sched.out_dir
    os.makedirs(out_dir, exist_ok=True)

    method = config.get_cfg("simulationMethod")
    if method not in METHODS:
        raise NotImplementedError(f"Simulation method {method} not implemented")
    container = METHODS[method][0](config, GGUI=False, rigid_backend=args.rigid_backend)
    solver = METHODS[method][1](container)
    print(f"Simulation method: {method}")
    solver.prepare()

    recon = None
    if args.reconstruct or args.render_meshes:
        from sph_project_amd.surface import SurfaceReconstructor
        recon = SurfaceReconstructor(container.dx)
        post = surface_postprocess(args)
        if post is not None:
            recon.set_postprocess(**post)
        if args.anisotropic:
            recon.set_anisotropy(**surface_anisotropy(args))
    renderer = raw = surface = meshes_out = None
    if sched.output_frames or args.render_surface:
        renderer = make_renderer(container, args)
    if sched.output_frames:   # run_simulation.py:131-134
        raw = ImageOutput("raw_view.png", "raw_view.avi", renderer, args, out_dir)
    if args.render_surface:   # the surface objects: the fluid particles of the visible objects.  The same renderer holds the raw frame
        # first, then the surface frame: encoders and a video file of its own
        chosen = dict(iterations=args.surface_iters, sigma=args.surface_sigma, range=args.surface_range)
        renderer.set_surface(**{k: v for k, v in chosen.items() if v is not None})
        if args.surface_thickness:
            chosen = dict(absorb=args.surface_absorb, scatter=args.surface_scatter, iterations=args.surface_thickness_iters)
            renderer.set_thickness(**{k: v for k, v in chosen.items() if v is not None})
        surface = ImageOutput("surface_view.png", "surface_view.avi", renderer, args, out_dir)
    if args.render_meshes:   # render.py: every mesh of the frame -> {frame}/render.png
        mesh_renderer = make_renderer(container, args, box=(np.zeros(3), np.asarray(container.domain_end, dtype=np.float64)))
        if args.raytrace:
            mesh_renderer.set_trace(**trace_keywords(args))
        meshes_out = ImageOutput("render.png", "render.avi", mesh_renderer, args, out_dir)

    diffuse = None   # --foam: a second particle set that reads the fluid and never writes it
    stepped = solver
    if args.foam:
        diffuse = make_foam(container, solver, config, args)
        stepped = FoamStepper(solver, container, diffuse, args.foam_every, float(solver.dt[None]))
        if args.surface_foam:   # into the surface frames; as spheres into the particle frame exactly when that frame is written
            chosen = dict(density=args.surface_foam_density, depth_bias=args.surface_foam_bias)
            renderer.set_surface_foam(diffuse, raw_spheres=raw is not None, **{k: v for k, v in chosen.items() if v is not None})
        elif raw is not None:
            renderer.set_foam(diffuse)

    exporter = None   # --export_device: the text files come from the device state
    if args.export_device:
        from sph_project_amd.text import TextExporter
        exporter = TextExporter()

    def write_frame(cnt):
        wrote = False
        held = set()
        if raw is not None:
            raw.store(frame_dir(out_dir, cnt), lambda dl: renderer.from_container(container, download=dl))
            wrote = True
        if surface is not None:   # the same splat: the raw frame's rgb is overwritten on the device once its file is written
            if raw is None:
                renderer.from_container(container, download=False)
            surface.store(frame_dir(out_dir, cnt), lambda dl: renderer.surface(download=dl))
            wrote = True
        if diffuse is not None:   # key order; a header and no vertex while there is none
            write_ply_ascii(f"{frame_dir(out_dir, cnt)}/diffuse_particles.ply", diffuse.download()["x"])
            wrote = True
        if sched.output_ply:
            d = frame_dir(out_dir, cnt)
            for f_body_id in container.object_id_fluid_body:
                if exporter is not None:
                    exporter.ply_object(container, f_body_id).write(f"{d}/particle_object_{f_body_id}.ply")
                else:
                    write_ply_ascii(f"{d}/particle_object_{f_body_id}.ply", container.dump(obj_id=f_body_id)["position"])
                if args.reconstruct:   # what surface_reconstruction.py would make of that PLY, without reading it back
                    if exporter is not None:   # the mesh stays on the device: formatted there, and the mesh frame below reads it there
                        recon.from_container(container, f_body_id, download=False)
                        exporter.obj_surface(recon).write(f"{d}/particle_object_{f_body_id}.obj")
                    else:
                        recon.from_container(container, f_body_id)
                        recon.write_obj(f"{d}/particle_object_{f_body_id}.obj")
                    held = {f_body_id}   # the reconstructor still holds this object's mesh: the mesh frame below need not redo it
                wrote = True
        if sched.output_obj:   # run_simulation.py:146-150
            d = frame_dir(out_dir, cnt)
            for r_body_id in container.object_id_rigid_body:
                if "mesh" not in container.object_collection[r_body_id]:   # body given as pre-voxelised points only
                    continue
                with open(f"{d}/mesh_object_{r_body_id}.obj", "w") as f:
                    f.write(container.object_collection[r_body_id]["mesh"].export(file_type="obj"))
                wrote = True
        if meshes_out is not None:
            meshes = frame_meshes(container, solver, recon, held, water=args.raytrace)
            meshes_out.store(frame_dir(out_dir, cnt), lambda dl: mesh_renderer.from_meshes(meshes, download=dl))
            wrote = True
        return wrote

    outputs = [o for o in (raw, surface, meshes_out) if o is not None]
    t0 = time.perf_counter()
    wants = sched.output_ply or sched.output_obj or outputs or diffuse is not None
    if getattr(solver, "cfl_method", "none") == "velocity":   # adaptive time stepping: the loop goes by scene time
        cnt, t_export, frames = run_loop_timed(stepped, container.engine, sched, wants, write_frame,
                                               [o.avi for o in outputs if o.avi is not None], max_steps=args.max_steps)
    else:
        cnt, t_export, frames = run_loop(stepped, container.engine, sched, wants, write_frame, [o.avi for o in outputs if o.avi is not None])
    report(cnt, f"{container.particle_num[None]} particles", t0, t_export, frames)
    if diffuse is not None:
        st = diffuse.stats()
        print(f"Diffuse particles: {st['diffuse']} after {st['step']} steps ({st['born_total']} born, {st['died_total']} died, "
              f"{st['dropped_total']} dropped)")
    return container, solver


if __name__ == "__main__":
    main()
