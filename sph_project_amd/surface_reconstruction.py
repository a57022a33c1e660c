#!/usr/bin/env python
"""Drop-in for the reference's surface_reconstruction.py: every frame directory under --input_dir, every particle_object_{id}.ply in
it -> the .obj beside it (ply_path.replace(".ply", ".obj")).  The reference runs `splashsurf reconstruct` per file in a process pool;
here one GPU reconstructs the frames in order (sph_project_amd/surface.py), so --num_workers is accepted and ignored.

    python sph_project_amd/surface_reconstruction.py --input_dir final_scene0_output --radius 0.01 [--smoothing-length 3.5]
        [--mesh-smoothing-weights=on --mesh-smoothing-iters=25 --normals-smoothing-iters=10]
        [--anisotropic [--aniso-ratio 2 --aniso-min-neighbours 25 --aniso-sparse-scale 0.5]]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--input_dir", type=str, required=True)
    parser.add_argument("--num_workers", type=int, default=4, help="accepted for compatibility; frames run in order on one GPU")
    parser.add_argument("--radius", type=float, default=0.01)
    parser.add_argument("--smoothing-length", type=float, default=3.5)
    parser.add_argument("--cube-size", type=float, default=0.5, help="splashsurf -c (multiples of the radius)")
    parser.add_argument("--surface-threshold", type=float, default=0.6, help="splashsurf -t")
    parser.add_argument("--no-normals", action="store_true", help="no vn lines (splashsurf --normals=off)")
    # splashsurf's post-processing; the reference's command: 25 / on / 10.  Not given: no smoothing
    parser.add_argument("--mesh-smoothing-iters", type=int, default=None)
    parser.add_argument("--mesh-smoothing-weights", choices=["on", "off"], default=None)
    parser.add_argument("--mesh-smoothing-weights-normalization", type=float, default=None)
    parser.add_argument("--normals-smoothing-iters", type=int, default=None)
    # anisotropic kernels (run_simulation.py's --anisotropic, --aniso_ratio, ...).  Not given: the isotropic kernel
    parser.add_argument("--anisotropic", action="store_true")
    parser.add_argument("--aniso-ratio", type=float, default=None, help="with --anisotropic: >= 1 (2)")
    parser.add_argument("--aniso-min-neighbours", type=int, default=None, help="with --anisotropic (25)")
    parser.add_argument("--aniso-sparse-scale", type=float, default=None, help="with --anisotropic: in (0, 1] (0.5)")
    parser.add_argument("--export_device", action="store_true",
                        help="format the .obj files on the GPU from the device mesh (DESIGN.md 23: the same bytes, no mesh download)")
    args = parser.parse_args(argv)
    for flag in ("aniso_ratio", "aniso_min_neighbours", "aniso_sparse_scale"):
        if getattr(args, flag) is not None and not args.anisotropic:
            parser.error(f"--{flag.replace('_', '-')} sets a parameter of the anisotropic kernels: give --anisotropic as well")
    if args.anisotropic:
        from sph_project_amd.run_simulation import anisotropy_error
        why = anisotropy_error(args.aniso_ratio, args.aniso_min_neighbours, args.aniso_sparse_scale)
        if why:
            parser.error(why.replace("--aniso_", "--aniso-").replace("min_neighbours", "min-neighbours").replace("sparse_scale", "sparse-scale"))
    return args


def postprocess_settings(args):
    """set_postprocess keywords of the smoothing flags, or None when none of them was given."""
    given = (args.mesh_smoothing_iters, args.mesh_smoothing_weights, args.mesh_smoothing_weights_normalization, args.normals_smoothing_iters)
    if all(g is None for g in given):
        return None
    return dict(mesh_smoothing_iters=args.mesh_smoothing_iters or 0, mesh_smoothing_weights=args.mesh_smoothing_weights == "on",
                weights_normalization=13.0 if args.mesh_smoothing_weights_normalization is None else args.mesh_smoothing_weights_normalization,
                normals_smoothing_iters=args.normals_smoothing_iters or 0)


def frame_jobs(input_dir):
    """(ply_path, obj_path) of every frame in the reference's order: frame directories by int(name), .ply files in listdir order."""
    frames = sorted(os.listdir(input_dir), key=lambda x: int(x))
    jobs = []
    for frame in frames:
        frame_dir = os.path.join(input_dir, frame)
        for ply_file in [f for f in os.listdir(frame_dir) if f.endswith(".ply")]:
            ply_path = os.path.join(frame_dir, ply_file)
            jobs.append((ply_path, ply_path.replace(".ply", ".obj")))
    return jobs


def main(argv=None):
    args = parse_args(argv)
    jobs = frame_jobs(args.input_dir)
    from sph_project_amd.run_simulation import read_ply_ascii
    from sph_project_amd.surface import SurfaceReconstructor
    recon = SurfaceReconstructor(args.radius, smoothing_length=args.smoothing_length, cube_size=args.cube_size,
                                 iso=args.surface_threshold, normals=not args.no_normals)
    post = postprocess_settings(args)
    if post is not None:
        recon.set_postprocess(**post)
    if args.anisotropic:
        from sph_project_amd.run_simulation import surface_anisotropy
        recon.set_anisotropy(**surface_anisotropy(args))
    exporter = None
    if args.export_device:
        from sph_project_amd.text import TextExporter
        exporter = TextExporter()
    for ply_path, obj_path in jobs:
        try:
            if exporter is not None:
                recon.from_points(read_ply_ascii(ply_path), download=False)
                exporter.obj_surface(recon).write(obj_path)
            else:
                recon.from_points(read_ply_ascii(ply_path))
                recon.write_obj(obj_path)
        except Exception as e:   # the reference's worker reports a failed frame and goes on
            print(f"failed to process {os.path.dirname(ply_path)}")
            print(e)
    return jobs


if __name__ == "__main__":
    main()
