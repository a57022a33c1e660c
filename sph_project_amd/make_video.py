#!/usr/bin/env python
"""The command line of the reference's make_video.py, without imageio: the frames of a run directory -> one Motion-JPEG AVI.

    python sph_project_amd/make_video.py --input_dir high_fluid_output --output_path high_fluid.avi [--image_name raw_view.png] [--fps 20]

As in the reference the frame directories are taken in the order of their integer names and a frame whose image does not load is
reported and skipped.  Each PNG is decoded on the host (video.decode_png) and compressed on the GPU (video.VideoEncoder);
the container is a classic AVI, which every player and ffmpeg read.  For a directory written by run_simulation.py --video this gives
the bytes of the driver's own {out}/raw_view.avi (or render.avi with --image_name render.png)."""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--input_dir", type=str, required=True, help="experiment directory")
    parser.add_argument("--image_name", type=str, default="raw_view.png")
    parser.add_argument("--output_path", type=str, required=True, help="output video path (.avi)")
    parser.add_argument("--fps", type=int, default=20)
    parser.add_argument("--quality", type=int, default=90, help="JPEG quality 1..100 (not in the reference)")
    parser.add_argument("--chroma", default="420", choices=["420", "444"], help="chroma subsampling (not in the reference)")
    return parser.parse_args(argv)


def frame_directories(input_dir):
    """The sub-directories with integer names, in integer order (anything else in the run directory is no frame)."""
    names = [d for d in os.listdir(input_dir) if d.isdigit() and os.path.isdir(os.path.join(input_dir, d))]
    return sorted(names, key=int)


def main(argv=None):
    args = parse_args(argv)
    if not args.output_path.lower().endswith(".avi"):
        sys.exit(f"make_video: {args.output_path!r}: the only container written here is Motion-JPEG in AVI (no imageio, no H.264 "
                 "encoder); give an output path that ends in .avi")
    if not 1 <= args.fps <= 1000:
        sys.exit(f"make_video: --fps {args.fps}: the frame rate is an integer in 1..1000")
    from sph_project_amd.video import AviWriter, VideoEncoder, decode_png
    encoder = writer = None
    try:
        for frame in frame_directories(args.input_dir):
            file_path = os.path.join(args.input_dir, frame, args.image_name)
            try:
                with open(file_path, "rb") as f:
                    image = decode_png(f.read())
                if encoder is not None and image.shape != (encoder.height, encoder.width, 3):
                    raise ValueError(f"{image.shape[1]} x {image.shape[0]} pixels, the video is {encoder.width} x {encoder.height}")
            except (OSError, ValueError) as e:
                print(f"failed to load image from frame {frame} ({e})")
                continue
            if encoder is None:
                h, w = image.shape[:2]
                encoder = VideoEncoder(w, h, quality=args.quality, chroma=args.chroma)
                writer = AviWriter(args.output_path, w, h, args.fps)
            writer.add(encoder.encode(image))
    finally:
        if writer is not None:
            writer.close()
    if writer is None:
        sys.exit(f"make_video: no frame of {args.input_dir!r} holds a readable {args.image_name}")
    print(f"{args.output_path}: {writer.frames} frame(s), {writer.size} bytes")


if __name__ == "__main__":
    main()
