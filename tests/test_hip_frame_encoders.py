"""GPU: what both frame encoders (png.PngEncoder, video.VideoEncoder) make of each of the renderer's four frame states: encode_last is
exactly encode(renderer.last_rgb()) where the renderer holds a frame -- particles, meshes, particles with another renderer's layer
merged in -- and raises "holds no frame" where it holds none."""
import numpy as np
import pytest

from sph_project_amd.png import PngEncoder
from sph_project_amd.render import FrameRenderer
from sph_project_amd.video import VideoEncoder

pytestmark = pytest.mark.gpu

W, H = 37, 53


def _renderer():
    return FrameRenderer(0.05, width=W, height=H, box=((0, 0, 0), (2, 2, 2)))


def _points(seed, first_id):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 2.0, (200, 3)).astype(np.float32)
    return x, rng.integers(0, 256, (200, 3), dtype=np.uint8), np.arange(first_id, first_id + 200, dtype=np.uint32)


@pytest.mark.parametrize("Encoder", [PngEncoder, VideoEncoder])
def test_encode_last_in_every_frame_state(gpu, Encoder):
    enc = Encoder(W, H)
    r = _renderer()
    with pytest.raises(Encoder.Error, match="encode_last: the renderer holds no frame"):   # nothing drawn: said on the Python side
        enc.encode_last(r)
    r._last = r._native(r.box)   # ... and by the library, of a native renderer that has drawn nothing yet
    with pytest.raises(Encoder.Error, match=f"{Encoder.ABI}_encode_render: the renderer holds no frame"):
        enc.encode_last(r)

    r.from_points(*_points(3, 0))
    particles = enc.encode_last(r)
    assert (r.ids() >= 0).sum() > 50 and particles == enc.encode(r.last_rgb())

    v = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [1, 1, 1.5]], np.float32)
    t = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]], np.int32)
    r.from_meshes([(v, t, None, (60, 140, 230))])
    meshes = enc.encode_last(r)
    assert (r.ids() >= 0).sum() > 50 and meshes == enc.encode(r.last_rgb()) and meshes != particles

    other = _renderer()
    other.from_points(*_points(4, 200))
    r.from_points(*_points(3, 0))
    merged_rgb = r.merge_layer(*other.layer())
    merged = enc.encode_last(r)
    assert merged == enc.encode(merged_rgb) == enc.encode(r.last_rgb()) and merged != particles
