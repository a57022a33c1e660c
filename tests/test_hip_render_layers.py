"""GPU, one process: layers of particle frames.  The frame of a particle set is the per-pixel minimum of the key images of
its parts, so parts rendered apart and merged -- in any order -- must give the frame of the whole set with no tolerance at all: colours,
ids and keys.  Also the tail of the four-pixels-per-lane merge kernel, the refusals, and the simulation left untouched."""
import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd.render import FrameRenderer, RenderError
from tests import helpers as H

pytestmark = pytest.mark.gpu

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
Z_NEAR = 0.1


def _spheres(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    c = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    ids = rng.permutation(np.arange(10 * n, dtype=np.uint32))[:n]   # distinct, global
    return x, c, ids


def _reference_set(seed):
    return _spheres(2000, 0.0, 2.0, seed)


CLOSE_EYE, CLOSE_R = np.array([0.0, 0.3, 1.2]), 0.12


def _close_up_set(seed):
    """About 2,000 spheres behind two that matter: one 0.25 in front of the eye to the left (its bounds exceed 4096 pixels: the large
    list) and one to the right whose centre lies 0.21 deep, so that it straddles the near plane (whole-screen bounds; its middle is
    nearer than z_near and not drawn, the rest is)."""
    x, c, ids = _spheres(1998, (-3.0, -3.0, -6.0), (3.0, 3.0, 0.0), seed)
    f = -CLOSE_EYE / np.linalg.norm(CLOSE_EYE)
    s = np.cross(f, [0.0, 1.0, 0.0])
    s /= np.linalg.norm(s)
    near = CLOSE_EYE + 0.25 * f - 0.2 * s
    straddle = CLOSE_EYE + 0.21 * f + 0.15 * s
    depth = float(f @ (straddle - CLOSE_EYE))
    assert depth - CLOSE_R < Z_NEAR < depth + CLOSE_R and np.linalg.norm(straddle - CLOSE_EYE) > CLOSE_R
    return (np.concatenate([x, near[None], straddle[None]]).astype(np.float32),
            np.concatenate([c, [[200, 40, 90], [30, 220, 120]]]).astype(np.uint8),
            np.concatenate([ids, [30001, 30002]]).astype(np.uint32))


CAMERAS = {
    "reference": (_reference_set, 0.03, dict(box=((0, 0, 0), (2, 2, 2)))),
    "close_up": (_close_up_set, CLOSE_R, dict(camera_position=tuple(CLOSE_EYE), camera_lookat=(0.0, 0.0, 0.0), fov=70.0, z_near=Z_NEAR,
                                              box=((-1, -1, -1), (1, 1, 1)))),
}


def _fold(layers):
    key, rgb = layers[0][0].copy(), layers[0][1].copy()
    for k_in, c_in in layers[1:]:
        take = k_in < key
        key = np.where(take, k_in, key)
        rgb = np.where(take[..., None], c_in, rgb)
    return key, rgb


def _merged(base, other, parts, order):
    """Part order[0] rendered by `base`, the layers of order[1:] (rendered by `other`) merged in, in that order."""
    base.from_points(*parts[order[0]])
    rgb = None
    for p in order[1:]:
        other.from_points(*parts[p])
        rgb = base.merge_layer(*other.layer())
    assert rgb.tobytes() == base.last_rgb().tobytes()
    return rgb, base.ids(), base.layer(), base.stats()


def _check_split(make, radius, kw, W, H, fast, seeds, ks):
    whole, base, other = (FrameRenderer(radius, width=W, height=H, fast_math=fast, **kw) for _ in range(3))
    for seed in seeds:
        x, c, ids = make(seed)
        rgb_w = whole.from_points(x, c, ids)
        ids_w, (key_w, lrgb_w), st_w = whole.ids(), whole.layer(), whole.stats()
        assert lrgb_w.tobytes() == rgb_w.tobytes()
        assert (ids_w >= 0).sum() > 200 and (ids_w <= -2).sum() > 20, (seed, "spheres and box lines are in the picture")
        for k in ks:
            part_of = np.random.default_rng(100 * seed + k).integers(0, k, len(x))
            parts = [(x[part_of == p], c[part_of == p], ids[part_of == p]) for p in range(k)]
            layers = []
            for p in range(k):
                other.from_points(*parts[p])
                layers.append(other.layer())
            key_f, rgb_f = _fold(layers)
            assert key_f.tobytes() == key_w.tobytes() and rgb_f.tobytes() == lrgb_w.tobytes(), (seed, k, "numpy fold of the parts' layers")
            for order in (list(range(k)), list(range(k - 1, -1, -1))):
                rgb, ids_m, (key_m, lrgb_m), st = _merged(base, other, parts, order)
                assert rgb.tobytes() == rgb_w.tobytes(), (seed, k, order, int((rgb != rgb_w).any(axis=2).sum()))
                assert ids_m.tobytes() == ids_w.tobytes(), (seed, k, order)
                assert key_m.tobytes() == key_w.tobytes() and lrgb_m.tobytes() == rgb_w.tobytes(), (seed, k, order)
                assert st["covered_pixels"] == st_w["covered_pixels"] == int((ids_w >= 0).sum())
    return st_w


@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fast"])
def test_merged_parts_equal_the_whole_set(gpu, camera, fast):
    make, radius, kw = CAMERAS[camera]
    st = _check_split(make, radius, kw, 160, 120, fast, seeds=(1, 2, 3), ks=(2, 5))
    if camera == "close_up":
        assert st["large"] >= 2   # the sphere in front of the eye and the one across the near plane went through k_render_large


@pytest.mark.parametrize("fast", [False, True], ids=["strict", "fast"])
def test_pixel_count_that_is_no_multiple_of_four(gpu, fast):
    """161 x 119 = 19,159 pixels: 4,789 full groups and a tail of three.  The split scene as above, then a layer of random keys and
    colours that wins about half of ALL pixels, the last three among them."""
    W, Hh = 161, 119
    assert (W * Hh) % 4 == 3
    make, radius, kw = CAMERAS["close_up"]
    _check_split(make, radius, kw, W, Hh, fast, seeds=(4,), ks=(3,))
    r = FrameRenderer(radius, width=W, height=Hh, fast_math=fast, **kw)
    x, c, ids = make(5)
    r.from_points(x, c, ids)
    key0, rgb0 = r.layer()
    rng = np.random.default_rng(11)
    # keys around the frame's own (depth bits of 0.1 .. 4.0, any id below the line ids), a quarter of them empty
    t = rng.uniform(0.1, 4.0, (Hh, W)).astype(np.float32).view(np.uint32).astype(np.uint64)
    key1 = (t << np.uint64(32)) | rng.integers(0, 0xFFFFFFF0, (Hh, W), dtype=np.uint64)
    key1[rng.random((Hh, W)) < 0.25] = NONE
    key1.reshape(-1)[-3:] = np.uint64(1)   # the tail pixels: taken for certain
    rgb1 = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    got = r.merge_layer(key1, rgb1)
    key_f, rgb_f = _fold([(key0, rgb0), (key1, rgb1)])
    take = key1 < key0
    assert 0.2 < take.mean() < 0.9 and take.reshape(-1)[-3:].all()
    key_m, rgb_m = r.layer()
    assert key_m.tobytes() == key_f.tobytes()
    assert got.tobytes() == rgb_f.tobytes() == rgb_m.tobytes()
    lo = (key_f & np.uint64(0xFFFFFFFF)).astype(np.int64)
    want_ids = np.where(key_f == NONE, -1, np.where(lo >= 0xFFFFFFF0, -2 - (lo - 0xFFFFFFF0), lo.astype(np.uint32).view(np.int32)))
    assert np.array_equal(r.ids(), want_ids.astype(np.int32))
    assert r.stats()["covered_pixels"] == int(((key_f != NONE) & (lo < 0xFFFFFFF0)).sum())
    # merging the same layer again changes nothing (ties keep what is there; finish may run any number of times)
    assert r.merge_layer(key1, rgb1).tobytes() == got.tobytes()
    assert r.stats()["covered_pixels"] == int(((key_f != NONE) & (lo < 0xFFFFFFF0)).sum())


def test_layers_need_a_particle_frame(gpu):
    r = FrameRenderer(0.05, width=64, height=48)
    key, rgb = np.full((48, 64), NONE, np.uint64), np.zeros((48, 64, 3), np.uint8)
    with pytest.raises(RenderError) as e:
        r.merge_layer(key, rgb)
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(RenderError) as e:
        r.layer()
    assert e.value.code == L.ERR_INVALID
    h = r._native(None)   # the C-ABI itself, on a renderer that has drawn nothing
    assert r.lib.sph_render_layer_merge(h, key.ctypes.data, rgb.ctypes.data) == L.ERR_INVALID
    assert r.lib.sph_render_layer_download(h, key.ctypes.data, rgb.ctypes.data) == L.ERR_INVALID
    r.from_points(np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError):
        r.merge_layer(key[:, :-1], rgb)   # shapes are checked on the host
    tri = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], np.float32)
    r.from_meshes([(tri, np.array([[0, 1, 2]], np.int32), None, (255, 0, 0))])
    with pytest.raises(RenderError) as e:
        r.layer()
    assert e.value.code == L.ERR_INVALID and "mesh frame" in str(e.value)
    with pytest.raises(RenderError) as e:
        r.merge_layer(key, rgb)
    assert e.value.code == L.ERR_INVALID
    r.from_points(np.zeros((1, 3), np.float32))   # a particle frame again: layers are back
    assert r.layer()[0].shape == (48, 64)


def test_rendering_and_layers_leave_an_unsharded_simulation_bit_identical(gpu):
    """The handle path of an unsharded container goes through the code this change touched (settling, the composite branch not taken):
    stepping on after renders, layer reads and a merge compares bit for bit with a run that never rendered."""
    def run(render):
        container, solver = H.build_product(P.dam_break_scene(method="wcsph", end=(0.16, 0.2, 0.16)))
        solver.prepare()
        r = FrameRenderer(container.dx, width=96, height=64, camera_position=(1.2, 0.7, 1.4), camera_lookat=(0.2, 0.2, 0.2)) if render else None
        frames = []
        for k in range(6):
            solver.step()
            if r is not None and k % 2 == 0:
                a = r.from_container(container)
                cs = r.composite_stats()
                assert cs["ranks"] == 1 and cs["hops"] == 0 and cs["pieces_sent"] == cs["pieces_recv"] == 0
                assert cs["drawn_global"] == r.stats()["drawn"] > 0 and r.has_frame()
                key, rgb = r.layer()
                assert r.merge_layer(key, rgb).tobytes() == a.tobytes()   # its own layer: every key ties
                frames.append(a)
        solver.advance(5)
        eng = container.engine
        eng.synchronize()
        return eng.download(L.F_POSITION), eng.download(L.F_VELOCITY), eng.download(L.F_PARTICLE_ID), solver.stats(), frames
    a, b = run(False), run(True)
    for u, w in zip(a[:3], b[:3]):
        assert u.tobytes() == w.tobytes()
    assert a[3] == b[3]
    assert len(b[4]) == 3 and (b[4][0] != 0).any()
