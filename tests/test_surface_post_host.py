"""CPU: surface post-processing without a GPU -- the C-ABI mirror, the smoothing flags of the drop-in CLI and of the
driver, and properties of the numpy restatement (tests/surface_post_model.py) on the model meshes of tests/surface_model.py."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from sph_project_amd import _lib as L
from tests import surface_model as SM
from tests import surface_post_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["sph_surface_set_postprocess", "sph_surface_post_stats", "sph_surface_download_post"]


# --- C-ABI -----------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header and name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("struct", ["SphSurfacePostParams", "SphSurfacePostStats"])
def test_post_structs_match_the_header(struct):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None
    cls = getattr(L, struct)
    names = [n for n, _ in cls._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"sph_hip.h\"\nint main(void){\n"
    src += "".join(f'printf("%zu\\n", offsetof({struct}, {n}));\n' for n in names)
    src += f'printf("%zu\\n", sizeof({struct})); return 0; }}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "o.c"), os.path.join(d, "o")
        open(c, "w").write(src)
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    assert [getattr(cls, n).offset for n in names] == vals[:-1]
    assert ctypes.sizeof(cls) == vals[-1]


def test_post_calls_refuse_null_handles():
    lib = L.load()
    p = L.SphSurfacePostParams(mesh_smoothing_iters=1, mesh_smoothing_weights=0, weights_normalization=13.0, normals_smoothing_iters=0)
    assert lib.sph_surface_set_postprocess(None, ctypes.byref(p)) == -1
    st = L.SphSurfacePostStats()
    assert lib.sph_surface_post_stats(None, ctypes.byref(st)) == -1
    assert lib.sph_surface_download_post(None, None, None, None) == -1


# --- the drop-in CLI and the driver --------------------------------------------------------------------------------------------------

def _fake_cli(tmp_path, monkeypatch, argv):
    from sph_project_amd import surface, surface_reconstruction as SR
    from sph_project_amd.run_simulation import write_ply_ascii
    os.makedirs(tmp_path / "0")
    write_ply_ascii(str(tmp_path / "0" / "particle_object_0.ply"), np.zeros((2, 3), np.float32))
    calls = []

    class Fake:
        def __init__(self, radius, smoothing_length, cube_size, iso, normals):
            calls.append(("create", radius, smoothing_length, cube_size, iso, normals))

        def set_postprocess(self, **kw):
            calls.append(("post", kw))

        def from_points(self, xyz):
            calls.append(("points",))

        def write_obj(self, path):
            calls.append(("obj",))

    monkeypatch.setattr(surface, "SurfaceReconstructor", Fake)
    SR.main(["--input_dir", str(tmp_path)] + argv)
    return calls


def test_cli_without_smoothing_flags_never_calls_set_postprocess(tmp_path, monkeypatch):
    calls = _fake_cli(tmp_path, monkeypatch, ["--radius", "0.02"])
    assert [c[0] for c in calls] == ["create", "points", "obj"]


def test_cli_passes_the_reference_smoothing_flags(tmp_path, monkeypatch):
    calls = _fake_cli(tmp_path, monkeypatch, ["--mesh-smoothing-weights=on", "--mesh-smoothing-iters=25", "--normals-smoothing-iters=10"])
    assert [c[0] for c in calls] == ["create", "post", "points", "obj"]
    assert calls[1][1] == dict(mesh_smoothing_iters=25, mesh_smoothing_weights=True, weights_normalization=13.0, normals_smoothing_iters=10)


def test_cli_passes_every_smoothing_flag(tmp_path, monkeypatch):
    calls = _fake_cli(tmp_path, monkeypatch, ["--mesh-smoothing-iters", "7", "--mesh-smoothing-weights", "off",
                                              "--mesh-smoothing-weights-normalization", "20.5"])
    assert calls[1] == ("post", dict(mesh_smoothing_iters=7, mesh_smoothing_weights=False, weights_normalization=20.5,
                                     normals_smoothing_iters=0))
    from sph_project_amd import surface_reconstruction as SR
    with pytest.raises(SystemExit):
        SR.parse_args(["--input_dir", "x", "--mesh-smoothing-weights", "maybe"])


def test_driver_forwards_the_smoothing_flags():
    from sph_project_amd import run_simulation as RS, surface_reconstruction as SR
    base = ["--scene_file", "x.json", "--reconstruct"]
    assert RS.surface_postprocess(RS.parse_args(base)) is None
    got = RS.surface_postprocess(RS.parse_args(base + ["--mesh_smoothing_iters", "25", "--mesh_smoothing_weights",
                                                       "--normals_smoothing_iters", "10"]))
    assert got == dict(mesh_smoothing_iters=25, mesh_smoothing_weights=True, weights_normalization=13.0, normals_smoothing_iters=10)
    # the same settings as the drop-in CLI's spelling of them (both then write the same bytes)
    cli = SR.postprocess_settings(SR.parse_args(["--input_dir", "x", "--mesh-smoothing-iters=25", "--mesh-smoothing-weights=on",
                                                 "--normals-smoothing-iters=10"]))
    assert got == cli
    assert RS.surface_postprocess(RS.parse_args(base + ["--normals_smoothing_iters", "3"])) == dict(
        mesh_smoothing_iters=0, mesh_smoothing_weights=False, weights_normalization=13.0, normals_smoothing_iters=3)
    # main hands exactly these keywords to the reconstructor
    src = open(os.path.join(ROOT, "sph_project_amd", "run_simulation.py")).read()
    assert "post = surface_postprocess(args)" in src and "recon.set_postprocess(**post)" in src


# --- the model -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ball():
    x = SM.lattice_ball((0.31, 0.27, 0.33), 0.08, 0.02)
    return x, SM.reconstruct(x, 0.01, normals=False)


def test_model_adjacency_is_symmetric_and_closed_meshes_have_degree_3(ball):
    _, m = ball
    nv = len(m["vertices"])
    off, nb = PM.adjacency(nv, m["triangles"])
    deg = np.diff(off)
    assert deg.min() >= 3
    src = np.repeat(np.arange(nv), deg)
    fwd = set(zip(src.tolist(), nb.tolist()))
    assert all((b, a) in fwd for a, b in fwd)
    assert (src != nb).all()
    for i in range(0, nv, 97):   # ascending, unique
        row = nb[off[i]:off[i + 1]]
        assert (np.diff(row) > 0).all()
    # on a closed 2-manifold every vertex has as many neighbours as incident triangles
    inc = np.bincount(m["triangles"].ravel(), minlength=nv)
    assert np.array_equal(deg, inc)


def test_model_smoothing_lowers_the_spread_of_radii(ball):
    _, m = ball
    v = m["vertices"].astype(np.float32)
    off, nb = PM.adjacency(len(v), m["triangles"])
    c = np.array([0.31, 0.27, 0.33])
    r0 = np.linalg.norm(v - c, axis=1)
    s = PM.smooth(v, off, nb, iters=25)
    r1 = np.linalg.norm(s.astype(np.float64) - c, axis=1)
    assert r1.std() < r0.std() and r1.std() / r1.mean() < r0.std() / r0.mean(), (r0.std(), r1.std())
    # the marching-cubes facets go: the distance of a vertex to the mean of its neighbours drops by far more than the radius spread

    def rough(p):
        p = p.astype(np.float64)
        sums = np.add.reduceat(p[nb], off[:-1], axis=0)
        return np.linalg.norm(p - sums / np.diff(off)[:, None], axis=1).mean()
    assert rough(s) < 0.3 * rough(v), (rough(v), rough(s))
    assert s.dtype == np.float32 and np.isfinite(s).all()
    # zero weight: nothing moves; no iteration: nothing moves
    assert np.array_equal(PM.smooth(v, off, nb, w=np.zeros(len(v), np.float32), iters=3), v)
    assert np.array_equal(PM.smooth(v, off, nb, iters=0), v)


def test_model_normal_smoothing_keeps_unit_length(ball):
    x, m = ball
    mm = SM.reconstruct(x, 0.01)
    off, nb = PM.adjacency(len(mm["vertices"]), mm["triangles"])
    n = PM.smooth_normals(mm["normals"].astype(np.float32), off, nb, iters=10)
    assert np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # smoothing turns the normals towards the ball's radial direction, never away on average
    radial = mm["vertices"] - np.array([0.31, 0.27, 0.33])
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    assert (np.einsum("ij,ij->i", n, radial).mean() >= np.einsum("ij,ij->i", mm["normals"], radial).mean() - 1e-9)


def test_model_gives_an_isolated_particle_weight_zero():
    block = SM.lattice_ball((0.2, 0.2, 0.2), 0.05, 0.02)
    drop = np.array([[0.6, 0.6, 0.6]], np.float32)
    x = np.concatenate([block, drop])
    m = SM.reconstruct(x, 0.01, normals=False)
    h = m["h"]
    w = PM.weights(m["vertices"], x, h)
    near_drop = np.linalg.norm(m["vertices"] - drop[0], axis=1) < h
    assert near_drop.sum() > 20
    assert (w[near_drop] == 0.0).all()
    assert (w[~near_drop] == 1.0).mean() > 0.9   # the block's surface particles have far more than 13 in c_j
    c, n_max = PM.particle_counts(x, h)
    assert c[-1] == 0.0 and n_max > 20
