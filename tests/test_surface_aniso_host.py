"""CPU: anisotropic kernels of the surface reconstruction without a GPU -- the float64 model
(tests/surface_aniso_model.py) against numpy and against its own limit cases, the library's f32 eigen and clamp routine run on the host
against the model, the thin-shape table, mutants of the model, the C-ABI mirror and the drivers' argument errors."""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd.surface import SurfaceError, aniso_matrix_host
from tests import surface_aniso_model as AM
from tests import surface_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, SPACING = 0.01, 0.02
H = 2.0 * 3.5 * R

NEW_SYMBOLS = ["sph_surface_set_anisotropy", "sph_surface_anisotropy_stats", "sph_surface_download_anisotropy",
               "sph_surface_aniso_matrix_host"]


def iso_field(x, h):
    return SM.Field(x, h)


def aniso_field(mutant=None, **kw):
    return lambda x, h: AM.AnisoField(x, h, **dict(AM.DEFAULTS, mutant=mutant, **kw))


# --- the model's eigen path ------------------------------------------------------------------------------------------------------

def test_model_eigen_path_agrees_with_numpy():
    C6, _ = AM.matrix_set()
    C = AM.from6(C6)
    lam, v = AM.eig_sym3(C)
    ref = np.linalg.eigvalsh(C)
    scale = np.abs(ref).max(axis=1, keepdims=True) + 1e-300
    assert (np.abs(np.sort(lam, axis=1) - ref) <= 1e-13 * scale).all()
    assert np.abs(np.einsum("nki,nkj->nij", v, v) - np.eye(3)).max() < 1e-13            # orthonormal
    back = np.einsum("nik,nk,njk->nij", v, lam, v)
    assert (np.abs(back - C).max(axis=(1, 2)) <= 1e-13 * scale[:, 0]).all()             # C = V diag(lambda) V^T


# --- the library's routine on the host against the model ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_matrices():
    C6, N = AM.matrix_set()
    return C6, N, aniso_matrix_host(C6, N, **AM.DEFAULTS), AM.kernel_matrix(AM.from6(C6), N, **AM.DEFAULTS)


def test_host_routine_matches_the_model_within_the_measured_bound(host_matrices):
    C6, N, A32, (A, det, sparse, clamped) = host_matrices
    assert len(C6) > 4000 and sparse.sum() > 100 and clamped.sum() > 1000 and (~clamped & ~sparse).sum() > 100
    err = np.linalg.norm(AM.from6(A32) - A, axis=(1, 2))
    print(f"f32 routine vs model: max ||dA||_F = {err.max():.3e} (recorded {AM.A_F32_MEASURED:.3e}, bound {AM.A_F32_BOUND:.3e})")
    assert AM.A_F32_BOUND == 8.0 * AM.A_F32_MEASURED
    assert err.max() <= AM.A_F32_BOUND, err.max()


def test_host_routine_outputs_are_symmetric_clamped_matrices(host_matrices):
    C6, N, A32, (A, det, sparse, clamped) = host_matrices
    M = AM.from6(A32)                      # (six stored entries: symmetric by construction; the layout is what from6 assumes)
    assert np.array_equal(M, M.transpose(0, 2, 1))
    w = np.linalg.eigvalsh(M)
    # an eigenvalue moves by at most ||dA||_2 <= ||dA||_F
    assert w.min() >= 1.0 - AM.A_F32_BOUND and w.max() <= AM.DEFAULTS["max_ratio"] + AM.A_F32_BOUND
    # the sparse rule is exact: I / sparse_scale
    assert sparse[N < AM.DEFAULTS["min_neighbours"]].all() and sparse[~np.any(C6, axis=1)].all()
    assert np.array_equal(A32[sparse], np.tile(np.float32([2, 0, 0, 2, 0, 2]), (sparse.sum(), 1)))
    assert (N[sparse & np.any(C6 > 0, axis=1)] == AM.DEFAULTS["min_neighbours"] - 1).all()   # a count at min_neighbours is not sparse


def test_host_routine_other_parameters():
    C6, N = AM.matrix_set(max_ratio=4.0, min_neighbours=3)
    A32 = aniso_matrix_host(C6, N, max_ratio=4.0, min_neighbours=3, sparse_scale=1.0)
    A, _, sparse, _ = AM.kernel_matrix(AM.from6(C6), N, 4.0, 3, 1.0)
    # the constant of the spectral function is max_ratio^2: the error grows by (4 / 2)^2 at most
    assert np.linalg.norm(AM.from6(A32) - A, axis=(1, 2)).max() <= 4.0 * AM.A_F32_BOUND
    assert np.array_equal(A32[sparse], np.tile(np.float32([1, 0, 0, 1, 0, 1]), (sparse.sum(), 1)))
    # max_ratio = 1: the identity whatever the covariance
    A1 = aniso_matrix_host(C6, None, max_ratio=1.0, min_neighbours=0)
    keep = np.any(C6 != 0, axis=1)
    assert np.abs(A1[keep] - np.float32([1, 0, 0, 1, 0, 1])).max() <= AM.A_F32_BOUND


# --- the thin-shape table ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tables():
    return AM.shape_table(iso_field), AM.shape_table(aniso_field())


def test_thin_shapes_are_meshed_one_radius_outside_their_centres(tables):
    iso, ani = tables
    print({k: (round(iso[k], 2), round(ani[k], 2)) for k in iso})
    assert len(ani) == 5
    for row, v in ani.items():
        assert abs(v - 1.0) <= 0.15, (row, v)
    assert iso["single layer 12x12x1"] > 1.3 and iso["double layer 12x12x2"] > 1.3


def test_lone_particle_radius():
    assert AM.lone_radius(aniso_field()) < 1.2
    assert AM.lone_radius(iso_field) > 1.9


# --- limit cases -------------------------------------------------------------------------------------------------------------------

def test_full_lattice_neighbourhood_is_isotropic():
    x = AM.lattice((9, 9, 9), SPACING)
    F = AM.AnisoField(x, H, **AM.DEFAULTS)
    i = int(np.argmin(np.linalg.norm(x - 4 * SPACING, axis=1)))   # the middle particle: every neighbour within h is there
    lam = np.linalg.eigvalsh(F.C[i])
    assert abs(lam[0] / lam[2] - 1.0) < 1e-12
    assert np.abs(F.A[i] - np.eye(3)).max() < 1e-12 and not F.sparse[i]


def test_ratio_one_without_the_sparse_rule_is_the_isotropic_field():
    x = SM.jittered_block((0.0, 0.0, 0.0), (6, 5, 3), SPACING, 0.3, 5)
    F = AM.AnisoField(x, H, max_ratio=1.0, min_neighbours=0, sparse_scale=0.5)
    G = SM.Field(x, H)
    pts = np.random.default_rng(2).uniform(-0.03, 0.13, (300, 3))
    assert np.array_equal(F.V, G.V)
    assert np.array_equal(F.phi(pts), G.phi(pts))


# --- properties that pin the method (each is what one mutant of the model breaks) -------------------------------------------------------

def _face_block():
    return AM.lattice((8, 8, 8), SPACING)


def check_covariance_is_about_the_weighted_mean(make):
    x = _face_block()
    F = make(x, H)
    i = int(np.argmin(np.linalg.norm(x - np.array([3, 3, 7]) * SPACING, axis=1)))   # on the top face
    d = np.linalg.norm(x - x[i], axis=1)
    near = d < H
    ref = np.cov(x[near].T, aweights=1.0 - (d[near] / H) ** 3, bias=True)
    assert np.abs(F.C[i] - ref).max() <= 1e-12 * np.abs(ref).max()


def check_every_kernel_integrates_to_one(make):
    x = AM.lattice((12, 12, 1), SPACING)
    F = make(x, H)
    j = 5 * 12 + 5
    assert not F.sparse[j] and np.linalg.eigvalsh(F.A[j]).max() > 1.9        # a flattened kernel
    g = (np.arange(-40, 41) + 0.5) * (H / 40.0)
    pts = x[j] + np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    total = sum(F._w(pts[a:a + 4096], np.array([j]))[0].sum() for a in range(0, len(pts), 4096)) * (H / 40.0) ** 3
    assert abs(total - 1.0) < 0.01, total


def check_gradient_is_the_derivative_of_phi(make):
    x = AM.lattice((12, 12, 2), SPACING)
    F = make(x, H)
    pts = np.array([[0.1, 0.1, 0.03], [0.23, 0.11, 0.01], [0.05, 0.06, -0.009], [0.11, 0.22, 0.025]])
    g, _ = F.grad(pts)
    eps = 1e-6
    fd = np.stack([(F.phi(pts + eps * np.eye(3)[a]) - F.phi(pts - eps * np.eye(3)[a])) / (2 * eps) for a in range(3)], axis=1)
    assert np.abs(g - fd).max() <= 1e-5 * np.abs(fd).max(), (g, fd)


def check_every_stretch_is_clamped(make):
    x = AM.lattice((40, 2, 1), SPACING / 4)      # a flat rod: lambda_1 >> lambda_2 > lambda_3 = 0, enough neighbours
    F = make(x, H)
    assert not F.sparse[40]
    w = np.linalg.eigvalsh(F.A[40])
    assert w.min() >= 1.0 - 1e-12 and w.max() <= AM.DEFAULTS["max_ratio"] + 1e-12, w


def check_count_is_strict(make):
    x = np.array([[0.0, 0.0, 0.0], [H, 0.0, 0.0], [0.0, 0.5 * H, 0.0]])
    F = make(x, H)
    assert list(F.N) == [1, 0, 1]                # the pair at exactly h does not count


def check_volumes_normalise_the_anisotropic_kernels(make):
    x = AM.lattice((12, 12, 1), SPACING)
    F = make(x, H)
    j = 5 * 12 + 5
    own = F._w(x[j:j + 1], np.arange(len(x)))[0].sum()
    assert abs(F.V[j] * own - 1.0) < 1e-12


CHECKS = {
    "cov_about_xi": check_covariance_is_about_the_weighted_mean,
    "no_det": check_every_kernel_integrates_to_one,
    "grad_A": check_gradient_is_the_derivative_of_phi,
    "clamp_l3_only": check_every_stretch_is_clamped,
    "count_le": check_count_is_strict,
    "iso_V": check_volumes_normalise_the_anisotropic_kernels,
}


@pytest.mark.parametrize("name", list(CHECKS))
def test_model_has_the_property(name):
    CHECKS[name](aniso_field())


@pytest.mark.parametrize("name", list(AM.MUTANTS))
def test_mutant_is_caught(name):
    assert set(CHECKS) == set(AM.MUTANTS) and len(AM.MUTANTS) >= 6
    with pytest.raises(AssertionError):
        CHECKS[name](aniso_field(mutant=name))


def test_mutants_also_move_the_table(tables):
    """the end-to-end figure notices the mutants that change the field itself"""
    _, ani = tables
    for name, row, n, k in (("iso_V", "single layer 12x12x1", (12, 12, 1), (5, 5, 0)), ("cov_about_xi", "face of an 8x8x8 block", (8, 8, 8), (3, 3, 7))):
        x = AM.lattice(n, SPACING)
        v = AM.offset_along(aniso_field(mutant=name)(x, H), AM._rays_over_cell(np.array(k) * SPACING, SPACING), (0, 0, 1))
        assert abs(v - ani[row]) > 0.02, (name, v, ani[row])


# --- C-ABI -----------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header and name in L.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("struct", ["SphSurfaceAnisoParams", "SphSurfaceAnisoStats"])
def test_aniso_structs_match_the_header(struct):
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


def test_aniso_calls_refuse_null_handles():
    lib = L.load()
    p = L.SphSurfaceAnisoParams(enabled=1, min_neighbours=25, max_ratio=2.0, sparse_scale=0.5)
    assert lib.sph_surface_set_anisotropy(None, ctypes.byref(p)) == L.ERR_INVALID
    assert lib.sph_surface_set_anisotropy(None, None) == L.ERR_INVALID
    st = L.SphSurfaceAnisoStats()
    assert lib.sph_surface_anisotropy_stats(None, ctypes.byref(st)) == L.ERR_INVALID
    assert lib.sph_surface_download_anisotropy(None, None, None, None, None) == L.ERR_INVALID


BAD = [dict(max_ratio=0.99), dict(max_ratio=float("nan")), dict(max_ratio=float("inf")), dict(max_ratio=1e39), dict(sparse_scale=0.0),
       dict(sparse_scale=-0.5), dict(sparse_scale=1.0001), dict(sparse_scale=float("nan")), dict(sparse_scale=1e-39),
       dict(min_neighbours=-1)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_bad_parameters_are_refused(bad):
    """the check the setter applies, through the host routine that shares it (the setter itself needs a device: tests/test_hip_surface_aniso.py)"""
    C6 = np.float32([[1, 0, 0, 1, 0, 1]])
    assert aniso_matrix_host(C6, **AM.DEFAULTS).shape == (1, 6)
    with pytest.raises(SurfaceError) as ei:
        aniso_matrix_host(C6, **dict(AM.DEFAULTS, **bad))
    assert ei.value.code == L.ERR_INVALID


# --- the drivers ---------------------------------------------------------------------------------------------------------------------

def _exit_code(module, argv):
    """exit code and stderr of `python -m module argv` in a process that cannot see a GPU"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", module] + argv, cwd=ROOT, env=env, capture_output=True, text=True)
    return p.returncode, p.stderr


@pytest.mark.parametrize("argv, word", [
    (["--anisotropic"], "--reconstruct"),
    (["--reconstruct", "--aniso_ratio", "3"], "--anisotropic"),
    (["--render_meshes", "--aniso_min_neighbours", "5"], "--anisotropic"),
    (["--reconstruct", "--aniso_sparse_scale", "0.4"], "--anisotropic"),
    (["--reconstruct", "--anisotropic", "--aniso_ratio", "0.5"], "--aniso_ratio"),
    (["--reconstruct", "--anisotropic", "--aniso_sparse_scale", "1.5"], "--aniso_sparse_scale"),
    (["--reconstruct", "--anisotropic", "--aniso_min_neighbours", "-2"], "--aniso_min_neighbours"),
])
def test_driver_argument_errors_exit_with_2(argv, word):
    rc, err = _exit_code("sph_project_amd.run_simulation", ["--scene_file", "no_such_scene.json"] + argv)
    assert rc == 2 and word in err, (rc, err)


@pytest.mark.parametrize("argv, word", [
    (["--aniso-ratio", "3"], "--anisotropic"),
    (["--aniso-min-neighbours", "5"], "--anisotropic"),
    (["--aniso-sparse-scale", "0.4"], "--anisotropic"),
    (["--anisotropic", "--aniso-ratio", "nan"], "--aniso-ratio"),
    (["--anisotropic", "--aniso-sparse-scale", "0"], "--aniso-sparse-scale"),
    (["--anisotropic", "--aniso-min-neighbours", "-1"], "--aniso-min-neighbours"),
])
def test_cli_argument_errors_exit_with_2(argv, word):
    rc, err = _exit_code("sph_project_amd.surface_reconstruction", ["--input_dir", "no_such_dir"] + argv)
    assert rc == 2 and word in err, (rc, err)


def test_driver_flags_reach_the_reconstructor():
    from sph_project_amd import run_simulation as RS, surface_reconstruction as SR
    a = RS.parse_args(["--scene_file", "x.json", "--render_meshes", "--anisotropic", "--aniso_ratio", "3", "--aniso_sparse_scale", "0.25"])
    assert RS.surface_anisotropy(a) == dict(max_ratio=3.0, sparse_scale=0.25)
    b = SR.parse_args(["--input_dir", "x", "--anisotropic", "--aniso-min-neighbours", "12"])
    assert RS.surface_anisotropy(b) == dict(min_neighbours=12)
    assert RS.surface_anisotropy(RS.parse_args(["--scene_file", "x.json", "--reconstruct", "--anisotropic"])) == {}
    assert not RS.parse_args(["--scene_file", "x.json", "--reconstruct"]).anisotropic
