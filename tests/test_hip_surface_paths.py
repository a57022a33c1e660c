"""GPU: the device paths of the surface reconstruction (csrc/sph_surface.hpp) that smooth shapes never take, each forced
by one input of tests/surface_cases.py and compared with the float64 model like the smooth shapes of tests/test_hip_surface.py: every
case-table row, 8 points per thread, bricks split into parts (full and partial last part), runs staged in more than one chunk, the
scan's carry between rounds, negative coordinates, one particle, duplicate particles, bricks smaller than a workgroup -- in the strict
and in the fast build.  tests/test_surface_host.py checks on the CPU that the inputs force what they claim."""
import pytest

from tests import surface_cases as SC

pytestmark = pytest.mark.gpu

# stats()["pair_tests"] is the one observable of the field pass's tests * pts bookkeeping, which splitting a brick into parts (pts of the
# last, partial part) and chunking a run (tests += cnt per chunk) touch
PAIR_TESTS = ("ball_b17", "dense_b2")


@pytest.fixture(scope="module")
def models():
    return {name: SC.model(name) for name in SC.PATH_CASES}


@pytest.mark.parametrize("name", list(SC.PATH_CASES))
def test_forced_path_matches_the_model(gpu, models, name):
    SC.check_mesh_against_model(*models[name], smooth=False, pair_tests=name in PAIR_TESTS, label=name)


@pytest.mark.parametrize("name", list(SC.PATH_CASES))
def test_forced_path_matches_the_model_in_the_fast_build(gpu, models, name):
    """Triangles, counts, vertices and normals as in the strict build, with the strict build's bounds: q = r * (1 / h) rounds once more
    than r / h, one ulp per term of the (2 N + 12) u that allow 12 per term.  Not the brick statistics: x * (1 / (B e)) may bin a
    particle on a cell face into the neighbouring cell, which changes the set of active bricks but neither the mesh nor its order."""
    SC.check_mesh_against_model(*models[name], smooth=False, fast_math=True, label=name)
