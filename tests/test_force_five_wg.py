"""The all-fluid, one-mass WCSPH force pass of the fast build at five workgroups per CU (WcsphForcePass::FIVE_WG): a 32-byte tile record
(p_j / rho_j^2 in A.w instead of the candidate's mass, no third LDS array), <= 96 VGPRs without spills, a <= 32 KB tile.

CPU: the resource remarks the fast kernels were compiled with (sph_project_amd/csrc/build/kernels_fast.resources, written by every build).
GPU: the new layout against the generic all-fluid instantiation (SPH_NO_UNIFORM_MASS: the 36-byte record at four workgroups per CU), which
computes the same roundings in the same order -- every field bit for bit, on the headline scene from rest and after its collapse, and
through the rarely taken walks (debug modes 1 and 4) on a small scene."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from sph_project_amd import _lib as L, product as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOURCES = os.path.join(ROOT, "sph_project_amd", "csrc", "build", "kernels_fast.resources")


def _kernel_resources(path):
    """{demangled kernel name: {remark: value}} from hipcc's -Rpass-analysis=kernel-resource-usage output."""
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?):\s+(\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = subprocess.run(["c++filt"], input="\n".join(kernels), text=True, capture_output=True, check=True).stdout.splitlines()
    assert len(names) == len(kernels)
    return dict(zip(names, kernels.values()))


def test_five_wg_force_pass_fits_96_vgprs_and_32_kb():
    assert os.path.exists(RESOURCES), "build the library first (__graft_entry__.build())"
    res = _kernel_resources(RESOURCES)
    five = {k: v for k, v in res.items() if k.startswith("void sph_fast_ns::k_nbr_pass<sph_fast_ns::WcsphForcePass<true, true, false>,")}
    assert len(five) == 2, sorted(five)   # MASKMODE 2 and its mode-0 fallback
    for name, r in five.items():
        assert int(r["VGPRs"]) <= 96, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        # five workgroups per CU in LDS allocation granules of 1280 B: 5 x 25 granules fit 160 KB, 5 x 26 do not (the compiler's occupancy
        # remark does not know the granule: 32,552 B was reported as 5 waves per SIMD and ran 4 workgroups per CU)
        assert -(-int(r["LDS Size [bytes/block]"]) // 1280) * 5 <= 160 * 1024, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 5, (name, r)
    # every other force-pass instantiation keeps its layout: the 36-byte record and its 38-40 KB tile, four workgroups per CU
    others = {k: v for k, v in res.items() if "WcsphForcePass<" in k and k not in five}
    assert others
    for name, r in others.items():
        assert int(r["LDS Size [bytes/block]"]) > 32768 and int(r["Occupancy [waves/SIMD]"]) == 4, (name, r)


def _fields(container):
    e = container.engine
    ids = e.download(L.F_PARTICLE_ID)
    return [H.by_id(ids, e.download(f)) for f in (L.F_POSITION, L.F_VELOCITY, L.F_DENSITY)]


def _both_layouts(monkeypatch, build, checkpoints):
    """Run `build()`'s scene with the five-workgroup layout and with the generic one; the states at every checkpoint (step counts)."""
    out = []
    for generic in (False, True):
        if generic:
            monkeypatch.setenv("SPH_NO_UNIFORM_MASS", "1")
        else:
            monkeypatch.delenv("SPH_NO_UNIFORM_MASS", raising=False)
        container, solver = build()
        solver.prepare()
        states, done = [], 0
        for k in checkpoints:
            container.engine.step(k - done)
            done = k
            states.append(_fields(container))
        out.append(states)
        del container, solver
    return out


@pytest.mark.gpu
def test_five_wg_layout_is_bit_identical_on_the_headline_scene(gpu, monkeypatch):
    """C2 (1,231,200 particles, fast build): 20 steps from rest, then on into the collapse (step 1500, where moving groups pile up past
    the 32 KB tile and take a second staging round)."""
    cfg = P.c2_scene("wcsph")
    a, b = _both_layouts(monkeypatch, lambda: P.build_product(cfg, fast_math=1), (20, 1500))
    for sa, sb in zip(a, b):
        for x, y in zip(sa, sb):
            np.testing.assert_array_equal(x, y)
    assert not np.array_equal(a[0][1], a[1][1])   # (the scene did move between the two checkpoints)


@pytest.mark.gpu
@pytest.mark.parametrize("fg", [1, 4], ids=["chunked-overflow-walk", "ordered-walk"])
def test_five_wg_layout_is_bit_identical_on_the_rare_walks(gpu, monkeypatch, fg):
    """Debug mode 1 sends every run through the tile-overflow walk (MASKMODE 0), mode 4 every group through the ordered walk: both read
    the record's A.w as p_j / rho_j^2 in the new layout."""
    cfg = H.dam_break_scene(end=(0.3, 0.26, 0.22), translation=(0.13, 0.11, 0.07))
    a, b = _both_layouts(monkeypatch, lambda: H.build_product(cfg, jitter=0.003, seed=2, fast_math=1, force_global=fg), (10,))
    for x, y in zip(a[0], b[0]):
        np.testing.assert_array_equal(x, y)
