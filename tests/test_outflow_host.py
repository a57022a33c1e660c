"""CPU: outflow volumes without a device -- the kernels' predicate run on the host (sph_outflow_test_host,
sph_outflow_active_host) against the numpy float32 model tests/outflow_model.py on points exactly on the faces, one ulp either side, on
a sphere's surface, with invert and across the edges of the time window; mutants of the model; every refusal of the scene parser by
message; the host entries' refusals; the channel scene; the driver's --gpus 2 refusal and the ABI symbols.

The predicate is defined in float32 with a fixed evaluation order, so model and library must agree bit for bit: every comparison here is
an equality, no tolerance."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd import scene
from sph_project_amd.SPH.utils import SimConfig
from tests import outflow_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = float(np.float32(4e-4))
F = np.float32

BOX = {"shape": "box", "min": [0.1, 0.2, 0.3], "max": [0.25, 0.4, 0.55]}
SPHERE = {"shape": "sphere", "center": [0.5, 0.5, 0.5], "radius": 0.25}
WINDOW = dict(BOX, start=3.0 * DT, end=7.0 * DT)


def _cfg(outflows, method="wcsph", **keys):
    cfg = P.dam_break_scene(method=method, domain_end=(0.6, 0.6, 0.6), start=(0.08, 0.08, 0.08), end=(0.16, 0.16, 0.16), translation=(0, 0, 0), dt=4e-4)
    cfg["Outflows"] = copy.deepcopy(outflows)
    cfg["Configuration"].update(keys)
    return SimConfig(config=cfg)


def _both(entry, mutant=None):
    can = scene.outflows_of(_cfg([entry]), "wcsph", 3)[0]
    return can, L.outflow_program(can), M.Volume.from_entry(entry, mutant=mutant)


def _ulps(v):
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def box_points(entry):
    """Every combination of (one ulp below, on, one ulp above) each face coordinate and a mid coordinate: 5^3 points, float32."""
    lo, hi = np.asarray(entry["min"], np.float64).astype(F), np.asarray(entry["max"], np.float64).astype(F)
    axes = [_ulps(lo[c]) + _ulps(hi[c]) + [F(0.5) * (lo[c] + hi[c])] for c in range(3)]
    return np.array([[x, y, z] for x in axes[0] for y in axes[1] for z in axes[2]], F)


def sphere_points(entry):
    """Points on the sphere's surface along the axes and a 3-4-5 direction (exact in float32 for these numbers), one ulp either side in
    the leading coordinate, the centre, and random points in a shell around the surface."""
    c, r = np.asarray(entry["center"], np.float64).astype(F), F(entry["radius"])
    pts = [c.copy()]
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for v in _ulps(c[axis] + F(sign) * r):
                p = c.copy(); p[axis] = v; pts.append(p)
    for v in _ulps(c[0] + F(0.6) * r):
        pts.append(np.array([v, c[1] + F(0.8) * r, c[2]], F))
    rng = np.random.default_rng(7)
    d = rng.normal(size=(4000, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    shell = c.astype(np.float64) + d * float(r) * (1.0 + rng.uniform(-3e-7, 3e-7, (4000, 1)))
    return np.concatenate([np.array(pts, F), shell.astype(F)])


# ------------------------------------------------------------------------------------------- the predicate against the model
@pytest.mark.parametrize("invert", [False, True])
def test_box_faces(invert):
    entry = dict(BOX, invert=invert)
    _, prog, m = _both(entry)
    pts = box_points(entry)
    got, want = L.outflow_test_host(prog, pts), m.inside(pts)
    assert np.array_equal(got, want)
    on = np.all((pts >= m.lo) & (pts <= m.hi), axis=1)
    assert np.array_equal(want, ~on if invert else on) and 0 < on.sum() < len(pts)
    corner_lo, corner_hi = m.lo[None, :], m.hi[None, :]
    assert L.outflow_test_host(prog, corner_lo)[0] == (not invert) and L.outflow_test_host(prog, corner_hi)[0] == (not invert)   # inclusive faces


@pytest.mark.parametrize("invert", [False, True])
def test_sphere_surface(invert):
    entry = dict(SPHERE, invert=invert)
    _, prog, m = _both(entry)
    pts = sphere_points(entry)
    got, want = L.outflow_test_host(prog, pts), m.inside(pts)
    assert np.array_equal(got, want)
    # the six axis points lie exactly on the surface (0.5 +- 0.25 is exact): inside
    on = np.array([[0.75, 0.5, 0.5], [0.25, 0.5, 0.5], [0.5, 0.75, 0.5], [0.5, 0.5, 0.25]], F)
    assert np.all(L.outflow_test_host(prog, on) == (not invert))
    shell = want[-4000:]
    assert 0.2 < shell.mean() < 0.8   # the shell straddles the surface


def test_random_volumes():
    rng = np.random.default_rng(11)
    for trial in range(40):
        if trial % 2:
            lo = rng.uniform(0.0, 0.4, 3); entry = {"shape": "box", "min": list(lo), "max": list(lo + rng.uniform(0.01, 0.3, 3))}
        else:
            entry = {"shape": "sphere", "center": list(rng.uniform(0.1, 0.5, 3)), "radius": float(rng.uniform(0.02, 0.3))}
        entry["invert"] = bool(trial % 3 == 0)
        _, prog, m = _both(entry)
        pts = rng.uniform(-0.1, 0.7, (2000, 3)).astype(F)
        extra = box_points(entry) if entry["shape"] == "box" else sphere_points(entry)
        pts = np.concatenate([pts, extra])
        assert np.array_equal(L.outflow_test_host(prog, pts), m.inside(pts)), entry


def test_time_window_edges():
    can, prog, m = _both(WINDOW)
    got = [L.outflow_active_host(prog, DT, k) for k in range(12)]
    assert got == [m.active(k, DT) for k in range(12)] == [3 <= k <= 7 for k in range(12)]
    _, forever, mf = _both(BOX)
    assert all(L.outflow_active_host(forever, DT, k) and mf.active(k, DT) for k in (0, 1, 10 ** 6))
    _, late, ml = _both(dict(BOX, start=2.5 * DT))
    assert [L.outflow_active_host(late, DT, k) for k in range(5)] == [ml.active(k, DT) for k in range(5)] == [False, False, False, True, True]


def _scenario():
    """Three volumes that overlap, one inverted, one windowed; points on all the special places."""
    entries = [dict(BOX, start=3.0 * DT, end=7.0 * DT), dict(SPHERE, center=[0.25, 0.4, 0.5], radius=0.125),
               {"shape": "box", "min": [0.0, 0.0, 0.0], "max": [0.6, 0.6, 0.5], "invert": True}]
    pts = np.concatenate([box_points(entries[0]), sphere_points(entries[1]), box_points(entries[2]),
                          np.random.default_rng(3).uniform(0.0, 0.6, (3000, 3)).astype(F)])
    return entries, pts


def _library_attribution(entries, pts, k):
    hit = np.full(len(pts), -1, np.int64)
    for q in reversed(range(len(entries))):
        _, prog, _ = _both(entries[q])
        if L.outflow_active_host(prog, DT, k):
            hit[L.outflow_test_host(prog, pts)] = q
    return hit


def test_lowest_index_rule():
    entries, pts = _scenario()
    vols = [M.Volume.from_entry(e) for e in entries]
    for k in (2, 3, 7, 8):
        want = M.attribute(vols, pts, k, DT)
        assert np.array_equal(_library_attribution(entries, pts, k), want)
        assert {int(q) for q in np.unique(want)} >= ({-1, 0, 1, 2} if 3 <= k <= 7 else {-1, 1, 2})
    both = M.Volume.from_entry(entries[0]).inside(pts) & M.Volume.from_entry(entries[1]).inside(pts)
    assert both.any() and np.all(M.attribute(vols, pts, 5, DT)[both] == 0) and np.all(M.attribute(vols, pts, 8, DT)[both] == 1)


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_mutants_fail_a_check(mutant):
    """Each wrong variant of the model disagrees with the library on the points the tests above use."""
    entries, pts = _scenario()
    failed = False
    if mutant == "highest_index":
        vols = [M.Volume.from_entry(e) for e in entries]
        failed = not np.array_equal(_library_attribution(entries, pts, 5), M.attribute(vols, pts, 5, DT, mutant=mutant))
    elif mutant == "window_off_by_one":
        _, prog, m = _both(WINDOW, mutant)
        failed = [L.outflow_active_host(prog, DT, k) for k in range(12)] != [m.active(k, DT) for k in range(12)]
    else:
        for entry, points in ((dict(BOX), box_points(BOX)), (dict(SPHERE), sphere_points(SPHERE)), (dict(BOX, invert=True), box_points(BOX))):
            _, prog, m = _both(entry, mutant)
            failed = failed or not np.array_equal(L.outflow_test_host(prog, points), m.inside(points))
    assert failed, mutant


# ------------------------------------------------------------------------------------------- the scene parser
def test_parser_canonical_form():
    out = scene.outflows_of(_cfg([BOX, dict(SPHERE, invert=True, start=0.1, end=0.5, objects=[0])]), "wcsph", 3)
    assert [v["shape"] for v in out] == ["box", "sphere"] and out[0]["end"] == np.inf and out[0]["objects"] is None and not out[0]["invert"]
    assert out[1]["invert"] and (out[1]["start"], out[1]["end"]) == (0.1, 0.5) and out[1]["objects"] == [0] and out[1]["radius"] == 0.25
    assert scene.outflows_of(_cfg([]), "wcsph", 3) == [] and scene.outflows_of(SimConfig(config=P.dam_break_scene()), "pbf", 2) == []
    prog = L.outflow_program(out[1])
    assert (prog.shape, prog.invert, prog.n_objects, prog.objects[0], prog.radius) == (1, 1, 1, 0, 0.25)


REFUSALS = [
    (dict(BOX, colour=1), r"Outflows\[0\]\.colour: unknown key"),
    (dict(BOX, shape="cylinder"), r"Outflows\[0\]\.shape"),
    ({"min": [0, 0, 0], "max": [1, 1, 1]}, r"Outflows\[0\]\.shape is missing"),
    (dict(BOX, min=[0.1, float("nan"), 0.3]), r"Outflows\[0\]\.min"),
    (dict(BOX, max=[0.25, float("inf"), 0.55]), r"Outflows\[0\]\.max"),
    (dict(BOX, min=[0.1, 0.2]), r"Outflows\[0\]\.min"),
    (dict(BOX, max=[0.25, 0.2, 0.55]), r"Outflows\[0\]\.max: min .* >= max"),
    (dict(BOX, min=[0.3, 0.2, 0.3]), r"Outflows\[0\]\.max: min .* >= max"),
    (dict(BOX, radius=0.1), r"Outflows\[0\]\.radius belongs to a sphere"),
    ({"shape": "box", "min": [0, 0, 0]}, r"Outflows\[0\]\.max is missing"),
    (dict(SPHERE, radius=0.0), r"Outflows\[0\]\.radius"),
    (dict(SPHERE, radius=-1.0), r"Outflows\[0\]\.radius"),
    (dict(SPHERE, radius=float("inf")), r"Outflows\[0\]\.radius"),
    (dict(SPHERE, center=[0.5, "x", 0.5]), r"Outflows\[0\]\.center"),
    (dict(SPHERE, min=[0, 0, 0]), r"Outflows\[0\]\.min belongs to a box"),
    ({"shape": "sphere", "radius": 0.1}, r"Outflows\[0\]\.center is missing"),
    (dict(BOX, invert=1), r"Outflows\[0\]\.invert"),
    (dict(BOX, start=0.5, end=0.5), r"Outflows\[0\]\.end"),
    (dict(BOX, start=0.5, end=0.25), r"Outflows\[0\]\.end"),
    (dict(BOX, start=float("nan")), r"Outflows\[0\]\.start"),
    (dict(BOX, objects=[7]), r"Outflows\[0\]\.objects: 7 is not a fluid object"),
    (dict(BOX, objects=[]), r"Outflows\[0\]\.objects"),
    (dict(BOX, objects=[True]), r"Outflows\[0\]\.objects"),
    ("box", r"Outflows\[0\] must be an object"),
]


@pytest.mark.parametrize("entry,message", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_parser_refuses(entry, message):
    with pytest.raises(ValueError, match=message):
        scene.outflows_of(_cfg([entry]), "wcsph", 3)


def test_parser_refuses_scenes():
    with pytest.raises(ValueError, match="Outflows must be a list"):
        scene.outflows_of(_cfg({"shape": "box"}), "wcsph", 3)
    with pytest.raises(ValueError, match="9 volumes, at most 8"):
        scene.outflows_of(_cfg([BOX] * 9), "wcsph", 3)
    with pytest.raises(ValueError, match="Outflows.*PBF"):
        scene.outflows_of(_cfg([BOX], method="pbf"), "pbf", 3)
    with pytest.raises(ValueError, match="Outflows.*PBF"):
        scene.outflows_of(_cfg([BOX], method="pbf", pbfVariant="consistent"), "pbf", 3)
    with pytest.raises(ValueError, match="Outflows.*3-D"):
        scene.outflows_of(_cfg([BOX]), "wcsph", 2)
    with pytest.raises(ValueError, match="Outflows.*gravitationUpper"):
        scene.outflows_of(_cfg([BOX], gravitationUpper=0.3), "wcsph", 3)
    elastic = _cfg([BOX])
    elastic.config["FluidBlocks"][0]["elasticity"] = {"youngsModulus": 1e5, "poissonRatio": 0.3}
    with pytest.raises(ValueError, match="Outflows.*elastic"):
        scene.outflows_of(elastic, "wcsph", 3)
    assert scene.outflows_of(_cfg([dict(BOX, objects=[0])]), "wcsph", 3)[0]["objects"] == [0]   # the dam break's block is object 0


def test_container_refuses_before_a_device(monkeypatch):
    from sph_project_amd.SPH import containers
    monkeypatch.setattr(L, "Engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device was opened")))
    with pytest.raises(ValueError, match=r"Outflows\[0\]\.radius"):
        containers.WCSPHContainer(_cfg([dict(SPHERE, radius=0.0)]), GGUI=False)
    with pytest.raises(ValueError, match="Outflows.*sharded"):
        containers.WCSPHContainer(_cfg([BOX]), GGUI=False, slab=dict(rank=0, nranks=2, unique_id=b"", cuts=[0, 1, 2]))
    with pytest.raises(ValueError, match="Outflows.*PBF"):
        containers.PBFContainer(_cfg([BOX], method="pbf"), GGUI=False)


def test_channel_scene():
    cfg = P.channel_scene(nozzle=(6, 6), speed=2.0, length=40, method="dfsph")
    sc = SimConfig(config=copy.deepcopy(cfg))
    em = scene.emitters_of(sc, "dfsph", 3)
    out = scene.outflows_of(sc, "dfsph", 3)
    assert len(em) == 1 and em[0]["layerParticles"] == 36 and np.allclose(em[0]["direction"], [1, 0, 0]) and em[0]["speed"] == 2.0
    assert len(out) == 1 and out[0]["shape"] == "box" and not out[0]["invert"] and out[0]["objects"] is None
    L_, w = cfg["Configuration"]["domainEnd"][0], cfg["Configuration"]["domainEnd"][1]
    assert L_ == pytest.approx(40 * 0.02) and list(out[0]["max"]) == [L_, w, w] and out[0]["min"][0] > em[0]["position"][0] + 10 * 0.02
    assert out[0]["min"][1] == 0.0 and out[0]["min"][2] == 0.0   # across the whole cross-section
    assert cfg["Configuration"]["simulationMethod"] == "dfsph"


# ------------------------------------------------------------------------------------------- the host entries
def test_host_entries_refuse():
    can, prog, _ = _both(BOX)
    pts = np.zeros((2, 3), F)
    for change, word in ((dict(shape=2), "shape"), (dict(end=0.0), "end"), (dict(n_objects=17), "n_objects"), (dict(reserved=1), "reserved")):
        bad = L.outflow_program(can)
        for k, v in change.items():
            setattr(bad, k, v)
        with pytest.raises(L.SphError) as e:
            L.outflow_test_host(bad, pts)
        assert e.value.code == -1 and word in str(e.value) and "outflow 0" in str(e.value), str(e.value)
    bad = L.outflow_program(can); bad.min[1] = bad.max[1]
    with pytest.raises(L.SphError, match="min .* >= max"):
        L.outflow_test_host(bad, pts)
    bad = L.outflow_program(can); bad.max[2] = float("nan")
    with pytest.raises(L.SphError, match="not finite"):
        L.outflow_test_host(bad, pts)
    sph = L.outflow_program(scene.outflows_of(_cfg([SPHERE]), "wcsph", 3)[0]); sph.radius = 0.0
    with pytest.raises(L.SphError, match="radius"):
        L.outflow_test_host(sph, pts)
    with pytest.raises(L.SphError, match="k must be >= 0"):
        L.outflow_active_host(prog, DT, -1)
    assert L.outflow_test_host(prog, np.zeros((0, 3), F)).shape == (0,)


def test_abi_symbols(tmp_path):
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "sph_hip.h")).read()
    for name in ("sph_set_outflow", "sph_get_outflow_state", "sph_remove_particles", "sph_outflow_test_host", "sph_outflow_active_host"):
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS and f"int {name}(" in header, name
    assert L.PH_OUTFLOW == 33 and L.K_OUTFLOW == 36 and L.MAX_OUTFLOWS == 8 == scene.MAX_OUTFLOWS
    for text in ("SPH_PH_OUTFLOW = 33", "SPH_K_OUTFLOW = 36", "#define SPH_MAX_OUTFLOWS 8", "#define SPH_OUTFLOW_MAX_OBJECTS 16"):
        assert text in header, text
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sph_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(SphOutflow), sizeof(SphOutflowState), offsetof(SphOutflow, start), offsetof(SphOutflow, objects)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(L.SphOutflow), C.sizeof(L.SphOutflowState), L.SphOutflow.start.offset, L.SphOutflow.objects.offset]


def test_driver_refuses_gpus_2_on_an_outflow_scene(tmp_path):
    path = tmp_path / "channel.json"
    cfg = P.dam_break_scene()
    cfg["Outflows"] = [dict(BOX)]
    path.write_text(json.dumps(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sph_project_amd", "run_simulation.py"), "--scene_file", str(path), "--gpus", "2"],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--gpus 2" in r.stderr and "Outflows" in r.stderr, (r.returncode, r.stderr[-400:])
