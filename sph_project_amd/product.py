"""Scene dicts and builders of the product path (no oracle, no test code): what bench.py, __graft_entry__.smoke()
and the tests use to go from a JSON-like scene in the reference's format to a container + solver pair driven exactly
like the reference's run_simulation.py drives its own (XContainer(config) -> XSolver(container) -> prepare() -> step()).
"""
from __future__ import annotations

import copy

import numpy as np

from . import scene
from .SPH.utils import SimConfig


def dam_break_scene(method="wcsph", domain_end=(1.0, 1.0, 1.0), start=(0.0, 0.0, 0.0), end=(0.4, 0.4, 0.4),
                    translation=(0.1, 0.1, 0.1), velocity=(0.0, 0.0, 0.0), dt=4e-4, viscosity=10.0,
                    add_domain_box=False, viscosity_method="standard", radius=0.01, **extra):
    """SURVEY 8(d) config C1 by default: 20^3 = 8000-particle cube, WCSPH."""
    cfg = {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": list(domain_end), "addDomainBox": add_domain_box,
            "particleRadius": radius, "density0": 1000, "simulationMethod": method,
            "viscosityMethod": viscosity_method, "gravitation": [0.0, -9.81, 0.0], "timeStepSize": dt,
            "viscosity": viscosity,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": list(start), "end": list(end), "translation": list(translation),
            "scale": [1, 1, 1], "velocity": list(velocity), "density": 1000.0, "color": [50, 100, 200],
            "entryTime": -1.0,
        }],
    }
    cfg["Configuration"].update(extra)
    return cfg


def c2_scene(method="wcsph", scale_z=1):
    """block identical to data/scenes/final_scene0.json:55-59 of the reference.
    scale_z = N (weak scaling over N GPUs): the block and the domain are N times as deep in z, i.e. N x 80 lattice
    planes = N x 1,231,200 particles, so every z-slab holds one C2's worth of work."""
    dt = 6e-4 if method == "dfsph" else 4e-4
    return {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [8.5, 8.0, 0.4 + 1.6 * scale_z], "addDomainBox": False,
            "particleRadius": 0.01, "density0": 1000, "simulationMethod": method, "viscosityMethod": "standard",
            "gravitation": [0.0, -9.81, 0.0], "timeStepSize": dt, "viscosity": 10.0,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": [0.09, 0.2, 0.2], "end": [1.7, 4.0, 0.2 + 1.6 * scale_z],
            "translation": [0.0, 0.0, 0.0], "scale": [1, 1, 1], "velocity": [0.0, -0.5, 0.0], "density": 1000.0,
            "color": [50, 100, 200], "entryTime": -1.0,
        }],
    }


def c4_scene(method="wcsph"):
    """100 x 250 x 160 = 4,000,000 particles; the block spans the full z extent, so z-slabs stay
    balanced while the dam breaks along x.  One fixed scene: sharding it over N GPUs is strong scaling."""
    return {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [6.0, 6.0, 3.36], "addDomainBox": False,
            "particleRadius": 0.01, "density0": 1000, "simulationMethod": method, "viscosityMethod": "standard",
            "gravitation": [0.0, -9.81, 0.0], "timeStepSize": 4e-4, "viscosity": 10.0,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": [0.1, 0.1, 0.08], "end": [2.1, 5.1, 3.28], "translation": [0.0, 0.0, 0.0],
            "scale": [1, 1, 1], "velocity": [0.0, -0.5, 0.0], "density": 1000.0, "color": [50, 100, 200],
            "entryTime": -1.0,
        }],
    }


def c5_scene(domain_end=(4.0, 20.0, 8.0), start=(1.12, 1.0, 1.0), end=(1.88, 12.2, 1.08), g_upper=2.5,
             velocity=(0.0, -2.2, 0.75)):
    """the reference's buckling scene data/scenes/final_scene3.json (DFSPH + implicit viscosity,
    mu = mu_b = 1800, dt 1e-3, emitter above y = 2.5, a 38 x 560 x 5 fluid sheet inside a 4 x 20 x 8 domain box of
    ~2.07 M static boundary particles, G = 10 M cells) without its mesh rigid body (cookie_bar_small.obj needs trimesh).
    The arguments shrink the box and the sheet for tests; the defaults are the reference's numbers."""
    return {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": list(domain_end), "addDomainBox": True,
            "particleRadius": 0.01, "density0": 1000, "simulationMethod": "dfsph", "viscosityMethod": "implicit",
            "gravitation": [0.0, -9.81, 0.0], "gravitationUpper": g_upper, "timeStepSize": 0.001,
            "viscosity": 1800.0, "viscosity_b": 1800.0,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": list(start), "end": list(end), "translation": [0.0, 0.0, 0.0],
            "scale": [1, 1, 1], "velocity": list(velocity), "density": 1000.0, "color": [50, 100, 200],
            "entryTime": -1.0,
        }],
    }


def iisph_bath_scene(domain_end=(5.0, 3.0, 2.0), start=(0.3, 0.2, 0.5), end=(1.2, 2.8, 1.6)):
    """The configuration of the reference's IISPH scene data/scenes/dragon_bath_iisph.json: a 5 x 3 x 2 domain box, dx 0.01,
    dt 8e-4, mu 10, mu_b 5, one fluid block (translated by (0.2, 0, 0.2)) falling at 1 m/s.  The arguments shrink the domain
    and the block for tests; the defaults are the reference's numbers."""
    return {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": list(domain_end), "addDomainBox": True,
            "particleRadius": 0.01, "fps": 30.0, "totalTime": 8.0, "density0": 1000,
            "gravitation": [0.0, -9.81, 0.0], "simulationMethod": "iisph", "viscosityMethod": "standard",
            "timeStepSize": 0.0008, "viscosity": 10.0, "viscosity_b": 5.0, "boundaryHandlingMethod": 0,
            "exportFrame": True, "exportPly": False, "exportObj": False,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": list(start), "end": list(end), "translation": [0.2, 0.0, 0.2],
            "scale": [1, 1, 1], "velocity": [0.0, -1.0, 0.0], "density": 1000.0, "color": [50, 100, 200],
            "entryTime": -1.0,
        }],
    }


def pbf_scene(domain_end=(2.0, 1.6, 1.0), start=(0.1, 0.1, 0.1), end=(0.6, 1.0, 0.9), add_domain_box=True, dt=4e-4):
    """A 3-D dam break under PBF for the driver and the benchmarks: one fluid block in the corner of a domain box (the
    reference's only PBF scene, data/scenes/high_fluid_pbf_2d.json, is 2-D, which neither it nor this project runs in 3-D
    form).  tools/bench_pbf.py times PBF on c2_scene("pbf") instead."""
    return {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": list(domain_end), "addDomainBox": add_domain_box,
            "particleRadius": 0.01, "fps": 30.0, "totalTime": 2.0, "density0": 1000,
            "gravitation": [0.0, -9.81, 0.0], "simulationMethod": "pbf", "viscosityMethod": "standard",
            "timeStepSize": dt, "viscosity": 10.0, "viscosity_b": 5.0, "boundaryHandlingMethod": 0,
            "exportFrame": True, "exportPly": False, "exportObj": False,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": list(start), "end": list(end), "translation": [0.0, 0.0, 0.0],
            "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0, "color": [50, 100, 200],
            "entryTime": -1.0,
        }],
    }


def pbf_consistent_scene(domain_end=(2.0, 1.6, 1.0), start=(0.1, 0.1, 0.1), end=(0.6, 1.0, 0.9), add_domain_box=True, dt=4e-4, **pbf_keys):
    """pbf_scene under the consistent variant (Configuration.pbfVariant "consistent"); pbf_keys: pbfMaxError,
    pbfMinIterations, pbfMaxIterations, pbfEpsilon."""
    cfg = pbf_scene(domain_end=domain_end, start=start, end=end, add_domain_box=add_domain_box, dt=dt)
    cfg["Configuration"]["pbfVariant"] = "consistent"
    cfg["Configuration"].update(pbf_keys)
    return cfg


def coupling_scene(method="dfsph", models_dir=None, fluid_end=(2.3, 1.4, 2.38)):
    """The reference's rigid-fluid coupling showcase data/scenes/final_scene1.json: its box, fluid block, dt and the placements of its
    nine dynamic bodies, with tests/golden/models/cube.obj in place of the dragon and sphere.obj in place of the rubber ducks (those
    meshes are not in this tree).  fluid_end shrinks the block for tests."""
    import os
    models = models_dir or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "models")
    body = lambda oid, mesh, t, axis, angle, density, v: {
        "objectId": oid, "geometryFile": os.path.join(models, mesh), "translation": list(t), "rotationAxis": list(axis),
        "rotationAngle": angle, "scale": [0.6, 0.6, 0.6], "velocity": list(v), "density": density, "color": [255, 255, 255],
        "isDynamic": True, "entryTime": -1.0}
    down = (0.0, -0.5, 0.0)
    return {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [2.5, 7.0, 2.5], "addDomainBox": True, "particleRadius": 0.01,
            "fps": 60.0, "totalTime": 10.0, "numberOfStepsPerRenderUpdate": 1, "density0": 1000, "gravitation": [0.0, -9.81, 0.0],
            "simulationMethod": method, "viscosityMethod": "standard", "timeStepSize": 0.0007, "viscosity": 13.0, "viscosity_b": 0.3,
            "boundaryHandlingMethod": 0, "exportFrame": True, "exportPly": False, "exportObj": False,
        },
        "RigidBodies": [
            body(1, "cube.obj", (1.5, 3.4, 1.5), (0, 0, 1), 45, 900.0, (0.0, 0.0, 0.0)),
            body(2, "sphere.obj", (0.3, 2.4, 1.25), (0, 1, 0), 0, 500.0, down),
            body(3, "sphere.obj", (1.1, 2.8, 0.3), (0, 1, 0), 0, 500.0, down),
            body(4, "sphere.obj", (2.2, 2.7, 1.15), (0, 1, 0), 0, 500.0, down),
            body(5, "sphere.obj", (2.2, 2.2, 2.2), (0, 1, 0), 0, 500.0, down),
            body(6, "sphere.obj", (0.8, 2.3, 0.7), (0, 1, 0), 0, 300.0, down),
            body(7, "sphere.obj", (2.25, 2.6, 1.7), (0, 1, 0), 180, 300.0, down),
            body(8, "sphere.obj", (2.1, 2.2, 1.2), (0, 1, 0), 180, 300.0, down),
            body(9, "sphere.obj", (1.4, 2.0, 1.4), (0, 1, 0), 0, 300.0, down),
        ],
        "FluidBlocks": [{
            "objectId": 0, "start": [0.2, 0.09, 0.11], "end": list(fluid_end), "translation": [0.0, 0.0, 0.0],
            "scale": [1, 1, 1], "velocity": [0.0, -0.5, 0.0], "density": 1000.0, "color": [50, 100, 200], "entryTime": -1.0,
        }],
    }


def wave_tank_scene(method="wcsph", length=2.4, width=0.5, depth=0.24, stroke=0.03, frequency=1.0, dt=4e-4, radius=0.01,
                    models_dir=None):
    """A wave tank with a piston paddle, the first scene a scripted rigid body is for: a shallow layer of water (depth)
    in a long tank (length along x, width along z) and, at the -x end, a plate -- tests/golden/models/cube.obj scaled to three particle
    layers in x, one and a half water depths in y, the water's width in z -- that a harmonic program moves along x with amplitude
    `stroke` at `frequency`, ramped in over one period.  The sizes go down to a few hundred particles
    (length=0.5, width=0.2, depth=0.06)."""
    import os
    models = models_dir or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "models")
    d, edge, m = 2.0 * radius, 0.298142, 6.0 * radius   # particle diameter, cube.obj's edge, margin to the domain faces
    plate = [3 * d, 1.5 * depth, width - 2 * m]
    plate_x = m + 0.5 * plate[0] + stroke + d
    return {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [length, max(3.0 * depth, 0.3), width], "addDomainBox": False,
            "particleRadius": radius, "density0": 1000, "simulationMethod": method, "viscosityMethod": "standard",
            "gravitation": [0.0, -9.81, 0.0], "timeStepSize": dt, "viscosity": 10.0,
        },
        "RigidBodies": [{
            "objectId": 1, "geometryFile": os.path.join(models, "cube.obj"), "translation": [plate_x, m + 0.5 * plate[1], 0.5 * width],
            "rotationAxis": [0.0, 1.0, 0.0], "rotationAngle": 0.0, "scale": [p / edge for p in plate], "velocity": [0.0, 0.0, 0.0],
            "density": 1000.0, "color": [230, 180, 60], "isDynamic": False, "entryTime": -1.0,
            "motion": {"harmonic": {"frequency": frequency, "ramp": 1.0 / frequency if frequency > 0 else 0.0,
                                    "direction": [1.0, 0.0, 0.0], "amplitude": stroke}},
        }],
        "FluidBlocks": [{
            "objectId": 0, "start": [plate_x + 0.5 * plate[0] + stroke + 2 * d, m, m], "end": [length - m, m + depth, width - m],
            "translation": [0.0, 0.0, 0.0], "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0,
            "color": [50, 100, 200], "entryTime": -1.0,
        }],
    }


def droplet_scene(edge=10, method="wcsph", gamma=1.0, beta=0.0, gravity=0.0, plate_gap=None, cube_gap=None, cube_edge=4,
                  radius=0.01, dt=4e-4, viscosity=10.0, viscosity_b=None, margin=12, viscosity_method="standard"):
    """The first scene of the Akinci surface tension: a cube of edge^3 fluid particles on the rest lattice in the middle
    of a box it never touches (`margin` particle diameters to every face, no domain box), surfaceTensionMethod "akinci" with
    gamma / beta; gravity is the magnitude along -y.  gamma = None leaves the three keys out (the reference's term).
    plate_gap (particle diameters, None: no plate): a static, lattice-aligned plate of two layers under the cube, its upper layer
    plate_gap diameters below the cube's lowest one, four particles wider than the cube on every side.
    cube_gap (diameters, None: no cube): a dynamic rigid cube of cube_edge^3 particles on the same lattice beside the +x face."""
    d = 2.0 * radius
    lo = margin * d
    size = lo + edge * d + lo
    cfg = {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [size + (cube_edge + 2) * d * (cube_gap is not None), size, size],
            "addDomainBox": False, "particleRadius": radius, "density0": 1000, "simulationMethod": method,
            "viscosityMethod": viscosity_method, "gravitation": [0.0, -float(gravity), 0.0], "timeStepSize": dt, "viscosity": viscosity,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": [lo, lo, lo], "end": [lo + (edge - 0.5) * d] * 3, "translation": [0.0, 0.0, 0.0],
            "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0, "color": [50, 100, 200], "entryTime": -1.0,
        }],
    }
    if viscosity_b is not None:
        cfg["Configuration"]["viscosity_b"] = viscosity_b
    if gamma is not None:
        cfg["Configuration"].update(surfaceTensionMethod="akinci", surfaceTension=float(gamma), surfaceAdhesion=float(beta))
    body = lambda oid, pts, t, dyn: {
        "objectId": oid, "geometryFile": "unused.obj", "voxelizedPoints": np.asarray(pts, np.float32).tolist(), "translation": list(t),
        "rotationAxis": [0.0, 1.0, 0.0], "rotationAngle": 0.0, "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0,
        "color": [230, 180, 60], "isDynamic": dyn, "entryTime": -1.0}
    lattice = lambda n: np.stack(np.meshgrid(*[d * np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3)
    bodies = []
    if plate_gap is not None:
        corner = np.array([lo - 4 * d, lo - (plate_gap + 1) * d, lo - 4 * d])
        bodies.append(body(1, corner + lattice((edge + 8, 2, edge + 8)), (0.0, 0.0, 0.0), False))
    if cube_gap is not None:   # a dynamic body's particles are given in body coordinates (about its centre), its translation places it
        pts = lattice((cube_edge,) * 3)
        centre = pts.mean(0)
        corner = np.array([lo + (edge - 1 + cube_gap) * d, lo, lo])
        bodies.append(body(2, pts - centre, corner + centre, True))
    if bodies:
        cfg["RigidBodies"] = bodies
    return cfg


def stirred_tank_scene(edge=10, omega=10.0, method="wcsph", gravity=0.0, radius=0.01, dt=4e-4, viscosity=0.01, margin=8,
                       vorticity_method="micropolar", **keys):
    """The first scene of the micropolar vorticity model: a block of edge^3 fluid particles on the rest lattice in a
    closed box (sampled domain box; `margin` particle diameters from the domain's faces, of which the box's shell takes the first 3.5), started in rigid rotation v = W x (x - centre)
    with W = omega about the vertical (y) axis (block key angularVelocity); gravity is the magnitude along -y.  keys: further
    Configuration keys (vorticity, viscosityOmega, inertiaInverse, ...); vorticity_method = None leaves the vorticity keys out."""
    d = 2.0 * radius
    lo = margin * d
    size = lo + edge * d + lo
    cfg = {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [size, size, size], "addDomainBox": True, "particleRadius": radius,
            "density0": 1000, "simulationMethod": method, "viscosityMethod": "standard", "gravitation": [0.0, -float(gravity), 0.0],
            "timeStepSize": dt, "viscosity": viscosity,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": [lo, lo, lo], "end": [lo + (edge - 0.5) * d] * 3, "translation": [0.0, 0.0, 0.0],
            "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "angularVelocity": [0.0, float(omega), 0.0], "density": 1000.0,
            "color": [50, 100, 200], "entryTime": -1.0,
        }],
    }
    if vorticity_method is not None:
        cfg["Configuration"]["vorticityMethod"] = vorticity_method
    cfg["Configuration"].update(keys)
    return cfg


def jelly_scene(edge=8, young=2.0e4, poisson=0.3, drop=2, pool=0, method="dfsph", radius=0.01, dt=2.5e-4, gravity=9.81, viscosity=0.01,
                margin=6, **keys):
    """The first scene of the elastic solids: a cube of edge^3 particles on the rest lattice, `drop` particle diameters
    above the floor of a closed sampled box (or above the surface of a pool of plain fluid, `pool` layers deep, that fills the box from
    wall to wall), under gravity (the magnitude along -y).  The cube is object 0 and carries the key "elasticity" (young = None leaves
    the key out: the same cube as plain fluid); the pool is object 1.  `margin`: particle diameters between the cube and the box's
    faces sideways (the shell takes the first 3.5).  keys: further Configuration keys."""
    d = 2.0 * radius
    floor = 4 * d                      # first lattice plane above the box's shell
    lo = margin * d
    side = lo + edge * d + lo
    y0 = floor + (pool + drop) * d if pool else floor + drop * d
    height = y0 + (edge + 6) * d + 4 * d
    cfg = {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [side, height, side], "addDomainBox": True, "particleRadius": radius,
            "density0": 1000, "simulationMethod": method, "viscosityMethod": "standard", "gravitation": [0.0, -float(gravity), 0.0],
            "timeStepSize": dt, "viscosity": viscosity,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": [lo, y0, lo], "end": [lo + (edge - 0.5) * d, y0 + (edge - 0.5) * d, lo + (edge - 0.5) * d],
            "translation": [0.0, 0.0, 0.0], "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0,
            "color": [230, 90, 120], "entryTime": -1.0,
        }],
    }
    if young is not None:
        cfg["FluidBlocks"][0]["elasticity"] = {"youngsModulus": float(young), "poissonRatio": float(poisson)}
    if pool:
        cfg["FluidBlocks"].append({
            "objectId": 1, "start": [floor, floor, floor], "end": [side - floor - 0.5 * d, floor + (pool - 0.5) * d, side - floor - 0.5 * d],
            "translation": [0.0, 0.0, 0.0], "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0,
            "color": [50, 100, 200], "entryTime": -1.0,
        })
    cfg["Configuration"].update(keys)
    return cfg


def faucet_scene(nozzle=(6, 6), speed=1.0, hold=2, basin=0, method="wcsph", radius=0.01, dt=4e-4, side=24, height=30, max_layers=40,
                 shape="rectangle", viscosity=0.01, gravity=9.81, **keys):
    """The first scene of the fluid emitters: a nozzle of nozzle[0] x nozzle[1] lattice points (shape "circle": a circle of
    diameter nozzle[0] points) under the lid of a closed sampled box of side x height x side particle diameters, pointing down, over
    a pool `basin` layers deep (0: a dry floor).  The emitter is object 0 (budget: max_layers layers), the pool object 1.  keys:
    further Configuration keys."""
    d = 2.0 * radius
    floor = 4 * d                      # first lattice plane above the box's shell
    w, h = side * d, height * d
    emitter = {"objectId": 0, "shape": shape, "position": [0.5 * w, h - 6 * d, 0.5 * w], "direction": [0.0, -1.0, 0.0],
               "speed": float(speed), "start": 0.0, "end": None, "hold": int(hold), "density": 1000.0, "color": [50, 100, 200]}
    if shape == "circle":
        emitter["radius"] = 0.5 * (nozzle[0] + 0.2) * d
        layer = int(scene.emitter_lattice("circle", 0.0, 0.0, emitter["radius"], d).shape[0])
    else:
        emitter.update(width=(nozzle[0] + 0.5) * d, height=(nozzle[1] + 0.5) * d, up=[0.0, 0.0, 1.0])
        layer = int(nozzle[0]) * int(nozzle[1])
    emitter["maxParticles"] = int(max_layers) * layer
    cfg = {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [w, h, w], "addDomainBox": True, "particleRadius": radius,
            "density0": 1000, "simulationMethod": method, "viscosityMethod": "standard", "gravitation": [0.0, -float(gravity), 0.0],
            "timeStepSize": dt, "viscosity": viscosity,
        },
        "FluidBlocks": [],
        "Emitters": [emitter],
    }
    if basin:
        cfg["FluidBlocks"].append({
            "objectId": 1, "start": [floor, floor, floor], "end": [w - floor - 0.5 * d, floor + (basin - 0.5) * d, w - floor - 0.5 * d],
            "translation": [0.0, 0.0, 0.0], "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0,
            "color": [50, 100, 200], "entryTime": -1.0,
        })
    cfg["Configuration"].update(keys)
    return cfg


def channel_scene(nozzle=(6, 6), speed=2.0, length=40, method="wcsph", radius=0.01, dt=4e-4, side=None, hold=2, max_layers=None,
                  kill=3, viscosity=0.01, gravity=9.81, **keys):
    """The first scene of the outflow volumes: a closed sampled box of length x side x side particle diameters (side:
    the nozzle's larger edge + 12 unless given) with a nozzle of nozzle[0] x nozzle[1] lattice points at its x = 0 end, pointing along
    +x at `speed` m / s, and a kill box `kill` diameters thick across the whole cross-section in front of the far wall.  The emitter is
    object 0 (budget: max_layers layers, 4 * length unless given).  keys: further Configuration keys."""
    d = 2.0 * radius
    floor = 4 * d                      # first lattice plane inside the box's shell
    if side is None:
        side = max(int(nozzle[0]), int(nozzle[1])) + 12
    if max_layers is None:
        max_layers = 4 * int(length)
    L, w = length * d, side * d
    emitter = {"objectId": 0, "shape": "rectangle", "position": [floor + 2 * d, 0.5 * w, 0.5 * w], "direction": [1.0, 0.0, 0.0],
               "up": [0.0, 1.0, 0.0], "width": (nozzle[0] + 0.5) * d, "height": (nozzle[1] + 0.5) * d,
               "speed": float(speed), "start": 0.0, "end": None, "hold": int(hold), "density": 1000.0, "color": [50, 100, 200],
               "maxParticles": int(max_layers) * int(nozzle[0]) * int(nozzle[1])}
    cfg = {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [L, w, w], "addDomainBox": True, "particleRadius": radius,
            "density0": 1000, "simulationMethod": method, "viscosityMethod": "standard", "gravitation": [0.0, -float(gravity), 0.0],
            "timeStepSize": dt, "viscosity": viscosity,
        },
        "FluidBlocks": [],
        "Emitters": [emitter],
        "Outflows": [{"shape": "box", "min": [L - floor - kill * d, 0.0, 0.0], "max": [L, w, w], "invert": False, "start": 0.0,
                      "end": None, "objects": None}],
    }
    cfg["Configuration"].update(keys)
    return cfg


def wind_jet_scene(nozzle=(4, 4), speed=3.0, wind=(5.0, 0.0, 0.0), drag=1.0, method="wcsph", side=20, height=36, max_layers=24,
                   drag_method="gissler", **keys):
    """The first scene of the air drag: faucet_scene's downward nozzle (nozzle[0] x nozzle[1] lattice points, `speed`
    m / s) under the lid of a tall closed sampled box of side x height x side particle diameters with a dry floor, in a constant
    wind (Configuration.airVelocity) with the drag scaled by `drag`.  The emitter is object 0 (budget: max_layers layers).
    drag_method = None leaves the drag keys out (the jet in a vacuum); keys: further Configuration keys (airDensity, ...) and
    faucet_scene's radius, dt, viscosity, gravity, hold."""
    faucet = {k: keys.pop(k) for k in ("radius", "dt", "viscosity", "gravity", "hold", "shape") if k in keys}
    cfg = faucet_scene(nozzle=nozzle, speed=speed, basin=0, method=method, side=side, height=height, max_layers=max_layers, **faucet)
    if drag_method is not None:
        cfg["Configuration"]["dragMethod"] = drag_method
        if drag_method == "gissler":
            cfg["Configuration"].update(drag=float(drag), airVelocity=[float(c) for c in wind])
    cfg["Configuration"].update(keys)
    return cfg


def heated_tank_scene(edge=8, hot=60.0, cold=20.0, alpha=1.0e-4, beta=0.0, plate=True, method="wcsph", gravity=9.81, radius=0.01,
                      dt=4e-4, viscosity=0.01, margin=8, **keys):
    """The first scene of the heat conduction: a block of edge^3 fluid particles on the rest lattice at temperature
    `cold` in a closed sampled box (adiabatic; `margin` particle diameters from the domain's faces, of which the shell takes the first
    3.5), one particle diameter above a static, lattice-aligned plate of two layers (object 1, two particles wider than the block on
    every side) held at `hot`.  thermalMethod "conduction" with thermalDiffusivity alpha, thermalExpansion beta and
    referenceTemperature cold; gravity is the magnitude along -y.  hot = None leaves the plate's key out (an adiabatic plate),
    plate = False the plate itself; alpha = None leaves every thermal key out.  keys: further Configuration keys."""
    d = 2.0 * radius
    lo = margin * d
    size = lo + edge * d + lo
    cfg = {
        "Configuration": {
            "domainStart": [0.0, 0.0, 0.0], "domainEnd": [size, size, size], "addDomainBox": True, "particleRadius": radius,
            "density0": 1000, "simulationMethod": method, "viscosityMethod": "standard", "gravitation": [0.0, -float(gravity), 0.0],
            "timeStepSize": dt, "viscosity": viscosity,
        },
        "FluidBlocks": [{
            "objectId": 0, "start": [lo, lo, lo], "end": [lo + (edge - 0.5) * d] * 3, "translation": [0.0, 0.0, 0.0],
            "scale": [1, 1, 1], "velocity": [0.0, 0.0, 0.0], "density": 1000.0, "color": [50, 100, 200], "entryTime": -1.0,
        }],
    }
    if plate:
        n = (edge + 4, 2, edge + 4)
        pts = np.stack(np.meshgrid(*[d * np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3) + np.array([lo - 2 * d, lo - 2 * d, lo - 2 * d])
        cfg["RigidBodies"] = [{
            "objectId": 1, "geometryFile": "unused.obj", "voxelizedPoints": np.asarray(pts, np.float32).tolist(),
            "translation": [0.0, 0.0, 0.0], "rotationAxis": [0.0, 1.0, 0.0], "rotationAngle": 0.0, "scale": [1, 1, 1],
            "velocity": [0.0, 0.0, 0.0], "density": 1000.0, "color": [230, 180, 60], "isDynamic": False, "entryTime": -1.0}]
    if alpha is not None:
        cfg["Configuration"].update(thermalMethod="conduction", thermalDiffusivity=float(alpha), thermalExpansion=float(beta),
                                    referenceTemperature=float(cold))
        cfg["FluidBlocks"][0]["temperature"] = float(cold)
        if plate and hot is not None:
            cfg["RigidBodies"][0]["temperature"] = float(hot)
    cfg["Configuration"].update(keys)
    return cfg


def scene_particles(cfg_dict):
    """Host lattice of every object present at prepare(), in the reference's insertion order
    (domain box first: base_container.py:192, then FluidBlocks: :215).  Blocks with entryTime > 0 are listed with
    their entry time (`entry_time`); callers that cannot insert late skip or reject them."""
    cfg = SimConfig(config=copy.deepcopy(cfg_dict))
    geo = scene.derive_geometry(cfg)
    batches = []
    blocks = cfg.get_fluid_blocks()
    if geo.add_domain_box:
        pos = scene.box_lattice(geo.domain_box_start, geo.domain_box_size, geo.domain_box_thickness, geo.particle_spacing)
        n = pos.shape[0]
        # BaseSolver.prepare() -> init_object_id() (base_solver.py:680) runs after the box was added in
        # BaseContainer.__init__, so the reference's box particles carry object id -1
        batches.append(dict(object_id=-1, pos=pos, vel=np.zeros((n, 3), np.float32),
                            density=np.full(n, 1000.0, np.float32), material=np.full(n, 2, np.int32),
                            is_dynamic=np.zeros(n, np.int32), entry_time=-1.0))
    for blk in blocks:
        off = np.array(blk["translation"])
        s, e = np.array(blk["start"]) + off, np.array(blk["end"]) + off
        pos = scene.cube_lattice(s, (e - s) * np.array(blk["scale"]), geo.particle_spacing)
        n = pos.shape[0]
        vel = np.tile(np.asarray(blk["velocity"], np.float32), (n, 1))
        if blk.get("angularVelocity") is not None and n > 0:   # (this project's block key: BaseContainer.add_cube)
            w = np.asarray(blk["angularVelocity"], np.float64).reshape(3)
            vel = (vel + np.cross(w, pos.astype(np.float64) - pos.astype(np.float64).mean(0))).astype(np.float32)
        batches.append(dict(object_id=blk["objectId"], pos=pos, vel=vel,
                            density=np.full(n, blk["density"], np.float32), material=np.full(n, 1, np.int32),
                            is_dynamic=np.ones(n, np.int32), entry_time=float(blk.get("entryTime", -1.0))))
    return cfg, geo, batches


def build_product(cfg_dict, **engine_opts):
    """Containers + solver of the product path for a scene dict (what run_simulation.py:46-63 does for a scene file)."""
    from .SPH import containers, fluid_solvers
    cfg = SimConfig(config=copy.deepcopy(cfg_dict))
    method = cfg.get_cfg("simulationMethod")
    ccls = {"wcsph": containers.WCSPHContainer, "dfsph": containers.DFSPHContainer, "pcisph": containers.PCISPHContainer,
            "iisph": containers.IISPHContainer, "pbf": containers.PBFContainer}[method]
    scls = {"wcsph": fluid_solvers.WCSPHSolver, "dfsph": fluid_solvers.DFSPHSolver, "pcisph": fluid_solvers.PCISPHSolver,
            "iisph": fluid_solvers.IISPHSolver, "pbf": fluid_solvers.PBFSolver}[method]
    container = ccls(cfg, GGUI=False, **engine_opts)
    solver = scls(container)
    return container, solver
