"""ctypes binding of libsph_hip.so (C-ABI declared in include/sph_hip.h).

The product path has no CPU fallback: if the HIP library is missing or no gfx950 device is
visible, loading / creating a handle raises.  Nothing in here imports the oracle.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPH_HIP_LIB", os.path.join(_HERE, "libsph_hip.so"))  # override: A/B builds only

MAX_OBJECTS = 20
MAT_FLUID, MAT_RIGID = 1, 2
METHOD = {"wcsph": 0, "dfsph": 1, "pcisph": 2, "iisph": 3, "pbf": 4}

# enum SphField
(F_POSITION, F_VELOCITY, F_ACCELERATION, F_DENSITY, F_PRESSURE, F_REST_VOLUME, F_MASS, F_MATERIAL,
 F_OBJECT_ID, F_IS_DYNAMIC, F_COLOR, F_PARTICLE_ID, F_GRID_ID, F_DFSPH_ALPHA, F_DFSPH_KAPPA,
 F_DFSPH_KAPPA_V, F_DENSITY_STAR, F_DENSITY_DERIV, F_PRESSURE_ACCEL, F_PREDICTED_VEL, F_PREDICTED_POS,
 F_CG_X, F_ORIG_POSITION, F_GHOST, F_DFSPH_KAPPA_NEXT, F_DFSPH_KAPPA_V_NEXT, F_DEBUG_CAPTURE,
 F_IISPH_DII, F_IISPH_AII, F_IISPH_DIJ_PJ, F_IISPH_SUM_I, F_PBF_OLD_POSITION, F_PBF_LAMBDA, F_RIGID_CONTACT_DN,
 F_RIGID_CONTACT_COUNT, F_NON_PRESSURE_ACCEL) = range(36)
# implicit viscosity, download only: the CG vectors, D^-1 (n, 9) and the three parts of a split A p walk (3, n, 3)
F_CG_B, F_CG_R, F_CG_P, F_CG_AP, F_CG_V0, F_CG_DINV, F_CG_AP_PARTS = range(36, 43)
# Akinci surface tension, download only: the colour-field normals (fluid rows)
F_SURFACE_NORMAL = 43
# micropolar vorticity model: the angular velocities (up- and download, current order) and a_mp of the last walk (download only)
F_ANGULAR_VELOCITY, F_MICROPOLAR_ACCEL = 44, 45
# elastic solids, current order, zero outside captured elastic objects: a_el, F (row-major) and the stress (xx, xy, xz, yy, yz, zz) of the
# last pass (download only) and the rotation quaternions (x, y, z, w; up- and download)
F_ELASTIC_ACCEL, F_ELASTIC_DEFGRAD, F_ELASTIC_STRESS, F_ELASTIC_ROTATION = 46, 47, 48, 49
# air drag, download only, written on active fluid rows by the last walk: a_drag and (n_i, w, C_D, A_un, y)
F_DRAG_ACCEL, F_DRAG_TERMS = 50, 51
# heat, current order: the temperatures (up- and download through the ids; an upload writes fluid rows only) and dT/dt of the last
# walk (download only, valid until the next sort)
F_TEMPERATURE, F_TEMPERATURE_RATE = 52, 53

_FIELD_SPEC = {  # field -> (dtype, components)
    F_POSITION: (np.float32, 3), F_VELOCITY: (np.float32, 3), F_ACCELERATION: (np.float32, 3),
    F_DENSITY: (np.float32, 1), F_PRESSURE: (np.float32, 1), F_REST_VOLUME: (np.float32, 1),
    F_MASS: (np.float32, 1), F_MATERIAL: (np.int32, 1), F_OBJECT_ID: (np.int32, 1),
    F_IS_DYNAMIC: (np.int32, 1), F_COLOR: (np.int32, 3), F_PARTICLE_ID: (np.int32, 1),
    F_GRID_ID: (np.int32, 1), F_DFSPH_ALPHA: (np.float32, 1), F_DFSPH_KAPPA: (np.float32, 1),
    F_DFSPH_KAPPA_V: (np.float32, 1), F_DENSITY_STAR: (np.float32, 1), F_DENSITY_DERIV: (np.float32, 1),
    F_PRESSURE_ACCEL: (np.float32, 3), F_PREDICTED_VEL: (np.float32, 3), F_PREDICTED_POS: (np.float32, 3),
    F_CG_X: (np.float32, 3), F_ORIG_POSITION: (np.float32, 3), F_GHOST: (np.int32, 1),
    F_DFSPH_KAPPA_NEXT: (np.float32, 1), F_DFSPH_KAPPA_V_NEXT: (np.float32, 1), F_DEBUG_CAPTURE: (np.float32, 1),
    F_IISPH_DII: (np.float32, 3), F_IISPH_AII: (np.float32, 1), F_IISPH_DIJ_PJ: (np.float32, 3), F_IISPH_SUM_I: (np.float32, 1),
    F_PBF_OLD_POSITION: (np.float32, 3), F_PBF_LAMBDA: (np.float32, 1),
    F_RIGID_CONTACT_DN: (np.float32, 3), F_RIGID_CONTACT_COUNT: (np.float32, 1), F_NON_PRESSURE_ACCEL: (np.float32, 3),
    F_CG_B: (np.float32, 3), F_CG_R: (np.float32, 3), F_CG_P: (np.float32, 3), F_CG_AP: (np.float32, 3), F_CG_V0: (np.float32, 3),
    F_CG_DINV: (np.float32, 9), F_CG_AP_PARTS: (np.float32, 9), F_SURFACE_NORMAL: (np.float32, 3),
    F_ANGULAR_VELOCITY: (np.float32, 3), F_MICROPOLAR_ACCEL: (np.float32, 3),
    F_ELASTIC_ACCEL: (np.float32, 3), F_ELASTIC_DEFGRAD: (np.float32, 9), F_ELASTIC_STRESS: (np.float32, 6),
    F_ELASTIC_ROTATION: (np.float32, 4), F_DRAG_ACCEL: (np.float32, 3), F_DRAG_TERMS: (np.float32, 5),
    F_TEMPERATURE: (np.float32, 1), F_TEMPERATURE_RATE: (np.float32, 1),
}

# enum SphPhase
(PH_NEIGHBOR_SEARCH, PH_RIGID_VOLUME, PH_DENSITY, PH_NON_PRESSURE, PH_PRESSURE_INTEGRATE, PH_DFSPH_ALPHA,
 PH_DFSPH_DIVERGENCE, PH_DFSPH_DENSITY, PH_IISPH_PREPARE, PH_IISPH_ITERATION, PH_PBF_DENSITY_LAMBDA,
 PH_PBF_FIX_POSITION, PH_PBF_PREDICT, PH_PBF_FINISH, PH_RIGID_CONTACT) = range(15)
# the consistent PBF variant (sph_set_pbf_variant)
PH_PBFC_PREDICT, PH_PBFC_DENSITY_LAMBDA, PH_PBFC_DELTA, PH_PBFC_FINISH = 15, 16, 17, 18
# PCISPH pass by pass (after PH_NON_PRESSURE): init_step, and the two walks of one iteration of refine
PH_PCISPH_INIT, PH_PCISPH_RHO_STAR, PH_PCISPH_PRESSURE_ACCEL = 19, 20, 21
# DFSPH: the end of a step behind the sort as the step runs it (density + alpha + first D rho / Dt in one walk, then the divergence loop)
PH_DFSPH_ALPHA_DIVERGENCE = 22
# implicit viscosity: the launches of the CG solve inside PH_NON_PRESSURE one pass each (PH_CG_UPDATE_P launches nothing where the step
# folds the p update into the next A p pass)
PH_CG_PREPARE, PH_CG_AP, PH_CG_UPDATE_XR, PH_CG_UPDATE_P, PH_CG_END = 23, 24, 25, 26, 27
# Akinci surface tension: the normal pass alone (PH_NON_PRESSURE then runs on the stored normals)
PH_SURFACE_NORMALS = 28
# micropolar vorticity model: the walk alone (PH_NON_PRESSURE / PH_CG_END then add the stored a_mp)
PH_MICROPOLAR = 29
# elastic solids: the scatter and the passes A and B alone (PH_NON_PRESSURE / PH_CG_END then add the stored a_el)
PH_ELASTIC = 30
PH_EMIT = 31   # fluid emitters: the hold and the emission of the current step count alone
PH_DRAG = 32   # air drag: the walk alone (PH_NON_PRESSURE / PH_CG_END then add the stored a_drag)
PH_OUTFLOW = 33   # outflow: the mark and the count of the current step count alone (no sort)
PH_CFL = 34       # adaptive time stepping: the reduce of the largest speed alone (no new step size)
PH_HEAT = 35      # heat: the gather and the walk alone (PH_NON_PRESSURE / PH_CG_END then add the buoyancy of the gathered T)

# enum SphKernelId
KERNEL_IDS = ["hash_count", "scan", "scatter", "density", "non_pressure", "pressure_integrate",
              "rigid_volume", "dfsph_density_alpha", "dfsph_rho_adv", "dfsph_correct", "reduce",
              "pcisph_rho_star", "pcisph_pressure_accel", "cg_prepare", "cg_ap", "cg_vector", "misc", "halo",
              "wcsph_forces", "iisph_prepare", "iisph_dij_pj", "iisph_sum_i", "pbf_density_lambda", "pbf_fix_position",
              "pbf_update"]
K_RIGID_CONTACT = 25   # sph_kernel_name(25) == "rigid_contact" (KERNEL_IDS keeps its PBF tail)
K_RIGID_INTEGRATE = 26   # sph_kernel_name(26) == "rigid_integrate": the device rigid backend's launch
K_RIGID_CONTACT_SOLVE = 27   # sph_kernel_name(27) == "rigid_contact_solve": the device_contact rigid backend's launch
K_PBFC_DENSITY_LAMBDA = 28   # sph_kernel_name(28) == "pbfc_density_lambda": walk A of the consistent PBF variant
K_PBFC_DELTA = 29            # sph_kernel_name(29) == "pbfc_delta": its walk B
K_RIGID_MOTION = 30          # SPH_K_RIGID_MOTION: the launch that moves the scripted rigid bodies (sph_kernel_name's table ends at 29)
K_SURFACE_NORMALS = 31       # SPH_K_SURFACE_NORMALS: the normal pass of the Akinci surface tension
K_MICROPOLAR = 32            # SPH_K_MICROPOLAR: the gather + walk of the micropolar vorticity model
K_ELASTIC = 33               # SPH_K_ELASTIC: scatter + pass A + pass B of the elastic solids
K_EMIT = 34                  # SPH_K_EMIT: the hold launch and the emit launch of the fluid emitters
K_DRAG = 35                  # SPH_K_DRAG: the walk of the air drag
K_OUTFLOW = 36               # SPH_K_OUTFLOW: the mark launch of the outflow volumes / of a removal by id
K_CFL = 37                   # SPH_K_CFL: the reduce of the largest speed (adaptive time stepping)
K_HEAT = 38                  # SPH_K_HEAT: the gather + walk of the heat conduction
RIGID_MOTION_MAX_KEYS = 64
MAX_EMITTERS = 8             # SPH_MAX_EMITTERS
EMITTER_MAX_HOLD = 8         # SPH_EMITTER_MAX_HOLD
EMITTER_SHAPES = {"rectangle": 0, "circle": 1}
ELASTIC_MAX_NEIGHBOURS = 64  # SPH_ELASTIC_MAX_NEIGHBOURS

# rigid contact table (sph_get_rigid_contacts): [object A][partner B][normal bin][value]; partners 20..25 are the domain box /
# the wall planes, one per bin; values: pairs, midpoint sum (3), depth * n sum (3), maximum depth
CONTACT_PARTNERS, CONTACT_BINS, CONTACT_VALUES = 26, 6, 8
CONTACT_WALL0 = 20
# one row of sph_get_rigid_contact_rows: A, B (-1: infinite mass), point (3), normal (3), depth, ln, lt (2), lr (2), lp, table partner
CONTACT_ROW_VALUES = 16


class SphParams(C.Structure):
    _fields_ = [
        ("domain_size", C.c_double * 3), ("particle_radius", C.c_double), ("support_radius", C.c_double),
        ("V0", C.c_double), ("padding", C.c_double), ("grid_num", C.c_int32 * 3),
        ("gravity", C.c_double * 3), ("g_upper", C.c_double), ("viscosity", C.c_double),
        ("viscosity_b", C.c_double), ("density_0", C.c_double), ("surface_tension", C.c_double),
        ("dt", C.c_double), ("particle_max_num", C.c_int32), ("viscosity_implicit", C.c_int32),
        ("method", C.c_int32), ("fixed_iterations", C.c_int32), ("fast_math", C.c_int32),
        ("device", C.c_int32), ("force_global", C.c_int32), ("deterministic", C.c_int32),
    ]


class SphStats(C.Structure):
    _fields_ = [
        ("steps", C.c_int64), ("pair_interactions", C.c_int64), ("particle_num", C.c_int32),
        ("fluid_particle_num", C.c_int32), ("iter_divergence", C.c_int32), ("iter_density", C.c_int32),
        ("iter_pcisph", C.c_int32), ("iter_cg", C.c_int32), ("err_divergence", C.c_float),
        ("err_density", C.c_float), ("err_pcisph", C.c_float), ("err_cg", C.c_float),
        ("lds_fallback_blocks", C.c_int64), ("total_time", C.c_double), ("pair_evaluations", C.c_int64),
        ("hash_launches", C.c_int64), ("prehashed_sorts", C.c_int64), ("list_sorts", C.c_int64),
        ("carried_sorts", C.c_int64), ("iter_iisph", C.c_int32), ("err_iisph", C.c_float), ("pbf_recentred", C.c_int64),
    ]


class SphGridLayout(C.Structure):
    """The uniform grid in the library's frame and the sizes of its device tables (include/sph_hip.h)."""
    _fields_ = [
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("G", C.c_int32), ("scan_tile", C.c_int32),
        ("axis_map", C.c_int32 * 3), ("cell_size", C.c_float), ("n", C.c_int32), ("tiles", C.c_int32),
        ("tile_header_ints", C.c_int32), ("tiles_valid", C.c_int32),
    ]


GRID_CELL_START, GRID_TILE_HEADER, GRID_LANE_PERM, GRID_CELL_WORD = 0, 1, 2, 3   # SphGridTable


class SphRigidMotion(C.Structure):
    """A scripted body's program in canonical form (include/sph_hip.h): radians, unit-or-zero vectors, end = +inf for never."""
    _fields_ = [
        ("start", C.c_double), ("end", C.c_double), ("pivot", C.c_double * 3),
        ("nkeys", C.c_int32), ("interpolation", C.c_int32), ("repeat", C.c_int32), ("reserved", C.c_int32),
        ("key_times", C.c_double * 64), ("key_translations", C.c_double * 3 * 64), ("key_rotations", C.c_double * 3 * 64),
        ("frequency", C.c_double), ("phase", C.c_double), ("ramp", C.c_double),
        ("direction", C.c_double * 3), ("amplitude", C.c_double), ("axis", C.c_double * 3), ("angle", C.c_double),
        ("drift_velocity", C.c_double * 3), ("drift_axis", C.c_double * 3), ("drift_rate", C.c_double),
    ]


class SphRigidMotionState(C.Structure):
    _fields_ = [("com", C.c_double * 3), ("rot", C.c_double * 9), ("vel", C.c_double * 3), ("angvel", C.c_double * 3),
                ("force", C.c_double * 3), ("torque", C.c_double * 3), ("impulse", C.c_double * 3),
                ("angular_impulse", C.c_double * 3), ("steps", C.c_int64)]


def rigid_motion_state_dict(st):
    """A SphRigidMotionState as numpy arrays: com, rot[3, 3], vel, angvel, force, torque, impulse, angular_impulse, steps."""
    out = {k: np.array(getattr(st, k), np.float64) for k in ("com", "vel", "angvel", "force", "torque", "impulse", "angular_impulse")}
    out["rot"] = np.array(st.rot, np.float64).reshape(3, 3)
    out["steps"] = int(st.steps)
    return out


def rigid_motion_eval_host(program, com_rest, rot_rest, dt, k):
    """The device's evaluator run on the CPU (sph_rigid_motion_eval_host): pose and velocities of step k -> k + 1.  No device."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    c, r = f(com_rest), f(rot_rest)
    st = SphRigidMotionState()
    rc = load().sph_rigid_motion_eval_host(C.byref(program), _ptr(c), _ptr(r), float(dt), int(k), C.byref(st))
    if rc:
        raise SphError(f"sph_rigid_motion_eval_host failed ({rc}): " + (load().sph_last_error(None) or b"").decode(), rc)
    return rigid_motion_state_dict(st)


class SphEmitter(C.Structure):
    """A fluid emitter's program in canonical form (include/sph_hip.h): an orthonormal basis, end = +inf for never."""
    _fields_ = [
        ("object_id", C.c_int32), ("shape", C.c_int32), ("max_particles", C.c_int32), ("hold", C.c_int32),
        ("position", C.c_double * 3), ("direction", C.c_double * 3), ("tangent1", C.c_double * 3), ("tangent2", C.c_double * 3),
        ("width", C.c_double), ("height", C.c_double), ("radius", C.c_double), ("speed", C.c_double),
        ("start", C.c_double), ("end", C.c_double), ("density", C.c_double),
        ("color", C.c_int32 * 3), ("reserved", C.c_int32),
    ]


class SphEmitterState(C.Structure):
    _fields_ = [("object_id", C.c_int32), ("layer_particles", C.c_int32), ("max_layers", C.c_int32), ("layers", C.c_int32),
                ("emitted", C.c_int32), ("held_layers", C.c_int32), ("held_first", C.c_int32), ("exhausted", C.c_int32),
                ("held_id_base", C.c_int32 * 9), ("reserved", C.c_int32 * 3)]


class SphEmitterEval(C.Structure):
    _fields_ = [("T", C.c_double), ("s", C.c_double), ("born", C.c_int32), ("held_first", C.c_int32), ("held_layers", C.c_int32),
                ("layer_particles", C.c_int32), ("max_layers", C.c_int32), ("nu", C.c_int32), ("nv", C.c_int32), ("reserved", C.c_int32),
                ("layer_offset", C.c_double)]


def emitter_program(spec):
    """SphEmitter from a canonical emitter dict (scene.emitters_of)."""
    e = SphEmitter()
    e.object_id, e.shape = int(spec["objectId"]), EMITTER_SHAPES[spec["shape"]]
    e.max_particles, e.hold = int(spec["maxParticles"]), int(spec["hold"])
    for name, key in (("position", "position"), ("direction", "direction"), ("tangent1", "tangent1"), ("tangent2", "tangent2")):
        getattr(e, name)[:] = [float(x) for x in spec[key]]
    e.width, e.height, e.radius = float(spec["width"]), float(spec["height"]), float(spec["radius"])
    e.speed, e.start, e.end, e.density = float(spec["speed"]), float(spec["start"]), float(spec["end"]), float(spec["density"])
    e.color[:] = [int(c) for c in spec["color"]]
    return e


def emitter_eval_host(program, dt, spacing, k, layer=-1, positions=False):
    """The kernels' evaluator run on the CPU (sph_emitter_eval_host): the schedule after k steps as a dict and, with positions, the
    float32 positions (layer_particles, 3) of `layer` at that count.  No device."""
    out = SphEmitterEval()
    lib = load()
    rc = lib.sph_emitter_eval_host(C.byref(program), float(dt), float(spacing), int(k), -1, C.byref(out), None)
    xyz = None
    if not rc and (layer >= 0 or positions):
        xyz = np.zeros((out.layer_particles, 3), np.float32) if positions else None
        rc = lib.sph_emitter_eval_host(C.byref(program), float(dt), float(spacing), int(k), int(layer), C.byref(out), _ptr(xyz) if positions else None)
    if rc:
        raise SphError(f"sph_emitter_eval_host failed ({rc}): " + (lib.sph_last_error(None) or b"").decode(), rc)
    d = struct_dict(out, skip=("reserved",))
    return (d, xyz) if positions else d


MAX_OUTFLOWS = 8             # SPH_MAX_OUTFLOWS
OUTFLOW_MAX_OBJECTS = 16     # SPH_OUTFLOW_MAX_OBJECTS
OUTFLOW_SHAPES = {"box": 0, "sphere": 1}


class SphOutflow(C.Structure):
    """An outflow volume in canonical form (include/sph_hip.h): an axis-aligned box or a sphere, end = +inf for ever."""
    _fields_ = [
        ("shape", C.c_int32), ("invert", C.c_int32),
        ("min", C.c_double * 3), ("max", C.c_double * 3), ("center", C.c_double * 3), ("radius", C.c_double),
        ("start", C.c_double), ("end", C.c_double),
        ("n_objects", C.c_int32), ("objects", C.c_int32 * OUTFLOW_MAX_OBJECTS), ("reserved", C.c_int32),
    ]


class SphOutflowState(C.Structure):
    _fields_ = [("removed", C.c_int64), ("removed_last_step", C.c_int32), ("active", C.c_int32), ("reserved", C.c_int32 * 4)]


def outflow_program(spec):
    """SphOutflow from a canonical outflow dict (scene.outflows_of)."""
    v = SphOutflow()
    v.shape, v.invert = OUTFLOW_SHAPES[spec["shape"]], int(bool(spec["invert"]))
    v.min[:] = [float(x) for x in spec["min"]]
    v.max[:] = [float(x) for x in spec["max"]]
    v.center[:] = [float(x) for x in spec["center"]]
    v.radius, v.start, v.end = float(spec["radius"]), float(spec["start"]), float(spec["end"])
    objects = spec.get("objects") or []
    v.n_objects = len(objects)
    for k, o in enumerate(objects):
        v.objects[k] = int(o)
    return v


def outflow_test_host(program, xyz):
    """The kernels' predicate run on the CPU (sph_outflow_test_host): bool (n,) for float32 positions (n, 3); geometry and invert.
    No device."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    inside = np.zeros(len(xyz), np.uint8)
    lib = load()
    rc = lib.sph_outflow_test_host(C.byref(program), _ptr(xyz) if len(xyz) else None, len(xyz), _ptr(inside) if len(xyz) else None)
    if rc:
        raise SphError(f"sph_outflow_test_host failed ({rc}): " + (lib.sph_last_error(None) or b"").decode(), rc)
    return inside.astype(bool)


def outflow_active_host(program, dt, k):
    """The window test of a volume at step count k (sph_outflow_active_host).  No device."""
    lib = load()
    rc = lib.sph_outflow_active_host(C.byref(program), float(dt), int(k))
    if rc < 0:
        raise SphError(f"sph_outflow_active_host failed ({rc}): " + (lib.sph_last_error(None) or b"").decode(), rc)
    return bool(rc)


PBF_VARIANTS = {"reference": 0, "consistent": 1}


CFL_METHODS = {"none": 0, "velocity": 1}
CFL_CLAMPED_MAX, CFL_CLAMPED_MIN, CFL_LANDING, CFL_STALE = 1, 2, 4, 8   # SphTimeState::flags


class SphCflParams(C.Structure):
    """Adaptive time stepping (include/sph_hip.h): the method, cflFactor and the clamps of the step size."""
    _fields_ = [("method", C.c_int32), ("reserved", C.c_int32), ("factor", C.c_double), ("min_dt", C.c_double), ("max_dt", C.c_double)]


class SphTimeState(C.Structure):
    _fields_ = [("time", C.c_double), ("dt_next", C.c_double), ("dt_last", C.c_double), ("target", C.c_double), ("vmax2", C.c_float),
                ("flags", C.c_int32), ("steps", C.c_int64), ("reserved", C.c_int32 * 4)]


def cfl_params(method="velocity", factor=0.5, min_dt=0.0, max_dt=0.0):
    return SphCflParams(int(CFL_METHODS.get(method, method)), 0, float(factor), float(min_dt), float(max_dt))


def cfl_dt_host(params, diameter, vmax2, remaining=float("nan")):
    """The rule on the CPU (sph_cfl_dt_host): (dt, flags) for a float32 maximum of |v|^2; remaining not finite: no time target.
    No device."""
    lib = load()
    dt, flags = C.c_double(), C.c_int32()
    rc = lib.sph_cfl_dt_host(C.byref(params), float(diameter), C.c_float(vmax2), float(remaining), C.byref(dt), C.byref(flags))
    if rc != 0:
        raise SphError(f"sph_cfl_dt_host failed ({rc}): " + (lib.sph_last_error(None) or b"").decode(), rc)
    return dt.value, flags.value


def cfl_meta(material, is_dynamic, ghost=None, removed=None):
    """The particle words sph_cfl_speed2_host takes, from per-particle materials and dynamic flags."""
    m = (np.asarray(material, np.int32) << 8) | ((np.asarray(is_dynamic, np.int32) != 0).astype(np.int32) << 10)
    if ghost is not None:
        m = m | ((np.asarray(ghost, np.int32) != 0).astype(np.int32) << 11)
    if removed is not None:
        m = m | ((np.asarray(removed, np.int32) != 0).astype(np.int32) << 12)
    return np.ascontiguousarray(m, np.int32)


def cfl_speed2_host(vel, meta):
    """The reduce on the CPU (sph_cfl_speed2_host): (float32 maximum of |v|^2 over the particles that count, non-finite flag).
    No device."""
    lib = load()
    vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 3)
    meta = np.ascontiguousarray(meta, np.int32).reshape(-1)
    assert len(vel) == len(meta)
    v, bad = C.c_float(), C.c_int32()
    rc = lib.sph_cfl_speed2_host(len(vel), _ptr(vel) if len(vel) else None, _ptr(meta) if len(vel) else None, C.byref(v), C.byref(bad))
    if rc != 0:
        raise SphError(f"sph_cfl_speed2_host failed ({rc}): " + (lib.sph_last_error(None) or b"").decode(), rc)
    return np.float32(v.value), bool(bad.value)


class SphPbfParams(C.Structure):
    _fields_ = [("variant", C.c_int32), ("min_iterations", C.c_int32), ("max_iterations", C.c_int32), ("max_error", C.c_float),
                ("epsilon", C.c_float)]


SURFACE_TENSION_METHODS = {"reference": 0, "akinci": 1}


class SphSurfaceTensionParams(C.Structure):
    _fields_ = [("method", C.c_int32), ("gamma", C.c_double), ("beta", C.c_double)]


def surface_tension_kernels_host(h, r, fast=False):
    """(C(r), A(r)) of the Akinci splines from the kernels' own source run on the CPU (sph_surface_tension_kernels_host), float32.
    No device."""
    r = np.ascontiguousarray(r, dtype=np.float32).reshape(-1)
    c_out, a_out = np.empty_like(r), np.empty_like(r)
    rc = load().sph_surface_tension_kernels_host(float(h), _ptr(r), r.shape[0], _ptr(c_out), _ptr(a_out), int(bool(fast)))
    if rc:
        raise SphError(f"sph_surface_tension_kernels_host failed ({rc}): " + (load().sph_last_error(None) or b"").decode(), rc)
    return c_out, a_out


THERMAL_METHODS = {"none": 0, "conduction": 1}


class SphThermal(C.Structure):
    _fields_ = [("method", C.c_int32), ("alpha", C.c_double), ("beta", C.c_double), ("t_ref", C.c_double)]


def heat_pair_host(records, fast=False):
    """The heat walk's pair arithmetic from the kernels' own source run on the CPU (sph_heat_pair_host): records (n, 12) float32 =
    (T_i, c_j, T_j, dx, dy, dz, r2, eps, gs, gx, gy, gz) -> (n,) float32, each pair's term c_j (T_i - T_j) F_ij.  No device."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 12)
    out = np.empty(rec.shape[0], np.float32)
    rc = load().sph_heat_pair_host(_ptr(rec), rec.shape[0], _ptr(out), int(bool(fast)))
    if rc:
        raise SphError(f"sph_heat_pair_host failed ({rc}): " + (load().sph_last_error(None) or b"").decode(), rc)
    return out


def heat_finish_host(records, fast=False):
    """What follows the walk's sum and the buoyancy (heat_finish, heat_buoyancy of csrc/sph_thermal.hpp) run on the CPU
    (sph_heat_finish_host): records (n, 12) float32 = (sum, 2 alpha, rho0, rho_i, dt, T_i, -beta, T_ref, g[3], unused) -> (n, 5)
    float32 = (dT/dt, T_new, a_b[3]).  No device."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 12)
    out = np.empty((rec.shape[0], 5), np.float32)
    rc = load().sph_heat_finish_host(_ptr(rec), rec.shape[0], _ptr(out), int(bool(fast)))
    if rc:
        raise SphError(f"sph_heat_finish_host failed ({rc}): " + (load().sph_last_error(None) or b"").decode(), rc)
    return out


VORTICITY_METHODS = {"none": 0, "micropolar": 1}


class SphMicropolarParams(C.Structure):
    _fields_ = [("method", C.c_int32), ("nu_t", C.c_double), ("zeta", C.c_double), ("theta_inv", C.c_double)]


def micropolar_pair_host(records, fast=False):
    """The micropolar walk's pair arithmetic from the kernels' own source run on the CPU (sph_micropolar_pair_host): records (n, 24)
    float32 as sph_hip.h lists them -> (n, 6) float32, each pair's share of the two sums.  No device."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 24)
    out = np.empty((rec.shape[0], 6), np.float32)
    rc = load().sph_micropolar_pair_host(_ptr(rec), rec.shape[0], _ptr(out), int(bool(fast)))
    if rc:
        raise SphError(f"sph_micropolar_pair_host failed ({rc}): " + (load().sph_last_error(None) or b"").decode(), rc)
    return out


class SphElasticParams(C.Structure):
    _fields_ = [("youngs_modulus", C.c_double), ("poisson_ratio", C.c_double)]


class SphElasticObjectInfo(C.Structure):
    _fields_ = [("captured", C.c_int32), ("count", C.c_int32), ("first_id", C.c_int32), ("longest_list", C.c_int32),
                ("min_eig_ratio", C.c_float), ("params", SphElasticParams)]


def elastic_lame(E, nu):
    """(mu, lambda) of Young's modulus E and Poisson's ratio nu."""
    return E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))


def elastic_particle_host(xi, xj, g0_ij, g0_ji, q_prev, q_j, sigma_j, V0, mass, mu, lam, fast=False):
    """Passes A and B of one elastic particle from the kernels' own source run on the CPU (sph_elastic_particle_host): the list's
    current positions xj (k, 3), rest vectors g0_ij / g0_ji (k, 3), the neighbours' pass-A results q_j (k, 4) and sigma_j (k, 6), the
    particle's position xi and warm start q_prev -> (F (3, 3), q (4,), sigma (6,), a_el (3,)).  No device."""
    f = lambda a, c: np.ascontiguousarray(a, dtype=np.float32).reshape(-1, c)
    xj, g0_ij, g0_ji, q_j, sigma_j = f(xj, 3), f(g0_ij, 3), f(g0_ji, 3), f(q_j, 4), f(sigma_j, 6)
    k = xj.shape[0]
    if not (g0_ij.shape[0] == g0_ji.shape[0] == q_j.shape[0] == sigma_j.shape[0] == k):
        raise ValueError("elastic_particle_host: the list arrays differ in length")
    xi = np.ascontiguousarray(xi, dtype=np.float32).reshape(3)
    q_prev = np.ascontiguousarray(q_prev, dtype=np.float32).reshape(4)
    F, q, sig, a = np.empty(9, np.float32), np.empty(4, np.float32), np.empty(6, np.float32), np.empty(3, np.float32)
    rc = load().sph_elastic_particle_host(k, _ptr(xi), _ptr(xj), _ptr(g0_ij), _ptr(g0_ji), _ptr(q_prev), _ptr(q_j), _ptr(sigma_j),
                                          float(V0), float(mass), float(mu), float(lam), _ptr(F), _ptr(q), _ptr(sig), _ptr(a),
                                          int(bool(fast)))
    if rc:
        raise SphError(f"sph_elastic_particle_host failed ({rc}): " + (load().sph_last_error(None) or b"").decode(), rc)
    return F.reshape(3, 3), q, sig, a


DRAG_METHODS = {"none": 0, "gissler": 1}


class SphDragParams(C.Structure):
    _fields_ = [("method", C.c_int32), ("k", C.c_double), ("rho_air", C.c_double), ("air_velocity", C.c_double * 3)]


def _drag_params(method, k, rho_air, air_velocity):
    u = np.asarray(air_velocity, np.float64).reshape(3)
    return SphDragParams(int(DRAG_METHODS.get(method, method)), float(k), float(rho_air), (C.c_double * 3)(*u))


def drag_particle_host(records, radius, rho0, k=1.0, rho_air=1.2041, air_velocity=(0.0, 0.0, 0.0), fast=False):
    """Everything behind the air drag's walk (drag_finish of csrc/sph_drag.hpp) from the kernels' own source run on the CPU
    (sph_drag_particle_host): records (n, 6) float32 = (v_i[3], m_i, n_i, q) -> (n, 7) float32 = (a_drag[3], w, C_D, A_un, y).  No device."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 6)
    out = np.empty((rec.shape[0], 7), np.float32)
    p = _drag_params("gissler", k, rho_air, air_velocity)
    rc = load().sph_drag_particle_host(C.byref(p), float(radius), float(rho0), rec.shape[0], _ptr(rec), _ptr(out), int(bool(fast)))
    if rc:
        raise SphError(f"sph_drag_particle_host failed ({rc}): " + (load().sph_last_error(None) or b"").decode(), rc)
    return out


def drag_constants_host(radius, rho0, rho_air=1.2041):
    """The air drag's per-handle constants as the library derives them (sph_drag_constants_host): dict(L, inv_td, omega2, t_max, c_def,
    y_coeff, n23, re_coeff).  SphError (ERR_INVALID) where omega^2 <= 0.  No device."""
    out = np.zeros(8, np.float64)
    p = _drag_params("gissler", 1.0, rho_air, (0.0, 0.0, 0.0))
    rc = load().sph_drag_constants_host(C.byref(p), float(radius), float(rho0), _ptr(out))
    if rc:
        raise SphError(f"sph_drag_constants_host failed ({rc}): " + (load().sph_last_error(None) or b"").decode(), rc)
    return dict(zip(("L", "inv_td", "omega2", "t_max", "c_def", "y_coeff", "n23", "re_coeff"), (float(v) for v in out)))


class SphPbfStats(C.Structure):
    _fields_ = [("variant", C.c_int32), ("iterations", C.c_int32), ("error", C.c_float)]


class SphSurfaceParams(C.Structure):
    _fields_ = [
        ("radius", C.c_double), ("smoothing_length", C.c_double), ("cube_size", C.c_double), ("iso", C.c_double),
        ("normals", C.c_int32), ("fast_math", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32),
        ("memory_cap_bytes", C.c_int64),
    ]


class SphSurfaceStats(C.Structure):
    _fields_ = [
        ("particles", C.c_int64), ("active_bricks", C.c_int64), ("points_evaluated", C.c_int64), ("pair_tests", C.c_int64),
        ("vertices", C.c_int64), ("triangles", C.c_int64), ("bytes_allocated", C.c_int64), ("B", C.c_int32), ("reserved", C.c_int32),
        ("ms_bin", C.c_double), ("ms_bricks", C.c_double), ("ms_field", C.c_double), ("ms_mesh", C.c_double),
        ("ms_normals", C.c_double), ("ms_total", C.c_double),
    ]


class SphSurfacePostParams(C.Structure):
    _fields_ = [
        ("mesh_smoothing_iters", C.c_int32), ("mesh_smoothing_weights", C.c_int32), ("weights_normalization", C.c_double),
        ("normals_smoothing_iters", C.c_int32), ("reserved", C.c_int32),
    ]


class SphSurfacePostStats(C.Structure):
    _fields_ = [
        ("adjacency_entries", C.c_int64), ("max_degree", C.c_int32), ("reserved", C.c_int32), ("ms_adjacency", C.c_double),
        ("ms_weights", C.c_double), ("ms_smoothing", C.c_double), ("ms_normals", C.c_double), ("ms_normal_smoothing", C.c_double),
        ("ms_total", C.c_double),
    ]


class SphSurfaceAnisoParams(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("min_neighbours", C.c_int32), ("max_ratio", C.c_double), ("sparse_scale", C.c_double)]


class SphSurfaceAnisoStats(C.Structure):
    _fields_ = [("sparse_particles", C.c_int64), ("clamped_particles", C.c_int64), ("ms_moments", C.c_double), ("ms_volume", C.c_double)]


class SphRenderParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("eye", C.c_double * 3), ("target", C.c_double * 3), ("up", C.c_double * 3),
        ("fov_deg", C.c_double), ("z_near", C.c_double), ("radius", C.c_double), ("light_pos", C.c_double * 3),
        ("light_rgb", C.c_double * 3), ("ambient", C.c_double), ("background_rgb", C.c_int32 * 3), ("draw_box", C.c_int32),
        ("box_lo", C.c_double * 3), ("box_hi", C.c_double * 3), ("box_rgb", C.c_int32 * 3), ("fast_math", C.c_int32),
        ("device", C.c_int32), ("reserved", C.c_int32),
    ]


class SphRenderStats(C.Structure):
    _fields_ = [
        ("particles", C.c_int64), ("drawn", C.c_int64), ("skipped_nonfinite", C.c_int64), ("large", C.c_int64),
        ("atomics", C.c_int64), ("covered_pixels", C.c_int64),
        ("ms_input", C.c_double), ("ms_splat", C.c_double), ("ms_shade", C.c_double), ("ms_total", C.c_double),
    ]


class SphRenderCompositeStats(C.Structure):
    _fields_ = [
        ("ranks", C.c_int32), ("hops", C.c_int32), ("pieces_sent", C.c_int64), ("pieces_recv", C.c_int64),
        ("bytes_sent", C.c_int64), ("bytes_recv", C.c_int64), ("drawn_global", C.c_int64), ("ms_composite", C.c_double),
    ]


class SphRenderSurfaceParams(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32), ("rmax", C.c_int32), ("sigma", C.c_double), ("range", C.c_double), ("spec", C.c_double),
        ("shininess", C.c_double), ("object_mask", C.c_int64),
    ]


class SphRenderSurfaceStats(C.Structure):
    _fields_ = [
        ("surface_pixels", C.c_int64), ("iterations", C.c_int64), ("taps_visited", C.c_int64), ("taps_accepted", C.c_int64),
        ("clamped_rmax", C.c_int64), ("ms_base", C.c_double), ("ms_smooth", C.c_double), ("ms_shade", C.c_double),
    ]


class SphRenderThicknessParams(C.Structure):
    _fields_ = [("absorb", C.c_float), ("scatter", C.c_float), ("iterations", C.c_int32)]


class SphRenderThicknessStats(C.Structure):
    _fields_ = [
        ("adds", C.c_int64), ("clipped", C.c_int64), ("removed", C.c_int64), ("empty_pixels", C.c_int64), ("max_thickness", C.c_int64),
        ("iterations", C.c_int64), ("taps_visited", C.c_int64), ("ms_opaque", C.c_double), ("ms_splat", C.c_double),
        ("ms_smooth", C.c_double), ("ms_shade", C.c_double),
    ]


class SphRenderSurfaceFoamParams(C.Structure):
    _fields_ = [("radius_scale", C.c_double), ("density", C.c_double), ("depth_bias", C.c_double), ("rgb", C.c_uint8 * 3),
                ("raw_spheres", C.c_uint8), ("reserved", C.c_int32)]


class SphRenderSurfaceFoamStats(C.Structure):
    _fields_ = [
        ("diffuse", C.c_int64), ("large", C.c_int64), ("adds_over", C.c_int64), ("adds_under", C.c_int64), ("clipped", C.c_int64),
        ("removed", C.c_int64), ("pixels_over", C.c_int64), ("pixels_under", C.c_int64), ("ms_splat", C.c_double), ("ms_raw", C.c_double),
        ("ms_composite", C.c_double),
    ]


class SphRenderMeshStats(C.Structure):
    _fields_ = [
        ("meshes", C.c_int64), ("triangles", C.c_int64), ("vertices", C.c_int64), ("large", C.c_int64),
        ("skipped_nonfinite", C.c_int64), ("skipped_degenerate", C.c_int64), ("bad_index", C.c_int64), ("atomics", C.c_int64),
        ("covered_pixels", C.c_int64), ("hit", C.c_int64),
        ("ms_depth", C.c_double), ("ms_shade", C.c_double), ("ms_finish", C.c_double), ("ms_total", C.c_double),
    ]


class SphRenderTraceParams(C.Structure):
    _fields_ = [
        ("max_depth", C.c_int32), ("ior", C.c_float), ("absorb", C.c_float), ("shadows", C.c_int32), ("floor", C.c_int32),
        ("floor_cell", C.c_float), ("use_bvh", C.c_int32), ("record", C.c_int32),
    ]


class SphRenderTraceStats(C.Structure):
    _fields_ = [
        ("triangles", C.c_int64), ("nodes", C.c_int64), ("depth", C.c_int64), ("skipped_nonfinite", C.c_int64),
        ("skipped_degenerate", C.c_int64), ("bad_index", C.c_int64), ("rays_primary", C.c_int64), ("rays_path", C.c_int64),
        ("rays_reflect", C.c_int64), ("rays_shadow", C.c_int64), ("node_visits", C.c_int64), ("triangle_tests", C.c_int64),
        ("truncated", C.c_int64), ("aborted_rays", C.c_int64),
        ("ms_setup", C.c_double), ("ms_sort", C.c_double), ("ms_hierarchy", C.c_double), ("ms_fit", C.c_double), ("ms_trace", C.c_double),
        ("ms_finish", C.c_double), ("ms_total", C.c_double),
    ]


RENDER_MATERIALS = {"diffuse": 0, "water": 1}   # SPH_RENDER_MATERIAL_*
RENDER_TRACE_FLOOR_ID = -14                      # SPH_RENDER_TRACE_FLOOR_ID
RENDER_TRACE_SEGMENT_WORDS = 24                  # SPH_RENDER_TRACE_SEGMENT_WORDS


class SphVideoParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("quality", C.c_int32), ("chroma", C.c_int32), ("fast_math", C.c_int32),
        ("device", C.c_int32), ("reserved", C.c_int32),
    ]


class SphVideoStats(C.Structure):
    _fields_ = [
        ("blocks", C.c_int64), ("scan_bytes", C.c_int64), ("stuffed_bytes", C.c_int64), ("restart_intervals", C.c_int64),
        ("ms_input", C.c_double), ("ms_count", C.c_double), ("ms_scan", C.c_double), ("ms_write", C.c_double), ("ms_total", C.c_double),
    ]


class SphPngParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("filter", C.c_int32), ("fast_math", C.c_int32), ("device", C.c_int32),
        ("reserved", C.c_int32),
    ]


class SphPngStats(C.Structure):
    _fields_ = [
        ("raw_bytes", C.c_int64), ("zlib_bytes", C.c_int64), ("file_bytes", C.c_int64), ("segments", C.c_int64),
        ("stored_segments", C.c_int64), ("literals", C.c_int64), ("matches", C.c_int64), ("filter_rows", C.c_int64 * 5),
        ("ms_input", C.c_double), ("ms_filter", C.c_double), ("ms_count", C.c_double), ("ms_scan", C.c_double), ("ms_write", C.c_double),
        ("ms_total", C.c_double), ("dynamic_segments", C.c_int64), ("dynamic_header_bits", C.c_int64),
    ]


class SphPngWindowStats(C.Structure):
    _fields_ = [
        ("window_segments", C.c_int64), ("window_matches", C.c_int64), ("window_far_matches", C.c_int64), ("window_header_bits", C.c_int64),
        ("ms_candidates", C.c_double),
    ]


PNG_CODING_FIXED, PNG_CODING_DYNAMIC = 0, 1
PNG_CODING_WINDOW = 3   # (2 is no coding: the library refuses it)


class SphTextParams(C.Structure):
    _fields_ = [("piece_rows", C.c_int32), ("fast_math", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32)]


class SphTextStats(C.Structure):
    _fields_ = [
        ("rows", C.c_int64), ("values", C.c_int64), ("bytes", C.c_int64), ("pieces", C.c_int64), ("longest_row", C.c_int64),
        ("ms_source", C.c_double), ("ms_count", C.c_double), ("ms_scan", C.c_double), ("ms_write", C.c_double), ("ms_copy", C.c_double),
        ("ms_file", C.c_double), ("ms_total", C.c_double),
    ]


class SphFoamParams(C.Structure):
    _fields_ = [
        ("radius", C.c_double), ("domain_lo", C.c_double * 3), ("domain_hi", C.c_double * 3), ("padding", C.c_double),
        ("gravity", C.c_double * 3),
        ("ta_min", C.c_double), ("ta_max", C.c_double), ("wc_min", C.c_double), ("wc_max", C.c_double),
        ("e_min", C.c_double), ("e_max", C.c_double), ("k_ta", C.c_double), ("k_wc", C.c_double),
        ("life_min", C.c_double), ("life_max", C.c_double), ("k_b", C.c_double), ("k_d", C.c_double), ("normal_min", C.c_double),
        ("n_spray", C.c_int32), ("n_bubble", C.c_int32), ("max_per_particle", C.c_int32), ("fast_math", C.c_int32),
        ("device", C.c_int32), ("reserved", C.c_int32), ("max_diffuse", C.c_int64), ("seed", C.c_uint64),
    ]


class SphFoamStats(C.Structure):
    _fields_ = [
        ("step", C.c_int64), ("fluid", C.c_int64), ("diffuse", C.c_int64), ("spray", C.c_int64), ("foam", C.c_int64), ("bubble", C.c_int64),
        ("born", C.c_int64), ("died", C.c_int64), ("dropped", C.c_int64),
        ("born_total", C.c_int64), ("died_total", C.c_int64), ("dropped_total", C.c_int64),
        ("pairs_visited", C.c_int64 * 3), ("pairs_accepted", C.c_int64 * 3), ("bytes_allocated", C.c_int64),
        ("ms_grid", C.c_double), ("ms_advect", C.c_double), ("ms_normals", C.c_double), ("ms_potentials", C.c_double),
        ("ms_generate", C.c_double), ("ms_total", C.c_double),
    ]


# return codes (include/sph_hip.h)
ERR_INVALID, ERR_CAPACITY = -1, -2
ERR_UNSUPPORTED = -6


class SphError(RuntimeError):
    """.code: the library's return code (None: raised on the Python side of the binding)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def struct_dict(st, skip=()):
    """The fields of a ctypes structure as a dict."""
    return {k: getattr(st, k) for k, _ in st._fields_ if k not in skip}


_lib = None

# every symbol include/sph_hip.h declares: (name, restype, argtypes)
_VP = C.c_void_p
_SIGNATURES = [
    ("sph_create", C.c_int, [C.POINTER(SphParams), C.POINTER(_VP)]),
    ("sph_destroy", None, [_VP]),
    ("sph_last_error", C.c_char_p, [_VP]),
    ("sph_append_particles", C.c_int, [_VP, C.c_int, C.c_int] + [_VP] * 7),
    ("sph_set_appended_ids", C.c_int, [_VP, C.c_int, _VP]),
    ("sph_set_object", C.c_int, [_VP, C.c_int, C.c_int, C.c_int]),
    ("sph_set_rigid_pose", C.c_int, [_VP, C.c_int] + [_VP] * 5),
    ("sph_get_rigid_wrench", C.c_int, [_VP, _VP, _VP, C.c_int]),
    ("sph_set_rigid_contact", C.c_int, [_VP, C.c_int, C.c_float, _VP, _VP]),
    ("sph_get_rigid_contacts", C.c_int, [_VP, _VP, C.c_int]),
    ("sph_get_rigid_contact_pairs", C.c_int, [_VP, C.POINTER(C.c_int64)]),
    ("sph_set_pbf_variant", C.c_int, [_VP, C.POINTER(SphPbfParams)]),
    ("sph_get_pbf_stats", C.c_int, [_VP, C.POINTER(SphPbfStats)]),
    ("sph_set_surface_tension", C.c_int, [_VP, C.POINTER(SphSurfaceTensionParams)]),
    ("sph_get_surface_tension", C.c_int, [_VP, C.POINTER(SphSurfaceTensionParams)]),
    ("sph_surface_tension_kernels_host", C.c_int, [C.c_double, _VP, C.c_int64, _VP, _VP, C.c_int]),
    ("sph_set_micropolar", C.c_int, [_VP, C.POINTER(SphMicropolarParams)]),
    ("sph_get_micropolar", C.c_int, [_VP, C.POINTER(SphMicropolarParams)]),
    ("sph_micropolar_pair_host", C.c_int, [_VP, C.c_int64, _VP, C.c_int]),
    ("sph_set_drag", C.c_int, [_VP, C.POINTER(SphDragParams)]),
    ("sph_get_drag", C.c_int, [_VP, C.POINTER(SphDragParams)]),
    ("sph_drag_particle_host", C.c_int, [C.POINTER(SphDragParams), C.c_double, C.c_double, C.c_int64, _VP, _VP, C.c_int]),
    ("sph_drag_constants_host", C.c_int, [C.POINTER(SphDragParams), C.c_double, C.c_double, _VP]),
    ("sph_set_elastic_object", C.c_int, [_VP, C.c_int, C.POINTER(SphElasticParams)]),
    ("sph_get_elastic_object", C.c_int, [_VP, C.c_int, C.POINTER(SphElasticObjectInfo)]),
    ("sph_get_elastic_rest", C.c_int, [_VP, C.c_int, _VP, _VP, _VP]),
    ("sph_elastic_particle_host", C.c_int, [C.c_int] + [_VP] * 7 + [C.c_double] * 4 + [_VP] * 4 + [C.c_int]),
    # device rigid integrator; what each stands in for in the reference's SPH/rigid_solver/bullet_solver.py:
    ("sph_set_rigid_integrator", C.c_int, [_VP, C.c_int, _VP, _VP, _VP]),                        # :19-71 __init__ (gravity, dt, walls)
    ("sph_set_rigid_body", C.c_int, [_VP, C.c_int, C.c_double] + [_VP] * 7 + [C.c_int]),        # :75-131 insert_rigid_object
    ("sph_get_rigid_state", C.c_int, [_VP, C.c_int, _VP, _VP, _VP, _VP]),                        # :158-176 pose read-back
    ("sph_rigid_integrate", C.c_int, [_VP]),                                                     # :144-167 step
    # device contact solver: ContactSolver.__init__ + slop / patch, and the rows of the last solve
    ("sph_set_rigid_contact_solver", C.c_int, [_VP, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double]),
    ("sph_get_rigid_contact_rows", C.c_int, [_VP, _VP, C.c_int, _VP]),
    # scripted rigid bodies
    ("sph_set_rigid_motion", C.c_int, [_VP, C.c_int, C.POINTER(SphRigidMotion), _VP, _VP, _VP]),
    ("sph_get_rigid_motion_state", C.c_int, [_VP, C.c_int, C.POINTER(SphRigidMotionState)]),
    ("sph_rigid_motion_eval_host", C.c_int, [C.POINTER(SphRigidMotion), _VP, _VP, C.c_double, C.c_int64, C.POINTER(SphRigidMotionState)]),
    ("sph_set_emitter", C.c_int, [_VP, C.c_int, C.POINTER(SphEmitter)]),
    ("sph_get_emitter_state", C.c_int, [_VP, C.c_int, C.POINTER(SphEmitterState)]),
    ("sph_emitter_eval_host", C.c_int, [C.POINTER(SphEmitter), C.c_double, C.c_double, C.c_int64, C.c_int, C.POINTER(SphEmitterEval), _VP]),
    ("sph_set_outflow", C.c_int, [_VP, C.c_int, C.POINTER(SphOutflow)]),
    ("sph_get_outflow_state", C.c_int, [_VP, C.c_int, C.POINTER(SphOutflowState)]),
    ("sph_remove_particles", C.c_int, [_VP, _VP, C.c_int]),
    ("sph_outflow_test_host", C.c_int, [C.POINTER(SphOutflow), _VP, C.c_int, _VP]),
    ("sph_outflow_active_host", C.c_int, [C.POINTER(SphOutflow), C.c_double, C.c_int64]),
    ("sph_set_time_step", C.c_int, [_VP, C.c_double]),
    ("sph_set_thermal", C.c_int, [_VP, C.POINTER(SphThermal)]),
    ("sph_get_thermal", C.c_int, [_VP, C.POINTER(SphThermal)]),
    ("sph_set_object_temperature", C.c_int, [_VP, C.c_int, C.c_double, C.c_int]),
    ("sph_heat_pair_host", C.c_int, [_VP, C.c_int64, _VP, C.c_int]),
    ("sph_heat_finish_host", C.c_int, [_VP, C.c_int64, _VP, C.c_int]),
    ("sph_set_cfl", C.c_int, [_VP, C.POINTER(SphCflParams)]),
    ("sph_get_cfl", C.c_int, [_VP, C.POINTER(SphCflParams)]),
    ("sph_get_time_state", C.c_int, [_VP, C.POINTER(SphTimeState)]),
    ("sph_set_time_target", C.c_int, [_VP, C.c_double]),
    ("sph_advance_until", C.c_int, [_VP, C.c_double, C.c_int, C.POINTER(C.c_int)]),
    ("sph_cfl_dt_host", C.c_int, [C.POINTER(SphCflParams), C.c_double, C.c_float, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    ("sph_cfl_speed2_host", C.c_int, [C.c_int64, _VP, _VP, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    ("sph_prepare", C.c_int, [_VP]),
    ("sph_step", C.c_int, [_VP, C.c_int]),
    ("sph_step_async", C.c_int, [_VP, C.c_int]),
    ("sph_synchronize", C.c_int, [_VP]),
    ("sph_step_begin", C.c_int, [_VP]),
    ("sph_step_end", C.c_int, [_VP]),
    ("sph_run_phase", C.c_int, [_VP, C.c_int]),
    ("sph_download", C.c_int, [_VP, C.c_int, _VP, C.c_size_t]),
    ("sph_upload", C.c_int, [_VP, C.c_int, _VP, C.c_size_t]),
    ("sph_particle_num", C.c_int, [_VP]),
    ("sph_fluid_particle_num", C.c_int, [_VP]),
    ("sph_get_stats", C.c_int, [_VP, C.POINTER(SphStats)]),
    ("sph_get_cg_scalars", C.c_int, [_VP, C.POINTER(C.c_float)]),
    ("sph_profile_enable", C.c_int, [_VP, C.c_int, C.c_int]),
    ("sph_profile_reset", C.c_int, [_VP]),
    ("sph_profile_read", C.c_int, [_VP, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    ("sph_kernel_name", C.c_char_p, [C.c_int]),
    ("sph_device_info", C.c_int, [_VP, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    ("sph_measure_copy_rate", C.c_int, [_VP, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    ("sph_comm_unique_id", C.c_int, [_VP]),
    ("sph_comm_init", C.c_int, [_VP, C.c_int, C.c_int, _VP]),
    ("sph_comm_transport", C.c_char_p, [_VP]),
    ("sph_comm_set_slab", C.c_int, [_VP, C.c_int, C.c_int]),
    ("sph_comm_get_slab", C.c_int, [_VP] + [C.POINTER(C.c_int)] * 4),
    ("sph_comm_set_rebalance", C.c_int, [_VP, C.c_int]),
    ("sph_comm_add_global_count", C.c_int, [_VP, C.c_int, C.c_int]),
    ("sph_device_count", C.c_int, []),
    ("sph_voxelize_mesh", C.c_int, [_VP, C.c_int, _VP, C.c_int, C.c_double, _VP, C.c_int64, C.POINTER(C.c_int64)]),
    ("sph_points_in_mesh", C.c_int, [_VP, C.c_int, _VP, C.c_int] + [_VP, C.c_int] * 3 + [_VP]),
    ("sph_write_ply_ascii", C.c_int, [C.c_char_p, _VP, C.c_int64]),
    ("sph_write_ply_ascii_part", C.c_int, [C.c_char_p, _VP, C.c_int64, C.c_int64, C.c_int]),
    ("sph_format_f32", C.c_int, [C.c_float, C.c_char_p]),
    ("sph_write_obj_ascii", C.c_int, [C.c_char_p, _VP, C.c_int64, _VP, _VP, C.c_int64]),
    ("sph_surface_create", C.c_int, [C.POINTER(SphSurfaceParams), C.POINTER(_VP)]),
    ("sph_surface_destroy", None, [_VP]),
    ("sph_surface_last_error", C.c_char_p, [_VP]),
    ("sph_surface_reconstruct", C.c_int, [_VP, _VP, C.c_int64]),
    ("sph_surface_reconstruct_object", C.c_int, [_VP, _VP, C.c_int]),
    ("sph_surface_mesh_size", C.c_int, [_VP, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("sph_surface_download", C.c_int, [_VP, _VP, _VP, _VP]),
    ("sph_surface_stats", C.c_int, [_VP, C.POINTER(SphSurfaceStats)]),
    ("sph_surface_set_postprocess", C.c_int, [_VP, C.POINTER(SphSurfacePostParams)]),
    ("sph_surface_post_stats", C.c_int, [_VP, C.POINTER(SphSurfacePostStats)]),
    ("sph_surface_download_post", C.c_int, [_VP, _VP, _VP, _VP]),
    ("sph_surface_set_anisotropy", C.c_int, [_VP, C.POINTER(SphSurfaceAnisoParams)]),
    ("sph_surface_anisotropy_stats", C.c_int, [_VP, C.POINTER(SphSurfaceAnisoStats)]),
    ("sph_surface_download_anisotropy", C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    ("sph_surface_aniso_matrix_host", C.c_int, [_VP, C.c_int64, _VP, C.POINTER(SphSurfaceAnisoParams), _VP]),
    ("sph_render_create", C.c_int, [C.POINTER(SphRenderParams), C.POINTER(_VP)]),
    ("sph_render_destroy", None, [_VP]),
    ("sph_render_last_error", C.c_char_p, [_VP]),
    ("sph_render_points", C.c_int, [_VP, _VP, _VP, _VP, C.c_int64]),
    ("sph_render_handle", C.c_int, [_VP, _VP, C.c_uint32]),
    ("sph_render_download", C.c_int, [_VP, _VP, _VP]),
    ("sph_render_stats", C.c_int, [_VP, C.POINTER(SphRenderStats)]),
    ("sph_render_layer_download", C.c_int, [_VP, _VP, _VP]),
    ("sph_render_layer_merge", C.c_int, [_VP, _VP, _VP]),
    ("sph_render_composite_stats", C.c_int, [_VP, C.POINTER(SphRenderCompositeStats)]),
    ("sph_render_set_surface", C.c_int, [_VP, C.POINTER(SphRenderSurfaceParams)]),
    ("sph_render_points_surface_mask", C.c_int, [_VP, _VP, C.c_int]),
    ("sph_render_surface", C.c_int, [_VP]),
    ("sph_render_surface_download_depth", C.c_int, [_VP, _VP]),
    ("sph_render_surface_stats", C.c_int, [_VP, C.POINTER(SphRenderSurfaceStats)]),
    ("sph_render_set_thickness", C.c_int, [_VP, C.POINTER(SphRenderThicknessParams)]),
    ("sph_render_surface_download_thickness", C.c_int, [_VP, _VP, C.c_int]),
    ("sph_render_surface_download_opaque", C.c_int, [_VP, _VP, _VP]),
    ("sph_render_thickness_stats", C.c_int, [_VP, C.POINTER(SphRenderThicknessStats)]),
    ("sph_render_mesh_begin", C.c_int, [_VP]),
    ("sph_render_mesh_add", C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int64, _VP]),
    ("sph_render_mesh_add_surface", C.c_int, [_VP, _VP, _VP]),
    ("sph_render_mesh_end", C.c_int, [_VP]),
    ("sph_render_mesh_stats", C.c_int, [_VP, C.POINTER(SphRenderMeshStats)]),
    ("sph_render_set_trace", C.c_int, [_VP, C.POINTER(SphRenderTraceParams)]),
    ("sph_render_mesh_material", C.c_int, [_VP, C.c_int, C.c_int]),
    ("sph_render_trace_stats", C.c_int, [_VP, C.POINTER(SphRenderTraceStats)]),
    ("sph_render_trace_download_bvh", C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    ("sph_render_trace_download_paths", C.c_int, [_VP, _VP]),
    ("sph_video_create", C.c_int, [C.POINTER(SphVideoParams), C.POINTER(_VP)]),
    ("sph_video_destroy", None, [_VP]),
    ("sph_video_last_error", C.c_char_p, [_VP]),
    ("sph_video_header", C.c_int, [C.POINTER(SphVideoParams), _VP, C.POINTER(C.c_int64)]),
    ("sph_video_encode_rgb", C.c_int, [_VP, _VP]),
    ("sph_video_encode_render", C.c_int, [_VP, _VP]),
    ("sph_video_size", C.c_int, [_VP, C.POINTER(C.c_int64)]),
    ("sph_video_download", C.c_int, [_VP, _VP]),
    ("sph_video_stats", C.c_int, [_VP, C.POINTER(SphVideoStats)]),
    ("sph_png_create", C.c_int, [C.POINTER(SphPngParams), C.POINTER(_VP)]),
    ("sph_png_destroy", None, [_VP]),
    ("sph_png_last_error", C.c_char_p, [_VP]),
    ("sph_png_bound", C.c_int, [C.POINTER(SphPngParams), C.POINTER(C.c_int64)]),
    ("sph_png_set_coding", C.c_int, [_VP, C.c_int32]),
    ("sph_png_encode_rgb", C.c_int, [_VP, _VP]),
    ("sph_png_encode_render", C.c_int, [_VP, _VP]),
    ("sph_png_size", C.c_int, [_VP, C.POINTER(C.c_int64)]),
    ("sph_png_download", C.c_int, [_VP, _VP]),
    ("sph_png_stats", C.c_int, [_VP, C.POINTER(SphPngStats)]),
    ("sph_png_window_stats", C.c_int, [_VP, C.POINTER(SphPngWindowStats)]),
    ("sph_png_download_candidates", C.c_int, [_VP, _VP, C.c_size_t]),
    ("sph_text_create", C.c_int, [C.POINTER(SphTextParams), C.POINTER(_VP)]),
    ("sph_text_destroy", None, [_VP]),
    ("sph_text_last_error", C.c_char_p, [_VP]),
    ("sph_text_ply_points", C.c_int, [_VP, _VP, C.c_int64]),
    ("sph_text_ply_object", C.c_int, [_VP, _VP, C.c_int]),
    ("sph_text_obj_mesh", C.c_int, [_VP, _VP, C.c_int64, _VP, _VP, C.c_int64]),
    ("sph_text_obj_surface", C.c_int, [_VP, _VP]),
    ("sph_text_write", C.c_int, [_VP, C.c_char_p]),
    ("sph_text_size", C.c_int, [_VP, C.POINTER(C.c_int64)]),
    ("sph_text_read", C.c_int, [_VP, _VP, C.c_int64]),
    ("sph_text_stats", C.c_int, [_VP, C.POINTER(SphTextStats)]),
    ("sph_text_format_f32_host", C.c_int, [_VP, C.c_int64, _VP, C.c_int64, _VP]),
    ("sph_foam_create", C.c_int, [C.POINTER(SphFoamParams), C.POINTER(_VP)]),
    ("sph_foam_destroy", None, [_VP]),
    ("sph_foam_last_error", C.c_char_p, [_VP]),
    ("sph_foam_step_handle", C.c_int, [_VP, _VP, C.c_double]),
    ("sph_foam_step_points", C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_double]),
    ("sph_foam_seed", C.c_int, [_VP, _VP, _VP, _VP, C.c_int64]),
    ("sph_foam_count", C.c_int, [_VP, C.POINTER(C.c_int64)]),
    ("sph_foam_download", C.c_int, [_VP] * 6),
    ("sph_foam_download_potentials", C.c_int, [_VP] * 7),
    ("sph_foam_clear", C.c_int, [_VP]),
    ("sph_foam_stats", C.c_int, [_VP, C.POINTER(SphFoamStats)]),
    ("sph_render_set_foam", C.c_int, [_VP, _VP, C.c_double, _VP, _VP, _VP]),
    ("sph_render_set_surface_foam", C.c_int, [_VP, _VP, C.POINTER(SphRenderSurfaceFoamParams)]),
    ("sph_render_surface_download_foam", C.c_int, [_VP, C.c_int, _VP]),
    ("sph_render_surface_foam_stats", C.c_int, [_VP, C.POINTER(SphRenderSurfaceFoamStats)]),
    ("sph_get_grid_layout", C.c_int, [_VP, C.POINTER(SphGridLayout)]),
    ("sph_download_grid_table", C.c_int, [_VP, C.c_int, _VP, C.c_size_t]),
    ("sph_comm_allreduce", C.c_int, [_VP, C.POINTER(C.c_double), C.c_int, C.c_int]),
    ("sph_comm_barrier", C.c_int, [_VP]),
    ("sph_comm_selftest", C.c_int, [_VP, C.c_int]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]


def load():
    """Load libsph_hip.so; raises SphError if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SphError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(or `make -C sph_project_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, res, args in _SIGNATURES:
        fn = getattr(lib, name)  # AttributeError => header / library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class NativeObject:
    """Owner of native handles of one kind: ABI + "_create" / "_destroy" / "_last_error" are its functions, Error is what a non-zero
    return code raises.  self.h is the handle the calls of _chk are about unless they name another."""
    ABI = "sph"
    Error = SphError
    h = None

    def __init__(self):
        self.lib = load()
        self._owned = []

    def _create(self, params):
        h = C.c_void_p()
        name = self.ABI + "_create"
        self._chk(getattr(self.lib, name)(C.byref(params), C.byref(h)), name, None)
        self._owned.append(h)
        return h

    def close(self):
        for h in getattr(self, "_owned", []):
            getattr(self.lib, self.ABI + "_destroy")(h)
        self._owned = []
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what, *h):
        """h: the handle whose message explains rc (None: the create error); default self.h."""
        if rc != 0:
            msg = getattr(self.lib, self.ABI + "_last_error")(h[0] if h else self.h)
            raise self.Error(f"{what} failed ({rc}): {msg.decode() if msg else ''}", rc)


class FrameEncoder(NativeObject):
    """An encoder of RGB frames of one size into files of one format (csrc/sph_encoder_api.hpp): ABI + "_encode_rgb" / "_encode_render" /
    "_size" / "_download" / "_stats" are its functions, Stats their statistics structure."""
    Stats = None

    def _call(self, name, *args):
        self._need_open(name)
        name = f"{self.ABI}_{name}"
        self._chk(getattr(self.lib, name)(self.h, *args), name)

    def _need_open(self, what):
        if self.h is None:
            raise self.Error(f"{what}: the encoder is closed", ERR_INVALID)

    def _download(self):
        self._need_open("download")
        n = C.c_int64()
        self._call("size", C.byref(n))
        buf = np.empty(n.value, np.uint8)
        self._call("download", buf.ctypes.data)
        return buf.tobytes()

    def encode(self, rgb):
        """The file of uint8 (height, width, 3)."""
        self._need_open("encode")
        a = np.ascontiguousarray(rgb, dtype=np.uint8)
        if a.shape != (self.height, self.width, 3):
            raise ValueError(f"encode: expected ({self.height}, {self.width}, 3), got {a.shape}")
        self._call("encode_rgb", a.ctypes.data)
        return self._download()

    def encode_last(self, frame_renderer):
        """The file of a FrameRenderer's last frame (particles or meshes), read from its device buffer."""
        self._need_open("encode_last")
        if frame_renderer._last is None:
            raise self.Error("encode_last: the renderer holds no frame", ERR_INVALID)
        self._call("encode_render", frame_renderer._last)
        return self._download()

    def _stats(self):
        st = self.Stats()
        self._call("stats", C.byref(st))
        return st

    def stats(self):
        return struct_dict(self._stats())

    def write(self, path, frame_renderer):
        """{path} <- the renderer's last frame; the pixels never reach the host."""
        with open(path, "wb") as f:
            f.write(self.encode_last(frame_renderer))


class Engine(NativeObject):
    """Owns one SphHandle.  All arrays crossing the boundary are C-contiguous numpy f32 / i32."""

    def __init__(self, params: SphParams):
        super().__init__()
        self.params = params
        self.h = self._create(params)

    # -- scene upload
    def append_particles(self, object_id, pos, vel, density, pressure, material, is_dynamic, color):
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        n = pos.shape[0]
        vel = np.ascontiguousarray(vel, dtype=np.float32).reshape(n, 3)
        density = np.ascontiguousarray(density, dtype=np.float32).reshape(n)
        pressure = np.ascontiguousarray(pressure, dtype=np.float32).reshape(n)
        material = np.ascontiguousarray(material, dtype=np.int32).reshape(n)
        is_dynamic = np.ascontiguousarray(is_dynamic, dtype=np.int32).reshape(n)
        color = np.ascontiguousarray(color, dtype=np.int32).reshape(n, 3)
        self._chk(self.lib.sph_append_particles(self.h, int(object_id), n, _ptr(pos), _ptr(vel), _ptr(density),
                                                _ptr(pressure), _ptr(material), _ptr(is_dynamic), _ptr(color)),
                  "sph_append_particles")

    def set_appended_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        self._chk(self.lib.sph_set_appended_ids(self.h, ids.shape[0], _ptr(ids)), "sph_set_appended_ids")

    def set_object(self, object_id, material, is_dynamic):
        self._chk(self.lib.sph_set_object(self.h, int(object_id), int(material), int(bool(is_dynamic))), "sph_set_object")

    def set_rigid_pose(self, object_id, com, rot, vel, angvel, com0=None):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        com, rot, vel, angvel = f(com), f(rot), f(vel), f(angvel)
        com0 = None if com0 is None else f(com0)
        self._chk(self.lib.sph_set_rigid_pose(self.h, int(object_id), _ptr(com), _ptr(rot), _ptr(vel), _ptr(angvel),
                                              _ptr(com0)), "sph_set_rigid_pose")

    def get_rigid_wrench(self, reset=True):
        force = np.zeros((MAX_OBJECTS, 3), np.float32)
        torque = np.zeros((MAX_OBJECTS, 3), np.float32)
        self._chk(self.lib.sph_get_rigid_wrench(self.h, _ptr(force), _ptr(torque), int(reset)), "sph_get_rigid_wrench")
        return force, torque

    def set_rigid_contact(self, on=True, distance=0.0, wall_lo=None, wall_hi=None):
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(3)
        lo, hi = f(wall_lo), f(wall_hi)
        self._chk(self.lib.sph_set_rigid_contact(self.h, int(bool(on)), float(distance), _ptr(lo), _ptr(hi)), "sph_set_rigid_contact")

    def get_rigid_contacts(self, reset=True):
        table = np.zeros((MAX_OBJECTS, CONTACT_PARTNERS, CONTACT_BINS, CONTACT_VALUES), np.float64)
        self._chk(self.lib.sph_get_rigid_contacts(self.h, _ptr(table), int(reset)), "sph_get_rigid_contacts")
        return table

    def get_rigid_contact_pairs(self):
        n = C.c_int64(0)
        self._chk(self.lib.sph_get_rigid_contact_pairs(self.h, C.byref(n)), "sph_get_rigid_contact_pairs")
        return n.value

    # -- PBF variant
    def set_pbf_variant(self, variant="consistent", min_iterations=1, max_iterations=50, max_error=1e-3, epsilon=1e-6):
        """variant: "reference" / "consistent" (or 0 / 1); between create and prepare only."""
        p = SphPbfParams(int(PBF_VARIANTS.get(variant, variant)), int(min_iterations), int(max_iterations), float(max_error), float(epsilon))
        self._chk(self.lib.sph_set_pbf_variant(self.h, C.byref(p)), "sph_set_pbf_variant")

    def pbf_stats(self):
        st = SphPbfStats()
        self._chk(self.lib.sph_get_pbf_stats(self.h, C.byref(st)), "sph_get_pbf_stats")
        return struct_dict(st)

    # -- surface tension model
    def set_surface_tension(self, method="akinci", gamma=1.0, beta=0.0):
        """method: "reference" / "akinci" (or 0 / 1); gamma, beta: cohesion and adhesion coefficients of the Akinci model."""
        p = SphSurfaceTensionParams(int(SURFACE_TENSION_METHODS.get(method, method)), float(gamma), float(beta))
        self._chk(self.lib.sph_set_surface_tension(self.h, C.byref(p)), "sph_set_surface_tension")

    def get_surface_tension(self):
        p = SphSurfaceTensionParams()
        self._chk(self.lib.sph_get_surface_tension(self.h, C.byref(p)), "sph_get_surface_tension")
        return {"method": {v: k for k, v in SURFACE_TENSION_METHODS.items()}[p.method], "gamma": p.gamma, "beta": p.beta}

    # -- micropolar vorticity model
    def set_micropolar(self, method="micropolar", nu_t=0.01, zeta=0.1, theta_inv=0.5):
        """method: "none" / "micropolar" (or 0 / 1); nu_t: transfer coefficient, zeta: angular dissipation, theta_inv: inverse microinertia."""
        p = SphMicropolarParams(int(VORTICITY_METHODS.get(method, method)), float(nu_t), float(zeta), float(theta_inv))
        self._chk(self.lib.sph_set_micropolar(self.h, C.byref(p)), "sph_set_micropolar")

    # -- heat
    def set_thermal(self, method="conduction", alpha=1.0e-4, beta=0.0, t_ref=0.0):
        """method: "none" / "conduction" (or 0 / 1; None: off); alpha: thermal diffusivity, m^2 / s; beta: thermal expansion, 1 / K (0: no
        buoyancy); t_ref: the reference temperature (a_b = -beta (T - t_ref) g, and what particles without a temperature of their own
        are inserted with)."""
        if method is None:
            self._chk(self.lib.sph_set_thermal(self.h, None), "sph_set_thermal")
            return
        p = SphThermal(int(THERMAL_METHODS.get(method, method)), float(alpha), float(beta), float(t_ref))
        self._chk(self.lib.sph_set_thermal(self.h, C.byref(p)), "sph_set_thermal")

    def get_thermal(self):
        p = SphThermal()
        self._chk(self.lib.sph_get_thermal(self.h, C.byref(p)), "sph_get_thermal")
        return {"method": {v: k for k, v in THERMAL_METHODS.items()}[p.method], "alpha": p.alpha, "beta": p.beta, "t_ref": p.t_ref}

    def set_object_temperature(self, object_id, temperature=None):
        """A fluid object: the temperature its particles are inserted with from now on; a rigid object (-1: the domain box): the
        temperature it is held at.  None: none of its own (fluid: the reference temperature; rigid: adiabatic)."""
        has = temperature is not None
        self._chk(self.lib.sph_set_object_temperature(self.h, int(object_id), float(temperature) if has else 0.0, int(has)),
                  "sph_set_object_temperature")

    def get_micropolar(self):
        p = SphMicropolarParams()
        self._chk(self.lib.sph_get_micropolar(self.h, C.byref(p)), "sph_get_micropolar")
        return {"method": {v: k for k, v in VORTICITY_METHODS.items()}[p.method], "nu_t": p.nu_t, "zeta": p.zeta, "theta_inv": p.theta_inv}

    # -- air drag and wind
    def set_drag(self, method="gissler", k=1.0, rho_air=1.2041, air_velocity=(0.0, 0.0, 0.0)):
        """method: "none" / "gissler" (or 0 / 1); k: scales the force, rho_air: the air's density, air_velocity: a constant wind, m / s."""
        p = _drag_params(method, k, rho_air, air_velocity)
        self._chk(self.lib.sph_set_drag(self.h, C.byref(p)), "sph_set_drag")

    def get_drag(self):
        p = SphDragParams()
        self._chk(self.lib.sph_get_drag(self.h, C.byref(p)), "sph_get_drag")
        return {"method": {v: k for k, v in DRAG_METHODS.items()}[p.method], "k": p.k, "rho_air": p.rho_air,
                "air_velocity": tuple(float(v) for v in p.air_velocity)}

    # -- elastic solids
    def set_elastic_object(self, object_id, youngs_modulus, poisson_ratio=0.3):
        """Marks a fluid object as an elastic solid; the next neighbour search that holds its particles captures its rest configuration."""
        p = SphElasticParams(float(youngs_modulus), float(poisson_ratio))
        self._chk(self.lib.sph_set_elastic_object(self.h, int(object_id), C.byref(p)), "sph_set_elastic_object")

    def get_elastic_object(self, object_id):
        p = SphElasticObjectInfo()
        self._chk(self.lib.sph_get_elastic_object(self.h, int(object_id), C.byref(p)), "sph_get_elastic_object")
        return {"captured": p.captured == 2, "state": p.captured, "count": p.count, "first_id": p.first_id, "longest_list": p.longest_list,
                "min_eig_ratio": p.min_eig_ratio, "youngs_modulus": p.params.youngs_modulus, "poisson_ratio": p.params.poisson_ratio}

    def get_elastic_rest(self, object_id):
        """(nbr int32 (count, 64), g0_ij float32 (count, 64, 3), g0_ji likewise) of a captured object; row r = particle id first_id + r."""
        n = self.get_elastic_object(object_id)["count"]
        nbr = np.empty((n, ELASTIC_MAX_NEIGHBOURS), np.int32)
        gij = np.empty((n, ELASTIC_MAX_NEIGHBOURS, 3), np.float32)
        gji = np.empty((n, ELASTIC_MAX_NEIGHBOURS, 3), np.float32)
        self._chk(self.lib.sph_get_elastic_rest(self.h, int(object_id), _ptr(nbr), _ptr(gij), _ptr(gji)), "sph_get_elastic_rest")
        return nbr, gij, gji

    # -- device rigid integrator (the "device" rigid backend)
    def set_rigid_integrator(self, on=True, gravity=(0.0, 0.0, 0.0), wall_lo=(0.0, 0.0, 0.0), wall_hi=(0.0, 0.0, 0.0)):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(3)
        g, lo, hi = f(gravity), f(wall_lo), f(wall_hi)
        self._chk(self.lib.sph_set_rigid_integrator(self.h, int(bool(on)), _ptr(g), _ptr(lo), _ptr(hi)), "sph_set_rigid_integrator")

    def set_rigid_body(self, object_id, mass, inertia_body, com, rot, vel, angvel, com0=None, points=None):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        inertia, com, rot, vel, angvel = f(inertia_body), f(com), f(rot), f(vel), f(angvel)
        assert inertia.size == 9 and rot.size == 9 and com.size == 3 and vel.size == 3 and angvel.size == 3
        com0 = None if com0 is None else f(com0)
        pts = np.zeros((0, 3)) if points is None else np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        self._chk(self.lib.sph_set_rigid_body(self.h, int(object_id), float(mass), _ptr(inertia), _ptr(com), _ptr(rot), _ptr(vel),
                                              _ptr(angvel), _ptr(com0), _ptr(pts) if len(pts) else None, len(pts)), "sph_set_rigid_body")

    def get_rigid_state(self, object_id):
        """(com, rot[3, 3], vel, angvel) of a registered body, float64; drains the stream."""
        com, rot, vel, angvel = np.zeros(3), np.zeros((3, 3)), np.zeros(3), np.zeros(3)
        self._chk(self.lib.sph_get_rigid_state(self.h, int(object_id), _ptr(com), _ptr(rot), _ptr(vel), _ptr(angvel)), "sph_get_rigid_state")
        return com, rot, vel, angvel

    def rigid_integrate(self):
        self._chk(self.lib.sph_rigid_integrate(self.h), "sph_rigid_integrate")

    # -- scripted rigid bodies
    def set_rigid_motion(self, object_id, program, com_rest, rot_rest, com0=None):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        com_rest, rot_rest = f(com_rest), f(rot_rest)
        assert com_rest.size == 3 and rot_rest.size == 9
        com0 = None if com0 is None else f(com0)
        self._chk(self.lib.sph_set_rigid_motion(self.h, int(object_id), C.byref(program), _ptr(com_rest), _ptr(rot_rest), _ptr(com0)),
                  "sph_set_rigid_motion")

    def get_rigid_motion_state(self, object_id):
        """dict(com, rot[3, 3], vel, angvel, force, torque, impulse, angular_impulse, steps) of a scripted body; drains the stream."""
        st = SphRigidMotionState()
        self._chk(self.lib.sph_get_rigid_motion_state(self.h, int(object_id), C.byref(st)), "sph_get_rigid_motion_state")
        return rigid_motion_state_dict(st)

    # -- fluid emitters
    def set_emitter(self, index, program):
        self._chk(self.lib.sph_set_emitter(self.h, int(index), C.byref(program)), "sph_set_emitter")

    def get_emitter_state(self, index):
        """dict(object_id, layer_particles, max_layers, layers, emitted, held_layers, held_first, exhausted, held_id_base) of an emitter:
        what the host knows, no device access."""
        st = SphEmitterState()
        self._chk(self.lib.sph_get_emitter_state(self.h, int(index), C.byref(st)), "sph_get_emitter_state")
        d = struct_dict(st, skip=("reserved", "held_id_base"))
        d["held_id_base"] = [int(x) for x in st.held_id_base[:st.held_layers]]
        return d

    # -- outflow
    def set_outflow(self, index, program):
        """Sets (program: SphOutflow) or clears (None) the outflow volume `index`."""
        self._chk(self.lib.sph_set_outflow(self.h, int(index), C.byref(program) if program is not None else None), "sph_set_outflow")

    def outflow_state(self, index):
        """dict(removed, removed_last_step, active) of an outflow volume: what the host knows, no device access."""
        st = SphOutflowState()
        self._chk(self.lib.sph_get_outflow_state(self.h, int(index), C.byref(st)), "sph_get_outflow_state")
        return struct_dict(st, skip=("reserved",))

    def remove_particles(self, ids):
        """Removes the live fluid particles with these persistent ids (sph_remove_particles)."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        self._chk(self.lib.sph_remove_particles(self.h, _ptr(ids) if len(ids) else None, len(ids)), "sph_remove_particles")

    # -- adaptive time stepping
    def set_time_step(self, dt):
        """A new step size between steps (sph_set_time_step); refused while the CFL mode is on."""
        self._chk(self.lib.sph_set_time_step(self.h, float(dt)), "sph_set_time_step")

    def set_cfl(self, method="velocity", factor=0.5, min_dt=0.0, max_dt=0.0):
        """method: "none" / "velocity" (or 0 / 1); "none" switches the mode off and restores the creation step size."""
        if CFL_METHODS.get(method, method) == 0:
            self._chk(self.lib.sph_set_cfl(self.h, None), "sph_set_cfl")
            return
        p = cfl_params(method, factor, min_dt, max_dt)
        self._chk(self.lib.sph_set_cfl(self.h, C.byref(p)), "sph_set_cfl")

    def get_cfl(self):
        p = SphCflParams()
        self._chk(self.lib.sph_get_cfl(self.h, C.byref(p)), "sph_get_cfl")
        return {"method": {v: k for k, v in CFL_METHODS.items()}[p.method], "factor": p.factor, "min_dt": p.min_dt, "max_dt": p.max_dt}

    def time_state(self):
        """dict(time, dt_next, dt_last, target, vmax2, flags, steps): what the host knows, no device access."""
        st = SphTimeState()
        self._chk(self.lib.sph_get_time_state(self.h, C.byref(st)), "sph_get_time_state")
        return struct_dict(st, skip=("reserved",))

    def set_time_target(self, t_end):
        """The step sizes land on t_end from now on; None (or a value that is not finite) clears the target."""
        self._chk(self.lib.sph_set_time_target(self.h, float("nan") if t_end is None else float(t_end)), "sph_set_time_target")

    def advance_until(self, t_end, max_steps=1 << 30):
        """Steps until the scene time reaches t_end or max_steps steps are done; returns the steps done."""
        done = C.c_int(0)
        self._chk(self.lib.sph_advance_until(self.h, float(t_end), int(max_steps), C.byref(done)), "sph_advance_until")
        return done.value

    # -- device contact solver (the "device_contact" rigid backend)
    def set_rigid_contact_solver(self, on=True, restitution=0.2, friction=0.5, iterations=10, beta=0.2, slop=0.0, patch=0.0):
        self._chk(self.lib.sph_set_rigid_contact_solver(self.h, int(bool(on)), float(restitution), float(friction), int(iterations),
                                                        float(beta), float(slop), float(patch)), "sph_set_rigid_contact_solver")

    def get_rigid_contact_row_count(self):
        n = C.c_int(0)
        self._chk(self.lib.sph_get_rigid_contact_rows(self.h, None, 0, C.byref(n)), "sph_get_rigid_contact_rows")
        return n.value

    def get_rigid_contact_rows(self):
        """The rows of the last solve, (n, CONTACT_ROW_VALUES) float64; drains the stream."""
        rows = np.zeros((self.get_rigid_contact_row_count(), CONTACT_ROW_VALUES), np.float64)
        n = C.c_int(0)
        self._chk(self.lib.sph_get_rigid_contact_rows(self.h, _ptr(rows) if len(rows) else None, len(rows), C.byref(n)),
                  "sph_get_rigid_contact_rows")
        return rows

    # -- stepping
    def prepare(self):
        self._chk(self.lib.sph_prepare(self.h), "sph_prepare")

    def step(self, nsteps=1):
        self._chk(self.lib.sph_step(self.h, int(nsteps)), "sph_step")

    def step_async(self, nsteps=1):
        self._chk(self.lib.sph_step_async(self.h, int(nsteps)), "sph_step_async")

    def synchronize(self):
        self._chk(self.lib.sph_synchronize(self.h), "sph_synchronize")

    def step_begin(self):
        self._chk(self.lib.sph_step_begin(self.h), "sph_step_begin")

    def step_end(self):
        self._chk(self.lib.sph_step_end(self.h), "sph_step_end")

    def run_phase(self, phase):
        self._chk(self.lib.sph_run_phase(self.h, int(phase)), "sph_run_phase")

    # -- state access
    @property
    def particle_num(self):
        return self.lib.sph_particle_num(self.h)

    @property
    def fluid_particle_num(self):
        return self.lib.sph_fluid_particle_num(self.h)

    def download(self, field):
        dtype, comp = _FIELD_SPEC[field]
        n = self.particle_num
        out = np.empty((n, comp) if comp > 1 else (n,), dtype=dtype)
        self._chk(self.lib.sph_download(self.h, int(field), _ptr(out), out.nbytes), f"sph_download({field})")
        return out.reshape(3, n, 3) if field == F_CG_AP_PARTS else out

    def upload(self, field, arr):
        dtype, comp = _FIELD_SPEC[field]
        arr = np.ascontiguousarray(arr, dtype=dtype)
        self._chk(self.lib.sph_upload(self.h, int(field), _ptr(arr), arr.nbytes), f"sph_upload({field})")

    def stats(self):
        st = SphStats()
        self._chk(self.lib.sph_get_stats(self.h, C.byref(st)), "sph_get_stats")
        return struct_dict(st)

    def grid_layout(self):
        """The grid in the library's frame and the sizes of its tables, as a dict (axis_map: a tuple)."""
        lay = SphGridLayout()
        self._chk(self.lib.sph_get_grid_layout(self.h, C.byref(lay)), "sph_get_grid_layout")
        d = struct_dict(lay)
        d["axis_map"] = tuple(lay.axis_map)
        return d

    def download_grid_table(self, which, layout=None):
        """One table of the last sort (GRID_*), read only: cell_start i32[G + 1], tile headers i32[tiles][20], lane permutation
        u8[tiles][256], cell words u32[n]."""
        lay = layout or self.grid_layout()
        shape, dtype = {GRID_CELL_START: ((lay["G"] + 1,), np.int32), GRID_TILE_HEADER: ((lay["tiles"], lay["tile_header_ints"]), np.int32),
                        GRID_LANE_PERM: ((lay["tiles"], 256), np.uint8), GRID_CELL_WORD: ((lay["n"],), np.uint32)}[which]
        out = np.empty(shape, dtype)
        self._chk(self.lib.sph_download_grid_table(self.h, int(which), out.ctypes.data_as(C.c_void_p), out.nbytes), f"sph_download_grid_table({which})")
        return out

    def cg_scalars(self):
        """(alpha, beta, error) of the implicit-viscosity solve as the last launch left them on the device, f32"""
        out = (C.c_float * 3)()
        self._chk(self.lib.sph_get_cg_scalars(self.h, out), "sph_get_cg_scalars")
        return np.array(out[:], np.float32)

    # -- profiling
    def profile_enable(self, kernel_id=-1, on=True):
        self._chk(self.lib.sph_profile_enable(self.h, int(kernel_id), int(on)), "sph_profile_enable")

    def profile_reset(self):
        self._chk(self.lib.sph_profile_reset(self.h), "sph_profile_reset")

    def profile_read(self, kernel_id):
        n, ms = C.c_int64(), C.c_double()
        self._chk(self.lib.sph_profile_read(self.h, int(kernel_id), C.byref(n), C.byref(ms)), "sph_profile_read")
        return n.value, ms.value

    # -- multi-GPU (z-slab sharding)
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        self._chk(self.lib.sph_comm_unique_id(buf), "sph_comm_unique_id")
        return buf.raw

    def comm_init(self, rank, nranks, unique_id: bytes):
        assert len(unique_id) == 128
        self._chk(self.lib.sph_comm_init(self.h, int(rank), int(nranks), C.c_char_p(unique_id)), "sph_comm_init")

    def comm_set_slab(self, z_lo, z_hi):
        self._chk(self.lib.sph_comm_set_slab(self.h, int(z_lo), int(z_hi)), "sph_comm_set_slab")

    def comm_add_global_count(self, n, n_fluid):
        self._chk(self.lib.sph_comm_add_global_count(self.h, int(n), int(n_fluid)), "sph_comm_add_global_count")

    def comm_set_rebalance(self, every_steps):
        self._chk(self.lib.sph_comm_set_rebalance(self.h, int(every_steps)), "sph_comm_set_rebalance")

    def comm_get_slab(self, counts=True):
        v = [C.c_int() for _ in range(4)]
        args = [C.byref(v[0]), C.byref(v[1])] + ([C.byref(v[2]), C.byref(v[3])] if counts else [None, None])
        self._chk(self.lib.sph_comm_get_slab(self.h, *args), "sph_comm_get_slab")
        out = dict(z_lo=v[0].value, z_hi=v[1].value)
        if counts:
            out.update(n_owned=v[2].value, n_ghost=v[3].value)
        return out

    def comm_allreduce(self, values, op="sum"):
        """In-place all-reduce of up to 16 doubles over the communicator; returns the list of reduced values."""
        vals = [float(v) for v in (values if isinstance(values, (list, tuple)) else [values])]
        buf = (C.c_double * len(vals))(*vals)
        self._chk(self.lib.sph_comm_allreduce(self.h, buf, len(vals), {"sum": 0, "max": 1, "min": 2}[op]), "sph_comm_allreduce")
        return list(buf)

    def comm_barrier(self):
        self._chk(self.lib.sph_comm_barrier(self.h), "sph_comm_barrier")

    def comm_selftest(self, n=4096):
        self._chk(self.lib.sph_comm_selftest(self.h, int(n)), "sph_comm_selftest")

    def measure_copy_rate(self, nbytes=1 << 30, reps=10):
        """GB/s (read + written) of device-to-device copies on this GPU, measured now."""
        v = C.c_double()
        self._chk(self.lib.sph_measure_copy_rate(self.h, int(nbytes), int(reps), C.byref(v)), "sph_measure_copy_rate")
        return v.value

    def comm_transport(self):
        return self.lib.sph_comm_transport(self.h).decode()

    def device_info(self):
        name = C.create_string_buffer(256)
        cu, mem = C.c_int(), C.c_int64()
        self._chk(self.lib.sph_device_info(self.h, name, C.byref(cu), C.byref(mem)), "sph_device_info")
        return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}
