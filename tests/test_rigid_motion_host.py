"""CPU: scripted rigid bodies -- known answers of the host model RigidMotion (SPH/rigid_solver/motion.py), the relations
its backward-difference velocities keep over consecutive steps, the device's evaluator run on the host (sph_rigid_motion_eval_host, the
same source the kernel compiles) against the model, every validation error by message, and a scene without the key.  No device is
touched.

Bounds of the evaluator comparison: pose within 1e-12 max(1, |x|) -- a pose is on the order of a hundred float64 roundings of values of
order 1 (1e-14), the bound test_hip_rigid_device.py derives for a step's worth of them -- and velocities within
2e-12 max(1, |com|) / dt, because a velocity is the difference of two poses divided by dt."""
import copy
import math

import numpy as np
import pytest

from sph_project_amd import _lib as L
from sph_project_amd import product as P
from sph_project_amd.SPH.rigid_solver import host_rigid_solver as R
from sph_project_amd.SPH.rigid_solver.motion import RigidMotion

DT = 4e-4


def _body(motion, translation=(0.3, 0.2, 0.3), axis=(0, 1, 0), angle=0.0, **extra):
    body = {"objectId": 3, "translation": list(translation), "rotationAxis": list(axis), "rotationAngle": angle, "isDynamic": False,
            "motion": motion}
    body.update(extra)
    return body


def _motion(motion, dt=DT, **body):
    return RigidMotion.from_body(_body(motion, **body), dt)


ALL_THREE = {
    "start": 0.002, "end": 0.07, "pivot": [0.02, -0.01, 0.03],
    "keyframes": {"times": [0, 0.01, 0.025, 0.04], "translations": [[0, 0, 0], [0.02, 0, 0.01], [0.02, 0.03, 0], [-0.01, 0.01, 0.02]],
                  "rotations": [[0, 0, 0], [10, 0, 5], [0, 25, 0], [-15, 5, 30]], "interpolation": "smooth", "repeat": "pingpong"},
    "harmonic": {"frequency": 40.0, "phase": 30.0, "ramp": 0.01, "direction": [1, 2, 0], "amplitude": 0.015, "axis": [0, 1, 1], "angle": 20.0},
    "drift": {"velocity": [0.2, -0.1, 0.05], "axis": [1, 0, 0], "rate": 200.0},
}


# ---------------------------------------------------------------------------------------------- known answers
def test_harmonic_translation_quarter_and_half_period():
    f, amp = 2.0, 0.05
    m = _motion({"harmonic": {"frequency": f, "direction": [0, 3, 4], "amplitude": amp}})
    c0, _ = m.rest()
    com, rot = m.pose(0.25 / f)
    np.testing.assert_allclose(com - c0, amp * np.array([0, 0.6, 0.8]), rtol=0, atol=1e-16)
    assert np.array_equal(rot, np.eye(3))
    com, _ = m.pose(0.5 / f)
    np.testing.assert_allclose(com - c0, 0.0, atol=amp * 2e-16 * 4)   # sin(pi) in float64 is 1.2e-16


def test_drift_rotation_about_a_pivot():
    """90 deg/s about z for one second, pivot p: body point x goes to c0 + p + Rz(90) (x - p); with p = (1, 0, 0) + offsets the body
    point (1, 0, 0) relative to the pivot lands on (0, 1, 0)."""
    p = np.array([0.5, -0.25, 0.125])
    m = _motion({"pivot": list(p), "drift": {"axis": [0, 0, 2], "rate": 90.0}}, translation=(0, 0, 0))
    com, rot = m.pose(1.0)
    x = p + np.array([1.0, 0.0, 0.0])            # the body point one unit in +x of the pivot
    np.testing.assert_allclose(com + rot @ x, p + np.array([0.0, 1.0, 0.0]), atol=1e-15)
    np.testing.assert_allclose(com + rot @ p, p, atol=1e-15)   # the pivot stays where it is
    # ... and about the origin, literally (1, 0, 0) -> (0, 1, 0)
    m0 = _motion({"drift": {"axis": [0, 0, 1], "rate": 90.0}}, translation=(0, 0, 0))
    com, rot = m0.pose(1.0)
    np.testing.assert_allclose(com + rot @ np.array([1.0, 0, 0]), [0, 1, 0], atol=1e-15)


@pytest.mark.parametrize("interpolation", ["linear", "smooth"])
def test_keyframes_are_hit_exactly(interpolation):
    kf = copy.deepcopy(ALL_THREE["keyframes"])
    kf.update(interpolation=interpolation, repeat="hold")
    m = _motion({"keyframes": kf}, translation=(0, 0, 0))
    for t, d, r in zip(kf["times"], kf["translations"], kf["rotations"]):
        com, rot = m.pose(t)
        assert np.array_equal(com, np.array(d, np.float64)), (t, com, d)
        want = R._skew_exp(np.array(r, np.float64) * (math.pi / 180.0))
        np.testing.assert_allclose(rot, want, atol=1e-15)
    com, _ = m.pose(1.0)   # hold: the last key
    assert np.array_equal(com, np.array(kf["translations"][-1], np.float64))
    # halfway through the first segment both interpolations are at the midpoint
    com, _ = m.pose(0.005)
    np.testing.assert_allclose(com, 0.5 * np.array(kf["translations"][1]), atol=1e-17)


def test_smooth_has_zero_velocity_at_a_key():
    """Backward difference of s^2 (3 - 2 s) at a key: over a step dt that ends at the key, the displacement is
    (b - a) (1 - smooth(1 - dt / T)) = (b - a) (3 e^2 - 2 e^3), e = dt / T -- the velocity vanishes linearly with dt, where the linear
    interpolation keeps (b - a) / T."""
    T, b = 0.01, 0.02
    for n in (25, 250, 2500):
        dt = float(np.float32(T / n))
        kf = {"times": [0, n * dt, 2 * n * dt], "translations": [[0, 0, 0], [b, 0, 0], [0, 0, 0]], "interpolation": "smooth"}
        m = _motion({"keyframes": kf}, dt=dt, translation=(0, 0, 0))
        _, _, vel, _ = m.step(n - 1)   # the step that ends at key 1
        e = 1.0 / n
        want = b * (3 * e * e - 2 * e ** 3) / dt
        assert abs(vel[0] - want) <= 1e-9 * abs(b / dt), (n, vel[0], want)
        assert abs(vel[0]) < 4 * (b / (n * dt)) / n
        kf["interpolation"] = "linear"
        _, _, vlin, _ = _motion({"keyframes": kf}, dt=dt, translation=(0, 0, 0)).step(n - 1)
        assert abs(vlin[0] - b / (n * dt)) <= 1e-9 * b / (n * dt)


def test_loop_and_pingpong_are_periodic():
    kf = copy.deepcopy(ALL_THREE["keyframes"])
    T = kf["times"][-1]
    for repeat, period in (("loop", T), ("pingpong", 2 * T)):
        kf["repeat"] = repeat
        if repeat == "loop":   # a closed loop (last key = first key): t + period in floating point may fall on either side of the seam
            kf["translations"][-1], kf["rotations"][-1] = kf["translations"][0], kf["rotations"][0]
        else:
            kf = dict(copy.deepcopy(ALL_THREE["keyframes"]), repeat=repeat)
        m = _motion({"keyframes": kf})
        for t in (0.0, 0.003, 0.0125, 0.031, 0.0399):
            a, ra = m.pose(t)
            for cycles in (1, 3):
                b, rb = m.pose(t + cycles * period)
                np.testing.assert_allclose(b, a, atol=1e-14)
                np.testing.assert_allclose(rb, ra, atol=1e-13)
    kf["repeat"] = "pingpong"
    m = _motion({"keyframes": kf})
    a, _ = m.pose(T - 0.004)
    b, _ = m.pose(T + 0.004)   # the way back mirrors the way there
    np.testing.assert_allclose(a, b, atol=1e-14)


def test_start_end_and_ramp():
    hm = {"frequency": 5.0, "ramp": 0.1, "direction": [1, 0, 0], "amplitude": 0.01}
    m = _motion({"start": 0.05, "end": 0.3, "harmonic": hm, "drift": {"velocity": [0, 1, 0]}}, translation=(0, 0, 0))
    for t in (0.0, 0.02, 0.05):   # before start: pose(0)
        com, rot = m.pose(t)
        assert np.array_equal(com, np.zeros(3)) and np.array_equal(rot, np.eye(3))
    tau = 0.025   # inside the ramp: a quarter of it
    com, _ = m.pose(0.05 + tau)
    assert abs(com[0] - (tau / 0.1) * math.sin(2 * math.pi * 5.0 * tau) * 0.01) < 1e-16 and abs(com[1] - tau) < 1e-16
    tau = 0.15    # behind the ramp
    com, _ = m.pose(0.05 + tau)
    assert abs(com[0] - math.sin(2 * math.pi * 5.0 * tau) * 0.01) < 1e-16
    held, _ = m.pose(0.3)
    for t in (0.31, 1.0, 50.0):   # after end: pose(end - start)
        com, _ = m.pose(t)
        assert np.array_equal(com, held)
    assert abs(held[1] - 0.25) < 1e-16
    never = _motion({"end": None, "drift": {"velocity": [0, 1, 0]}}, translation=(0, 0, 0))
    assert abs(never.pose(1000.0)[0][1] - 1000.0) < 1e-12
    # after end the backward differences vanish
    k = int(0.3 / m.dt) + 5
    _, _, vel, w = m.step(k)
    assert np.array_equal(vel, np.zeros(3)) and np.array_equal(w, np.zeros(3))


# ---------------------------------------------------------------------------------------------- consecutive steps
def test_200_consecutive_steps_keep_the_integrators_relations():
    m = _motion(ALL_THREE, axis=(1, 0, 1), angle=25.0)
    com0, rot0 = m.pose(0.0)
    prev_com, prev_rot = com0, rot0
    worst = [0.0, 0.0, 0.0]
    moved = turned = False
    for k in range(200):
        com, rot, vel, w = m.step(k)
        ulp = np.spacing(np.abs(com).max())
        d = np.abs((prev_com + m.dt * vel) - com).max()
        worst[0] = max(worst[0], d / ulp)
        assert d <= 4 * ulp, (k, d, ulp)
        e = np.abs(R._skew_exp(m.dt * w) @ prev_rot - rot).max()
        worst[1] = max(worst[1], e)
        assert e <= 1e-12, (k, e)
        o = np.abs(rot @ rot.T - np.eye(3)).max()
        worst[2] = max(worst[2], o)
        assert o <= 1e-12, (k, o)
        moved |= bool(np.any(vel != 0)); turned |= bool(np.any(w != 0))
        prev_com, prev_rot = com, rot
    print(f"200 steps: com relation {worst[0]:.2f} ulp, rotation relation {worst[1]:.3e}, orthonormality {worst[2]:.3e}")
    assert moved and turned
    last = m.step(199)
    assert np.array_equal(last[0], m.pose(200 * m.dt)[0])   # t_k is a product of the step count: no running sum


# ---------------------------------------------------------------------------------------------- the device's evaluator on the host
_PROGRAMS = {
    "keyframes": {"keyframes": ALL_THREE["keyframes"]},
    "keyframes_linear_loop": {"pivot": [0.01, 0.02, 0.03], "keyframes": dict(ALL_THREE["keyframes"], interpolation="linear", repeat="loop")},
    "harmonic": {"harmonic": ALL_THREE["harmonic"]},
    "drift": {"pivot": [0.05, 0, 0], "drift": ALL_THREE["drift"]},
    "all": ALL_THREE,
}


def test_the_device_evaluator_on_the_host_against_the_model():
    worst_pose = worst_vel = 0.0
    for name, prog in _PROGRAMS.items():
        m = _motion(prog, axis=(1, 2, 0), angle=-35.0)
        c0, r0 = m.rest()
        st = m.to_struct()
        for k in list(range(0, 130)) + [170, 171, 174, 175, 176, 1000, 123456]:
            got = L.rigid_motion_eval_host(st, c0, r0, m.dt, k)
            com, rot, vel, w = m.step(k)
            assert got["steps"] == k + 1
            scale = max(1.0, float(np.abs(com).max()))
            for what, g, want in (("com", got["com"], com), ("rot", got["rot"], rot)):
                d = float(np.max(np.abs(g - want) / np.maximum(1.0, np.abs(want))))
                worst_pose = max(worst_pose, d)
                assert d <= 1e-12, (name, k, what, d)
            for what, g, want in (("vel", got["vel"], vel), ("angvel", got["angvel"], w)):
                d = float(np.max(np.abs(g - want))) * m.dt / scale
                worst_vel = max(worst_vel, d)
                assert d <= 2e-12, (name, k, what, d)
    print(f"sph_rigid_motion_eval_host against RigidMotion.step: worst pose difference {worst_pose:.3e} (bound 1e-12), "
          f"worst velocity difference x dt / max(1, |com|) {worst_vel:.3e} (bound 2e-12)")


def test_the_host_entry_refuses_bad_arguments():
    lib = L.load()
    m = _motion(ALL_THREE)
    c0, r0 = m.rest()
    msg = lambda: (lib.sph_last_error(None) or b"").decode()
    with pytest.raises(L.SphError, match="dt"):
        L.rigid_motion_eval_host(m.to_struct(), c0, r0, 0.0, 0)
    st = m.to_struct()
    st.nkeys = 65
    with pytest.raises(L.SphError, match="65 keys") as err:
        L.rigid_motion_eval_host(st, c0, r0, DT, 0)
    assert err.value.code == L.ERR_INVALID
    st = m.to_struct()
    st.key_times[2] = st.key_times[1]
    with pytest.raises(L.SphError, match="increase strictly"):
        L.rigid_motion_eval_host(st, c0, r0, DT, 0)
    st = m.to_struct()
    st.direction[0] = 2.0
    with pytest.raises(L.SphError, match="direction"):
        L.rigid_motion_eval_host(st, c0, r0, DT, 0)
    st = m.to_struct()
    st.end = st.start
    with pytest.raises(L.SphError, match="end"):
        L.rigid_motion_eval_host(st, c0, r0, DT, 0)
    assert "end" in msg()


def test_struct_sizes_match_a_compiled_sizeof(tmp_path):
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sph_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(SphRigidMotion), sizeof(SphRigidMotionState), '
                   'offsetof(SphRigidMotion, key_rotations), offsetof(SphRigidMotion, drift_rate), offsetof(SphRigidMotionState, steps), '
                   '(int)SPH_K_RIGID_MOTION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    M, S = L.SphRigidMotion, L.SphRigidMotionState
    assert got == [ctypes.sizeof(M), ctypes.sizeof(S), M.key_rotations.offset, M.drift_rate.offset, S.steps.offset, L.K_RIGID_MOTION]
    assert L.K_RIGID_MOTION == 30 and L.RIGID_MOTION_MAX_KEYS == 64


# ---------------------------------------------------------------------------------------------- validation
def _bad(motion, match, **kw):
    with pytest.raises(ValueError, match=match) as err:
        RigidMotion.from_body(_body(motion, **{k: v for k, v in kw.items() if k in ("isDynamic",)}), DT,
                              **{k: v for k, v in kw.items() if k in ("method", "dim", "backend")})
    assert "rigid body 3" in str(err.value)


def test_validation_errors_name_the_body_and_the_field():
    drift = {"drift": {"velocity": [1, 0, 0]}}
    _bad(drift, "isDynamic: true together with motion", isDynamic=True)
    _bad({"drift": {"velocity": [1, 0, 0]}, "stat": 0.0}, r"motion\.stat: unknown key")
    _bad({"harmonic": {"frequency": 1.0, "amplitud": 0.1}}, r"motion\.harmonic\.amplitud: unknown key")
    _bad({"keyframes": {"times": [0], "tranlations": [[0, 0, 0]]}}, r"motion\.keyframes\.tranlations: unknown key")
    _bad({"drift": {"speed": [1, 0, 0]}}, r"motion\.drift\.speed: unknown key")
    _bad({"start": 0.0}, "no block at all")
    _bad({"keyframes": {"times": [0.1, 0.2], "translations": [[0, 0, 0]] * 2}}, r"keyframes\.times: times must start at 0")
    _bad({"keyframes": {"times": [0, 0.2, 0.2], "translations": [[0, 0, 0]] * 3}}, r"keyframes\.times: .*increase strictly")
    _bad({"keyframes": {"times": [0, 0.2], "translations": [[0, 0, 0]] * 3}}, r"keyframes\.translations: array lengths differ")
    _bad({"keyframes": {"times": [0, 0.2], "rotations": [[0, 0, 0]]}}, r"keyframes\.rotations: array lengths differ")
    many = [0.01 * i for i in range(65)]
    _bad({"keyframes": {"times": many, "translations": [[0, 0, 0]] * 65}}, r"keyframes\.times: more than 64 keys")
    _bad({"drift": {"velocity": [1, float("nan"), 0]}}, r"drift\.velocity: nan is not a finite number")
    _bad({"harmonic": {"frequency": float("inf"), "direction": [1, 0, 0], "amplitude": 0.1}}, r"harmonic\.frequency: inf is not a finite number")
    _bad({"harmonic": {"frequency": 1.0, "direction": [0, 0, 0], "amplitude": 0.1}}, r"harmonic\.direction: a zero vector beside a non-zero amplitude")
    _bad({"harmonic": {"frequency": 1.0, "axis": [0, 0, 0], "angle": 5.0}}, r"harmonic\.axis: a zero vector beside a non-zero angle")
    _bad({"drift": {"rate": 5.0}}, r"drift\.axis: a zero vector beside a non-zero rate")
    _bad({"harmonic": {"frequency": -1.0, "direction": [1, 0, 0], "amplitude": 0.1}}, r"harmonic\.frequency: negative frequency")
    _bad({"harmonic": {"frequency": 1.0, "ramp": -0.5, "direction": [1, 0, 0], "amplitude": 0.1}}, r"harmonic\.ramp: negative ramp")
    _bad(dict(drift, start=0.5, end=0.5), r"motion\.end: end 0\.5 <= start 0\.5")
    _bad(dict(drift, start=0.5, end=0.25), r"motion\.end: end 0\.25 <= start 0\.5")
    _bad(drift, "PBF moves no rigid body", method="pbf")
    _bad(drift, "3-D scene", dim=2)
    _bad(drift, "pybullet", backend="pybullet")
    # 64 keys are fine, and so is a zero direction beside a zero amplitude
    ok = RigidMotion.from_body(_body({"keyframes": {"times": many[:64], "translations": [[0, 0, 0]] * 64},
                                      "harmonic": {"frequency": 1.0}}), DT)
    assert len(ok.times) == 64 and ok.to_struct().nkeys == 64


def test_canonical_form():
    m = _motion(ALL_THREE, axis=(0, 0, 1), angle=90.0)
    assert m.dt == float(np.float32(DT))
    np.testing.assert_allclose(np.linalg.norm(m.direction), 1.0, atol=1e-15)
    np.testing.assert_allclose(m.direction, np.array([1, 2, 0]) / math.sqrt(5.0), atol=1e-16)
    assert m.phase == 30.0 * (math.pi / 180.0) and m.drift_rate == 200.0 * (math.pi / 180.0)
    c0, r0 = m.rest()
    np.testing.assert_allclose(r0 @ np.array([1.0, 0, 0]), [0, 1, 0], atol=1e-15)
    st = m.to_struct()
    assert st.nkeys == 4 and st.interpolation == 1 and st.repeat == 2 and st.end == 0.07
    assert _motion({"drift": {"velocity": [1, 0, 0]}}).to_struct().end == math.inf


# ---------------------------------------------------------------------------------------------- scenes
class _Engine:
    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} touched")


class _Cfg:
    def __init__(self, bodies):
        self._b = bodies

    def get_rigid_bodies(self):
        return self._b

    def get_rigid_blocks(self):
        return []

    def get_cfg(self, k):
        return None


def _container(bodies):
    import types
    return types.SimpleNamespace(dim=3, cfg=_Cfg(bodies), padding=0.04, particle_diameter=0.02, domain_box_thickness=0.0,
                                 domain_start=np.zeros(3), domain_end=np.ones(3), engine=_Engine(), rigid_backend="native",
                                 METHOD="wcsph", step_count=0, in_step=False)


def test_a_scene_without_motion_has_no_scripted_body():
    body = {"objectId": 1, "isDynamic": False, "entryTime": -1.0, "translation": [0, 0, 0], "rotationAxis": [0, 1, 0], "rotationAngle": 0.0}
    rs = R.HostRigidSolver(_container([body]), dt=DT)
    assert rs.scripted == {} and rs.bodies == {}
    rs.insert_rigid_object()
    assert rs.scripted == {} and rs.bodies == {} and rs.present_rigid_object == [1]
    rs.step()   # nothing to move: the engine is not touched
    assert not P.dam_break_scene().get("RigidBodies")


def test_wave_tank_scene_is_a_valid_scripted_scene():
    cfg = P.wave_tank_scene(length=0.5, width=0.2, depth=0.06)
    (body,) = cfg["RigidBodies"]
    m = RigidMotion.from_body(body, cfg["Configuration"]["timeStepSize"], method="wcsph")
    assert body["isDynamic"] is False and m.ramp == 1.0 and m.amplitude == 0.03 and m.direction == [1.0, 0.0, 0.0]
    c0, _ = m.rest()
    com, rot = m.pose(1.25)   # behind the ramp, a quarter period on: the full stroke
    np.testing.assert_allclose(com - c0, [0.03, 0, 0], atol=1e-15)
    assert np.array_equal(rot, np.eye(3))
