"""Adaptive time stepping restated in numpy from its definition (include/sph_hip.h, sph_set_cfl): the rule in float64, the speed in
float32 with every product and sum rounded.  sqrt, /, * and ceil are exactly rounded in numpy as in C, so the library's results are
compared with equalities.  MUTANTS are deliberately wrong variants; tests/test_cfl_host.py shows that its cases tell each from the
model."""
import math

import numpy as np

CLAMPED_MAX, CLAMPED_MIN, LANDING = 1, 2, 4
REACHED = 2.0 ** -20   # a time t counts as t_end when t_end - t <= REACHED * dt_max

MAT_FLUID, MAT_RIGID = 1, 2
MUTANTS = ("radius", "no_04", "clamp_order", "floor", "static_counted", "dynamic_ignored", "abs_v")


def counted(material, is_dynamic, ghost=None, removed=None, mutant=None):
    """bool (n,): active fluid particles and the rigid particles of dynamic bodies; never a ghost, never a removed particle."""
    material, is_dynamic = np.asarray(material), np.asarray(is_dynamic) != 0
    rigid = (material == MAT_RIGID) & is_dynamic
    if mutant == "static_counted":
        rigid = material == MAT_RIGID
    if mutant == "dynamic_ignored":
        rigid = np.zeros(len(material), bool)
    ok = (material == MAT_FLUID) | rigid
    if ghost is not None:
        ok &= np.asarray(ghost) == 0
    if removed is not None:
        ok &= np.asarray(removed) == 0
    return ok


def speed2(vel, mutant=None):
    """float32 (n,): (vx vx + vy vy) + vz vz, five roundings."""
    v = np.asarray(vel, np.float32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        if mutant == "abs_v":
            s = np.sqrt(s)
    return s.astype(np.float32)


def vmax2(vel, material, is_dynamic, ghost=None, removed=None, mutant=None):
    """(float32 maximum of |v|^2 over the particles that count -- non-finite squares left out --, whether there was one)."""
    s = speed2(vel, mutant)[counted(material, is_dynamic, ghost, removed, mutant)]
    fin = np.isfinite(s)
    best = np.float32(s[fin].max()) if fin.any() else np.float32(0.0)
    return best, bool((~fin).any())


def rule(factor, dt_min, dt_max, diameter, v2, remaining=None, mutant=None):
    """(dt, flags): the next step size from the float32 maximum v2; remaining: t_end - t with a time target, None without."""
    d = float(diameter) * (0.5 if mutant == "radius" else 1.0)
    k = 1.0 if mutant == "no_04" else 0.4
    v = math.sqrt(float(np.float32(v2)))
    lim = factor * k * d
    flags = 0
    if v * dt_max > lim:
        dt = lim / v
    else:
        dt, flags = dt_max, flags | CLAMPED_MAX
    if dt < dt_min:
        dt, flags = dt_min, flags | CLAMPED_MIN
    if remaining is not None and math.isfinite(remaining) and remaining > REACHED * dt_max:
        n = (math.floor if mutant == "floor" else math.ceil)(remaining / dt)
        dt = remaining / n if n > 0 else math.inf
        flags |= LANDING
        if mutant == "clamp_order":   # the clamps behind the landing instead of in front of it: a landing step below dt_min is raised again
            dt = max(min(dt, dt_max), dt_min)   # (the two clamps themselves commute while dt_min <= dt_max: their mutual order shows nowhere)
    with np.errstate(over="ignore"):
        return float(np.float32(dt)), flags


def reached(t, t_end, dt_max):
    return t_end - t <= REACHED * dt_max


def advance(factor, dt_min, dt_max, diameter, v2_of_step, t0, t_end, max_steps=1 << 30):
    """The step sizes of a run from t0 to t_end: v2_of_step(k) is the maximum the reduce finds before step k.  (dts, time)."""
    t, dts = float(t0), []
    while len(dts) < max_steps and not reached(t, t_end, dt_max):
        dt, _ = rule(factor, dt_min, dt_max, diameter, v2_of_step(len(dts)), t_end - t)
        dts.append(dt)
        t += dt
    return dts, t
