"""A numpy float32 model of the outflow predicate (include/sph_hip.h sph_set_outflow), written from the specification and
not from csrc/sph_outflow_eval.hpp: the bounds rounded to float32 once, inclusive box faces, the sphere as (dx dx + dy dy) + dz dz <=
r r with every operation rounded to float32, invert, the time window start <= k dt <= end, and the lowest-index rule.  MUTANTS are
deliberately wrong variants: tests/test_outflow_host.py shows that each fails a check the right model passes."""
import numpy as np

F = np.float32


class Volume:
    def __init__(self, shape, min=None, max=None, center=None, radius=0.0, invert=False, start=0.0, end=None, objects=None, mutant=None):
        self.shape, self.invert, self.start = shape, bool(invert), float(start)
        self.end = np.inf if end is None else float(end)
        self.objects = None if objects is None else sorted(int(o) for o in objects)
        self.mutant = mutant
        if shape == "box":
            self.lo, self.hi = np.asarray(min, np.float64).astype(F), np.asarray(max, np.float64).astype(F)
        else:
            self.c, self.r = np.asarray(center, np.float64).astype(F), F(radius)

    @classmethod
    def from_entry(cls, e, mutant=None):
        return cls(e["shape"], e.get("min"), e.get("max"), e.get("center"), e.get("radius") or 0.0, e.get("invert") or False,
                   e.get("start") or 0.0, e.get("end"), e.get("objects"), mutant=mutant)

    def inside(self, xyz):
        """bool (n,): geometry and invert, on float32 positions (n, 3)."""
        x = np.asarray(xyz, F).reshape(-1, 3)
        if self.shape == "box":
            if self.mutant == "exclusive_face":
                ins = np.all((x > self.lo) & (x < self.hi), axis=1)
            else:
                ins = np.all((x >= self.lo) & (x <= self.hi), axis=1)
        else:
            d = (x - self.c).astype(F)
            sq = (d * d).astype(F)
            d2 = ((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)
            r2 = F(self.r * self.r)
            ins = d2 < r2 if self.mutant == "sphere_strict" else d2 <= r2
        if self.invert and self.mutant != "invert_ignored":
            ins = ~ins
        return ins

    def active(self, k, dt):
        """the window at step count k: T_k = k dt, a float64 product"""
        if self.mutant == "window_off_by_one":
            k = k - 1
        t = float(k) * float(dt)
        return self.start <= t <= self.end


def attribute(volumes, xyz, k, dt, object_ids=None, fluid=None, mutant=None):
    """int (n,): the index of the volume that removes each particle at step count k, -1 for none.  The lowest index wins
    (mutant "highest_index": the highest)."""
    x = np.asarray(xyz, F).reshape(-1, 3)
    hit = np.full(len(x), -1, np.int64)
    order = range(len(volumes))
    for q in (reversed(order) if mutant != "highest_index" else order):
        v = volumes[q]
        if v is None or not v.active(k, dt):
            continue
        ins = v.inside(x)
        if v.objects is not None and object_ids is not None:
            ins &= np.isin(object_ids, v.objects)
        hit[ins] = q
    if fluid is not None:
        hit[~np.asarray(fluid, bool)] = -1
    return hit


MUTANTS = ("exclusive_face", "sphere_strict", "window_off_by_one", "invert_ignored", "highest_index")
