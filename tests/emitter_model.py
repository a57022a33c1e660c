"""Float64 restatement of the fluid emitters (include/sph_hip.h sph_set_emitter), for the tests: written from the formulas
of the scene format, not from the C++.

  lattice   nu = floor(width / spacing), nv = floor(height / spacing); point (i, j) at ((i + 0.5 - nu / 2) spacing, (j + 0.5 - nv / 2)
            spacing) in the plane's basis, j slow and i fast; a circle takes the lattice of its bounding square and keeps a^2 + b^2 <= r^2
  basis     direction normalised; tangent2 = the part of `up` perpendicular to it, normalised; tangent1 = tangent2 x direction
  schedule  T_k = k dt;  s(k) = speed max(0, min(T_k, end) - start);  born(k) = 0 if T_k < start else min(Lmax, floor(s / spacing) + 1),
            Lmax = floor(maxParticles / layer_n);  a_j(k) = s(k) - j spacing;  layer j < born(k) is held while a_j(k) < hold spacing and
            T_k <= end
  position  position + a_j direction + a tangent1 + b tangent2
  ids       the particle count at the moment of the emission + the index within the batch; emitters in list order, a layer in lattice order

`mutant` switches one deliberate mistake on (the host test shows that each fails a check)."""
import math

import numpy as np

MUTANTS = ("floor_plus_one", "running_sum", "end_ignored", "lattice_not_centred", "circle_radius", "emitter_order")


class Emitter:
    def __init__(self, position, direction, speed, max_particles, spacing, dt, shape="rectangle", width=0.0, height=0.0, radius=0.0,
                 up=None, start=0.0, end=math.inf, hold=2, density=1000.0, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant
        self.shape, self.width, self.height, self.radius = shape, float(width), float(height), float(radius)
        self.position = np.asarray(position, np.float64)
        d = np.asarray(direction, np.float64)
        self.direction = d / math.sqrt(float(d @ d))
        if up is None:
            up = [0.0, 1.0, 0.0] if abs(self.direction[1]) < 0.999 else [1.0, 0.0, 0.0]
        up = np.asarray(up, np.float64)
        t2 = up - float(up @ self.direction) * self.direction
        self.tangent2 = t2 / math.sqrt(float(t2 @ t2))
        self.tangent1 = np.cross(self.tangent2, self.direction)
        self.speed, self.start, self.end, self.hold, self.density = float(speed), float(start), float(end), int(hold), float(density)
        self.spacing, self.dt, self.max_particles = float(spacing), float(dt), int(max_particles)
        self.lattice = self._lattice()
        self.layer_n = len(self.lattice)
        self.max_layers = self.max_particles // self.layer_n if self.layer_n else 0

    def _lattice(self):
        w, h = (2.0 * self.radius, 2.0 * self.radius) if self.shape == "circle" else (self.width, self.height)
        nu, nv = int(math.floor(w / self.spacing)), int(math.floor(h / self.spacing))
        centre_u, centre_v = (0.0, 0.0) if self.mutant == "lattice_not_centred" else (nu / 2.0, nv / 2.0)
        r = self.radius + 0.5 * self.spacing if self.mutant == "circle_radius" else self.radius
        pts = []
        for j in range(nv):
            for i in range(nu):
                a, b = (i + 0.5 - centre_u) * self.spacing, (j + 0.5 - centre_v) * self.spacing
                if self.shape != "circle" or a * a + b * b <= r * r:
                    pts.append((a, b))
        self.nu, self.nv = nu, nv
        return np.array(pts, np.float64).reshape(-1, 2)

    def time(self, k):
        if self.mutant == "running_sum":
            t = 0.0
            for _ in range(k):
                t += self.dt
            return t
        return k * self.dt

    def s(self, k):
        t = self.time(k)
        te = t if self.mutant == "end_ignored" else min(t, self.end)
        return self.speed * max(0.0, te - self.start)

    def born(self, k):
        if self.time(k) < self.start:
            return 0
        extra = 0 if self.mutant == "floor_plus_one" else 1
        return min(self.max_layers, int(math.floor(self.s(k) / self.spacing)) + extra)

    def offset(self, j, k):
        return self.s(k) - j * self.spacing

    def held(self, k):
        """(first, count) of the held layers after k steps."""
        born = self.born(k)
        if self.hold <= 0 or not self.time(k) <= self.end:
            return born, 0
        js = [j for j in range(born) if self.offset(j, k) < self.hold * self.spacing]
        return (js[0], len(js)) if js else (born, 0)

    def positions(self, j, k):
        """float64 (layer_n, 3): layer j after k steps."""
        a = self.offset(j, k)
        return (self.position + a * self.direction)[None, :] + self.lattice[:, :1] * self.tangent1[None, :] + self.lattice[:, 1:] * self.tangent2[None, :]

    def velocity(self):
        return self.speed * self.direction

    def emitted_mass(self, k, V0):
        return self.layer_n * self.born(k) * V0 * self.density


def assign_ids(emitters, steps, n0=0, mutant=None):
    """The persistent id of the first particle of every layer: {(emitter index, layer): id}, and the particle count after every step count
    0 .. steps (index 0: after prepare).  n0: particles present before the emitters' first layer."""
    order = list(range(len(emitters)))
    if mutant == "emitter_order":
        order.reverse()
    n, done, base, counts = n0, [0] * len(emitters), {}, []
    for k in range(steps + 1):
        for q in order:
            e = emitters[q]
            while done[q] < e.born(k):
                base[(q, done[q])] = n
                n += e.layer_n
                done[q] += 1
        counts.append(n)
    return base, counts
