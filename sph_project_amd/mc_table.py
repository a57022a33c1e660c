"""Marching-cubes case table of the surface reconstruction, generated from first principles.

Conventions (shared with sph_surface.hpp and tests/surface_model.py):
  * corner k of a cube sits at offset (k & 1, (k >> 1) & 1, (k >> 2) & 1) from its lower grid point;
  * case = sum of 1 << k over the corners that are INSIDE (phi > iso);
  * the 12 edges are (lower-corner offset, axis): 0-3 along x from (0,0,0) (0,1,0) (0,0,1) (0,1,1), 4-7 along y from (0,0,0)
    (1,0,0) (0,0,1) (1,0,1), 8-11 along z from (0,0,0) (1,0,0) (0,1,0) (1,1,0).

Construction, per case:
  1. On each of the 6 faces the crossing edges are paired into segments.  A face with two diagonal inside corners (the ambiguous
     face) is always cut so that the INSIDE corners are separated: the choice depends on that face's four signs alone, so the two
     cubes sharing a face cut it identically, which keeps the mesh free of cracks.
  2. Each segment is directed so that, seen from outside the cube, the inside corners it cuts off lie on a fixed side; the directed
     segments then chain into closed loops (every crossing edge lies on two faces: one segment enters it, one leaves).
  3. Each loop is triangulated without a diagonal that lies in a cube face (a diagonal in a face could coincide with the neighbour's and
     make an edge with four triangles); triangles keep the loop's direction, which winds them counter-clockwise seen from outside
     (the phi < iso side).
`python -m sph_project_amd.mc_table` rewrites csrc/sph_mc_table.hpp; tests/test_surface_host.py checks the two agree.
"""
from __future__ import annotations

import os

import numpy as np

CORNERS = np.array([(k & 1, (k >> 1) & 1, (k >> 2) & 1) for k in range(8)], dtype=np.int64)
EDGES = []   # (offset, axis)
for _axis in range(3):
    _o = [(0, 0), (1, 0), (0, 1), (1, 1)]
    for _a, _b in _o:
        off = [0, 0, 0]
        others = [d for d in range(3) if d != _axis]
        off[others[0]], off[others[1]] = _a, _b
        EDGES.append((tuple(off), _axis))
# corner pair of every edge
EDGE_CORNERS = []
for _off, _axis in EDGES:
    c0 = _off[0] + 2 * _off[1] + 4 * _off[2]
    EDGE_CORNERS.append((c0, c0 + (1 << _axis)))
# faces: (axis, side); corners of a face in cyclic order (around the face)
FACES = []
for _axis in range(3):
    for _side in range(2):
        u, v = [d for d in range(3) if d != _axis]
        cyc = []
        for a, b in [(0, 0), (1, 0), (1, 1), (0, 1)]:
            p = [0, 0, 0]
            p[_axis], p[u], p[v] = _side, a, b
            cyc.append(p[0] + 2 * p[1] + 4 * p[2])
        FACES.append((_axis, _side, cyc))


def _edge_of(c0, c1):
    key = (min(c0, c1), max(c0, c1))
    for e, (a, b) in enumerate(EDGE_CORNERS):
        if (a, b) == key:
            return e
    raise KeyError(key)


def edge_mid(e):
    off, axis = EDGES[e]
    p = np.array(off, dtype=np.float64)
    p[axis] += 0.5
    return p


def face_edges(f):
    cyc = FACES[f][2]
    return [_edge_of(cyc[i], cyc[(i + 1) % 4]) for i in range(4)]


def face_segments(case, f):
    """Directed segments (edge_from, edge_to) of face f in configuration `case` (inside corners separated on ambiguous faces)."""
    axis, side, cyc = FACES[f]
    ins = [(case >> c) & 1 for c in cyc]
    fe = face_edges(f)   # fe[i] joins cyc[i] and cyc[i+1]
    crossing = [i for i in range(4) if ins[i] != ins[(i + 1) % 4]]
    if not crossing:
        return []
    # pair crossings: each inside run of corners (cyclically consecutive inside corners) is cut off by one segment
    segs = []
    if len(crossing) == 2:
        # one run of inside corners
        runs = [[i for i in range(4) if ins[i]]]
        pairs = [tuple(crossing)]
    else:   # 4 crossings: ambiguous face, inside corners separated -> one segment per inside corner
        runs, pairs = [], []
        for i in range(4):
            if ins[i]:
                runs.append([i])
                pairs.append(((i - 1) % 4, i))   # edges before and after corner i
    nF = np.zeros(3)
    nF[axis] = 1.0 if side == 1 else -1.0
    for (ia, ib), run in zip(pairs, runs):
        ea, eb = fe[ia], fe[ib]
        if len(crossing) == 2:
            # the inside corners on one side of the segment: the run between the two crossings
            inside_corners = [cyc[i] for i in range(4) if ins[i]]
        else:
            inside_corners = [cyc[i] for i in run]
        c_in = CORNERS[inside_corners].mean(axis=0)
        pa, pb = edge_mid(ea), edge_mid(eb)
        o = 0.5 * (pa + pb) - c_in                 # from the cut-off inside corners towards the outside
        d = pb - pa
        if np.dot(np.cross(o, d), nF) < 0:
            segs.append((ea, eb))
        else:
            segs.append((eb, ea))
    return segs


def _shares_face(e0, e1):
    for f in range(6):
        fe = face_edges(f)
        if e0 in fe and e1 in fe:
            return True
    return False


def _triangulations(poly):
    """All triangulations of a polygon (vertex list), as lists of (a, b, c) keeping its orientation."""
    n = len(poly)
    if n < 3:
        return [[]]
    if n == 3:
        return [[tuple(poly)]]
    out = []
    for k in range(1, n - 1):   # the triangle on the closing edge (last, first) has apex poly[k]; vertex order = loop order
        for tl in _triangulations(poly[: k + 1]):
            for tr in _triangulations(poly[k:]):
                out.append([(poly[0], poly[k], poly[-1])] + tl + tr)
    return out


def _triangulate(loop):
    """A triangulation of the loop none of whose diagonals lies in a cube face (first such in a fixed search order)."""
    n = len(loop)
    loop_edges = {frozenset((loop[i], loop[(i + 1) % n])) for i in range(n)}
    for tris in _triangulations(list(loop)):
        ok = True
        for t in tris:
            for i in range(3):
                e = frozenset((t[i], t[(i + 1) % 3]))
                if e not in loop_edges and _shares_face(t[i], t[(i + 1) % 3]):
                    ok = False
                    break
            if not ok:
                break
        if ok:
            return tris
    raise RuntimeError(f"no face-free triangulation of loop {loop}")


def case_loops(case):
    nxt = {}
    for f in range(6):
        for a, b in face_segments(case, f):
            assert a not in nxt
            nxt[a] = b
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops


def build_table():
    """list of 256 lists of (e0, e1, e2) triangles."""
    table = []
    for case in range(256):
        tris = []
        for loop in case_loops(case):
            tris.extend(_triangulate(loop))
        table.append(tris)
    return table


TABLE = build_table()
MAX_TRIS = max(len(t) for t in TABLE)


def header_text():
    lines = ["// sph_mc_table.hpp -- GENERATED by `python -m sph_project_amd.mc_table` (sph_project_amd/mc_table.py); do not edit.",
             "// Marching-cubes case table of the surface reconstruction (DESIGN.md 14): inside corners separated on ambiguous faces,",
             "// loops triangulated without diagonals in a cube face, triangles counter-clockwise seen from the phi < iso side.",
             "#pragma once",
             f"#define SPH_MC_MAX_TRIS {MAX_TRIS}",
             "// triangles of each case",
             "__constant__ const unsigned char sph_mc_ntri[256] = {"]
    counts = [len(t) for t in TABLE]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(c) for c in counts[r:r + 32]) + ",")
    lines.append("};")
    lines.append(f"// edge ids of each case's triangles, 3 per triangle, padded with 12 to {MAX_TRIS} triangles")
    lines.append(f"__constant__ const unsigned char sph_mc_tri[256][{3 * MAX_TRIS}] = {{")
    for case in range(256):
        flat = [e for t in TABLE[case] for e in t]
        flat += [12] * (3 * MAX_TRIS - len(flat))
        lines.append("    {" + ", ".join(str(v) for v in flat) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "sph_mc_table.hpp")

if __name__ == "__main__":
    with open(HEADER_PATH, "w") as f:
        f.write(header_text())
    print(f"wrote {HEADER_PATH}: max {MAX_TRIS} triangles per case")
