"""Float64 restatement of the rigid contact pass (csrc/sph_contact.hpp, include/sph_hip.h sph_set_rigid_contact): brute force over
pairs, the same keys, bins and wall rule.  Pure numpy + scipy; no device, no library.

Targets are the particles of dynamic rigid objects (object id >= 0, not ghosts).  Partners are rigid particles of any other object
with 1e-6 < |x_i - x_j| < D; the domain box (object id -1) files under partner 20 + bin.  Without a box, the six planes wall_lo /
wall_hi are partners 20 + bin when a particle is closer than D / 2.  Table: [A][B][bin][pairs, midpoint sum (3), depth * n sum (3),
maximum depth]."""
import numpy as np
from scipy.spatial import cKDTree

NOBJ, PARTNERS, BINS, VALUES, WALL0 = 20, 26, 6, 8, 20


def bin_of(v):
    """2 * dominant axis (first of equal magnitudes) + (that component < 0), per row of v"""
    a = np.abs(v)
    ax = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    return 2 * ax + (v[np.arange(len(v)), ax] < 0)


def contact_pairs(pos, obj, mat, dyn, D, wall_lo=None, wall_hi=None, ghost=None, targets=None):
    """Every accepted contact as arrays: target index i, partner index j (-1 for a wall plane), key (A, B, bin), midpoint, depth * n,
    depth, and |r - D| (how close a particle pair sits to the acceptance edge, inf for planes)."""
    pos = np.asarray(pos, np.float64)
    obj, mat, dyn = np.asarray(obj), np.asarray(mat), np.asarray(dyn)
    ghost = np.zeros(len(pos), bool) if ghost is None else np.asarray(ghost).astype(bool)
    tgt_mask = (mat == 2) & (dyn != 0) & (obj >= 0) & ~ghost
    tgt = np.nonzero(tgt_mask)[0] if targets is None else np.asarray(targets)
    tgt = tgt[tgt_mask[tgt]]
    rig = np.nonzero(mat == 2)[0]
    tree = cKDTree(pos[rig])
    lists = tree.query_ball_point(pos[tgt], D)
    ii = np.repeat(tgt, [len(l) for l in lists])
    jj = rig[np.concatenate([np.asarray(l, np.int64) for l in lists])] if len(lists) else np.zeros(0, np.int64)
    d = pos[ii] - pos[jj]
    r = np.sqrt((d * d).sum(1))
    keep = (obj[jj] != obj[ii]) & (r > 1e-6) & (r < D)
    ii, jj, d, r = ii[keep], jj[keep], d[keep], r[keep]
    depth = D - r
    dn = d * (depth / r)[:, None]
    b = bin_of(d)
    B = np.where(obj[jj] >= 0, obj[jj], WALL0 + b)
    out = dict(i=ii, j=jj, A=obj[ii], B=B, bin=b, mid=0.5 * (pos[ii] + pos[jj]), dn=dn, depth=depth, edge=np.abs(r - D))
    if wall_lo is not None:
        rows = [out]
        for ax in range(3):
            for side in range(2):
                x = pos[tgt, ax]
                dist = x - wall_lo[ax] if side == 0 else wall_hi[ax] - x
                m = dist < 0.5 * D
                t, dist = tgt[m], dist[m]
                sg = 1.0 if side == 0 else -1.0
                dep = 0.5 * D - dist
                mid = pos[t].copy(); mid[:, ax] -= sg * dist
                dnv = np.zeros((len(t), 3)); dnv[:, ax] = sg * dep
                bn = np.full(len(t), 2 * ax + side)
                rows.append(dict(i=t, j=np.full(len(t), -1), A=obj[t], B=WALL0 + bn, bin=bn, mid=mid, dn=dnv, depth=dep,
                                 edge=np.full(len(t), np.inf)))
        out = {k: np.concatenate([r_[k] for r_ in rows]) for k in out}
    return out


def table_of(pairs):
    t = np.zeros((NOBJ, PARTNERS, BINS, VALUES))
    key = (pairs["A"], pairs["B"], pairs["bin"])
    np.add.at(t[..., 0], key, 1.0)
    for c in range(3):
        np.add.at(t[..., 1 + c], key, pairs["mid"][:, c])
        np.add.at(t[..., 4 + c], key, pairs["dn"][:, c])
    np.maximum.at(t[..., 7], key, pairs["depth"])
    return t


def per_particle(pairs, n):
    """(sum of depth * n, contact count) per particle"""
    dn, cnt = np.zeros((n, 3)), np.zeros(n)
    np.add.at(dn, pairs["i"], pairs["dn"])
    np.add.at(cnt, pairs["i"], 1.0)
    return dn, cnt


def contact_table(pos, obj, mat, dyn, D, wall_lo=None, wall_hi=None, ghost=None, targets=None):
    return table_of(contact_pairs(pos, obj, mat, dyn, D, wall_lo, wall_hi, ghost, targets))
