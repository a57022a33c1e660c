"""Host model of the uniform grid's device tables (numpy, no GPU): a counting sort of the particles into cells and everything the
neighbour passes read through it -- cell_start, the per-tile headers, the cell words, and what correctness asks of the lane
permutation.  Written from the documented layout (include/sph_hip.h SphGridLayout / SphGridTable) and the reference's
grid build (base_container.py:496-557: pos_to_index, the counting sort, the prefix sum), not from the kernels.  All integer work:
check_tables compares exactly.

Frames: the model works in the LIBRARY's frame, library axis k = scene axis axis_map[k], x the slowest axis of the cell order.
to_library() brings scene-frame positions there."""
import numpy as np

TILE = 256            # particle slots per tile of the neighbour passes
HDR_INTS = 20         # [0] first cell, [1] last cell, [2..10] run start, [11..19] run length
SCAN_TILE_SHIFT = 11  # cell_start is scanned in tiles of 2048 cells


def make_layout(grid_num_scene, cell_size, n, axis_map=(0, 1, 2)):
    """The dict Engine.grid_layout() returns, for a grid given in the scene's frame (CPU tests)."""
    nx, ny, nz = (int(grid_num_scene[a]) for a in axis_map)
    return dict(nx=nx, ny=ny, nz=nz, G=nx * ny * nz, scan_tile=1 << SCAN_TILE_SHIFT, axis_map=tuple(int(a) for a in axis_map),
                cell_size=float(np.float32(cell_size)), n=int(n), tiles=(int(n) + TILE - 1) // TILE, tile_header_ints=HDR_INTS, tiles_valid=1)


def to_library(pos_scene, axis_map):
    """scene-frame rows -> library-frame rows"""
    return np.ascontiguousarray(np.asarray(pos_scene, np.float32)[:, list(axis_map)])


def cells_of(pos_lib, layout):
    """(cx, cy, cz, lin) of library-frame float32 positions: clamp(int(x / cell), 0, n_axis - 1) per axis, the division in float32"""
    pos = np.asarray(pos_lib, np.float32)
    cs = np.float32(layout["cell_size"])
    out = []
    for k, nk in enumerate((layout["nx"], layout["ny"], layout["nz"])):
        q = pos[:, k] / cs                                   # float32 IEEE division
        assert q.dtype == np.float32
        out.append(np.clip(np.trunc(q).astype(np.int64), 0, nk - 1))
    cx, cy, cz = out
    return cx, cy, cz, (cx * layout["ny"] + cy) * layout["nz"] + cz


class GridModel:
    """What a sort of `pos_lib` (library frame, in the slot order the sort found: `prev_ids[slot]` is the particle's id) must leave.

    lin_in        cell of every particle, in the order given
    cell_start    int64[G + 1], exclusive prefix sum of the populations, [G] = n
    order         the stable counting sort: new slot s holds old slot order[s]
    ids           prev_ids[order]: the ids in the new order (deterministic sorts must match it; others per cell as a set)
    lin, cx, cy, cz   cells in the new order
    headers       int64[tiles][20]
    cell_word     uint32[n]
    """

    def __init__(self, pos_lib, prev_ids, layout):
        self.layout = lay = dict(layout)
        n, G, ny, nz = len(pos_lib), lay["G"], lay["ny"], lay["nz"]
        assert n == len(prev_ids)
        self.n, self.tiles = n, (n + TILE - 1) // TILE
        cx, cy, cz, lin = cells_of(pos_lib, lay)
        self.lin_in = lin
        self.counts = np.bincount(lin, minlength=G).astype(np.int64)
        self.cell_start = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.order = np.argsort(lin, kind="stable")
        self.ids = np.asarray(prev_ids)[self.order]
        self.lin, self.cx, self.cy, self.cz = lin[self.order], cx[self.order], cy[self.order], cz[self.order]
        # tile headers
        t0 = np.arange(self.tiles) * TILE
        first = self.lin[t0] if n else np.zeros(0, np.int64)
        last = self.lin[np.minimum(t0 + TILE - 1, n - 1)] if n else np.zeros(0, np.int64)
        hdr = np.zeros((self.tiles, HDR_INTS), np.int64)
        hdr[:, 0], hdr[:, 1] = first, last
        for k in range(9):
            shift = (k // 3 - 1) * ny * nz + (k % 3 - 1) * nz
            lo, hi = first + shift - 1, last + shift + 1
            outside = (hi < 0) | (lo > G - 1)
            lo_c, hi_c = np.clip(lo, 0, G - 1), np.clip(hi, 0, G - 1)
            start = self.cell_start[lo_c]
            length = self.cell_start[hi_c + 1] - start
            hdr[:, 2 + k] = np.where(outside, 0, start)
            hdr[:, 11 + k] = np.where(outside, 0, length)
        self.headers = hdr
        # cell words
        z0 = np.maximum(self.cz - 1, 0)
        z1 = np.minimum(self.cz + 1, nz - 1)
        tile_first = first[np.arange(n) // TILE] if n else np.zeros(0, np.int64)
        entry = ((self.lin - tile_first) + (z0 - self.cz) + 1) & 0xff
        dom = np.zeros(n, np.int64)
        for ox in (-1, 0, 1):
            for oy in (-1, 0, 1):
                inside = (self.cx + ox >= 0) & (self.cx + ox < lay["nx"]) & (self.cy + oy >= 0) & (self.cy + oy < ny)
                dom |= inside.astype(np.int64) << (3 * (ox + 1) + (oy + 1))
        self.cell_word = (entry | ((z1 - z0 + 1) << 8) | (dom << 11)).astype(np.uint32)

    def tables(self):
        """tables that pass check_tables: the model's own, with the identity as lane permutation"""
        return dict(ids=self.ids.copy(), cell_start=self.cell_start.astype(np.int32), headers=self.headers.astype(np.int32),
                    lane_perm=np.tile(np.arange(TILE, dtype=np.uint8), (self.tiles, 1)), cell_word=self.cell_word.copy())


def _cell_start_violations(got, m):
    G, want = m.layout["G"], m.cell_start
    if got.shape != want.shape:
        return ["cell_start: %d entries, want G + 1 = %d" % (got.size, want.size)]
    bad = np.flatnonzero(got.astype(np.int64) != want)
    out = []
    if bad.size and bad[-1] == G:     # the entry behind the grid
        out.append("cell_start[G = %d] (the total): got %d, want n = %d" % (G, int(got[G]), int(want[G])))
        bad = bad[:-1]
    for t in np.unique(bad >> SCAN_TILE_SHIFT):
        c0, c1 = int(t) << SCAN_TILE_SHIFT, min((int(t) + 1) << SCAN_TILE_SHIFT, G)
        mine = bad[(bad >> SCAN_TILE_SHIFT) == t]
        held = int(m.counts[c0:c1].sum())
        c = int(mine[0])
        out.append("cell_start: scan tile %d (cells %d..%d, %s, %d particles before it): %d entries differ, first at cell %d: got %d, want %d"
                   % (t, c0, c1 - 1, "holds %d particles" % held if held else "empty", int(want[c0]), mine.size, c, int(got[c]), int(want[c])))
    return out


def _order_violations(got_ids, m, deterministic):
    if got_ids.shape != m.ids.shape:
        return ["order: %d ids, want %d" % (got_ids.size, m.ids.size)]
    if deterministic:
        bad = np.flatnonzero(got_ids != m.ids)
        if bad.size == 0:
            return []
        s = int(bad[0])
        same_set = np.array_equal(np.sort(got_ids), np.sort(m.ids))
        return ["order: %d slots differ from the stable counting sort (%s), first at slot %d (cell %d): holds id %d, want id %d"
                % (bad.size, "a permutation of the same ids" if same_set else "NOT the same set of ids", s, int(m.lin[s]), int(got_ids[s]), int(m.ids[s]))]
    a, b = np.lexsort((got_ids, m.lin)), np.lexsort((m.ids, m.lin))   # per cell as a multiset
    bad = np.flatnonzero(got_ids[a] != m.ids[b])
    if bad.size == 0:
        return []
    return ["order: the cells do not hold the model's particles: %d differences, first in cell %d" % (bad.size, int(m.lin[b][bad[0]]))]


def _header_violations(got, m):
    if got.shape != m.headers.shape:
        return ["tile headers: shape %s, want %s" % (got.shape, m.headers.shape)]
    names = ["first cell", "last cell"] + ["run start k=%d" % k for k in range(9)] + ["run length k=%d" % k for k in range(9)]
    out = []
    ts, fs = np.nonzero(got.astype(np.int64) != m.headers)
    for t in np.unique(ts)[:8]:
        f = fs[ts == t]
        out.append("tile header %d (cells %d..%d): %s" % (t, int(m.headers[t, 0]), int(m.headers[t, 1]),
                   "; ".join("%s got %d want %d" % (names[k], int(got[t, k]), int(m.headers[t, k])) for k in f[:4])))
    if np.unique(ts).size > 8:
        out.append("tile headers: %d more tiles differ" % (np.unique(ts).size - 8))
    return out


def _cell_word_violations(got, m):
    if got.shape != m.cell_word.shape:
        return ["cell words: %d, want %d" % (got.size, m.cell_word.size)]
    diff = got.astype(np.int64) ^ m.cell_word.astype(np.int64)
    out = []
    for name, mask in (("window entry (bits 0-7)", 0xff), ("z span (bits 8-10)", 0x700), ("column-exists bits (11-19)", 0xff800), ("bits above 19", ~0xfffff)):
        bad = np.flatnonzero(diff & mask)
        if bad.size:
            s = int(bad[0])
            out.append("cell word, %s: %d slots differ, first at slot %d (cell (%d, %d, %d) of a %d x %d x %d grid): got 0x%05x, want 0x%05x"
                       % (name, bad.size, s, int(m.cx[s]), int(m.cy[s]), int(m.cz[s]), m.layout["nx"], m.layout["ny"], m.layout["nz"],
                          int(got[s]), int(m.cell_word[s])))
    return out


def _lane_perm_violations(got, m):
    if got.shape != (m.tiles, TILE):
        return ["lane permutation: shape %s, want %s" % (got.shape, (m.tiles, TILE))]
    out = []
    srt = np.sort(got, axis=1)
    for t in np.flatnonzero((srt != np.arange(TILE, dtype=got.dtype)).any(axis=1))[:8]:
        vals, cnt = np.unique(got[t], return_counts=True)
        out.append("lane permutation of tile %d is no bijection of 0..255: byte %d occurs %d times" % (t, int(vals[cnt.argmax()]), int(cnt.max())))
    nvalid = m.n - (m.tiles - 1) * TILE
    if m.tiles and nvalid < TILE and (got[-1, :nvalid] >= nvalid).any():
        out.append("lane permutation of the last tile: a slot >= n = %d does not come last" % m.n)
    return out


def check_tables(tables, model, deterministic=True):
    """Human-readable violations of `tables` (dict: ids, cell_start, headers, lane_perm, cell_word -- a missing key is not checked)
    against the model; [] = every entry is right.  cell_start violations name the scan tile (cell >> 11) and say whether it holds
    particles; the lane permutation is checked for what correctness needs only (a bijection per tile, slots >= n last)."""
    out = []
    if "cell_start" in tables:
        out += _cell_start_violations(np.asarray(tables["cell_start"]), model)
    if "ids" in tables:
        out += _order_violations(np.asarray(tables["ids"]), model, deterministic)
    if "headers" in tables:
        out += _header_violations(np.asarray(tables["headers"]), model)
    if "cell_word" in tables:
        out += _cell_word_violations(np.asarray(tables["cell_word"]), model)
    if "lane_perm" in tables:
        out += _lane_perm_violations(np.asarray(tables["lane_perm"]), model)
    return out
