"""The test-owned numpy encoder for coding="window", written from DESIGN.md 21 ('Window matches'), not from the kernels.  Filters, the
five-distance token rule and the chunk framing are those of tests/png_model.py, the length rules and the stored / fixed / dynamic choice
those of tests/png_dynamic_model.py; this file adds the window candidate (the most recent earlier occurrence of a position's three bytes
within 32768 bytes of the whole filtered stream), the window parse, its dynamic block over all 30 distance symbols and the choice per
segment between that block and the dynamic coding's.  encode() returns the file and fills `info` with the counters of the encoder's
stats and the model's own notes (leading underscore) for the branch tests."""
import struct
import zlib

import numpy as np

from tests import png_dynamic_model as D
from tests import png_model as M

WINDOW = 32768
NONE = 0xFFFFFFFF            # prev: no candidate
FAR = 4096                   # a match further back than this counts as far
WDIST_LIMIT = 15
NDIST = 30
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]                                                      # RFC 1951 3.2.5
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def candidates(b):
    """prev[i] = c(i): the largest j < i with i - j <= WINDOW and b[j..j+2] == b[i..i+2]; NONE where there is none or i + 2 >= n.  A
    stable sort of the positions by their three bytes puts every position behind the most recent one with the same key."""
    n = len(b)
    prev = np.full(n, NONE, np.uint32)
    if n < 4:
        return prev
    v = b.astype(np.int64)
    key = v[:-2] | v[1:-1] << 8 | v[2:] << 16
    order = np.argsort(key, kind="stable")
    same = (key[order[1:]] == key[order[:-1]]) & (order[1:] - order[:-1] <= WINDOW)
    prev[order[1:][same]] = order[:-1][same]
    return prev


def window_lengths(b, prev):
    """L_w per position: the common prefix of b[i..] and b[c(i)..], at most 258 and not past the end of i's segment (0: no candidate)"""
    n = len(b)
    idx = np.flatnonzero(prev != NONE)
    src = prev[idx].astype(np.int64)
    end = np.minimum((idx // M.SEG + 1) * M.SEG, n)
    run = np.zeros(len(idx), np.int64)
    live = np.arange(len(idx))
    while len(live):
        at = idx[live] + run[live]
        ok = (run[live] < M.MAX_MATCH) & (at < end[live])
        live = live[ok]
        ok = b[idx[live] + run[live]] == b[src[live] + run[live]]      # (the source may overlap the target, and may cross a border)
        live = live[ok]
        run[live] += 1
    out = np.zeros(n, np.int64)
    out[idx] = run
    return out


def dist_symbol(d):
    return np.searchsorted(np.asarray(DIST_BASE), d, side="right") - 1


def window_tokens(b, prev):
    """(length, distance, taken from the window) per position: the longest of the five fixed-distance runs and L_w, among equal lengths
    the smaller distance; below 3 a literal.  The fixed run is taken before it is cut to a literal: a window candidate of the same
    length and distance as a fixed one is the fixed one."""
    n = len(b)
    idx = np.arange(n)
    best_len, best_dist = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for d in M.DIST:                                 # (as png_model.match_lengths, the runs kept below 3)
        eq = np.zeros(n, bool)
        eq[d:] = b[d:] == b[:-d]
        eq &= (idx % M.SEG) >= d
        stop = np.minimum.accumulate(np.where(eq, n, idx)[::-1])[::-1]
        run = np.minimum(stop - idx, M.MAX_MATCH)
        better = run > best_len
        best_len[better], best_dist[better] = run[better], d
    lw = window_lengths(b, prev)
    dw = np.where(prev != NONE, idx - prev.astype(np.int64), 0)
    take = (lw >= M.MIN_MATCH) & ((lw > best_len) | ((lw == best_len) & (dw < best_dist)))
    best_len[take], best_dist[take] = lw[take], dw[take]
    short = best_len < M.MIN_MATCH
    best_len[short], best_dist[short] = 0, 0
    return best_len, best_dist, take


def window_block(b, tl, td, final, notes):
    """(payload bytes, header bits) of the window parse's tokens (b: the byte at every token) as one dynamic block over the 30 distance
    symbols, or None when its lit/len code would pass 15 bits"""
    lit = tl == 0
    ds = dist_symbol(td[~lit])
    hist_ll = np.bincount(np.concatenate([b[lit].astype(np.int64), M.LEN_SYM[tl[~lit]], [256]]), minlength=286)
    hist_d = np.bincount(ds, minlength=NDIST)
    len_ll = D.huffman_lengths(hist_ll)
    if max(len_ll) > D.LL_LIMIT:
        notes["overlong"] += 1
        return None
    len_d = D.limited_lengths(hist_d, WDIST_LIMIT)
    hlit = max(257, max(s for s in range(286) if len_ll[s]) + 1)
    hdist = max([1] + [s + 1 for s in range(NDIST) if len_d[s]])
    rle = D.run_length(len_ll[:hlit] + len_d[:hdist])
    hist_cl = np.bincount([s for s, _, _ in rle], minlength=19)
    len_cl = D.limited_lengths(hist_cl, D.CL_LIMIT)
    hclen = max(4, max(k for k in range(19) if len_cl[D.CL_ORDER[k]]) + 1)
    used_d = int((hist_d > 0).sum())
    assert D.kraft(len_ll, 15) == 1 << 15 and D.kraft(len_cl, 7) == 1 << 7 and max(len_cl) <= 7 and max(len_d) <= 15
    assert D.kraft(len_d, 15) == ((1 << 15) if used_d > 1 else (1 << 14) if used_d else 0)
    assert hlit + hdist <= 316
    notes["most_dist_symbols"] = max(notes["most_dist_symbols"], used_d)
    notes["longest_dist_code"] = max(notes["longest_dist_code"], max(len_d))

    code_ll, code_d, code_cl = D.canonical(len_ll), D.canonical(len_d) if used_d else [0] * NDIST, D.canonical(len_cl)
    vals, bits = [int(final) | 4, hlit - 257, hdist - 1, hclen - 4], [3, 5, 5, 4]
    for k in range(hclen):
        vals.append(len_cl[D.CL_ORDER[k]])
        bits.append(3)
    for s, extra, eb in rle:
        vals.append(M._reverse(code_cl[s], len_cl[s]) | extra << len_cl[s])
        bits.append(len_cl[s] + eb)
    header_bits = sum(bits) - 3
    rev_ll = np.array([M._reverse(c, n) if n else 0 for c, n in zip(code_ll, len_ll)], np.int64)
    rev_d = np.array([M._reverse(c, n) if n else 0 for c, n in zip(code_d, len_d)], np.int64)
    nb_ll, nb_d = np.asarray(len_ll, np.int64), np.asarray(len_d, np.int64)
    sym = np.where(lit, b.astype(np.int64), M.LEN_SYM[tl])
    tv, tb = rev_ll[sym], nb_ll[sym]
    m = ~lit
    if m.any():
        v, nb = tv[m], tb[m]
        v |= (tl[m] - M.LEN_BASE_OF[tl[m]]) << nb
        nb = nb + M.LEN_EXTRA_OF[tl[m]]
        v |= rev_d[ds] << nb
        nb = nb + nb_d[ds]
        v |= (td[m] - np.asarray(DIST_BASE)[ds]) << nb
        nb = nb + np.asarray(DIST_EXTRA)[ds]
        tv[m], tb[m] = v, nb
    vals = np.concatenate([vals, tv, [rev_ll[256]]]).astype(np.int64)
    bits = np.concatenate([bits, tb, [nb_ll[256]]]).astype(np.int64)
    total = int(bits.sum())
    nbytes = -(-total // 8) if final else -(-(total + 3) // 8) + 4
    out = np.packbits(M._pack(vals, bits, 0, nbytes * 8), bitorder="little")
    if not final:
        out[-2:] = 0xFF
    return out.tobytes(), header_bits


def segment_payload(b, ln, ds, wl, wd, wt, final, info, force=False):
    """The deflate bytes of one segment: the dynamic coding's choice on the five-distance parse first, one dynamic block of the window
    parse only when it is strictly shorter (force: whenever it can be offered -- the unconditional parse of the model table)."""
    base_info = dict(stored_segments=0, literals=0, matches=0, dynamic_segments=0, dynamic_header_bits=0, _modes=[], _notes=info["_dnotes"])
    base = D.segment_payload(b, ln, ds, final, base_info)
    pos = D.parse(wl)
    tl, td = wl[pos], wd[pos]
    win = window_block(b[pos], tl, td, final, info["_notes"])
    info["_window_bytes"].append(len(win[0]) if win else None)
    info["_base_bytes"].append(len(base))
    if win is not None and (len(win[0]) < len(base) or force):
        from_window = wt[pos] & (tl > 0)
        info["window_segments"] += 1
        info["window_header_bits"] += win[1]
        info["window_matches"] += int(from_window.sum())
        info["window_far_matches"] += int((td > FAR).sum())
        info["literals"] += int((tl == 0).sum())
        info["matches"] += int((tl > 0).sum())
        info["_modes"].append(3)
        notes = info["_notes"]
        notes["longest"] = max(notes["longest"], int(tl.max()))
        notes["overlap"] += int(((td < tl) & from_window).sum())
        notes["capped"] += int((from_window & (pos + tl == len(b)) & (tl < M.MAX_MATCH)).sum())
        notes["crossing"] += int((from_window & (td > pos) & (td < pos + tl)).sum())      # starts before the segment, ends inside it
        return win[0]
    for key in ("stored_segments", "literals", "matches", "dynamic_segments", "dynamic_header_bits"):
        info[key] += base_info[key]
    info["_modes"].append(base_info["_modes"][0])
    return base


def encode(img, filt="adaptive", info=None, force=False):
    """The .png file of uint8 (H, W, 3) in coding="window".  info receives the counters of the encoder's stats, `_modes` (per segment 0
    stored, 1 fixed, 2 dynamic, 3 window), `_prev` (the candidates), `_base_bytes` / `_window_bytes` (per segment the payload of the
    dynamic coding's choice and of the window block, None where it is not offered) and `_notes` over the window blocks written:
    most_dist_symbols, longest_dist_code, longest match, overlap (distance < length), capped (a window match cut by the segment's end),
    crossing (a source that starts in the preceding segment and runs over the border), overlong (not offered: lit/len code past 15)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    info = {} if info is None else info
    rows, types = M.filtered(img, M.filter_setting(filt))
    b = rows.reshape(-1)
    raw = len(b)
    nseg = -(-raw // M.SEG)
    info.update(raw_bytes=raw, segments=nseg, stored_segments=0, literals=0, matches=0, dynamic_segments=0, dynamic_header_bits=0,
                window_segments=0, window_matches=0, window_far_matches=0, window_header_bits=0,
                filter_rows=[int((types == t).sum()) for t in range(5)], _modes=[], _base_bytes=[], _window_bytes=[],
                _dnotes=dict(cl_limit=0, no_dist=0, one_dist=0, hlit286=0, overlong=0, longest_code=0),
                _notes=dict(most_dist_symbols=0, longest_dist_code=0, longest=0, overlap=0, capped=0, crossing=0, overlong=0))
    ln, ds = M.match_lengths(b)
    prev = candidates(b)
    wl, wd, wt = window_tokens(b, prev)
    info["_prev"] = prev
    out = [M.SIGNATURE, M._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))]
    zbytes = 0
    for k in range(nseg):
        lo, hi = k * M.SEG, min((k + 1) * M.SEG, raw)
        body = (b"\x78\x01" if k == 0 else b"") + segment_payload(b[lo:hi], ln[lo:hi], ds[lo:hi], wl[lo:hi], wd[lo:hi], wt[lo:hi],
                                                                  k == nseg - 1, info, force)
        zbytes += len(body)
        out.append(M._chunk(b"IDAT", body))
    out.append(M._chunk(b"IDAT", struct.pack(">I", zlib.adler32(b.tobytes()) & 0xFFFFFFFF)))
    out.append(M._chunk(b"IEND", b""))
    data = b"".join(out)
    info.update(zlib_bytes=zbytes + 4, file_bytes=len(data))
    return data


def one_colour_discs(width, height, seed=7, count=None):
    """Own picture: shaded discs of one colour under one light on a flat background, as a particle frame has them"""
    rng = np.random.default_rng(seed)
    img = np.empty((height, width, 3), np.uint8)
    img[:] = (25, 25, 30)
    depth = np.full((height, width), np.inf)
    count = count or width * height // 600
    r = max(4, min(width, height) // 40)
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    inside = xx * xx + yy * yy <= r * r
    nz = np.sqrt(np.maximum(r * r - xx * xx - yy * yy, 0)) / r
    shade = np.clip(0.25 + 0.75 * (0.4 * xx / r - 0.5 * yy / r + 0.76 * nz), 0, 1)
    sprite = np.rint(shade[..., None] * np.array([40, 110, 230])).astype(np.uint8)
    for _ in range(count):
        cx, cy, z = int(rng.integers(0, width)), int(rng.integers(0, height)), float(rng.random())
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, height), max(cx - r, 0), min(cx + r + 1, width)
        sy, sx = slice(y0 - cy + r, y1 - cy + r), slice(x0 - cx + r, x1 - cx + r)
        vis = inside[sy, sx] & (z < depth[y0:y1, x0:x1])
        img[y0:y1, x0:x1][vis] = sprite[sy, sx][vis]
        depth[y0:y1, x0:x1][vis] = z
    return img
