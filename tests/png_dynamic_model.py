"""The test-owned numpy encoder for coding="dynamic", written from DESIGN.md 21 ('Dynamic blocks'), not from the kernels.  Filters, the
token rule, the fixed code's tables and the chunk framing are those of tests/png_model.py; this file adds the per-segment choice among
stored, fixed and dynamic, the code lengths (two-queue Huffman for lit/len, package-merge for the distance and the code-length code),
canonical codes and the header's run-length rule.  encode() returns the file and fills `info` with the counters of SphPngStats and the
model's own notes (leading underscore) for the branch tests."""
import struct
import zlib

import numpy as np

from tests import png_model as M

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)   # RFC 1951 3.2.7
LL_LIMIT, DIST_LIMIT, CL_LIMIT = 15, 4, 7


def huffman_lengths(hist):
    """Plain Huffman depths by the two-queue construction.  The used symbols sorted by (count, symbol) are the leaf queue; an internal
    node joins the two lightest heads and goes to the back of the internal queue; a leaf is taken before an internal node of equal
    weight.  One used symbol gets length 1, none gives all zeros."""
    used = sorted((int(c), s) for s, c in enumerate(hist) if c > 0)
    n, out = len(used), [0] * len(hist)
    if n == 1:
        out[used[0][1]] = 1
    if n < 2:
        return out
    wt = [c for c, _ in used] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    leaf, inner = 0, n
    for node in range(n, 2 * n - 1):
        for _ in range(2):
            if leaf < n and (inner >= node or wt[leaf] <= wt[inner]):
                pick, leaf = leaf, leaf + 1
            else:
                pick, inner = inner, inner + 1
            wt[node] += wt[pick]
            parent[pick] = node
    for k, (_, s) in enumerate(used):
        at, depth = k, 0
        while at != 2 * n - 2:
            at, depth = parent[at], depth + 1
        out[s] = depth
    return out


def limited_lengths(hist, limit):
    """Optimal lengths under a limit by package-merge.  Leaves: the used symbols sorted by (count, symbol).  List 1 is the leaves; list
    j pairs the items of list j - 1 in order (an odd last item is dropped) and merges those packages with the leaves by weight, a leaf
    before a package of equal weight.  A symbol's length is the number of times it occurs in the first 2 n - 2 items of list `limit`.
    One used symbol gets length 1, none gives all zeros."""
    used = sorted((int(c), s) for s, c in enumerate(hist) if c > 0)
    n, out = len(used), [0] * len(hist)
    if n == 1:
        out[used[0][1]] = 1
    if n < 2:
        return out
    assert (1 << limit) >= n
    leaves = [(c, {s: 1}) for c, s in used]
    cur = leaves
    for _ in range(limit - 1):
        packs = []
        for k in range(0, len(cur) - 1, 2):
            both = dict(cur[k][1])
            for s, m in cur[k + 1][1].items():
                both[s] = both.get(s, 0) + m
            packs.append((cur[k][0] + cur[k + 1][0], both))
        nxt, a, b = [], 0, 0
        while a < n or b < len(packs):
            if a < n and (b >= len(packs) or leaves[a][0] <= packs[b][0]):
                nxt.append(leaves[a])
                a += 1
            else:
                nxt.append(packs[b])
                b += 1
        cur = nxt
    for _, members in cur[:2 * n - 2]:
        for s, m in members.items():
            out[s] += m
    return out


def kraft(lengths, limit):
    """sum of 2^(limit - length) over the used symbols; a complete code gives 2^limit"""
    return sum(1 << (limit - ln) for ln in lengths if ln)


def canonical(lengths):
    """symbol -> code (RFC 1951 3.2.2), most significant bit first"""
    top = max(lengths)
    count = [0] * (top + 2)
    for ln in lengths:
        if ln:
            count[ln] += 1
    nxt, code = [0] * (top + 2), 0
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lengths)
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = nxt[ln]
            nxt[ln] += 1
    return out


def run_length(seq):
    """[(code-length symbol, extra value, extra bits)] of the lit/len and distance lengths as one sequence.  A run of zeros: 18 in
    chunks of at most 138 while at least 11 remain, then one 17 for 3..10, else single zeros.  A run of a non-zero value: the value
    once, then 16 in chunks of at most 6 while at least 3 remain, else the value again."""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11, 7))
                r -= k
            if r >= 3:
                out.append((17, r - 3, 3))
                r = 0
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3, 2))
                r -= k
        out.extend([(v, 0, 0)] * r)
    return out


def parse(ln):
    """positions of the greedy parse's tokens"""
    pos, at, step = [], 0, np.maximum(ln, 1).tolist()
    while at < len(ln):
        pos.append(at)
        at += step[at]
    return np.asarray(pos, np.int64)


def histograms(b, tl, td):
    """lit/len counts [286] (with the end of block) and distance counts [5] of a segment's tokens (b: the byte at every token)"""
    lit = tl == 0
    ll = np.bincount(np.concatenate([b[lit].astype(np.int64), M.LEN_SYM[tl[~lit]], [256]]), minlength=286)
    dd = np.bincount(np.searchsorted(np.asarray(M.DIST), td[~lit]), minlength=5)
    return ll, dd


def dynamic_block(b, tl, td, final, notes):
    """(payload bytes, header bits) of the tokens (b: the byte at every token) as one dynamic block, or None when its lit/len code would pass 15 bits"""
    hist_ll, hist_d = histograms(b, tl, td)
    len_ll = huffman_lengths(hist_ll)
    if max(len_ll) > LL_LIMIT:
        notes["overlong"] += 1
        return None
    len_d = limited_lengths(hist_d, DIST_LIMIT)
    hlit = max(257, max(s for s in range(286) if len_ll[s]) + 1)
    hdist = max([1] + [s + 1 for s in range(5) if len_d[s]])
    rle = run_length(len_ll[:hlit] + len_d[:hdist])
    hist_cl = np.bincount([s for s, _, _ in rle], minlength=19)
    len_cl = limited_lengths(hist_cl, CL_LIMIT)
    hclen = max(4, max(k for k in range(19) if len_cl[CL_ORDER[k]]) + 1)
    assert kraft(len_ll, 15) == 1 << 15 and kraft(len_cl, 7) == 1 << 7 and max(len_cl) <= 7
    used_d = int((hist_d > 0).sum())
    assert kraft(len_d, 4) == (16 if used_d > 1 else 8 if used_d else 0)
    notes["cl_limit"] += max(huffman_lengths(hist_cl)) > CL_LIMIT
    notes["no_dist"] += used_d == 0
    notes["one_dist"] += used_d == 1
    notes["hlit286"] += hlit == 286
    notes["longest_code"] = max(notes["longest_code"], max(len_ll))

    code_ll, code_d, code_cl = canonical(len_ll), canonical(len_d), canonical(len_cl)
    vals, bits = [int(final) | 4, hlit - 257, hdist - 1, hclen - 4], [3, 5, 5, 4]      # BFINAL, BTYPE 10 (its low bit first)
    for k in range(hclen):
        vals.append(len_cl[CL_ORDER[k]])
        bits.append(3)
    for s, extra, eb in rle:
        vals.append(M._reverse(code_cl[s], len_cl[s]) | extra << len_cl[s])
        bits.append(len_cl[s] + eb)
    header_bits = sum(bits) - 3
    rev_ll = np.array([M._reverse(c, n) if n else 0 for c, n in zip(code_ll, len_ll)], np.int64)
    rev_d = np.array([M._reverse(c, n) if n else 0 for c, n in zip(code_d, len_d)], np.int64)
    nb_ll, nb_d = np.asarray(len_ll, np.int64), np.asarray(len_d, np.int64)
    lit = tl == 0
    sym = np.where(lit, b.astype(np.int64), M.LEN_SYM[tl])
    tv, tb = rev_ll[sym], nb_ll[sym]
    m = ~lit
    if m.any():
        v, nb = tv[m], tb[m]
        v |= (tl[m] - M.LEN_BASE_OF[tl[m]]) << nb
        nb = nb + M.LEN_EXTRA_OF[tl[m]]
        k = np.searchsorted(np.asarray(M.DIST), td[m])
        v |= rev_d[k] << nb
        nb = nb + nb_d[k]
        v |= (td[m] - np.asarray(M.DIST_BASE)[k]) << nb
        nb = nb + np.asarray(M.DIST_EXTRA)[k]
        tv[m], tb[m] = v, nb
    vals = np.concatenate([vals, tv, [rev_ll[256]]]).astype(np.int64)
    bits = np.concatenate([bits, tb, [nb_ll[256]]]).astype(np.int64)
    total = int(bits.sum())
    nbytes = -(-total // 8) if final else -(-(total + 3) // 8) + 4
    out = np.packbits(M._pack(vals, bits, 0, nbytes * 8), bitorder="little")
    if not final:                                    # the empty stored block 000 + padding, 00 00 FF FF
        out[-2:] = 0xFF
    return out.tobytes(), header_bits


def segment_payload(b, ln, ds, final, info):
    """The deflate bytes of one segment: today's choice (fixed, or stored when that is shorter) first, a dynamic block only when it
    is strictly shorter than that choice."""
    base_info = dict(stored_segments=0, literals=0, matches=0)
    base = M.segment_payload(b, ln, ds, final, base_info)
    pos = parse(ln)
    tl, td = ln[pos], ds[pos]
    dyn = dynamic_block(b[pos], tl, td, final, info["_notes"])
    if dyn is not None and len(dyn[0]) < len(base):
        info["dynamic_segments"] += 1
        info["dynamic_header_bits"] += dyn[1]
        info["literals"] += int((tl == 0).sum())
        info["matches"] += int((tl > 0).sum())
        info["_modes"].append(2)
        return dyn[0]
    for key in ("stored_segments", "literals", "matches"):
        info[key] += base_info[key]
    info["_modes"].append(0 if base_info["stored_segments"] else 1)
    return base


def encode(img, filt="adaptive", info=None):
    """The .png file of uint8 (H, W, 3) in coding="dynamic".  info receives the counters of SphPngStats, `_modes` (per segment 0 stored,
    1 fixed, 2 dynamic) and `_notes`: counts over the dynamic blocks offered (cl_limit: plain Huffman would have given the code-length
    code more than 7 bits; no_dist / one_dist: no or one distance code used; hlit286; overlong: lit/len code past 15, not offered) and
    longest_code, the longest lit/len code."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    info = {} if info is None else info
    rows, types = M.filtered(img, M.filter_setting(filt))
    b = rows.reshape(-1)
    raw = len(b)
    nseg = -(-raw // M.SEG)
    info.update(raw_bytes=raw, segments=nseg, stored_segments=0, literals=0, matches=0, dynamic_segments=0, dynamic_header_bits=0,
                filter_rows=[int((types == t).sum()) for t in range(5)], _modes=[],
                _notes=dict(cl_limit=0, no_dist=0, one_dist=0, hlit286=0, overlong=0, longest_code=0))
    ln, ds = M.match_lengths(b)
    out = [M.SIGNATURE, M._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))]
    zbytes = 0
    for k in range(nseg):
        lo, hi = k * M.SEG, min((k + 1) * M.SEG, raw)
        body = (b"\x78\x01" if k == 0 else b"") + segment_payload(b[lo:hi], ln[lo:hi], ds[lo:hi], k == nseg - 1, info)
        zbytes += len(body)
        out.append(M._chunk(b"IDAT", body))
    out.append(M._chunk(b"IDAT", struct.pack(">I", zlib.adler32(b.tobytes()) & 0xFFFFFFFF)))
    out.append(M._chunk(b"IEND", b""))
    data = b"".join(out)
    info.update(zlib_bytes=zbytes + 4, file_bytes=len(data))
    return data


def period5(width=2000):
    """Own picture, one row: under filter 0 its bytes repeat with period 5 (five distinct values), which none of the candidate
    distances 1, 2, 3, 4, 6 matches: literals only, an empty distance set."""
    v = np.array([10, 80, 150, 220, 45], np.uint8)
    return v[np.arange(3 * width) % 5].reshape(1, width, 3)
