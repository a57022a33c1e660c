// sph_png.hpp -- PNG encoding (one RGB frame on the device -> the IDAT chunks of a PNG file): kernels and launchers; included by
// sph_kernels.hip inside the per-build namespace.  The stream is defined in DESIGN.md 21, the entry points in include/sph_hip.h
// (sph_png_create), the restatement in tests/png_model.py.  Integer arithmetic only: the strict and the fast build write the same bytes.
//
// k_png_filter    one workgroup per row: the five costs (sum of |residual as int8|), the winner (ties: the lowest type), the filtered row
// k_png_segment   one workgroup (4 waves) per segment of PNG_SEG filtered bytes, held in LDS; thread t owns positions [16 t, 16 t + 16):
//   matches   per candidate distance a 16-bit mask of byte equalities; the run that starts at a position is the mask's trailing ones,
//             continued through the following threads' masks (their leading runs lie in LDS; at most 258 / 16 + 1 of them are read)
//   parse     next[i] = i + max(1, length[i]) is a chain from position 0.  Pointer doubling: in round r every marked position marks
//             next_r[i], then next_{r+1}[i] = next_r[next_r[i]]; the marked set doubles (the first 2^r tokens -> the first 2^(r+1)),
//             every lane works in every round, and the loop ends when 2^r hops from position 0 leave the segment
//   layout    the marked positions' bit counts scanned over the workgroup: fixed-code bytes against stored bytes, the shorter wins
//   bytes     (WRITE) every marked position ORs its bits into the segment's LDS image (deflate packs from bit 0: a little-endian word
//             image is the byte stream), the chunk goes to its scanned offset, and its CRC-32 is 256 pieces of PNG_CRC_PIECE bytes joined
//             by multiplication with x^(8 n) mod the polynomial (the message is right-aligned in the pieces: leading zeros leave a
//             zero register unchanged, so every join of a level uses one constant)
//   dynamic   (the DYN instantiations, coding = dynamic) COUNT also builds the segment's own codes from its tokens' histograms and keeps
//             a dynamic block where it is strictly shorter; the lengths go to a side record from which WRITE rebuilds the canonical codes
//   window    (the WIN instantiations, coding = window) COUNT then parses the segment again with one more candidate per position -- prev[],
//             the most recent earlier occurrence of its three bytes within 32 KB of the whole stream, from the sort at the end of this
//             file -- builds that parse's codes over all 30 distance symbols and keeps its block where it is shorter still; WRITE
//             parses only the parse that was chosen
// The kernel runs twice per frame as the video encoder's does: COUNT leaves the chunk's byte count and the Adler sums, k_png_scan scans
// the counts (the host sizes the output from the total) and joins the Adler sums, WRITE computes the same bytes again and stores them.
#pragma once

#define PNG_PER (PNG_SEG / 256)                // positions per thread
#define PNG_IMG_WORDS (PNG_SEG / 2 + 8)        // next[PNG_SEG + 1] as 16-bit values, later the bit image (<= 2 + 5 + PNG_SEG bytes + 2 words)
static_assert(PNG_PER == 16, "a thread's byte equalities are one 16-bit mask");
static_assert(PNG_SEG < 65535, "positions fit 16 bits, a segment fits one stored block");
static_assert(PNG_IMG_WORDS * 4 >= (PNG_SEG + 1) * 2 && PNG_IMG_WORDS * 4 >= 2 + 5 + PNG_SEG + 8, "the image array holds both of its uses");

static __device__ const int PNG_DIST[PNG_ND] = PNG_DIST_LIST;

__device__ __forceinline__ int png_abs8(int r) { return r < 128 ? r : 256 - r; }

// the residual of filter type t: x the byte, a the byte of the pixel to the left, b above, c above left
__device__ __forceinline__ int png_residual(int t, int x, int a, int b, int c) {
    int pred = 0;
    if (t == 1) pred = a;
    else if (t == 2) pred = b;
    else if (t == 3) pred = (a + b) >> 1;
    else if (t == 4) {
        const int p = a + b - c;
        const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (x - pred) & 255;
}

__global__ void __launch_bounds__(256) k_png_filter(PngDev d) {
    __shared__ int s_cost[4][5];
    __shared__ int s_type;
    const int tid = threadIdx.x, y = blockIdx.x, n = 3 * d.W;
    const unsigned char *cur = d.rgb + (size_t)y * n;
    const unsigned char *up = y ? cur - n : nullptr;   // row 0 sees a zero row above it
    int type = d.filter;
    if (type < 0) {   // (workgroup-uniform)
        int cost[5] = {0, 0, 0, 0, 0};   // <= 3 x 16384 x 128: an int
        for (int j = tid; j < n; j += 256) {
            const int x = cur[j], a = j >= 3 ? cur[j - 3] : 0, b = up ? up[j] : 0, c = (up && j >= 3) ? up[j - 3] : 0;
#pragma unroll
            for (int t = 0; t < 5; ++t) cost[t] += png_abs8(png_residual(t, x, a, b, c));
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int v = video_wave_sum(cost[t]);
            if ((tid & 63) == 0) s_cost[tid >> 6][t] = v;
        }
        __syncthreads();
        if (tid == 0) {
            int best = 0, bc = 0;
            for (int t = 0; t < 5; ++t) {
                const int v = s_cost[0][t] + s_cost[1][t] + s_cost[2][t] + s_cost[3][t];
                if (t == 0 || v < bc) { best = t; bc = v; }
            }
            s_type = best;
        }
        __syncthreads();
        type = s_type;
    }
    unsigned char *o = d.flt + (size_t)y * d.stride;
    if (tid == 0) { o[0] = (unsigned char)type; atomicAdd(&d.cnt[type], 1ull); }
    for (int j = tid; j < n; j += 256) {
        const int x = cur[j], a = j >= 3 ? cur[j - 3] : 0, b = up ? up[j] : 0, c = (up && j >= 3) ? up[j - 3] : 0;
        o[1 + j] = (unsigned char)png_residual(type, x, a, b, c);
    }
}

// a Huffman code enters the stream most significant bit first: the n-bit code reversed
__device__ __forceinline__ unsigned png_rev(unsigned v, int n) { return __brev(v) >> (32 - n); }

// the bits of a literal / of a match in the fixed code (RFC 1951 3.2.5, 3.2.6), in stream order from bit 0 of val
__device__ __forceinline__ void png_literal(unsigned b, unsigned &val, int &nb) {
    if (b < 144u) { val = png_rev(0x30u + b, 8); nb = 8; }
    else { val = png_rev(0x190u + b - 144u, 9); nb = 9; }
}
// the lit/len symbol of a match length, its extra bits and their value
__device__ __forceinline__ void png_len_sym(int len, int &sym, int &eb, unsigned &ev) {
    const int l = len - 3;
    eb = 0; ev = 0u;
    if (len == 258) sym = 285;
    else if (l < 8) sym = 257 + l;
    else { eb = 29 - __clz(l); sym = 257 + 4 * eb + (l >> eb); ev = (unsigned)l & ((1u << eb) - 1u); }   // groups of four codes per extra bit
}
__device__ __forceinline__ void png_match(int len, int dist, unsigned &val, int &nb) {
    int sym, eb;
    unsigned ev;
    png_len_sym(len, sym, eb, ev);
    if (sym < 280) { val = png_rev((unsigned)sym - 256u, 7); nb = 7; }
    else { val = png_rev(0xC0u + (unsigned)sym - 280u, 8); nb = 8; }
    val |= ev << nb; nb += eb;
    const int m = dist - 1;
    int dc = m, db = 0;
    unsigned dv = 0u;
    if (m >= 4) { db = 30 - __clz(m); dc = 2 * db + 2 + ((m >> db) & 1); dv = (unsigned)m & ((1u << db) - 1u); }   // pairs of codes per extra bit
    val |= png_rev((unsigned)dc, 5) << nb; nb += 5;
    val |= dv << nb; nb += db;   // <= 8 + 5 + 5 + 13 = 31 bits
}

__device__ __forceinline__ unsigned png_crc_byte(unsigned r, unsigned b) {
    r ^= b;
#pragma unroll
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (PNG_CRC_POLY & (0u - (r & 1u)));
    return r;
}

// --- dynamic blocks (coding = dynamic; DESIGN.md 21 'Dynamic blocks') ---
// A segment's side record (PNG_SIDE bytes, written by the count pass, read by the write pass): the lengths of the lit/len code [286],
// of the distance code [5] and of the code-length code [19] as bytes, then two ints: the mode (0 stored, 1 fixed, 2 dynamic) and the
// header's bits (HLIT ... the last coded length).
#define PNG_NLL 286
#define PNG_NDC 5
#define PNG_NCL 19
#define PNG_NLEN (PNG_NLL + PNG_NDC + PNG_NCL)   // 310 lengths, padded to 312 bytes
static_assert(PNG_ND == PNG_NDC, "the candidate distances 1, 2, 3, 4, 6 are the distance codes 0..4 (code 4: 5..6, one extra bit)");
static_assert(PNG_SIDE == 312 + 8, "lengths, mode, header bits");
static __device__ const unsigned char PNG_CL_ORDER[PNG_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
// the count pass's arrays inside s_img (words), which is free between the end of pointer doubling and the bit image
#define PNG_C_HLL 0        // [288] lit/len counts
#define PNG_C_HD 288       // [8] distance counts
#define PNG_C_HCL 296      // [24] code-length symbol counts
#define PNG_C_SYM 320      // [288] the symbol of every leaf, leaves sorted by (count, symbol)
#define PNG_C_WT 608       // [572] weights of the leaves, then of the internal nodes in the order they are made
#define PNG_C_PAR 1180     // [572] 16-bit parents
#define PNG_C_LEN 1466     // [312] bytes: the three length arrays as in the side record
#define PNG_C_PMW 1544     // [100] package-merge: leaf weights [20], two lists of [40]
#define PNG_C_PML 1644     // [100] the items' symbol multiplicities, 3 bits per symbol: low words
#define PNG_C_PMH 1744     // [100] high words
#define PNG_C_MISC 1844    // [0] the lit/len code is deeper than 15, [1] header bits
static_assert(PNG_C_MISC + 8 <= PNG_IMG_WORDS, "the count pass's arrays fit the image array");

__device__ __forceinline__ int png_fixed_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// Optimal code lengths under `limit` by package-merge, one lane.  Leaves: the used symbols sorted by (count, symbol).  List 1 is the
// leaves; list j pairs the items of list j - 1 in order (an odd last item is dropped) and merges the packages with the leaves by weight,
// a leaf before a package of equal weight.  A symbol's length is the number of times it occurs in the first 2 n - 2 items of the last
// list.  An item carries its symbols' multiplicities (<= limit <= 7) in 3 bits per symbol (nsym <= 19: 57 bits, two words).
__device__ __forceinline__ void png_package_merge(const unsigned *hist, int nsym, int limit, unsigned char *out, unsigned *w, unsigned *ml, unsigned *mh) {
    int n = 0;
    for (int s = 0; s < nsym; ++s) {
        out[s] = 0;
        const unsigned c = hist[s];
        if (!c) continue;
        int j = n++;
        for (; j > 0 && w[j - 1] > c; --j) { w[j] = w[j - 1]; ml[j] = ml[j - 1]; mh[j] = mh[j - 1]; }   // (symbols ascend: behind its equals)
        const unsigned long long m = 1ull << (3 * s);
        w[j] = c; ml[j] = (unsigned)m; mh[j] = (unsigned)(m >> 32);
    }
    if (n == 0) return;
    if (n == 1) { out[ml[0] ? __builtin_ctz(ml[0]) / 3 : (32 + __builtin_ctz(mh[0])) / 3] = 1; return; }
    int cur = 20, nxt = 60, ncur = n;
    for (int k = 0; k < n; ++k) { w[cur + k] = w[k]; ml[cur + k] = ml[k]; mh[cur + k] = mh[k]; }
    for (int lev = 2; lev <= limit; ++lev) {
        const int np = ncur >> 1;
        int a = 0, b = 0, k = 0;
        while (a < n || b < np) {   // (k < n + np <= 19 + 18)
            const unsigned pw = b < np ? w[cur + 2 * b] + w[cur + 2 * b + 1] : 0u;
            if (a < n && (b >= np || w[a] <= pw)) { w[nxt + k] = w[a]; ml[nxt + k] = ml[a]; mh[nxt + k] = mh[a]; ++a; }
            else {
                const unsigned long long m = ((unsigned long long)mh[cur + 2 * b] << 32 | ml[cur + 2 * b]) +
                                             ((unsigned long long)mh[cur + 2 * b + 1] << 32 | ml[cur + 2 * b + 1]);
                w[nxt + k] = pw; ml[nxt + k] = (unsigned)m; mh[nxt + k] = (unsigned)(m >> 32);
                ++b;
            }
            ++k;
        }
        const int t = cur; cur = nxt; nxt = t;
        ncur = k;
    }
    unsigned long long tot = 0ull;
    for (int k = 0; k < 2 * n - 2; ++k) tot += (unsigned long long)mh[cur + k] << 32 | ml[cur + k];   // (2^limit >= n: the list is long enough)
    for (int s = 0; s < nsym; ++s) out[s] = (unsigned char)((tot >> (3 * s)) & 7ull);
}

// The lit/len lengths [0, hlit) and the distance lengths [0, hdist) run-length coded as one sequence (RFC 1951 3.2.7), one lane.  Zeros:
// 18 in chunks of at most 138 while at least 11 remain, then one 17 for 3..10, else single zeros.  A non-zero value: once, then 16 in
// chunks of at most 6 while at least 3 remain, else the value again.  emit(code-length symbol, extra value, extra bits).
template <class F>
__device__ __forceinline__ void png_run_length(const unsigned char *len, int hlit, int hdist, F emit) {
    const int N = hlit + hdist;
    int i = 0;
    while (i < N) {
        const int v = len[i < hlit ? i : PNG_NLL + i - hlit];
        int r = 1;
        while (i + r < N && len[i + r < hlit ? i + r : PNG_NLL + i + r - hlit] == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) { const int k = min(r, 138); emit(18, k - 11, 7); r -= k; }
            if (r >= 3) { emit(17, r - 3, 3); r = 0; }
        } else {
            emit(v, 0, 0); --r;
            while (r >= 3) { const int k = min(r, 6); emit(16, k - 3, 2); r -= k; }
        }
        for (; r > 0; --r) emit(v, 0, 0);
    }
}
__device__ __forceinline__ int png_hlit(const unsigned char *len) { int h = PNG_NLL; while (h > 257 && !len[h - 1]) --h; return h; }
template <int ND = PNG_NDC>   // (ND: the distance symbols of the length arrays; PNG_WND in the window coding's)
__device__ __forceinline__ int png_hdist(const unsigned char *len) { int h = ND; while (h > 1 && !len[PNG_NLL + h - 1]) --h; return h; }
template <int ND = PNG_NDC>
__device__ __forceinline__ int png_hclen(const unsigned char *len) {
    int h = PNG_NCL;
    while (h > 4 && !len[PNG_NLL + ND + PNG_CL_ORDER[h - 1]]) --h;
    return h;
}

// the canonical code (RFC 1951 3.2.2) of entry e of the three length arrays: the shorter codes of its array before it, then the codes
// of its length at smaller symbols.  Returned as the code reversed (stream order) | length << 16; 0 for an unused symbol.
template <int ND = PNG_NDC>
__device__ __forceinline__ unsigned png_canonical(const unsigned char *len, int e) {
    const int lo = e < PNG_NLL ? 0 : e < PNG_NLL + ND ? PNG_NLL : PNG_NLL + ND;
    const int hi = e < PNG_NLL ? PNG_NLL : e < PNG_NLL + ND ? PNG_NLL + ND : PNG_NLL + ND + PNG_NCL;
    const int l = len[e];
    if (!l) return 0u;
    unsigned code = 0u;
    for (int k = lo; k < hi; ++k) {
        const int lk = len[k];
        if (lk && lk < l) code += 1u << (l - lk);
        else if (lk == l && k < e) code += 1u;
    }
    return png_rev(code, l) | (unsigned)l << 16;
}

// a token in the segment's own code (tab: png_canonical of the 310 entries); <= 15 + 5 + 4 + 1 bits
__device__ __forceinline__ void png_dyn_token(const unsigned *tab, unsigned t, unsigned byte, unsigned &val, int &nb) {
    if (!t) { const unsigned e = tab[byte]; val = e & 0xFFFFu; nb = (int)(e >> 16); return; }
    int sym, eb;
    unsigned ev;
    png_len_sym((int)(t & 511u), sym, eb, ev);
    const unsigned e = tab[sym], q = t >> 9, f = tab[PNG_NLL + q];
    val = e & 0xFFFFu; nb = (int)(e >> 16);
    val |= ev << nb; nb += eb;
    val |= (f & 0xFFFFu) << nb; nb += (int)(f >> 16);
    if (q == 4u) { val |= 1u << nb; nb += 1; }   // distance 6: code 4 (5..6), extra bit 1
}

// --- window matches (coding = window; DESIGN.md 21 'Window matches') ---
// prev[i] = c(i), the most recent earlier position within PNG_WINDOW whose three bytes are those at i, comes from the candidate sort
// below.  A token of the window parse is 32 bits: length | distance << 9 | (it came from the window candidate) << 25.  The window block's
// lengths: lit/len [286], distance [PNG_WND], code-length code [19], padded to PNG_WLEN_WORDS words.  A segment's side record is the
// dynamic coding's (the choice on the five-distance parse) followed by these lengths and two ints: 3 when the window block is written
// (else 0), and its header's bits.
#define PNG_WND 30
#define PNG_WLEN_WORDS 84
#define PNG_WNLEN (PNG_NLL + PNG_WND + PNG_NCL)
static_assert(4 * PNG_WLEN_WORDS >= PNG_WNLEN && PNG_WSIDE >= PNG_SIDE + 4 * PNG_WLEN_WORDS + 8 && PNG_WSIDE % 16 == 0, "the window record holds both parts");
// the window count pass's arrays inside s_img (words), as PNG_C_* above; its package-merge lists lie in an array of their own
#define PNG_W_HLL 0        // [288]
#define PNG_W_HD 288       // [32]
#define PNG_W_HCL 320      // [24]
#define PNG_W_SYM 344      // [288]
#define PNG_W_WT 632       // [572]
#define PNG_W_PAR 1204     // [572] 16-bit parents
#define PNG_W_LEN 1490     // [PNG_WLEN_WORDS]
#define PNG_W_MISC 1574    // [0] the lit/len code is deeper than 15, [1] header bits
#define PNG_W_PM 750       // words of the lists: weights [150] (leaves [30], two lists of [60]), multiplicities [150][4]
static_assert(PNG_W_MISC + 8 <= PNG_IMG_WORDS, "the window count pass's arrays fit the image array");

// the distance symbol of a match distance, its extra bits and their value
__device__ __forceinline__ void png_dist_sym(int dist, int &dc, int &db, unsigned &dv) {
    const int m = dist - 1;
    dc = m; db = 0; dv = 0u;
    if (m >= 4) { db = 30 - __clz(m); dc = 2 * db + 2 + ((m >> db) & 1); dv = (unsigned)m & ((1u << db) - 1u); }   // pairs of codes per extra bit
}

// png_package_merge for the PNG_WND distance symbols under limit 15: multiplicities (<= 15) in 4 bits per symbol, four words per item;
// a list has fewer than 2 n <= 60 items
__device__ __forceinline__ void png_package_merge_wide(const unsigned *hist, unsigned char *out, unsigned *w, unsigned *mu) {
    int n = 0;
    for (int s = 0; s < PNG_WND; ++s) {
        out[s] = 0;
        const unsigned c = hist[s];
        if (!c) continue;
        int j = n++;
        for (; j > 0 && w[j - 1] > c; --j) {
            w[j] = w[j - 1];
            for (int q = 0; q < 4; ++q) mu[4 * j + q] = mu[4 * (j - 1) + q];
        }
        w[j] = c;
        for (int q = 0; q < 4; ++q) mu[4 * j + q] = (s >> 3) == q ? 1u << (4 * (s & 7)) : 0u;
    }
    if (n == 0) return;
    if (n == 1) { for (int s = 0; s < PNG_WND; ++s) if (hist[s]) out[s] = 1; return; }
    int cur = 30, nxt = 90, ncur = n;
    for (int k = 0; k < n; ++k) {
        w[cur + k] = w[k];
        for (int q = 0; q < 4; ++q) mu[4 * (cur + k) + q] = mu[4 * k + q];
    }
    for (int lev = 2; lev <= 15; ++lev) {
        const int np = ncur >> 1;
        int a = 0, b = 0, k = 0;
        while (a < n || b < np) {   // (k < n + np <= 30 + 29)
            const unsigned pw = b < np ? w[cur + 2 * b] + w[cur + 2 * b + 1] : 0u;
            if (a < n && (b >= np || w[a] <= pw)) {
                w[nxt + k] = w[a];
                for (int q = 0; q < 4; ++q) mu[4 * (nxt + k) + q] = mu[4 * a + q];
                ++a;
            } else {
                w[nxt + k] = pw;
                for (int q = 0; q < 4; ++q) mu[4 * (nxt + k) + q] = mu[4 * (cur + 2 * b) + q] + mu[4 * (cur + 2 * b + 1) + q];   // (no field passes 15)
                ++b;
            }
            ++k;
        }
        const int t = cur; cur = nxt; nxt = t;
        ncur = k;
    }
    unsigned tot[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < min(2 * n - 2, ncur); ++k)
        for (int q = 0; q < 4; ++q) tot[q] += mu[4 * (cur + k) + q];
    for (int s = 0; s < PNG_WND; ++s) out[s] = (unsigned char)((tot[s >> 3] >> (4 * (s & 7))) & 15u);
}

// the 32 bits at byte offset o of a little-endian word array (the word behind them is read too: the arrays have one to spare)
__device__ __forceinline__ unsigned png_word_at(const unsigned *w, int o) {
    return __builtin_amdgcn_alignbyte(w[(o >> 2) + 1], w[o >> 2], (unsigned)o & 3u);
}
// how many bytes from offset t of tgt equal the source's (src(l): its 32 bits at l bytes in), at most cap: four bytes a step
template <class S>
__device__ __forceinline__ int png_common_prefix(const unsigned *tgt, int t, S src, int cap) {
    int l = 0;
    while (l < cap) {
        const unsigned x = png_word_at(tgt, t + l) ^ src(l);
        if (x) { l += __builtin_ctz(x) >> 3; break; }
        l += 4;
    }
    return min(l, cap);
}

// The window parse's tokens of thread tid's positions and their next pointers.  The five distances' masks and entering runs are made
// again here as k_png_segment makes them (from the bytes and s_lead: cheaper than keeping them in registers across the count pass's
// first code construction).  The candidate's length is compared in LDS when its source lies in the segment and in the stream when it
// starts before it; a candidate at one of the five distances whose source lies in the segment is that distance's run and is skipped.
__device__ __forceinline__ void png_window_tokens(const PngDev &d, int seg, int n, int tid, const unsigned *s_raw, const unsigned short (*s_lead)[256],
                                                  unsigned *s_wtok, unsigned short *s_next) {
    const int base = tid * PNG_PER, start = seg * PNG_SEG;
    const unsigned char *s_b = (const unsigned char *)s_raw;
    unsigned m[PNG_ND];
    int carry[PNG_ND];
    {
        unsigned char c[8 + PNG_PER];
#pragma unroll
        for (int k = 0; k < 8 + PNG_PER; ++k) c[k] = base + k >= 8 ? s_b[base + k - 8] : (unsigned char)0;
#pragma unroll
        for (int q = 0; q < PNG_ND; ++q) {
            const int dist = PNG_DIST[q];
            unsigned mk = 0u;
#pragma unroll
            for (int k = 0; k < PNG_PER; ++k)
                if (base + k >= dist && base + k < n && c[8 + k] == c[8 + k - dist]) mk |= 1u << k;
            m[q] = mk;
            int r = 0;
            for (int u = tid + 1; u < 256 && r < 258; ++u) {
                const unsigned v = s_lead[q][u];
                r += (int)(v & 0x7FFFu);
                if (!(v & 0x8000u)) break;
            }
            carry[q] = r;
        }
    }
    unsigned pv[PNG_PER];
#pragma unroll
    for (int q = 0; q < PNG_PER / 4; ++q) {   // (prev is allocated in whole segments: entries behind the stream's end are read, not used)
        const uint4 v = ((const uint4 *)(d.prev + (size_t)start + base))[q];
        pv[4 * q] = v.x; pv[4 * q + 1] = v.y; pv[4 * q + 2] = v.z; pv[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < PNG_PER; ++k) {
        const int i = base + k;
        int best = 0, bq = 0;
#pragma unroll
        for (int q = 0; q < PNG_ND; ++q) {
            int run = __builtin_ctz(~(m[q] >> k));
            if (run == PNG_PER - k) run += carry[q];
            run = min(run, 258);
            if (run > best) { best = run; bq = q; }
        }
        int len = best, dist = PNG_DIST[bq];
        unsigned from = 0u;
        const unsigned p = i < n ? pv[k] : PNG_NONE;
        if (p != PNG_NONE) {
            const int dw = start + i - (int)p, j = (int)p - start;
            if (!(j >= 0 && (dw <= 4 || dw == 6))) {
                const int cap = min(258, n - i);
                int lw;
                if (j >= 0) lw = png_common_prefix(s_raw, i, [&](int l) { return png_word_at(s_raw, j + l); }, cap);
                else lw = png_common_prefix(s_raw, i, [&](int l) { return png_word_at((const unsigned *)d.flt, (int)p + l); }, cap);
                if (lw >= 3 && (lw > best || (lw == best && dw < dist))) { len = lw; dist = dw; from = 1u; }   // equal lengths: the smaller distance
            }
        }
        if (len < 3) { len = 0; dist = 0; }
        s_wtok[i] = (unsigned)len | (unsigned)dist << 9 | from << 25;
        s_next[i] = (unsigned short)(i < n ? i + max(len, 1) : n);
    }
}

// the pointer doubling of k_png_segment's parse once more, for the window count pass's second parse (all threads of the workgroup)
__device__ __forceinline__ void png_chain(unsigned short *s_next, unsigned char *s_mark, int n, int tid) {
    for (int r = 0; r < 12; ++r) {
        if (s_next[0] >= n) break;
        unsigned short j[PNG_PER], jj[PNG_PER];
        unsigned char mk[PNG_PER];
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k) {
            const int i = tid + 256 * k;
            j[k] = s_next[i];
            jj[k] = s_next[j[k]];
            mk[k] = s_mark[i];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k) {
            const int i = tid + 256 * k;
            if (mk[k]) s_mark[j[k]] = 1;
            s_next[i] = jj[k];
        }
        __syncthreads();
    }
    __syncthreads();
}

// (all threads of the workgroup) The codes of the window parse's marked tokens, as the dynamic count pass builds them for the five-distance
// parse: lit/len by two queues, the PNG_WND distance symbols by package-merge under 15, the code-length code under 7.  The lengths are
// left at s_img + PNG_W_LEN; returns the block's bits (3 + header + tokens + end of block); ok: the lit/len code stays within 15.
__device__ __forceinline__ int png_window_codes(unsigned *s_img, unsigned *s_pm, unsigned *s_red, const unsigned *s_wtok, const unsigned char *s_mark,
                                                const unsigned char *s_b, int n, int tid, int &hbits, bool &ok) {
    unsigned *h_ll = s_img + PNG_W_HLL, *h_d = s_img + PNG_W_HD, *h_cl = s_img + PNG_W_HCL, *l_sym = s_img + PNG_W_SYM, *wt = s_img + PNG_W_WT;
    unsigned short *par = (unsigned short *)(s_img + PNG_W_PAR);
    unsigned char *len = (unsigned char *)(s_img + PNG_W_LEN);
    unsigned *misc = s_img + PNG_W_MISC;
    for (int w = tid; w < PNG_W_SYM; w += 256) s_img[w] = 0u;
    if (tid < PNG_WLEN_WORDS) s_img[PNG_W_LEN + tid] = 0u;
    if (tid < 8) misc[tid] = 0u;
    __syncthreads();
    int xbits = 0;   // the extra bits of the thread's matches
    for (int k = 0; k < PNG_PER; ++k) {
        const int i = tid * PNG_PER + k;
        if (i < n && s_mark[i]) {
            const unsigned t = s_wtok[i];
            if (t) {
                int sym, eb, dc, db;
                unsigned ev, dv;
                png_len_sym((int)(t & 511u), sym, eb, ev);
                png_dist_sym((int)((t >> 9) & 0xFFFFu), dc, db, dv);
                atomicAdd(&h_ll[sym], 1u);
                atomicAdd(&h_d[dc], 1u);
                xbits += eb + db;
            } else atomicAdd(&h_ll[s_b[i]], 1u);
        }
    }
    if (tid == 0) atomicAdd(&h_ll[256], 1u);   // the end of block
    __syncthreads();
    int nleaf = 0;
    {   // the used lit/len symbols sorted by (count, symbol)
        const int s0 = tid, s1 = tid + 256;
        const unsigned c0 = h_ll[s0], c1 = s1 < PNG_NLL ? h_ll[s1] : 0u;
        const unsigned k0 = c0 << 9 | (unsigned)s0, k1 = c1 << 9 | (unsigned)s1;
        int r0 = 0, r1 = 0;
        for (int j = 0; j < PNG_NLL; ++j) {
            const unsigned cj = h_ll[j], kj = cj << 9 | (unsigned)j;
            if (cj) { ++nleaf; r0 += kj < k0; r1 += kj < k1; }
        }
        if (c0) { l_sym[r0] = (unsigned)s0; wt[r0] = c0; }
        if (c1) { l_sym[r1] = (unsigned)s1; wt[r1] = c1; }
    }
    __syncthreads();
    const int root = 2 * nleaf - 2;   // (nleaf >= 2: a literal or a length, and the end of block)
    if (tid == 0) {
        int leaf = 0, inner = nleaf;
        for (int node = nleaf; node <= root; ++node) {
            unsigned sum = 0u;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                int pick;
                if (leaf < nleaf && (inner >= node || wt[leaf] <= wt[inner])) pick = leaf++;
                else pick = inner++;
                sum += wt[pick];
                par[pick] = (unsigned short)node;
            }
            wt[node] = sum;
        }
    }
    if (tid == 64) png_package_merge_wide(h_d, len + PNG_NLL, s_pm, s_pm + 150);
    __syncthreads();
    for (int k = tid; k < nleaf; k += 256) {
        int at = k, depth = 0;
        while (at != root && depth < 16) { at = par[at]; ++depth; }
        if (at != root || depth > 15) atomicOr(&misc[0], 1u);
        len[l_sym[k]] = (unsigned char)depth;
    }
    __syncthreads();
    if (tid == 0) {
        int extra = 0;
        png_run_length(len, png_hlit(len), png_hdist<PNG_WND>(len), [&](int sym, int, int eb) { h_cl[sym] += 1u; extra += eb; });
        png_package_merge(h_cl, PNG_NCL, 7, len + PNG_NLL + PNG_WND, s_pm, s_pm + 100, s_pm + 200);
        int hb = 5 + 5 + 4 + 3 * png_hclen<PNG_WND>(len) + extra;
        for (int q = 0; q < PNG_NCL; ++q) hb += (int)h_cl[q] * len[PNG_NLL + PNG_WND + q];
        misc[1] = (unsigned)hb;
    }
    __syncthreads();
    int bits = xbits;
    for (int e = tid; e < PNG_NLL + PNG_WND; e += 256) bits += (int)s_img[e < PNG_NLL ? PNG_W_HLL + e : PNG_W_HD + e - PNG_NLL] * (int)len[e];
    bits = video_wave_sum(bits);
    if ((tid & 63) == 0) s_red[8 + (tid >> 6)] = (unsigned)bits;
    __syncthreads();
    hbits = (int)misc[1];
    ok = !misc[0];
    return 3 + hbits + (int)(s_red[8] + s_red[9] + s_red[10] + s_red[11]);
}

// a token of the window parse in the segment's own code (tab: png_canonical<PNG_WND> of the 335 entries), in two pieces: the literal or
// the length with its extra bits (<= 15 + 5), the distance with its extra bits (<= 15 + 13; none for a literal)
__device__ __forceinline__ void png_win_token(const unsigned *tab, unsigned t, unsigned byte, unsigned &v0, int &n0, unsigned &v1, int &n1) {
    v1 = 0u; n1 = 0;
    if (!t) { const unsigned e = tab[byte]; v0 = e & 0xFFFFu; n0 = (int)(e >> 16); return; }
    int sym, eb, dc, db;
    unsigned ev, dv;
    png_len_sym((int)(t & 511u), sym, eb, ev);
    png_dist_sym((int)((t >> 9) & 0xFFFFu), dc, db, dv);
    const unsigned e = tab[sym], f = tab[PNG_NLL + dc];
    n0 = (int)(e >> 16); v0 = (e & 0xFFFFu) | ev << n0; n0 += eb;
    n1 = (int)(f >> 16); v1 = (f & 0xFFFFu) | dv << n1; n1 += db;
}

// what a segment's chunk is made of once the layout is known
struct PngSeg { int n, pre, fixed, final, body; };   // raw bytes; 2 = the zlib header goes first; a bit image (fixed or dynamic code) / stored; last segment; payload bytes
__device__ __forceinline__ unsigned png_payload_byte(const PngSeg &s, const unsigned *img, const unsigned char *raw, int j) {
    if (s.fixed) return (img[j >> 2] >> (8 * (j & 3))) & 255u;
    if (j < s.pre) return j == 0 ? 0x78u : 0x01u;
    j -= s.pre;
    const unsigned n = (unsigned)s.n;
    if (j == 0) return (unsigned)s.final;   // BFINAL, BTYPE 00, the rest of the byte skipped
    if (j == 1) return n & 255u;
    if (j == 2) return n >> 8;
    if (j == 3) return ~n & 255u;
    if (j == 4) return (~n >> 8) & 255u;
    return raw[j - 5];
}

template <bool WRITE, bool DYN = false, bool WIN = false>   // (WIN goes with DYN: the window coding starts from the dynamic coding's choice)
__global__ void __launch_bounds__(256) k_png_segment(PngDev d) {
    static_assert(DYN || !WIN, "the window instantiations are the dynamic ones and more");
    constexpr int SIDE = WIN ? PNG_WSIDE : PNG_SIDE;   // bytes of a segment's side record
    __shared__ unsigned s_dyn[DYN && WRITE ? (WIN ? PNG_WLEN_WORDS + PNG_WNLEN + 1 : 80 + PNG_NLEN + 2) : 1];   // (dynamic write pass) the lengths [312 bytes], the codes [310]
    __shared__ unsigned s_pm[WIN && !WRITE ? PNG_W_PM : 1];    // (window count pass) the package-merge lists
    __shared__ unsigned s_raw[PNG_SEG / 4 + (WIN ? 4 : 0)];    // (window: a word to spare behind the bytes, png_word_at)
    __shared__ __attribute__((aligned(WIN ? 4 : 2))) unsigned short s_tok[WIN ? 2 * PNG_SEG : PNG_SEG];   // per position: match length | index of its distance << 9 (0: a literal)
    unsigned *s_tokw = (unsigned *)s_tok;              // (window) the window parse's tokens are 32 bits each
    __shared__ unsigned s_img[PNG_IMG_WORDS];
    __shared__ unsigned char s_mark[PNG_SEG + 4];      // 1: a token starts here ([n]: the chain's end, written and never read)
    __shared__ unsigned short s_lead[PNG_ND][256];     // per thread and distance: the leading run of its mask | 0x8000 when that is all of it
    __shared__ unsigned s_red[256];
    __shared__ int s_w[4];
    __shared__ int s_tokens[WIN ? 4 : 2];
    const int tid = threadIdx.x, seg = blockIdx.x;
    const int n = min(PNG_SEG, d.raw - seg * PNG_SEG);
    const unsigned char *src = d.flt + (size_t)seg * PNG_SEG;
    unsigned char *s_b = (unsigned char *)s_raw;
    unsigned short *s_next = (unsigned short *)s_img;
    const int base = tid * PNG_PER;

    for (int w = tid; w < PNG_SEG / 4; w += 256) {   // (the segment starts on a multiple of PNG_SEG in an allocation: aligned words)
        const int i = 4 * w;
        unsigned v = 0u;
        if (i + 3 < n) v = ((const unsigned *)src)[w];
        else for (int k = 0; k < 4; ++k) if (i + k < n) v |= (unsigned)src[i + k] << (8 * k);
        s_raw[w] = v;
    }
    for (int i = tid; i < PNG_SEG + 4; i += 256) s_mark[i] = i == 0 ? 1 : 0;
    if (tid < (WIN ? 4 : 2)) s_tokens[tid] = 0;
    if (WIN && tid < 4) s_raw[PNG_SEG / 4 + tid] = 0u;
    bool win = false;     // (window coding) the segment is one dynamic block of the window parse
    if (WIN && WRITE) win = ((const unsigned *)(d.side + (size_t)seg * SIDE))[PNG_SIDE / 4 + PNG_WLEN_WORDS] == 3u;   // (workgroup-uniform)
    __syncthreads();

    // the thread's bytes and the eight before them
    unsigned char c[8 + PNG_PER];
#pragma unroll
    for (int k = 0; k < 8 + PNG_PER; ++k) c[k] = base + k >= 8 ? s_b[base + k - 8] : (unsigned char)0;

    if (!WRITE) {   // Adler sums of the segment: a = sum of bytes, b = sum of (n - j) byte[j]; <= 4096 x 4097 / 2 x 255 < 2^32
        unsigned a = 0u, b = 0u;
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k)
            if (base + k < n) { a += c[8 + k]; b += (unsigned)(n - base - k) * c[8 + k]; }
        a = (unsigned)video_wave_sum((int)a); b = (unsigned)video_wave_sum((int)b);
        if ((tid & 63) == 0) { s_red[tid >> 6] = a; s_red[4 + (tid >> 6)] = b; }
        __syncthreads();
        if (tid == 0) {
            d.adler[2 * seg] = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) % 65521u;
            d.adler[2 * seg + 1] = (s_red[4] + s_red[5] + s_red[6] + s_red[7]) % 65521u;
        }
    }

    // byte equalities per distance
    unsigned m[PNG_ND];
#pragma unroll
    for (int q = 0; q < PNG_ND; ++q) {
        const int dist = PNG_DIST[q];
        unsigned mk = 0u;
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k)
            if (base + k >= dist && base + k < n && c[8 + k] == c[8 + k - dist]) mk |= 1u << k;   // (nothing before the segment is seen)
        m[q] = mk;
        s_lead[q][tid] = mk == 0xFFFFu ? (unsigned short)(0x8000u | PNG_PER) : (unsigned short)__builtin_ctz(~mk);
    }
    __syncthreads();
    int carry[PNG_ND];   // the run that enters the next thread's positions (as far as the longest match needs it)
#pragma unroll
    for (int q = 0; q < PNG_ND; ++q) {
        int r = 0;
        for (int u = tid + 1; u < 256 && r < 258; ++u) {
            const unsigned v = s_lead[q][u];
            r += (int)(v & 0x7FFFu);
            if (!(v & 0x8000u)) break;
        }
        carry[q] = r;
    }
    // longest first, then the smallest distance (PNG_DIST ascends: a later one must be strictly longer)
    if (WIN && win) png_window_tokens(d, seg, n, tid, s_raw, s_lead, s_tokw, s_next);
    else
#pragma unroll
    for (int k = 0; k < PNG_PER; ++k) {
        int best = 0, bq = 0;
#pragma unroll
        for (int q = 0; q < PNG_ND; ++q) {
            int run = __builtin_ctz(~(m[q] >> k));   // (bits 16 - k and up of the shifted mask are 0: run <= 16 - k)
            if (run == PNG_PER - k) run += carry[q];
            run = min(run, 258);
            if (run > best) { best = run; bq = q; }
        }
        if (best < 3) { best = 0; bq = 0; }
        const int i = base + k;
        s_tok[i] = (unsigned short)(best | (bq << 9));
        s_next[i] = (unsigned short)(i < n ? i + max(best, 1) : n);   // (a run ends before byte n: i + best <= n)
    }
    if (tid == 0) s_next[PNG_SEG] = (unsigned short)n;   // (n == PNG_SEG: the end of the chain points at itself)
    __syncthreads();

    // the greedy parse from position 0 by pointer doubling; position i of round k: tid + 256 k
    for (int r = 0; r < 12; ++r) {   // 2^12 = PNG_SEG hops at the most
        if (s_next[0] >= n) break;   // (workgroup-uniform: read behind a barrier, written only behind the next one)
        unsigned short j[PNG_PER], jj[PNG_PER];
        unsigned char mk[PNG_PER];
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k) {
            const int i = tid + 256 * k;
            j[k] = s_next[i];
            jj[k] = s_next[j[k]];
            mk[k] = s_mark[i];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k) {
            const int i = tid + 256 * k;
            if (mk[k]) s_mark[j[k]] = 1;   // (one predecessor per position on the chain: no two lanes write one byte)
            s_next[i] = jj[k];
        }
        __syncthreads();
    }
    __syncthreads();

    // bits per token
    int bits = 0, nlit = 0, nmat = 0;
    if (!(WIN && win))
#pragma unroll
    for (int k = 0; k < PNG_PER; ++k) {
        const int i = base + k;
        if (i < n && s_mark[i]) {
            const unsigned t = s_tok[i];
            unsigned val; int nb;
            if (t) { png_match((int)(t & 511u), PNG_DIST[t >> 9], val, nb); ++nmat; }
            else { png_literal(c[8 + k], val, nb); ++nlit; }
            bits += nb;
        }
    }
    int tot;
    const int before = block_excl_scan_256(bits, s_w, tot);   // (its barriers also end every use of s_next)
    PngSeg s;
    s.n = n;
    s.pre = seg == 0 ? 2 : 0;
    s.final = seg == d.nseg - 1 ? 1 : 0;
    const int fixed_bits = 3 + tot + 7;   // block header, tokens, end of block
    // not the last segment: an empty stored block (000, padding to a byte, 00 00 FF FF) brings the next segment to a byte boundary
    const int fixed_bytes = s.final ? (fixed_bits + 7) >> 3 : ((fixed_bits + 3 + 7) >> 3) + 4;
    s.fixed = fixed_bytes <= 5 + n ? 1 : 0;   // ties go to the fixed code
    s.body = s.pre + (s.fixed ? fixed_bytes : 5 + n);
    bool dyn = false;     // the segment is a dynamic block (strictly shorter than the choice above)
    int hbits = 0;        // its header's bits

    if (DYN && !WRITE) {
        // histograms of the tokens by the marked positions; the three codes' lengths; the header's bits
        unsigned *h_ll = s_img + PNG_C_HLL, *h_d = s_img + PNG_C_HD, *h_cl = s_img + PNG_C_HCL, *l_sym = s_img + PNG_C_SYM, *wt = s_img + PNG_C_WT;
        unsigned short *par = (unsigned short *)(s_img + PNG_C_PAR);
        unsigned char *len = (unsigned char *)(s_img + PNG_C_LEN);
        unsigned *misc = s_img + PNG_C_MISC;
        for (int w = tid; w < PNG_C_SYM; w += 256) s_img[w] = 0u;
        if (tid < 78) s_img[PNG_C_LEN + tid] = 0u;
        if (tid < 8) misc[tid] = 0u;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k) {
            const int i = base + k;
            if (i < n && s_mark[i]) {
                const unsigned t = s_tok[i];
                if (t) {
                    int sym, eb;
                    unsigned ev;
                    png_len_sym((int)(t & 511u), sym, eb, ev);
                    atomicAdd(&h_ll[sym], 1u);
                    atomicAdd(&h_d[t >> 9], 1u);
                } else atomicAdd(&h_ll[c[8 + k]], 1u);
            }
        }
        if (tid == 0) atomicAdd(&h_ll[256], 1u);   // the end of block
        __syncthreads();
        // the used lit/len symbols sorted by (count, symbol): every symbol counts the keys below its own
        int nleaf = 0;
        {
            const int s0 = tid, s1 = tid + 256;
            const unsigned c0 = h_ll[s0], c1 = s1 < PNG_NLL ? h_ll[s1] : 0u;
            const unsigned k0 = c0 << 9 | (unsigned)s0, k1 = c1 << 9 | (unsigned)s1;
            int r0 = 0, r1 = 0;
            for (int j = 0; j < PNG_NLL; ++j) {
                const unsigned cj = h_ll[j], kj = cj << 9 | (unsigned)j;
                if (cj) { ++nleaf; r0 += kj < k0; r1 += kj < k1; }
            }
            if (c0) { l_sym[r0] = (unsigned)s0; wt[r0] = c0; }
            if (c1) { l_sym[r1] = (unsigned)s1; wt[r1] = c1; }
        }
        __syncthreads();
        const int root = 2 * nleaf - 2;   // (nleaf >= 2: the segment's first byte is a literal, and the end of block)
        if (tid == 0) {
            // Huffman by two queues: the leaves in order and the internal nodes in the order they are made; a node joins the two
            // lightest heads, a leaf before an internal node of equal weight
            int leaf = 0, inner = nleaf;
            for (int node = nleaf; node <= root; ++node) {
                unsigned sum = 0u;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    int pick;
                    if (leaf < nleaf && (inner >= node || wt[leaf] <= wt[inner])) pick = leaf++;
                    else pick = inner++;
                    sum += wt[pick];
                    par[pick] = (unsigned short)node;
                }
                wt[node] = sum;
            }
        }
        if (tid == 64) png_package_merge(h_d, PNG_NDC, 4, len + PNG_NLL, s_img + PNG_C_PMW, s_img + PNG_C_PML, s_img + PNG_C_PMH);
        __syncthreads();
        for (int k = tid; k < nleaf; k += 256) {   // depths: every leaf walks its parents
            int at = k, depth = 0;
            while (at != root && depth < 16) { at = par[at]; ++depth; }
            if (at != root || depth > 15) atomicOr(&misc[0], 1u);   // deeper than 15: the segment is not offered a dynamic block
            len[l_sym[k]] = (unsigned char)depth;
        }
        __syncthreads();
        if (tid == 0) {
            int extra = 0;
            png_run_length(len, png_hlit(len), png_hdist(len), [&](int sym, int, int eb) { h_cl[sym] += 1u; extra += eb; });
            png_package_merge(h_cl, PNG_NCL, 7, len + PNG_NLL + PNG_NDC, s_img + PNG_C_PMW, s_img + PNG_C_PML, s_img + PNG_C_PMH);
            int hb = 5 + 5 + 4 + 3 * png_hclen(len) + extra;
            for (int q = 0; q < PNG_NCL; ++q) hb += (int)h_cl[q] * len[PNG_NLL + PNG_NDC + q];
            misc[1] = (unsigned)hb;
        }
        __syncthreads();
        // the block's bits: the fixed block's with every code's length exchanged, and the header
        int delta = 0;
        for (int e = tid; e < PNG_NLL + PNG_NDC; e += 256)
            delta += e < PNG_NLL ? (int)h_ll[e] * ((int)len[e] - png_fixed_len(e)) : (int)h_d[e - PNG_NLL] * ((int)len[e] - 5);
        delta = video_wave_sum(delta);
        if ((tid & 63) == 0) s_red[8 + (tid >> 6)] = (unsigned)delta;
        __syncthreads();
        hbits = (int)misc[1];
        const int dyn_bits = fixed_bits + hbits + (int)(s_red[8] + s_red[9] + s_red[10] + s_red[11]);
        const int dyn_bytes = s.final ? (dyn_bits + 7) >> 3 : ((dyn_bits + 3 + 7) >> 3) + 4;
        dyn = !misc[0] && s.pre + dyn_bytes < s.body;
        if (dyn) s.body = s.pre + dyn_bytes;
        unsigned *side = (unsigned *)(d.side + (size_t)seg * SIDE);
        if (tid < 78) side[tid] = s_img[PNG_C_LEN + tid];
        if (tid == 78) side[78] = dyn ? 2u : (unsigned)s.fixed;
        if (tid == 79) side[79] = (unsigned)hbits;
    }

    int whbits = 0;       // the window block's header bits
    if (WIN && !WRITE) {
        // the window parse over the same arrays (the five-distance parse is done with them), its block against the choice above
        __syncthreads();
        for (int i = tid; i < PNG_SEG + 4; i += 256) s_mark[i] = i == 0 ? 1 : 0;
        png_window_tokens(d, seg, n, tid, s_raw, s_lead, s_tokw, s_next);
        if (tid == 0) s_next[PNG_SEG] = (unsigned short)n;
        __syncthreads();
        png_chain(s_next, s_mark, n, tid);
        bool ok;
        const int wbits = png_window_codes(s_img, s_pm, s_red, s_tokw, s_mark, s_b, n, tid, whbits, ok);
        const int wbytes = s.final ? (wbits + 7) >> 3 : ((wbits + 3 + 7) >> 3) + 4;
        win = ok && s.pre + wbytes < s.body;   // strictly shorter, or the choice above stands
        unsigned *side = (unsigned *)(d.side + (size_t)seg * SIDE) + PNG_SIDE / 4;
        if (tid < PNG_WLEN_WORDS) side[tid] = s_img[PNG_W_LEN + tid];
        if (tid == PNG_WLEN_WORDS) side[PNG_WLEN_WORDS] = win ? 3u : 0u;
        if (tid == PNG_WLEN_WORDS + 1) side[PNG_WLEN_WORDS + 1] = (unsigned)whbits;
        if (win) {   // (workgroup-uniform) the counters are those of the parse written
            s.body = s.pre + wbytes;
            s.fixed = 1; dyn = false;
            nlit = 0; nmat = 0;
            int nwin = 0, nfar = 0;
            for (int k = 0; k < PNG_PER; ++k) {
                const int i = base + k;
                if (i < n && s_mark[i]) {
                    const unsigned t = s_tokw[i];
                    if (t) { ++nmat; nwin += (int)(t >> 25); nfar += ((t >> 9) & 0xFFFFu) > PNG_FAR; }
                    else ++nlit;
                }
            }
            if (nwin) atomicAdd(&s_tokens[2], nwin);
            if (nfar) atomicAdd(&s_tokens[3], nfar);
        }
    }

    if (!WRITE) {
        if (s.fixed || dyn) {
            if (nlit) atomicAdd(&s_tokens[0], nlit);
            if (nmat) atomicAdd(&s_tokens[1], nmat);
        }
        __syncthreads();
        if (tid == 0) {
            d.len[seg] = 12 + s.body;
            if (!s.fixed && !dyn) atomicAdd(&d.cnt[5], 1ull);
            if (s_tokens[0]) atomicAdd(&d.cnt[6], (unsigned long long)s_tokens[0]);
            if (s_tokens[1]) atomicAdd(&d.cnt[7], (unsigned long long)s_tokens[1]);
            if (DYN && dyn) { atomicAdd(&d.cnt[8], 1ull); atomicAdd(&d.cnt[9], (unsigned long long)hbits); }
            if (WIN && win) {
                atomicAdd(&d.cnt[10], 1ull); atomicAdd(&d.cnt[13], (unsigned long long)whbits);
                if (s_tokens[2]) atomicAdd(&d.cnt[11], (unsigned long long)s_tokens[2]);
                if (s_tokens[3]) atomicAdd(&d.cnt[12], (unsigned long long)s_tokens[3]);
            }
        }
        return;
    }

    if (WIN && WRITE && win) {   // the window block, as the dynamic block below with PNG_WND distance symbols and tokens in two pieces
        const unsigned *side = (const unsigned *)(d.side + (size_t)seg * SIDE) + PNG_SIDE / 4;
        whbits = (int)side[PNG_WLEN_WORDS + 1];
        unsigned char *len = (unsigned char *)s_dyn;
        unsigned *tab = s_dyn + PNG_WLEN_WORDS;
        if (tid < PNG_WLEN_WORDS) s_dyn[tid] = side[tid];
        __syncthreads();
        for (int e = tid; e < PNG_WNLEN; e += 256) tab[e] = png_canonical<PNG_WND>(len, e);
        __syncthreads();
        int dbits = 0;
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k) {
            const int i = base + k;
            if (i < n && s_mark[i]) {
                unsigned v0, v1; int n0, n1;
                png_win_token(tab, s_tokw[i], c[8 + k], v0, n0, v1, n1);
                dbits += n0 + n1;
            }
        }
        int dtot;
        const int dbefore = block_excl_scan_256(dbits, s_w, dtot);
        const unsigned eob = tab[256];
        s.fixed = 1; dyn = true;   // (a bit image, built here)
        s.body = min(d.len[seg + 1] - d.len[seg] - 12, s.pre + 5 + n);   // the payload the count pass allotted
        const int words = ((s.body + 3) >> 2) + 2;
        for (int w = tid; w < words; w += 256) s_img[w] = 0u;
        __syncthreads();
        const int top = 32 * words;   // (bits past the image are never written, whatever the side record says)
        auto put = [&](int o, unsigned val, int nb) {
            const int w = o >> 5, sh = o & 31;
            if (o + nb > top) return;
            atomicOr(&s_img[w], val << sh);
            if (sh + nb > 32) atomicOr(&s_img[w + 1], val >> (32 - sh));
        };
        int o = 8 * s.pre + 3 + whbits + dbefore;
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k) {
            const int i = base + k;
            if (i < n && s_mark[i]) {
                unsigned v0, v1; int n0, n1;
                png_win_token(tab, s_tokw[i], c[8 + k], v0, n0, v1, n1);
                put(o, v0, n0);
                if (n1) put(o + n0, v1, n1);
                o += n0 + n1;
            }
        }
        if (tid == 0) {
            if (s.pre) atomicOr(&s_img[0], 0x0178u);
            atomicOr(&s_img[s.pre >> 2], (unsigned)(s.final | 4) << (8 * s.pre));   // BFINAL, BTYPE 10 (its low bit first)
            put(8 * s.pre + 3 + whbits + dtot, eob & 0xFFFFu, (int)(eob >> 16));
            if (!s.final) {
                const int e = s.body - 2;
                atomicOr(&s_img[e >> 2], 0xFFu << (8 * (e & 3)));
                atomicOr(&s_img[(e + 1) >> 2], 0xFFu << (8 * ((e + 1) & 3)));
            }
        }
        if (tid == 64) {   // the header: HLIT, HDIST, HCLEN, the code-length code's lengths, the coded lengths
            const int hlit = png_hlit(len), hdist = png_hdist<PNG_WND>(len), hclen = png_hclen<PNG_WND>(len);
            int ho = 8 * s.pre + 3;
            put(ho, (unsigned)(hlit - 257) | (unsigned)(hdist - 1) << 5 | (unsigned)(hclen - 4) << 10, 14);
            ho += 14;
            for (int q = 0; q < hclen; ++q) { put(ho, len[PNG_NLL + PNG_WND + PNG_CL_ORDER[q]], 3); ho += 3; }
            png_run_length(len, hlit, hdist, [&](int sym, int ev, int eb) {
                const unsigned e = tab[PNG_NLL + PNG_WND + sym];
                const int nb = (int)(e >> 16);
                put(ho, (e & 0xFFFFu) | (unsigned)ev << nb, nb + eb);
                ho += nb + eb;
            });
        }
        __syncthreads();
    }

    if (DYN && WRITE && !(WIN && win)) {
        const unsigned *side = (const unsigned *)(d.side + (size_t)seg * SIDE);
        dyn = side[78] == 2u;   // (workgroup-uniform)
        if (dyn) {
            hbits = (int)side[79];
            unsigned char *len = (unsigned char *)s_dyn;
            unsigned *tab = s_dyn + 80;
            if (tid < 78) s_dyn[tid] = side[tid];
            __syncthreads();
            for (int e = tid; e < PNG_NLEN; e += 256) tab[e] = png_canonical(len, e);
            __syncthreads();
            int dbits = 0;
#pragma unroll
            for (int k = 0; k < PNG_PER; ++k) {
                const int i = base + k;
                if (i < n && s_mark[i]) {
                    unsigned val; int nb;
                    png_dyn_token(tab, s_tok[i], c[8 + k], val, nb);
                    dbits += nb;
                }
            }
            int dtot;
            const int dbefore = block_excl_scan_256(dbits, s_w, dtot);
            const unsigned eob = tab[256];
            s.fixed = 1;   // (a bit image)
            // the payload the count pass allotted: 3 + header + tokens + end of block, closed as a fixed block is; shorter than stored
            s.body = min(d.len[seg + 1] - d.len[seg] - 12, s.pre + 5 + n);
            const int words = ((s.body + 3) >> 2) + 2;
            for (int w = tid; w < words; w += 256) s_img[w] = 0u;
            __syncthreads();
            const int top = 32 * words;   // (bits past the image are never written, whatever the side record says)
            auto put = [&](int o, unsigned val, int nb) {
                const int w = o >> 5, sh = o & 31;
                if (o + nb > top) return;
                atomicOr(&s_img[w], val << sh);
                if (sh + nb > 32) atomicOr(&s_img[w + 1], val >> (32 - sh));
            };
            int o = 8 * s.pre + 3 + hbits + dbefore;
#pragma unroll
            for (int k = 0; k < PNG_PER; ++k) {
                const int i = base + k;
                if (i < n && s_mark[i]) {
                    unsigned val; int nb;
                    png_dyn_token(tab, s_tok[i], c[8 + k], val, nb);
                    put(o, val, nb);
                    o += nb;
                }
            }
            if (tid == 0) {
                if (s.pre) atomicOr(&s_img[0], 0x0178u);
                atomicOr(&s_img[s.pre >> 2], (unsigned)(s.final | 4) << (8 * s.pre));   // BFINAL, BTYPE 10 (its low bit first)
                put(8 * s.pre + 3 + hbits + dtot, eob & 0xFFFFu, (int)(eob >> 16));
                if (!s.final) {
                    const int e = s.body - 2;
                    atomicOr(&s_img[e >> 2], 0xFFu << (8 * (e & 3)));
                    atomicOr(&s_img[(e + 1) >> 2], 0xFFu << (8 * ((e + 1) & 3)));
                }
            }
            if (tid == 64) {   // the header: HLIT, HDIST, HCLEN, the code-length code's lengths, the coded lengths
                const int hlit = png_hlit(len), hdist = png_hdist(len), hclen = png_hclen(len);
                int ho = 8 * s.pre + 3;
                put(ho, (unsigned)(hlit - 257) | (unsigned)(hdist - 1) << 5 | (unsigned)(hclen - 4) << 10, 14);
                ho += 14;
                for (int q = 0; q < hclen; ++q) { put(ho, len[PNG_NLL + PNG_NDC + PNG_CL_ORDER[q]], 3); ho += 3; }
                png_run_length(len, hlit, hdist, [&](int sym, int ev, int eb) {
                    const unsigned e = tab[PNG_NLL + PNG_NDC + sym];
                    const int nb = (int)(e >> 16);
                    put(ho, (e & 0xFFFFu) | (unsigned)ev << nb, nb + eb);
                    ho += nb + eb;
                });
            }
            __syncthreads();
        }
    }

    if (s.fixed && !dyn) {   // (workgroup-uniform)
        const int words = ((s.body + 3) >> 2) + 2;   // + the word a token's bits can spill into, + padding
        for (int w = tid; w < words; w += 256) s_img[w] = 0u;
        __syncthreads();
        int o = 8 * s.pre + 3 + before;
#pragma unroll
        for (int k = 0; k < PNG_PER; ++k) {
            const int i = base + k;
            if (i < n && s_mark[i]) {
                const unsigned t = s_tok[i];
                unsigned val; int nb;
                if (t) png_match((int)(t & 511u), PNG_DIST[t >> 9], val, nb);
                else png_literal(c[8 + k], val, nb);
                const int w = o >> 5, sh = o & 31;
                atomicOr(&s_img[w], val << sh);
                if (sh + nb > 32) atomicOr(&s_img[w + 1], val >> (32 - sh));   // (then sh > 0)
                o += nb;
            }
        }
        if (tid == 0) {
            if (s.pre) atomicOr(&s_img[0], 0x0178u);                          // CMF 78, FLG 01
            atomicOr(&s_img[s.pre >> 2], (unsigned)(s.final | 2) << (8 * s.pre));   // BFINAL, BTYPE 01 (its low bit first)
            if (!s.final) {                                                   // LEN 0000 stays zero, NLEN FFFF
                const int e = s.body - 2;
                atomicOr(&s_img[e >> 2], 0xFFu << (8 * (e & 3)));
                atomicOr(&s_img[(e + 1) >> 2], 0xFFu << (8 * ((e + 1) & 3)));
            }
        }
        __syncthreads();
    }

    // the chunk: length, tag, payload at the scanned offset
    unsigned char *out = d.out + (size_t)d.len[seg];
    const unsigned tag = 0x54414449u;   // "IDAT", first letter in the low byte
    for (int q = tid; q < 8 + s.body; q += 256) {
        unsigned v;
        if (q < 4) v = ((unsigned)s.body >> (8 * (3 - q))) & 255u;
        else if (q < 8) v = (tag >> (8 * (q - 4))) & 255u;
        else v = png_payload_byte(s, s_img, s_b, q - 8);
        out[q] = (unsigned char)v;
    }
    // CRC-32 of tag + payload.  The register starts at all ones: the same as a zero register and the first four bytes complemented.
    const int total = 4 + s.body, pad = 256 * PNG_CRC_PIECE - total;
    unsigned r = 0u;
    for (int k = 0; k < PNG_CRC_PIECE; ++k) {
        const int v = tid * PNG_CRC_PIECE + k - pad;
        if (v >= 0) r = png_crc_byte(r, v < 4 ? ((tag >> (8 * v)) & 255u) ^ 255u : png_payload_byte(s, s_img, s_b, v - 4));
    }
    s_red[tid] = r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        __syncthreads();
        if ((tid & ((2 << j) - 1)) == 0) s_red[tid] = png_crc_mul(s_red[tid], d.crc_pow[j]) ^ s_red[tid + (1 << j)];
    }
    if (tid == 0) {
        const unsigned crc = ~s_red[0];
        unsigned char *e = out + 8 + s.body;
        e[0] = (unsigned char)(crc >> 24); e[1] = (unsigned char)(crc >> 16); e[2] = (unsigned char)(crc >> 8); e[3] = (unsigned char)crc;
    }
    if (seg == 0 && tid == 64) {   // the Adler-32 closes the zlib stream in a chunk of its own (behind the last segment's)
        unsigned char *a = d.out + (size_t)d.len[d.nseg];
        const unsigned sum = d.sum[0];
        unsigned cr = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < 12; ++k) {   // length 4, tag, the sum with its high byte first
            const unsigned v = k < 4 ? (k == 3 ? 4u : 0u) : k < 8 ? (tag >> (8 * (k - 4))) & 255u : (sum >> (8 * (11 - k))) & 255u;
            a[k] = (unsigned char)v;
            if (k >= 4) cr = png_crc_byte(cr, v);
        }
        cr = ~cr;
        a[12] = (unsigned char)(cr >> 24); a[13] = (unsigned char)(cr >> 16); a[14] = (unsigned char)(cr >> 8); a[15] = (unsigned char)cr;
    }
}

// exclusive scan of len[0, nseg) in place, len[nseg] = the total (one workgroup walks the array, as k_video_scan does: 769 segments at
// 1024^2, 49,164 at the 2^26 pixels sph_png_create accepts), and the Adler-32 of the whole stream from the segments' sums:
//   A = 1 + sum a_k,  B = raw + sum (b_k + a_k x bytes behind segment k),  both mod 65521
// The offsets are int: the largest file is below 2^26 x 3 + 2^14 + 17 x 49,164 + 75 < 2^31.
__global__ void __launch_bounds__(256) k_png_scan(PngDev d) {
    __shared__ int s_w[4];
    __shared__ unsigned long long s_a[256], s_b[256];
    const int tid = threadIdx.x, n = d.nseg;
    int run = 0;
    unsigned long long a = 0ull, b = 0ull;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        const int v = i < n ? d.len[i] : 0;
        int tot;
        const int ex = block_excl_scan_256(v, s_w, tot);
        if (i < n) {
            d.len[i] = run + ex;
            const long long end = min((long long)(i + 1) * PNG_SEG, (long long)d.raw);
            const unsigned long long ak = d.adler[2 * i], bk = d.adler[2 * i + 1];
            a += ak;                                                        // < 2^16 each, <= 49,164 segments
            b += bk + ak * (unsigned long long)((d.raw - end) % 65521);     // < 2^33 each
        }
        run += tot;
    }
    s_a[tid] = a; s_b[tid] = b;
    __syncthreads();
    if (tid == 0) {
        d.len[n] = run;
        unsigned long long sa = 1ull, sb = (unsigned long long)d.raw;
        for (int k = 0; k < 256; ++k) { sa += s_a[k]; sb += s_b[k]; }
        d.sum[0] = (unsigned)(sb % 65521ull) << 16 | (unsigned)(sa % 65521ull);
    }
}

// --- the candidates of the whole stream (coding = window) ---
// A stable LSD radix sort of the positions [0, raw - 2) by their three bytes, one byte a pass, leaves equal keys in stream order: a
// position's predecessor in the sorted order is the most recent earlier position with its key, and k_png_prev keeps it when it lies
// within PNG_WINDOW.  A pass is three kernels: k_png_sort_hist counts the digits of every workgroup's tile of PNG_SORT_TILE items,
// k_png_sort_scan (one workgroup per digit) scans each digit's counts over the workgroups and leaves its total, k_png_sort_scatter ranks
// its tile again and moves (key, position) to the other side.  Item g of a tile belongs to wave g / 1024, round (g / 64) % 16, lane
// g % 64: a wave walks its 1024 items in order, 64 at a time.  The rank of an item among the wave's earlier items of its digit is the
// wave's running count (LDS, one row per wave: nobody else touches it) plus the lanes below it with the same digit, found from eight
// ballots -- no atomic, so nothing serialises on a flat picture (every key equal).
#define PNG_SORT_ROUNDS (PNG_SORT_TILE / 256)
static_assert(PNG_SORT_TILE == 4 * 64 * PNG_SORT_ROUNDS, "four waves, whole rounds");

template <int PASS>
__device__ __forceinline__ void png_sort_item(const PngDev &d, int g, int m, unsigned &key, unsigned &pos) {
    key = 0u; pos = 0u;
    if (g >= m) return;
    if (PASS == 0) { key = (unsigned)d.flt[g] | (unsigned)d.flt[g + 1] << 8 | (unsigned)d.flt[g + 2] << 16; pos = (unsigned)g; }   // (g + 2 < raw)
    else { key = d.sort_key[(PASS - 1) & 1][g]; pos = d.sort_pos[(PASS - 1) & 1][g]; }
}
// one round of a wave: the item's rank among the wave's items so far with its digit; cnt: the wave's counts [256]
__device__ __forceinline__ int png_sort_rank(unsigned digit, bool valid, int *cnt, int lane) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long on = __ballot(bit);
        peers &= bit ? on : ~on;
    }
    int rank = 0;
    if (valid) {
        const int had = cnt[digit];
        rank = had + __popcll(peers & ((1ull << lane) - 1ull));
        if (((peers >> lane) >> 1) == 0ull) cnt[digit] = had + __popcll(peers);   // the highest lane of the digit writes: one lane per address
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the next round reads what this one wrote, in other lanes of this wave
    __builtin_amdgcn_wave_barrier();
    return rank;
}

template <int PASS, bool SCATTER>
__global__ void __launch_bounds__(256) k_png_sort(PngDev d) {
    __shared__ int s_cnt[4][256];
    __shared__ int s_base[256];
    __shared__ int s_w[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wg = blockIdx.x;
    const int m = d.raw - 2;
    const int first = wg * PNG_SORT_TILE + wave * (PNG_SORT_TILE / 4) + lane;
#pragma unroll
    for (int w = 0; w < 4; ++w) s_cnt[w][tid] = 0;
    __syncthreads();
    unsigned key[PNG_SORT_ROUNDS], pos[PNG_SORT_ROUNDS];
    int rank[PNG_SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < PNG_SORT_ROUNDS; ++r) png_sort_item<PASS>(d, first + 64 * r, m, key[r], pos[r]);
#pragma unroll
    for (int r = 0; r < PNG_SORT_ROUNDS; ++r) rank[r] = png_sort_rank((key[r] >> (8 * PASS)) & 255u, first + 64 * r < m, s_cnt[wave], lane);
    __syncthreads();
    const int c0 = s_cnt[0][tid], c1 = s_cnt[1][tid], c2 = s_cnt[2][tid], c3 = s_cnt[3][tid];   // digit tid in the four waves
    if (!SCATTER) { d.hist[(size_t)tid * d.nsort + wg] = c0 + c1 + c2 + c3; return; }
    int total;
    const int below = block_excl_scan_256(d.hist[(size_t)256 * d.nsort + tid], s_w, total);   // the items of the smaller digits
    s_base[tid] = below + d.hist[(size_t)tid * d.nsort + wg];                                 // + this digit's in the earlier workgroups
    s_cnt[0][tid] = 0; s_cnt[1][tid] = c0; s_cnt[2][tid] = c0 + c1; s_cnt[3][tid] = c0 + c1 + c2;   // + in this workgroup's earlier waves
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PNG_SORT_ROUNDS; ++r) {
        if (first + 64 * r >= m) continue;
        const unsigned digit = (key[r] >> (8 * PASS)) & 255u;
        const int to = s_base[digit] + s_cnt[wave][digit] + rank[r];   // the ranks are a permutation of [0, m)
        if ((unsigned)to >= (unsigned)m) continue;                     // (never: no store leaves the arrays whatever the counts say)
        d.sort_key[PASS & 1][to] = key[r];
        d.sort_pos[PASS & 1][to] = pos[r];
    }
}

// one workgroup per digit: its counts over the sort's workgroups -> their exclusive scan in place, the total behind the table
__global__ void __launch_bounds__(256) k_png_sort_scan(PngDev d) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, n = d.nsort;
    int *row = d.hist + (size_t)blockIdx.x * n;
    int run = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        int tot;
        const int ex = block_excl_scan_256(i < n ? row[i] : 0, s_w, tot);
        if (i < n) row[i] = run + ex;
        run += tot;
    }
    if (tid == 0) d.hist[(size_t)256 * n + blockIdx.x] = run;
}

// prev of every position: the sorted predecessor where it has the same key and lies within the window (the sort is stable: it is the
// most recent one); the stream's last two positions have no key
__global__ void __launch_bounds__(256) k_png_prev(PngDev d) {
    const int k = blockIdx.x * 256 + threadIdx.x, m = max(d.raw - 2, 0);
    if (k < d.raw - m) d.prev[m + k] = PNG_NONE;
    if (k >= m) return;
    const unsigned i = d.sort_pos[0][k];   // (three passes: the sorted order ends on side 0)
    unsigned p = PNG_NONE;
    if (k > 0 && d.sort_key[0][k - 1] == d.sort_key[0][k]) {
        const unsigned j = d.sort_pos[0][k - 1];
        if (i - j <= PNG_WINDOW) p = j;
    }
    if (i < (unsigned)m) d.prev[i] = p;   // (always)
}

template <int PASS>
static void l_png_sort_pass(PngDev &d) {
    hipLaunchKernelGGL((k_png_sort<PASS, false>), dim3(d.nsort), dim3(256), 0, d.stream, d);
    hipLaunchKernelGGL(k_png_sort_scan, dim3(256), dim3(256), 0, d.stream, d);
    hipLaunchKernelGGL((k_png_sort<PASS, true>), dim3(d.nsort), dim3(256), 0, d.stream, d);
}
static void l_png_candidates(PngDev &d) {
    if (d.nsort > 0) { l_png_sort_pass<0>(d); l_png_sort_pass<1>(d); l_png_sort_pass<2>(d); }
    hipLaunchKernelGGL(k_png_prev, dim3((max(d.raw - 2, 2) + 255) / 256), dim3(256), 0, d.stream, d);
}

static void l_png_filter(PngDev &d) { hipLaunchKernelGGL(k_png_filter, dim3(d.H), dim3(256), 0, d.stream, d); }
static void l_png_count(PngDev &d) {
    if (d.prev) hipLaunchKernelGGL((k_png_segment<false, true, true>), dim3(d.nseg), dim3(256), 0, d.stream, d);
    else if (d.side) hipLaunchKernelGGL((k_png_segment<false, true>), dim3(d.nseg), dim3(256), 0, d.stream, d);
    else hipLaunchKernelGGL((k_png_segment<false>), dim3(d.nseg), dim3(256), 0, d.stream, d);
}
static void l_png_scan(PngDev &d) { hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(256), 0, d.stream, d); }
static void l_png_write(PngDev &d) {
    if (d.prev) hipLaunchKernelGGL((k_png_segment<true, true, true>), dim3(d.nseg), dim3(256), 0, d.stream, d);
    else if (d.side) hipLaunchKernelGGL((k_png_segment<true, true>), dim3(d.nseg), dim3(256), 0, d.stream, d);
    else hipLaunchKernelGGL((k_png_segment<true>), dim3(d.nseg), dim3(256), 0, d.stream, d);
}

static void register_png_launchers(Launch &L) {
    L.png_filter = l_png_filter;
    L.png_candidates = l_png_candidates;
    L.png_count = l_png_count;
    L.png_scan = l_png_scan;
    L.png_write = l_png_write;
}
