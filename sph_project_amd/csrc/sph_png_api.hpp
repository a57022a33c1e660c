// sph_png_api.hpp -- the SphPng object of include/sph_hip.h: the size bound, the fixed chunks (signature, IHDR, IEND), the frame source
// (sph_encoder_api.hpp), the four passes and the stage marks.  Host code, included at the end of sph_api.hip; the kernels are in
// sph_png.hpp, the stream is defined in DESIGN.md 21.
#pragma once

enum PngBufId { PB_FLT, PB_LEN, PB_ADLER, PB_CNT, PB_SIDE, PB_WSIDE, PB_PREV, PB_KEY0, PB_KEY1, PB_POS0, PB_POS1, PB_HIST, PB_COUNT_ };   // from PB_WSIDE on: coding = window

struct SphPng : FrameEncoder {   // header: signature, IHDR; payload: the segments' chunks and the Adler-32's; trailer: IEND
    SphPngParams prm;
    PngDev d{};
    DevBuf buf[PB_COUNT_];
    SphPngStats stats{};           // of the frame held
    SphPngWindowStats wstats{};
    bool have_candidates = false;  // the frame held was encoded in coding = window: prev[] is its candidates
    int32_t coding = SPH_PNG_CODING_FIXED;
};

static const char *png_check(const SphPngParams &p) {
    if (const char *why = enc_check_size(p.width, p.height)) return why;
    if (p.filter < -1 || p.filter > 4) return "filter is -1 (adaptive) or a PNG filter type 0..4";
    if (p.reserved != 0) return "reserved must be 0";
    return nullptr;
}

static int64_t png_raw_bytes(const SphPngParams &p) { return (int64_t)p.height * (1 + 3 * (int64_t)p.width); }
static int64_t png_segments(const SphPngParams &p) { return (png_raw_bytes(p) + PNG_SEG - 1) / PNG_SEG; }
// signature 8, IHDR 25, per segment a chunk frame of 12 and at worst a stored block header of 5 around its raw bytes, the zlib header 2,
// the Adler-32's chunk 16, IEND 12.  The same in either coding: a dynamic block is written only where it is strictly shorter than the
// fixed / stored choice, and a window block only where it is strictly shorter than that, so no segment grows.
static int64_t png_bound(const SphPngParams &p) { return 8 + 25 + png_segments(p) * (12 + 5) + png_raw_bytes(p) + 2 + 16 + 12; }

// CRC-32 on the host: for the 17 bytes of IHDR only (the payload's CRCs are the device's)
static uint32_t png_crc_host(const uint8_t *p, size_t n) {
    uint32_t r = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        r ^= p[i];
        for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (PNG_CRC_POLY & (0u - (r & 1u)));
    }
    return ~r;
}
static void png_be32(std::vector<uint8_t> &o, uint32_t v) { for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s)); }
static std::vector<uint8_t> png_header(const SphPngParams &p) {
    std::vector<uint8_t> o{0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    png_be32(o, 13);
    const size_t tag = o.size();
    o.insert(o.end(), {'I', 'H', 'D', 'R'});
    png_be32(o, (uint32_t)p.width); png_be32(o, (uint32_t)p.height);
    o.insert(o.end(), {8, 2, 0, 0, 0});   // 8 bits, colour type 2 (RGB), deflate, filter method 0, not interlaced
    png_be32(o, png_crc_host(o.data() + tag, o.size() - tag));
    return o;
}
static const uint8_t PNG_IEND[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};

extern "C" int sph_png_bound(const SphPngParams *params, int64_t *bytes) {
    if (!params || !bytes) return fail(nullptr, SPH_ERR_INVALID, "sph_png_bound: null argument");
    if (const char *why = png_check(*params)) return fail(nullptr, SPH_ERR_INVALID, "sph_png_bound: %s", why);
    *bytes = png_bound(*params);
    return SPH_OK;
}

extern "C" int sph_png_create(const SphPngParams *params, SphPng **out) {
    if (!params || !out) return fail(nullptr, SPH_ERR_INVALID, "sph_png_create: null argument");
    *out = nullptr;
    const SphPngParams p = *params;
    if (const char *why = png_check(p)) return fail(nullptr, SPH_ERR_INVALID, "sph_png_create: %s", why);
    int dev = 0;
    { int rc = pick_device("sph_png_create", p.device, &dev); if (rc) return rc; }
    SphPng *v = new SphPng();
    v->prm = p;
    v->header = png_header(p);
    v->trailer.assign(PNG_IEND, PNG_IEND + 12);
    PngDev &d = v->d;
    d.W = p.width; d.H = p.height; d.filter = p.filter;
    d.stride = 1 + 3 * p.width;
    d.raw = (int)png_raw_bytes(p);   // <= 3 x 2^26 + 2^14
    d.nseg = (int)png_segments(p);
    d.crc_pow[0] = 0x80000000u;   // x^0; a register step with no data multiplies by x
    for (int k = 0; k < 8 * PNG_CRC_PIECE; ++k) d.crc_pow[0] = (d.crc_pow[0] >> 1) ^ (PNG_CRC_POLY & (0u - (d.crc_pow[0] & 1u)));
    for (int j = 1; j < 8; ++j) d.crc_pow[j] = png_crc_mul(d.crc_pow[j - 1], d.crc_pow[j - 1]);
    DevBuf *b = v->buf;
    int rc = enc_open(v, "sph_png_create", p.width, p.height, dev, p.fast_math);
    if (!rc && (b[PB_FLT].reserve(nullptr, (size_t)d.nseg * PNG_SEG + 16) ||   // (+ 16: png_word_at reads the word behind a byte)
                b[PB_LEN].reserve(nullptr, sizeof(int) * ((size_t)d.nseg + 1)) ||
                b[PB_ADLER].reserve(nullptr, sizeof(unsigned) * 2 * (size_t)d.nseg) ||
                b[PB_CNT].reserve(nullptr, PNG_NCNT * sizeof(unsigned long long) + sizeof(unsigned)) || b[PB_SIDE].reserve(nullptr, (size_t)d.nseg * PNG_SIDE)))
        rc = enc_no_room(v, "sph_png_create");
    if (rc) { sph_png_destroy(v); return rc; }
    d.flt = (unsigned char *)b[PB_FLT].p; d.len = (int *)b[PB_LEN].p; d.adler = (unsigned *)b[PB_ADLER].p;
    d.cnt = (unsigned long long *)b[PB_CNT].p; d.sum = (unsigned *)(d.cnt + PNG_NCNT);
    d.side = nullptr;   // coding = fixed
    d.prev = nullptr;
    d.stream = v->stream;
    *out = v;
    return SPH_OK;
}

extern "C" void sph_png_destroy(SphPng *v) {
    if (!v) return;
    enc_close(v, v->buf, PB_COUNT_);
    delete v;
}

extern "C" const char *sph_png_last_error(SphPng *v) { return last_error(v); }

extern "C" int sph_png_set_coding(SphPng *v, int32_t coding) {
    if (!v) return fail(nullptr, SPH_ERR_INVALID, "sph_png_set_coding: null encoder");
    if (coding != SPH_PNG_CODING_FIXED && coding != SPH_PNG_CODING_DYNAMIC && coding != SPH_PNG_CODING_WINDOW)
        return fail(v, SPH_ERR_INVALID, "sph_png_set_coding: coding is %d (fixed), %d (dynamic) or %d (window), not %d", SPH_PNG_CODING_FIXED,
                    SPH_PNG_CODING_DYNAMIC, SPH_PNG_CODING_WINDOW, (int)coding);
    PngDev &d = v->d;
    if (coding == SPH_PNG_CODING_WINDOW) {   // the sort's two sides, prev and the larger side records: only an encoder that asks has them
        HIPCHK(v, hipSetDevice(v->device));
        DevBuf *b = v->buf;
        const size_t words = sizeof(unsigned) * (size_t)d.raw;
        const int nsort = d.raw > 2 ? (d.raw - 2 + PNG_SORT_TILE - 1) / PNG_SORT_TILE : 0;
        int rc = b[PB_WSIDE].reserve(v, (size_t)d.nseg * PNG_WSIDE);
        if (!rc) rc = b[PB_PREV].reserve(v, sizeof(unsigned) * (size_t)d.nseg * PNG_SEG);
        for (int k = PB_KEY0; !rc && k <= PB_POS1; ++k) rc = b[k].reserve(v, words);
        if (!rc) rc = b[PB_HIST].reserve(v, sizeof(int) * 256 * ((size_t)nsort + 1));
        if (rc) return rc;   // (the encoder is as it was)
        d.nsort = nsort;
        d.sort_key[0] = (unsigned *)b[PB_KEY0].p; d.sort_key[1] = (unsigned *)b[PB_KEY1].p;
        d.sort_pos[0] = (unsigned *)b[PB_POS0].p; d.sort_pos[1] = (unsigned *)b[PB_POS1].p;
        d.hist = (int *)b[PB_HIST].p;
    }
    v->coding = coding;
    // which instantiations the launchers run
    d.side = (unsigned char *)(coding == SPH_PNG_CODING_DYNAMIC ? v->buf[PB_SIDE].p : coding == SPH_PNG_CODING_WINDOW ? v->buf[PB_WSIDE].p : nullptr);
    d.prev = coding == SPH_PNG_CODING_WINDOW ? (unsigned *)v->buf[PB_PREV].p : nullptr;
    return SPH_OK;
}

// after the opening of an encode: filter, count, scan, size the output, write; synchronous
static int png_run(SphPng *v) {
    PngDev &d = v->d;
    StageClock &k = v->clk[0];
    d.rgb = v->src;
    HIPCHK(v, hipMemsetAsync(d.cnt, 0, PNG_NCNT * sizeof(unsigned long long) + sizeof(unsigned), v->stream));
    HIPCHK(v, k.mark(1));
    v->L->png_filter(d);
    HIPCHK(v, k.mark(2));
    StageClock &kc = v->clk[1];   // (its first two events: around the candidates)
    if (d.prev) {
        HIPCHK(v, kc.mark(0));
        v->L->png_candidates(d);
        HIPCHK(v, kc.mark(1));
    }
    v->L->png_count(d);
    HIPCHK(v, k.mark(3));
    v->L->png_scan(d);
    int total = 0;
    unsigned long long c[PNG_NCNT] = {};
    HIPCHK(v, hipMemcpyAsync(&total, d.len + d.nseg, sizeof(int), hipMemcpyDeviceToHost, v->stream));
    HIPCHK(v, hipMemcpyAsync(c, d.cnt, sizeof(c), hipMemcpyDeviceToHost, v->stream));
    HIPCHK(v, k.mark(4));
    HIPCHK(v, hipStreamSynchronize(v->stream));
    HIPCHK(v, hipGetLastError());
    const int64_t most = png_bound(v->prm) - (int64_t)v->header.size() - 12 - 16;
    if (total < 13 || total > most) return fail(v, SPH_ERR_HIP, "sph_png: the count pass left %d chunk bytes (at most %lld)", total, (long long)most);
    { int rc = enc_room(v, total, 16); if (rc) return rc; }   // (16: the Adler-32's chunk)
    d.out = (unsigned char *)v->out.p;
    v->L->png_write(d);
    HIPCHK(v, k.mark(5));
    HIPCHK(v, hipStreamSynchronize(v->stream));
    HIPCHK(v, hipGetLastError());
    v->have_frame = true;
    SphPngStats &o = v->stats;
    o.raw_bytes = d.raw;
    o.zlib_bytes = (int64_t)total - 12 * (int64_t)d.nseg + 4;
    o.file_bytes = enc_file_bytes(v);
    o.segments = d.nseg; o.stored_segments = (int64_t)c[5]; o.literals = (int64_t)c[6]; o.matches = (int64_t)c[7];
    o.dynamic_segments = (int64_t)c[8]; o.dynamic_header_bits = (int64_t)c[9];
    for (int t = 0; t < 5; ++t) o.filter_rows[t] = (int64_t)c[t];
    o.ms_input = k.ms(0, 1); o.ms_filter = k.ms(1, 2); o.ms_count = k.ms(2, 3); o.ms_scan = k.ms(3, 4); o.ms_write = k.ms(4, 5);
    o.ms_total = k.ms(0, 5);
    SphPngWindowStats &w = v->wstats;
    w = SphPngWindowStats{};
    v->have_candidates = d.prev != nullptr;
    if (d.prev) {
        w.window_segments = (int64_t)c[10]; w.window_matches = (int64_t)c[11]; w.window_far_matches = (int64_t)c[12];
        w.window_header_bits = (int64_t)c[13];
        w.ms_candidates = kc.ms(0, 1);
        o.ms_count = ev_ms(kc.ev[1], k.ev[3]);   // (the count pass alone, as in the other codings)
    }
    return SPH_OK;
}

extern "C" int sph_png_encode_rgb(SphPng *v, const uint8_t *rgb) {
    const int rc = enc_begin_rgb(v, "sph_png_encode_rgb", rgb);
    return rc ? rc : png_run(v);
}

extern "C" int sph_png_encode_render(SphPng *v, SphRender *r) {
    const int rc = enc_begin_render(v, "sph_png_encode_render", r);
    return rc ? rc : png_run(v);
}

extern "C" int sph_png_size(SphPng *v, int64_t *bytes) { return enc_size(v, "sph_png_size", bytes); }

extern "C" int sph_png_download(SphPng *v, uint8_t *dst) { return enc_download(v, "sph_png_download", dst); }

extern "C" int sph_png_window_stats(SphPng *v, SphPngWindowStats *out) {
    if (!v || !out) return SPH_ERR_INVALID;
    *out = v->have_frame ? v->wstats : SphPngWindowStats{};
    return SPH_OK;
}

extern "C" int sph_png_download_candidates(SphPng *v, uint32_t *prev, size_t n) {
    if (!v || !prev) return SPH_ERR_INVALID;
    if (!v->have_frame || !v->have_candidates) return fail(v, SPH_ERR_INVALID, "sph_png_download_candidates: the frame held was not encoded in the window coding");
    if (n != (size_t)v->d.raw) return fail(v, SPH_ERR_INVALID, "sph_png_download_candidates: the filtered stream has %d bytes, not %zu", v->d.raw, n);
    HIPCHK(v, hipSetDevice(v->device));
    HIPCHK(v, hipMemcpy(prev, v->buf[PB_PREV].p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return SPH_OK;
}

extern "C" int sph_png_stats(SphPng *v, SphPngStats *out) {
    if (!v || !out) return SPH_ERR_INVALID;
    *out = v->have_frame ? v->stats : SphPngStats{};   // (a frame that went with the opening of an encode took its figures along)
    return SPH_OK;
}
