// sph_video_api.hpp -- the SphVideo object of include/sph_hip.h: the tables of T.81 Annex K and the fixed headers built from them, the
// frame source (sph_encoder_api.hpp), the two-pass encode and the stage marks.  Host code, included at the end of sph_api.hip; the
// kernels are in sph_video.hpp, the stream is defined in DESIGN.md 18.
#pragma once

static const unsigned char VIDEO_K1[64] = {   // T.81 table K.1 (luminance), natural order
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99};
static const unsigned char VIDEO_K2[64] = {   // T.81 table K.2 (chrominance)
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99};
static const unsigned char VIDEO_DC0_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};   // T.81 table K.3
static const unsigned char VIDEO_DC0_VALS[12] = {
    0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b};
static const unsigned char VIDEO_AC0_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};   // T.81 table K.5
static const unsigned char VIDEO_AC0_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const unsigned char VIDEO_DC1_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};   // T.81 table K.4
static const unsigned char VIDEO_DC1_VALS[12] = {
    0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b};
static const unsigned char VIDEO_AC1_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};   // T.81 table K.6
static const unsigned char VIDEO_AC1_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const unsigned char VIDEO_ZIGZAG[64] = {   // zigzag position -> natural index (T.81 figure A.6)
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

enum VideoBufId { VB_TAB, VB_LEN, VB_CNT, VB_COUNT_ };

struct SphVideo : FrameEncoder {   // header: SOI ... SOS; payload: the entropy-coded scan; trailer: EOI
    SphVideoParams prm;
    VideoDev d{};
    DevBuf buf[VB_COUNT_];
    SphVideoStats stats{};         // of the frame held
};

static const char *video_check(const SphVideoParams &p) {
    if (const char *why = enc_check_size(p.width, p.height)) return why;
    if (p.quality < 1 || p.quality > 100) return "quality is 1..100";
    if (p.chroma != 420 && p.chroma != 444) return "chroma is 420 or 444";
    if (p.reserved != 0) return "reserved must be 0";
    return nullptr;
}

// the Annex K tables scaled by the IJG rule: quality < 50: 5000 / quality, else 200 - 2 quality; (step * scale + 50) / 100 in 1..255
static void video_quant(int quality, VideoTables &t) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        t.q[0][k] = (unsigned short)std::min(std::max((VIDEO_K1[k] * scale + 50) / 100, 1), 255);
        t.q[1][k] = (unsigned short)std::min(std::max((VIDEO_K2[k] * scale + 50) / 100, 1), 255);
    }
}
// canonical codes from a BITS / HUFFVAL pair (T.81 annex C): out[symbol] = code | length << 16
static void video_codes(const unsigned char *bits, const unsigned char *vals, unsigned *out) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = code++ | (unsigned)len << 16;
        code <<= 1;
    }
}
static VideoTables video_tables(int quality) {
    VideoTables t{};
    video_quant(quality, t);
    video_codes(VIDEO_DC0_BITS, VIDEO_DC0_VALS, t.dc[0]);
    video_codes(VIDEO_DC1_BITS, VIDEO_DC1_VALS, t.dc[1]);
    video_codes(VIDEO_AC0_BITS, VIDEO_AC0_VALS, t.ac[0]);
    video_codes(VIDEO_AC1_BITS, VIDEO_AC1_VALS, t.ac[1]);
    return t;
}

static void video_segment(std::vector<uint8_t> &o, int marker, const std::vector<uint8_t> &body) {
    const size_t n = body.size() + 2;
    o.push_back(0xff); o.push_back((uint8_t)marker); o.push_back((uint8_t)(n >> 8)); o.push_back((uint8_t)n);
    o.insert(o.end(), body.begin(), body.end());
}
static void video_dht(std::vector<uint8_t> &o, int cls_id, const unsigned char *bits, const unsigned char *vals) {
    std::vector<uint8_t> b{(uint8_t)cls_id};
    int n = 0;
    for (int k = 0; k < 16; ++k) { b.push_back(bits[k]); n += bits[k]; }
    b.insert(b.end(), vals, vals + n);
    video_segment(o, 0xC4, b);
}
// SOI, APP0 (JFIF 1.01, no density), DQT luminance, DQT chrominance, SOF0, DHT DC0 AC0 DC1 AC1, DRI, SOS
static std::vector<uint8_t> video_header(const SphVideoParams &p) {
    const VideoTables t = video_tables(p.quality);
    std::vector<uint8_t> o{0xff, 0xd8};
    video_segment(o, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int k = 0; k < 2; ++k) {
        std::vector<uint8_t> b{(uint8_t)k};
        for (int z = 0; z < 64; ++z) b.push_back((uint8_t)t.q[k][VIDEO_ZIGZAG[z]]);
        video_segment(o, 0xDB, b);
    }
    const uint8_t samp = p.chroma == 420 ? 0x22 : 0x11;
    video_segment(o, 0xC0, {8, (uint8_t)(p.height >> 8), (uint8_t)p.height, (uint8_t)(p.width >> 8), (uint8_t)p.width, 3, 1, samp, 0, 2, 0x11, 1, 3, 0x11, 1});
    video_dht(o, 0x00, VIDEO_DC0_BITS, VIDEO_DC0_VALS);
    video_dht(o, 0x10, VIDEO_AC0_BITS, VIDEO_AC0_VALS);
    video_dht(o, 0x01, VIDEO_DC1_BITS, VIDEO_DC1_VALS);
    video_dht(o, 0x11, VIDEO_AC1_BITS, VIDEO_AC1_VALS);
    video_segment(o, 0xDD, {(uint8_t)(VIDEO_RI >> 8), (uint8_t)VIDEO_RI});
    video_segment(o, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return o;
}

extern "C" int sph_video_header(const SphVideoParams *params, uint8_t *dst_or_NULL, int64_t *bytes) {
    if (!params || !bytes) return fail(nullptr, SPH_ERR_INVALID, "sph_video_header: null argument");
    if (const char *why = video_check(*params)) return fail(nullptr, SPH_ERR_INVALID, "sph_video_header: %s", why);
    const std::vector<uint8_t> h = video_header(*params);
    *bytes = (int64_t)h.size();
    if (dst_or_NULL) memcpy(dst_or_NULL, h.data(), h.size());
    return SPH_OK;
}

extern "C" int sph_video_create(const SphVideoParams *params, SphVideo **out) {
    if (!params || !out) return fail(nullptr, SPH_ERR_INVALID, "sph_video_create: null argument");
    *out = nullptr;
    const SphVideoParams p = *params;
    if (const char *why = video_check(p)) return fail(nullptr, SPH_ERR_INVALID, "sph_video_create: %s", why);
    int dev = 0;
    { int rc = pick_device("sph_video_create", p.device, &dev); if (rc) return rc; }
    SphVideo *v = new SphVideo();
    v->prm = p;
    v->header = video_header(p);
    v->trailer = {0xff, 0xd9};
    VideoDev &d = v->d;
    d.W = p.width; d.H = p.height; d.c420 = p.chroma == 420 ? 1 : 0;
    const int m = d.c420 ? 16 : 8;
    d.mw = (p.width + m - 1) / m;
    d.nmcu = d.mw * ((p.height + m - 1) / m);
    d.nint = (d.nmcu + VIDEO_RI - 1) / VIDEO_RI;
    DevBuf *b = v->buf;
    int rc = enc_open(v, "sph_video_create", p.width, p.height, dev, p.fast_math);
    if (!rc && (b[VB_TAB].reserve(nullptr, sizeof(VideoTables)) || b[VB_LEN].reserve(nullptr, sizeof(int) * ((size_t)d.nint + 1)) || b[VB_CNT].reserve(nullptr, 16)))
        rc = enc_no_room(v, "sph_video_create");
    if (rc) { sph_video_destroy(v); return rc; }
    const VideoTables t = video_tables(p.quality);
    if (hipMemcpy(b[VB_TAB].p, &t, sizeof(t), hipMemcpyHostToDevice) != hipSuccess) {
        sph_video_destroy(v);
        return fail(nullptr, SPH_ERR_HIP, "sph_video_create: table upload");
    }
    d.tab = (const VideoTables *)b[VB_TAB].p; d.len = (int *)b[VB_LEN].p; d.cnt = (unsigned long long *)b[VB_CNT].p;
    d.stream = v->stream;
    *out = v;
    return SPH_OK;
}

extern "C" void sph_video_destroy(SphVideo *v) {
    if (!v) return;
    enc_close(v, v->buf, VB_COUNT_);
    delete v;
}

extern "C" const char *sph_video_last_error(SphVideo *v) { return last_error(v); }

// after the opening of an encode: count, scan, size the output, write; synchronous
static int video_run(SphVideo *v) {
    VideoDev &d = v->d;
    StageClock &k = v->clk[0];
    d.rgb = v->src;
    HIPCHK(v, hipMemsetAsync(d.cnt, 0, 16, v->stream));
    HIPCHK(v, k.mark(1));
    v->L->video_count(d);
    HIPCHK(v, k.mark(2));
    v->L->video_scan(d);
    int total = 0;
    unsigned long long c[2] = {0, 0};
    HIPCHK(v, hipMemcpyAsync(&total, d.len + d.nint, sizeof(int), hipMemcpyDeviceToHost, v->stream));
    HIPCHK(v, hipMemcpyAsync(c, d.cnt, sizeof(c), hipMemcpyDeviceToHost, v->stream));
    HIPCHK(v, k.mark(3));
    HIPCHK(v, hipStreamSynchronize(v->stream));
    HIPCHK(v, hipGetLastError());
    if (total < 1) return fail(v, SPH_ERR_HIP, "sph_video: the count pass left %d scan bytes", total);
    { int rc = enc_room(v, total, 0); if (rc) return rc; }
    d.out = (unsigned char *)v->out.p;
    v->L->video_write(d);
    HIPCHK(v, k.mark(4));
    HIPCHK(v, hipStreamSynchronize(v->stream));
    HIPCHK(v, hipGetLastError());
    v->have_frame = true;
    SphVideoStats &o = v->stats;
    o.blocks = (int64_t)d.nmcu * (d.c420 ? 6 : 3);
    o.scan_bytes = total; o.stuffed_bytes = (int64_t)c[0]; o.restart_intervals = d.nint;
    o.ms_input = k.ms(0, 1); o.ms_count = k.ms(1, 2); o.ms_scan = k.ms(2, 3); o.ms_write = k.ms(3, 4); o.ms_total = k.ms(0, 4);
    return SPH_OK;
}

extern "C" int sph_video_encode_rgb(SphVideo *v, const uint8_t *rgb) {
    const int rc = enc_begin_rgb(v, "sph_video_encode_rgb", rgb);
    return rc ? rc : video_run(v);
}

extern "C" int sph_video_encode_render(SphVideo *v, SphRender *r) {
    const int rc = enc_begin_render(v, "sph_video_encode_render", r);
    return rc ? rc : video_run(v);
}

extern "C" int sph_video_size(SphVideo *v, int64_t *bytes) { return enc_size(v, "sph_video_size", bytes); }

extern "C" int sph_video_download(SphVideo *v, uint8_t *dst) { return enc_download(v, "sph_video_download", dst); }

extern "C" int sph_video_stats(SphVideo *v, SphVideoStats *out) {
    if (!v || !out) return SPH_ERR_INVALID;
    *out = v->have_frame ? v->stats : SphVideoStats{};   // (a frame that went with the opening of an encode took its figures along)
    return SPH_OK;
}
