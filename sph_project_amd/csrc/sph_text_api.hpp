// sph_text_api.hpp -- the SphText object of include/sph_hip.h: the sources (host points, an object of a live handle, a host mesh, a
// surface's mesh), the piece loop with its two pinned buffers and the stage marks.  Host code, included at the end of sph_api.hip; the
// kernels are in sph_text_passes.hpp, the number formats in sph_text.hpp, the method in DESIGN.md 23.
#pragma once
#include <chrono>
#include "sph_text.hpp"

enum TextBufId { TB_XYZ, TB_NRM, TB_TRI, TB_SLOT, TB_LEN, TB_SCAN, TB_OUT, TB_SMALL, TB_COUNT_ };
#define TEXT_PIECE_ROWS_DEFAULT (1 << 20)
#define TEXT_PIECE_ROWS_MAX (1 << 22)
static_assert((int64_t)TEXT_PIECE_ROWS_MAX * TEXT_ROW_MAX < ((int64_t)1 << 31), "offsets inside a piece fit 32 bits");

struct SphText : DevObj {   // clk[k & 1]: the stages of piece k (0 count 1 scan 2 | 3 write 4 copy 5)
    SphTextParams prm;
    TextDev d{};
    DevBuf buf[TB_COUNT_];
    int piece_rows = TEXT_PIECE_ROWS_DEFAULT;
    bool bound = false;
    int64_t rows_total = 0, values = 0;
    void *pin[2] = {nullptr, nullptr};   // pinned host memory: piece k lands in pin[k & 1]
    size_t pin_bytes[2] = {0, 0};
    int *tot = nullptr;                  // pinned [2]: the bytes of piece k arrive in tot[k & 1] without blocking the host
    hipEvent_t ev_src[2] = {nullptr, nullptr};
    double ms_source = 0.0;
    SphTextStats stats{};
};

static double text_now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

extern "C" int sph_text_create(const SphTextParams *params, SphText **out) {
    if (!params || !out) return fail(nullptr, SPH_ERR_INVALID, "sph_text_create: null argument");
    *out = nullptr;
    const SphTextParams p = *params;
    if (p.piece_rows < 0 || p.piece_rows > TEXT_PIECE_ROWS_MAX)
        return fail(nullptr, SPH_ERR_INVALID, "sph_text_create: piece_rows is 1..%d (0: the default %d), not %d", TEXT_PIECE_ROWS_MAX, TEXT_PIECE_ROWS_DEFAULT, (int)p.piece_rows);
    if (p.reserved != 0) return fail(nullptr, SPH_ERR_INVALID, "sph_text_create: reserved must be 0");
    int dev = 0;
    { int rc = pick_device("sph_text_create", p.device, &dev); if (rc) return rc; }
    SphText *t = new SphText();
    t->prm = p;
    t->piece_rows = p.piece_rows ? p.piece_rows : TEXT_PIECE_ROWS_DEFAULT;
    int rc = devobj_open(t, "sph_text_create", dev, p.fast_math);
    if (!rc && (hipEventCreate(&t->ev_src[0]) != hipSuccess || hipEventCreate(&t->ev_src[1]) != hipSuccess)) rc = fail(nullptr, SPH_ERR_HIP, "sph_text_create: event");
    if (!rc && (t->buf[TB_SMALL].reserve(nullptr, 64) || hipHostMalloc((void **)&t->tot, 64, hipHostMallocDefault) != hipSuccess))
        rc = fail(nullptr, SPH_ERR_HIP, "sph_text_create: buffers");
    if (rc) { sph_text_destroy(t); return rc; }
    t->d.stream = t->stream;
    t->d.longest = (int *)t->buf[TB_SMALL].p;   // [0] longest row, [1] bad index flag
    *out = t;
    return SPH_OK;
}

extern "C" void sph_text_destroy(SphText *t) {
    if (!t) return;
    devobj_close(t, t->buf, TB_COUNT_);
    for (hipEvent_t e : t->ev_src) if (e) hipEventDestroy(e);
    for (void *p : t->pin) if (p) hipHostFree(p);
    if (t->tot) hipHostFree(t->tot);
    delete t;
}

extern "C" const char *sph_text_last_error(SphText *t) { return last_error(t); }

static void text_unbind(SphText *t) {
    t->bound = false;
    t->rows_total = t->values = 0;
    t->ms_source = 0.0;
    t->stats = SphTextStats{};
}
// the source is in place (its arrival between ev_src[0] and ev_src[1] on the stream, already waited for)
static int text_bind(SphText *t, int kind, int64_t nv, int64_t nt) {
    TextDev &d = t->d;
    d.kind = kind; d.nv = nv; d.nt = nt;
    const int64_t per = d.nrm ? 2 : 1;
    t->rows_total = kind == 0 ? nv : per * nv + nt;
    t->values = kind == 0 ? 3 * nv : 3 * per * nv + 3 * per * nt;
    t->ms_source = ev_ms(t->ev_src[0], t->ev_src[1]);
    t->stats.ms_source = t->ms_source;
    t->bound = true;
    return SPH_OK;
}

extern "C" int sph_text_ply_points(SphText *t, const float *xyz, int64_t n) {
    if (!t) return SPH_ERR_INVALID;
    text_unbind(t);
    if (n < 0) return fail(t, SPH_ERR_INVALID, "sph_text_ply_points: negative count %lld", (long long)n);
    if (n > 0 && !xyz) return fail(t, SPH_ERR_INVALID, "sph_text_ply_points: null points");
    HIPCHK(t, hipSetDevice(t->device));
    { int rc = t->buf[TB_XYZ].reserve(t, 12 * (size_t)n + 16); if (rc) return rc; }
    HIPCHK(t, hipEventRecord(t->ev_src[0], t->stream));
    if (n) HIPCHK(t, hipMemcpyAsync(t->buf[TB_XYZ].p, xyz, 12 * (size_t)n, hipMemcpyHostToDevice, t->stream));
    HIPCHK(t, hipEventRecord(t->ev_src[1], t->stream));
    HIPCHK(t, hipStreamSynchronize(t->stream));
    t->d.xyz = (const unsigned *)t->buf[TB_XYZ].p; t->d.nrm = nullptr; t->d.tri = nullptr;
    return text_bind(t, 0, n, 0);
}

extern "C" int sph_text_ply_object(SphText *t, SphHandle *h, int object_id) {
    if (!t) return SPH_ERR_INVALID;
    text_unbind(t);
    if (!h) return fail(t, SPH_ERR_INVALID, "sph_text_ply_object: null handle");
    if (h->st.slab_active || h->swap_axis)
        return fail(t, SPH_ERR_UNSUPPORTED, "sph_text_ply_object: sharded handle (write each rank's download with sph_write_ply_ascii_part instead)");
    if (h->device != t->device) return fail(t, SPH_ERR_INVALID, "sph_text_ply_object: handle on device %d, exporter on device %d", h->device, t->device);
    if (h->in_step) return fail(t, SPH_ERR_INVALID, "sph_text_ply_object: between sph_step_begin and sph_step_end");
    if (object_id < 0 || object_id >= SPH_MAX_OBJECTS) return fail(t, SPH_ERR_INVALID, "sph_text_ply_object: object id %d", object_id);
    HIPCHK(t, hipSetDevice(t->device));
    HIPCHK(t, hipStreamSynchronize(h->st.stream));   // the handle's last step has written the positions
    const int n_all = h->n;
    { int rc = t->buf[TB_XYZ].reserve(t, 12 * (size_t)n_all + 16); if (rc) return rc; }
    { int rc = t->buf[TB_SLOT].reserve(t, sizeof(int) * ((size_t)n_all + 1)); if (rc) return rc; }
    { int rc = t->buf[TB_SCAN].reserve(t, sizeof(int) * ((size_t)n_all / 1024 + 2)); if (rc) return rc; }
    t->d.scan_tmp = (int *)t->buf[TB_SCAN].p;
    int *slot = (int *)t->buf[TB_SLOT].p;
    HIPCHK(t, hipEventRecord(t->ev_src[0], t->stream));
    t->L->text_compact(t->d, h->st.posv.cur(), h->st.meta.cur(), n_all, object_id, slot, (float *)t->buf[TB_XYZ].p);
    int n = 0;
    HIPCHK(t, hipMemcpyAsync(&n, slot + n_all, sizeof(int), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(t, hipEventRecord(t->ev_src[1], t->stream));
    HIPCHK(t, hipStreamSynchronize(t->stream));
    HIPCHK(t, hipGetLastError());
    if (n < 0 || n > n_all) return fail(t, SPH_ERR_HIP, "sph_text_ply_object: the compaction left %d of %d particles", n, n_all);
    t->d.xyz = (const unsigned *)t->buf[TB_XYZ].p; t->d.nrm = nullptr; t->d.tri = nullptr;
    return text_bind(t, 0, n, 0);
}

// the mesh is on the device (t->d.xyz / nrm / tri): its indices, checked before a byte is written
static int text_bind_mesh(SphText *t, const char *who, int64_t nv, int64_t nt) {
    TextDev &d = t->d;
    d.nv = nv; d.nt = nt;
    int *bad_dev = d.longest + 1;
    t->L->text_check_tri(d, bad_dev);
    int bad = 0;
    HIPCHK(t, hipMemcpyAsync(&bad, bad_dev, sizeof(int), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(t, hipEventRecord(t->ev_src[1], t->stream));
    HIPCHK(t, hipStreamSynchronize(t->stream));
    HIPCHK(t, hipGetLastError());
    if (bad) return fail(t, SPH_ERR_INVALID, "%s: a triangle index lies outside [0, %lld)", who, (long long)nv);
    return text_bind(t, 1, nv, nt);
}

extern "C" int sph_text_obj_mesh(SphText *t, const float *v, int64_t nv, const float *nrm, const int32_t *tri, int64_t nt) {
    if (!t) return SPH_ERR_INVALID;
    text_unbind(t);
    if (nv < 0 || nt < 0) return fail(t, SPH_ERR_INVALID, "sph_text_obj_mesh: negative count (nv = %lld, nt = %lld)", (long long)nv, (long long)nt);
    if (nv > (int64_t)INT32_MAX) return fail(t, SPH_ERR_INVALID, "sph_text_obj_mesh: %lld vertices, more than int32 indices reach", (long long)nv);
    if ((nv > 0 && !v) || (nt > 0 && !tri)) return fail(t, SPH_ERR_INVALID, "sph_text_obj_mesh: null array");
    HIPCHK(t, hipSetDevice(t->device));
    { int rc = t->buf[TB_XYZ].reserve(t, 12 * (size_t)nv + 16); if (rc) return rc; }
    if (nrm) { int rc = t->buf[TB_NRM].reserve(t, 12 * (size_t)nv + 16); if (rc) return rc; }
    { int rc = t->buf[TB_TRI].reserve(t, 12 * (size_t)nt + 16); if (rc) return rc; }
    HIPCHK(t, hipEventRecord(t->ev_src[0], t->stream));
    if (nv) HIPCHK(t, hipMemcpyAsync(t->buf[TB_XYZ].p, v, 12 * (size_t)nv, hipMemcpyHostToDevice, t->stream));
    if (nv && nrm) HIPCHK(t, hipMemcpyAsync(t->buf[TB_NRM].p, nrm, 12 * (size_t)nv, hipMemcpyHostToDevice, t->stream));
    if (nt) HIPCHK(t, hipMemcpyAsync(t->buf[TB_TRI].p, tri, 12 * (size_t)nt, hipMemcpyHostToDevice, t->stream));
    t->d.xyz = (const unsigned *)t->buf[TB_XYZ].p;
    t->d.nrm = nrm ? (const unsigned *)t->buf[TB_NRM].p : nullptr;
    t->d.tri = (const int *)t->buf[TB_TRI].p;
    return text_bind_mesh(t, "sph_text_obj_mesh", nv, nt);
}

extern "C" int sph_text_obj_surface(SphText *t, SphSurface *s) {
    if (!t) return SPH_ERR_INVALID;
    text_unbind(t);
    if (!s) return fail(t, SPH_ERR_INVALID, "sph_text_obj_surface: null surface");
    if (!s->have_mesh) return fail(t, SPH_ERR_INVALID, "sph_text_obj_surface: the surface holds no mesh (no reconstruction has succeeded yet)");
    if (s->device != t->device) return fail(t, SPH_ERR_INVALID, "sph_text_obj_surface: surface on device %d, exporter on device %d", s->device, t->device);
    HIPCHK(t, hipSetDevice(t->device));
    HIPCHK(t, hipStreamSynchronize(s->stream));   // (the reconstruct calls are synchronous: the mesh is complete)
    HIPCHK(t, hipEventRecord(t->ev_src[0], t->stream));
    const bool any = s->nv > 0;
    t->d.xyz = any ? (const unsigned *)s->d.vert : nullptr;
    t->d.nrm = s->prm.normals ? (any ? (const unsigned *)s->d.nrm : (const unsigned *)t->buf[TB_SMALL].p) : nullptr;   // (non-null: "with normals")
    t->d.tri = s->nt > 0 ? (const int *)s->d.tri : nullptr;
    return text_bind_mesh(t, "sph_text_obj_surface", s->nv, s->nt);   // read in place: nothing of the surface is written
}

static int text_pin(SphText *t, int k, size_t need) {
    if (t->pin_bytes[k] >= need) return SPH_OK;
    if (t->pin[k]) hipHostFree(t->pin[k]);
    t->pin[k] = nullptr; t->pin_bytes[k] = 0;
    need += need / 4 + 4096;   // some room: pieces of one file are of similar size
    HIPCHK(t, hipHostMalloc(&t->pin[k], need, hipHostMallocDefault));
    t->pin_bytes[k] = need;
    return SPH_OK;
}

// count and scan of piece k, its byte total on the way to tot
static int text_enqueue_count(SphText *t, int64_t k, int *tot) {
    TextDev &d = t->d;
    StageClock &c = t->clk[k & 1];
    d.row0 = k * (int64_t)t->piece_rows;
    d.rows = (int)std::min<int64_t>(t->piece_rows, t->rows_total - d.row0);
    HIPCHK(t, c.mark(0));
    t->L->text_count(d);
    HIPCHK(t, c.mark(1));
    t->L->text_scan(d);
    HIPCHK(t, hipMemcpyAsync(tot, d.len + d.rows, sizeof(int), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(t, c.mark(2));
    return SPH_OK;
}

// the file of the bound source into f, into dst[cap], or (neither) only counted.  Piece k: count, scan | host reads its bytes | write,
// copy to pin[k & 1]; the count of piece k + 1 is enqueued behind it, and while the device works the host stores piece k - 1.
static int text_run(SphText *t, const char *who, FILE *f, char *dst, int64_t cap) {
    if (!t->bound) return fail(t, SPH_ERR_INVALID, "%s: no source bound (call one of sph_text_ply_points / _ply_object / _obj_mesh / _obj_surface first)", who);
    HIPCHK(t, hipSetDevice(t->device));
    const double t_begin = text_now_ms();
    TextDev &d = t->d;
    const bool store = f || dst;
    SphTextStats o{};
    o.rows = t->rows_total; o.values = t->values; o.ms_source = t->ms_source;
    char header[256];
    int nh = 0;
    if (d.kind == 0)
        nh = snprintf(header, sizeof(header), "ply\nformat ascii 1.0\ncomment created by PLYWriter\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\nend_header\n", (long long)t->rows_total);
    int64_t total = nh;
    double ms_file = 0.0;
    auto sink = [&](const void *p, size_t n, int64_t at) -> int {   // n bytes of the file at offset `at`
        const double a = text_now_ms();
        int rc = SPH_OK;
        if (f && n && fwrite(p, 1, n, f) != n) rc = fail(t, SPH_ERR_UNSUPPORTED, "%s: write failed", who);
        if (dst) {
            if (at + (int64_t)n > cap) rc = fail(t, SPH_ERR_CAPACITY, "%s: the file is longer than the %lld bytes given", who, (long long)cap);
            else if (n) memcpy(dst + at, p, n);
        }
        ms_file += text_now_ms() - a;
        return rc;
    };
    { int rc = sink(header, (size_t)nh, 0); if (rc) return rc; }
    const int64_t pieces = (t->rows_total + t->piece_rows - 1) / t->piece_rows;
    const int most = (int)std::min<int64_t>(t->piece_rows, t->rows_total);
    { int rc = t->buf[TB_LEN].reserve(t, sizeof(int) * ((size_t)most + 1)); if (rc) return rc; }
    { int rc = t->buf[TB_SCAN].reserve(t, sizeof(int) * ((size_t)most / 1024 + 2)); if (rc) return rc; }
    d.len = (int *)t->buf[TB_LEN].p; d.scan_tmp = (int *)t->buf[TB_SCAN].p;
    HIPCHK(t, hipMemsetAsync(d.longest, 0, sizeof(int), t->stream));
    int *tot = t->tot;
    tot[0] = tot[1] = 0;
    int64_t at_prev = 0, bytes_prev = 0;   // piece k - 1: where it goes in the file, its bytes (in pin[(k - 1) & 1])
    if (pieces) { int rc = text_enqueue_count(t, 0, &tot[0]); if (rc) return rc; }
    for (int64_t k = 0; k < pieces; ++k) {
        HIPCHK(t, hipStreamSynchronize(t->stream));   // piece k is counted; piece k - 1 lies in its pinned buffer
        HIPCHK(t, hipGetLastError());
        const StageClock &ck = t->clk[k & 1];
        o.ms_count += ck.ms(0, 1); o.ms_scan += ck.ms(1, 2);
        if (k > 0 && store) { const StageClock &cp = t->clk[(k - 1) & 1]; o.ms_write += cp.ms(3, 4); o.ms_copy += cp.ms(4, 5); }
        const int bytes = tot[k & 1];
        const int rows_k = (int)std::min<int64_t>(t->piece_rows, t->rows_total - k * (int64_t)t->piece_rows);
        if (bytes < rows_k || (int64_t)bytes > (int64_t)rows_k * TEXT_ROW_MAX)
            return fail(t, SPH_ERR_HIP, "%s: the count pass left %d bytes for %d rows", who, bytes, rows_k);
        const int64_t at = total;
        total += bytes;
        if (store) {
            { int rc = t->buf[TB_OUT].reserve(t, (size_t)bytes + (size_t)bytes / 4 + 64); if (rc) return rc; }
            { int rc = text_pin(t, (int)(k & 1), (size_t)bytes); if (rc) return rc; }
            d.out = (unsigned char *)t->buf[TB_OUT].p;
            // (d.row0 / d.rows are still piece k's: text_enqueue_count set them last)
            StageClock &c = t->clk[k & 1];
            HIPCHK(t, c.mark(3));
            t->L->text_write(d);
            HIPCHK(t, c.mark(4));
            HIPCHK(t, hipMemcpyAsync(t->pin[k & 1], d.out, (size_t)bytes, hipMemcpyDeviceToHost, t->stream));
            HIPCHK(t, c.mark(5));
        }
        if (k + 1 < pieces) { int rc = text_enqueue_count(t, k + 1, &tot[(k + 1) & 1]); if (rc) return rc; }
        if (k > 0 && store) { int rc = sink(t->pin[(k - 1) & 1], (size_t)bytes_prev, at_prev); if (rc) return rc; }
        at_prev = at; bytes_prev = bytes;
    }
    int longest = 0;
    HIPCHK(t, hipMemcpyAsync(&longest, d.longest, sizeof(int), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(t, hipStreamSynchronize(t->stream));
    HIPCHK(t, hipGetLastError());
    if (pieces && store) {
        const StageClock &cp = t->clk[(pieces - 1) & 1];
        o.ms_write += cp.ms(3, 4); o.ms_copy += cp.ms(4, 5);
        int rc = sink(t->pin[(pieces - 1) & 1], (size_t)bytes_prev, at_prev);
        if (rc) return rc;
    }
    o.bytes = total; o.pieces = pieces; o.longest_row = longest;
    o.ms_file = ms_file;
    o.ms_total = text_now_ms() - t_begin;
    t->stats = o;
    return SPH_OK;
}

extern "C" int sph_text_write(SphText *t, const char *path) {
    if (!t) return SPH_ERR_INVALID;
    if (!path) return fail(t, SPH_ERR_INVALID, "sph_text_write: null path");
    if (!t->bound) return text_run(t, "sph_text_write", nullptr, nullptr, 0);   // (the refusal, before the file is touched)
    FILE *f = fopen(path, "wb");
    if (!f) return fail(t, SPH_ERR_UNSUPPORTED, "sph_text_write: cannot open %s for writing", path);
    int rc = text_run(t, "sph_text_write", f, nullptr, 0);
    if (fclose(f) != 0 && rc == SPH_OK) rc = fail(t, SPH_ERR_UNSUPPORTED, "sph_text_write: closing %s failed", path);
    return rc;
}

extern "C" int sph_text_size(SphText *t, int64_t *bytes) {
    if (!t) return SPH_ERR_INVALID;
    if (!bytes) return fail(t, SPH_ERR_INVALID, "sph_text_size: null argument");
    const int rc = text_run(t, "sph_text_size", nullptr, nullptr, 0);
    if (rc == SPH_OK) *bytes = t->stats.bytes;
    return rc;
}

extern "C" int sph_text_read(SphText *t, void *dst, int64_t cap) {
    if (!t) return SPH_ERR_INVALID;
    if (!dst || cap < 0) return fail(t, SPH_ERR_INVALID, "sph_text_read: null destination or negative capacity");
    return text_run(t, "sph_text_read", nullptr, (char *)dst, cap);
}

extern "C" int sph_text_stats(SphText *t, SphTextStats *out) {
    if (!t || !out) return SPH_ERR_INVALID;
    *out = t->stats;
    return SPH_OK;
}

extern "C" int sph_text_format_f32_host(const float *values, int64_t n, char *out, int64_t cap, int64_t *lengths) {
    if (n < 0 || cap < 0) return fail(nullptr, SPH_ERR_INVALID, "sph_text_format_f32_host: negative count or capacity");
    if (!out || !lengths || (n > 0 && !values)) return fail(nullptr, SPH_ERR_INVALID, "sph_text_format_f32_host: null argument");
    int64_t used = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t bits;
        memcpy(&bits, &values[i], 4);
        const int len = text_f32_len(bits);
        if (used + len > cap) return fail(nullptr, SPH_ERR_CAPACITY, "sph_text_format_f32_host: value %lld needs %d bytes, %lld left", (long long)i, len, (long long)(cap - used));
        text_f32(bits, out + used);
        lengths[i] = len;
        used += len;
    }
    return SPH_OK;
}
