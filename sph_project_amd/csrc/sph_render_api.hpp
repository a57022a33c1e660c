// sph_render_api.hpp -- the SphRender object of include/sph_hip.h: camera set-up and box-line clipping in double, the frame buffers, the
// particle sources (host points, a live handle) and the stage events.  Host code, included at the end of sph_api.hip; the kernels are in
// sph_render.hpp, the image is defined in DESIGN.md 15.
#pragma once
#include <climits>

struct SphRender {
    SphRenderParams prm;
    const Launch *L = nullptr;
    int device = 0;
    std::string err;
    RenderDev d{};
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {};
    unsigned long long *key = nullptr;
    unsigned char *rgb = nullptr;
    int *ids = nullptr;
    unsigned long long *cnt = nullptr;
    float4 *pos = nullptr;
    int *idv = nullptr, *large = nullptr;
    unsigned *col = nullptr;
    size_t cap_pts = 0, cap_large = 0;
    bool have_frame = false;
    SphRenderStats stats{};
    // mesh frames: the list between mesh_begin and mesh_end, concatenated on the device
    bool mesh_open = false;
    std::vector<MeshRec> mesh_rec;
    int64_t mesh_nv = 0, mesh_nt = 0;
    void *mvert = nullptr, *mnrm = nullptr, *mtri = nullptr, *mrec = nullptr;
    size_t cap_mvert = 0, cap_mnrm = 0, cap_mtri = 0, cap_mrec = 0;   // bytes
    hipEvent_t mev[5] = {};
    SphRenderMeshStats mstats{};
};

static int rend_fail(SphRender *r, int code, const char *fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof(b), fmt, ap);
    va_end(ap);
    if (r) r->err = b; else g_create_error = b;
    return code;
}
#define RENDCHK(r, call)                                                                                                   \
    do {                                                                                                                    \
        hipError_t e_ = (call);                                                                                             \
        if (e_ != hipSuccess) return rend_fail((r), SPH_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static bool rend_finite3(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
static double rend_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void rend_cross(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
static bool rend_normalize(double *a) {
    const double l = sqrt(rend_dot(a, a));
    if (!(l > 1e-300) || !std::isfinite(l)) return false;
    for (int k = 0; k < 3; ++k) a[k] /= l;
    return true;
}

// the 12 box edges (the reference's box_anchors / box_lines_indices, run_simulation.py:91-108), clipped at z_near and projected
static void rend_lines(const SphRenderParams &p, const double *E, const double *f, const double *s, const double *u, double tx, double ty,
                       RenderDev &d) {
    static const int idx[24] = {0, 1, 0, 2, 1, 3, 2, 3, 4, 5, 4, 6, 5, 7, 6, 7, 0, 4, 1, 5, 2, 6, 3, 7};
    double A[8][3];
    for (int a = 0; a < 8; ++a) {   // anchor a: x from bit 1, y from bit 0, z from bit 2
        A[a][0] = (a & 2) ? p.box_hi[0] : p.box_lo[0];
        A[a][1] = (a & 1) ? p.box_hi[1] : p.box_lo[1];
        A[a][2] = (a & 4) ? p.box_hi[2] : p.box_lo[2];
    }
    for (int e = 0; e < 12; ++e) {
        d.line_axis[e] = -1;
        double P[2][3], z[2];
        for (int q = 0; q < 2; ++q) {
            for (int k = 0; k < 3; ++k) P[q][k] = A[idx[2 * e + q]][k] - E[k];
            z[q] = rend_dot(f, P[q]);
        }
        if (z[0] <= p.z_near && z[1] <= p.z_near) continue;
        for (int q = 0; q < 2; ++q)
            if (z[q] < p.z_near) {   // move this end along the edge to the near plane
                const double w = (p.z_near - z[q]) / (z[1 - q] - z[q]);
                for (int k = 0; k < 3; ++k) P[q][k] += w * (P[1 - q][k] - P[q][k]);
                z[q] = p.z_near;
            }
        double px[2], py[2];
        for (int q = 0; q < 2; ++q) {
            px[q] = (rend_dot(s, P[q]) / z[q] / tx + 1.0) * 0.5 * p.width;
            py[q] = (1.0 - rend_dot(u, P[q]) / z[q] / ty) * 0.5 * p.height;
        }
        const int ax = fabs(px[1] - px[0]) >= fabs(py[1] - py[0]) ? 0 : 1;
        const double *ma = ax == 0 ? px : py, *mi = ax == 0 ? py : px;
        const int n_major = ax == 0 ? p.width : p.height;
        if (!(fabs(ma[1] - ma[0]) > 1e-9)) continue;
        const double k0 = std::max(ceil(std::min(ma[0], ma[1]) - 0.5), 0.0), k1 = std::min(floor(std::max(ma[0], ma[1]) - 0.5), (double)(n_major - 1));
        if (k0 > k1) continue;
        const double g[8] = {ma[0], mi[0], ma[1], mi[1], 1.0 / z[0], 1.0 / z[1], k0, k1};
        for (int k = 0; k < 8; ++k) d.line[e][k] = (float)g[k];
        d.line_axis[e] = ax;
    }
}

extern "C" int sph_render_create(const SphRenderParams *params, SphRender **out) {
    if (!params || !out) return rend_fail(nullptr, SPH_ERR_INVALID, "sph_render_create: null argument");
    *out = nullptr;
    const SphRenderParams p = *params;
    if (p.width < 1 || p.height < 1 || p.width > 16384 || p.height > 16384 || (int64_t)p.width * p.height > ((int64_t)1 << 26))
        return rend_fail(nullptr, SPH_ERR_INVALID, "sph_render_create: %d x %d pixels (each 1..16384, at most 2^26 in all)", p.width, p.height);
    if (!rend_finite3(p.eye) || !rend_finite3(p.target) || !rend_finite3(p.up) || !rend_finite3(p.light_pos) || !rend_finite3(p.light_rgb) ||
        !(p.fov_deg > 0.0 && p.fov_deg < 180.0) || !(p.z_near > 0.0) || !std::isfinite(p.z_near) || !(p.radius > 0.0) ||
        !std::isfinite(p.radius) || !(p.ambient >= 0.0) || !std::isfinite(p.ambient) || p.reserved != 0)
        return rend_fail(nullptr, SPH_ERR_INVALID, "sph_render_create: camera, light, fov in (0, 180), z_near > 0, radius > 0 and ambient >= 0 must be finite");
    for (int k = 0; k < 3; ++k)
        if (p.background_rgb[k] < 0 || p.background_rgb[k] > 255 || p.box_rgb[k] < 0 || p.box_rgb[k] > 255)
            return rend_fail(nullptr, SPH_ERR_INVALID, "sph_render_create: colours are 0..255");
    if (p.draw_box && (!rend_finite3(p.box_lo) || !rend_finite3(p.box_hi)))
        return rend_fail(nullptr, SPH_ERR_INVALID, "sph_render_create: box corners must be finite");
    double E[3] = {p.eye[0], p.eye[1], p.eye[2]}, f[3], s[3], u[3];
    for (int k = 0; k < 3; ++k) f[k] = p.target[k] - E[k];
    if (!rend_normalize(f)) return rend_fail(nullptr, SPH_ERR_INVALID, "sph_render_create: target equals eye");
    rend_cross(f, p.up, s);
    if (!rend_normalize(s)) return rend_fail(nullptr, SPH_ERR_INVALID, "sph_render_create: up is parallel to the view direction");
    rend_cross(s, f, u);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return rend_fail(nullptr, SPH_ERR_NO_DEVICE, "sph_render_create: no HIP device visible (libsph_hip has no CPU path)");
    int dev = p.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) return rend_fail(nullptr, SPH_ERR_NO_DEVICE, "sph_render_create: device %d not present", dev);
    hipDeviceProp_t prop;
    if (hipSetDevice(dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return rend_fail(nullptr, SPH_ERR_HIP, "sph_render_create: device %d unusable", dev);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return rend_fail(nullptr, SPH_ERR_NO_DEVICE, "sph_render_create: device %d is %s, this library is built for gfx950 only", dev, prop.gcnArchName);
    SphRender *r = new SphRender();
    r->prm = p;
    r->device = dev;
    r->L = p.fast_math ? sph_launch_fast() : sph_launch_strict();
    const size_t px = (size_t)p.width * p.height;
    if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) { delete r; return rend_fail(nullptr, SPH_ERR_HIP, "sph_render_create: stream"); }
    bool ok = true;
    for (auto &e_ : r->ev) ok = ok && hipEventCreate(&e_) == hipSuccess;
    ok = ok && hipMalloc(&r->key, px * 8) == hipSuccess && hipMalloc(&r->rgb, px * 3) == hipSuccess && hipMalloc(&r->ids, px * 4) == hipSuccess &&
         hipMalloc(&r->cnt, 64) == hipSuccess;
    if (!ok) { sph_render_destroy(r); return rend_fail(nullptr, SPH_ERR_HIP, "sph_render_create: %zu pixels of frame buffers", px); }
    RenderDev &d = r->d;
    d.W = p.width; d.H = p.height;
    const double ty = tan(0.5 * p.fov_deg * M_PI / 180.0), tx = ty * p.width / p.height;
    double lv[3];
    for (int k = 0; k < 3; ++k) lv[k] = p.light_pos[k] - E[k];
    for (int k = 0; k < 3; ++k) {
        d.E[k] = (float)E[k]; d.f[k] = (float)f[k]; d.s[k] = (float)s[k]; d.u[k] = (float)u[k];
        d.lrgb[k] = (float)p.light_rgb[k];
    }
    d.light[0] = (float)rend_dot(s, lv); d.light[1] = (float)rend_dot(u, lv); d.light[2] = (float)rend_dot(f, lv);
    d.tx = (float)tx; d.ty = (float)ty;
    d.zn = (float)p.z_near; d.r = (float)p.radius; d.r2 = (float)(p.radius * p.radius);
    d.amb = (float)p.ambient;
    d.bg = (unsigned)p.background_rgb[0] | (unsigned)p.background_rgb[1] << 8 | (unsigned)p.background_rgb[2] << 16;
    d.box = (unsigned)p.box_rgb[0] | (unsigned)p.box_rgb[1] << 8 | (unsigned)p.box_rgb[2] << 16;
    d.draw_box = p.draw_box ? 1 : 0;
    for (int e = 0; e < 12; ++e) d.line_axis[e] = -1;
    if (d.draw_box) rend_lines(p, E, f, s, u, tx, ty, d);
    d.key = r->key; d.rgb = r->rgb; d.ids = r->ids; d.cnt = r->cnt;
    d.stream = r->stream;
    *out = r;
    return SPH_OK;
}

extern "C" void sph_render_destroy(SphRender *r) {
    if (!r) return;
    hipSetDevice(r->device);
    if (r->stream) hipStreamSynchronize(r->stream);
    for (void *b : {(void *)r->key, (void *)r->rgb, (void *)r->ids, (void *)r->cnt, (void *)r->pos, (void *)r->idv, (void *)r->large, (void *)r->col,
                    r->mvert, r->mnrm, r->mtri, r->mrec})
        if (b) hipFree(b);
    for (auto e_ : r->ev) if (e_) hipEventDestroy(e_);
    for (auto e_ : r->mev) if (e_) hipEventDestroy(e_);
    if (r->stream) hipStreamDestroy(r->stream);
    delete r;
}

extern "C" const char *sph_render_last_error(SphRender *r) { return r ? r->err.c_str() : g_create_error.c_str(); }

// room for n particles in the large list (and, points path, in the uploaded arrays)
static int rend_room(SphRender *r, size_t n, bool points) {
    if (n == 0) n = 1;
    if (r->cap_large < n) {
        if (r->large) { hipFree(r->large); r->large = nullptr; r->cap_large = 0; }
        RENDCHK(r, hipMalloc(&r->large, n * 4));
        r->cap_large = n;
    }
    if (points && r->cap_pts < n) {
        for (void **b : {(void **)&r->pos, (void **)&r->idv, (void **)&r->col}) if (*b) { hipFree(*b); *b = nullptr; }
        r->cap_pts = 0;
        RENDCHK(r, hipMalloc(&r->pos, n * sizeof(float4)));
        RENDCHK(r, hipMalloc(&r->idv, n * 4));
        RENDCHK(r, hipMalloc(&r->col, n * 4));
        r->cap_pts = n;
    }
    return SPH_OK;
}

// after the source is set in d and ev[0] recorded: clear, splat, shade; synchronous
static int rend_run(SphRender *r, int64_t n_in) {
    RenderDev &d = r->d;
    d.large = r->large;
    RENDCHK(r, hipMemsetAsync(r->key, 0xff, (size_t)d.W * d.H * 8, r->stream));
    RENDCHK(r, hipMemsetAsync(r->cnt, 0, 64, r->stream));
    RENDCHK(r, hipEventRecord(r->ev[1], r->stream));
    r->L->render_splat(d);
    RENDCHK(r, hipEventRecord(r->ev[2], r->stream));
    r->L->render_shade(d);
    RENDCHK(r, hipEventRecord(r->ev[3], r->stream));
    unsigned long long c[8];
    RENDCHK(r, hipMemcpyAsync(c, r->cnt, sizeof(c), hipMemcpyDeviceToHost, r->stream));
    RENDCHK(r, hipStreamSynchronize(r->stream));
    RENDCHK(r, hipGetLastError());
    SphRenderStats &o = r->stats;
    o.particles = n_in; o.drawn = (int64_t)c[0]; o.skipped_nonfinite = (int64_t)c[1]; o.large = (int64_t)c[2]; o.atomics = (int64_t)c[3];
    o.covered_pixels = (int64_t)c[4];
    o.ms_input = ev_ms(r->ev[0], r->ev[1]); o.ms_splat = ev_ms(r->ev[1], r->ev[2]); o.ms_shade = ev_ms(r->ev[2], r->ev[3]);
    o.ms_total = ev_ms(r->ev[0], r->ev[3]);
    r->have_frame = true;
    return SPH_OK;
}

extern "C" int sph_render_points(SphRender *r, const float *xyz, const uint8_t *rgb_or_NULL, const uint32_t *ids_or_NULL, int64_t n) {
    if (!r) return SPH_ERR_INVALID;
    if (n < 0 || n > INT_MAX / 2 || (n > 0 && !xyz)) return rend_fail(r, SPH_ERR_INVALID, "sph_render_points: bad particle array (n = %lld)", (long long)n);
    if (ids_or_NULL)
        for (int64_t i = 0; i < n; ++i)
            if (ids_or_NULL[i] >= RENDER_LINE_ID0) return rend_fail(r, SPH_ERR_INVALID, "sph_render_points: id %u >= 0xFFFFFFF0 (reserved)", ids_or_NULL[i]);
    RENDCHK(r, hipSetDevice(r->device));
    r->have_frame = false;
    r->stats = SphRenderStats{};
    { int rc = rend_room(r, (size_t)n, true); if (rc) return rc; }
    std::vector<float4> p4((size_t)n);
    std::vector<unsigned> id((size_t)n), col((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        p4[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0f);
        id[i] = ids_or_NULL ? ids_or_NULL[i] : (unsigned)i;
        col[i] = rgb_or_NULL ? (unsigned)rgb_or_NULL[3 * i] | (unsigned)rgb_or_NULL[3 * i + 1] << 8 | (unsigned)rgb_or_NULL[3 * i + 2] << 16 : 0xffffffu;
    }
    RENDCHK(r, hipEventRecord(r->ev[0], r->stream));
    if (n) {
        RENDCHK(r, hipMemcpyAsync(r->pos, p4.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, r->stream));
        RENDCHK(r, hipMemcpyAsync(r->idv, id.data(), 4 * (size_t)n, hipMemcpyHostToDevice, r->stream));
        RENDCHK(r, hipMemcpyAsync(r->col, col.data(), 4 * (size_t)n, hipMemcpyHostToDevice, r->stream));
    }
    RenderDev &d = r->d;
    d.n = (int)n; d.pos = r->pos; d.meta = nullptr; d.id = r->idv; d.col = r->col; d.col_home = nullptr; d.mask = ~0u;
    return rend_run(r, n);   // (the host vectors stay alive: rend_run synchronises)
}

extern "C" int sph_render_handle(SphRender *r, SphHandle *h, uint32_t object_mask) {
    if (!r || !h) return SPH_ERR_INVALID;
    if (h->st.slab_active || h->swap_axis)
        return rend_fail(r, SPH_ERR_UNSUPPORTED, "sph_render_handle: sharded handle (render each rank's download instead)");
    if (h->device != r->device) return rend_fail(r, SPH_ERR_INVALID, "sph_render_handle: handle on device %d, renderer on %d", h->device, r->device);
    if (h->in_step) return rend_fail(r, SPH_ERR_INVALID, "sph_render_handle: between sph_step_begin and sph_step_end");
    RENDCHK(r, hipSetDevice(r->device));
    r->have_frame = false;
    r->stats = SphRenderStats{};
    State &s = h->st;
    RenderDev &d = r->d;
    // colours as sph_download(SPH_F_COLOR) reads them: at home by particle id while the ids are the append order, else the sorted copy
    d.col_home = nullptr; d.col = nullptr;
    if (s.color_home && s.color_home_ok) d.col_home = s.color_home;
    else { h->L->ensure_color(s); d.col = s.color.cur(); }
    RENDCHK(r, hipStreamSynchronize(s.stream));   // the handle's last step has written the positions (and ensure_color the colours)
    const int n = h->n;
    { int rc = rend_room(r, (size_t)n, false); if (rc) return rc; }
    RENDCHK(r, hipEventRecord(r->ev[0], r->stream));
    d.n = n; d.pos = s.posv.cur(); d.meta = s.meta.cur(); d.id = s.pid.cur(); d.mask = object_mask;
    return rend_run(r, n);
}

extern "C" int sph_render_download(SphRender *r, uint8_t *rgb, int32_t *ids_or_NULL) {
    if (!r || !rgb) return SPH_ERR_INVALID;
    if (!r->have_frame) return rend_fail(r, SPH_ERR_INVALID, "sph_render_download: no frame has been rendered yet");
    RENDCHK(r, hipSetDevice(r->device));
    const size_t px = (size_t)r->d.W * r->d.H;
    RENDCHK(r, hipMemcpy(rgb, r->rgb, px * 3, hipMemcpyDeviceToHost));
    if (ids_or_NULL) RENDCHK(r, hipMemcpy(ids_or_NULL, r->ids, px * 4, hipMemcpyDeviceToHost));
    return SPH_OK;
}

extern "C" int sph_render_stats(SphRender *r, SphRenderStats *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    *out = r->stats;
    return SPH_OK;
}

// --- mesh frames: begin, add ..., end; the kernels are in sph_render_mesh.hpp ----------------------------------------------
extern "C" int sph_render_mesh_begin(SphRender *r) {
    if (!r) return SPH_ERR_INVALID;
    r->mesh_open = true;
    r->mesh_rec.clear();
    r->mesh_nv = r->mesh_nt = 0;
    return SPH_OK;
}

// room for `need` bytes in a list buffer whose first `used` bytes belong to earlier meshes of the frame (kept, as far as the buffer
// reaches: the normals buffer is grown for smooth meshes only, so the slots of flat meshes before them may lie beyond its end -- they are
// never read)
static int rend_grow(SphRender *r, void **buf, size_t *cap, size_t used, size_t need) {
    if (need <= *cap) return SPH_OK;
    const size_t ncap = std::max(need, *cap + *cap / 2);
    void *nb = nullptr;
    RENDCHK(r, hipMalloc(&nb, ncap));
    used = std::min(used, *cap);
    if (*buf && used) {
        hipError_t e_ = hipMemcpyAsync(nb, *buf, used, hipMemcpyDeviceToDevice, r->stream);
        if (e_ == hipSuccess) e_ = hipStreamSynchronize(r->stream);
        if (e_ != hipSuccess) { hipFree(nb); return rend_fail(r, SPH_ERR_HIP, "mesh list: copy failed: %s", hipGetErrorString(e_)); }
    }
    if (*buf) hipFree(*buf);
    *buf = nb;
    *cap = ncap;
    return SPH_OK;
}

// checks of one added mesh and room for it; the caller then copies into slots [mesh_nv, +nv) and triangles [mesh_nt, +nt)
static int rend_mesh_room(SphRender *r, const char *who, int64_t nv, int64_t nt, bool arrays_ok, bool normals, const uint8_t *rgb) {
    if (!r) return SPH_ERR_INVALID;
    if (!r->mesh_open) return rend_fail(r, SPH_ERR_INVALID, "%s: no sph_render_mesh_begin before it", who);
    if (nv < 0 || nt < 0 || !arrays_ok || !rgb) return rend_fail(r, SPH_ERR_INVALID, "%s: bad mesh arrays (nv = %lld, nt = %lld)", who, (long long)nv, (long long)nt);
    if (r->mesh_nv + nv > (int64_t)INT_MAX || r->mesh_nt + nt >= (int64_t)RENDER_LINE_ID0)
        return rend_fail(r, SPH_ERR_INVALID, "%s: the frame would hold %lld vertices (at most 2^31 - 1) and %lld triangles (below 0xFFFFFFF0)", who,
                         (long long)(r->mesh_nv + nv), (long long)(r->mesh_nt + nt));
    RENDCHK(r, hipSetDevice(r->device));
    int rc = rend_grow(r, &r->mvert, &r->cap_mvert, 12 * (size_t)r->mesh_nv, 12 * (size_t)(r->mesh_nv + nv));
    if (!rc) rc = rend_grow(r, &r->mtri, &r->cap_mtri, 12 * (size_t)r->mesh_nt, 12 * (size_t)(r->mesh_nt + nt));
    if (!rc && normals) rc = rend_grow(r, &r->mnrm, &r->cap_mnrm, 12 * (size_t)r->mesh_nv, 12 * (size_t)(r->mesh_nv + nv));
    return rc;
}

static void rend_mesh_push(SphRender *r, int64_t nv, int64_t nt, bool normals, const uint8_t *rgb) {
    MeshRec m{};
    m.t0 = r->mesh_nt; m.v0 = r->mesh_nv; m.nv = (int)nv;
    m.col = (unsigned)rgb[0] | (unsigned)rgb[1] << 8 | (unsigned)rgb[2] << 16;
    m.smooth = normals ? 1 : 0;
    r->mesh_rec.push_back(m);
    r->mesh_nv += nv;
    r->mesh_nt += nt;
}

static int rend_mesh_copy(SphRender *r, const void *vertices, const void *normals, const void *triangles, int64_t nv, int64_t nt, hipMemcpyKind kind) {
    if (nv) RENDCHK(r, hipMemcpyAsync((char *)r->mvert + 12 * (size_t)r->mesh_nv, vertices, 12 * (size_t)nv, kind, r->stream));
    if (nv && normals) RENDCHK(r, hipMemcpyAsync((char *)r->mnrm + 12 * (size_t)r->mesh_nv, normals, 12 * (size_t)nv, kind, r->stream));
    if (nt) RENDCHK(r, hipMemcpyAsync((char *)r->mtri + 12 * (size_t)r->mesh_nt, triangles, 12 * (size_t)nt, kind, r->stream));
    RENDCHK(r, hipStreamSynchronize(r->stream));   // the caller's arrays are free again
    return SPH_OK;
}

extern "C" int sph_render_mesh_add(SphRender *r, const float *vertices, const float *normals_or_NULL, const int32_t *triangles, int64_t nv,
                                   int64_t nt, const uint8_t rgb[3]) {
    const bool normals = normals_or_NULL != nullptr && nv > 0;
    int rc = rend_mesh_room(r, "sph_render_mesh_add", nv, nt, (nv == 0 || vertices) && (nt == 0 || triangles), normals, rgb);
    if (rc) return rc;
    rc = rend_mesh_copy(r, vertices, normals ? normals_or_NULL : nullptr, triangles, nv, nt, hipMemcpyHostToDevice);
    if (rc) return rc;
    rend_mesh_push(r, nv, nt, normals, rgb);
    return SPH_OK;
}

extern "C" int sph_render_mesh_add_surface(SphRender *r, SphSurface *s, const uint8_t rgb[3]) {
    if (!r || !s) return SPH_ERR_INVALID;
    if (!r->mesh_open) return rend_fail(r, SPH_ERR_INVALID, "sph_render_mesh_add_surface: no sph_render_mesh_begin before it");
    if (!s->have_mesh) return rend_fail(r, SPH_ERR_INVALID, "sph_render_mesh_add_surface: the surface object holds no mesh");
    if (s->device != r->device) return rend_fail(r, SPH_ERR_INVALID, "sph_render_mesh_add_surface: surface on device %d, renderer on %d", s->device, r->device);
    const int64_t nv = s->nv, nt = s->nt;
    const bool normals = s->prm.normals && s->d.nrm && nv > 0;
    int rc = rend_mesh_room(r, "sph_render_mesh_add_surface", nv, nt, true, normals, rgb);
    if (rc) return rc;
    RENDCHK(r, hipStreamSynchronize(s->stream));   // (the surface calls are synchronous: its mesh is complete)
    rc = rend_mesh_copy(r, s->d.vert, normals ? s->d.nrm : nullptr, s->d.tri, nv, nt, hipMemcpyDeviceToDevice);
    if (rc) return rc;
    rend_mesh_push(r, nv, nt, normals, rgb);
    return SPH_OK;
}

extern "C" int sph_render_mesh_end(SphRender *r) {
    if (!r) return SPH_ERR_INVALID;
    if (!r->mesh_open) return rend_fail(r, SPH_ERR_INVALID, "sph_render_mesh_end: no sph_render_mesh_begin before it");
    r->mesh_open = false;
    RENDCHK(r, hipSetDevice(r->device));
    r->have_frame = false;
    r->stats = SphRenderStats{};
    r->mstats = SphRenderMeshStats{};
    for (auto &ev_ : r->mev) if (!ev_) RENDCHK(r, hipEventCreate(&ev_));
    const size_t nm = r->mesh_rec.size();
    { int rc = rend_room(r, (size_t)r->mesh_nt, false); if (rc) return rc; }
    { int rc = rend_grow(r, &r->mrec, &r->cap_mrec, 0, sizeof(MeshRec) * std::max<size_t>(nm, 1)); if (rc) return rc; }
    RenderDev &d = r->d;
    MeshDev m{};
    m.nm = (int)nm; m.nt = r->mesh_nt;
    m.rec = (const MeshRec *)r->mrec; m.vert = (const float *)r->mvert; m.nrm = (const float *)r->mnrm; m.tri = (const int *)r->mtri;
    m.large = (unsigned *)r->large;
    d.n = 0; d.pos = nullptr; d.meta = nullptr; d.id = nullptr; d.col = nullptr; d.col_home = nullptr; d.large = r->large;
    RENDCHK(r, hipEventRecord(r->mev[0], r->stream));
    if (nm) RENDCHK(r, hipMemcpyAsync(r->mrec, r->mesh_rec.data(), sizeof(MeshRec) * nm, hipMemcpyHostToDevice, r->stream));
    RENDCHK(r, hipMemsetAsync(r->key, 0xff, (size_t)d.W * d.H * 8, r->stream));
    RENDCHK(r, hipMemsetAsync(r->cnt, 0, 64, r->stream));
    RENDCHK(r, hipEventRecord(r->mev[1], r->stream));
    r->L->render_mesh_depth(d, m);
    RENDCHK(r, hipEventRecord(r->mev[2], r->stream));
    r->L->render_mesh_shade(d, m);
    RENDCHK(r, hipEventRecord(r->mev[3], r->stream));
    r->L->render_mesh_finish(d);
    RENDCHK(r, hipEventRecord(r->mev[4], r->stream));
    unsigned long long c[8];
    RENDCHK(r, hipMemcpyAsync(c, r->cnt, sizeof(c), hipMemcpyDeviceToHost, r->stream));
    RENDCHK(r, hipStreamSynchronize(r->stream));
    RENDCHK(r, hipGetLastError());
    SphRenderMeshStats &o = r->mstats;
    o.meshes = (int64_t)nm; o.triangles = r->mesh_nt; o.vertices = r->mesh_nv;
    o.hit = (int64_t)c[0]; o.skipped_nonfinite = (int64_t)c[1]; o.large = (int64_t)c[2]; o.atomics = (int64_t)c[3];
    o.covered_pixels = (int64_t)c[4]; o.skipped_degenerate = (int64_t)c[5]; o.bad_index = (int64_t)c[6];
    o.ms_depth = ev_ms(r->mev[1], r->mev[2]); o.ms_shade = ev_ms(r->mev[2], r->mev[3]); o.ms_finish = ev_ms(r->mev[3], r->mev[4]);
    o.ms_total = ev_ms(r->mev[0], r->mev[4]);
    r->have_frame = true;
    if (o.bad_index)
        return rend_fail(r, SPH_ERR_INVALID, "sph_render_mesh_end: %lld triangle(s) with a vertex index outside their mesh (skipped; the frame holds the rest)",
                         (long long)o.bad_index);
    return SPH_OK;
}

extern "C" int sph_render_mesh_stats(SphRender *r, SphRenderMeshStats *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    *out = r->mstats;
    return SPH_OK;
}
