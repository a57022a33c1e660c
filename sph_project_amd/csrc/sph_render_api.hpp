// sph_render_api.hpp -- the SphRender object of include/sph_hip.h: camera set-up and box-line clipping in double, the frame buffers, the
// particle sources (host points, a live handle) and the stage marks.  Host code, included at the end of sph_api.hip; the kernels are in
// sph_render.hpp, the image is defined in DESIGN.md 15.
#pragma once
#include <climits>

// the frame buffers, the particle list (large: also the mesh frames' triangle list) and the mesh lists
// and an incoming layer; RB_S*: the planes of the surface mode, RB_T*: those of its thickness mode
// (DESIGN.md 25), each allocated when the mode is first used
enum RendBufId { RB_KEY, RB_RGB, RB_IDS, RB_CNT, RB_LARGE, RB_POS, RB_IDV, RB_COL, RB_MVERT, RB_MNRM, RB_MTRI, RB_MREC, RB_LKEY, RB_LRGB, RB_SBASE, RB_SQ0, RB_SQ1, RB_SCNT, RB_SMASK,
                 RB_TOKEY, RB_TORGB, RB_TOCNT, RB_TOLARGE, RB_TT0, RB_TT1, RB_TCNT,
                 RB_FID, RB_FCOL, RB_FCNT,   // ids, colours and counters of the diffuse particles' layer
                 RB_WFO, RB_WFU, RB_WDU, RB_WCNT, RB_WLARGE, RB_WNL, RB_WKEY0, RB_WRGB0,   // diffuse particles in the surface frames
                 RB_COUNT_ };

// what the renderer holds.  RF_ON_RANK0: the last frame was composited over a communicator and lies on rank 0, not here; RF_MESH: a mesh
// frame has no layer (triangle indices do not compose)
enum RendFrame { RF_NONE, RF_ON_RANK0, RF_PARTICLE, RF_MESH };

struct SphRender : DevObj {   // clk[0]: a particle frame's stages, clk[1]: a mesh frame's
    SphRenderParams prm;
    RenderDev d{};
    DevBuf buf[RB_COUNT_];
    RendFrame frame = RF_NONE;
    SphRenderStats stats{};
    SphRenderCompositeStats cstats{};
    // mesh frames: the list between mesh_begin and mesh_end, concatenated on the device
    bool mesh_open = false;
    std::vector<MeshRec> mesh_rec;
    int64_t mesh_nv = 0, mesh_nt = 0;
    SphRenderMeshStats mstats{};
    // surface mode: sclk marks 0 / 1 around the base plane, 2 / 3 / 4 quantise + smooth / shade
    bool surf_on = false;
    bool base_valid = false;      // the base plane belongs to the frame held (drawn with the mode on, not merged since)
    bool depth_valid = false;     // sph_render_surface has run on the frame held
    int depth_plane = 0;
    SphRenderSurfaceParams sprm{};
    RenderSurfDev sd{};
    StageClock sclk;
    std::vector<uint8_t> pmask;   // sph_render_points_surface_mask: for the next sph_render_points
    bool pmask_set = false;
    SphRenderSurfaceStats sstats{};
    // thickness mode: tclk marks 0 / 1 / 2 around the opaque layer and the splat, 3 / 4 / 5 smooth / composite
    bool thick_on = false;
    bool thick_valid = false;     // the opaque layer and the summed plane belong to the frame held
    bool thick_shaded = false;    // sph_render_surface has run on them
    const unsigned *thick_plane = nullptr;   // the smoothed plane of that call
    SphRenderThicknessParams tprm{};
    RenderThickDev td{};
    StageClock tclk;
    SphRenderThicknessStats tstats{};
    // diffuse particles (sph_render_set_foam in sph_foam_api.hpp): drawn by sph_render_handle while set
    struct SphFoam *foam = nullptr;
    double foam_scale = 0.5;
    unsigned foam_rgb[3] = {0, 0, 0};   // spray, foam, bubble
    // diffuse particles in the surface frames (sph_render_set_surface_foam in sph_foam_api.hpp): fclk marks 0 / 1 / 2 around
    // the splat and the raw spheres' merge, 3 / 4 around the composite
    struct SphFoam *sfoam = nullptr;
    SphRenderSurfaceFoamParams fprm{};
    RenderFoamDev fd{};
    bool from_handle = false;     // the frame held was drawn by sph_render_handle (the points path ignores the mode)
    bool sfoam_valid = false;     // the three planes belong to the frame held
    bool sfoam_thick = false;     // ... and were summed against the thickness mode's limits
    StageClock fclk;
    SphRenderSurfaceFoamStats fstats{};
    // traced mesh frames (sph_render_set_trace in sph_render_trace_api.hpp): set while the mode is on
    struct RendTrace *tr = nullptr;
};
static void rend_trace_free(SphRender *r);
static int rend_trace_end(SphRender *r, MeshDev &m);
static int rend_draw_foam(SphRender *r, struct SphFoam *f, double scale, const unsigned rgb[3]);
static int rend_surface_foam_check(SphRender *r, SphHandle *h);
static int rend_surface_foam_draw(SphRender *r);

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
    if (!params || !out) return fail(nullptr, SPH_ERR_INVALID, "sph_render_create: null argument");
    *out = nullptr;
    const SphRenderParams p = *params;
    if (p.width < 1 || p.height < 1 || p.width > 16384 || p.height > 16384 || (int64_t)p.width * p.height > ((int64_t)1 << 26))
        return fail(nullptr, SPH_ERR_INVALID, "sph_render_create: %d x %d pixels (each 1..16384, at most 2^26 in all)", p.width, p.height);
    if (!rend_finite3(p.eye) || !rend_finite3(p.target) || !rend_finite3(p.up) || !rend_finite3(p.light_pos) || !rend_finite3(p.light_rgb) ||
        !(p.fov_deg > 0.0 && p.fov_deg < 180.0) || !(p.z_near > 0.0) || !std::isfinite(p.z_near) || !(p.radius > 0.0) ||
        !std::isfinite(p.radius) || !(p.ambient >= 0.0) || !std::isfinite(p.ambient) || p.reserved != 0)
        return fail(nullptr, SPH_ERR_INVALID, "sph_render_create: camera, light, fov in (0, 180), z_near > 0, radius > 0 and ambient >= 0 must be finite");
    for (int k = 0; k < 3; ++k)
        if (p.background_rgb[k] < 0 || p.background_rgb[k] > 255 || p.box_rgb[k] < 0 || p.box_rgb[k] > 255)
            return fail(nullptr, SPH_ERR_INVALID, "sph_render_create: colours are 0..255");
    if (p.draw_box && (!rend_finite3(p.box_lo) || !rend_finite3(p.box_hi)))
        return fail(nullptr, SPH_ERR_INVALID, "sph_render_create: box corners must be finite");
    double E[3] = {p.eye[0], p.eye[1], p.eye[2]}, f[3], s[3], u[3];
    for (int k = 0; k < 3; ++k) f[k] = p.target[k] - E[k];
    if (!rend_normalize(f)) return fail(nullptr, SPH_ERR_INVALID, "sph_render_create: target equals eye");
    rend_cross(f, p.up, s);
    if (!rend_normalize(s)) return fail(nullptr, SPH_ERR_INVALID, "sph_render_create: up is parallel to the view direction");
    rend_cross(s, f, u);
    int dev = 0;
    { int rc = pick_device("sph_render_create", p.device, &dev); if (rc) return rc; }
    SphRender *r = new SphRender();
    r->prm = p;
    const size_t px = (size_t)p.width * p.height;
    DevBuf *b = r->buf;
    int rc = devobj_open(r, "sph_render_create", dev, p.fast_math);
    if (rc && !r->stream) { sph_render_destroy(r); return rc; }
    if (rc || b[RB_KEY].reserve(nullptr, px * 8) || b[RB_RGB].reserve(nullptr, px * 3) || b[RB_IDS].reserve(nullptr, px * 4) || b[RB_CNT].reserve(nullptr, 64)) {
        sph_render_destroy(r);
        return fail(nullptr, SPH_ERR_HIP, "sph_render_create: %zu pixels of frame buffers", px);
    }
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
    d.key = (unsigned long long *)b[RB_KEY].p; d.rgb = (unsigned char *)b[RB_RGB].p; d.ids = (int *)b[RB_IDS].p;
    d.cnt = (unsigned long long *)b[RB_CNT].p;
    d.stream = r->stream;
    *out = r;
    return SPH_OK;
}

extern "C" void sph_render_destroy(SphRender *r) {
    if (!r) return;
    hipSetDevice(r->device);
    if (r->stream) hipStreamSynchronize(r->stream);
    for (hipEvent_t e : r->sclk.ev) if (e) hipEventDestroy(e);
    for (hipEvent_t e : r->tclk.ev) if (e) hipEventDestroy(e);
    for (hipEvent_t e : r->fclk.ev) if (e) hipEventDestroy(e);
    rend_trace_free(r);
    devobj_close(r, r->buf, RB_COUNT_);
    delete r;
}

extern "C" const char *sph_render_last_error(SphRender *r) { return last_error(r); }

// room for n particles in the large list (and, points path, in the uploaded arrays)
static int rend_room(SphRender *r, size_t n, bool points) {
    if (n == 0) n = 1;
    int rc = r->buf[RB_LARGE].reserve(r, n * 4);
    if (!rc && points) rc = r->buf[RB_POS].reserve(r, n * sizeof(float4));
    if (!rc && points) rc = r->buf[RB_IDV].reserve(r, n * 4);
    if (!rc && points) rc = r->buf[RB_COL].reserve(r, n * 4);
    r->d.large = (int *)r->buf[RB_LARGE].p;
    return rc;
}

// the opening of a frame on the stream: no key in any pixel, the counters zero, stage mark k
static int rend_open(SphRender *r, StageClock &c, int k) {
    HIPCHK(r, hipMemsetAsync(r->d.key, 0xff, (size_t)r->d.W * r->d.H * 8, r->stream));
    HIPCHK(r, hipMemsetAsync(r->d.cnt, 0, 64, r->stream));
    HIPCHK(r, c.mark(k));
    return SPH_OK;
}
// the closing: the counters in c, the stream idle, the frame (of this kind) there
static int rend_close(SphRender *r, unsigned long long c[8], RendFrame kind) {
    HIPCHK(r, hipMemcpyAsync(c, r->d.cnt, 8 * sizeof(*c), hipMemcpyDeviceToHost, r->stream));
    HIPCHK(r, hipStreamSynchronize(r->stream));
    HIPCHK(r, hipGetLastError());
    r->frame = kind;
    return SPH_OK;
}

// surface mode: its planes, counters and clock on first use
static int rsurf_room(SphRender *r) {
    const size_t px = (size_t)r->d.W * r->d.H;
    DevBuf *b = r->buf;
    int rc = b[RB_SBASE].reserve(r, px * 4);
    if (!rc) rc = b[RB_SQ0].reserve(r, px * 4);
    if (!rc) rc = b[RB_SQ1].reserve(r, px * 4);
    if (!rc) rc = b[RB_SCNT].reserve(r, RSURF_CNT_BANKS * 64);
    if (rc) return rc;
    if (!r->sclk.stream) {
        for (hipEvent_t &e : r->sclk.ev) HIPCHK(r, hipEventCreate(&e));
        r->sclk.stream = r->stream;
    }
    RenderSurfDev &s = r->sd;
    s.base = (unsigned *)b[RB_SBASE].p; s.q[0] = (unsigned *)b[RB_SQ0].p; s.q[1] = (unsigned *)b[RB_SQ1].p;
    s.cnt = (unsigned long long *)b[RB_SCNT].p;
    return SPH_OK;
}

// thickness mode: the opaque layer, the thickness planes, counters and clock on first use; the large list follows the particle count
static int rthick_room(SphRender *r) {
    const size_t px = (size_t)r->d.W * r->d.H;
    DevBuf *b = r->buf;
    int rc = b[RB_TOKEY].reserve(r, px * 8);
    if (!rc) rc = b[RB_TORGB].reserve(r, px * 3);
    if (!rc) rc = b[RB_TOCNT].reserve(r, 64);
    if (!rc) rc = b[RB_TOLARGE].reserve(r, (size_t)std::max(r->d.n, 1) * 4);
    if (!rc) rc = b[RB_TT0].reserve(r, px * 4);
    if (!rc) rc = b[RB_TT1].reserve(r, px * 4);
    if (!rc) rc = b[RB_TCNT].reserve(r, 2 * RSURF_CNT_BANKS * 64);
    if (rc) return rc;
    if (!r->tclk.stream) {
        for (hipEvent_t &e : r->tclk.ev) HIPCHK(r, hipEventCreate(&e));
        r->tclk.stream = r->stream;
    }
    RenderThickDev &t = r->td;
    t.okey = (unsigned long long *)b[RB_TOKEY].p; t.orgb = (unsigned char *)b[RB_TORGB].p;
    t.ocnt = (unsigned long long *)b[RB_TOCNT].p; t.olarge = (int *)b[RB_TOLARGE].p;
    t.T[0] = (unsigned *)b[RB_TT0].p; t.T[1] = (unsigned *)b[RB_TT1].p;
    t.cnt = (unsigned long long *)b[RB_TCNT].p;
    return SPH_OK;
}

// the sum over the banks of counter group g
static int rthick_counters(SphRender *r, int g, unsigned long long c[8], bool max_word2) {
    unsigned long long bank[RSURF_CNT_BANKS][8];
    HIPCHK(r, hipMemcpyAsync(bank, r->td.cnt + (size_t)g * RSURF_CNT_BANKS * 8, sizeof(bank), hipMemcpyDeviceToHost, r->stream));
    HIPCHK(r, hipStreamSynchronize(r->stream));
    HIPCHK(r, hipGetLastError());
    for (int w = 0; w < 8; ++w) c[w] = 0;
    for (int b = 0; b < RSURF_CNT_BANKS; ++b)
        for (int w = 0; w < 8; ++w) c[w] = (max_word2 && w == 2) ? std::max(c[w], bank[b][w]) : c[w] + bank[b][w];
    return SPH_OK;
}

// after the source is set in d and stage mark 0 recorded: clear, splat, shade; synchronous
static int rend_run(SphRender *r, int64_t n_in) {
    RenderDev &d = r->d;
    StageClock &k = r->clk[0];
    const bool thick = r->surf_on && r->thick_on;
    r->thick_valid = r->thick_shaded = false;
    r->sfoam_valid = false;
    if (thick && n_in > (int64_t)RTHICK_MAX_PARTICLES) {
        HIPCHK(r, hipStreamSynchronize(r->stream));   // (the points path's uploads: the caller's vectors are free again)
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_set_thickness: %lld particles in the frame, a pixel's u32 thickness holds %d contributions",
                    (long long)n_in, RTHICK_MAX_PARTICLES);
    }
    { int rc = rend_open(r, k, 1); if (rc) return rc; }
    r->L->render_splat(d);
    HIPCHK(r, k.mark(2));
    r->L->render_shade(d);
    HIPCHK(r, k.mark(3));
    r->base_valid = r->depth_valid = false;
    if (r->surf_on) {   // the base plane, while the source is the one that was drawn
        { int rc = rsurf_room(r); if (rc) return rc; }
        HIPCHK(r, r->sclk.mark(0));
        r->L->render_surface_base(d, r->sd);
        HIPCHK(r, r->sclk.mark(1));
    }
    if (thick) {   // what lies behind the fluid, then the fluid along every ray: both need the source that was drawn
        { int rc = rthick_room(r); if (rc) return rc; }
        HIPCHK(r, r->tclk.mark(0));
        r->L->render_thick_opaque(d, r->sd, r->td);
        HIPCHK(r, r->tclk.mark(1));
        r->L->render_thick_splat(d, r->sd, r->td);
        HIPCHK(r, r->tclk.mark(2));
    }
    unsigned long long c[8];
    { int rc = rend_close(r, c, RF_PARTICLE); if (rc) return rc; }
    r->sstats = SphRenderSurfaceStats{};
    if (r->surf_on) { r->base_valid = true; r->sstats.ms_base = r->sclk.ms(0, 1); }
    r->tstats = SphRenderThicknessStats{};
    if (thick) {
        unsigned long long tc[8];
        { int rc = rthick_counters(r, 0, tc, false); if (rc) return rc; }
        r->thick_valid = true;
        r->tstats.adds = (int64_t)tc[0]; r->tstats.clipped = (int64_t)tc[1]; r->tstats.removed = (int64_t)tc[2];
        r->tstats.ms_opaque = r->tclk.ms(0, 1); r->tstats.ms_splat = r->tclk.ms(1, 2);
    }
    SphRenderStats &o = r->stats;
    o.particles = n_in; o.drawn = (int64_t)c[0]; o.skipped_nonfinite = (int64_t)c[1]; o.large = (int64_t)c[2]; o.atomics = (int64_t)c[3];
    o.covered_pixels = (int64_t)c[4];
    o.ms_input = k.ms(0, 1); o.ms_splat = k.ms(1, 2); o.ms_shade = k.ms(2, 3); o.ms_total = k.ms(0, 3);
    r->cstats = SphRenderCompositeStats{};
    r->cstats.ranks = 1; r->cstats.drawn_global = o.drawn;
    return SPH_OK;
}

// --- layers: the key and rgb planes of a particle frame, and another renderer's folded into this one ----------------------
static int rend_layer_room(SphRender *r) {
    const size_t px = (size_t)r->d.W * r->d.H;
    int rc = r->buf[RB_LKEY].reserve(r, px * 8);
    if (!rc) rc = r->buf[RB_LRGB].reserve(r, px * 3);
    return rc;
}

// the incoming layer (complete in RB_LKEY / RB_LRGB before the call) folded in on the renderer's stream
static void rend_merge_incoming(SphRender *r) {
    r->L->render_merge(r->d, (const unsigned long long *)r->buf[RB_LKEY].p, (const unsigned char *)r->buf[RB_LRGB].p);
}

// after merges: background, id image and the covered-pixel count of the merged frame; synchronous
static int rend_refinish(SphRender *r) {
    HIPCHK(r, hipMemsetAsync(r->d.cnt + 4, 0, sizeof(unsigned long long), r->stream));
    r->L->render_finish(r->d);
    unsigned long long c[8];
    { int rc = rend_close(r, c, RF_PARTICLE); if (rc) return rc; }
    r->stats.covered_pixels = (int64_t)c[4];
    return SPH_OK;
}

static int rend_layer_check(SphRender *r, const char *who) {
    if (r->frame == RF_ON_RANK0) return fail(r, SPH_ERR_INVALID, "%s: the composited frame lies on rank 0, this rank holds none", who);
    if (r->frame == RF_NONE) return fail(r, SPH_ERR_INVALID, "%s: no frame has been rendered yet", who);
    if (r->frame == RF_MESH) return fail(r, SPH_ERR_INVALID, "%s: the last frame is a mesh frame (triangle indices do not compose: layers are particle frames)", who);
    return SPH_OK;
}

extern "C" int sph_render_layer_download(SphRender *r, uint64_t *key, uint8_t *rgb) {
    if (!r || !key || !rgb) return SPH_ERR_INVALID;
    { int rc = rend_layer_check(r, "sph_render_layer_download"); if (rc) return rc; }
    HIPCHK(r, hipSetDevice(r->device));
    const size_t px = (size_t)r->d.W * r->d.H;
    HIPCHK(r, hipMemcpy(key, r->d.key, px * 8, hipMemcpyDeviceToHost));
    HIPCHK(r, hipMemcpy(rgb, r->d.rgb, px * 3, hipMemcpyDeviceToHost));
    return SPH_OK;
}

extern "C" int sph_render_layer_merge(SphRender *r, const uint64_t *key, const uint8_t *rgb) {
    if (!r || !key || !rgb) return SPH_ERR_INVALID;
    { int rc = rend_layer_check(r, "sph_render_layer_merge"); if (rc) return rc; }
    r->base_valid = r->depth_valid = false;   // (the merged pixels' colours and flags are not known here)
    r->thick_valid = r->thick_shaded = false;
    r->sfoam_valid = false;
    HIPCHK(r, hipSetDevice(r->device));
    { int rc = rend_layer_room(r); if (rc) return rc; }
    const size_t px = (size_t)r->d.W * r->d.H;
    HIPCHK(r, hipMemcpyAsync(r->buf[RB_LKEY].p, key, px * 8, hipMemcpyHostToDevice, r->stream));
    HIPCHK(r, hipMemcpyAsync(r->buf[RB_LRGB].p, rgb, px * 3, hipMemcpyHostToDevice, r->stream));
    rend_merge_incoming(r);
    return rend_refinish(r);   // (synchronous: the caller's arrays are free again)
}

extern "C" int sph_render_composite_stats(SphRender *r, SphRenderCompositeStats *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    *out = r->cstats;
    return SPH_OK;
}

// Sort-last compositing down the rank chain: this rank's frame is drawn (rend_run: the renderer's stream is idle).  Hop k
// moves the layer of rank nranks-1-k to rank nranks-2-k, which folds it into its own and passes the result on in hop k+1; rank 0 ends
// with the frame.  Transport: comm_exchange (mailboxes or RCCL send / recv on the handle's stream), pieces of at most the mailbox
// capacity out of / into the renderer's device buffers.  Every rank makes the same sequence of calls -- empty-handed where a hop is not
// its own -- which is what keeps the mailboxes' message numbers in step.  The two streams are ordered on the host: the renderer's is
// drained before the handle's stream (or the mailbox copy) reads its planes, the handle's (bounded) before the merge reads the incoming
// planes.
static int rend_composite(SphRender *r, SphHandle *h) {
    SlabComm &c = h->comm;
    SphRenderCompositeStats &cs = r->cstats;
    cs = SphRenderCompositeStats{};
    cs.ranks = c.nranks;
    r->frame = RF_NONE;   // (rend_run's: this rank's layer alone, not a frame before the chain is through)
    const size_t px = (size_t)r->d.W * r->d.H;
    const size_t plane[2] = {px * 8, px * 3};
    const size_t cap = c.kind == 2 ? (size_t)c.mbox_cap : ((size_t)16 << 20);
    if (cap == 0) return fail(r, SPH_ERR_COMM, "sph_render_handle: the communicator has no message capacity");
    if (c.nranks > 1) { int rc = rend_layer_room(r); if (rc) return rc; }
    bool started = false;   // stage mark 4: this rank's first exchange, 5: behind its last merge
    for (int hop = 0; hop < c.nranks - 1; ++hop) {
        const int src = c.nranks - 1 - hop, dst = src - 1;
        const bool sending = c.rank == src, receiving = c.rank == dst;
        if (c.kind == 1 && !sending && !receiving) continue;   // (RCCL send / recv carries no message numbers)
        if (sending || receiving) cs.hops += 1;
        char *out[2] = {(char *)r->d.key, (char *)r->d.rgb};
        char *in[2] = {(char *)r->buf[RB_LKEY].p, (char *)r->buf[RB_LRGB].p};
        if (!started) { HIPCHK(r, r->clk[0].mark(4)); started = true; }
        for (int pl = 0; pl < 2; ++pl)
            for (size_t off = 0; off < plane[pl]; off += cap) {
                const size_t nb = std::min(cap, plane[pl] - off);
                const void *send[2] = {sending ? out[pl] + off : nullptr, nullptr};       // down
                void *recv[2] = {nullptr, receiving ? in[pl] + off : nullptr};           // from above
                const size_t bs[2] = {sending ? nb : 0, 0};
                size_t br[2] = {0, receiving ? nb : 0};
                int rc = comm_exchange(h, send, bs, recv, br, true);
                if (!rc && c.kind == 1) rc = stream_sync_bounded(h, "layer exchange over RCCL");
                if (rc) return fail(r, rc, "sph_render_handle: layer exchange (hop %d): %s", hop, last_error(h));
                if (sending) { cs.pieces_sent += 1; cs.bytes_sent += (int64_t)nb; }
                if (receiving) { cs.pieces_recv += 1; cs.bytes_recv += (int64_t)nb; }
            }
        if (receiving) {
            rend_merge_incoming(r);
            HIPCHK(r, hipStreamSynchronize(r->stream));   // merged before the next hop reads the planes (or finish counts them)
        }
    }
    if (started) {
        HIPCHK(r, r->clk[0].mark(5));
        HIPCHK(r, hipStreamSynchronize(r->stream));
        cs.ms_composite = r->clk[0].ms(4, 5);
    }
    double drawn = (double)r->stats.drawn;
    { int rc = sph_comm_allreduce(h, &drawn, 1, 0); if (rc) return fail(r, rc, "sph_render_handle: %s", last_error(h)); }
    cs.drawn_global = (int64_t)drawn;
    if (c.rank != 0) { r->frame = RF_ON_RANK0; return SPH_OK; }
    if (c.nranks > 1) return rend_refinish(r);
    r->frame = RF_PARTICLE;
    return SPH_OK;
}

extern "C" int sph_render_points(SphRender *r, const float *xyz, const uint8_t *rgb_or_NULL, const uint32_t *ids_or_NULL, int64_t n) {
    if (!r) return SPH_ERR_INVALID;
    if (n < 0 || n > INT_MAX / 2 || (n > 0 && !xyz)) return fail(r, SPH_ERR_INVALID, "sph_render_points: bad particle array (n = %lld)", (long long)n);
    if (ids_or_NULL)
        for (int64_t i = 0; i < n; ++i)
            if (ids_or_NULL[i] >= RENDER_LINE_ID0) return fail(r, SPH_ERR_INVALID, "sph_render_points: id %u >= 0xFFFFFFF0 (reserved)", ids_or_NULL[i]);
    if (r->pmask_set && (int64_t)r->pmask.size() != n) {
        const size_t nm = r->pmask.size();
        r->pmask_set = false; r->pmask.clear();   // (the mask was for this call)
        return fail(r, SPH_ERR_INVALID, "sph_render_points: surface mask of %zu points, %lld particles", nm, (long long)n);
    }
    HIPCHK(r, hipSetDevice(r->device));
    r->frame = RF_NONE;
    r->from_handle = false;
    r->stats = SphRenderStats{};
    { int rc = rend_room(r, (size_t)n, true); if (rc) return rc; }
    std::vector<float4> p4((size_t)n);
    std::vector<unsigned> id((size_t)n), col((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        p4[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0f);
        id[i] = ids_or_NULL ? ids_or_NULL[i] : (unsigned)i;
        col[i] = rgb_or_NULL ? (unsigned)rgb_or_NULL[3 * i] | (unsigned)rgb_or_NULL[3 * i + 1] << 8 | (unsigned)rgb_or_NULL[3 * i + 2] << 16 : 0xffffffu;
    }
    void *pos = r->buf[RB_POS].p, *idv = r->buf[RB_IDV].p, *colv = r->buf[RB_COL].p;
    HIPCHK(r, r->clk[0].mark(0));
    if (n) {
        HIPCHK(r, hipMemcpyAsync(pos, p4.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, r->stream));
        HIPCHK(r, hipMemcpyAsync(idv, id.data(), 4 * (size_t)n, hipMemcpyHostToDevice, r->stream));
        HIPCHK(r, hipMemcpyAsync(colv, col.data(), 4 * (size_t)n, hipMemcpyHostToDevice, r->stream));
    }
    RenderDev &d = r->d;
    d.n = (int)n; d.pos = (const float4 *)pos; d.meta = nullptr; d.id = (const int *)idv; d.col = (const unsigned *)colv; d.col_home = nullptr; d.mask = ~0u;
    r->sd.pmask = nullptr;
    if (r->pmask_set && r->surf_on && n) {
        { int rc = r->buf[RB_SMASK].reserve(r, (size_t)n); if (rc) return rc; }
        HIPCHK(r, hipMemcpyAsync(r->buf[RB_SMASK].p, r->pmask.data(), (size_t)n, hipMemcpyHostToDevice, r->stream));
        r->sd.pmask = (const unsigned char *)r->buf[RB_SMASK].p;
    }
    const int rc = rend_run(r, n);   // (the host vectors stay alive: rend_run synchronises)
    r->pmask_set = false; r->pmask.clear();
    return rc;
}

extern "C" int sph_render_handle(SphRender *r, SphHandle *h, uint32_t object_mask) {
    if (!r || !h) return SPH_ERR_INVALID;
    if (h->swap_axis)
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_handle: the handle's library frame is a permutation of the scene's (SPH_SLAB_LAYOUT=slow): not rendered");
    if (h->device != r->device) return fail(r, SPH_ERR_INVALID, "sph_render_handle: handle on device %d, renderer on %d", h->device, r->device);
    if (h->in_step) return fail(r, SPH_ERR_INVALID, "sph_render_handle: between sph_step_begin and sph_step_end");
    if (r->foam && (r->surf_on || h->st.slab_active))
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_handle: diffuse particles are set (sph_render_set_foam): no surface mode, no sharded handle");
    if (r->foam && (int64_t)h->st.cap > (int64_t)INT_MAX)
        return fail(r, SPH_ERR_INVALID, "sph_render_handle: particle ids reach 2^31, diffuse ids could not be told from them");
    if (r->sfoam) { int rc = rend_surface_foam_check(r, h); if (rc) return rc; }
    HIPCHK(r, hipSetDevice(r->device));
    r->frame = RF_NONE;
    r->stats = SphRenderStats{};
    State &s = h->st;
    RenderDev &d = r->d;
    const bool sharded = s.slab_active != 0;
    if (sharded && !h->n_exact) {   // asynchronous steps are settled first, as sph_synchronize does
        HIPCHK(r, hipSetDevice(h->device));
        const int rc = slab_settle(h);
        if (rc) return fail(r, rc, "sph_render_handle: %s", last_error(h));
    }
    // colours as sph_download(SPH_F_COLOR) reads them: at home by particle id while the ids are the append order, else the sorted copy
    d.col_home = nullptr; d.col = nullptr;
    if (s.color_home && s.color_home_ok) d.col_home = s.color_home;
    else d.col = h->L->sorted_color(s);
    HIPCHK(r, hipStreamSynchronize(s.stream));   // the handle's last step has written the positions (and sorted_color the colours)
    const int n = h->n;
    { int rc = rend_room(r, (size_t)n, false); if (rc) return rc; }
    HIPCHK(r, r->clk[0].mark(0));
    d.n = n; d.pos = s.posv.cur(); d.meta = s.meta.cur(); d.id = s.pid.cur(); d.mask = object_mask;
    { int rc = rend_run(r, n); if (rc) return rc; }
    r->from_handle = true;
    if (r->foam) return rend_draw_foam(r, r->foam, r->foam_scale, r->foam_rgb);
    if (r->sfoam) return rend_surface_foam_draw(r);   // (never with a sharded handle: rend_surface_foam_check)
    if (!sharded) return SPH_OK;
    return rend_composite(r, h);   // collective: every rank of the communicator is here with the same renderer parameters and mask
}

extern "C" int sph_render_download(SphRender *r, uint8_t *rgb, int32_t *ids_or_NULL) {
    if (!r || !rgb) return SPH_ERR_INVALID;
    if (r->frame == RF_ON_RANK0) return fail(r, SPH_ERR_INVALID, "sph_render_download: the composited frame lies on rank 0, this rank holds none");
    if (r->frame == RF_NONE) return fail(r, SPH_ERR_INVALID, "sph_render_download: no frame has been rendered yet");
    HIPCHK(r, hipSetDevice(r->device));
    const size_t px = (size_t)r->d.W * r->d.H;
    HIPCHK(r, hipMemcpy(rgb, r->d.rgb, px * 3, hipMemcpyDeviceToHost));
    if (ids_or_NULL) HIPCHK(r, hipMemcpy(ids_or_NULL, r->d.ids, px * 4, hipMemcpyDeviceToHost));
    return SPH_OK;
}

// the frame held, for an object on `device` that reads w x h pixels of it in place (an encoder; `o` takes its message, `who` names its
// call): the checks, the renderer's stream drained (the render calls are synchronous: the frame is complete), the rgb plane
static int rend_frame_rgb(SphRender *r, int w, int h, int device, ErrSink *o, const char *who, const unsigned char **rgb) {
    if (r->frame != RF_PARTICLE && r->frame != RF_MESH) return fail(o, SPH_ERR_INVALID, "%s: the renderer holds no frame", who);
    if (r->d.W != w || r->d.H != h)
        return fail(o, SPH_ERR_INVALID, "%s: the renderer's frame is %d x %d, the encoder's %d x %d", who, r->d.W, r->d.H, w, h);
    if (r->device != device) return fail(o, SPH_ERR_INVALID, "%s: renderer on device %d, encoder on %d", who, r->device, device);
    HIPCHK(o, hipSetDevice(device));
    HIPCHK(o, hipStreamSynchronize(r->stream));
    *rgb = r->d.rgb;
    return SPH_OK;
}

extern "C" int sph_render_stats(SphRender *r, SphRenderStats *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    *out = r->stats;
    return SPH_OK;
}

// --- surface mode: the kernels are in sph_render_surface.hpp ---------------------------------------------------------------
extern "C" int sph_render_set_surface(SphRender *r, const SphRenderSurfaceParams *params) {
    if (!r) return SPH_ERR_INVALID;
    if (!params) { r->surf_on = r->thick_on = false; r->sfoam = nullptr; r->sfoam_valid = false; return SPH_OK; }
    const SphRenderSurfaceParams p = *params;
    if (p.iterations < 0 || p.iterations > 64) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface: iterations %d outside 0..64", p.iterations);
    if (p.rmax < 1 || p.rmax > RSURF_RMAX_CAP) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface: rmax %d outside 1..%d", p.rmax, RSURF_RMAX_CAP);
    if (!(p.sigma > 0.0) || !std::isfinite(p.sigma)) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface: sigma %g must be finite and positive", p.sigma);
    if (!(p.range > 0.0) || !std::isfinite(p.range)) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface: range %g must be finite and positive", p.range);
    if (!(p.spec >= 0.0) || !std::isfinite(p.spec)) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface: spec %g must be finite and not negative", p.spec);
    if (!(p.shininess >= 1.0) || !std::isfinite(p.shininess)) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface: shininess %g must be finite and at least 1", p.shininess);
    if (p.object_mask < -1 || p.object_mask > (int64_t)0xFFFFFFFFll)
        return fail(r, SPH_ERR_INVALID, "sph_render_set_surface: object_mask %lld is neither -1 nor a mask of the 32 objects", (long long)p.object_mask);
    const double ty = tan(0.5 * r->prm.fov_deg * M_PI / 180.0), tx = ty * r->prm.width / r->prm.height;
    const double rnum = std::round(256.0 * p.sigma * r->prm.height / (2.0 * ty)), dq = std::round(256.0 * p.range);
    if (!(rnum < 2147483648.0)) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface: sigma %g gives a window numerator of %.0f (below 2^31)", p.sigma, rnum);
    if (!(dq >= 1.0 && dq <= 16777216.0)) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface: range %g gives a depth range of %.0f units (1..2^24)", p.range, dq);
    RenderSurfDev &s = r->sd;
    const unsigned omask = p.object_mask < 0 ? ~0u : (unsigned)p.object_mask;
    const int fluid_only = p.object_mask < 0 ? 1 : 0;
    if (!r->surf_on || omask != s.omask || fluid_only != s.fluid_only)   // the frame held has no base plane (or thickness) for this mask
        r->base_valid = r->thick_valid = r->thick_shaded = r->sfoam_valid = false;
    s.omask = omask; s.fluid_only = fluid_only;
    s.inv_u = (float)(256.0 / (double)r->d.r);
    s.u = (float)((double)r->d.r / 256.0);
    s.rnum = (unsigned)rnum; s.dq = (unsigned)dq; s.rmax = p.rmax;
    s.dX = (float)(2.0 * tx / r->prm.width); s.dY = (float)(-2.0 * ty / r->prm.height);
    s.spec = (float)p.spec; s.shin = (float)p.shininess;
    r->sprm = p;
    r->surf_on = true;
    return SPH_OK;
}

extern "C" int sph_render_points_surface_mask(SphRender *r, const uint8_t *mask, int n) {
    if (!r) return SPH_ERR_INVALID;
    if (n < 0) return fail(r, SPH_ERR_INVALID, "sph_render_points_surface_mask: n = %d", n);
    r->pmask_set = mask != nullptr;
    r->pmask.clear();
    if (mask) r->pmask.assign(mask, mask + n);
    return SPH_OK;
}

extern "C" int sph_render_surface(SphRender *r) {
    if (!r) return SPH_ERR_INVALID;
    if (r->frame == RF_ON_RANK0 || (r->frame == RF_PARTICLE && r->cstats.ranks > 1))
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_surface: the frame was composited from a sharded handle (its layers carry no base colour or surface flag)");
    if (r->frame == RF_NONE) return fail(r, SPH_ERR_INVALID, "sph_render_surface: no particle frame has been rendered yet");
    if (r->frame == RF_MESH) return fail(r, SPH_ERR_INVALID, "sph_render_surface: the last frame is a mesh frame");
    if (!r->surf_on) return fail(r, SPH_ERR_INVALID, "sph_render_surface: the surface mode is off (sph_render_set_surface)");
    if (!r->base_valid)
        return fail(r, SPH_ERR_INVALID, "sph_render_surface: the frame held was drawn before the mode was switched on, or changed by sph_render_layer_merge");
    if (r->thick_on && !r->thick_valid)
        return fail(r, SPH_ERR_INVALID, "sph_render_surface: the frame held was drawn before the thickness mode was switched on (sph_render_set_thickness)");
    const bool wfoam = r->sfoam && r->from_handle;   // diffuse particles over and under the surface
    if (wfoam && !r->sfoam_valid)
        return fail(r, SPH_ERR_INVALID, "sph_render_surface: the frame held was drawn before the diffuse particles were set (sph_render_set_surface_foam)");
    if (wfoam && r->sfoam_thick != r->thick_on)
        return fail(r, SPH_ERR_INVALID, "sph_render_surface: the thickness mode was switched after the frame held was drawn with diffuse particles "
                                        "(sph_render_set_surface_foam): its planes were summed against the other limits");
    HIPCHK(r, hipSetDevice(r->device));
    RenderDev &d = r->d;
    RenderSurfDev &s = r->sd;
    StageClock &k = r->sclk;
    const int iters = r->sprm.iterations;
    r->depth_valid = false;
    HIPCHK(r, hipMemsetAsync(s.cnt, 0, RSURF_CNT_BANKS * 64, r->stream));
    HIPCHK(r, k.mark(2));
    RenderDev dq = d;   // what the quantise pass reads: the frame's key plane, or its copy from before the raw spheres were merged in
    if (wfoam) {
        HIPCHK(r, hipMemcpyAsync(d.rgb, r->buf[RB_WRGB0].p, (size_t)d.W * d.H * 3, hipMemcpyDeviceToDevice, r->stream));   // a repeat starts from the frame
        dq.key = (unsigned long long *)r->fd.key0;
    }
    r->L->render_surface_quantise(dq, s);
    for (int it = 0; it < iters; ++it) r->L->render_surface_smooth(d, s, it);
    HIPCHK(r, k.mark(3));
    r->depth_plane = iters & 1;
    const bool thick = r->thick_on;
    const int titers = r->tprm.iterations;
    r->thick_shaded = false;
    if (thick) {
        // T[0] -> T[1] -> the idle depth plane -> T[1] ...: the summed plane stays as it is, a repeated call starts from it again
        RenderThickDev &t = r->td;
        const unsigned *Q = s.q[r->depth_plane];
        unsigned *pong[2] = {t.T[1], s.q[1 - r->depth_plane]};
        const unsigned *in = t.T[0];
        HIPCHK(r, hipMemsetAsync(t.cnt + (size_t)RSURF_CNT_BANKS * 8, 0, RSURF_CNT_BANKS * 64, r->stream));   // group 1
        HIPCHK(r, r->tclk.mark(3));
        for (int it = 0; it < titers; ++it) {
            r->L->render_thick_smooth(d, s, t, Q, in, pong[it & 1]);
            in = pong[it & 1];
        }
        HIPCHK(r, r->tclk.mark(4));
        r->L->render_thick_shade(d, s, t, Q, in);
        HIPCHK(r, r->tclk.mark(5));
        r->thick_plane = in;
    } else
        r->L->render_surface_shade(d, s, r->depth_plane);
    HIPCHK(r, k.mark(4));
    if (wfoam) {
        HIPCHK(r, r->fclk.mark(3));
        if (thick) r->L->render_foam_under(d, s, r->td, r->fd, s.q[r->depth_plane], r->thick_plane);
        r->L->render_foam_over(d, r->fd);
        HIPCHK(r, r->fclk.mark(4));
    }
    unsigned long long bank[RSURF_CNT_BANKS][8], c[8] = {};
    HIPCHK(r, hipMemcpyAsync(bank, s.cnt, sizeof(bank), hipMemcpyDeviceToHost, r->stream));
    HIPCHK(r, hipStreamSynchronize(r->stream));
    HIPCHK(r, hipGetLastError());
    for (int b = 0; b < RSURF_CNT_BANKS; ++b)
        for (int w = 0; w < 8; ++w) c[w] += bank[b][w];
    r->depth_valid = true;
    SphRenderSurfaceStats &o = r->sstats;
    o.surface_pixels = (int64_t)c[0]; o.iterations = iters; o.taps_visited = (int64_t)c[1]; o.taps_accepted = (int64_t)c[2];
    o.clamped_rmax = (int64_t)c[3];
    o.ms_smooth = k.ms(2, 3); o.ms_shade = k.ms(3, 4);
    if (thick) {
        unsigned long long tc[8];
        { int rc = rthick_counters(r, 1, tc, true); if (rc) return rc; }
        r->thick_shaded = true;
        SphRenderThicknessStats &ts = r->tstats;
        ts.iterations = titers; ts.taps_visited = (int64_t)tc[0]; ts.empty_pixels = (int64_t)tc[1]; ts.max_thickness = (int64_t)tc[2];
        ts.ms_smooth = r->tclk.ms(3, 4); ts.ms_shade = r->tclk.ms(4, 5);
    }
    if (wfoam) {
        HIPCHK(r, hipMemcpy(bank, r->fd.cnt + (size_t)RSURF_CNT_BANKS * 8, sizeof(bank), hipMemcpyDeviceToHost));   // group 1 (the stream is idle)
        int64_t po = 0, pu = 0;
        for (int b = 0; b < RSURF_CNT_BANKS; ++b) { po += (int64_t)bank[b][0]; pu += (int64_t)bank[b][1]; }
        r->fstats.pixels_over = po; r->fstats.pixels_under = pu;
        r->fstats.ms_composite = r->fclk.ms(3, 4);
    }
    return SPH_OK;
}

// --- thickness mode of the surface frames: the kernels are in sph_render_thickness.hpp -------------------------------------
extern "C" int sph_render_set_thickness(SphRender *r, const SphRenderThicknessParams *params) {
    if (!r) return SPH_ERR_INVALID;
    if (!params) { r->thick_on = false; return SPH_OK; }
    const SphRenderThicknessParams p = *params;
    if (!r->surf_on) return fail(r, SPH_ERR_INVALID, "sph_render_set_thickness: the surface mode is off (sph_render_set_surface)");
    if (!(p.absorb >= 0.0f) || !std::isfinite(p.absorb)) return fail(r, SPH_ERR_INVALID, "sph_render_set_thickness: absorb %g must be finite and not negative", (double)p.absorb);
    if (!(p.scatter >= 0.0f) || !std::isfinite(p.scatter)) return fail(r, SPH_ERR_INVALID, "sph_render_set_thickness: scatter %g must be finite and not negative", (double)p.scatter);
    if (p.iterations < 0 || p.iterations > 64) return fail(r, SPH_ERR_INVALID, "sph_render_set_thickness: iterations %d outside 0..64", p.iterations);
    if (!r->thick_on) r->thick_valid = r->thick_shaded = false;   // the frame held has no opaque layer and no thickness
    r->td.absorb = p.absorb; r->td.scatter = p.scatter;
    r->tprm = p;
    r->thick_on = true;
    return SPH_OK;
}

static int rthick_held(SphRender *r, const char *who, bool shaded) {
    if (r->frame != RF_PARTICLE || !r->thick_valid || (shaded && !r->thick_shaded))
        return fail(r, SPH_ERR_INVALID, "%s: no surface frame with thickness is held (sph_render_set_thickness, a particle frame, sph_render_surface)", who);
    return SPH_OK;
}

extern "C" int sph_render_surface_download_thickness(SphRender *r, uint32_t *T, int raw) {
    if (!r || !T) return SPH_ERR_INVALID;
    { int rc = rthick_held(r, "sph_render_surface_download_thickness", true); if (rc) return rc; }
    HIPCHK(r, hipSetDevice(r->device));
    const size_t px = (size_t)r->d.W * r->d.H;
    HIPCHK(r, hipMemcpy(T, raw ? r->td.T[0] : r->thick_plane, px * 4, hipMemcpyDeviceToHost));
    if (raw) return SPH_OK;
    std::vector<uint32_t> q(px);   // the smoothing writes surface pixels only: the rest is 0 by definition
    HIPCHK(r, hipMemcpy(q.data(), r->sd.q[r->depth_plane], px * 4, hipMemcpyDeviceToHost));
    for (size_t p = 0; p < px; ++p)
        if (q[p] == RSURF_SENT) T[p] = 0;
    return SPH_OK;
}

extern "C" int sph_render_surface_download_opaque(SphRender *r, uint64_t *key, uint8_t *rgb) {
    if (!r || !key || !rgb) return SPH_ERR_INVALID;
    { int rc = rthick_held(r, "sph_render_surface_download_opaque", false); if (rc) return rc; }
    HIPCHK(r, hipSetDevice(r->device));
    const size_t px = (size_t)r->d.W * r->d.H;
    HIPCHK(r, hipMemcpy(key, r->td.okey, px * 8, hipMemcpyDeviceToHost));
    HIPCHK(r, hipMemcpy(rgb, r->td.orgb, px * 3, hipMemcpyDeviceToHost));
    return SPH_OK;
}

extern "C" int sph_render_thickness_stats(SphRender *r, SphRenderThicknessStats *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    *out = r->tstats;
    return SPH_OK;
}

extern "C" int sph_render_surface_download_depth(SphRender *r, uint32_t *q) {
    if (!r || !q) return SPH_ERR_INVALID;
    if (r->frame != RF_PARTICLE || !r->depth_valid) return fail(r, SPH_ERR_INVALID, "sph_render_surface_download_depth: no surface frame is held (sph_render_surface)");
    HIPCHK(r, hipSetDevice(r->device));
    HIPCHK(r, hipMemcpy(q, r->sd.q[r->depth_plane], (size_t)r->d.W * r->d.H * 4, hipMemcpyDeviceToHost));
    return SPH_OK;
}

extern "C" int sph_render_surface_stats(SphRender *r, SphRenderSurfaceStats *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    *out = r->sstats;
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
static int rend_grow(SphRender *r, int k, size_t used, size_t need) {
    DevBuf &b = r->buf[k];
    if (need <= b.bytes) return SPH_OK;
    return b.reserve(r, std::max(need, b.bytes + b.bytes / 2), used, r->stream);
}

// checks of one added mesh and room for it; the caller then copies into slots [mesh_nv, +nv) and triangles [mesh_nt, +nt)
static int rend_mesh_room(SphRender *r, const char *who, int64_t nv, int64_t nt, bool arrays_ok, bool normals, const uint8_t *rgb) {
    if (!r) return SPH_ERR_INVALID;
    if (!r->mesh_open) return fail(r, SPH_ERR_INVALID, "%s: no sph_render_mesh_begin before it", who);
    if (nv < 0 || nt < 0 || !arrays_ok || !rgb) return fail(r, SPH_ERR_INVALID, "%s: bad mesh arrays (nv = %lld, nt = %lld)", who, (long long)nv, (long long)nt);
    if (r->mesh_nv + nv > (int64_t)INT_MAX || r->mesh_nt + nt >= (int64_t)RENDER_LINE_ID0)
        return fail(r, SPH_ERR_INVALID, "%s: the frame would hold %lld vertices (at most 2^31 - 1) and %lld triangles (below 0xFFFFFFF0)", who,
                         (long long)(r->mesh_nv + nv), (long long)(r->mesh_nt + nt));
    HIPCHK(r, hipSetDevice(r->device));
    int rc = rend_grow(r, RB_MVERT, 12 * (size_t)r->mesh_nv, 12 * (size_t)(r->mesh_nv + nv));
    if (!rc) rc = rend_grow(r, RB_MTRI, 12 * (size_t)r->mesh_nt, 12 * (size_t)(r->mesh_nt + nt));
    if (!rc && normals) rc = rend_grow(r, RB_MNRM, 12 * (size_t)r->mesh_nv, 12 * (size_t)(r->mesh_nv + nv));
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
    if (nv) HIPCHK(r, hipMemcpyAsync((char *)r->buf[RB_MVERT].p + 12 * (size_t)r->mesh_nv, vertices, 12 * (size_t)nv, kind, r->stream));
    if (nv && normals) HIPCHK(r, hipMemcpyAsync((char *)r->buf[RB_MNRM].p + 12 * (size_t)r->mesh_nv, normals, 12 * (size_t)nv, kind, r->stream));
    if (nt) HIPCHK(r, hipMemcpyAsync((char *)r->buf[RB_MTRI].p + 12 * (size_t)r->mesh_nt, triangles, 12 * (size_t)nt, kind, r->stream));
    HIPCHK(r, hipStreamSynchronize(r->stream));   // the caller's arrays are free again
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
    if (!r->mesh_open) return fail(r, SPH_ERR_INVALID, "sph_render_mesh_add_surface: no sph_render_mesh_begin before it");
    if (!s->have_mesh) return fail(r, SPH_ERR_INVALID, "sph_render_mesh_add_surface: the surface object holds no mesh");
    if (s->device != r->device) return fail(r, SPH_ERR_INVALID, "sph_render_mesh_add_surface: surface on device %d, renderer on %d", s->device, r->device);
    const int64_t nv = s->nv, nt = s->nt;
    const bool normals = s->prm.normals && s->d.nrm && nv > 0;
    int rc = rend_mesh_room(r, "sph_render_mesh_add_surface", nv, nt, true, normals, rgb);
    if (rc) return rc;
    HIPCHK(r, hipStreamSynchronize(s->stream));   // (the surface calls are synchronous: its mesh is complete)
    rc = rend_mesh_copy(r, s->d.vert, normals ? s->d.nrm : nullptr, s->d.tri, nv, nt, hipMemcpyDeviceToDevice);
    if (rc) return rc;
    rend_mesh_push(r, nv, nt, normals, rgb);
    return SPH_OK;
}

extern "C" int sph_render_mesh_end(SphRender *r) {
    if (!r) return SPH_ERR_INVALID;
    if (!r->mesh_open) return fail(r, SPH_ERR_INVALID, "sph_render_mesh_end: no sph_render_mesh_begin before it");
    r->mesh_open = false;
    HIPCHK(r, hipSetDevice(r->device));
    r->frame = RF_NONE;
    r->stats = SphRenderStats{};
    r->cstats = SphRenderCompositeStats{};
    r->mstats = SphRenderMeshStats{};
    r->base_valid = r->depth_valid = r->thick_valid = r->thick_shaded = false;
    const size_t nm = r->mesh_rec.size();
    { int rc = rend_room(r, (size_t)r->mesh_nt, false); if (rc) return rc; }
    { int rc = rend_grow(r, RB_MREC, 0, sizeof(MeshRec) * std::max<size_t>(nm, 1)); if (rc) return rc; }
    RenderDev &d = r->d;
    StageClock &k = r->clk[1];
    MeshDev m{};
    m.nm = (int)nm; m.nt = r->mesh_nt;
    m.rec = (const MeshRec *)r->buf[RB_MREC].p; m.vert = (const float *)r->buf[RB_MVERT].p; m.nrm = (const float *)r->buf[RB_MNRM].p;
    m.tri = (const int *)r->buf[RB_MTRI].p;
    m.large = (unsigned *)d.large;
    d.n = 0; d.pos = nullptr; d.meta = nullptr; d.id = nullptr; d.col = nullptr; d.col_home = nullptr;
    HIPCHK(r, k.mark(0));
    if (nm) HIPCHK(r, hipMemcpyAsync(r->buf[RB_MREC].p, r->mesh_rec.data(), sizeof(MeshRec) * nm, hipMemcpyHostToDevice, r->stream));
    if (r->tr) { HIPCHK(r, k.mark(1)); return rend_trace_end(r, m); }   // the mode is on: the traced frame instead
    { int rc = rend_open(r, k, 1); if (rc) return rc; }
    r->L->render_mesh_depth(d, m);
    HIPCHK(r, k.mark(2));
    r->L->render_mesh_shade(d, m);
    HIPCHK(r, k.mark(3));
    r->L->render_mesh_finish(d);
    HIPCHK(r, k.mark(4));
    unsigned long long c[8];
    { int rc = rend_close(r, c, RF_MESH); if (rc) return rc; }
    SphRenderMeshStats &o = r->mstats;
    o.meshes = (int64_t)nm; o.triangles = r->mesh_nt; o.vertices = r->mesh_nv;
    o.hit = (int64_t)c[0]; o.skipped_nonfinite = (int64_t)c[1]; o.large = (int64_t)c[2]; o.atomics = (int64_t)c[3];
    o.covered_pixels = (int64_t)c[4]; o.skipped_degenerate = (int64_t)c[5]; o.bad_index = (int64_t)c[6];
    o.ms_depth = k.ms(1, 2); o.ms_shade = k.ms(2, 3); o.ms_finish = k.ms(3, 4); o.ms_total = k.ms(0, 4);
    if (o.bad_index)
        return fail(r, SPH_ERR_INVALID, "sph_render_mesh_end: %lld triangle(s) with a vertex index outside their mesh (skipped; the frame holds the rest)",
                         (long long)o.bad_index);
    return SPH_OK;
}

extern "C" int sph_render_mesh_stats(SphRender *r, SphRenderMeshStats *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    *out = r->mstats;
    return SPH_OK;
}
