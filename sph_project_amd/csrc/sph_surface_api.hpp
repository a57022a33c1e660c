// sph_surface_api.hpp -- the SphSurface object of include/sph_hip.h: its buffers under the memory cap, the pass sequence with its three
// host reads (coarse bounds, active bricks, vertex / triangle totals) and the stage events.  Host code, included at the end of
// sph_api.hip; the kernels are in sph_surface.hpp (anisotropic kernels: sph_surface_aniso.hpp), the method in DESIGN.md 14 and 29.
#pragma once
#include <algorithm>
#include <climits>
#include "sph_surface_aniso_eig.hpp"

enum SurfBufId { SB_XIN, SB_XTMP, SB_XS, SB_PCELL, SB_PSLOT, SB_CELL_START, SB_FLAG, SB_BRICK_ID, SB_BRICK_CELL, SB_PHI, SB_EDGE, SB_VBASE,
                 SB_TBASE, SB_VERT, SB_NRM, SB_TRI, SB_SMALL, SB_SCAN,
                 // post-processing
                 SB_ADJ_RAW, SB_ADJ_CNT, SB_ADJ_SLOT, SB_ADJ, SB_PCOUNT, SB_WEIGHT, SB_WORK_A, SB_WORK_B,
                 // anisotropic kernels
                 SB_ANISO_M, SB_ANISO_N, SB_ANISO_V, SB_COUNT_ };

struct SphSurface : DevObj {   // clk[0]: the reconstruction's stages, clk[1]: the post-processing's
    SphSurfaceParams prm;
    SurfDev d{};
    DevBuf buf[SB_COUNT_];
    bool live[SB_COUNT_] = {};   // holds data of the reconstruction running now
    int64_t nv = 0, nt = 0;
    bool have_mesh = false;
    SphSurfaceStats stats{};
    SphSurfacePostParams post{0, 0, 13.0, 0, 0};   // off
    SurfPost p{};
    bool have_post = false;   // the last reconstruction built the adjacency
    bool have_weights = false;
    SphSurfacePostStats post_stats{};
    SphSurfaceAnisoParams aniso{0, 25, 2.0, 0.5};   // off
    SurfAniso a{};
    StageClock aclk;             // moments + eigen, V_j
    bool have_aniso = false;     // the last reconstruction ran with anisotropic kernels
    SphSurfaceAnisoStats aniso_stats{};
};

static size_t surf_total(const SphSurface *s) {
    size_t t = 0;
    for (const DevBuf &b : s->buf) t += b.bytes;
    return t;
}
// buffer k with room for `need` bytes.  Past the cap, the buffers that hold nothing of this reconstruction go first; if it still does not
// fit: SPH_ERR_CAPACITY, nothing allocated.
static int surf_ensure(SphSurface *s, int k, size_t need, const char *what) {
    if (need == 0) need = 16;
    s->live[k] = true;
    DevBuf &b = s->buf[k];
    if (b.bytes >= need) return SPH_OK;
    const size_t cap = (size_t)s->prm.memory_cap_bytes;
    if (cap && surf_total(s) - b.bytes + need > cap) {
        for (int j = 0; j < SB_COUNT_; ++j)
            if (!s->live[j]) s->buf[j].release();
        if (surf_total(s) - b.bytes + need > cap)
            return fail(s, SPH_ERR_CAPACITY, "surface: %s needs %zu bytes, %zu held, cap %zu", what, need, surf_total(s) - b.bytes, cap);
    }
    return b.reserve(s, need);
}
#define SURF_ENSURE(s, k, need, what) do { int rc_ = surf_ensure((s), (k), (need), (what)); if (rc_) return rc_; } while (0)

extern "C" int sph_surface_create(const SphSurfaceParams *params, SphSurface **out) {
    if (!params || !out) return fail(nullptr, SPH_ERR_INVALID, "sph_surface_create: null argument");
    *out = nullptr;
    const SphSurfaceParams p = *params;
    if (!(p.radius > 0.0) || !(p.smoothing_length > 0.0) || !(p.cube_size > 0.0) || !std::isfinite(p.radius) ||
        !std::isfinite(p.smoothing_length) || !std::isfinite(p.cube_size) || !std::isfinite(p.iso) || !(p.iso > 0.0) || p.memory_cap_bytes < 0)
        return fail(nullptr, SPH_ERR_INVALID, "sph_surface_create: radius, smoothing_length, cube_size and iso must be positive and finite, the cap >= 0");
    const double h = 2.0 * p.smoothing_length * p.radius, e = p.cube_size * p.radius;
    const double Bd = ceil(h / e - 1e-9);
    // the edge word keeps a vertex offset of 21 bits (3 B^3 < 2^21): B <= 64 is far beyond any useful grid
    if (!(Bd >= 1.0 && Bd <= 64.0))
        return fail(nullptr, SPH_ERR_INVALID, "sph_surface_create: %.0f grid points per brick edge (smoothing_length / cube_size * 2); at most 64", Bd);
    int dev = 0;
    { int rc = pick_device("sph_surface_create", p.device, &dev); if (rc) return rc; }
    SphSurface *s = new SphSurface();
    s->prm = p;
    { int rc = devobj_open(s, "sph_surface_create", dev, p.fast_math); if (rc) { sph_surface_destroy(s); return rc; } }
    s->aclk.stream = s->stream;
    for (int k = 0; k < 3; ++k)
        if (hipEventCreate(&s->aclk.ev[k]) != hipSuccess) { sph_surface_destroy(s); return fail(nullptr, SPH_ERR_HIP, "sph_surface_create: event"); }
    SurfDev &d = s->d;
    d.h = (float)h;
    d.h2 = (float)(h * h);
    d.kW = (float)(8.0 / (M_PI * h * h * h));
    d.kG = (float)(6.0 * 8.0 / (M_PI * h * h * h * h));
    d.e = (float)e;
    d.B = (int)Bd;
    d.P = d.B * d.B * d.B;
    d.be = (float)(d.B * e);
    d.iso = (float)p.iso;
    d.stream = s->stream;
    s->stats.B = d.B;
    *out = s;
    return SPH_OK;
}

extern "C" void sph_surface_destroy(SphSurface *s) {
    if (!s) return;
    devobj_close(s, s->buf, SB_COUNT_);
    for (hipEvent_t e : s->aclk.ev) if (e) hipEventDestroy(e);
    delete s;
}

extern "C" const char *sph_surface_last_error(SphSurface *s) { return last_error(s); }

static bool surf_post_on(const SphSurface *s) { return s->post.mesh_smoothing_iters > 0 || s->post.normals_smoothing_iters > 0; }
static int surf_post(SphSurface *s, int nv, int nt);

// the passes after the input is in xin[0, n) and stage mark 0 has been set before it was put there
static int surf_run(SphSurface *s, int n) {
    SurfDev &d = s->d;
    hipStream_t st = s->stream;
    d.n = n;
    d.nb = 0;
    d.cmin[0] = d.cmin[1] = d.cmin[2] = 0;
    const bool aniso = s->aniso.enabled != 0;
    if (n == 0) {   // no particle: the empty mesh (and, with the post stage on, its empty adjacency)
        HIPCHK(s, hipStreamSynchronize(st));
        s->have_mesh = true;
        s->have_aniso = aniso;
        s->have_post = surf_post_on(s);
        s->stats.bytes_allocated = (int64_t)surf_total(s);
        return SPH_OK;
    }
    // SB_SMALL, 16 int slots: [0, 7) bounds, [8] counter (compaction), [10, 12) pairs (u64), [12] largest degree (post-processing),
    // [13, 15) sparse / clamped particles (anisotropic kernels)
    SURF_ENSURE(s, SB_SMALL, 64, "counters");
    d.bounds = (int *)s->buf[SB_SMALL].p;
    d.counter = d.bounds + 8;
    d.pairs = (unsigned long long *)(d.bounds + 10);
    const int init[7] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0};
    HIPCHK(s, hipMemcpyAsync(d.bounds, init, sizeof(init), hipMemcpyHostToDevice, st));
    s->L->surf_bounds(d);
    int bnd[7];
    HIPCHK(s, hipMemcpyAsync(bnd, d.bounds, sizeof(bnd), hipMemcpyDeviceToHost, st));
    HIPCHK(s, hipStreamSynchronize(st));
    if (bnd[6]) return fail(s, SPH_ERR_INVALID, "surface: non-finite particle position (or one beyond 1e8 coarse cells)");
    int64_t G = 1;
    for (int a = 0; a < 3; ++a) {
        d.cmin[a] = bnd[a] - 1;                       // one empty coarse cell around the particles
        d.cn[a] = bnd[3 + a] - bnd[a] + 3;
        G *= d.cn[a];
    }
    if (G > (int64_t)INT_MAX / 2) return fail(s, SPH_ERR_CAPACITY, "surface: coarse grid of %lld cells", (long long)G);
    d.G = (int)G;
    SURF_ENSURE(s, SB_XTMP, sizeof(float4) * (size_t)n, "particles");
    SURF_ENSURE(s, SB_XS, sizeof(float4) * (size_t)n, "particles");
    SURF_ENSURE(s, SB_PCELL, sizeof(int) * (size_t)n, "particles");
    SURF_ENSURE(s, SB_PSLOT, sizeof(int) * (size_t)n, "particles");
    SURF_ENSURE(s, SB_CELL_START, sizeof(int) * ((size_t)G + 1), "coarse grid");
    SURF_ENSURE(s, SB_FLAG, sizeof(int) * ((size_t)G + 1), "coarse grid");
    SURF_ENSURE(s, SB_BRICK_ID, sizeof(int) * (size_t)G, "coarse grid");
    SURF_ENSURE(s, SB_SCAN, sizeof(int) * ((size_t)(G + 1) / 1024 + 2), "scan");
    d.xtmp = (float4 *)s->buf[SB_XTMP].p; d.xs = (float4 *)s->buf[SB_XS].p;
    d.pcell = (int *)s->buf[SB_PCELL].p; d.pslot = (int *)s->buf[SB_PSLOT].p;
    d.cell_start = (int *)s->buf[SB_CELL_START].p; d.flag = (int *)s->buf[SB_FLAG].p; d.brick_id = (int *)s->buf[SB_BRICK_ID].p;
    d.scan_tmp = (int *)s->buf[SB_SCAN].p;
    SurfAniso &a = s->a;
    if (aniso) {
        SURF_ENSURE(s, SB_ANISO_M, sizeof(float4) * (size_t)n, "kernel matrices");
        SURF_ENSURE(s, SB_ANISO_N, sizeof(float4) * (size_t)n, "kernel matrices");
        SURF_ENSURE(s, SB_ANISO_V, sizeof(float) * (size_t)n, "kernel matrices");
        a.h = 2.0 * s->prm.smoothing_length * s->prm.radius;
        a.prm.min_nb = s->aniso.min_neighbours;
        a.prm.inv_ratio = (float)(1.0 / s->aniso.max_ratio);
        a.prm.inv_scale = (float)(1.0 / s->aniso.sparse_scale);
        a.am = (float4 *)s->buf[SB_ANISO_M].p; a.an = (float4 *)s->buf[SB_ANISO_N].p; a.vol = (float *)s->buf[SB_ANISO_V].p;
        a.cnt = d.bounds + 13;
    }
    s->L->surf_bin(d);   // (leaves xs = the key-ordered particles with the isotropic V)
    if (aniso) {
        HIPCHK(s, s->aclk.mark(0));
        s->L->surf_aniso_moments(d, a);
        HIPCHK(s, s->aclk.mark(1));
        s->L->surf_aniso_volume(d, a);
        HIPCHK(s, s->aclk.mark(2));
    }
    HIPCHK(s, s->clk[0].mark(1));
    s->L->surf_flags(d);
    HIPCHK(s, s->clk[0].mark(2));
    int nb = 0;
    HIPCHK(s, hipMemcpyAsync(&nb, d.flag + G, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(s, hipStreamSynchronize(st));
    d.nb = nb;
    const size_t points = (size_t)nb * (size_t)d.P;
    SURF_ENSURE(s, SB_BRICK_CELL, sizeof(int) * (size_t)nb, "bricks");
    SURF_ENSURE(s, SB_PHI, sizeof(float) * points, "grid values");
    SURF_ENSURE(s, SB_EDGE, sizeof(unsigned) * points, "grid values");
    SURF_ENSURE(s, SB_VBASE, sizeof(int) * ((size_t)nb + 1), "bricks");
    SURF_ENSURE(s, SB_TBASE, sizeof(int) * ((size_t)nb + 1), "bricks");
    if ((size_t)nb + 1 > (size_t)(G + 1)) return fail(s, SPH_ERR_INVALID, "surface: internal brick count");
    d.brick_cell = (int *)s->buf[SB_BRICK_CELL].p; d.phi = (float *)s->buf[SB_PHI].p; d.edge = (unsigned *)s->buf[SB_EDGE].p;
    d.vbase = (int *)s->buf[SB_VBASE].p; d.tbase = (int *)s->buf[SB_TBASE].p;
    if (aniso) s->L->surf_field_aniso(d, a);
    else s->L->surf_field(d);
    HIPCHK(s, s->clk[0].mark(3));
    s->L->surf_count(d);
    int tot[2] = {0, 0};
    HIPCHK(s, hipMemcpyAsync(&tot[0], d.vbase + nb, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(s, hipMemcpyAsync(&tot[1], d.tbase + nb, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(s, hipStreamSynchronize(st));
    if (tot[0] < 0 || tot[1] < 0 || tot[1] > INT_MAX / 3 || tot[0] > INT_MAX / 3)
        return fail(s, SPH_ERR_CAPACITY, "surface: more than 2^31 / 3 vertices or triangles");
    SURF_ENSURE(s, SB_VERT, sizeof(float) * 3 * (size_t)tot[0], "vertices");
    SURF_ENSURE(s, SB_TRI, sizeof(int) * 3 * (size_t)tot[1], "triangles");
    if (s->prm.normals) SURF_ENSURE(s, SB_NRM, sizeof(float) * 3 * (size_t)tot[0], "normals");
    d.vert = (float *)s->buf[SB_VERT].p; d.tri = (int *)s->buf[SB_TRI].p; d.nrm = s->prm.normals ? (float *)s->buf[SB_NRM].p : nullptr;
    s->L->surf_emit(d);
    HIPCHK(s, s->clk[0].mark(4));
    // (smoothed positions get their normals in the post stage: none here then, and ms_normals ~ 0)
    if (s->prm.normals && !(surf_post_on(s) && s->post.mesh_smoothing_iters > 0)) {
        if (aniso) s->L->surf_normals_aniso(d, a, tot[0]);
        else s->L->surf_normals(d, tot[0]);
    }
    HIPCHK(s, s->clk[0].mark(5));
    unsigned long long pairs = 0;
    int acnt[2] = {0, 0};
    HIPCHK(s, hipMemcpyAsync(&pairs, d.pairs, sizeof(pairs), hipMemcpyDeviceToHost, st));
    if (aniso) HIPCHK(s, hipMemcpyAsync(acnt, a.cnt, sizeof(acnt), hipMemcpyDeviceToHost, st));
    HIPCHK(s, hipStreamSynchronize(st));
    HIPCHK(s, hipGetLastError());
    if (surf_post_on(s)) { const int rc = surf_post(s, tot[0], tot[1]); if (rc) return rc; }
    s->nv = tot[0];
    s->nt = tot[1];
    s->have_mesh = true;
    SphSurfaceStats &o = s->stats;
    o.particles = n; o.active_bricks = nb; o.points_evaluated = (int64_t)points; o.pair_tests = (int64_t)pairs;
    o.vertices = s->nv; o.triangles = s->nt; o.bytes_allocated = (int64_t)surf_total(s); o.B = d.B;
    const StageClock &c = s->clk[0];
    o.ms_bin = c.ms(0, 1); o.ms_bricks = c.ms(1, 2); o.ms_field = c.ms(2, 3);
    o.ms_mesh = c.ms(3, 4); o.ms_normals = c.ms(4, 5); o.ms_total = c.ms(0, 5);
    if (aniso) {
        s->have_aniso = true;
        s->aniso_stats = SphSurfaceAnisoStats{acnt[0], acnt[1], s->aclk.ms(0, 1), s->aclk.ms(1, 2)};
    }
    return SPH_OK;
}

static void surf_begin(SphSurface *s) {
    s->have_mesh = false;
    s->nv = s->nt = 0;
    for (bool &l : s->live) l = false;
    s->stats = SphSurfaceStats{};
    s->stats.B = s->d.B;
    s->have_post = s->have_weights = false;
    s->post_stats = SphSurfacePostStats{};
    s->have_aniso = false;
    s->aniso_stats = SphSurfaceAnisoStats{};
}

extern "C" int sph_surface_reconstruct(SphSurface *s, const float *xyz, int64_t n) {
    if (!s) return SPH_ERR_INVALID;
    if (n < 0 || n > INT_MAX / 2 || (n > 0 && !xyz)) return fail(s, SPH_ERR_INVALID, "sph_surface_reconstruct: bad particle array (n = %lld)", (long long)n);
    HIPCHK(s, hipSetDevice(s->device));
    surf_begin(s);
    std::vector<float4> tmp((size_t)n);
    for (int64_t i = 0; i < n; ++i) tmp[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0f);
    SURF_ENSURE(s, SB_XIN, sizeof(float4) * (size_t)n, "particles");
    s->d.xin = (float4 *)s->buf[SB_XIN].p;
    HIPCHK(s, s->clk[0].mark(0));
    if (n) HIPCHK(s, hipMemcpyAsync(s->d.xin, tmp.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, s->stream));
    return surf_run(s, (int)n);
}

extern "C" int sph_surface_reconstruct_object(SphSurface *s, SphHandle *h, int object_id) {
    if (!s || !h) return SPH_ERR_INVALID;
    if (h->st.slab_active || h->swap_axis)
        return fail(s, SPH_ERR_UNSUPPORTED, "sph_surface_reconstruct_object: sharded handle (reconstruct each rank's download instead)");
    if (h->device != s->device) return fail(s, SPH_ERR_INVALID, "sph_surface_reconstruct_object: handle on device %d, surface on %d", h->device, s->device);
    if (object_id < 0 || object_id >= SPH_MAX_OBJECTS) return fail(s, SPH_ERR_INVALID, "sph_surface_reconstruct_object: object id %d", object_id);
    HIPCHK(s, hipSetDevice(s->device));
    HIPCHK(s, hipStreamSynchronize(h->st.stream));   // the handle's last step has written the positions
    surf_begin(s);
    const int n_all = h->n;
    SURF_ENSURE(s, SB_XIN, sizeof(float4) * (size_t)n_all, "particles");
    SURF_ENSURE(s, SB_SMALL, 64, "counters");
    s->d.xin = (float4 *)s->buf[SB_XIN].p;
    s->d.counter = (int *)s->buf[SB_SMALL].p + 8;
    HIPCHK(s, s->clk[0].mark(0));
    s->L->surf_compact(s->d, h->st.posv.cur(), h->st.meta.cur(), n_all, object_id);
    int n = 0;
    HIPCHK(s, hipMemcpyAsync(&n, s->d.counter, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return surf_run(s, n);
}

extern "C" int sph_surface_mesh_size(SphSurface *s, int64_t *n_vertices, int64_t *n_triangles) {
    if (!s || !n_vertices || !n_triangles) return SPH_ERR_INVALID;
    if (!s->have_mesh) return fail(s, SPH_ERR_INVALID, "sph_surface_mesh_size: no reconstruction has succeeded yet");
    *n_vertices = s->nv;
    *n_triangles = s->nt;
    return SPH_OK;
}

extern "C" int sph_surface_download(SphSurface *s, float *vertices, float *normals_or_NULL, int32_t *triangles) {
    if (!s) return SPH_ERR_INVALID;
    if (!s->have_mesh) return fail(s, SPH_ERR_INVALID, "sph_surface_download: no reconstruction has succeeded yet");
    if ((s->nv && !vertices) || (s->nt && !triangles)) return fail(s, SPH_ERR_INVALID, "sph_surface_download: null output");
    if (normals_or_NULL && !s->prm.normals) return fail(s, SPH_ERR_INVALID, "sph_surface_download: created without normals");
    HIPCHK(s, hipSetDevice(s->device));
    if (s->nv) HIPCHK(s, hipMemcpy(vertices, s->d.vert, sizeof(float) * 3 * (size_t)s->nv, hipMemcpyDeviceToHost));
    if (s->nv && normals_or_NULL) HIPCHK(s, hipMemcpy(normals_or_NULL, s->d.nrm, sizeof(float) * 3 * (size_t)s->nv, hipMemcpyDeviceToHost));
    if (s->nt) HIPCHK(s, hipMemcpy(triangles, s->d.tri, sizeof(int) * 3 * (size_t)s->nt, hipMemcpyDeviceToHost));
    return SPH_OK;
}

extern "C" int sph_surface_stats(SphSurface *s, SphSurfaceStats *out) {
    if (!s || !out) return SPH_ERR_INVALID;
    *out = s->stats;
    return SPH_OK;
}

// --- post-processing: after the emit pass, on the mesh and the binned particles of this reconstruction ------------------
static int surf_post(SphSurface *s, int nv, int nt) {
    SurfDev &d = s->d;
    SurfPost &p = s->p;
    hipStream_t st = s->stream;
    const SphSurfacePostParams q = s->post;
    const bool weights = q.mesh_smoothing_weights && q.mesh_smoothing_iters > 0;
    // the slot ranges and CSR offsets are int and reach 6 nt (2 slots per triangle corner): refuse before anything is allocated or launched
    if ((int64_t)6 * nt > (int64_t)INT_MAX)
        return fail(s, SPH_ERR_CAPACITY, "surface: %d triangles, more than 2^31 / 6 for the smoothing's adjacency", nt);
    SURF_ENSURE(s, SB_ADJ_RAW, sizeof(int) * ((size_t)nv + 1), "adjacency");
    SURF_ENSURE(s, SB_ADJ_CNT, sizeof(int) * ((size_t)nv + 1), "adjacency");
    SURF_ENSURE(s, SB_ADJ_SLOT, sizeof(int) * 6 * (size_t)nt, "adjacency");
    SURF_ENSURE(s, SB_WORK_A, sizeof(float4) * (size_t)nv, "smoothing");
    SURF_ENSURE(s, SB_WORK_B, sizeof(float4) * (size_t)nv, "smoothing");
    if (weights) {
        SURF_ENSURE(s, SB_PCOUNT, sizeof(float) * (size_t)d.n, "smoothing weights");
        SURF_ENSURE(s, SB_WEIGHT, sizeof(float) * (size_t)nv, "smoothing weights");
    }
    // surf_scan's tile sums: sized for the coarse grid so far, now for nv as well
    SURF_ENSURE(s, SB_SCAN, std::max(s->buf[SB_SCAN].bytes, sizeof(int) * ((size_t)nv / 1024 + 2)), "scan");
    d.scan_tmp = (int *)s->buf[SB_SCAN].p;
    p = SurfPost{};
    p.nv = nv; p.nt = nt; p.tri = d.tri;
    p.raw = (int *)s->buf[SB_ADJ_RAW].p; p.cnt = (int *)s->buf[SB_ADJ_CNT].p; p.slot = (int *)s->buf[SB_ADJ_SLOT].p;
    p.maxdeg = d.bounds + 12;   // (SB_SMALL: see surf_run)
    p.pc = weights ? (float *)s->buf[SB_PCOUNT].p : nullptr;
    p.w = weights ? (float *)s->buf[SB_WEIGHT].p : nullptr;
    p.norm = (float)q.weights_normalization;
    p.a = (float4 *)s->buf[SB_WORK_A].p; p.b = (float4 *)s->buf[SB_WORK_B].p;
    HIPCHK(s, s->clk[1].mark(0));
    s->L->surf_post_adjacency(d, p);
    int cnt[2] = {0, 0};   // entries, largest degree
    HIPCHK(s, hipMemcpyAsync(&cnt[0], p.cnt + nv, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(s, hipMemcpyAsync(&cnt[1], p.maxdeg, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(s, hipStreamSynchronize(st));
    if (cnt[0] < 0 || (int64_t)cnt[0] > (int64_t)6 * nt) return fail(s, SPH_ERR_INVALID, "surface: internal adjacency count %d", cnt[0]);
    SURF_ENSURE(s, SB_ADJ, sizeof(int) * (size_t)cnt[0], "adjacency");
    p.adj = (int *)s->buf[SB_ADJ].p;
    s->L->surf_post_compact(d, p);
    HIPCHK(s, s->clk[1].mark(1));
    if (weights) s->L->surf_post_weights(d, p);   // at the unsmoothed positions
    HIPCHK(s, s->clk[1].mark(2));
    s->L->surf_post_smooth(d, p, q.mesh_smoothing_iters);
    HIPCHK(s, s->clk[1].mark(3));
    if (s->prm.normals && q.mesh_smoothing_iters > 0) {   // -grad phi at the smoothed positions
        if (s->aniso.enabled) s->L->surf_normals_aniso(d, s->a, nv);
        else s->L->surf_normals(d, nv);
    }
    HIPCHK(s, s->clk[1].mark(4));
    s->L->surf_post_nsmooth(d, p, q.normals_smoothing_iters);
    HIPCHK(s, s->clk[1].mark(5));
    HIPCHK(s, hipStreamSynchronize(st));
    HIPCHK(s, hipGetLastError());
    s->have_post = true;
    s->have_weights = weights;
    SphSurfacePostStats &o = s->post_stats;
    o.adjacency_entries = cnt[0]; o.max_degree = cnt[1];
    const StageClock &c = s->clk[1];
    o.ms_adjacency = c.ms(0, 1); o.ms_weights = c.ms(1, 2); o.ms_smoothing = c.ms(2, 3);
    o.ms_normals = c.ms(3, 4); o.ms_normal_smoothing = c.ms(4, 5); o.ms_total = c.ms(0, 5);
    return SPH_OK;
}

extern "C" int sph_surface_set_postprocess(SphSurface *s, const SphSurfacePostParams *params) {
    if (!s || !params) return SPH_ERR_INVALID;
    const SphSurfacePostParams q = *params;
    if (q.mesh_smoothing_iters < 0 || q.normals_smoothing_iters < 0)
        return fail(s, SPH_ERR_INVALID, "sph_surface_set_postprocess: negative iteration count");
    if (!std::isfinite(q.weights_normalization) || !(q.weights_normalization > 0.0) || !std::isfinite((float)q.weights_normalization) ||
        !((float)q.weights_normalization > 0.0f))
        return fail(s, SPH_ERR_INVALID, "sph_surface_set_postprocess: weights_normalization must be positive and finite");
    if (q.normals_smoothing_iters > 0 && !s->prm.normals)
        return fail(s, SPH_ERR_INVALID, "sph_surface_set_postprocess: normal smoothing on an object created without normals");
    s->post = q;
    return SPH_OK;
}

extern "C" int sph_surface_post_stats(SphSurface *s, SphSurfacePostStats *out) {
    if (!s || !out) return SPH_ERR_INVALID;
    *out = s->post_stats;
    return SPH_OK;
}

extern "C" int sph_surface_download_post(SphSurface *s, int32_t *offsets, int32_t *neighbours, float *weights) {
    if (!s) return SPH_ERR_INVALID;
    if (!s->have_mesh || !s->have_post)
        return fail(s, SPH_ERR_INVALID, "sph_surface_download_post: the last reconstruction ran no smoothing");
    HIPCHK(s, hipSetDevice(s->device));
    const size_t nv = (size_t)s->nv, ne = (size_t)s->post_stats.adjacency_entries;
    if (offsets && nv) HIPCHK(s, hipMemcpy(offsets, s->p.cnt, sizeof(int) * (nv + 1), hipMemcpyDeviceToHost));
    else if (offsets) offsets[0] = 0;
    if (neighbours && ne) HIPCHK(s, hipMemcpy(neighbours, s->p.adj, sizeof(int) * ne, hipMemcpyDeviceToHost));
    if (weights) {
        if (s->have_weights) { if (nv) HIPCHK(s, hipMemcpy(weights, s->p.w, sizeof(float) * nv, hipMemcpyDeviceToHost)); }
        else for (size_t i = 0; i < nv; ++i) weights[i] = 1.0f;
    }
    return SPH_OK;
}

// --- anisotropic kernels ----------------------------------------------------------------------------------------------
static const char *surf_aniso_check(const SphSurfaceAnisoParams &q) {
    if (q.min_neighbours < 0) return "min_neighbours must not be negative";
    if (!std::isfinite(q.max_ratio) || !std::isfinite((float)q.max_ratio) || !(q.max_ratio >= 1.0)) return "max_ratio must be finite and >= 1";
    if (!std::isfinite(q.sparse_scale) || !(q.sparse_scale > 0.0) || !(q.sparse_scale <= 1.0) || !std::isfinite((float)(1.0 / q.sparse_scale)))
        return "sparse_scale must lie in (0, 1]";
    return nullptr;
}

extern "C" int sph_surface_set_anisotropy(SphSurface *s, const SphSurfaceAnisoParams *params_or_NULL) {
    if (!s) return SPH_ERR_INVALID;
    if (!params_or_NULL || !params_or_NULL->enabled) { s->aniso.enabled = 0; return SPH_OK; }
    if (const char *why = surf_aniso_check(*params_or_NULL)) return fail(s, SPH_ERR_INVALID, "sph_surface_set_anisotropy: %s", why);
    s->aniso = *params_or_NULL;
    s->aniso.enabled = 1;
    return SPH_OK;
}

extern "C" int sph_surface_anisotropy_stats(SphSurface *s, SphSurfaceAnisoStats *out) {
    if (!s || !out) return SPH_ERR_INVALID;
    *out = s->aniso_stats;
    return SPH_OK;
}

extern "C" int sph_surface_download_anisotropy(SphSurface *s, float *xyz, float *A6, int32_t *neighbours, float *V) {
    if (!s) return SPH_ERR_INVALID;
    if (!s->have_mesh || !s->have_aniso)
        return fail(s, SPH_ERR_INVALID, "sph_surface_download_anisotropy: the last reconstruction ran without anisotropic kernels");
    HIPCHK(s, hipSetDevice(s->device));
    const size_t n = (size_t)s->stats.particles;
    if (!n) return SPH_OK;
    std::vector<float4> t(n), u(n);
    if (xyz) {
        HIPCHK(s, hipMemcpy(t.data(), s->d.xs, sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) { xyz[3 * i] = t[i].x; xyz[3 * i + 1] = t[i].y; xyz[3 * i + 2] = t[i].z; }
    }
    if (A6 || neighbours) {
        HIPCHK(s, hipMemcpy(t.data(), s->a.am, sizeof(float4) * n, hipMemcpyDeviceToHost));
        HIPCHK(s, hipMemcpy(u.data(), s->a.an, sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (A6) { float *o = A6 + 6 * i; o[0] = t[i].x; o[1] = t[i].y; o[2] = t[i].z; o[3] = t[i].w; o[4] = u[i].x; o[5] = u[i].y; }
            if (neighbours) memcpy(&neighbours[i], &u[i].w, sizeof(int32_t));
        }
    }
    if (V) HIPCHK(s, hipMemcpy(V, s->a.vol, sizeof(float) * n, hipMemcpyDeviceToHost));
    return SPH_OK;
}

// the device's eigen and clamp routine (sph_surface_aniso_eig.hpp) on the host: no GPU involved
extern "C" int sph_surface_aniso_matrix_host(const float *C6, int64_t n, const int32_t *neighbours, const SphSurfaceAnisoParams *p, float *A6) {
    if (n < 0 || !p || (n > 0 && (!C6 || !A6)) || surf_aniso_check(*p)) return SPH_ERR_INVALID;
    const SurfAnisoPrm prm = {p->min_neighbours, (float)(1.0 / p->max_ratio), (float)(1.0 / p->sparse_scale)};
    for (int64_t i = 0; i < n; ++i) {
        float det;
        surf_aniso_matrix(C6 + 6 * i, neighbours ? neighbours[i] : INT_MAX, prm, A6 + 6 * i, &det);
    }
    return SPH_OK;
}
