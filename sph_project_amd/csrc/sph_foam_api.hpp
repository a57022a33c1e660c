// sph_foam_api.hpp -- the SphFoam object of include/sph_hip.h: its buffers, the two fluid sources (host arrays, a live handle), the pass
// sequence with its one host read (the counters) and the stage events; and the renderer's hook that draws the diffuse set
// (sph_render_set_foam).  Host code, included at the end of sph_api.hip; the kernels are in sph_foam.hpp, the method in DESIGN.md 26.
#pragma once
#include <climits>

enum FoamBufId { FB_XIN, FB_VIN, FB_IDIN, FB_PCELL, FB_PSLOT, FB_CELL, FB_XT, FB_VT, FB_IDT, FB_SRCT, FB_XS, FB_VS, FB_IDS, FB_SRC, FB_NRM,
                 FB_POT, FB_CNT, FB_DX0, FB_DX1, FB_DV0, FB_DV1, FB_KEY0, FB_KEY1, FB_KEEP, FB_CTR, FB_SCAN, FB_HFLAG, FB_COUNT_ };

struct SphFoam : DevObj {   // clk[0]: the stages of a step
    SphFoamParams prm;
    FoamDev d{};
    DevBuf buf[FB_COUNT_];
    int64_t count = 0;          // diffuse particles
    int64_t cap = 0;            // 0: not sized yet
    int64_t steps = 0;
    uint64_t serial = 0;        // of the seeded particles
    bool have_step = false;
    bool from_handle = false;
    SphFoamStats stats{};
};

static size_t foam_total(const SphFoam *f) {
    size_t t = 0;
    for (const DevBuf &b : f->buf) t += b.bytes;
    return t;
}
#define FOAM_ROOM(f, k, need) do { int rc_ = (f)->buf[k].reserve((f), std::max<size_t>((need), 16)); if (rc_) return rc_; } while (0)

// the diffuse banks, once: capacity `cap` (and the scan's tile sums for it)
static int foam_size_diffuse(SphFoam *f, int64_t cap) {
    if (f->cap) return SPH_OK;
    if (cap < 1) cap = 1;
    if (cap > INT_MAX / 2) return fail(f, SPH_ERR_CAPACITY, "foam: a diffuse capacity of %lld particles (at most 2^30)", (long long)cap);
    const size_t c = (size_t)cap;
    FOAM_ROOM(f, FB_DX0, sizeof(float4) * c); FOAM_ROOM(f, FB_DX1, sizeof(float4) * c);
    FOAM_ROOM(f, FB_DV0, sizeof(float4) * c); FOAM_ROOM(f, FB_DV1, sizeof(float4) * c);
    FOAM_ROOM(f, FB_KEY0, 8 * c); FOAM_ROOM(f, FB_KEY1, 8 * c);
    FOAM_ROOM(f, FB_KEEP, sizeof(int) * (c + 1));
    FoamDev &d = f->d;
    d.dx[0] = (float4 *)f->buf[FB_DX0].p; d.dx[1] = (float4 *)f->buf[FB_DX1].p;
    d.dv[0] = (float4 *)f->buf[FB_DV0].p; d.dv[1] = (float4 *)f->buf[FB_DV1].p;
    d.dkey[0] = (unsigned long long *)f->buf[FB_KEY0].p; d.dkey[1] = (unsigned long long *)f->buf[FB_KEY1].p;
    d.keep = (int *)f->buf[FB_KEEP].p;
    d.cap = (int)cap;
    f->cap = cap;
    return SPH_OK;
}

extern "C" int sph_foam_create(const SphFoamParams *params, SphFoam **out) {
    if (!params || !out) return fail(nullptr, SPH_ERR_INVALID, "sph_foam_create: null argument");
    *out = nullptr;
    const SphFoamParams p = *params;
    const double all[] = {p.radius, p.padding, p.ta_min, p.ta_max, p.wc_min, p.wc_max, p.e_min, p.e_max, p.k_ta, p.k_wc, p.life_min, p.life_max,
                          p.k_b, p.k_d, p.normal_min, p.domain_lo[0], p.domain_lo[1], p.domain_lo[2], p.domain_hi[0], p.domain_hi[1], p.domain_hi[2],
                          p.gravity[0], p.gravity[1], p.gravity[2]};
    for (double v : all)
        if (!std::isfinite(v) || !std::isfinite((float)v)) return fail(nullptr, SPH_ERR_INVALID, "sph_foam_create: a parameter is not finite");
    if (!(p.radius > 0.0) || p.padding < 0.0 || !(p.ta_max > p.ta_min) || !(p.wc_max > p.wc_min) || !(p.e_max > p.e_min) || p.k_ta < 0.0 ||
        p.k_wc < 0.0 || !(p.life_min > 0.0) || !(p.life_max >= p.life_min) || p.normal_min < 0.0 || p.n_spray < 0 || p.n_bubble < p.n_spray ||
        p.max_per_particle < 0 || p.max_per_particle > 255 || p.max_diffuse < 0 || p.reserved != 0)
        return fail(nullptr, SPH_ERR_INVALID, "sph_foam_create: radius > 0, padding >= 0, limits with max > min, rates >= 0, 0 < life_min <= life_max, "
                                              "0 <= n_spray <= n_bubble, max_per_particle 0..255, max_diffuse >= 0, reserved 0");
    const double h = 4.0 * p.radius;
    int cn[3];
    double G = 1.0;
    for (int a = 0; a < 3; ++a) {
        if (!(p.domain_hi[a] > p.domain_lo[a])) return fail(nullptr, SPH_ERR_INVALID, "sph_foam_create: empty domain along axis %d", a);
        const double c = ceil((p.domain_hi[a] - p.domain_lo[a]) / h) + 2.0;
        if (!(c < 1e6)) return fail(nullptr, SPH_ERR_INVALID, "sph_foam_create: %.0f cells along axis %d", c, a);
        cn[a] = (int)c;
        G *= c;
    }
    if (!(G <= 1073741824.0)) return fail(nullptr, SPH_ERR_INVALID, "sph_foam_create: a grid of %.0f cells (at most 2^30)", G);
    int dev = 0;
    { int rc = pick_device("sph_foam_create", p.device, &dev); if (rc) return rc; }
    SphFoam *f = new SphFoam();
    f->prm = p;
    { int rc = devobj_open(f, "sph_foam_create", dev, p.fast_math); if (rc) { sph_foam_destroy(f); return rc; } }
    FoamDev &d = f->d;
    d.h = (float)h; d.pr = (float)p.radius;
    d.G = 1;
    for (int a = 0; a < 3; ++a) {
        d.glo[a] = (float)p.domain_lo[a]; d.cn[a] = cn[a]; d.G *= cn[a];
        d.lo[a] = (float)(p.domain_lo[a] + p.padding); d.hi[a] = (float)(p.domain_hi[a] - p.padding);
        d.g[a] = (float)p.gravity[a];
    }
    d.ta_lo = (float)p.ta_min; d.ta_hi = (float)p.ta_max; d.wc_lo = (float)p.wc_min; d.wc_hi = (float)p.wc_max;
    d.e_lo = (float)p.e_min; d.e_hi = (float)p.e_max; d.k_ta = (float)p.k_ta; d.k_wc = (float)p.k_wc;
    d.life_lo = (float)p.life_min; d.life_hi = (float)p.life_max; d.k_b = (float)p.k_b; d.k_d = (float)p.k_d;
    d.nmin_h = (float)p.normal_min * d.h;
    d.n_spray = p.n_spray; d.n_bubble = p.n_bubble; d.max_pp = p.max_per_particle;
    d.seed_lo = (unsigned)(p.seed & 0xffffffffu); d.seed_hi = (unsigned)(p.seed >> 32);
    d.stream = f->stream;
    int rc = f->buf[FB_CELL].reserve(nullptr, sizeof(int) * ((size_t)d.G + 1));
    if (!rc) rc = f->buf[FB_CTR].reserve(nullptr, 8 * FOAM_CTR_WORDS);
    if (!rc) rc = f->buf[FB_SCAN].reserve(nullptr, sizeof(int) * ((size_t)d.G / 1024 + 2));
    if (!rc && p.max_diffuse) rc = foam_size_diffuse(f, p.max_diffuse);
    if (rc) {
        const std::string msg = f->err;
        sph_foam_destroy(f);
        return fail(nullptr, rc, "sph_foam_create: %s", msg.empty() ? "device buffers" : msg.c_str());
    }
    d.cell_start = (int *)f->buf[FB_CELL].p;
    d.ctr = (unsigned long long *)f->buf[FB_CTR].p;
    *out = f;
    return SPH_OK;
}

extern "C" void sph_foam_destroy(SphFoam *f) {
    if (!f) return;
    devobj_close(f, f->buf, FB_COUNT_);
    delete f;
}

extern "C" const char *sph_foam_last_error(SphFoam *f) { return last_error(f); }

// the fluid-sized buffers for n particles, and the scan's tile sums for everything scanned in a step
static int foam_room_fluid(SphFoam *f, size_t n, size_t n_scan_extra) {
    FOAM_ROOM(f, FB_XIN, sizeof(float4) * n); FOAM_ROOM(f, FB_VIN, sizeof(float4) * n); FOAM_ROOM(f, FB_IDIN, 4 * n);
    FOAM_ROOM(f, FB_PCELL, 4 * n); FOAM_ROOM(f, FB_PSLOT, 4 * n);
    FOAM_ROOM(f, FB_XT, sizeof(float4) * n); FOAM_ROOM(f, FB_VT, sizeof(float4) * n); FOAM_ROOM(f, FB_IDT, 4 * n); FOAM_ROOM(f, FB_SRCT, 4 * n);
    FOAM_ROOM(f, FB_XS, sizeof(float4) * n); FOAM_ROOM(f, FB_VS, sizeof(float4) * n); FOAM_ROOM(f, FB_IDS, 4 * n); FOAM_ROOM(f, FB_SRC, 4 * n);
    FOAM_ROOM(f, FB_NRM, sizeof(float4) * n); FOAM_ROOM(f, FB_POT, sizeof(float4) * n); FOAM_ROOM(f, FB_CNT, 4 * (n + 1));
    const size_t longest = std::max(std::max((size_t)f->d.G, n), std::max((size_t)f->cap, n_scan_extra)) + 1;
    FOAM_ROOM(f, FB_SCAN, sizeof(int) * (longest / 1024 + 2));
    FoamDev &d = f->d;
    DevBuf *b = f->buf;
    d.xin = (float4 *)b[FB_XIN].p; d.vin = (float4 *)b[FB_VIN].p; d.idin = (int *)b[FB_IDIN].p;
    d.pcell = (int *)b[FB_PCELL].p; d.pslot = (int *)b[FB_PSLOT].p;
    d.xt = (float4 *)b[FB_XT].p; d.vt = (float4 *)b[FB_VT].p; d.idt = (int *)b[FB_IDT].p; d.srct = (int *)b[FB_SRCT].p;
    d.xs = (float4 *)b[FB_XS].p; d.vs = (float4 *)b[FB_VS].p; d.ids = (int *)b[FB_IDS].p; d.src = (int *)b[FB_SRC].p;
    d.nrm = (float4 *)b[FB_NRM].p; d.pot = (float4 *)b[FB_POT].p; d.cnt = (int *)b[FB_CNT].p;
    d.scan_tmp = (int *)b[FB_SCAN].p;
    return SPH_OK;
}

// the step after the fluid set is in xin / vin / idin [0, n) and stage mark 0 has been set before it was put there
static int foam_run(SphFoam *f, int n, double dt) {
    FoamDev &d = f->d;
    hipStream_t st = f->stream;
    StageClock &c = f->clk[0];
    d.n = n;
    d.nd = (int)f->count;
    d.dt = (float)dt;
    d.t = (unsigned)(f->steps & 0xffffffff);
    HIPCHK(f, hipMemsetAsync(d.ctr, 0, 8 * FOAM_CTR_WORDS, st));
    f->L->foam_grid(d);
    HIPCHK(f, c.mark(1));
    f->L->foam_advect(d);
    HIPCHK(f, c.mark(2));
    f->L->foam_normals(d);
    HIPCHK(f, c.mark(3));
    f->L->foam_potentials(d);
    HIPCHK(f, c.mark(4));
    f->L->foam_generate(d);
    HIPCHK(f, c.mark(5));
    unsigned long long ctr[FOAM_CTR_WORDS];
    HIPCHK(f, hipMemcpyAsync(ctr, d.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    HIPCHK(f, hipStreamSynchronize(st));
    HIPCHK(f, hipGetLastError());
    if ((int64_t)ctr[FC_COUNT] > f->cap) return fail(f, SPH_ERR_INVALID, "foam: internal count %llu beyond the capacity %lld", ctr[FC_COUNT], (long long)f->cap);
    // the survivors and the children lie in bank 1: it becomes the current one
    std::swap(d.dx[0], d.dx[1]); std::swap(d.dv[0], d.dv[1]); std::swap(d.dkey[0], d.dkey[1]);
    f->count = (int64_t)ctr[FC_COUNT];
    f->steps++;
    f->have_step = true;
    SphFoamStats &o = f->stats;
    o.step = f->steps; o.fluid = n; o.diffuse = f->count;
    o.spray = (int64_t)ctr[FC_CLASS]; o.foam = (int64_t)ctr[FC_CLASS + 1]; o.bubble = (int64_t)ctr[FC_CLASS + 2];
    o.born = (int64_t)ctr[FC_BORN]; o.died = (int64_t)ctr[FC_DIED]; o.dropped = (int64_t)ctr[FC_DROPPED];
    o.born_total += o.born; o.died_total += o.died; o.dropped_total += o.dropped;
    for (int k = 0; k < 3; ++k) { o.pairs_visited[k] = (int64_t)ctr[FC_VISIT + k]; o.pairs_accepted[k] = (int64_t)ctr[FC_ACCEPT + k]; }
    o.bytes_allocated = (int64_t)foam_total(f);
    o.ms_grid = c.ms(0, 1); o.ms_advect = c.ms(1, 2); o.ms_normals = c.ms(2, 3); o.ms_potentials = c.ms(3, 4); o.ms_generate = c.ms(4, 5);
    o.ms_total = c.ms(0, 5);
    return SPH_OK;
}

static int foam_check_dt(SphFoam *f, const char *who, double dt) {
    if (!(dt > 0.0) || !std::isfinite(dt) || !std::isfinite((float)dt) || !((float)dt > 0.0f))
        return fail(f, SPH_ERR_INVALID, "%s: dt %g must be positive and finite", who, dt);
    return SPH_OK;
}

extern "C" int sph_foam_step_points(SphFoam *f, const float *xyz, const float *vel, const int32_t *ids, int64_t n, double dt) {
    if (!f) return SPH_ERR_INVALID;
    if (n < 0 || n > INT_MAX / 2 || (n > 0 && (!xyz || !vel || !ids)))
        return fail(f, SPH_ERR_INVALID, "sph_foam_step_points: bad particle arrays (n = %lld)", (long long)n);
    { int rc = foam_check_dt(f, "sph_foam_step_points", dt); if (rc) return rc; }
    HIPCHK(f, hipSetDevice(f->device));
    { int rc = foam_size_diffuse(f, 2 * n); if (rc) return rc; }
    { int rc = foam_room_fluid(f, (size_t)n, 0); if (rc) return rc; }
    std::vector<float4> x4((size_t)n), v4((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        x4[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0f);
        v4[i] = make_float4(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2], 0.0f);
    }
    HIPCHK(f, f->clk[0].mark(0));
    if (n) {
        HIPCHK(f, hipMemcpyAsync(f->d.xin, x4.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemcpyAsync(f->d.vin, v4.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemcpyAsync(f->d.idin, ids, 4 * (size_t)n, hipMemcpyHostToDevice, f->stream));
    }
    f->from_handle = false;
    return foam_run(f, (int)n, dt);   // (the host vectors stay alive: foam_run synchronises)
}

extern "C" int sph_foam_step_handle(SphFoam *f, SphHandle *h, double dt) {
    if (!f || !h) return SPH_ERR_INVALID;
    if (h->st.slab_active || h->swap_axis)
        return fail(f, SPH_ERR_UNSUPPORTED, "sph_foam_step_handle: sharded handle (diffuse particles run on unsharded scenes)");
    if (h->device != f->device) return fail(f, SPH_ERR_INVALID, "sph_foam_step_handle: handle on device %d, foam on %d", h->device, f->device);
    if (h->in_step) return fail(f, SPH_ERR_INVALID, "sph_foam_step_handle: between sph_step_begin and sph_step_end");
    { int rc = foam_check_dt(f, "sph_foam_step_handle", dt); if (rc) return rc; }
    HIPCHK(f, hipSetDevice(f->device));
    HIPCHK(f, hipStreamSynchronize(h->st.stream));   // the handle's last step has written the particles
    const int n_all = h->n;
    { int rc = foam_size_diffuse(f, 2 * (int64_t)std::max(h->st.cap, 1)); if (rc) return rc; }
    { int rc = foam_room_fluid(f, (size_t)n_all, (size_t)n_all); if (rc) return rc; }
    FOAM_ROOM(f, FB_HFLAG, sizeof(int) * ((size_t)n_all + 1));
    int *flag = (int *)f->buf[FB_HFLAG].p;
    HIPCHK(f, f->clk[0].mark(0));
    f->L->foam_compact(f->d, h->st.posv.cur(), h->st.velm.cur(), h->st.pid.cur(), h->st.meta.cur(), n_all, flag);
    int n = 0;
    HIPCHK(f, hipMemcpyAsync(&n, flag + n_all, sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipStreamSynchronize(f->stream));
    if (n < 0 || n > n_all) return fail(f, SPH_ERR_INVALID, "sph_foam_step_handle: internal fluid count %d of %d", n, n_all);
    f->from_handle = true;
    return foam_run(f, n, dt);
}

extern "C" int sph_foam_seed(SphFoam *f, const float *xyz, const float *vel, const float *life, int64_t n) {
    if (!f) return SPH_ERR_INVALID;
    if (n < 0 || (n > 0 && (!xyz || !vel || !life))) return fail(f, SPH_ERR_INVALID, "sph_foam_seed: bad arrays (n = %lld)", (long long)n);
    if (!f->cap) return fail(f, SPH_ERR_INVALID, "sph_foam_seed: the diffuse set has no size yet (max_diffuse = 0 and no step taken)");
    if (f->count + n > f->cap)
        return fail(f, SPH_ERR_CAPACITY, "sph_foam_seed: %lld held + %lld seeded, capacity %lld", (long long)f->count, (long long)n, (long long)f->cap);
    if (n == 0) return SPH_OK;
    HIPCHK(f, hipSetDevice(f->device));
    std::vector<float4> x4((size_t)n), v4((size_t)n);
    std::vector<unsigned long long> key((size_t)n);
    const int born = 3;
    float cls;
    memcpy(&cls, &born, 4);
    for (int64_t i = 0; i < n; ++i) {
        x4[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], life[i]);
        v4[i] = make_float4(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2], cls);
        key[i] = 0x8000000000000000ull | (f->serial + (uint64_t)i);
    }
    const size_t at = (size_t)f->count;
    HIPCHK(f, hipMemcpy(f->d.dx[0] + at, x4.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(f, hipMemcpy(f->d.dv[0] + at, v4.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(f, hipMemcpy(f->d.dkey[0] + at, key.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
    f->serial += (uint64_t)n;
    f->count += n;
    f->stats.diffuse = f->count;
    return SPH_OK;
}

extern "C" int sph_foam_count(SphFoam *f, int64_t *n) {
    if (!f || !n) return SPH_ERR_INVALID;
    *n = f->count;
    return SPH_OK;
}

extern "C" int sph_foam_download(SphFoam *f, float *xyz, float *vel, float *life, uint64_t *key, int32_t *cls) {
    if (!f) return SPH_ERR_INVALID;
    const size_t n = (size_t)f->count;
    if (n == 0) return SPH_OK;
    HIPCHK(f, hipSetDevice(f->device));
    std::vector<float4> t(n);
    if (xyz || life) {
        HIPCHK(f, hipMemcpy(t.data(), f->d.dx[0], sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (xyz) { xyz[3 * i] = t[i].x; xyz[3 * i + 1] = t[i].y; xyz[3 * i + 2] = t[i].z; }
            if (life) life[i] = t[i].w;
        }
    }
    if (vel || cls) {
        HIPCHK(f, hipMemcpy(t.data(), f->d.dv[0], sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (vel) { vel[3 * i] = t[i].x; vel[3 * i + 1] = t[i].y; vel[3 * i + 2] = t[i].z; }
            if (cls) memcpy(&cls[i], &t[i].w, 4);
        }
    }
    if (key) HIPCHK(f, hipMemcpy(key, f->d.dkey[0], 8 * n, hipMemcpyDeviceToHost));
    return SPH_OK;
}

extern "C" int sph_foam_download_potentials(SphFoam *f, float *ta, float *wc, float *e, float *nd, float *normal, int32_t *ids) {
    if (!f) return SPH_ERR_INVALID;
    if (!f->have_step) return fail(f, SPH_ERR_INVALID, "sph_foam_download_potentials: no step has been taken yet");
    const size_t n = (size_t)f->d.n;
    if (n == 0) return SPH_OK;
    HIPCHK(f, hipSetDevice(f->device));
    // grid order on the device; src[] leads back to the row of the input
    std::vector<int> src(n), id(n);
    std::vector<float4> t(n);
    HIPCHK(f, hipMemcpy(src.data(), f->d.src, 4 * n, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; ++k)
        if (src[k] < 0 || (size_t)src[k] >= n) return fail(f, SPH_ERR_INVALID, "sph_foam_download_potentials: internal source index");
    if (ta || wc || e || nd) {
        HIPCHK(f, hipMemcpy(t.data(), f->d.pot, sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; ++k) {
            const size_t i = (size_t)src[k];
            if (ta) ta[i] = t[k].x;
            if (wc) wc[i] = t[k].y;
            if (e) e[i] = t[k].z;
            if (nd) nd[i] = t[k].w;
        }
    }
    if (normal) {
        HIPCHK(f, hipMemcpy(t.data(), f->d.nrm, sizeof(float4) * n, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; ++k) {
            const size_t i = (size_t)src[k];
            normal[3 * i] = t[k].x; normal[3 * i + 1] = t[k].y; normal[3 * i + 2] = t[k].z;
        }
    }
    if (ids) {
        HIPCHK(f, hipMemcpy(id.data(), f->d.ids, 4 * n, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; ++k) ids[src[k]] = id[k];
    }
    return SPH_OK;
}

extern "C" int sph_foam_clear(SphFoam *f) {
    if (!f) return SPH_ERR_INVALID;
    f->count = 0;
    f->stats.diffuse = f->stats.spray = f->stats.foam = f->stats.bubble = 0;
    return SPH_OK;
}

extern "C" int sph_foam_stats(SphFoam *f, SphFoamStats *out) {
    if (!f || !out) return SPH_ERR_INVALID;
    *out = f->stats;
    out->bytes_allocated = (int64_t)foam_total(f);
    return SPH_OK;
}

// --- the renderer's hook (sph_render_api.hpp: SphRender::foam) ------------------------------------------------------------------------------
extern "C" int sph_render_set_foam(SphRender *r, SphFoam *foam, double radius_scale, const uint8_t *rgb_spray, const uint8_t *rgb_foam,
                                   const uint8_t *rgb_bubble) {
    if (!r) return SPH_ERR_INVALID;
    if (!foam) { r->foam = nullptr; return SPH_OK; }
    if (r->surf_on)
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_set_foam: the surface mode is on (diffuse particles are drawn into particle frames only; "
                                            "sph_render_set_surface_foam draws them into surface frames)");
    if (foam->device != r->device) return fail(r, SPH_ERR_INVALID, "sph_render_set_foam: foam on device %d, renderer on %d", foam->device, r->device);
    if (!(radius_scale > 0.0) || !std::isfinite(radius_scale) || !((float)(radius_scale * r->prm.radius) > 0.0f))
        return fail(r, SPH_ERR_INVALID, "sph_render_set_foam: radius_scale %g must be positive and finite", radius_scale);
    static const uint8_t def[3][3] = {{250, 250, 255}, {255, 255, 255}, {225, 235, 250}};
    const uint8_t *c[3] = {rgb_spray ? rgb_spray : def[0], rgb_foam ? rgb_foam : def[1], rgb_bubble ? rgb_bubble : def[2]};
    for (int k = 0; k < 3; ++k) r->foam_rgb[k] = (unsigned)c[k][0] | (unsigned)c[k][1] << 8 | (unsigned)c[k][2] << 16;
    r->foam_scale = radius_scale;
    r->foam = foam;
    return SPH_OK;
}

// The diffuse set as a layer of its own -- the splat and shade passes on the layer planes with the diffuse particles as their source --
// folded into the frame just drawn, and the pixels finished again.  Called by sph_render_handle behind rend_run (which has synchronised).
static int rend_draw_foam(SphRender *r, SphFoam *f, double scale, const unsigned rgb[3]) {
    const int n = (int)f->count;
    if (n == 0) return SPH_OK;
    const size_t px = (size_t)r->d.W * r->d.H;
    { int rc = rend_layer_room(r); if (rc) return rc; }
    { int rc = r->buf[RB_FID].reserve(r, 4 * (size_t)n); if (rc) return rc; }
    { int rc = r->buf[RB_FCOL].reserve(r, 4 * (size_t)n); if (rc) return rc; }
    { int rc = r->buf[RB_FCNT].reserve(r, 64); if (rc) return rc; }
    { int rc = r->buf[RB_LARGE].reserve(r, 4 * (size_t)std::max(n, r->d.n)); if (rc) return rc; }
    r->d.large = (int *)r->buf[RB_LARGE].p;
    FoamDev src = f->d;
    src.stream = r->stream;   // (the foam's own stream is idle: its calls are synchronous)
    r->L->foam_render_source(src, n, (int *)r->buf[RB_FID].p, (unsigned *)r->buf[RB_FCOL].p, rgb);
    RenderDev l = r->d;
    l.key = (unsigned long long *)r->buf[RB_LKEY].p; l.rgb = (unsigned char *)r->buf[RB_LRGB].p;
    l.cnt = (unsigned long long *)r->buf[RB_FCNT].p;
    l.n = n; l.pos = f->d.dx[0]; l.meta = nullptr; l.id = (const int *)r->buf[RB_FID].p; l.col = (const unsigned *)r->buf[RB_FCOL].p;
    l.col_home = nullptr; l.mask = ~0u;
    l.ids = nullptr;   // (the id image is written when the merged frame is finished)
    const double rad = scale * r->prm.radius;
    l.r = (float)rad; l.r2 = (float)(rad * rad);
    l.draw_box = 0;
    for (int e = 0; e < 12; ++e) l.line_axis[e] = -1;
    HIPCHK(r, hipMemsetAsync(l.key, 0xff, px * 8, r->stream));
    HIPCHK(r, hipMemsetAsync(l.cnt, 0, 64, r->stream));
    r->L->render_splat(l);
    r->L->render_shade(l);
    rend_merge_incoming(r);
    return rend_refinish(r);
}

// --- diffuse particles in the surface frames: the kernels are in sph_render_foam.hpp ---------------------------------------
static const uint8_t RFOAM_CLASS_RGB[3][3] = {{250, 250, 255}, {255, 255, 255}, {225, 235, 250}};   // sph_render_set_foam's defaults

extern "C" int sph_render_set_surface_foam(SphRender *r, SphFoam *foam, const SphRenderSurfaceFoamParams *params) {
    if (!r) return SPH_ERR_INVALID;
    // (a frame whose raw spheres are merged in no longer matches its base plane without the copies: sph_render_surface refuses it)
    if (!foam) { if (r->sfoam_valid && r->fprm.raw_spheres) r->base_valid = false; r->sfoam = nullptr; r->sfoam_valid = false; return SPH_OK; }
    SphRenderSurfaceFoamParams p{};
    p.radius_scale = 0.5; p.density = 1.0; p.depth_bias = 1.0; p.rgb[0] = p.rgb[1] = p.rgb[2] = 255; p.raw_spheres = 1;
    if (params) p = *params;
    if (!r->surf_on) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface_foam: the surface mode is off (sph_render_set_surface)");
    if (r->foam)
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_set_surface_foam: diffuse particles are set for the particle frames (sph_render_set_foam): clear them first");
    if (foam->device != r->device) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface_foam: foam on device %d, renderer on %d", foam->device, r->device);
    if (!(p.radius_scale > 0.0) || !std::isfinite(p.radius_scale) || !((float)(p.radius_scale * r->prm.radius) > 0.0f) ||
        !std::isfinite((float)(p.radius_scale * r->prm.radius)))
        return fail(r, SPH_ERR_INVALID, "sph_render_set_surface_foam: radius_scale %g must be positive and finite", p.radius_scale);
    if (!(p.density >= 0.0) || !std::isfinite(p.density) || !std::isfinite((float)p.density))
        return fail(r, SPH_ERR_INVALID, "sph_render_set_surface_foam: density %g must be finite and not negative", p.density);
    if (!(p.depth_bias >= 0.0) || !std::isfinite(p.depth_bias) || !std::isfinite((float)(p.depth_bias * (double)r->d.r)))
        return fail(r, SPH_ERR_INVALID, "sph_render_set_surface_foam: depth_bias %g must be finite and not negative", p.depth_bias);
    if (p.reserved != 0) return fail(r, SPH_ERR_INVALID, "sph_render_set_surface_foam: reserved must be 0");
    p.raw_spheres = p.raw_spheres ? 1 : 0;
    if (r->sfoam != foam || memcmp(&p, &r->fprm, sizeof(p)) != 0) {   // the frame held has no planes for these
        if (r->sfoam_valid && r->fprm.raw_spheres) r->base_valid = false;
        r->sfoam_valid = false;
    }
    r->fprm = p;
    r->sfoam = foam;
    return SPH_OK;
}

// what sph_render_handle refuses before anything is launched
static int rend_surface_foam_check(SphRender *r, SphHandle *h) {
    if (h->st.slab_active)
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_handle: diffuse particles are set (sph_render_set_surface_foam): no sharded handle");
    if (!r->surf_on) { r->sfoam = nullptr; return SPH_OK; }   // (sph_render_set_surface(NULL) clears it: not reached)
    const double per = ceil(512.0 * r->fprm.radius_scale);
    if ((double)r->sfoam->count * per >= 4294967296.0)
        return fail(r, SPH_ERR_UNSUPPORTED, "sph_render_set_surface_foam: %lld diffuse particles of at most %.0f units each (radius_scale %g): a pixel's u32 "
                                            "holds fewer than 2^32", (long long)r->sfoam->count, per, r->fprm.radius_scale);
    if (r->fprm.raw_spheres && (int64_t)h->st.cap > (int64_t)INT_MAX)
        return fail(r, SPH_ERR_INVALID, "sph_render_handle: particle ids reach 2^31, diffuse ids could not be told from them (raw_spheres)");
    return SPH_OK;
}

// behind rend_run (which has synchronised): the three planes from the diffuse set as it is now, then -- raw_spheres -- section 26's layer
// folded into the particle frame, whose key and rgb planes are copied first
static int rend_surface_foam_draw(SphRender *r) {
    SphFoam *f = r->sfoam;
    const SphRenderSurfaceFoamParams &p = r->fprm;
    const int n = (int)f->count;
    const size_t px = (size_t)r->d.W * r->d.H;
    DevBuf *b = r->buf;
    int rc = b[RB_WFO].reserve(r, px * 4);
    if (!rc) rc = b[RB_WFU].reserve(r, px * 4);
    if (!rc) rc = b[RB_WDU].reserve(r, px * 4);
    if (!rc) rc = b[RB_WCNT].reserve(r, 2 * RSURF_CNT_BANKS * 64);
    if (!rc) rc = b[RB_WLARGE].reserve(r, 4 * (size_t)std::max(n, 1));
    if (!rc) rc = b[RB_WNL].reserve(r, 64);
    if (!rc) rc = b[RB_WRGB0].reserve(r, px * 3);
    if (!rc && p.raw_spheres) rc = b[RB_WKEY0].reserve(r, px * 8);
    if (rc) return rc;
    if (!r->fclk.stream) {
        for (hipEvent_t &e : r->fclk.ev) HIPCHK(r, hipEventCreate(&e));
        r->fclk.stream = r->stream;
    }
    const bool thick = r->thick_on;
    const double rad = p.radius_scale * r->prm.radius;
    RenderFoamDev &w = r->fd;
    w.n = n; w.pos = f->d.dx[0];
    w.large = (int *)b[RB_WLARGE].p; w.nlarge = (unsigned long long *)b[RB_WNL].p;
    w.fo = (unsigned *)b[RB_WFO].p; w.fu = (unsigned *)b[RB_WFU].p; w.du = (unsigned *)b[RB_WDU].p;
    w.cnt = (unsigned long long *)b[RB_WCNT].p;
    w.rf = (float)rad; w.rf2 = (float)(rad * rad);
    w.bias = (float)(p.depth_bias * (double)r->d.r);
    w.density = (float)p.density;
    w.rgb = (unsigned)p.rgb[0] | (unsigned)p.rgb[1] << 8 | (unsigned)p.rgb[2] << 16;
    w.key0 = r->d.key;
    w.okey = thick ? r->td.okey : nullptr;
    HIPCHK(r, r->fclk.mark(0));
    HIPCHK(r, hipMemcpyAsync(b[RB_WRGB0].p, r->d.rgb, px * 3, hipMemcpyDeviceToDevice, r->stream));
    if (p.raw_spheres) {
        HIPCHK(r, hipMemcpyAsync(b[RB_WKEY0].p, r->d.key, px * 8, hipMemcpyDeviceToDevice, r->stream));
        w.key0 = (const unsigned long long *)b[RB_WKEY0].p;
    }
    r->L->render_foam_splat(r->d, r->sd, w);   // (the foam's own stream is idle: its calls are synchronous)
    HIPCHK(r, r->fclk.mark(1));
    unsigned long long bank[RSURF_CNT_BANKS][8], nl = 0;
    HIPCHK(r, hipMemcpyAsync(bank, w.cnt, sizeof(bank), hipMemcpyDeviceToHost, r->stream));
    HIPCHK(r, hipMemcpyAsync(&nl, w.nlarge, 8, hipMemcpyDeviceToHost, r->stream));
    HIPCHK(r, hipStreamSynchronize(r->stream));
    HIPCHK(r, hipGetLastError());
    if (p.raw_spheres) {
        unsigned cls[3];
        for (int k = 0; k < 3; ++k) cls[k] = (unsigned)RFOAM_CLASS_RGB[k][0] | (unsigned)RFOAM_CLASS_RGB[k][1] << 8 | (unsigned)RFOAM_CLASS_RGB[k][2] << 16;
        const int rcd = rend_draw_foam(r, f, p.radius_scale, cls);
        if (rcd) return rcd;
    }
    HIPCHK(r, r->fclk.mark(2));
    HIPCHK(r, hipStreamSynchronize(r->stream));
    SphRenderSurfaceFoamStats &o = r->fstats;
    o = SphRenderSurfaceFoamStats{};
    o.diffuse = n; o.large = (int64_t)nl;
    for (int k = 0; k < RSURF_CNT_BANKS; ++k) {
        o.adds_over += (int64_t)bank[k][0]; o.adds_under += (int64_t)bank[k][1]; o.clipped += (int64_t)bank[k][2]; o.removed += (int64_t)bank[k][3];
    }
    o.ms_splat = r->fclk.ms(0, 1); o.ms_raw = r->fclk.ms(1, 2);
    r->sfoam_valid = true;
    r->sfoam_thick = thick;
    return SPH_OK;
}

extern "C" int sph_render_surface_download_foam(SphRender *r, int plane, uint32_t *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    if (plane < 0 || plane > 2) return fail(r, SPH_ERR_INVALID, "sph_render_surface_download_foam: plane %d is none of 0 (fo), 1 (fu), 2 (du)", plane);
    if (r->frame != RF_PARTICLE || !r->sfoam_valid)
        return fail(r, SPH_ERR_INVALID, "sph_render_surface_download_foam: no frame with diffuse particles is held (sph_render_set_surface_foam, sph_render_handle)");
    HIPCHK(r, hipSetDevice(r->device));
    const unsigned *src = plane == 0 ? r->fd.fo : plane == 1 ? r->fd.fu : r->fd.du;
    HIPCHK(r, hipMemcpy(out, src, (size_t)r->d.W * r->d.H * 4, hipMemcpyDeviceToHost));
    return SPH_OK;
}

extern "C" int sph_render_surface_foam_stats(SphRender *r, SphRenderSurfaceFoamStats *out) {
    if (!r || !out) return SPH_ERR_INVALID;
    *out = r->fstats;
    return SPH_OK;
}
