// sph_elastic_api.hpp -- elastic solids, host side: marking, the deferred capture, the C-ABI entries and the four fields; included by
// sph_api.hip in front of ph_neighbor_search.  Kernels and arithmetic: sph_elastic.hpp; semantics: include/sph_hip.h
// (sph_set_elastic_object); design: DESIGN.md 34.
#pragma once
#include "sph_elastic.hpp"

static_assert(ELASTIC_MAX_NEIGHBOURS == SPH_ELASTIC_MAX_NEIGHBOURS, "sph_hip.h and sph_elastic.hpp disagree on the list length");

static void el_lame(double E, double nu, double *mu, double *lambda) {
    *mu = E / (2.0 * (1.0 + nu));
    *lambda = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu));
}

// the home arrays, allocated when the first object is marked (dalloc clears).  Each array on its own: a call that failed part-way
// leaves the rest to the next one, and nothing is launched before every array exists (no object is marked when this fails)
static int el_allocate(SphHandle *h) {
    State &s = h->st;
    const size_t cap = (size_t)s.cap;
    int rc;
    if (!s.el_x_home && (rc = dalloc(h, &s.el_x_home, cap))) return rc;
    if (!s.el_slot_home && (rc = dalloc(h, &s.el_slot_home, cap))) return rc;
    if (!s.el_q[0] && (rc = dalloc(h, &s.el_q[0], cap))) return rc;
    if (!s.el_q[1] && (rc = dalloc(h, &s.el_q[1], cap))) return rc;
    if (!s.el_sig && (rc = dalloc(h, &s.el_sig, 2 * cap))) return rc;
    if (!s.el_F && (rc = dalloc(h, &s.el_F, 3 * cap))) return rc;
    if (!s.el_acc && (rc = dalloc(h, &s.el_acc, cap))) return rc;
    if (!s.el_cnt && (rc = dalloc(h, &s.el_cnt, (size_t)4))) return rc;
    return SPH_OK;
}

extern "C" int sph_set_elastic_object(SphHandle *h, int o, const SphElasticParams *p) {
    if (!h) return SPH_ERR_INVALID;
    if (!p) return fail(h, SPH_ERR_INVALID, "sph_set_elastic_object: null argument");
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_elastic_object: not on a PBF handle (either variant)");
    if (h->st.slab_active || h->comm.slab_ready)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_elastic_object: not on a sharded handle (the rest lists name particles by id across every slab)");
    if (o < 0 || o >= SPH_NOBJ) return fail(h, SPH_ERR_INVALID, "sph_set_elastic_object: unknown object %d", o);
    if (h->of_n > 0 || h->of_removed_any)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_elastic_object: object %d: an outflow volume is set or particles have been removed (a rest list names particles that must not leave)", o);
    if (em_of_object(h, o) >= 0)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_elastic_object: object %d belongs to emitter %d (a growing object has no rest configuration)", o, em_of_object(h, o));
    if (!(p->youngs_modulus > 0.0) || !std::isfinite(p->youngs_modulus))
        return fail(h, SPH_ERR_INVALID, "sph_set_elastic_object: object %d: Young's modulus %g is not a finite number > 0", o, p->youngs_modulus);
    if (!(p->poisson_ratio >= 0.0 && p->poisson_ratio <= 0.49))
        return fail(h, SPH_ERR_INVALID, "sph_set_elastic_object: object %d: Poisson's ratio %g is outside [0, 0.49]", o, p->poisson_ratio);
    if (h->pose_h.material[o] != SPH_MAT_FLUID)
        return fail(h, SPH_ERR_INVALID, "sph_set_elastic_object: object %d is not a fluid object (sph_set_object)", o);
    State &s = h->st;
    ElObjHost &e = h->el[o];
    if (e.state != 2 && s.ids_custom)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_elastic_object: particle ids were set from outside (sph_set_appended_ids / SPH_F_PARTICLE_ID): "
                                            "the rest lists are stored by id and need the append order");
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = el_allocate(h); if (rc) return rc; }
    e.E = p->youngs_modulus; e.nu = p->poisson_ratio;
    if (e.state == 2) {   // captured: the parameters alone
        double mu, lambda;
        el_lame(e.E, e.nu, &mu, &lambda);
        s.el_obj[e.slot].mu = (float)mu; s.el_obj[e.slot].lambda = (float)lambda;
        return SPH_OK;
    }
    if (e.state == 0 || e.state == 3) { s.el_marked++; s.el_pending++; }
    e.state = 1;
    return SPH_OK;
}

extern "C" int sph_get_elastic_object(SphHandle *h, int o, SphElasticObjectInfo *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    if (o < 0 || o >= SPH_NOBJ) return fail(h, SPH_ERR_INVALID, "sph_get_elastic_object: unknown object %d", o);
    const ElObjHost &e = h->el[o];
    out->captured = e.state;
    out->count = e.state == 2 ? e.n : h->obj_n[o];
    out->first_id = e.state == 2 ? e.id0 : h->obj_first[o];
    out->longest_list = e.longest;
    out->min_eig_ratio = e.min_ratio;
    out->params.youngs_modulus = e.E; out->params.poisson_ratio = e.nu;
    return SPH_OK;
}

// a marked object whose particles are here: the sort that is about to run captures it
static bool el_capture_due(SphHandle *h) {
    for (int o = 0; o < SPH_NOBJ; ++o)
        if (h->el[o].state == 1 && h->obj_n[o] > 0) return true;
    return false;
}

// the object is refused: it stays plain fluid
static int el_refuse(SphHandle *h, int o, int rc) {
    h->el[o].state = 3;
    h->st.el_marked--; h->st.el_pending--;
    return rc;
}

// One object on the cell lists of the sort that has just run: scatter, lists + M + g0_ij, g0_ji; ONE synchronisation, then the
// counters decide.  The kernels fill a table of all ELASTIC_MAX_NEIGHBOURS entries; what the object keeps is its first `longest` ones.
static int el_capture_object(SphHandle *h, int o) {
    State &s = h->st;
    ElObjHost &e = h->el[o];
    if (h->obj_split[o])
        return el_refuse(h, o, fail(h, SPH_ERR_UNSUPPORTED, "elastic object %d: its particle ids are not one contiguous append range", o));
    const int n = h->obj_n[o], id0 = h->obj_first[o];
    float4 *tmp = nullptr;
    {   // (2 KiB per particle, for the length of this call: an object that does not fit is refused like any other failure, not retried)
        const hipError_t e0 = hipMalloc((void **)&tmp, (size_t)2 * ELASTIC_MAX_NEIGHBOURS * (size_t)n * sizeof(float4));
        if (e0 != hipSuccess) {
            (void)hipGetLastError();
            return el_refuse(h, o, fail(h, SPH_ERR_HIP, "elastic object %d: no memory for the capture's table of %d particles: %s", o, n, hipGetErrorString(e0)));
        }
    }
    const unsigned init[4] = {0u, 0u, 0x7f800000u, 0u};
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    hipError_t err = hipMemcpyAsync(s.el_cnt, init, sizeof(init), hipMemcpyHostToDevice, s.stream);
    if (err == hipSuccess) {
        ProfScope p(h, SPH_K_MISC);
        h->L->elastic_capture(s, ElCaptureArgs{o, id0, n, tmp, s.el_cnt});
    }
    if (err == hipSuccess) err = hipMemcpyAsync(cnt, s.el_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(s.stream);
    if (err != hipSuccess) { hipFree(tmp); return el_refuse(h, o, fail(h, SPH_ERR_HIP, "elastic object %d: capture failed: %s", o, hipGetErrorString(err))); }
    float ratio;
    memcpy(&ratio, &cnt[2], sizeof(float));
    e.longest = (int)cnt[0]; e.min_ratio = ratio; e.n = n; e.id0 = id0;
    int rc = SPH_OK;
    if (cnt[0] > (unsigned)ELASTIC_MAX_NEIGHBOURS)
        rc = fail(h, SPH_ERR_CAPACITY, "elastic object %d: a rest list of %u neighbours exceeds %d entries (no list is truncated); sample the object coarser", o, cnt[0], ELASTIC_MAX_NEIGHBOURS);
    else if (cnt[3])
        rc = fail(h, SPH_ERR_INVALID, "elastic object %d: %u inconsistent list entries (an id outside the object's range, or a neighbour that does not list the particle back)", o, cnt[3]);
    else if (cnt[1])
        rc = fail(h, SPH_ERR_INVALID, "elastic object %d: %u degenerate particles (smallest eigenvalue of M below %g of the largest: a sheet, or fewer than three non-coplanar neighbours)", o, cnt[1], (double)ELASTIC_MIN_EIG_RATIO);
    if (rc) { hipFree(tmp); return el_refuse(h, o, rc); }
    const size_t keep = (size_t)2 * (size_t)e.longest * (size_t)n;
    float4 *rest = nullptr;
    err = hipMalloc((void **)&rest, (keep ? keep : 1) * sizeof(float4));
    if (err == hipSuccess && keep) err = hipMemcpy(rest, tmp, keep * sizeof(float4), hipMemcpyDeviceToDevice);
    hipFree(tmp);
    if (err != hipSuccess) { if (rest) hipFree(rest); return el_refuse(h, o, fail(h, SPH_ERR_HIP, "elastic object %d: %s", o, hipGetErrorString(err))); }
    h->allocs.push_back(rest);
    e.rest = rest;
    double mu, lambda;
    el_lame(e.E, e.nu, &mu, &lambda);
    e.slot = s.el_nobj;
    s.el_obj[s.el_nobj++] = ElObjDev{id0, n, e.longest, (float)mu, (float)lambda, rest};
    s.el_mask |= 1u << o;
    s.el_pending--;
    e.state = 2;
    return SPH_OK;
}

// every marked object whose particles are here; the first error is the one the searching call returns
static int el_capture_pending(SphHandle *h) {
    int first = SPH_OK;
    h->st.c.n = h->n;
    for (int o = 0; o < SPH_NOBJ; ++o) {
        if (h->el[o].state != 1 || h->obj_n[o] <= 0) continue;
        const int rc = el_capture_object(h, o);
        if (rc && !first) first = rc;
    }
    return first;
}

extern "C" int sph_get_elastic_rest(SphHandle *h, int o, int32_t *nbr, float *g0_ij, float *g0_ji) {
    if (!h || !nbr || !g0_ij || !g0_ji) return fail(h, SPH_ERR_INVALID, "sph_get_elastic_rest: null argument");
    if (o < 0 || o >= SPH_NOBJ || h->el[o].state != 2) return fail(h, SPH_ERR_INVALID, "sph_get_elastic_rest: object %d has no captured rest configuration", o);
    const ElObjHost &e = h->el[o];
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    const size_t n = (size_t)e.n, K = ELASTIC_MAX_NEIGHBOURS;
    std::vector<float4> t((size_t)2 * (size_t)e.longest * n);
    if (!t.empty()) HIPCHK(h, hipMemcpy(t.data(), e.rest, t.size() * sizeof(float4), hipMemcpyDeviceToHost));
    const int ix0 = h->inv[0], ix1 = h->inv[1], ix2 = h->inv[2];   // library frame -> scene frame
    for (size_t r = 0; r < n; ++r)
        for (size_t k = 0; k < K; ++k) {
            int32_t j = -1;
            float a[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
            if (k < (size_t)e.longest) {
                const float4 p0 = t[(2 * k) * n + r], p1 = t[(2 * k + 1) * n + r];
                memcpy(&j, &p0.w, 4);
                if (j >= 0) { a[0] = p0.x; a[1] = p0.y; a[2] = p0.z; b[0] = p1.x; b[1] = p1.y; b[2] = p1.z; }
                else j = -1;
            }
            nbr[r * K + k] = j;
            float *ga = g0_ij + 3 * (r * K + k), *gb = g0_ji + 3 * (r * K + k);
            ga[0] = a[ix0]; ga[1] = a[ix1]; ga[2] = a[ix2];
            gb[0] = b[ix0]; gb[1] = b[ix1]; gb[2] = b[ix2];
        }
    return SPH_OK;
}

extern "C" int sph_elastic_particle_host(int nnb, const float *xi, const float *xj, const float *g0_ij, const float *g0_ji, const float *q_prev,
                                         const float *q_j, const float *sigma_j, double V0, double mass, double mu, double lambda,
                                         float *F_out, float *q_out, float *sigma_out, float *a_out, int fast) {
    if (nnb < 0 || nnb > ELASTIC_MAX_NEIGHBOURS) return fail(nullptr, SPH_ERR_INVALID, "sph_elastic_particle_host: %d list entries (0 .. %d)", nnb, ELASTIC_MAX_NEIGHBOURS);
    if (!xi || !q_prev || !F_out || !q_out || !sigma_out || !a_out || (nnb > 0 && (!xj || !g0_ij || !g0_ji || !q_j || !sigma_j)))
        return fail(nullptr, SPH_ERR_INVALID, "sph_elastic_particle_host: null argument");
    const float v0 = (float)V0;
    float F[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < nnb; ++k) {   // pass A (k_elastic_rotation)
        const float dx = xj[3 * k] - xi[0], dy = xj[3 * k + 1] - xi[1], dz = xj[3 * k + 2] - xi[2];
        if (fast) el_deformation_entry<true>(F, v0, dx, dy, dz, g0_ij[3 * k], g0_ij[3 * k + 1], g0_ij[3 * k + 2]);
        else el_deformation_entry<false>(F, v0, dx, dy, dz, g0_ij[3 * k], g0_ij[3 * k + 1], g0_ij[3 * k + 2]);
    }
    float q[4] = {q_prev[0], q_prev[1], q_prev[2], q_prev[3]}, R[9], sig[6];
    el_extract_rotation(q, F, ELASTIC_ROT_ITERS);
    el_quat_matrix(q, R);
    el_stress(F, R, (float)mu, (float)lambda, sig);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < nnb; ++k) {   // pass B (k_elastic_force)
        float Rj[9];
        el_quat_matrix(q_j + 4 * k, Rj);
        el_pair_force(acc, sig, R, g0_ij + 3 * k, sigma_j + 6 * k, Rj, g0_ji + 3 * k);
    }
    const float coef = (v0 * v0) / (float)mass;
    memcpy(F_out, F, sizeof(F)); memcpy(q_out, q, sizeof(q)); memcpy(sigma_out, sig, sizeof(sig));
    a_out[0] = coef * acc[0]; a_out[1] = coef * acc[1]; a_out[2] = coef * acc[2];
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- the four fields (current order; zero outside captured objects)
struct ElRows { std::vector<int> id, mt; };
static int el_rows(SphHandle *h, ElRows &r) {
    State &s = h->st;
    const size_t n = (size_t)h->n;
    r.id.resize(n); r.mt.resize(n);
    HIPCHK(h, hipStreamSynchronize(s.stream));
    if (n) {
        HIPCHK(h, hipMemcpy(r.id.data(), s.pid.cur(), n * 4, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(r.mt.data(), s.meta.cur(), n * 4, hipMemcpyDeviceToHost));
    }
    return SPH_OK;
}
static inline bool el_row_on(const SphHandle *h, int meta, int id) {
    const int o = META_OBJ(meta);
    return o >= 0 && o < SPH_NOBJ && ((h->st.el_mask >> o) & 1u) && id >= 0 && id < h->st.cap;
}

static int el_download(SphHandle *h, int field, float *d, size_t bytes) {
    State &s = h->st;
    if (!s.el_cnt) return fail(h, SPH_ERR_UNSUPPORTED, "download: field %d not allocated (sph_set_elastic_object)", field);
    const size_t n = (size_t)h->n, cap = (size_t)s.cap;
    const int comps = field == SPH_F_ELASTIC_ACCEL ? 3 : field == SPH_F_ELASTIC_DEFGRAD ? 9 : field == SPH_F_ELASTIC_STRESS ? 6 : 4;
    if (bytes != n * (size_t)comps * 4) return fail(h, SPH_ERR_INVALID, "download: field %d needs %zu bytes, got %zu", field, n * (size_t)comps * 4, bytes);
    HIPCHK(h, hipSetDevice(h->device));
    ElRows r;
    { int rc = el_rows(h, r); if (rc) return rc; }
    memset(d, 0, bytes);
    const int *iv = h->inv;   // scene axis k = library axis inv[k]
    if (field == SPH_F_ELASTIC_ACCEL) {
        std::vector<float4> a(n);
        if (n) HIPCHK(h, hipMemcpy(a.data(), s.el_acc, n * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (!el_row_on(h, r.mt[i], r.id[i])) continue;
            const float v[3] = {a[i].x, a[i].y, a[i].z};
            for (int k = 0; k < 3; ++k) d[3 * i + k] = v[iv[k]];
        }
    } else if (field == SPH_F_ELASTIC_ROTATION) {
        std::vector<float4> q(cap);
        HIPCHK(h, hipMemcpy(q.data(), s.el_q[s.el_qi], cap * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (!el_row_on(h, r.mt[i], r.id[i])) continue;
            const float4 w = q[(size_t)r.id[i]];
            const float v[3] = {w.x, w.y, w.z};
            for (int k = 0; k < 3; ++k) d[4 * i + k] = h->axial * v[iv[k]];
            d[4 * i + 3] = w.w;
        }
    } else if (field == SPH_F_ELASTIC_DEFGRAD) {
        std::vector<float4> F(3 * cap);
        HIPCHK(h, hipMemcpy(F.data(), s.el_F, 3 * cap * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (!el_row_on(h, r.mt[i], r.id[i])) continue;
            const float4 *f = &F[3 * (size_t)r.id[i]];
            const float m[3][3] = {{f[0].x, f[0].y, f[0].z}, {f[1].x, f[1].y, f[1].z}, {f[2].x, f[2].y, f[2].z}};
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) d[9 * i + 3 * a + b] = m[iv[a]][iv[b]];
        }
    } else {
        std::vector<float4> S(2 * cap);
        HIPCHK(h, hipMemcpy(S.data(), s.el_sig, 2 * cap * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (!el_row_on(h, r.mt[i], r.id[i])) continue;
            const float4 s0 = S[2 * (size_t)r.id[i]], s1 = S[2 * (size_t)r.id[i] + 1];
            const float m[3][3] = {{s0.x, s0.y, s0.z}, {s0.y, s0.w, s1.x}, {s0.z, s1.x, s1.y}};
            float *o = d + 6 * i;
            o[0] = m[iv[0]][iv[0]]; o[1] = m[iv[0]][iv[1]]; o[2] = m[iv[0]][iv[2]];
            o[3] = m[iv[1]][iv[1]]; o[4] = m[iv[1]][iv[2]]; o[5] = m[iv[2]][iv[2]];
        }
    }
    return SPH_OK;
}

// the warm start of the next pass A, rows of captured elastic objects only
static int el_upload_rotation(SphHandle *h, const float *f, size_t bytes) {
    State &s = h->st;
    if (!s.el_cnt) return fail(h, SPH_ERR_UNSUPPORTED, "upload: field %d not allocated (sph_set_elastic_object)", (int)SPH_F_ELASTIC_ROTATION);
    const size_t n = (size_t)h->n, cap = (size_t)s.cap;
    if (bytes != n * 16) return fail(h, SPH_ERR_INVALID, "upload: field %d needs %zu bytes", (int)SPH_F_ELASTIC_ROTATION, n * 16);
    HIPCHK(h, hipSetDevice(h->device));
    ElRows r;
    { int rc = el_rows(h, r); if (rc) return rc; }
    std::vector<float4> q(cap);
    HIPCHK(h, hipMemcpy(q.data(), s.el_q[s.el_qi], cap * sizeof(float4), hipMemcpyDeviceToHost));
    const int *pm = h->perm;   // library axis k = scene axis perm[k]
    for (size_t i = 0; i < n; ++i) {
        if (!el_row_on(h, r.mt[i], r.id[i])) continue;
        q[(size_t)r.id[i]] = make_float4(h->axial * f[4 * i + pm[0]], h->axial * f[4 * i + pm[1]], h->axial * f[4 * i + pm[2]], f[4 * i + 3]);
    }
    HIPCHK(h, hipMemcpy(s.el_q[s.el_qi], q.data(), cap * sizeof(float4), hipMemcpyHostToDevice));
    return SPH_OK;
}
