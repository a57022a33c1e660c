// sph_outflow_api.hpp -- outflow, host side (include/sph_hip.h sph_set_outflow): the entry points, the slot of a step that
// marks and counts, and the bookkeeping of the sort that drops the dead.  Included by sph_api.hip.  The time window is evaluated HERE,
// with the kernel's own source (sph_outflow_eval.hpp); the counts come back from the device: one copy of the counters into pinned
// memory and one stream wait per slot while a volume is active.
#pragma once
#include <algorithm>

static int outflow_check(SphHandle *h, const char *who, int index, const SphOutflow *v) {
#define OF_FAIL(...) return fail(h, SPH_ERR_INVALID, __VA_ARGS__)
    if (v->shape != SPH_OUTFLOW_BOX && v->shape != SPH_OUTFLOW_SPHERE) OF_FAIL("%s: outflow %d: shape %d is neither 0 (box) nor 1 (sphere)", who, index, v->shape);
    if (v->shape == SPH_OUTFLOW_BOX) {
        for (int c = 0; c < 3; ++c) {
            if (!std::isfinite(v->min[c]) || !std::isfinite(v->max[c])) OF_FAIL("%s: outflow %d: min / max: a component is not finite", who, index);
            if (!((float)v->min[c] < (float)v->max[c])) OF_FAIL("%s: outflow %d: min %g >= max %g in component %d", who, index, v->min[c], v->max[c], c);
        }
    } else {
        for (int c = 0; c < 3; ++c) if (!std::isfinite(v->center[c])) OF_FAIL("%s: outflow %d: center: a component is not finite", who, index);
        if (!((float)v->radius > 0.0f) || !std::isfinite(v->radius)) OF_FAIL("%s: outflow %d: radius %g is not positive and finite", who, index, v->radius);
    }
    if (!std::isfinite(v->start) || std::isnan(v->end) || !(v->end > v->start)) OF_FAIL("%s: outflow %d: end %g <= start %g", who, index, v->end, v->start);
    if (v->n_objects < 0 || v->n_objects > SPH_OUTFLOW_MAX_OBJECTS) OF_FAIL("%s: outflow %d: n_objects %d outside 0..%d", who, index, v->n_objects, SPH_OUTFLOW_MAX_OBJECTS);
    for (int k = 0; k < v->n_objects; ++k) {
        const int o = v->objects[k];
        if (o < 0 || o >= SPH_NOBJ) OF_FAIL("%s: outflow %d: objects[%d] = %d outside 0..%d", who, index, k, o, SPH_NOBJ - 1);
        if (h && h->pose_h.material[o] != SPH_MAT_FLUID) OF_FAIL("%s: outflow %d: objects[%d] = %d is not a fluid object (sph_set_object)", who, index, k, o);
    }
    if (v->reserved != 0) OF_FAIL("%s: outflow %d: reserved must be 0", who, index);
#undef OF_FAIL
    return SPH_OK;
}

// what a handle must be for particles to leave it (sph_set_outflow and sph_remove_particles)
static int outflow_supported(SphHandle *h, const char *who) {
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "%s: not on a PBF handle (either variant: its step has no insertion slot)", who);
    if (h->st.slab_active || h->comm.slab_ready) return fail(h, SPH_ERR_UNSUPPORTED, "%s: not on a sharded handle (the graveyard cells are the slab exchange's there)", who);
    if (h->prm.g_upper < 9999.0) return fail(h, SPH_ERR_UNSUPPORTED, "%s: not with g_upper set (gravitationUpper, the reference's frozen-block emitter)", who);
    // (today only sph_comm_set_slab permutes the axes, and a sharded handle has been refused above: this keeps the contract should
    //  another entry ever set an axis order)
    if (h->swap_axis) return fail(h, SPH_ERR_UNSUPPORTED, "%s: the handle's axis order is not \"xyz\"", who);
    if (h->st.ids_custom) return fail(h, SPH_ERR_UNSUPPORTED, "%s: particle ids were set from outside (sph_set_appended_ids / SPH_F_PARTICLE_ID): new ids come from the library's own counter", who);
    if (h->st.el_marked) return fail(h, SPH_ERR_UNSUPPORTED, "%s: an elastic object is present (its rest lists name particles that must not leave)", who);
    return SPH_OK;
}

static int outflow_alloc(SphHandle *h) {
    State &s = h->st;
    if (!s.outflow_ctr) { int rc = dalloc(h, &s.outflow_ctr, (size_t)(SPH_MAX_OUTFLOWS + 1) * SPH_OUTFLOW_CTR_STRIDE); if (rc) return rc; }
    if (!h->of_pinned) {
        void *p = nullptr;
        HIPCHK(h, hipHostMalloc(&p, sizeof(unsigned) * (SPH_MAX_OUTFLOWS + 1) * SPH_OUTFLOW_CTR_STRIDE, hipHostMallocDefault));
        memset(p, 0, sizeof(unsigned) * (SPH_MAX_OUTFLOWS + 1) * SPH_OUTFLOW_CTR_STRIDE);
        h->of_pinned = (unsigned *)p;
    }
    return SPH_OK;
}

extern "C" int sph_set_outflow(SphHandle *h, int index, const SphOutflow *v) {
    if (!h) return SPH_ERR_INVALID;
    if (index < 0 || index >= SPH_MAX_OUTFLOWS) return fail(h, SPH_ERR_INVALID, "sph_set_outflow: outflow index %d outside 0..%d", index, SPH_MAX_OUTFLOWS - 1);
    if (h->in_step) return fail(h, SPH_ERR_INVALID, "sph_set_outflow: outflow %d: between sph_step_begin and sph_step_end", index);
    OfHost &m = h->of[index];
    if (!v) {
        if (m.on) { m.on = false; h->of_n--; }
        return SPH_OK;
    }
    { int rc = outflow_supported(h, "sph_set_outflow"); if (rc) return rc; }
    if (h->cfl.on || h->cfl.irregular) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_outflow: outflow %d: the step size changes or has changed (sph_set_cfl / sph_set_time_step: the time window is a closed form of k dt)", index);
    { int rc = outflow_check(h, "sph_set_outflow", index, v); if (rc) return rc; }
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = outflow_alloc(h); if (rc) return rc; }
    if (!m.on) h->of_n++;
    m.on = true; m.v = *v; m.removed = 0; m.last = 0;
    return SPH_OK;
}

extern "C" int sph_get_outflow_state(SphHandle *h, int index, SphOutflowState *out) {
    if (!h) return SPH_ERR_INVALID;
    if (!out) return fail(h, SPH_ERR_INVALID, "sph_get_outflow_state: null");
    if (index < 0 || index >= SPH_MAX_OUTFLOWS || !h->of[index].on) return fail(h, SPH_ERR_INVALID, "sph_get_outflow_state: outflow %d is not set", index);
    const OfHost &m = h->of[index];
    memset(out, 0, sizeof(*out));
    out->removed = m.removed; out->removed_last_step = m.last;
    out->active = of_active(&m.v, (double)h->st.c.dt, (long long)h->steps);
    return SPH_OK;
}

extern "C" int sph_outflow_test_host(const SphOutflow *v, const float *xyz, int n, uint8_t *inside) {
    if (!v || n < 0 || (n > 0 && (!xyz || !inside))) return fail(nullptr, SPH_ERR_INVALID, "sph_outflow_test_host: null argument");
    { int rc = outflow_check(nullptr, "sph_outflow_test_host", 0, v); if (rc) return rc; }
    OutflowDev d;
    of_canonical(v, 0, &d);
    for (int k = 0; k < n; ++k) inside[k] = (uint8_t)of_inside(&d, xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]);
    return SPH_OK;
}

extern "C" int sph_outflow_active_host(const SphOutflow *v, double dt, int64_t k) {
    if (!v) return fail(nullptr, SPH_ERR_INVALID, "sph_outflow_active_host: null argument");
    { int rc = outflow_check(nullptr, "sph_outflow_active_host", 0, v); if (rc) return rc; }
    if (k < 0 || !(dt > 0.0) || !std::isfinite(dt)) return fail(nullptr, SPH_ERR_INVALID, "sph_outflow_active_host: k must be >= 0, dt positive and finite");
    return of_active(v, dt, (long long)k);
}

// the id the next new particle gets: the particle count until something has been removed, the monotone counter afterwards
static inline int next_id(const SphHandle *h) { return h->of_removed_any ? h->id_next : h->n; }

// `count` particles carry the dead bit now: the coming sort drops them.  A hash some pass made for that sort did not see the bit.
static void outflow_pending(SphHandle *h, int count) {
    if (count <= 0) return;
    State &s = h->st;
    if (!h->of_removed_any) { h->id_next = h->n; h->of_removed_any = true; }
    h->of_pending += count;
    if (h->prepared) h->sort_dirty = true;
    if (s.prehashed) { s.prehashed = 0; s.cell_count_clean = 0; s.hist_taken = 0; s.run_lists_filed = 0; }
}

// the counters, read back: one copy into pinned memory, one stream wait
static int outflow_read_counters(SphHandle *h) {
    State &s = h->st;
    HIPCHK(h, hipMemcpyAsync(h->of_pinned, s.outflow_ctr, sizeof(unsigned) * (SPH_MAX_OUTFLOWS + 1) * SPH_OUTFLOW_CTR_STRIDE, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(h, hipStreamSynchronize(s.stream));
    return SPH_OK;
}

// the slot: mark and count, for the step count k the running step ends at.  Nothing while no volume is set.
static int ph_outflow(SphHandle *h, long long k) {
    if (h->of_n <= 0) return SPH_OK;
    State &s = h->st;
    OutflowArgs a; memset(&a, 0, sizeof(a));
    for (int q = 0; q < SPH_MAX_OUTFLOWS; ++q) {
        OfHost &m = h->of[q];
        m.last = 0;
        if (m.on && of_active(&m.v, (double)s.c.dt, k)) of_canonical(&m.v, q, &a.v[a.nvol++]);
    }
    if (a.nvol <= 0 || h->n <= 0 || h->n_fluid <= 0) return SPH_OK;
    { ProfScope p(h, SPH_K_OUTFLOW); h->L->outflow_mark(s, a); }
    { int rc = outflow_read_counters(h); if (rc) return rc; }
    int total = 0;
    for (int t = 0; t < a.nvol; ++t) {
        const int q = a.v[t].index;
        const unsigned now = h->of_pinned[q * SPH_OUTFLOW_CTR_STRIDE];
        const int d = (int)(now - h->of_seen[q]);
        h->of_seen[q] = now;
        h->of[q].last = d; h->of[q].removed += d;
        total += d;
    }
    if (total < 0 || total > h->n_fluid) return fail(h, SPH_ERR_INVALID, "outflow: internal: the device counted %d removed of %d fluid particles", total, h->n_fluid);
    outflow_pending(h, total);
    return SPH_OK;
}

// a call that returns to the host leaves no dead particle behind: the sort its last slot asked for runs now.  The next step's own sort
// then finds every particle in its cell already (the same order: both sorts are stable).  DFSPH's passes behind an unexpected sort
// (dfsph_step_begin) still run: sort_dirty stays as it was.
static void outflow_settle(SphHandle *h) {
    if (h->of_pending <= 0 || h->in_step || !h->prepared) return;
    const bool dirty = h->sort_dirty;
    ph_neighbor_search(h, false, false);
    h->sort_dirty = dirty;
}

extern "C" int sph_remove_particles(SphHandle *h, const int32_t *ids, int n) {
    if (!h) return SPH_ERR_INVALID;
    if (n < 0 || (n > 0 && !ids)) return fail(h, SPH_ERR_INVALID, "sph_remove_particles: bad arguments");
    { int rc = outflow_supported(h, "sph_remove_particles"); if (rc) return rc; }
    if (!h->prepared) return fail(h, SPH_ERR_INVALID, "sph_remove_particles before sph_prepare");
    if (n == 0) return SPH_OK;
    if (n > h->n) return fail(h, SPH_ERR_INVALID, "sph_remove_particles: %d ids, %d particles", n, h->n);
    HIPCHK(h, hipSetDevice(h->device));
    State &s = h->st;
    std::vector<int> want(ids, ids + n);
    std::sort(want.begin(), want.end());
    for (int k = 1; k < n; ++k) if (want[k] == want[k - 1]) return fail(h, SPH_ERR_INVALID, "sph_remove_particles: id %d is listed twice", want[k]);
    // every id must name a live active fluid particle: the host looks (a removal from the host is no hot path)
    std::vector<int> pid((size_t)h->n), meta((size_t)h->n);
    HIPCHK(h, hipStreamSynchronize(s.stream));
    HIPCHK(h, hipMemcpy(pid.data(), s.pid.cur(), sizeof(int) * (size_t)h->n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(meta.data(), s.meta.cur(), sizeof(int) * (size_t)h->n, hipMemcpyDeviceToHost));
    int found = 0;
    for (int i = 0; i < h->n; ++i) {
        if (!std::binary_search(want.begin(), want.end(), pid[(size_t)i])) continue;
        const int m = meta[(size_t)i];
        if (META_DEAD(m)) return fail(h, SPH_ERR_INVALID, "sph_remove_particles: id %d has been removed already", pid[(size_t)i]);
        if (!META_ACTIVE_FLUID(m)) return fail(h, SPH_ERR_INVALID, "sph_remove_particles: id %d is not an active fluid particle", pid[(size_t)i]);
        found++;
    }
    if (found != n) return fail(h, SPH_ERR_INVALID, "sph_remove_particles: %d of the %d ids name no live particle", n - found, n);
    { int rc = outflow_alloc(h); if (rc) return rc; }
    if (s.outflow_ids_cap < n) {
        int cap = s.outflow_ids_cap > 0 ? s.outflow_ids_cap : 1024;
        while (cap < n) cap *= 2;
        int *p = nullptr;
        { int rc = dalloc(h, &p, (size_t)cap); if (rc) return rc; }   // (the smaller one stays until sph_destroy)
        s.outflow_ids = p; s.outflow_ids_cap = cap;
    }
    HIPCHK(h, hipMemcpy(s.outflow_ids, want.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    refresh_counts(h);
    { ProfScope p(h, SPH_K_OUTFLOW); h->L->outflow_mark_ids(s, n); }
    { int rc = check_async(h); if (rc) return rc; }
    // the device's own count of what it marked must be the host's: a cheap guard against the two disagreeing about who is alive
    { int rc = outflow_read_counters(h); if (rc) return rc; }
    const unsigned now = h->of_pinned[SPH_MAX_OUTFLOWS * SPH_OUTFLOW_CTR_STRIDE];
    const int marked = (int)(now - h->of_seen_ids);
    h->of_seen_ids = now;
    outflow_pending(h, marked);
    outflow_settle(h);
    if (marked != n) return fail(h, SPH_ERR_INVALID, "sph_remove_particles: internal: the device marked %d of %d ids", marked, n);
    { int rc = check_async(h); if (rc) return rc; }
    HIPCHK(h, hipStreamSynchronize(s.stream));
    return SPH_OK;
}
