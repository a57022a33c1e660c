// sph_cfl_api.hpp -- adaptive time stepping, host side (include/sph_hip.h sph_set_cfl): installing a step size, the slot
// of a step that reduces and sets the next one, and the entry points.  Included by sph_api.hip.  The rule is evaluated HERE, with the
// source the host entries and the stand-alone check compile (sph_cfl_eval.hpp); the maximum comes back from the device: one copy of the
// result pair into pinned memory and one stream wait per step while the mode is on.
#pragma once

// everything that holds the step size: the parameters (PCISPH derives its stiffness from them), the constants every kernel takes by
// value, and the argument structs of the device rigid launches (integrator and contact solver share RigidIntArgs)
static void install_dt(SphHandle *h, double dt) {
    h->prm.dt = dt;
    Consts &c = h->st.c;
    c.dt = (float)dt;
    c.inv_dt = 1.0f / c.dt;
    c.thr_kappa = (float)1e-5 * c.dt;
    if (h->prm.method == SPH_METHOD_PCISPH) c.pcisph_k = host_pcisph_k(h->prm);
    h->st.rigid_int.dt = (double)c.dt;
    h->st.rigid_motion_args.dt = (double)c.dt;
}

// what a handle must be for its step size to change (sph_set_cfl and sph_set_time_step)
static int cfl_supported(SphHandle *h, const char *who) {
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "%s: not on a PBF handle (either variant)", who);
    if (h->st.slab_active || h->comm.slab_ready) return fail(h, SPH_ERR_UNSUPPORTED, "%s: not on a sharded handle (every rank would need the same maximum)", who);
    if (h->prm.g_upper < 9999.0) return fail(h, SPH_ERR_UNSUPPORTED, "%s: not with g_upper set (gravitationUpper: its frozen particles carry the rigid material)", who);
    if (h->em_n > 0) return fail(h, SPH_ERR_UNSUPPORTED, "%s: an emitter is set (its schedule is a closed form of k dt)", who);
    if (h->of_n > 0) return fail(h, SPH_ERR_UNSUPPORTED, "%s: an outflow volume is set (its time window is a closed form of k dt)", who);
    for (int o = 0; o < SPH_NOBJ; ++o)
        if (h->rm_on[o]) return fail(h, SPH_ERR_UNSUPPORTED, "%s: object %d has a motion program (a closed form of k dt)", who, o);
    return SPH_OK;
}

static int cfl_alloc(SphHandle *h) {
    State &s = h->st;
    if (!s.cfl_words) { int rc = dalloc(h, &s.cfl_words, (size_t)2 * SPH_CFL_BANK_STRIDE); if (rc) return rc; }
    if (!h->cfl.pinned) {
        void *p = nullptr;
        HIPCHK(h, hipHostMalloc(&p, sizeof(unsigned) * SPH_CFL_BANK_STRIDE, hipHostMallocDefault));
        memset(p, 0, sizeof(unsigned) * SPH_CFL_BANK_STRIDE);
        h->cfl.pinned = (unsigned *)p;
    }
    return SPH_OK;
}

// the reduce and its read-back: one launch, one copy into pinned memory, one stream wait
static int cfl_reduce(SphHandle *h) {
    State &s = h->st;
    CflHost &m = h->cfl;
    const int bank = m.bank;
    m.bank ^= 1;   // (the launch clears the other pair: the next launch writes that one)
    { ProfScope p(h, SPH_K_CFL); h->L->cfl_speed(s, bank); }
    HIPCHK(h, hipMemcpyAsync(m.pinned, s.cfl_words + bank * SPH_CFL_BANK_STRIDE, sizeof(unsigned) * SPH_CFL_BANK_STRIDE, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(h, hipStreamSynchronize(s.stream));
    if (m.pinned[SPH_CFL_WORD_STRIDE]) { m.stale = true; return fail(h, SPH_ERR_INVALID, "cfl: non-finite velocity"); }
    memcpy(&m.vmax2, &m.pinned[0], sizeof(float));
    m.stale = false;
    return SPH_OK;
}

// the pending step size from the stored maximum and the target: host arithmetic only
static void cfl_pending(SphHandle *h) {
    CflHost &m = h->cfl;
    const double remaining = std::isfinite(m.target) ? m.target - h->total_time : NAN;
    int flags = 0;
    const double dt = cfl_rule(&m.p, 2.0 * h->prm.particle_radius, m.vmax2, remaining, &flags);
    m.flags = flags;
    install_dt(h, dt);
}

static inline bool cfl_reached(const SphHandle *h) { return h->cfl.target - h->total_time <= CFL_REACHED * h->cfl.p.max_dt; }

// the beginning of a step: a maximum that no longer describes the state (appends, uploads) is taken again
static int cfl_step_begin(SphHandle *h) {
    if (!h->cfl.on || !h->cfl.stale) return SPH_OK;
    { int rc = cfl_reduce(h); if (rc) return rc; }
    cfl_pending(h);
    return SPH_OK;
}

// the end of a step: the scene time advances by the step taken; with the mode on the reduce runs first and the next step size follows
static int cfl_step_end(SphHandle *h) {
    CflHost &m = h->cfl;
    const float dt_f = h->st.c.dt;
    int rc = SPH_OK;
    if (m.on) rc = cfl_reduce(h);
    h->total_time += (double)dt_f;  // base_solver.py:694
    h->steps++;
    m.dt_last = (double)dt_f;
    if (dt_f != m.dt_create_f) m.irregular = true;
    if (m.on && !rc) cfl_pending(h);
    return rc;
}

static int cfl_check(SphHandle *h, const char *who, const SphCflParams *p) {
    if (p->method != SPH_CFL_VELOCITY) return fail(h, SPH_ERR_INVALID, "%s: method %d is neither 0 (none) nor 1 (velocity)", who, p->method);
    if (!(p->factor > 0.0) || !std::isfinite(p->factor)) return fail(h, SPH_ERR_INVALID, "%s: factor %g is not a positive finite number", who, p->factor);
    if (!(p->min_dt > 0.0) || !std::isfinite(p->min_dt) || !((float)p->min_dt > 0.0f)) return fail(h, SPH_ERR_INVALID, "%s: min_dt %g is not a positive finite number", who, p->min_dt);
    if (!(p->max_dt > 0.0) || !std::isfinite(p->max_dt) || !std::isfinite((float)p->max_dt)) return fail(h, SPH_ERR_INVALID, "%s: max_dt %g is not a positive finite number", who, p->max_dt);
    if (p->min_dt > p->max_dt) return fail(h, SPH_ERR_INVALID, "%s: min_dt %g > max_dt %g", who, p->min_dt, p->max_dt);
    if (p->reserved != 0) return fail(h, SPH_ERR_INVALID, "%s: reserved must be 0", who);
    return SPH_OK;
}

extern "C" int sph_set_time_step(SphHandle *h, double dt) {
    if (!h) return SPH_ERR_INVALID;
    if (h->in_step) return fail(h, SPH_ERR_INVALID, "sph_set_time_step: between sph_step_begin and sph_step_end");
    if (!(dt > 0.0) || !std::isfinite(dt) || !std::isfinite((float)dt) || !((float)dt > 0.0f))
        return fail(h, SPH_ERR_INVALID, "sph_set_time_step: dt %g must be positive and finite", dt);
    if (h->cfl.on) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_time_step: the CFL mode is on (sph_set_cfl sets the step size)");
    { int rc = cfl_supported(h, "sph_set_time_step"); if (rc) return rc; }
    install_dt(h, dt);
    return SPH_OK;
}

extern "C" int sph_set_cfl(SphHandle *h, const SphCflParams *p) {
    if (!h) return SPH_ERR_INVALID;
    if (h->in_step) return fail(h, SPH_ERR_INVALID, "sph_set_cfl: between sph_step_begin and sph_step_end");
    CflHost &m = h->cfl;
    if (!p || p->method == SPH_CFL_NONE) {
        if (m.on) { m.on = false; m.target = NAN; m.flags = 0; install_dt(h, m.dt_create); }
        return SPH_OK;
    }
    { int rc = cfl_check(h, "sph_set_cfl", p); if (rc) return rc; }
    { int rc = cfl_supported(h, "sph_set_cfl"); if (rc) return rc; }
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = cfl_alloc(h); if (rc) return rc; }
    m.p = *p;
    m.on = true;
    m.stale = true;
    if (h->prepared) {
        refresh_counts(h);
        { int rc = cfl_reduce(h); if (rc) return rc; }
        cfl_pending(h);
    }
    return SPH_OK;
}

extern "C" int sph_get_cfl(SphHandle *h, SphCflParams *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    if (h->cfl.on) *out = h->cfl.p;
    return SPH_OK;
}

extern "C" int sph_get_time_state(SphHandle *h, SphTimeState *out) {
    if (!h) return SPH_ERR_INVALID;
    if (!out) return fail(h, SPH_ERR_INVALID, "sph_get_time_state: null");
    const CflHost &m = h->cfl;
    memset(out, 0, sizeof(*out));
    out->time = h->total_time;
    out->dt_next = (double)h->st.c.dt;
    out->dt_last = m.dt_last;
    out->target = m.on ? m.target : NAN;
    out->vmax2 = m.on ? m.vmax2 : 0.0f;
    out->flags = m.on ? (m.flags | (m.stale ? SPH_CFL_STALE : 0)) : 0;
    out->steps = h->steps;
    return SPH_OK;
}

extern "C" int sph_set_time_target(SphHandle *h, double t_end) {
    if (!h) return SPH_ERR_INVALID;
    if (!h->cfl.on) return fail(h, SPH_ERR_INVALID, "sph_set_time_target: the CFL mode is off (sph_set_cfl)");
    if (h->in_step) return fail(h, SPH_ERR_INVALID, "sph_set_time_target: between sph_step_begin and sph_step_end");
    h->cfl.target = std::isfinite(t_end) ? t_end : NAN;
    if (!h->cfl.stale) cfl_pending(h);   // (a stale maximum: the next step's reduce computes the step size with the target)
    return SPH_OK;
}

extern "C" int sph_advance_until(SphHandle *h, double t_end, int max_steps, int *steps_done) {
    if (!h) return SPH_ERR_INVALID;
    if (steps_done) *steps_done = 0;
    if (!h->cfl.on) return fail(h, SPH_ERR_INVALID, "sph_advance_until: the CFL mode is off (sph_set_cfl)");
    if (!h->prepared) return fail(h, SPH_ERR_INVALID, "sph_advance_until before sph_prepare");
    if (h->in_step) return fail(h, SPH_ERR_INVALID, "sph_advance_until: between sph_step_begin and sph_step_end");
    if (!std::isfinite(t_end) || max_steps < 0) return fail(h, SPH_ERR_INVALID, "sph_advance_until: t_end must be finite, max_steps >= 0");
    HIPCHK(h, hipSetDevice(h->device));
    refresh_counts(h);
    CflHost &m = h->cfl;
    m.target = t_end;
    if (!m.stale) cfl_pending(h);
    int done = 0, rc = SPH_OK;
    while (done < max_steps && !cfl_reached(h)) {
        rc = step_once(h);
        if (rc) break;
        done++;
    }
    m.target = NAN;
    if (!m.stale) cfl_pending(h);
    if (steps_done) *steps_done = done;
    if (rc) return rc;
    rc = check_async(h); if (rc) return rc;
    return finish_sync(h);
}

extern "C" int sph_cfl_dt_host(const SphCflParams *p, double diameter, float vmax2, double remaining, double *dt, int32_t *flags) {
    if (!p || !dt) return fail(nullptr, SPH_ERR_INVALID, "sph_cfl_dt_host: null argument");
    { int rc = cfl_check(nullptr, "sph_cfl_dt_host", p); if (rc) return rc; }
    if (!(diameter > 0.0) || !std::isfinite(diameter)) return fail(nullptr, SPH_ERR_INVALID, "sph_cfl_dt_host: diameter %g is not a positive finite number", diameter);
    if (!std::isfinite(vmax2) || vmax2 < 0.0f) return fail(nullptr, SPH_ERR_INVALID, "sph_cfl_dt_host: non-finite velocity");
    int f = 0;
    *dt = cfl_rule(p, diameter, vmax2, remaining, &f);
    if (flags) *flags = f;
    return SPH_OK;
}

extern "C" int sph_cfl_speed2_host(int64_t n, const float *vel, const int32_t *meta, float *vmax2, int32_t *nonfinite) {
    if (n < 0 || (n > 0 && (!vel || !meta)) || !vmax2 || !nonfinite) return fail(nullptr, SPH_ERR_INVALID, "sph_cfl_speed2_host: bad arguments");
    int bad = 0;
    cfl_speed2_max(n, vel, meta, vmax2, &bad);
    *nonfinite = bad;
    return SPH_OK;
}
