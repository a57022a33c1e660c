// sph_emitter_api.hpp -- fluid emitters, host side (include/sph_hip.h sph_set_emitter): the entry points, and the slot of a
// step that holds and emits.  Included by sph_api.hip.  The schedule is evaluated HERE, with the kernels' own source
// (sph_emitter_eval.hpp): the new particle count is known without a read-back, and a step with emitters has no synchronisation and no
// copy that a step without them lacks.
#pragma once
#include "sph_emitter_eval.hpp"

static inline double em_dt(const SphHandle *h) { return (double)h->st.c.dt; }
static inline double em_spacing(const SphHandle *h) { return 2.0 * h->prm.particle_radius; }

static int emitter_check(SphHandle *h, const char *who, int index, const SphEmitter *e, double dt, double spacing, int *nu, int *nv,
                         int *layer_n, int *max_layers) {
#define EM_FAIL(...) return fail(h, SPH_ERR_INVALID, __VA_ARGS__)
    const double *vecs[4] = {e->position, e->direction, e->tangent1, e->tangent2};
    for (int q = 0; q < 4; ++q)
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(vecs[q][c])) EM_FAIL("%s: emitter %d: position / direction / tangent: a component is not finite", who, index);
    if (e->shape != SPH_EMITTER_RECTANGLE && e->shape != SPH_EMITTER_CIRCLE) EM_FAIL("%s: emitter %d: shape %d is neither 0 (rectangle) nor 1 (circle)", who, index, e->shape);
    const double *b[3] = {e->direction, e->tangent1, e->tangent2};
    for (int p = 0; p < 3; ++p)
        for (int q = p; q < 3; ++q) {
            const double dot = b[p][0] * b[q][0] + b[p][1] * b[q][1] + b[p][2] * b[q][2];
            if (fabs(dot - (p == q ? 1.0 : 0.0)) > 1e-9) EM_FAIL("%s: emitter %d: direction, tangent1, tangent2 are not orthonormal", who, index);
        }
    if (e->shape == SPH_EMITTER_CIRCLE) { if (!(e->radius > 0.0) || !std::isfinite(e->radius)) EM_FAIL("%s: emitter %d: radius %g is not positive and finite", who, index, e->radius); }
    else if (!(e->width > 0.0) || !std::isfinite(e->width) || !(e->height > 0.0) || !std::isfinite(e->height))
        EM_FAIL("%s: emitter %d: width %g / height %g is not positive and finite", who, index, e->width, e->height);
    if (!(e->speed > 0.0) || !std::isfinite(e->speed)) EM_FAIL("%s: emitter %d: speed %g is not positive and finite", who, index, e->speed);
    if (!(e->density > 0.0) || !std::isfinite(e->density)) EM_FAIL("%s: emitter %d: density %g is not positive and finite", who, index, e->density);
    if (!std::isfinite(e->start) || std::isnan(e->end) || !(e->end > e->start)) EM_FAIL("%s: emitter %d: end %g <= start %g", who, index, e->end, e->start);
    if (e->hold < 0 || e->hold > SPH_EMITTER_MAX_HOLD) EM_FAIL("%s: emitter %d: hold %d outside 0..%d", who, index, e->hold, SPH_EMITTER_MAX_HOLD);
    if (e->max_particles <= 0) EM_FAIL("%s: emitter %d: max_particles %d is not positive", who, index, e->max_particles);
    if (e->reserved != 0) EM_FAIL("%s: emitter %d: reserved must be 0", who, index);
    if (!(dt > 0.0) || !std::isfinite(dt) || !(spacing > 0.0) || !std::isfinite(spacing)) EM_FAIL("%s: emitter %d: dt and spacing must be positive and finite", who, index);
    if (e->speed * dt > 0.5 * spacing) EM_FAIL("%s: emitter %d: speed %g * dt %g exceeds half a particle spacing %g (more than one layer per step)", who, index, e->speed, dt, spacing);
    em_lattice(e, spacing, nu, nv);
    *layer_n = (*nu > 0 && *nv > 0) ? em_layer_count(e, spacing) : 0;
    if (*layer_n <= 0) EM_FAIL("%s: emitter %d: the nozzle holds no lattice point (layer_n == 0) at spacing %g", who, index, spacing);
    if (e->max_particles < *layer_n) EM_FAIL("%s: emitter %d: max_particles %d is less than one layer (%d particles)", who, index, e->max_particles, *layer_n);
    *max_layers = e->max_particles / *layer_n;
#undef EM_FAIL
    return SPH_OK;
}

static long long em_reserved(const SphHandle *h) {   // slots the emitters may still fill
    long long r = 0;
    for (int q = 0; q < SPH_MAX_EMITTERS; ++q)
        if (h->em[q].on) r += (long long)(h->em[q].max_layers - h->em[q].layers) * h->em[q].layer_n;
    return r;
}
static int em_of_object(const SphHandle *h, int object_id) {
    for (int q = 0; q < SPH_MAX_EMITTERS; ++q) if (h->em[q].on && h->em[q].e.object_id == object_id) return q;
    return -1;
}

extern "C" int sph_set_emitter(SphHandle *h, int index, const SphEmitter *e) {
    if (!h) return SPH_ERR_INVALID;
    if (index < 0 || index >= SPH_MAX_EMITTERS) return fail(h, SPH_ERR_INVALID, "sph_set_emitter: emitter index %d outside 0..%d", index, SPH_MAX_EMITTERS - 1);
    if (!e) return fail(h, SPH_ERR_INVALID, "sph_set_emitter: emitter %d: null argument", index);
    if (h->prepared) return fail(h, SPH_ERR_INVALID, "sph_set_emitter: emitter %d: after sph_prepare (emitters are set before it)", index);
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_emitter: emitter %d: not on a PBF handle (either variant: PBF never inserts)", index);
    if (h->st.slab_active || h->comm.slab_ready) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_emitter: emitter %d: not on a sharded handle (the schedule knows one particle count)", index);
    if (h->prm.g_upper < 9999.0) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_emitter: emitter %d: not with g_upper set (gravitationUpper, the reference's frozen-block emitter)", index);
    if (h->cfl.on || h->cfl.irregular) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_emitter: emitter %d: the step size changes or has changed (sph_set_cfl / sph_set_time_step: the schedule is a closed form of k dt)", index);
    if (h->swap_axis) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_emitter: emitter %d: the handle's axis order is not \"xyz\"", index);
    if (h->st.ids_custom) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_emitter: emitter %d: particle ids were set from outside (sph_set_appended_ids / SPH_F_PARTICLE_ID): held layers are found by id and need the append order", index);
    const int o = e->object_id;
    if (o < 0 || o >= SPH_MAX_OBJECTS) return fail(h, SPH_ERR_INVALID, "sph_set_emitter: emitter %d: object_id %d outside 0..%d", index, o, SPH_MAX_OBJECTS - 1);
    if (h->obj_n[o] > 0) return fail(h, SPH_ERR_INVALID, "sph_set_emitter: emitter %d: object_id %d already owns %d particles", index, o, h->obj_n[o]);
    { const int other = em_of_object(h, o); if (other >= 0 && other != index) return fail(h, SPH_ERR_INVALID, "sph_set_emitter: emitter %d: object_id %d belongs to emitter %d", index, o, other); }
    if (h->el[o].state != 0) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_emitter: emitter %d: object_id %d is an elastic solid", index, o);
    EmHost m;
    { int rc = emitter_check(h, "sph_set_emitter", index, e, em_dt(h), em_spacing(h), &m.nu, &m.nv, &m.layer_n, &m.max_layers); if (rc) return rc; }
    const EmHost old = h->em[index];
    h->em[index].on = false;
    const long long need = (long long)next_id(h) + em_reserved(h) + (long long)m.max_layers * m.layer_n;
    if (need > (long long)h->st.cap) {
        h->em[index] = old;
        return fail(h, SPH_ERR_CAPACITY, "sph_set_emitter: emitter %d: %d particles + the emitters' budgets = %lld exceed particle_max_num %d", index, h->n, need, h->st.cap);
    }
    HIPCHK(h, hipSetDevice(h->device));
    State &s = h->st;
    if (!s.emitters) { int rc = dalloc(h, &s.emitters, (size_t)SPH_MAX_EMITTERS); if (rc) { h->em[index] = old; return rc; } }
    m.on = true; m.e = *e; m.layers = 0; m.base.clear();
    EmitterDev d; memset(&d, 0, sizeof(d));
    d.e = *e; d.nu = m.nu; d.nv = m.nv; d.layer_n = m.layer_n; d.max_layers = m.max_layers;
    HIPCHK(h, hipStreamSynchronize(s.stream));
    HIPCHK(h, hipMemcpy(s.emitters + index, &d, sizeof(EmitterDev), hipMemcpyHostToDevice));
    h->em[index] = m;
    h->em_n = 0;
    for (int q = 0; q < SPH_MAX_EMITTERS; ++q) h->em_n += h->em[q].on ? 1 : 0;
    // the uniform-mass instantiation of the fast build is decided HERE, from the emitter's density: it must not flip at the first emission
    const float mass = (float)h->prm.V0 * (float)e->density;
    if (!h->fluid_mass_seen) { h->fluid_mass_seen = true; h->fluid_mass0 = mass; }
    else if (mass != h->fluid_mass0) h->fluid_mass_uniform = false;
    refresh_counts(h);
    return SPH_OK;
}

// held layers of emitter q at count k among the layers emitted so far: [lo, hi)
static void em_held_range(const SphHandle *h, int q, long long k, EmSchedule *sc, int *lo, int *hi) {
    const EmHost &m = h->em[q];
    em_schedule(&m.e, m.max_layers, em_dt(h), em_spacing(h), k, sc);
    *hi = sc->born < m.layers ? sc->born : m.layers;
    *lo = sc->held_lo < *hi ? sc->held_lo : *hi;
}

extern "C" int sph_get_emitter_state(SphHandle *h, int index, SphEmitterState *out) {
    if (!h) return SPH_ERR_INVALID;
    if (!out) return fail(h, SPH_ERR_INVALID, "sph_get_emitter_state: null");
    if (index < 0 || index >= SPH_MAX_EMITTERS || !h->em[index].on) return fail(h, SPH_ERR_INVALID, "sph_get_emitter_state: emitter %d is not set", index);
    const EmHost &m = h->em[index];
    memset(out, 0, sizeof(*out));
    out->object_id = m.e.object_id; out->layer_particles = m.layer_n; out->max_layers = m.max_layers;
    out->layers = m.layers; out->emitted = m.layers * m.layer_n;
    EmSchedule sc; int lo, hi;
    em_held_range(h, index, (long long)h->steps, &sc, &lo, &hi);
    out->held_layers = hi - lo; out->held_first = lo;
    for (int j = lo; j < hi && j - lo <= SPH_EMITTER_MAX_HOLD; ++j) out->held_id_base[j - lo] = m.base[(size_t)j];
    out->exhausted = (m.layers >= m.max_layers || sc.T > m.e.end) ? 1 : 0;
    return SPH_OK;
}

extern "C" int sph_emitter_eval_host(const SphEmitter *e, double dt, double spacing, int64_t k, int layer, SphEmitterEval *out, float *xyz) {
    if (!e || !out) return fail(nullptr, SPH_ERR_INVALID, "sph_emitter_eval_host: null argument");
    if (k < 0) return fail(nullptr, SPH_ERR_INVALID, "sph_emitter_eval_host: k must be >= 0");
    int nu, nv, layer_n, max_layers;
    { int rc = emitter_check(nullptr, "sph_emitter_eval_host", 0, e, dt, spacing, &nu, &nv, &layer_n, &max_layers); if (rc) return rc; }
    EmSchedule sc;
    em_schedule(e, max_layers, dt, spacing, (long long)k, &sc);
    memset(out, 0, sizeof(*out));
    out->T = sc.T; out->s = sc.s; out->born = sc.born; out->held_first = sc.held_lo; out->held_layers = sc.born - sc.held_lo;
    out->layer_particles = layer_n; out->max_layers = max_layers; out->nu = nu; out->nv = nv;
    if (layer >= 0) {
        out->layer_offset = em_layer_offset(sc.s, layer, spacing);
        if (xyz)
            for (int idx = 0; idx < layer_n; ++idx) {
                double a, b;
                em_point(e, nu, nv, spacing, idx, &a, &b);
                em_position(e, out->layer_offset, a, b, xyz + 3 * idx);
            }
    }
    return SPH_OK;
}

// does the slot of the step that ends at count k hold or emit anything?  (the host knows before it launches the step's first pass:
// a force pass / position update must not hash for the coming sort when the slot moves or adds particles behind it)
static bool em_slot_touches(const SphHandle *h, long long k) {
    if (h->em_n <= 0) return false;
    for (int q = 0; q < SPH_MAX_EMITTERS; ++q) {
        if (!h->em[q].on) continue;
        EmSchedule sc; int lo, hi;
        em_held_range(h, q, k, &sc, &lo, &hi);
        if (sc.born > h->em[q].layers || hi > lo) return true;
    }
    return false;
}

// the slot: hold, then emit, for the step count k the running step ends at (sph_prepare: 0).  No synchronisation, no copy.
// stage 0: both; 1: the hold alone; 2: the emission alone (a step's slot: the outflow mark runs between them)
static int ph_emit(SphHandle *h, long long k, int stage = 0) {
    if (h->em_n <= 0) return SPH_OK;
    State &s = h->st;
    const double spacing = em_spacing(h);
    EmitHoldArgs ha; EmitArgs ea;
    ha.spacing = ea.spacing = spacing; ha.nlayers = 0; ha.id_lo = 0x7fffffff; ha.id_hi = 0; ea.nlayers = 0; ea.total = 0;
    int n_new = h->n, id_new = next_id(h);   // slots behind the last particle (dead ones included), ids from the counter
    for (int q = 0; q < SPH_MAX_EMITTERS; ++q) {
        EmHost &m = h->em[q];
        if (!m.on) continue;
        EmSchedule sc; int lo, hi;
        em_held_range(h, q, k, &sc, &lo, &hi);
        for (int j = lo; j < hi && ha.nlayers < SPH_EMIT_HOLD_ENTRIES; ++j) {
            const int base = m.base[(size_t)j];
            ha.emitter[ha.nlayers] = q; ha.id_base[ha.nlayers] = base; ha.offset[ha.nlayers] = em_layer_offset(sc.s, j, spacing);
            if (base < ha.id_lo) ha.id_lo = base;
            if (base + m.layer_n > ha.id_hi) ha.id_hi = base + m.layer_n;
            ha.nlayers++;
        }
        if (sc.born > m.layers) {
            // (speed dt <= spacing / 2: one layer per emitter and slot; a caller that skipped slots catches up one layer per slot)
            if ((long long)n_new + m.layer_n > (long long)s.cap) return fail(h, SPH_ERR_CAPACITY, "emitter %d: internal: the reserved capacity is gone (%d + %d > %d)", q, n_new, m.layer_n, s.cap);
            const int j = m.layers;
            ea.emitter[ea.nlayers] = q; ea.first[ea.nlayers] = n_new; ea.id_first[ea.nlayers] = id_new; ea.start[ea.nlayers] = ea.total; ea.offset[ea.nlayers] = em_layer_offset(sc.s, j, spacing);
            ea.nlayers++; ea.total += m.layer_n; ea.start[ea.nlayers] = ea.total;
            n_new += m.layer_n; id_new += m.layer_n;
        }
    }
    if (stage != 2 && ha.nlayers > 0 && h->n > 0) { ProfScope p(h, SPH_K_EMIT); h->L->emit_hold(s, ha); }
    if (stage == 1 || ea.nlayers <= 0) return SPH_OK;
    { ProfScope p(h, SPH_K_EMIT); h->L->emit(s, ea); }
    if (s.heat_T_home)   // heat: the newborn rows start at their emitter's temperature (ids and counts are known here in closed form)
        for (int t = 0; t < ea.nlayers; ++t) {
            const EmHost &m = h->em[ea.emitter[t]];
            h->L->heat_fill(s, ea.id_first[t], m.layer_n, heat_insert_T(h, m.e.object_id));
        }
    // the counts, as sph_append_particles changes them
    for (int t = 0; t < ea.nlayers; ++t) {
        EmHost &m = h->em[ea.emitter[t]];
        const int o = m.e.object_id;
        if (h->obj_n[o] == 0) h->obj_first[o] = ea.id_first[t];
        else if (h->obj_first[o] + h->obj_n[o] != ea.id_first[t]) h->obj_split[o] = true;
        h->obj_n[o] += m.layer_n;
        m.base.push_back(ea.id_first[t]);
        m.layers++;
    }
    h->n = n_new;
    h->id_next = id_new;
    h->n_fluid += ea.total;
    if (!h->prepared) h->rigid_volume_done = false;
    if (h->prepared) h->sort_dirty = true;
    s.masks_valid = 0;
    s.perm_n = -1; s.list_n = -1;
    refresh_counts(h);
    return SPH_OK;
}
