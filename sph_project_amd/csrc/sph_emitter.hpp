// sph_emitter.hpp -- fluid emitters: the two launches of an emitting step; included by sph_kernels.hip inside the per-build namespace.
// Semantics in include/sph_hip.h (sph_set_emitter), design in DESIGN.md 35.
//
// The host evaluates the schedule (sph_emitter_eval.hpp, the source these kernels compile too) and knows, without asking the device,
// which layers are born in a slot and which are held; it passes both as small tables by value.  k_emit_hold: elementwise over the live
// particles, a particle whose persistent id falls into a held layer gets position and velocity of the closed form; everybody else
// leaves after one id load and two compares.  k_emit: one thread per newborn particle of all emitters; it writes every per-particle
// array sph_append_particles writes, clears what late entry leaves cleared for a new fluid particle (the micropolar angular velocity at
// home, the CG warm start), and applies the domain boundary as k_post_insert does.  Plain vector stores only; float64 arithmetic is
// a few dozen operations per particle of a layer, a few thousand threads every few steps.
#pragma once
#include "sph_emitter_eval.hpp"

struct EmitOut {
    float4 *posv, *velm, *orig, *mp_w_home, *cg_x;
    int *meta, *pid;
    unsigned *color, *color_home;
    float *rho, *prs;
};

__global__ void __launch_bounds__(256)
k_emit_hold(const Consts c, const EmitHoldArgs a, const EmitterDev *emitters, const int *pid, float4 *posv, float4 *velm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= live_n(c)) return;
    const int id = pid[i];
    if (id < a.id_lo || id >= a.id_hi) return;
    for (int q = 0; q < a.nlayers; ++q) {
        const EmitterDev *d = emitters + a.emitter[q];
        const int idx = id - a.id_base[q];
        if (idx < 0 || idx >= d->layer_n) continue;
        double la, lb;
        em_point(&d->e, d->nu, d->nv, a.spacing, idx, &la, &lb);
        float x[3], v[3];
        em_position(&d->e, a.offset[q], la, lb, x);
        em_velocity(&d->e, v);
        const float vol = posv[i].w, mass = velm[i].w;
        posv[i] = make_float4(x[0], x[1], x[2], vol);
        velm[i] = make_float4(v[0], v[1], v[2], mass);
        return;
    }
}

__global__ void __launch_bounds__(256)
k_emit(const Consts c, const EmitArgs a, const EmitterDev *emitters, const EmitOut o) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.total) return;
    int q = 0;
    while (q + 1 < a.nlayers && t >= a.start[q + 1]) ++q;
    const EmitterDev *d = emitters + a.emitter[q];
    const int idx = t - a.start[q];
    if (idx >= d->layer_n) return;
    const int slot = a.first[q] + idx;   // the particle count at the emission + the index within the batch
    const int id = a.id_first[q] + idx;  // the persistent id: equal to the slot until a particle has been removed (outflow)
    double la, lb;
    em_point(&d->e, d->nu, d->nv, a.spacing, idx, &la, &lb);
    float x[3], v[3];
    em_position(&d->e, a.offset[q], la, lb, x);
    em_velocity(&d->e, v);
    const float rho = (float)d->e.density;
    float4 p = make_float4(x[0], x[1], x[2], c.V0), u = make_float4(v[0], v[1], v[2], c.V0 * rho);
    if (o.orig) o.orig[slot] = p;
    enforce_boundary(c, p.x, p.y, p.z, u.x, u.y, u.z);
    o.posv[slot] = p;
    o.velm[slot] = u;
    o.meta[slot] = META_PACK(d->e.object_id, SPH_MAT_FLUID, 1);
    o.pid[slot] = id;
    const unsigned col = (unsigned)(d->e.color[0] & 0xff) | ((unsigned)(d->e.color[1] & 0xff) << 8) | ((unsigned)(d->e.color[2] & 0xff) << 16);
    o.color[slot] = col;
    if (o.color_home) o.color_home[id] = col;
    o.rho[slot] = rho;
    o.prs[slot] = 0.0f;
    if (o.mp_w_home) o.mp_w_home[id] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (o.cg_x) o.cg_x[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// over the s.c.n particles alive BEFORE this slot's emission
static void l_emit_hold(State &s, const EmitHoldArgs &a) {
    if (a.nlayers <= 0 || s.c.n <= 0 || !s.emitters) return;
    hipLaunchKernelGGL(k_emit_hold, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, a, s.emitters, s.pid.cur(), s.posv.cur(), s.velm.cur());
    s.masks_valid = 0;  // positions moved
}

static void l_emit(State &s, const EmitArgs &a) {
    if (a.nlayers <= 0 || a.total <= 0 || !s.emitters) return;
    const EmitOut o{s.posv.cur(), s.velm.cur(), s.orig.cur(), s.mp_w_home, s.cg_x, s.meta.cur(), s.pid.cur(), s.color.cur(), s.color_home,
                    s.rho.cur(), s.prs};
    hipLaunchKernelGGL(k_emit, dim3(cdiv(a.total, 256)), dim3(256), 0, s.stream, s.c, a, s.emitters, o);
    s.masks_valid = 0;
}

static void register_emitter_launchers(Launch &L) { L.emit_hold = l_emit_hold; L.emit = l_emit; }
