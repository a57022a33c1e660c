// sph_emitter_eval.hpp -- the evaluator of a fluid emitter's program (SphEmitter, include/sph_hip.h): the lattice of a
// layer, the schedule (layers born after k steps, how far each lies in front of the nozzle plane, which are held) and the position of
// one lattice point.  ONE source for the emit kernel and the hold kernel (sph_emitter.hpp), the host side of a step and the host entry
// sph_emitter_eval_host (sph_api.hip), and the stand-alone check (tools/check_emitter.cpp).  Float64, every product rounded (no
// contraction in either build, as sph_rigid_motion_eval.hpp); a position is rounded to float32 once, at the end.  Needs <math.h> and
// include/sph_hip.h before it.
#pragma once

#if defined(__HIPCC__)
#define EM_HD __host__ __device__ static inline
#else
#define EM_HD static inline
#endif
#if defined(__clang__)
#define EM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EM_NO_CONTRACT   /* (build with -ffp-contract=off) */
#endif

// what the schedule says after k completed steps
struct EmSchedule {
    double T;        // k dt (a product)
    double s;        // speed * max(0, min(T, end) - start): how far layer 0 lies in front of the plane
    int born;        // layers born so far
    int held_lo;     // layers [held_lo, born) are held (held_lo == born: none)
};

// lattice counts of the bounding rectangle (a circle: of its bounding square)
EM_HD void em_lattice(const SphEmitter *e, double spacing, int *nu, int *nv) {
    EM_NO_CONTRACT
    if (e->shape == SPH_EMITTER_CIRCLE) {
        const double n = floor((2.0 * e->radius) / spacing);
        *nu = *nv = (n >= 1.0 && n < 32768.0) ? (int)n : 0;
    } else {
        const double a = floor(e->width / spacing), b = floor(e->height / spacing);
        *nu = (a >= 1.0 && a < 32768.0) ? (int)a : 0;
        *nv = (b >= 1.0 && b < 32768.0) ? (int)b : 0;
    }
}

// lattice coordinate of index i among n along one tangent: (i + 0.5 - n / 2) spacing
EM_HD double em_coord(int i, int n, double spacing) {
    EM_NO_CONTRACT
    return (((double)i + 0.5) - (double)n / 2.0) * spacing;
}

// circle: first kept column of row j (the kept columns of a row are first .. n - 1 - first: the lattice is symmetric and |a| falls towards
// the centre, so the test a^2 + b^2 <= r^2 is monotone over the left half), or -1 for an empty row
EM_HD int em_row_first(const SphEmitter *e, int n, double spacing, int j) {
    EM_NO_CONTRACT
    const double b = em_coord(j, n, spacing), r2 = e->radius * e->radius, b2 = b * b;
    int lo = 0, hi = (n + 1) / 2;   // the answer lies in [lo, hi]; hi: none
    const int none = hi;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        const double a = em_coord(mid, n, spacing);
        if (a * a + b2 <= r2) hi = mid; else lo = mid + 1;
    }
    return lo < none ? lo : -1;
}

// points of one layer
EM_HD int em_layer_count(const SphEmitter *e, double spacing) {
    int nu, nv;
    em_lattice(e, spacing, &nu, &nv);
    if (e->shape != SPH_EMITTER_CIRCLE) return nu * nv;
    int count = 0;
    for (int j = 0; j < nv; ++j) { const int f = em_row_first(e, nu, spacing, j); if (f >= 0) count += nu - 2 * f; }
    return count;
}

// lattice point idx of a layer (j slow, i fast; the circle in the same order with the gaps closed) -> its coordinates in the plane
EM_HD void em_point(const SphEmitter *e, int nu, int nv, double spacing, int idx, double *a, double *b) {
    int i = 0, j = 0;
    if (e->shape != SPH_EMITTER_CIRCLE) { j = idx / nu; i = idx - j * nu; }
    else {
        int acc = 0;
        for (j = 0; j < nv; ++j) {
            const int f = em_row_first(e, nu, spacing, j);
            const int cnt = f >= 0 ? nu - 2 * f : 0;
            if (idx < acc + cnt) { i = f + (idx - acc); break; }
            acc += cnt;
        }
    }
    *a = em_coord(i, nu, spacing); *b = em_coord(j, nv, spacing);
}

// the schedule after k completed steps; max_layers = floor(max_particles / layer_n)
EM_HD void em_schedule(const SphEmitter *e, int max_layers, double dt, double spacing, long long k, EmSchedule *out) {
    EM_NO_CONTRACT
    const double T = (double)k * dt;
    const double te = T < e->end ? T : e->end;
    const double tau = te - e->start;
    const double s = e->speed * (tau > 0.0 ? tau : 0.0);
    int born = 0;
    if (!(T < e->start)) {
        const double q = floor(s / spacing) + 1.0;
        born = q < (double)max_layers ? (int)q : max_layers;
    }
    int lo = born;
    if (e->hold > 0 && T <= e->end) {
        const double reach = (double)e->hold * spacing;
        while (lo > 0 && (s - (double)(lo - 1) * spacing) < reach) --lo;
    }
    out->T = T; out->s = s; out->born = born; out->held_lo = lo;
}

// a_j(k): how far layer j lies in front of the plane
EM_HD double em_layer_offset(double s, int j, double spacing) {
    EM_NO_CONTRACT
    return s - (double)j * spacing;
}

// position + a_j d + a t1 + b t2, rounded once to float32
EM_HD void em_position(const SphEmitter *e, double aj, double a, double b, float *xyz) {
    EM_NO_CONTRACT
#pragma unroll
    for (int c = 0; c < 3; ++c) xyz[c] = (float)(((e->position[c] + aj * e->direction[c]) + a * e->tangent1[c]) + b * e->tangent2[c]);
}

// velocity speed d, rounded to float32
EM_HD void em_velocity(const SphEmitter *e, float *v) {
    EM_NO_CONTRACT
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (float)(e->speed * e->direction[c]);
}
