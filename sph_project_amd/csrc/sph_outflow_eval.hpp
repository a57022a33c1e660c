// sph_outflow_eval.hpp -- the predicate of an outflow volume (SphOutflow, include/sph_hip.h): is a stored float32 position
// inside the volume, and does the volume's time window hold a step count.  ONE source for the mark kernel (sph_outflow.hpp), the host
// side of a step and the host entries sph_outflow_test_host / sph_outflow_active_host (sph_outflow_api.hpp), and the stand-alone check
// (tools/check_outflow.cpp).  Float32 with every product and sum rounded in the order written (no contraction in either build); the
// bounds are rounded to float32 once, by of_canonical.  Needs <math.h> and include/sph_hip.h before it.
#pragma once

#if defined(__HIPCC__)
#define OF_HD __host__ __device__ static inline
#else
#define OF_HD static inline
#endif
#if defined(__clang__)
#define OF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define OF_NO_CONTRACT   /* (build with -ffp-contract=off) */
#endif

// one volume as the kernel sees it: 48 bytes
struct OutflowDev {
    float lo[3], hi[3];      // box: the faces; sphere: lo = the centre, hi[0] = the radius
    int shape, invert;
    unsigned objects;        // bit o: object o is tested (all ones: every object)
    int index;               // the volume's index (the counter it adds to)
    int pad[2];
};

// SphOutflow -> OutflowDev: the one place where the bounds are rounded
OF_HD void of_canonical(const SphOutflow *v, int index, OutflowDev *d) {
    for (int c = 0; c < 3; ++c) {
        if (v->shape == SPH_OUTFLOW_SPHERE) { d->lo[c] = (float)v->center[c]; d->hi[c] = 0.0f; }
        else { d->lo[c] = (float)v->min[c]; d->hi[c] = (float)v->max[c]; }
    }
    if (v->shape == SPH_OUTFLOW_SPHERE) d->hi[0] = (float)v->radius;
    d->shape = v->shape; d->invert = v->invert ? 1 : 0;
    d->objects = 0xffffffffu;
    if (v->n_objects > 0) {
        d->objects = 0u;
        for (int k = 0; k < v->n_objects && k < SPH_OUTFLOW_MAX_OBJECTS; ++k)
            if (v->objects[k] >= 0 && v->objects[k] < 32) d->objects |= 1u << v->objects[k];
    }
    d->index = index; d->pad[0] = d->pad[1] = 0;
}

// the predicate: geometry and invert
OF_HD int of_inside(const OutflowDev *d, float x, float y, float z) {
    OF_NO_CONTRACT
    int in;
    if (d->shape == SPH_OUTFLOW_SPHERE) {
        const float dx = x - d->lo[0], dy = y - d->lo[1], dz = z - d->lo[2];
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const float d2 = (xx + yy) + zz;
        const float r2 = d->hi[0] * d->hi[0];
        in = d2 <= r2 ? 1 : 0;
    } else {
        in = (x >= d->lo[0] && x <= d->hi[0] && y >= d->lo[1] && y <= d->hi[1] && z >= d->lo[2] && z <= d->hi[2]) ? 1 : 0;
    }
    return d->invert ? 1 - in : in;
}

// the window at step count k: T_k = k dt (a product, never a running sum), active while start <= T_k <= end
OF_HD int of_active(const SphOutflow *v, double dt, long long k) {
    OF_NO_CONTRACT
    const double T = (double)k * dt;
    return (T >= v->start && T <= v->end) ? 1 : 0;
}
