// sph_rigid_motion_eval.hpp -- the evaluator of a scripted rigid body's motion program (SphRigidMotion, include/sph_hip.h):
// pose at a time, and pose + backward-difference velocities of one step.  ONE source for the kernel (sph_rigid_motion.hpp), the host
// entry sph_rigid_motion_eval_host (sph_api.hip) and the stand-alone check (tools/check_rigid_motion.cpp).  Float64, every product
// rounded (no contraction in either build, as sph_rigid.hpp): the host model SPH/rigid_solver/motion.py is written statement by
// statement like this file, and the two are compared to 1e-12.  The keys are read where the program lies (global memory on the device):
// no per-lane copy.  Needs <math.h> and include/sph_hip.h before it.
#pragma once

#if defined(__HIPCC__)
#define RM_HD __host__ __device__ static inline
#else
#define RM_HD static inline
#endif
#if defined(__clang__)
#define RM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RM_NO_CONTRACT   /* (build with -ffp-contract=off) */
#endif

RM_HD void rm_mul(const double *a, const double *b, double *c) {   // c = a b
    RM_NO_CONTRACT
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
RM_HD void rm_mul_t(const double *a, const double *b, double *c) {   // c = a b^T
    RM_NO_CONTRACT
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}
RM_HD void rm_mul_v(const double *a, const double *v, double *r) {   // r = a v
    RM_NO_CONTRACT
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}

// exp([w]x): rotation by |w| about w (Rodrigues), as rb_skew_exp (sph_rigid.hpp) and host_rigid_solver.py _skew_exp
RM_HD void rm_skew_exp(const double *w, double *e) {
    RM_NO_CONTRACT
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
    for (int q = 0; q < 9; ++q) e[q] = (q % 4 == 0) ? 1.0 : 0.0;
    if (th < 1e-12) return;
    const double k0 = w[0] / th, k1 = w[1] / th, k2 = w[2] / th;
    const double K[9] = {0.0, -k2, k1, k2, 0.0, -k0, -k1, k0, 0.0};
    double KK[9];
    rm_mul(K, K, KK);
    const double s = sin(th), c1 = 1.0 - cos(th);
#pragma unroll
    for (int q = 0; q < 9; ++q) e[q] = (e[q] + s * K[q]) + c1 * KK[q];
}

// the keyframe interpolant at tau: translation kd, rotation vector kth (zero without keys)
RM_HD void rm_keys(const SphRigidMotion *m, double tau, double *kd, double *kth) {
    RM_NO_CONTRACT
#pragma unroll
    for (int k = 0; k < 3; ++k) { kd[k] = 0.0; kth[k] = 0.0; }
    const int n = m->nkeys;
    if (n <= 0) return;
    const double T = m->key_times[n - 1];   // the period
    double tk = tau;
    if (T > 0.0) {
        if (m->repeat == 1) tk = fmod(tau, T);
        else if (m->repeat == 2) { const double r = fmod(tau, 2.0 * T); tk = r <= T ? r : 2.0 * T - r; }
    }
    int i = n - 1;   // at or behind the last key (hold; the turning point of pingpong): its values as given
    for (int q = 0; q + 1 < n; ++q)
        if (tk < m->key_times[q + 1]) { i = q; break; }
    if (i == n - 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { kd[k] = m->key_translations[i][k]; kth[k] = m->key_rotations[i][k]; }
        return;
    }
    const double t0 = m->key_times[i], t1 = m->key_times[i + 1];
    double s = (tk - t0) / (t1 - t0);
    if (m->interpolation == 1) s = (s * s) * (3.0 - 2.0 * s);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = m->key_translations[i][k], b = m->key_translations[i + 1][k];
        const double ra = m->key_rotations[i][k], rb = m->key_rotations[i + 1][k];
        kd[k] = a + s * (b - a);
        kth[k] = ra + s * (rb - ra);
    }
}

// com(t), rot(t) from the rest pose (c0, R0 row-major)
RM_HD void rm_pose(const SphRigidMotion *m, const double *c0, const double *R0, double t, double *com, double *rot) {
    RM_NO_CONTRACT
    double tc = t < m->start ? m->start : t;
    if (tc > m->end) tc = m->end;
    const double tau = tc - m->start;
    double ramp = 1.0;
    if (m->ramp > 0.0) { ramp = tau / m->ramp; if (ramp > 1.0) ramp = 1.0; }
    const double w = 6.283185307179586 * m->frequency;
    const double h = ramp * sin(w * tau + m->phase);
    double kd[3], kth[3], d[3], th[3];
    rm_keys(m, tau, kd, kth);
    const double ha = h * m->amplitude, hg = h * m->angle, tr = tau * m->drift_rate;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = (kd[k] + ha * m->direction[k]) + tau * m->drift_velocity[k];
        th[k] = kth[k] + (hg * m->axis[k] + tr * m->drift_axis[k]);
    }
    double E[9], q[3], Eq[3];
    rm_skew_exp(th, E);
    rm_mul(E, R0, rot);
    rm_mul_v(R0, m->pivot, q);
    rm_mul_v(E, q, Eq);
#pragma unroll
    for (int k = 0; k < 3; ++k) com[k] = ((c0[k] + q[k]) + d[k]) - Eq[k];
}

// step k -> k + 1: the pose at t_{k+1} and the backward differences that lead there from the pose at t_k
RM_HD void rm_step(const SphRigidMotion *m, const double *c0, const double *R0, double dt, long long k, double *com, double *rot,
                   double *vel, double *angvel) {
    RM_NO_CONTRACT
    const double ta = (double)k * dt, tb = (double)(k + 1) * dt;
    double ca[3], Ra[9], M[9];
    rm_pose(m, c0, R0, ta, ca, Ra);
    rm_pose(m, c0, R0, tb, com, rot);
#pragma unroll
    for (int q = 0; q < 3; ++q) vel[q] = (com[q] - ca[q]) / dt;
    rm_mul_t(rot, Ra, M);
    const double a[3] = {0.5 * (M[7] - M[5]), 0.5 * (M[2] - M[6]), 0.5 * (M[3] - M[1])};
    const double s = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double c = (((M[0] + M[4]) + M[8]) - 1.0) * 0.5;
    if (s > 1e-12) {
        const double f = atan2(s, c) / s;
#pragma unroll
        for (int q = 0; q < 3; ++q) angvel[q] = (f * a[q]) / dt;
    } else {
#pragma unroll
        for (int q = 0; q < 3; ++q) angvel[q] = a[q] / dt;
    }
}
