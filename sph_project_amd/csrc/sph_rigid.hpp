// sph_rigid.hpp -- the device rigid integrator (the host's "device" rigid backend): kernel and launcher; included by sph_kernels.hip
// inside the per-build namespace.  Semantics in include/sph_hip.h (sph_set_rigid_integrator), design in DESIGN.md 19.
//
// One workgroup of 256 threads per registered body does, between the two halves of a step, what HostRigidSolver.integrate does on the
// host (SPH/rigid_solver/host_rigid_solver.py): semi-implicit Euler in float64 under gravity and the fluid wrench, the gyroscopic term,
// rotation by exp([dt w]x), re-orthonormalisation to the orthogonal polar factor, inelastic wall contact of the body's axis-aligned
// extent in its new orientation.  The arithmetic on the 3 x 3 state is the same in every lane (it costs what one lane costs); the
// lanes share the one loop that is as long as the body: the bounds of rot * p over its points, reduced by wave shuffles and one LDS
// row per wave (minimum and maximum do not depend on the order).  Thread 0 then applies the walls and writes the float64 state and the
// float32 pose k_renew_rigid reads.  Every statement is kept as written (no contraction in either build): the host integrator
// rounds every product, and the two are compared to 1e-12.
#pragma once

__device__ __forceinline__ void rb_mul(const double *a, const double *b, double *c) {   // c = a b
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__device__ __forceinline__ void rb_mul_t(const double *a, const double *b, double *c) {   // c = a b^T
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}
__device__ __forceinline__ void rb_mul_v(const double *a, const double *v, double *r) {   // r = a v
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}

// exp([w]x): rotation by |w| about w (Rodrigues), host_rigid_solver.py _skew_exp
__device__ __forceinline__ void rb_skew_exp(const double *w, double *e) {
#pragma clang fp contract(off)
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
    for (int q = 0; q < 9; ++q) e[q] = (q % 4 == 0) ? 1.0 : 0.0;
    if (th < 1e-12) return;
    const double k0 = w[0] / th, k1 = w[1] / th, k2 = w[2] / th;
    const double K[9] = {0.0, -k2, k1, k2, 0.0, -k0, -k1, k0, 0.0};
    double KK[9];
    rb_mul(K, K, KK);
    const double s = sin(th), c1 = 1.0 - cos(th);
#pragma unroll
    for (int q = 0; q < 9; ++q) e[q] = (e[q] + s * K[q]) + c1 * KK[q];
}

// the orthogonal polar factor of a matrix that is a rotation up to rounding (the host's u @ vt of its SVD): Newton's iteration
// X <- (X + X^-T) / 2 converges quadratically from there, three steps are one more than it needs
__device__ __forceinline__ void rb_polar(double *x) {
#pragma clang fp contract(off)
    for (int it = 0; it < 3; ++it) {
        double c[9];   // cofactors: X^-T = C / det X
        c[0] = x[4] * x[8] - x[5] * x[7]; c[1] = x[5] * x[6] - x[3] * x[8]; c[2] = x[3] * x[7] - x[4] * x[6];
        c[3] = x[2] * x[7] - x[1] * x[8]; c[4] = x[0] * x[8] - x[2] * x[6]; c[5] = x[1] * x[6] - x[0] * x[7];
        c[6] = x[1] * x[5] - x[2] * x[4]; c[7] = x[2] * x[3] - x[0] * x[5]; c[8] = x[0] * x[4] - x[1] * x[3];
        const double det = x[0] * c[0] + x[1] * c[1] + x[2] * c[2];
#pragma unroll
        for (int q = 0; q < 9; ++q) x[q] = 0.5 * (x[q] + c[q] / det);
    }
}

__global__ void __launch_bounds__(256)
k_rigid_integrate(const RigidIntArgs a, RigidBodyDev *bodies, DevScalars *scal, RigidPose *pose) {
#pragma clang fp contract(off)
    __shared__ double s_red[4][6];
    const int tid = threadIdx.x;
    const int o = a.ids[blockIdx.x];
    if (o < 0 || o >= SPH_NOBJ) return;   // workgroup-uniform
    RigidBodyDev *b = bodies + o;
    // the wrench as sph_get_rigid_wrench hands it to the host: rounded through float32
    double f[3], t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f[k] = (double)(float)((double)scal->wrench[3 * o + k] / SPH_WRENCH_SCALE);
        t[k] = (double)(float)((double)scal->wrench[SPH_NOBJ * 3 + 3 * o + k] / SPH_WRENCH_SCALE);
    }
    double com[3], rot[9], vel[3], w[3], I[9], Ii[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) { com[k] = b->com[k]; vel[k] = b->vel[k]; w[k] = b->angvel[k]; }
#pragma unroll
    for (int q = 0; q < 9; ++q) { rot[q] = b->rot[q]; I[q] = b->inertia[q]; Ii[q] = b->inertia_inv[q]; }
    const double mass = b->mass, dt = a.dt;
    const double *pts = b->points;
    const int np = b->npoints;
    __syncthreads();   // every lane holds the wrench and the state: both may be overwritten now
    // the launch consumes the whole wrench array (sph_get_rigid_wrench(reset = 1)): every workgroup its body's words, the first one
    // the words of the objects no workgroup reads
    if (tid == 0)
        for (int k = 0; k < 3; ++k) { scal->wrench[3 * o + k] = 0; scal->wrench[SPH_NOBJ * 3 + 3 * o + k] = 0; }
    if (blockIdx.x == 0 && tid >= 64 && tid < 64 + SPH_NOBJ) {
        const int other = tid - 64;
        bool taken = false;
        for (int q = 0; q < a.nbodies; ++q) taken = taken || a.ids[q] == other;
        if (!taken)
            for (int k = 0; k < 3; ++k) { scal->wrench[3 * other + k] = 0; scal->wrench[SPH_NOBJ * 3 + 3 * other + k] = 0; }
    }
    // HostRigidSolver.integrate, statement by statement
    double tmp[9], I_inv[9], I_w[9], Iw[3], rhs[3], dw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vel[k] = vel[k] + dt * (f[k] / mass + a.g[k]);
    rb_mul(rot, Ii, tmp); rb_mul_t(tmp, rot, I_inv);
    rb_mul(rot, I, tmp); rb_mul_t(tmp, rot, I_w);
    rb_mul_v(I_w, w, Iw);
    rhs[0] = t[0] - (w[1] * Iw[2] - w[2] * Iw[1]);
    rhs[1] = t[1] - (w[2] * Iw[0] - w[0] * Iw[2]);
    rhs[2] = t[2] - (w[0] * Iw[1] - w[1] * Iw[0]);
    rb_mul_v(I_inv, rhs, dw);
#pragma unroll
    for (int k = 0; k < 3; ++k) { w[k] = w[k] + dt * dw[k]; com[k] = com[k] + dt * vel[k]; }
    const double dtw[3] = {dt * w[0], dt * w[1], dt * w[2]};
    double e[9];
    rb_skew_exp(dtw, e);
    rb_mul(e, rot, tmp);
    rb_polar(tmp);
#pragma unroll
    for (int q = 0; q < 9; ++q) rot[q] = tmp[q];
    // bounds of the particle set in the new orientation, about the centre of mass
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < np; i += 256) {
        const double p0 = pts[3 * i], p1 = pts[3 * i + 1], p2 = pts[3 * i + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = rot[3 * k] * p0 + rot[3 * k + 1] * p1 + rot[3 * k + 2] * p2;
            lo[k] = fmin(lo[k], v); hi[k] = fmax(hi[k], v);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fmin(lo[k], __shfl_xor(lo[k], off, 64));
            hi[k] = fmax(hi[k], __shfl_xor(hi[k], off, 64));
        }
    if ((tid & 63) == 0)
        for (int k = 0; k < 3; ++k) { s_red[tid >> 6][k] = lo[k]; s_red[tid >> 6][3 + k] = hi[k]; }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = fmin(fmin(s_red[0][k], s_red[1][k]), fmin(s_red[2][k], s_red[3][k]));
        hi[k] = fmax(fmax(s_red[0][3 + k], s_red[1][3 + k]), fmax(s_red[2][3 + k], s_red[3][3 + k]));
        if (np <= 0) lo[k] = hi[k] = 0.0;   // a body without a particle set is a point
    }
    // inelastic contact of that extent with the walls
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (com[k] + lo[k] < a.lo[k] && a.lo[k] - lo[k] <= a.hi[k] - hi[k]) {
            com[k] = a.lo[k] - lo[k];
            vel[k] = fmax(vel[k], 0.0);
        } else if (com[k] + hi[k] > a.hi[k]) {
            com[k] = fmax(a.hi[k] - hi[k], a.lo[k] - lo[k]);
            vel[k] = fmin(vel[k], 0.0);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b->com[k] = com[k]; b->vel[k] = vel[k]; b->angvel[k] = w[k];
        pose->com[o][k] = (float)com[k]; pose->vel[o][k] = (float)vel[k]; pose->angvel[o][k] = (float)w[k];
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) { b->rot[q] = rot[q]; pose->rot[o][q] = (float)rot[q]; }
}

static void l_rigid_integrate(State &s) {
    if (!s.rigid_int_on || s.rigid_int.nbodies <= 0 || !s.rigid_bodies) return;
    hipLaunchKernelGGL(k_rigid_integrate, dim3(s.rigid_int.nbodies), dim3(256), 0, s.stream, s.rigid_int, s.rigid_bodies, s.scal, s.pose);
}

static void register_rigid_launchers(Launch &L) { L.rigid_integrate = l_rigid_integrate; }
