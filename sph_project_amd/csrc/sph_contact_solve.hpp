// sph_contact_solve.hpp -- the device contact solver (the host's "device_contact" rigid backend): kernel and launcher; included by
// sph_kernels.hip inside the per-build namespace, behind sph_rigid.hpp (rb_mul, rb_skew_exp, rb_polar).  Semantics in include/sph_hip.h
// (sph_set_rigid_contact_solver), design in DESIGN.md 20.
//
// ONE workgroup of 256 threads does, between the two halves of a step, what the "contact" backend does on the host
// (SPH/rigid_solver/host_rigid_solver.py: contacts_from_table, then ContactSolver.step), statement by statement and in float64:
//   1. velocity half, one lane per registered body (world inverse inertia, velocities and pseudo-velocities stay in LDS);
//   2. contacts from the table: the SPH_CT_KEYS keys spread over the lanes, 256 at a time in ascending key order, the surviving keys
//      compacted by wave ballots and a prefix over the four waves -- row k here is row k of np.nonzero's (A, B, bin) order;
//   3. row build, by the lane that holds the key (arms, tangents, effective masses, target velocity, bias);
//   4. the launch consumes its inputs: the whole wrench array and the whole table are cleared with ordinary vector stores (all lanes,
//      before one of them is kept busy by the sweeps);
//   5. the sweeps, ONE lane: sequential impulses are sequential across rows, and the host's order is the order compared against;
//   6. positions, one lane per body.
// Rows live in a global buffer sized for every key (SPH_CS_ROW doubles each, under 1 MB: L2-resident); their first
// SPH_CONTACT_ROW_VALUES values are what sph_get_rigid_contact_rows hands out.  No statement is contracted in either build: the host
// rounds every product, and the strict and the fast build give the same bits.
#pragma once

// row layout (doubles): [0] A  [1] B or -1  [2..4] point  [5..7] normal  [8] depth  [9] ln  [10..11] lt  [12..13] lr  [14] lp
// [15] the table's partner index | [16..18] ra  [19..21] rb  [22..24] t1  [25..27] t2  [28] kn  [29..30] kt  [31..32] kr  [33] target
// [34] bias  [35] vn0    (SPH_CS_ROW doubles, sph_common.hpp)

struct ContactSolveLds {
    double inv_i[SPH_NOBJ][9], vel[SPH_NOBJ][3], w[SPH_NOBJ][3], pv[SPH_NOBJ][3], pw[SPH_NOBJ][3], com[SPH_NOBJ][3], mass[SPH_NOBJ];
    int registered[SPH_NOBJ];
    int wave_count[4];
    int base;
};

__device__ __forceinline__ void cs_cross(const double *a, const double *b, double *c) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double cs_dot(const double *a, const double *b) {
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
// d . ((I^-1 (r x d)) x r): the angular part of the effective mass along d at arm r (ContactSolver.step k_of)
__device__ __forceinline__ double cs_k_ang(const double *inv_i, const double *r, const double *d) {
#pragma clang fp contract(off)
    double rxd[3], t[3], c[3];
    cs_cross(r, d, rxd);
    rb_mul_v(inv_i, rxd, t);
    cs_cross(t, r, c);
    return cs_dot(d, c);
}
// t . I^-1 . t as the host evaluates it: (t^T I^-1) t
__device__ __forceinline__ double cs_quad(const double *inv_i, const double *t) {
#pragma clang fp contract(off)
    double r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = t[0] * inv_i[j] + t[1] * inv_i[3 + j] + t[2] * inv_i[6 + j];
    return cs_dot(r, t);
}
// ContactSolver._rel on the LDS state
__device__ __forceinline__ void cs_rel(const ContactSolveLds &s, int a, int b, const double *ra, const double *rb, double *v) {
#pragma clang fp contract(off)
    double c[3];
    cs_cross(s.w[a], ra, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = s.vel[a][k] + c[k];
    if (b >= 0) {
        cs_cross(s.w[b], rb, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] - s.vel[b][k] - c[k];
    }
}
// ContactSolver._apply on (vel, w) or, for the split impulses, on (pv, pw)
__device__ __forceinline__ void cs_apply(const ContactSolveLds &s, double (*lin)[3], double (*ang)[3], int a, int b, const double *ra,
                                         const double *rb, const double *j) {
#pragma clang fp contract(off)
    double c[3], d[3];
    cs_cross(ra, j, c);
    rb_mul_v(s.inv_i[a], c, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) { lin[a][k] = lin[a][k] + j[k] / s.mass[a]; ang[a][k] = ang[a][k] + d[k]; }
    if (b >= 0) {
        cs_cross(rb, j, c);
        rb_mul_v(s.inv_i[b], c, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) { lin[b][k] = lin[b][k] - j[k] / s.mass[b]; ang[b][k] = ang[b][k] - d[k]; }
    }
}

__global__ void __launch_bounds__(256)
k_rigid_contact_solve(const RigidIntArgs a, const ContactSolveArgs p, RigidBodyDev *bodies, DevScalars *scal, RigidPose *pose,
                      unsigned long long *table, double *rows, int *nrows) {
#pragma clang fp contract(off)
    __shared__ ContactSolveLds s;
    const int tid = threadIdx.x;
    const double dt = a.dt;
    if (tid < SPH_NOBJ) s.registered[tid] = 0;
    if (tid == 0) s.base = 0;
    __syncthreads();
    const int o = tid < a.nbodies ? a.ids[tid] : -1;   // this lane's body (stages 1 and 6)
    const bool mine = o >= 0 && o < SPH_NOBJ;
    // ---- 1. velocity half: ContactSolver.step's first loop
    if (mine) {
        const RigidBodyDev *b = bodies + o;
        double f[3], t[3], vel[3], w[3], rot[9], I[9], Ii[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // the wrench as sph_get_rigid_wrench hands it to the host: rounded through float32
            f[k] = (double)(float)((double)scal->wrench[3 * o + k] / SPH_WRENCH_SCALE);
            t[k] = (double)(float)((double)scal->wrench[SPH_NOBJ * 3 + 3 * o + k] / SPH_WRENCH_SCALE);
            vel[k] = b->vel[k]; w[k] = b->angvel[k];
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) { rot[q] = b->rot[q]; I[q] = b->inertia[q]; Ii[q] = b->inertia_inv[q]; }
        const double mass = b->mass;
        double tmp[9], I_inv[9], I_w[9], Iw[3], rhs[3], dw[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) vel[k] = vel[k] + dt * (f[k] / mass + a.g[k]);
        rb_mul(rot, I, tmp); rb_mul_t(tmp, rot, I_w);
        rb_mul(rot, Ii, tmp); rb_mul_t(tmp, rot, I_inv);
        rb_mul_v(I_w, w, Iw);
        rhs[0] = t[0] - (w[1] * Iw[2] - w[2] * Iw[1]);
        rhs[1] = t[1] - (w[2] * Iw[0] - w[0] * Iw[2]);
        rhs[2] = t[2] - (w[0] * Iw[1] - w[1] * Iw[0]);
        rb_mul_v(I_inv, rhs, dw);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s.vel[o][k] = vel[k]; s.w[o][k] = w[k] + dt * dw[k]; s.pv[o][k] = 0.0; s.pw[o][k] = 0.0; s.com[o][k] = b->com[k];
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) s.inv_i[o][q] = I_inv[q];
        s.mass[o] = mass;
        s.registered[o] = 1;
    }
    __syncthreads();
    // ---- 2. + 3. contacts_from_table and the row build, 256 keys at a time in ascending key order
    const double v_thr = 2.0 * sqrt(a.g[0] * a.g[0] + a.g[1] * a.g[1] + a.g[2] * a.g[2]) * dt;
    for (int k0 = 0; k0 < SPH_CT_KEYS; k0 += 256) {
        const int key = k0 + tid;
        bool keep = false;
        int A = 0, B = 0, bin = 0, partner = -1;
        double cnt = 0.0, sum_m[3] = {0.0, 0.0, 0.0}, dn[3] = {0.0, 0.0, 0.0}, nrm = 0.0, depth = 0.0;
        if (key < SPH_CT_KEYS) {
            const long long *v = (const long long *)table + (size_t)key * SPH_CT_VALUES;
            bin = key % SPH_CT_BINS; B = (key / SPH_CT_BINS) % SPH_CT_PARTNERS; A = key / (SPH_CT_BINS * SPH_CT_PARTNERS);
            const long long c0 = v[0];
            if (c0 > 0 && s.registered[A]) {
                partner = (B < SPH_NOBJ && s.registered[B]) ? B : -1;
                if (!(partner >= 0 && partner < A)) {
                    cnt = (double)c0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {   // contact_to_scene's conversion
                        sum_m[k] = (double)v[1 + k] / SPH_WRENCH_SCALE;
                        dn[k] = (double)v[4 + k] / SPH_WRENCH_SCALE;
                    }
                    depth = (double)(unsigned long long)v[7] / SPH_WRENCH_SCALE;
                    nrm = sqrt(dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2]);
                    keep = nrm > 0.0;
                }
            }
        }
        const unsigned long long ballot = __ballot(keep);
        const int lane = tid & 63, wave = tid >> 6;
        if (lane == 0) s.wave_count[wave] = __popcll(ballot);
        __syncthreads();
        int row = s.base + __popcll(ballot & ((1ull << lane) - 1ull));
        for (int q = 0; q < wave; ++q) row += s.wave_count[q];
        const int total = s.wave_count[0] + s.wave_count[1] + s.wave_count[2] + s.wave_count[3];
        if (keep && row < SPH_CT_KEYS) {
            double n[3], pt[3], ra[3], rb[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 3; ++k) { n[k] = dn[k] / nrm; pt[k] = sum_m[k] / cnt; }
            if (B >= SPH_NOBJ) {   // the domain box / a wall plane: an axis-aligned face, its normal is the bin's axis
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] = k == bin / 2 ? ((bin & 1) ? -1.0 : 1.0) : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { ra[k] = pt[k] - s.com[A][k]; if (partner >= 0) rb[k] = pt[k] - s.com[partner][k]; }
            // _tangents(n)
            const bool along_x = fabs(n[0]) < 0.9;
            const double u[3] = {along_x ? 1.0 : 0.0, along_x ? 0.0 : 1.0, 0.0};
            double t1[3], t2[3];
            cs_cross(n, u, t1);
            const double tn = sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) t1[k] = t1[k] / tn;
            cs_cross(n, t1, t2);
            // k_of(n), k_of(t1), k_of(t2), kr
            double kk[3], kr[2];
            const double *dirs[3] = {n, t1, t2};
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                double k = 1.0 / s.mass[A] + cs_k_ang(s.inv_i[A], ra, dirs[q]);
                if (partner >= 0) k += 1.0 / s.mass[partner] + cs_k_ang(s.inv_i[partner], rb, dirs[q]);
                kk[q] = k;
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) kr[q] = cs_quad(s.inv_i[A], dirs[1 + q]) + (partner >= 0 ? cs_quad(s.inv_i[partner], dirs[1 + q]) : 0.0);
            double vrel[3];
            cs_rel(s, A, partner, ra, rb, vrel);
            const double vn0 = cs_dot(vrel, n);
            const double target = vn0 < -v_thr ? -p.e * vn0 : 0.0;
            const double bias = p.beta * fmax(depth - p.slop, 0.0) / dt;
            double *r = rows + (size_t)row * SPH_CS_ROW;
            r[0] = (double)A; r[1] = (double)partner; r[8] = depth; r[9] = 0.0; r[10] = 0.0; r[11] = 0.0; r[12] = 0.0; r[13] = 0.0;
            r[14] = 0.0; r[15] = (double)B;
#pragma unroll
            for (int k = 0; k < 3; ++k) { r[2 + k] = pt[k]; r[5 + k] = n[k]; r[16 + k] = ra[k]; r[19 + k] = rb[k]; r[22 + k] = t1[k]; r[25 + k] = t2[k]; }
            r[28] = kk[0]; r[29] = kk[1]; r[30] = kk[2]; r[31] = kr[0]; r[32] = kr[1]; r[33] = target; r[34] = bias; r[35] = vn0;
        }
        __syncthreads();   // every lane has read base and the wave counts
        if (tid == 0) s.base += total;
        __syncthreads();
    }
    const int nr = s.base < SPH_CT_KEYS ? s.base : SPH_CT_KEYS;
    // ---- 4. the launch consumes its inputs (sph_get_rigid_wrench(reset = 1), sph_get_rigid_contacts(reset = 1)); every lane has read
    // what it needed of both behind the barrier above
    for (int q = tid; q < 2 * SPH_NOBJ * 3; q += 256) scal->wrench[q] = 0;
    for (int q = tid; q < SPH_CT_KEYS * SPH_CT_VALUES; q += 256) table[q] = 0ull;
    __threadfence_block();
    __syncthreads();   // the rows are in memory
    // ---- 5. the sweeps: one lane, the host's statements in the host's order
    if (tid == 0) {
        *nrows = nr;
        for (int it = 0; it < p.iterations; ++it)
            for (int c = 0; c < nr; ++c) {
                double *r = rows + (size_t)c * SPH_CS_ROW;
                const int A = (int)r[0], B = (int)r[1];
                const double n[3] = {r[5], r[6], r[7]}, ra[3] = {r[16], r[17], r[18]}, rb[3] = {r[19], r[20], r[21]};
                const double t1[3] = {r[22], r[23], r[24]}, t2[3] = {r[25], r[26], r[27]};
                const double kn = r[28], kt0 = r[29], kt1 = r[30], kr0 = r[31], kr1 = r[32], target = r[33];
                const double ln0 = r[9], lt0[2] = {r[10], r[11]}, lr0[2] = {r[12], r[13]};
                double vrel[3], j[3];
                cs_rel(s, A, B, ra, rb, vrel);
                const double ln = fmax(ln0 + (target - cs_dot(vrel, n)) / kn, 0.0);
#pragma unroll
                for (int k = 0; k < 3; ++k) j[k] = (ln - ln0) * n[k];
                cs_apply(s, s.vel, s.w, A, B, ra, rb, j);
                cs_rel(s, A, B, ra, rb, vrel);
                double lt[2] = {lt0[0] - cs_dot(vrel, t1) / kt0, lt0[1] - cs_dot(vrel, t2) / kt1};
                double cap = p.mu * ln, mag = sqrt(lt[0] * lt[0] + lt[1] * lt[1]);
                if (mag > cap) { const double f = cap / mag; lt[0] = lt[0] * f; lt[1] = lt[1] * f; }
                double d0 = lt[0] - lt0[0], d1 = lt[1] - lt0[1];
#pragma unroll
                for (int k = 0; k < 3; ++k) j[k] = d0 * t1[k] + d1 * t2[k];
                cs_apply(s, s.vel, s.w, A, B, ra, rb, j);
                // rolling resistance: the relative spin about the tangents, within mu lambda_n patch
                double wrel[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) wrel[k] = s.w[A][k] - (B >= 0 ? s.w[B][k] : 0.0);
                double lr[2] = {lr0[0] - cs_dot(wrel, t1) / kr0, lr0[1] - cs_dot(wrel, t2) / kr1};
                cap = p.mu * ln * p.patch; mag = sqrt(lr[0] * lr[0] + lr[1] * lr[1]);
                if (mag > cap) { const double f = cap / mag; lr[0] = lr[0] * f; lr[1] = lr[1] * f; }
                d0 = lr[0] - lr0[0]; d1 = lr[1] - lr0[1];
                double m[3], im[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) m[k] = d0 * t1[k] + d1 * t2[k];
                rb_mul_v(s.inv_i[A], m, im);
#pragma unroll
                for (int k = 0; k < 3; ++k) s.w[A][k] = s.w[A][k] + im[k];
                if (B >= 0) {
                    rb_mul_v(s.inv_i[B], m, im);
#pragma unroll
                    for (int k = 0; k < 3; ++k) s.w[B][k] = s.w[B][k] - im[k];
                }
                r[9] = ln; r[10] = lt[0]; r[11] = lt[1]; r[12] = lr[0]; r[13] = lr[1];
            }
        // split impulses on the pseudo-velocities
        for (int it = 0; it < p.iterations; ++it)
            for (int c = 0; c < nr; ++c) {
                double *r = rows + (size_t)c * SPH_CS_ROW;
                const int A = (int)r[0], B = (int)r[1];
                const double n[3] = {r[5], r[6], r[7]}, ra[3] = {r[16], r[17], r[18]}, rb[3] = {r[19], r[20], r[21]};
                const double kn = r[28], bias = r[34], lp0 = r[14];
                double cr[3], vp[3], j[3];
                cs_cross(s.pw[A], ra, cr);
#pragma unroll
                for (int k = 0; k < 3; ++k) vp[k] = s.pv[A][k] + cr[k];
                if (B >= 0) {
                    cs_cross(s.pw[B], rb, cr);
#pragma unroll
                    for (int k = 0; k < 3; ++k) vp[k] = vp[k] - s.pv[B][k] - cr[k];
                }
                const double lp = fmax(lp0 + (bias - cs_dot(vp, n)) / kn, 0.0);
#pragma unroll
                for (int k = 0; k < 3; ++k) j[k] = (lp - lp0) * n[k];
                r[14] = lp;
                cs_apply(s, s.pv, s.pw, A, B, ra, rb, j);
            }
    }
    __syncthreads();
    // ---- 6. positions: x += dt (v + pv), R <- polar(exp([dt (w + pw)]x) R); the float64 state and the float32 pose k_renew_rigid reads
    if (mine) {
        RigidBodyDev *b = bodies + o;
        double dtw[3], e[9], rot[9], tmp[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) rot[q] = b->rot[q];
#pragma unroll
        for (int k = 0; k < 3; ++k) dtw[k] = dt * (s.w[o][k] + s.pw[o][k]);
        rb_skew_exp(dtw, e);
        rb_mul(e, rot, tmp);
        rb_polar(tmp);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double com = s.com[o][k] + dt * (s.vel[o][k] + s.pv[o][k]), vel = s.vel[o][k], w = s.w[o][k];
            b->com[k] = com; b->vel[k] = vel; b->angvel[k] = w;
            pose->com[o][k] = (float)com; pose->vel[o][k] = (float)vel; pose->angvel[o][k] = (float)w;
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) { b->rot[q] = tmp[q]; pose->rot[o][q] = (float)tmp[q]; }
    }
}

static void l_rigid_contact_solve(State &s) {
    if (!s.rigid_int_on || !s.contact_solve_on || s.rigid_int.nbodies <= 0 || !s.rigid_bodies || !s.contact_table || !s.contact_rows) return;
    hipLaunchKernelGGL(k_rigid_contact_solve, dim3(1), dim3(256), 0, s.stream, s.rigid_int, s.contact_solve, s.rigid_bodies, s.scal, s.pose,
                       s.contact_table, s.contact_rows, s.contact_nrows);
}

static void register_contact_solve_launchers(Launch &L) { L.rigid_contact_solve = l_rigid_contact_solve; }
