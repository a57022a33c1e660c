// sph_elastic.hpp -- elastic solids: corotated linear SPH elasticity per fluid object (opt-in: sph_set_elastic_object).
// After Becker, Ihmsen, Teschner 2009 and SPlisHSPlasH's Elasticity_Becker2009, on a kernel-corrected rest configuration, with the
// rotation extraction of Mueller, Bender, Chentanez, Macklin 2016.  The particles of an elastic object stay material_fluid; the model is
// one more acceleration behind the non-pressure pass.  With x0 the positions at capture, x0_ji = x0_j - x0_i, gradW0_ij = gradW(x0_i - x0_j),
// V0 the rest volume, N0_i the same-object neighbours the step's acceptance test (r2 < h2 on the f32 differences) accepts at capture:
//   capture:   M_i = sum_{j in N0_i} V0 x0_ji (x) gradW0_ij;   g0_ij = M_i^-1 gradW0_ij (float64, rounded to f32);   q_i = identity
//   per step:  F_i = sum_j V0 (x_j - x_i) (x) g0_ij;   R_i = rotation of F_i (ELASTIC_ROT_ITERS warm-started iterations on q_i)
//              eps_i = 1/2 (F_i R_i^T + R_i F_i^T) - I;   sig_i = 2 mu eps_i + lambda tr(eps_i) I
//              a_el_i = (V0^2 / m_i) sum_j (sig_i R_i g0_ij - sig_j R_j g0_ji);   v_i <- v_i + dt a_el_i is k_elastic_apply's
// Rest neighbours need not be current neighbours, so the passes are driven by LISTS of persistent particle ids fixed at capture, not by
// the neighbour-walk framework.  Everything a list names lives AT HOME, indexed by id (ids = append order, as State::mp_w_home): the
// scatter brings positions and slots home, pass A (k_elastic_rotation) writes q, sigma and F of its own row, pass B (k_elastic_force)
// reads q and sigma of the listed neighbours.  No atomics, no LDS, no sums across lanes: every sum runs in list order.
// The per-particle arithmetic is ONE source for the kernels (both builds), the host entry sph_elastic_particle_host (sph_api.hip) and
// through it the CPU tests and tools/check_elastic.cpp.  The kernels exist in the kernel translation units only.
// Symmetric tensors are (xx, xy, xz, yy, yz, zz); matrices are row-major [row * 3 + column]; quaternions are (x, y, z, w).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define EL_HD __host__ __device__ static inline
#else
#define EL_HD static inline
#endif

#define ELASTIC_MAX_NEIGHBOURS 64   // = SPH_ELASTIC_MAX_NEIGHBOURS (sph_hip.h): a longer list refuses its object, it is never truncated
#define ELASTIC_ROT_ITERS 10
#define ELASTIC_MIN_EIG_RATIO 1e-3  // smallest / largest eigenvalue of M below this: degenerate (a sheet, fewer than three non-coplanar neighbours)

// a b + c: the strict form takes the product and the sum as written (its translation units compile with -ffp-contract=off), the fast
// form is one fused operation -- spelled out, so the host entry gives the fast kernels' arithmetic without a compiler flag
template <bool FAST> EL_HD float el_madd(float a, float b, float c) { return FAST ? fmaf(a, b, c) : a * b + c; }

// F += V0 (x_j - x_i) (x) g0_ij, one list entry; (dx, dy, dz) = x_j - x_i
template <bool FAST>
EL_HD void el_deformation_entry(float F[9], float V0, float dx, float dy, float dz, float gx, float gy, float gz) {
    const float vx = V0 * dx, vy = V0 * dy, vz = V0 * dz;
    F[0] = el_madd<FAST>(vx, gx, F[0]); F[1] = el_madd<FAST>(vx, gy, F[1]); F[2] = el_madd<FAST>(vx, gz, F[2]);
    F[3] = el_madd<FAST>(vy, gx, F[3]); F[4] = el_madd<FAST>(vy, gy, F[4]); F[5] = el_madd<FAST>(vy, gz, F[5]);
    F[6] = el_madd<FAST>(vz, gx, F[6]); F[7] = el_madd<FAST>(vz, gy, F[7]); F[8] = el_madd<FAST>(vz, gz, F[8]);
}

// the rotation matrix of a unit quaternion
EL_HD void el_quat_matrix(const float q[4], float R[9]) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0f - 2.0f * (yy + zz); R[1] = 2.0f * (xy - wz);        R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz);        R[4] = 1.0f - 2.0f * (xx + zz); R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy);        R[7] = 2.0f * (yz + wx);        R[8] = 1.0f - 2.0f * (xx + yy);
}

// Mueller et al. 2016: q <- normalize(quat(axis om / |om|, angle |om|) q) with om = sum_k r_k x f_k / (|sum_k r_k . f_k| + 1e-9) over the
// columns of R = mat(q) and F; `iters` iterations, stop when |om| < 1e-9.  q comes in as the warm start and goes out as the result.
EL_HD void el_extract_rotation(float q[4], const float F[9], int iters) {
    for (int it = 0; it < iters; ++it) {
        float R[9];
        el_quat_matrix(q, R);
        float ox = 0.0f, oy = 0.0f, oz = 0.0f, dot = 0.0f;
        for (int k = 0; k < 3; ++k) {
            const float rx = R[k], ry = R[3 + k], rz = R[6 + k], fx = F[k], fy = F[3 + k], fz = F[6 + k];
            ox += ry * fz - rz * fy; oy += rz * fx - rx * fz; oz += rx * fy - ry * fx;
            dot += rx * fx + ry * fy + rz * fz;
        }
        const float inv = 1.0f / (fabsf(dot) + 1e-9f);
        ox *= inv; oy *= inv; oz *= inv;
        const float w = sqrtf(ox * ox + oy * oy + oz * oz);
        if (w < 1e-9f) break;
        const float s = sinf(0.5f * w) / w, c = cosf(0.5f * w);
        const float dx = s * ox, dy = s * oy, dz = s * oz;
        // dq q (Hamilton product), dq = (dx, dy, dz, c)
        const float nx = c * q[0] + q[3] * dx + (dy * q[2] - dz * q[1]);
        const float ny = c * q[1] + q[3] * dy + (dz * q[0] - dx * q[2]);
        const float nz = c * q[2] + q[3] * dz + (dx * q[1] - dy * q[0]);
        const float nw = c * q[3] - (dx * q[0] + dy * q[1] + dz * q[2]);
        const float rn = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz + nw * nw);
        q[0] = nx * rn; q[1] = ny * rn; q[2] = nz * rn; q[3] = nw * rn;
    }
}

// eps = 1/2 (F R^T + R F^T) - I;  sig = 2 mu eps + lambda tr(eps) I
EL_HD void el_stress(const float F[9], const float R[9], float mu, float lambda, float sig[6]) {
    float A[9];   // F R^T
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) A[3 * a + b] = F[3 * a] * R[3 * b] + F[3 * a + 1] * R[3 * b + 1] + F[3 * a + 2] * R[3 * b + 2];
    const float exx = A[0] - 1.0f, eyy = A[4] - 1.0f, ezz = A[8] - 1.0f;
    const float exy = 0.5f * (A[1] + A[3]), exz = 0.5f * (A[2] + A[6]), eyz = 0.5f * (A[5] + A[7]);
    const float lt = lambda * (exx + eyy + ezz), m2 = 2.0f * mu;
    sig[0] = m2 * exx + lt; sig[1] = m2 * exy; sig[2] = m2 * exz;
    sig[3] = m2 * eyy + lt; sig[4] = m2 * eyz; sig[5] = m2 * ezz + lt;
}

// y = sig (R g)
EL_HD void el_stress_rot_vec(const float sig[6], const float R[9], float gx, float gy, float gz, float y[3]) {
    const float tx = R[0] * gx + R[1] * gy + R[2] * gz, ty = R[3] * gx + R[4] * gy + R[5] * gz, tz = R[6] * gx + R[7] * gy + R[8] * gz;
    y[0] = sig[0] * tx + sig[1] * ty + sig[2] * tz;
    y[1] = sig[1] * tx + sig[3] * ty + sig[4] * tz;
    y[2] = sig[2] * tx + sig[4] * ty + sig[5] * tz;
}

// acc += sig_i R_i g0_ij - sig_j R_j g0_ji, one list entry (antisymmetric in (i, j): the pair's momentum is zero to rounding)
EL_HD void el_pair_force(float acc[3], const float sig_i[6], const float R_i[9], const float gij[3], const float sig_j[6],
                         const float R_j[9], const float gji[3]) {
    float a[3], b[3];
    el_stress_rot_vec(sig_i, R_i, gij[0], gij[1], gij[2], a);
    el_stress_rot_vec(sig_j, R_j, gji[0], gji[1], gji[2], b);
    acc[0] += a[0] - b[0]; acc[1] += a[1] - b[1]; acc[2] += a[2] - b[2];
}

#ifdef SPH_LAUNCH_FN   // ------------------------------------------------------------------ kernel translation units only

// Positions and slots of the elastic objects' particles go home: x_home[id] = posv[i], slot_home[id] = i.  `mask`: bit o = object o is
// elastic and captured -- the per-object table is the only test.  (ids are the append order: < cap.)
__global__ void __launch_bounds__(256)
k_elastic_scatter(int n, int cap, unsigned mask, const int *__restrict__ meta, const int *__restrict__ pid, const float4 *__restrict__ posv,
                  float4 *__restrict__ x_home, int *__restrict__ slot_home) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int o = META_OBJ(meta[i]);
    if (o < 0 || o >= SPH_NOBJ || !((mask >> o) & 1u)) return;
    const int id = pid[i];
    if ((unsigned)id >= (unsigned)cap) return;
    x_home[id] = posv[i];
    slot_home[id] = i;
}

// entry k of row `row`: plane 0 = (g0_ij, bits of j), plane 1 = (g0_ji, 0); k-major, so a wave's 64 rows are 1 KiB in a row
__device__ __forceinline__ const float4 *el_entry(const ElObjDev &o, int k, int plane, int row) {
    return o.rest + ((size_t)(2 * k + plane) * (size_t)o.n + (size_t)row);
}

// Pass A: one lane per particle of one elastic object, addressed by id.  Reads x_home and the warm start q_prev; writes q, sigma
// (two float4 per id: xx xy xz yy | yz zz 0 0) and F (three float4 per id, the rows) of its own row.
// Bytes / particle with a list of K entries: R K (16 table + 16 x_home) + 16 + 16 -> W 16 + 32 + 48.
__global__ void __launch_bounds__(256)
k_elastic_rotation(const ElObjDev o, float V0, const float4 *__restrict__ x_home, const float4 *__restrict__ q_prev,
                   float4 *__restrict__ q_out, float4 *__restrict__ sig_out, float4 *__restrict__ F_out) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= o.n) return;
    const int id = o.id0 + row;
    const float4 xi = x_home[id];
    float F[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int k = 0; k < o.kmax; ++k) {
        const float4 e = *el_entry(o, k, 0, row);
        const int j = __float_as_int(e.w);
        if (j < 0) break;
        const float4 xj = ldg_idx(x_home, j);
        el_deformation_entry<SPH_FAST != 0>(F, V0, xj.x - xi.x, xj.y - xi.y, xj.z - xi.z, e.x, e.y, e.z);
    }
    const float4 qp = q_prev[id];
    float q[4] = {qp.x, qp.y, qp.z, qp.w}, R[9], sig[6];
    el_extract_rotation(q, F, ELASTIC_ROT_ITERS);
    el_quat_matrix(q, R);
    el_stress(F, R, o.mu, o.lambda, sig);
    q_out[id] = make_float4(q[0], q[1], q[2], q[3]);
    sig_out[2 * (size_t)id] = make_float4(sig[0], sig[1], sig[2], sig[3]);
    sig_out[2 * (size_t)id + 1] = make_float4(sig[4], sig[5], 0.0f, 0.0f);
    F_out[3 * (size_t)id] = make_float4(F[0], F[1], F[2], 0.0f);
    F_out[3 * (size_t)id + 1] = make_float4(F[3], F[4], F[5], 0.0f);
    F_out[3 * (size_t)id + 2] = make_float4(F[6], F[7], F[8], 0.0f);
}

// Pass B: the same shape.  Reads q and sigma of its own row and of the listed neighbours (pass A's output), the particle's slot and
// mass; writes a_el[slot] (sorted order, valid until the next sort).
// Bytes / particle: R K (32 table + 16 q + 32 sigma) + 16 + 32 + 4 + 16 -> W 16.
__global__ void __launch_bounds__(256)
k_elastic_force(const ElObjDev o, float V0, const float4 *__restrict__ q_home, const float4 *__restrict__ sig_home,
                const int *__restrict__ slot_home, const float4 *__restrict__ velm, float4 *__restrict__ a_el) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= o.n) return;
    const int id = o.id0 + row;
    const float4 qi = q_home[id], s0 = sig_home[2 * (size_t)id], s1 = sig_home[2 * (size_t)id + 1];
    const float qv[4] = {qi.x, qi.y, qi.z, qi.w}, sig_i[6] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y};
    float R_i[9], acc[3] = {0.0f, 0.0f, 0.0f};
    el_quat_matrix(qv, R_i);
#pragma unroll 1
    for (int k = 0; k < o.kmax; ++k) {
        const float4 e = *el_entry(o, k, 0, row);
        const int j = __float_as_int(e.w);
        if (j < 0) break;
        const float4 f = *el_entry(o, k, 1, row);
        const float4 qj = ldg_idx(q_home, j), t0 = sig_home[2 * (size_t)j], t1 = sig_home[2 * (size_t)j + 1];   // (2 j: past ldg_idx's 32-bit byte offset)
        const float qw[4] = {qj.x, qj.y, qj.z, qj.w}, sig_j[6] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y};
        const float gij[3] = {e.x, e.y, e.z}, gji[3] = {f.x, f.y, f.z};
        float R_j[9];
        el_quat_matrix(qw, R_j);
        el_pair_force(acc, sig_i, R_i, gij, sig_j, R_j, gji);
    }
    const int slot = slot_home[id];
    const float coef = fdiv(V0 * V0, velm[slot].w);
    a_el[slot] = make_float4(coef * acc[0], coef * acc[1], coef * acc[2], 0.0f);
}

// v += dt a_el behind the non-pressure phase, acc += a_el where a non-pressure acceleration is kept: the twin of k_micropolar_apply,
// over rows of elastic objects only (pass B wrote no other row of a_el)
__global__ void __launch_bounds__(256)
k_elastic_apply(const Consts c, unsigned mask, const int *__restrict__ meta, const float4 *__restrict__ a_el, float4 *__restrict__ velm,
                float4 *__restrict__ acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    const int m = meta[i], o = META_OBJ(m);
    if (!META_ACTIVE_FLUID(m) || o < 0 || o >= SPH_NOBJ || !((mask >> o) & 1u)) return;
    const float4 a = a_el[i];
    float4 v = velm[i];
    v.x += c.dt * a.x; v.y += c.dt * a.y; v.z += c.dt * a.z;
    velm[i] = v;
    if (acc) { float4 q = acc[i]; q.x += a.x; q.y += a.y; q.z += a.z; acc[i] = q; }
}

// ---------------------------------------------------------------------------------- capture (once per object)
// One lane per row of the object, behind a scatter that brought its positions and slots home.  A plain 27-cell walk around the
// particle's sorted cell (as sph_contact.hpp / sph_pbf.hpp) lists the same-object fluid neighbours the step's acceptance test accepts,
// in ascending id; M, its eigenvalue ratio (the Jacobi rotations of sph_surface_aniso_eig.hpp on M / max diagonal) and its inverse
// (float64 cofactors); g0_ij into plane 0 of the list table, -1 behind the list's end.  cnt: [0] longest list (the true count, also
// past the table's 64 entries), [1] degenerate particles, [2] bits of the smallest eigenvalue ratio, [3] inconsistencies (an id outside
// the object's range; k_elastic_partner: a partner that does not list the particle back).
__global__ void __launch_bounds__(256)
k_elastic_capture(const Consts c, const ElCaptureArgs a, const int *__restrict__ cell_start, const float4 *__restrict__ posv,
                  const int *__restrict__ meta, const int *__restrict__ pid, const float4 *__restrict__ x_home,
                  const int *__restrict__ slot_home, float4 *__restrict__ q_home, float4 *__restrict__ sig_home,
                  float4 *__restrict__ F_home) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= a.n) return;
    const int id = a.id0 + row, i = slot_home[id];
    const float4 p = posv[i];
    // the list is kept in the table itself (the w words of this row's plane-0 entries), not in a per-lane array: no scratch
    const size_t n = (size_t)a.n;
    float4 *const col = a.rest + row;
#define EL_NB(k) col[(size_t)(2 * (k)) * n]
    int cnt = 0;
    {
        const int cx = cell_coord_x(c, p.x), cy = cell_coord(p.y, c.grid_size, c.ny), cz = cell_coord_z(c, p.z);
        const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz < c.nz - 1 ? cz + 1 : c.nz - 1;
        for (int ox = -1; ox <= 1; ++ox) {
            const int x = cx + ox;
            if (x < 0 || x >= c.nx) continue;
            for (int oy = -1; oy <= 1; ++oy) {
                const int y = cy + oy;
                if (y < 0 || y >= c.ny) continue;
                const int b = cell_start[(x * c.ny + y) * c.nz + z0], e = cell_start[(x * c.ny + y) * c.nz + z1 + 1];
                for (int j = b; j < e; ++j) {
                    if (j == i) continue;
                    const float4 q = ldg_idx(posv, j);
                    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
                    const float r2 = dx * dx + dy * dy + dz * dz;
                    if (!(r2 < c.h2)) continue;
                    const int mj = ldg_idx(meta, j);
                    if (META_OBJ(mj) != a.obj || META_MAT(mj) != 1) continue;
                    const int idj = ldg_idx(pid, j);
                    if (idj < a.id0 || idj >= a.id0 + a.n) { atomicAdd(&a.cnt[3], 1u); continue; }
                    if (cnt < ELASTIC_MAX_NEIGHBOURS) EL_NB(cnt) = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(idj));
                    ++cnt;
                }
            }
        }
    }
    atomicMax(&a.cnt[0], (unsigned)cnt);
    q_home[id] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    sig_home[2 * (size_t)id] = sig_home[2 * (size_t)id + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    F_home[3 * (size_t)id] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    F_home[3 * (size_t)id + 1] = make_float4(0.0f, 1.0f, 0.0f, 0.0f);
    F_home[3 * (size_t)id + 2] = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    if (cnt > ELASTIC_MAX_NEIGHBOURS) {   // the object is refused (SPH_ERR_CAPACITY): no list is written, none is truncated
        for (int k = 0; k < ELASTIC_MAX_NEIGHBOURS; ++k) EL_NB(k) = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
        return;
    }
    for (int k = 1; k < cnt; ++k) {   // ascending id (insertion sort on the lane's own column)
        const float4 v = EL_NB(k);
        int t = k - 1;
        while (t >= 0 && __float_as_int(EL_NB(t).w) > __float_as_int(v.w)) { EL_NB(t + 1) = EL_NB(t); --t; }
        EL_NB(t + 1) = v;
    }
    double M[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double V0 = (double)c.V0;
    for (int k = 0; k < cnt; ++k) {
        const float4 q = ldg_idx(x_home, __float_as_int(EL_NB(k).w));
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        float gx, gy, gz;
        kernGrad(c, dx, dy, dz, geom(c, dx * dx + dy * dy + dz * dz), gx, gy, gz);
        const double d[3] = {-(double)dx, -(double)dy, -(double)dz}, g[3] = {(double)gx, (double)gy, (double)gz};
        for (int r = 0; r < 3; ++r)
            for (int s = 0; s < 3; ++s) M[3 * r + s] += V0 * d[r] * g[s];
    }
    // eigenvalue ratio of the symmetric part, scaled by its largest diagonal entry
    float ratio = 0.0f;
    {
        const float m = (float)fmax(M[0], fmax(M[4], M[8]));
        if (cnt >= 3 && m > 0.0f && m < 3.0e38f) {
            float v[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}}, e[3][3];
            for (int r = 0; r < 3; ++r)
                for (int s = 0; s < 3; ++s) e[r][s] = (float)(0.5 * (M[3 * r + s] + M[3 * s + r])) / m;
            {
                float (&a)[3][3] = e;   // (the macro's names)
#pragma unroll 1
                for (int sweep = 0; sweep < SURF_ANISO_SWEEPS; ++sweep) {
                    SURF_JACOBI_ROTATE(0, 1, 2);
                    SURF_JACOBI_ROTATE(0, 2, 1);
                    SURF_JACOBI_ROTATE(1, 2, 0);
                }
            }
            const float hi = fmaxf(e[0][0], fmaxf(e[1][1], e[2][2])), lo = fminf(e[0][0], fminf(e[1][1], e[2][2]));
            ratio = (hi > 0.0f && lo > 0.0f) ? lo / hi : 0.0f;
        }
    }
    atomicMin(&a.cnt[2], __float_as_uint(ratio));
    const bool degenerate = !(ratio >= (float)ELASTIC_MIN_EIG_RATIO);
    double Mi[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (degenerate) atomicAdd(&a.cnt[1], 1u);
    else {
        const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
        const double det = M[0] * c00 + M[1] * c01 + M[2] * c02, id_ = 1.0 / det;
        Mi[0] = c00 * id_; Mi[1] = (M[2] * M[7] - M[1] * M[8]) * id_; Mi[2] = (M[1] * M[5] - M[2] * M[4]) * id_;
        Mi[3] = c01 * id_; Mi[4] = (M[0] * M[8] - M[2] * M[6]) * id_; Mi[5] = (M[2] * M[3] - M[0] * M[5]) * id_;
        Mi[6] = c02 * id_; Mi[7] = (M[1] * M[6] - M[0] * M[7]) * id_; Mi[8] = (M[0] * M[4] - M[1] * M[3]) * id_;
    }
    for (int k = 0; k < ELASTIC_MAX_NEIGHBOURS; ++k) {
        float4 out = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
        if (k < cnt) {
            const int idj = __float_as_int(EL_NB(k).w);
            const float4 q = ldg_idx(x_home, idj);
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            float gx, gy, gz;
            kernGrad(c, dx, dy, dz, geom(c, dx * dx + dy * dy + dz * dz), gx, gy, gz);
            const double g[3] = {(double)gx, (double)gy, (double)gz};
            out = make_float4((float)(Mi[0] * g[0] + Mi[1] * g[1] + Mi[2] * g[2]), (float)(Mi[3] * g[0] + Mi[4] * g[1] + Mi[5] * g[2]),
                              (float)(Mi[6] * g[0] + Mi[7] * g[1] + Mi[8] * g[2]), __int_as_float(idj));
        }
        EL_NB(k) = out;
    }
#undef EL_NB
}

// g0_ji from the partner's row: plane 1 of entry k = plane 0 of the entry of row j that names i
__global__ void __launch_bounds__(256)
k_elastic_partner(const ElCaptureArgs a) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= a.n) return;
    const size_t n = (size_t)a.n;
    const int id = a.id0 + row;
    for (int k = 0; k < ELASTIC_MAX_NEIGHBOURS; ++k) {
        const int j = __float_as_int(a.rest[(size_t)(2 * k) * n + row].w);
        if (j < 0) break;
        const int rj = j - a.id0;
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool found = false;
        for (int t = 0; t < ELASTIC_MAX_NEIGHBOURS && !found; ++t) {
            const float4 e = a.rest[(size_t)(2 * t) * n + rj];
            const int back = __float_as_int(e.w);
            if (back < 0) break;
            if (back == id) { g = make_float4(e.x, e.y, e.z, 0.0f); found = true; }
        }
        if (!found) atomicAdd(&a.cnt[3], 1u);
        a.rest[(size_t)(2 * k + 1) * n + row] = g;
    }
}

// ---------------------------------------------------------------------------------- launchers
// scatter + pass A + pass B over every captured object; q is double-buffered (pass A reads State::el_q[el_qi] and writes the other)
static void l_elastic(State &s) {
    const int n = s.c.n;
    if (n == 0 || s.el_nobj == 0) return;
    hipLaunchKernelGGL(k_elastic_scatter, dim3(cdiv(n, 256)), dim3(256), 0, s.stream, n, s.cap, s.el_mask, s.meta.cur(), s.pid.cur(),
                       s.posv.cur(), s.el_x_home, s.el_slot_home);
    for (int k = 0; k < s.el_nobj; ++k)
        hipLaunchKernelGGL(k_elastic_rotation, dim3(cdiv(s.el_obj[k].n, 256)), dim3(256), 0, s.stream, s.el_obj[k], s.c.V0, s.el_x_home,
                           s.el_q[s.el_qi], s.el_q[s.el_qi ^ 1], s.el_sig, s.el_F);
    s.el_qi ^= 1;
    for (int k = 0; k < s.el_nobj; ++k)
        hipLaunchKernelGGL(k_elastic_force, dim3(cdiv(s.el_obj[k].n, 256)), dim3(256), 0, s.stream, s.el_obj[k], s.c.V0, s.el_q[s.el_qi],
                           s.el_sig, s.el_slot_home, s.velm.cur(), s.el_acc);
}
static void l_elastic_apply(State &s) {
    const int n = s.c.n;
    if (n == 0 || s.el_nobj == 0) return;
    hipLaunchKernelGGL(k_elastic_apply, dim3(cdiv(n, 256)), dim3(256), 0, s.stream, s.c, s.el_mask, s.meta.cur(), s.el_acc, s.velm.cur(),
                       kept_np_acc(s));
}
// the capture of one object on the cell lists of the sort that has just run (arrays in sorted order, nothing left to a density pass)
static void l_elastic_capture(State &s, const ElCaptureArgs &a) {
    const int n = s.c.n;
    if (n == 0 || a.n == 0) return;
    hipLaunchKernelGGL(k_elastic_scatter, dim3(cdiv(n, 256)), dim3(256), 0, s.stream, n, s.cap, 1u << a.obj, s.meta.cur(), s.pid.cur(),
                       s.posv.cur(), s.el_x_home, s.el_slot_home);
    hipLaunchKernelGGL(k_elastic_capture, dim3(cdiv(a.n, 256)), dim3(256), 0, s.stream, s.c, a, s.cell_start, s.posv.cur(), s.meta.cur(),
                       s.pid.cur(), s.el_x_home, s.el_slot_home, s.el_q[s.el_qi], s.el_sig, s.el_F);
    hipLaunchKernelGGL(k_elastic_partner, dim3(cdiv(a.n, 256)), dim3(256), 0, s.stream, a);
}

static void register_elastic_launchers(Launch &L) {
    L.elastic = l_elastic;
    L.elastic_apply = l_elastic_apply;
    L.elastic_capture = l_elastic_capture;
}

#endif   // SPH_LAUNCH_FN
