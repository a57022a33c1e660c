// sph_micropolar.hpp -- Bender, Koschier, Kugelstadt, Weiler 2017, "A micropolar material model for turbulent SPH fluids" (opt-in:
// sph_set_micropolar).  Every fluid particle carries an angular velocity w_i.  With R = x_i - x, gradW = gradW(R), j the
// fluid and k the boundary neighbours of an active fluid particle i, Psi_k = rho0 V_k, rho the density the method's viscous term reads:
//   a_mp_i  = nu_t / rho_i [ sum_j m_j (w_i - w_j) x gradW_ij + sum_k Psi_k w_i x gradW_ik ]
//   alpha_i = theta_inv { nu_t / rho_i [ sum_j m_j (v_i - v_j) x gradW_ij + sum_k Psi_k (v_i - v_k) x gradW_ik ]
//                         - 2 nu_t w_i - zeta sum_j (m_j / rho_j) (w_i - w_j) W_ij }
//   w_i <- w_i + dt alpha_i (Jacobi: every sum reads the w of the previous step);   v_i <- v_i + dt a_mp_i is k_micropolar_apply's
//   dynamic body of k:  force -m_i nu_t / rho_i Psi_k w_i x gradW_ik at x_k
// The pair arithmetic is ONE source for the kernels (both builds), the host entry sph_micropolar_pair_host (sph_api.hip) and through it
// the CPU tests.  The functor and the two elementwise kernels exist in the kernel translation units only (they need sph_device.hpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MP_HD __host__ __device__ static inline
#else
#define MP_HD static inline
#endif

// the two sums of a particle: A = sum m (w_i - w_j) x gradW (a_mp = nu_t / rho_i A), B = the braces of alpha without -2 nu_t w_i
struct MpSums { float ax, ay, az, bx, by, bz; };

// One neighbour's share of both sums.  A boundary neighbour is the same arithmetic with w_j = 0 and vol_j = 0 (x - 0 is exact and the
// dissipation term becomes -0 w_i): m_j = Psi_k, v_j = v_k.  c1 = nu_t / rho_i, vol_j = m_j / rho_j.  (cx, cy, cz): this pair's share of A,
// for the reaction on a dynamic body.
//   strict form: the gradient as a vector (gx, gy, gz), every term as written;
//   fast form:   gradW = gs (dx, dy, dz): the cross products are taken with R and the scalars m_j gs, c1 m_j gs applied once.
template <bool FAST>
MP_HD void mp_pair(MpSums &s, float vix, float viy, float viz, float wix, float wiy, float wiz, float c1, float mj, float vjx, float vjy,
                   float vjz, float wjx, float wjy, float wjz, float volj, float zeta, float dx, float dy, float dz, float gs, float gx,
                   float gy, float gz, float W, float &cx, float &cy, float &cz) {
    const float dwx = wix - wjx, dwy = wiy - wjy, dwz = wiz - wjz;
    const float dvx = vix - vjx, dvy = viy - vjy, dvz = viz - vjz;
    const float zw = (zeta * volj) * W;
    if (FAST) {
        const float k = mj * gs, kb = c1 * k;
        cx = k * (dwy * dz - dwz * dy); cy = k * (dwz * dx - dwx * dz); cz = k * (dwx * dy - dwy * dx);
        s.bx += kb * (dvy * dz - dvz * dy) - zw * dwx;
        s.by += kb * (dvz * dx - dvx * dz) - zw * dwy;
        s.bz += kb * (dvx * dy - dvy * dx) - zw * dwz;
    } else {
        const float kb = c1 * mj;
        cx = mj * (dwy * gz - dwz * gy); cy = mj * (dwz * gx - dwx * gz); cz = mj * (dwx * gy - dwy * gx);
        s.bx += kb * (dvy * gz - dvz * gy) - zw * dwx;
        s.by += kb * (dvz * gx - dvx * gz) - zw * dwy;
        s.bz += kb * (dvx * gy - dvy * gx) - zw * dwz;
    }
    s.ax += cx; s.ay += cy; s.az += cz;
}

// behind the sums: a_mp = c1 A;  w_new = w + dt theta_inv (B - 2 nu_t w)
MP_HD void mp_finish(const MpSums &s, float c1, float nu_t, float theta_inv, float dt, float wix, float wiy, float wiz, float *a_mp,
                     float *w_new) {
    a_mp[0] = c1 * s.ax; a_mp[1] = c1 * s.ay; a_mp[2] = c1 * s.az;
    const float n2 = 2.0f * nu_t;
    w_new[0] = wix + dt * (theta_inv * (s.bx - n2 * wix));
    w_new[1] = wiy + dt * (theta_inv * (s.by - n2 * wiy));
    w_new[2] = wiz + dt * (theta_inv * (s.bz - n2 * wiz));
}

#ifdef SPH_LAUNCH_FN   // ------------------------------------------------------------------ kernel translation units only

// The angular velocities stay AT HOME, indexed by the persistent particle id (State::mp_w_home; ids = append order, as for
// State::color_home): no sort moves them.  In front of the walk they are gathered into sorted order for the candidates' records; the
// walk stores the new value at home.  No launch reads and writes the same array.
__global__ void __launch_bounds__(256)
k_micropolar_gather(int n, const int *__restrict__ pid, const float4 *__restrict__ home, float4 *__restrict__ sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) sorted[i] = home[pid[i]];
}

// v += dt a_mp behind the non-pressure phase, acc += a_mp where a non-pressure acceleration is kept; active fluid rows only (the walk
// wrote no other row of a_mp)
__global__ void __launch_bounds__(256)
k_micropolar_apply(const Consts c, const int *__restrict__ meta, const float4 *__restrict__ a_mp, float4 *__restrict__ velm,
                   float4 *__restrict__ acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n || !META_ACTIVE_FLUID(meta[i])) return;
    const float4 a = a_mp[i];
    float4 v = velm[i];
    v.x += c.dt * a.x; v.y += c.dt * a.y; v.z += c.dt * a.z;
    velm[i] = v;
    if (acc) { float4 q = acc[i]; q.x += a.x; q.y += a.y; q.z += a.z; acc[i] = q; }
}

// One mask-reusing tiled walk.  Per candidate: A = (x, y, z, m_j | rho0 V_k), B = (v_j, rho_j | -1 static / -2 - body: dynamic rigid),
// C = (w_j, m_j / rho_j | 0 for a boundary particle) -- 48 B per slot: a heavy pass with the Akinci pass's tile (728 slots).
// Writes a_mp[i] (sorted order) and w_home[pid[i]], fluid rows only; reads the gathered copy of w.
// Bytes / particle: R posv 16 + velm 16 + rho 4 + w_sorted 16 + pid 4 -> W a_mp 16 + w_home 16.
template <bool AF>
struct MicropolarPass {
    static constexpr bool FLUID_BLOCKS_ONLY = true;   // active for fluid only, passive() empty
    static constexpr bool HAS_WRENCH = !AF;
    static constexpr int BLOCK = 256, GROUPS = 3;
    static constexpr bool USES_J = !AF;
    static constexpr bool HAS_B = true, COUNT_PAIRS = true, HAS_C = true;
    static constexpr int PAIR_WEIGHT = 1;
    static constexpr bool HAS_REDUCE = false;
    typedef float4 BT;
    typedef float4 CT;
    struct Own { float vx, vy, vz, wx, wy, wz, c1, m; MpSums s; };
    const float4 *posv, *velm; const int *meta; const float *rho;
    const float4 *w_sorted; const int *pid;
    float4 *a_mp, *w_home; DevScalars *scal; const RigidPose *pose; float rho0;
    float nu_t, zeta, theta_inv;

    __device__ float4 stage(const Consts &, int j, BT &bj, CT &cj) const {
        const float4 p = ldg_idx(posv, j);
        const float4 v = ldg_idx(velm, j);
        const float4 w = ldg_idx(w_sorted, j);
        if (AF) {
            const float r = ldg_idx(rho, j);
            bj = make_float4(v.x, v.y, v.z, r);
            cj = make_float4(w.x, w.y, w.z, fdiv(v.w, r));
            return make_float4(p.x, p.y, p.z, v.w);
        }
        const int m = meta[j];
        const bool fl = META_MAT(m) == 1;
        const float r = rho[j];
        bj = make_float4(v.x, v.y, v.z, fl ? r : rigid_tag(m));
        cj = fl ? make_float4(w.x, w.y, w.z, fdiv(v.w, r)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return make_float4(p.x, p.y, p.z, fl ? v.w : rho0 * p.w);
    }
    __device__ bool begin(const Consts &c, int i, const float4 &, Own &o) const {
        bool ok = true;   // no early return: begin()'s loads go out with the rest of the prologue (k_nbr_pass)
        if (!AF || c.ghosts) ok = META_ACTIVE_FLUID(meta[i]);
        const float4 v = velm[i], w = w_sorted[i];
        o.vx = v.x; o.vy = v.y; o.vz = v.z; o.m = v.w;
        o.wx = w.x; o.wy = w.y; o.wz = w.z;
        o.c1 = fdiv(nu_t, rho[i]);
        o.s.ax = o.s.ay = o.s.az = 0.0f;
        o.s.bx = o.s.by = o.s.bz = 0.0f;
        return ok;
    }
    __device__ void pair(const Consts &c, Own &o, float dx, float dy, float dz, float r2, const float4 &a,
                         const BT &bj, const CT &cj, int) const {
        const Geom g = geom(c, r2);
        float cx, cy, cz;
#if SPH_FAST
        mp_pair<true>(o.s, o.vx, o.vy, o.vz, o.wx, o.wy, o.wz, o.c1, a.w, bj.x, bj.y, bj.z, cj.x, cj.y, cj.z, cj.w, zeta, dx, dy, dz,
                      kernGradScale(c, g), 0.0f, 0.0f, 0.0f, kernW(c, g), cx, cy, cz);
#else
        float gx, gy, gz;
        kernGrad(c, dx, dy, dz, g, gx, gy, gz);
        mp_pair<false>(o.s, o.vx, o.vy, o.vz, o.wx, o.wy, o.wz, o.c1, a.w, bj.x, bj.y, bj.z, cj.x, cj.y, cj.z, cj.w, zeta, dx, dy, dz,
                       0.0f, gx, gy, gz, kernW(c, g), cx, cy, cz);
#endif
        if (!AF && bj.w <= -2.0f) {   // dynamic rigid neighbour: the reaction acts at x_k, arm x_k - com (the viscous wrench's convention)
            const int obj = (int)(-bj.w) - 2;
            const float f = -(o.m * o.c1);
            add_wrench_at(scal, obj, a.x, a.y, a.z, f * cx, f * cy, f * cz);
        }
    }
    __device__ float finish(const Consts &c, int i, const float4 &, Own &o) const {
        float am[3], wn[3];
        mp_finish(o.s, o.c1, nu_t, theta_inv, c.dt, o.wx, o.wy, o.wz, am, wn);
        a_mp[i] = make_float4(am[0], am[1], am[2], 0.0f);
        w_home[pid[i]] = make_float4(wn[0], wn[1], wn[2], 0.0f);
        return 0.0f;
    }
    __device__ void passive(const Consts &, int, const float4 &) const {}
};

#endif   // SPH_LAUNCH_FN
