// sph_surface_tension.hpp -- Akinci, Akinci, Teschner 2013, "Versatile surface tension and adhesion for SPH fluids" (opt-in:
// sph_set_surface_tension).  h = support radius, rho0 = rest density, j fluid neighbours, k boundary neighbours:
//   n_i      = h  sum_j (m_j / rho_j) gradW(x_i - x_j)                                  SurfaceNormalPass, stored per particle
//   a_coh_i  = -gamma sum_j K_ij m_j C(r_ij) (x_i - x_j) / r_ij,   K_ij = 2 rho0 / (rho_i + rho_j)
//   a_curv_i = -gamma sum_j K_ij (n_i - n_j)
//   a_adh_i  = -beta  sum_k Psi_k A(r_ik) (x_i - x_k) / r_ik,      Psi_k = rho0 V_k       AkinciNonPressurePass
// The two splines are ONE source for the kernels (both builds), the host entry sph_surface_tension_kernels_host (sph_api.hip) and
// through it the CPU tests.  The functors below exist in the kernel translation units only (they need sph_device.hpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ST_HD __host__ __device__ static inline
#else
#define ST_HD static inline
#endif

// constants of the two splines, derived on the host in float64 and rounded once
struct StSpline {
    float h, half_h;      // support radius, h / 2
    float cC;             // 32 / (pi h^9)
    float h6_64;          // h^6 / 64
    float cA;             // 0.007 / h^3.25
    float four_inv_h;     // 4 / h (fast form of A)
};
static inline StSpline st_spline(double h) {
    StSpline k;
    k.h = (float)h; k.half_h = (float)(0.5 * h);
    k.cC = (float)(32.0 / (M_PI * pow(h, 9.0)));
    k.h6_64 = (float)(pow(h, 6.0) / 64.0);
    k.cA = (float)(0.007 / pow(h, 3.25));
    k.four_inv_h = (float)(4.0 / h);
    return k;
}

// Cohesion spline C(r).  The two forms differ in shape only (branches / one select); the arithmetic is the same.  C is continuous at
// r = h / 2, so a comparison that rounding flips there is harmless.  r = 0, r > h and NaN give 0.
template <bool FAST> ST_HD float st_cohesion(const StSpline &k, float r) {
    const float t = k.h - r;
    const float p = ((t * t) * t) * ((r * r) * r);
    if (FAST) {
        const float v = (r + r > k.h) ? p : (p + p) - k.h6_64;
        return (r > 0.0f && r <= k.h) ? k.cC * v : 0.0f;
    }
    if (!(r > 0.0f) || !(r <= k.h)) return 0.0f;
    if (r + r > k.h) return k.cC * p;
    return k.cC * ((p + p) - k.h6_64);
}

// Adhesion spline A(r).  The radicand -4 r^2 / h + 6 r - 2 h = (4 / h) (r - h / 2) (h - r) is exactly 0 at r = h / 2 and r = h --
// one particle diameter and the support radius: where the neighbours of a rest lattice sit.  The strict form evaluates it as written
// and rounding can leave it slightly negative there; both forms clamp it at 0 before the root (a NaN here would reach every fluid
// particle within a few steps).  The fast form takes the factored radicand, whose factors are exact differences near the two zeros.
// A is only Hoelder-1/4 at the zeros: an error eps of the radicand moves A by up to cA eps^(1/4), an ABSOLUTE bound.
template <bool FAST> ST_HD float st_adhesion(const StSpline &k, float r) {
    if (!(r + r > k.h) || !(r <= k.h)) return 0.0f;
    float x;
    if (FAST) x = (k.four_inv_h * (r - k.half_h)) * (k.h - r);
    else x = ((-4.0f * (r * r)) / k.h + 6.0f * r) - 2.0f * k.h;
    x = x > 0.0f ? x : 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    if (FAST) return k.cA * __builtin_amdgcn_sqrtf(__builtin_amdgcn_sqrtf(x));
#endif
    return k.cA * sqrtf(sqrtf(x));
}

#ifdef SPH_LAUNCH_FN   // ------------------------------------------------------------------ kernel translation units only

// n_i = h sum_j (m_j / rho_j) gradW_ij over FLUID neighbours (rho: the density the viscous term of the method reads).  A mask-reusing
// light pass: one 16-byte record per candidate, (x, y, z, m_j / rho_j), zero weight for anything that is not fluid.  Fluid rows only:
// the row of a rigid particle keeps whatever it held (nobody reads it).  Bytes / particle: R posv 16 + velm 16 + rho 4 -> W normal 16.
template <bool AF>
struct SurfaceNormalPass {
    static constexpr bool FLUID_BLOCKS_ONLY = true;   // active for fluid only, passive() empty
    static constexpr int BLOCK = 256, GROUPS = 3;
    static constexpr bool USES_J = false;
    static constexpr bool HAS_B = false, COUNT_PAIRS = true;
    static constexpr int PAIR_WEIGHT = 1;
    static constexpr bool HAS_REDUCE = false;
    typedef int BT;
    struct Own { float nx, ny, nz; };
    const float4 *posv, *velm; const int *meta; const float *rho;
    float4 *normal;

    __device__ float4 stage_impl(int j) const {
        const float4 p = ldg_idx(posv, j);
        float w = fdiv(ldg_idx(velm, j).w, ldg_idx(rho, j));
        if (!AF && META_MAT(meta[j]) != 1) w = 0.0f;
        return make_float4(p.x, p.y, p.z, w);
    }
    __device__ float4 loadA(int j) const { return stage_impl(j); }
    __device__ BT loadB(int) const { return 0; }
    __device__ float4 stage(const Consts &, int j, BT &) const { return stage_impl(j); }
    __device__ bool begin(const Consts &c, int i, const float4 &, Own &o) const {
        o.nx = o.ny = o.nz = 0.0f;
        if (AF && !c.ghosts) return true;
        return META_ACTIVE_FLUID(meta[i]);
    }
    __device__ void pair(const Consts &c, Own &o, float dx, float dy, float dz, float r2, const float4 &a, const BT &, int) const {
        const Geom g = geom(c, r2);
#if SPH_FAST
        const float s = a.w * kernGradScale(c, g);
        o.nx += s * dx; o.ny += s * dy; o.nz += s * dz;
#else
        float gx, gy, gz;
        kernGrad(c, dx, dy, dz, g, gx, gy, gz);
        o.nx += a.w * gx; o.ny += a.w * gy; o.nz += a.w * gz;
#endif
    }
    __device__ float finish(const Consts &c, int i, const float4 &, Own &o) const {
        normal[i] = make_float4(c.h * o.nx, c.h * o.ny, c.h * o.nz, 0.0f);
        return 0.0f;
    }
    __device__ void passive(const Consts &, int, const float4 &) const {}
};

// NonPressurePass (sph_passes.hpp) with cohesion + curvature in the place of the reference's surface-tension term and adhesion, with
// its reaction on dynamic bodies, next to the boundary viscous branch.  Gravity, both viscosity branches, v += dt a, acc_out,
// skip_viscosity and visc_vel are NonPressurePass's.  Per candidate: A = (x, y, z, m_j | rho0 V_k), B = (v_j, rho_j | -1 static /
// -2 - body: dynamic rigid), C = n_j -- 48 B per slot: a heavy pass.
// One accumulator for the three new terms: S = sum_j g2r / (rho_i + rho_j) (m_j C(r) / r (x_i - x_j) + (n_i - n_j))
//                                               + sum_k Psi_k bA(r) / r (x_i - x_k),   a = -S
// with g2r = gamma 2 rho0 and bA = beta A folded into the spline's constant (sp.cA = beta 0.007 / h^3.25).  With beta = 0 the
// adhesion arithmetic does not run: `adhesion` is a kernel argument, one scalar branch.
template <bool AF>
struct AkinciNonPressurePass {
    static constexpr bool HAS_WRENCH = !AF;
    static constexpr int BLOCK = 256, GROUPS = 3;
    static constexpr bool USES_J = !AF;
    static constexpr bool HAS_B = true, COUNT_PAIRS = true, HAS_C = true;
    static constexpr int PAIR_WEIGHT = 2;  // surface tension + viscosity, as NonPressurePass
    static constexpr bool HAS_REDUCE = false;
    typedef float4 BT;
    typedef float4 CT;
    struct Own { float vx, vy, vz, m, rho, nx, ny, nz, sx, sy, sz, ax, ay, az; };
    const float4 *posv, *velm; const int *meta; const float *rho_raw;
    float4 *vel_out; DevScalars *scal; const RigidPose *pose; float rho0;
    int skip_viscosity;
    float4 *acc_out;
    const float4 *visc_vel;
    const float4 *normal;
    StSpline sp;         // (cA carries beta)
    float g2r;           // gamma 2 rho0
    int adhesion;        // beta != 0

    __device__ float4 stage(const Consts &, int j, BT &bj, CT &cj) const {
        const float4 p = ldg_idx(posv, j);
        float4 v = ldg_idx(velm, j);
        if (visc_vel && (AF || META_MAT(meta[j]) == 1)) { const float4 u = visc_vel[j]; v.x = u.x; v.y = u.y; v.z = u.z; }
        cj = ldg_idx(normal, j);
        float aw, bw;
        if (AF) { aw = v.w; bw = ldg_idx(rho_raw, j); }
        else {
            const int m = meta[j];
            const bool fl = META_MAT(m) == 1;
            aw = fl ? v.w : rho0 * p.w;
            bw = fl ? rho_raw[j] : rigid_tag(m);
        }
        bj = make_float4(v.x, v.y, v.z, bw);
        return make_float4(p.x, p.y, p.z, aw);
    }
    __device__ bool begin(const Consts &c, int i, const float4 &, Own &o) const {
        bool ok = true;   // no early return: begin()'s loads go out with the rest of the prologue (k_nbr_pass)
        if (!AF || c.ghosts) ok = META_ACTIVE_FLUID(meta[i]);
        float4 v = velm[i];
        if (visc_vel) { const float4 u = visc_vel[i]; v.x = u.x; v.y = u.y; v.z = u.z; }
        o.vx = v.x; o.vy = v.y; o.vz = v.z; o.m = v.w;
        o.rho = rho_raw[i];
        const float4 n = normal[i];
        o.nx = n.x; o.ny = n.y; o.nz = n.z;
        o.sx = o.sy = o.sz = 0.0f;
        o.ax = o.ay = o.az = 0.0f;
        return ok;
    }
    __device__ void pair(const Consts &c, Own &o, float dx, float dy, float dz, float r2, const float4 &a,
                         const BT &bj, const CT &cj, int) const {
        const Geom g = geom(c, r2);
#if SPH_FAST
        const float rinv = g.rinv;
#else
        const float rinv = g.rn > 0.0f ? 1.0f / g.rn : 0.0f;
#endif
        if (AF || bj.w >= 0.0f) {
            const float kij = fdiv(g2r, o.rho + bj.w);
            const float cr = (a.w * st_cohesion<SPH_FAST != 0>(sp, g.rn)) * rinv;
            o.sx += kij * (cr * dx + (o.nx - cj.x));
            o.sy += kij * (cr * dy + (o.ny - cj.y));
            o.sz += kij * (cr * dz + (o.nz - cj.z));
            if (skip_viscosity) return;
            const float v_xy = (o.vx - bj.x) * dx + (o.vy - bj.y) * dy + (o.vz - bj.z) * dz;
            const float m_ij = (o.m + a.w) * 0.5f;
#if SPH_FAST
            const float k = (fdiv2(c.cv * m_ij, bj.w, r2 + c.visc_eps) * v_xy) * kernGradScale(c, g);
            o.ax += k * dx; o.ay += k * dy; o.az += k * dz;
#else
            float gx, gy, gz;
            kernGrad(c, dx, dy, dz, g, gx, gy, gz);
            const float cc = fdiv2(c.cv * m_ij, bj.w, g.rn * g.rn + c.visc_eps) * v_xy;
            o.ax += cc * gx; o.ay += cc * gy; o.az += cc * gz;
#endif
        } else {
            float fx = 0.0f, fy = 0.0f, fz = 0.0f;   // force on the body, before the factor m_i
            if (adhesion) {   // (uniform)
                const float ar = (a.w * st_adhesion<SPH_FAST != 0>(sp, g.rn)) * rinv;
                fx = ar * dx; fy = ar * dy; fz = ar * dz;
                o.sx += fx; o.sy += fy; o.sz += fz;
            } else if (skip_viscosity) return;
            if (!skip_viscosity) {
                const float v_xy = (o.vx - bj.x) * dx + (o.vy - bj.y) * dy + (o.vz - bj.z) * dz;
#if SPH_FAST
                const float k = (fdiv2(c.cvb * a.w, o.rho, r2 + c.visc_eps) * v_xy) * kernGradScale(c, g);
                const float acx = k * dx, acy = k * dy, acz = k * dz;
#else
                float gx, gy, gz;
                kernGrad(c, dx, dy, dz, g, gx, gy, gz);
                const float cc = fdiv2(c.cvb * a.w, o.rho, g.rn * g.rn + c.visc_eps) * v_xy;
                const float acx = cc * gx, acy = cc * gy, acz = cc * gz;
#endif
                o.ax += acx; o.ay += acy; o.az += acz;
                fx -= fdiv(acx, c.rho0); fy -= fdiv(acy, c.rho0); fz -= fdiv(acz, c.rho0);
            }
            if (bj.w <= -2.0f) {  // dynamic rigid neighbour: both reactions act at x_k, arm x_k - com (base_solver.py:272-278)
                const int obj = (int)(-bj.w) - 2;
                fx *= o.m; fy *= o.m; fz *= o.m;
                add_wrench_at(scal, obj, a.x, a.y, a.z, fx, fy, fz);
            }
        }
    }
    __device__ float finish(const Consts &c, int i, const float4 &, Own &o) const {
        float ax = c.gx, ay = c.gy, az = c.gz;
        ax -= o.sx; ay -= o.sy; az -= o.sz;
        ax += fdiv(o.ax, c.rho0); ay += fdiv(o.ay, c.rho0); az += fdiv(o.az, c.rho0);
        if (acc_out) acc_out[i] = make_float4(ax, ay, az, 0.0f);
        float vx = o.vx, vy = o.vy, vz = o.vz;
        if (visc_vel) { const float4 v = velm[i]; vx = v.x; vy = v.y; vz = v.z; }
        vel_out[i] = make_float4(vx + c.dt * ax, vy + c.dt * ay, vz + c.dt * az, o.m);
        return 0.0f;
    }
    __device__ void passive(const Consts &, int i, const float4 &) const { vel_out[i] = velm[i]; }
};

#endif   // SPH_LAUNCH_FN
