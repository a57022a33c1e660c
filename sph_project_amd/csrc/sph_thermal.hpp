// sph_thermal.hpp -- heat: a temperature per fluid particle, conduction after Cleary and Monaghan 1999 ("Conduction modelling using
// smoothed particle hydrodynamics") with constant conductivity, and Boussinesq buoyancy (opt-in: sph_set_thermal).
// With R = x_i - x, gradW = gradW(R), F = (R . gradW) / (|R|^2 + 0.01 h^2) (never positive; the 0.01 h^2 is the viscous term's), j the
// fluid and k the boundary neighbours of an active fluid particle i, rho the density the method's viscous term reads:
//   dT_i/dt = 2 alpha (rho0 / rho_i) [ sum_j (m_j / rho_j) (T_i - T_j) F_ij + sum_k c_k (T_i - T_k) F_ik ]
//             c_k = V_k where k's object is held at a temperature T_k (Dirichlet), 0 otherwise (adiabatic: the term is exactly 0)
//   T_i <- T_i + dt dT_i/dt   (Jacobi: every sum reads the T of the previous step)
//   a_b_i = -beta (T_i - T_ref) g   (T_i: the previous step's), v_i <- v_i + dt a_b_i is k_heat_apply's
// Heat never reaches a body: no reaction, no wrench.  The pair arithmetic, the finish and the buoyancy are ONE source for the kernels
// (both builds), the host entries sph_heat_pair_host / sph_heat_finish_host (sph_api.hip), tools/check_thermal.cpp and through the host
// entries the CPU tests.  The functor and the elementwise kernels exist in the kernel translation units only (they need sph_device.hpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define HT_HD __host__ __device__ static inline
#else
#define HT_HD static inline
#endif

// entry of the per-object table for "no temperature": an adiabatic body (any finite temperature is below it)
#define HT_ADIABATIC 3.0e38f

// what the kernels read: every constant rounded once from double
struct HeatConsts { float k2a, kb, t_ref; };   // 2 alpha, -beta, T_ref
static inline HeatConsts heat_consts(double alpha, double beta, double t_ref) {
    HeatConsts k;
    k.k2a = (float)(2.0 * alpha); k.kb = (float)(-beta); k.t_ref = (float)t_ref;
    return k;
}

template <bool FAST> HT_HD float ht_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (FAST) return a * __builtin_amdgcn_rcpf(b);
#endif
    return a / b;
}

// One neighbour's term of the bracket: c_j (T_i - T_j) F_ij.  A boundary neighbour is the same arithmetic with c_j = V_k | 0 and
// T_j = T_k | 0: no branch.  eps = 0.01 h^2.
//   strict form: F from the gradient as a vector (gx, gy, gz): (dx gx + dy gy + dz gz) / (r2 + eps);
//   fast form:   gradW = gs (dx, dy, dz), so R . gradW = gs r2; the quotient through one reciprocal (v_rcp_f32 on the device).
template <bool FAST>
HT_HD float heat_pair(float Ti, float cj, float Tj, float dx, float dy, float dz, float r2, float eps, float gs, float gx, float gy,
                      float gz) {
    const float num = FAST ? gs * r2 : (dx * gx + dy * gy) + dz * gz;
    const float F = ht_div<FAST>(num, r2 + eps);
    return (cj * (Ti - Tj)) * F;
}

// behind the sum: dT/dt = 2 alpha (rho0 / rho_i) sum;  T_new = T + dt dT/dt
template <bool FAST>
HT_HD void heat_finish(float sum, float k2a, float rho0, float rho_i, float dt, float Ti, float *rate, float *T_new) {
    const float r = (k2a * ht_div<FAST>(rho0, rho_i)) * sum;
    *rate = r;
    *T_new = Ti + dt * r;
}

// a_b = -beta (T - T_ref) g
HT_HD void heat_buoyancy(float kb, float T, float t_ref, float gx, float gy, float gz, float *a) {
    const float f = kb * (T - t_ref);
    a[0] = f * gx; a[1] = f * gy; a[2] = f * gz;
}

#ifdef SPH_LAUNCH_FN   // ------------------------------------------------------------------ kernel translation units only

// The temperatures stay AT HOME, indexed by the persistent particle id (State::heat_T_home; ids = append order, as State::mp_w_home):
// no sort moves them.  Rows of new particles (an append, a late object, an emitter's newborn layer): the host knows first id and count.
__global__ void __launch_bounds__(256)
k_heat_fill(float *__restrict__ home, int first_id, int count, float T) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < count) home[first_id + k] = T;
}

// in front of the walk: T in sorted order for the candidates' records and for the buoyancy (no launch reads and writes the same array)
__global__ void __launch_bounds__(256)
k_heat_gather(int n, const int *__restrict__ pid, const float *__restrict__ home, float *__restrict__ sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) sorted[i] = home[pid[i]];
}

// v += dt a_b behind the non-pressure phase, acc += a_b where a non-pressure acceleration is kept; active fluid rows only.  Reads the
// gathered T: the temperatures the walk of this step read, not the ones it stored.
__global__ void __launch_bounds__(256)
k_heat_apply(const Consts c, const int *__restrict__ meta, const float *__restrict__ T_sorted, const HeatConsts k,
             float4 *__restrict__ velm, float4 *__restrict__ acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n || !META_ACTIVE_FLUID(meta[i])) return;
    float a[3];
    heat_buoyancy(k.kb, T_sorted[i], k.t_ref, c.gx, c.gy, c.gz, a);
    float4 v = velm[i];
    v.x += c.dt * a[0]; v.y += c.dt * a[1]; v.z += c.dt * a[2];
    velm[i] = v;
    if (acc) { float4 q = acc[i]; q.x += a[0]; q.y += a[1]; q.z += a[2]; acc[i] = q; }
}

// One mask-reusing tiled walk over fluid tiles.  Per candidate: A = (x, y, z, c_j), c_j = m_j / rho_j for a fluid candidate, V_k or 0
// for a boundary one (the per-object table, indexed by the low byte of the meta word: object id + 1); B = T_j, one float -- 20 B per
// slot: a medium record in the fast build (5 workgroups per CU).  One accumulator.  Writes T_home[pid[i]] and rate[i] = dT/dt (sorted
// order, valid until the next sort), active fluid rows only; reads the gathered copy of T.
// Bytes / particle: R posv 16 + velm 16 + rho 4 + T_sorted 4 + pid 4 -> W T_home 4 + rate 4 (the gather: R pid 4 + T_home 4 -> W 4).
template <bool AF>
struct HeatPass {
    static constexpr bool FLUID_BLOCKS_ONLY = true;   // active for fluid only, passive() empty
    static constexpr int BLOCK = 256, GROUPS = 3;
    static constexpr bool USES_J = false;
    static constexpr bool HAS_B = true, COUNT_PAIRS = true;
    static constexpr int PAIR_WEIGHT = 1;
    static constexpr bool HAS_REDUCE = false;
    typedef float BT;
    struct Own { float T, sum; };
    const float4 *posv, *velm; const int *meta; const float *rho;
    const float *T_sorted; const int *pid; const float *obj_T;
    float *T_home, *rate;
    HeatConsts k;

    __device__ float4 stage_impl(int j, BT &bj) const {
        const float4 p = ldg_idx(posv, j);
        const float m = ldg_idx(velm, j).w;
        const float r = ldg_idx(rho, j);
        const float t = ldg_idx(T_sorted, j);
        if (AF) { bj = t; return make_float4(p.x, p.y, p.z, fdiv(m, r)); }
        const int mm = meta[j];
        const bool fl = META_MAT(mm) == 1;
        const float tw = obj_T[mm & 0xff];
        const bool wall = tw < HT_ADIABATIC;
        bj = fl ? t : (wall ? tw : 0.0f);
        return make_float4(p.x, p.y, p.z, fl ? fdiv(m, r) : (wall ? p.w : 0.0f));
    }
    __device__ float4 loadA(int j) const { BT b; return stage_impl(j, b); }
    __device__ BT loadB(int j) const { BT b; stage_impl(j, b); return b; }
    __device__ float4 stage(const Consts &, int j, BT &bj) const { return stage_impl(j, bj); }
    __device__ bool begin(const Consts &c, int i, const float4 &, Own &o) const {
        bool ok = true;   // no early return: begin()'s loads go out with the rest of the prologue (k_nbr_pass)
        if (!AF || c.ghosts) ok = META_ACTIVE_FLUID(meta[i]);
        o.T = T_sorted[i];
        o.sum = 0.0f;
        return ok;
    }
    __device__ void pair(const Consts &c, Own &o, float dx, float dy, float dz, float r2, const float4 &a, const BT &bj, int) const {
        const Geom g = geom(c, r2);
#if SPH_FAST
        o.sum += heat_pair<true>(o.T, a.w, bj, dx, dy, dz, r2, c.visc_eps, kernGradScale(c, g), 0.0f, 0.0f, 0.0f);
#else
        float gx, gy, gz;
        kernGrad(c, dx, dy, dz, g, gx, gy, gz);
        o.sum += heat_pair<false>(o.T, a.w, bj, dx, dy, dz, r2, c.visc_eps, 0.0f, gx, gy, gz);
#endif
    }
    __device__ float finish(const Consts &c, int i, const float4 &, Own &o) const {
        float r, tn;
        heat_finish<SPH_FAST != 0>(o.sum, k.k2a, c.rho0, rho[i], c.dt, o.T, &r, &tn);
        T_home[pid[i]] = tn;
        rate[i] = r;
        return 0.0f;
    }
    __device__ void passive(const Consts &, int, const float4 &) const {}
};

#endif   // SPH_LAUNCH_FN
