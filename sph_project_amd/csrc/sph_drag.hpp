// sph_drag.hpp -- Gissler, Band, Peer, Ihmsen, Teschner 2017, "Approximate air-fluid interactions for SPH" (opt-in: sph_set_drag;
// DESIGN.md 36).  The air is not simulated: a constant wind u acts on every active fluid particle i through a drag force whose
// coefficient and cross section depend on how deformed the droplet it stands for is (y), on how many fluid neighbours it has (n_i)
// and on how far the neighbour that shields it most hides it from the relative wind (q).  With d = 2 r, rho_l = density0 and the
// constants of DragHost below, j over the fluid neighbours of i (r_ij < h, self excluded; rigid particles neither count nor shield):
//   v_rel = u - v_i;  s2 = |v_rel|^2;  s2 < 1e-6: a_drag_i = 0 and every term 0
//   s = sqrt(s2);  e = v_rel / s;  y = min(s2 y_coeff, 1);  Re = 2 max(rho_a s L / mu_a, 0.1)
//   C_sph = Re <= 1000 ? 24 / Re (1 + Re^(2/3) / 6) : 0.424;  C_liu = C_sph (1 + 2.632 y)
//   f = min(n23, n_i) / n23;  C_D = (1 - f) C_liu + f;  A_drop = pi (L + C_b L y)^2;  A_un = (1 - f) A_drop + f d^2
//   q = max_j e . (x_i - x_j) / |x_i - x_j| (0 without a neighbour, never below 0);  w = clamp(1 - q, 0, 1)
//   a_drag_i = k / (2 m_i) rho_a s v_rel C_D w A_un
// DragPass stores a_drag and the terms; k_drag_apply adds v += dt a_drag behind the non-pressure phase.  No reaction on anything.
// The per-particle arithmetic (drag_dir, drag_finish) is ONE source for the kernels (both builds), the host entry
// sph_drag_particle_host (sph_api.hip), tools/check_drag.cpp and through the host entry the CPU tests; it is evaluated without
// contraction everywhere, so the two builds differ in it only by v_rcp_f32 / v_rsq_f32 on the device and by the written forms below.
// The functor and the elementwise kernel exist in the kernel translation units only (they need sph_device.hpp).
#pragma once
#include <math.h>
#include <string.h>

#if defined(__HIPCC__)
#define DR_HD __host__ __device__ static inline
#else
#define DR_HD static inline
#endif
#if defined(__clang__)
#define DR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DR_NO_CONTRACT   /* (build with -ffp-contract=off) */
#endif

// water in air
#define DR_SIGMA 0.0724
#define DR_MU_L 0.00102
#define DR_MU_A 1.845e-5
#define DR_C_F (1.0 / 3.0)
#define DR_C_K 8.0
#define DR_C_D 5.0
#define DR_C_B 0.5
#define DR_N_FULL 38.0
#define DR_S2_MIN 1e-6f              // below this |v_rel|^2 there is no drag at all
#define DR_W_FLUSH 9.5367431640625e-7f   // 2^-20: a w below it is 0 (q carries up to 16 units of roundoff: a fully shielded particle feels NO force)

// the constants of one handle, in double on the host
struct DragHost { double L, inv_td, omega2, t_max, c_def, y_coeff, n23, re_coeff; };
// false: omega^2 <= 0 (the droplet's oscillation is overdamped at this radius and density: the deformation model does not apply)
static inline bool drag_host_constants(double radius, double rho_l, double rho_a, DragHost &k) {
    const double d = 2.0 * radius;
    k.L = cbrt(3.0 / (4.0 * M_PI)) * d;
    k.inv_td = DR_C_D * DR_MU_L / (2.0 * rho_l * k.L * k.L);
    k.omega2 = DR_C_K * DR_SIGMA / (rho_l * k.L * k.L * k.L) - k.inv_td * k.inv_td;
    k.n23 = 2.0 * DR_N_FULL / 3.0;
    k.re_coeff = rho_a * k.L / DR_MU_A;
    k.t_max = k.c_def = k.y_coeff = 0.0;
    if (!(k.omega2 > 0.0) || !isfinite(k.omega2)) return false;
    const double omega = sqrt(k.omega2), td = 1.0 / k.inv_td;
    k.t_max = -2.0 * (atan(sqrt(td * td * k.omega2)) - M_PI) / omega;
    k.c_def = 1.0 - exp(-k.t_max / td) * (cos(omega * k.t_max) + sin(omega * k.t_max) / (omega * td));
    k.y_coeff = DR_C_F * (rho_a * k.L / DR_SIGMA) * k.c_def / (DR_C_K * DR_C_B);
    return true;
}

// what the kernels read: every constant rounded once from double; the wind in the library's frame
struct DragConsts {
    float ux, uy, uz;
    float y_coeff, re_coeff;     // y = s2 y_coeff;  Re / 2 = re_coeff s
    float L, cbL, d2;            // L, C_b L, d^2
    float n23, inv_n23;
    float half_k_rho;            // k rho_a / 2
};
static inline DragConsts drag_consts(const DragHost &h, double radius, double rho_a, double k, const double *u_lib) {
    DragConsts c;
    c.ux = (float)u_lib[0]; c.uy = (float)u_lib[1]; c.uz = (float)u_lib[2];
    c.y_coeff = (float)h.y_coeff; c.re_coeff = (float)h.re_coeff;
    c.L = (float)h.L; c.cbL = (float)(DR_C_B * h.L); c.d2 = (float)(4.0 * radius * radius);
    c.n23 = (float)h.n23; c.inv_n23 = (float)(1.0 / h.n23);
    c.half_k_rho = (float)(0.5 * k * rho_a);
    return c;
}

template <bool FAST> DR_HD float dr_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (FAST) return a * __builtin_amdgcn_rcpf(b);
#endif
    return a / b;
}

// x^(1/3) for a normal x > 0 in plain float arithmetic: the classic bit seed (exponent / 3, within 3.5 % of the root) and two Halley
// steps t <- t (t^3 + 2 x) / (2 t^3 + x), which cube the relative error: 3.5e-2 -> 2.9e-5 -> 1.6e-14.  What is left is the roundoff of
// the last step: t^3 two roundings, entering the quotient with weights 1/3 and 2/3 (2 u), two sums, the division and the product (4 u):
// |dr_cbrt(x) / cbrt(x) - 1| <= 7 u, u = 2^-24.  The same bits on the host and in both device builds.
DR_HD float dr_cbrt(float x) {
    DR_NO_CONTRACT
    unsigned i;
    __builtin_memcpy(&i, &x, 4);
    i = i / 3u + 0x2a5137a0u;
    float t;
    __builtin_memcpy(&t, &i, 4);
    for (int it = 0; it < 2; ++it) {
        const float t3 = (t * t) * t;
        t = t * ((t3 + (x + x)) / ((t3 + t3) + x));
    }
    return t;
}

// e = v_rel / |v_rel|, or 0 below the threshold (then no neighbour shields: q stays 0)
template <bool FAST>
DR_HD void drag_dir(const DragConsts &k, float vx, float vy, float vz, float &ex, float &ey, float &ez) {
    DR_NO_CONTRACT
    const float rx = k.ux - vx, ry = k.uy - vy, rz = k.uz - vz;
    const float s2 = (rx * rx + ry * ry) + rz * rz;
    ex = ey = ez = 0.0f;
    if (!(s2 >= DR_S2_MIN)) return;
    if (FAST) {
#if defined(__HIP_DEVICE_COMPILE__)
        const float si = __builtin_amdgcn_rsqf(s2);
#else
        const float si = 1.0f / sqrtf(s2);
#endif
        ex = rx * si; ey = ry * si; ez = rz * si;
    } else {
        const float s = sqrtf(s2);
        ex = rx / s; ey = ry / s; ez = rz / s;
    }
}

struct DragOut { float ax, ay, az, w, cd, a_un, y; };

// Everything behind the walk's two results: n = the number of fluid neighbours, q = the largest e . (x_i - x_j) / |x_i - x_j| (>= 0).
//   strict form: every quotient a division, as written above;
//   fast form:   f = n inv_n23, 24 / Re and the final 1 / m_i through one reciprocal each (v_rcp_f32 on the device).
template <bool FAST>
DR_HD void drag_finish(const DragConsts &k, float vx, float vy, float vz, float m, float n, float q, DragOut &o) {
    DR_NO_CONTRACT
    o.ax = o.ay = o.az = o.w = o.cd = o.a_un = o.y = 0.0f;
    const float rx = k.ux - vx, ry = k.uy - vy, rz = k.uz - vz;
    const float s2 = (rx * rx + ry * ry) + rz * rz;
    if (!(s2 >= DR_S2_MIN)) return;
    const float s = sqrtf(s2);
    const float y = fminf(s2 * k.y_coeff, 1.0f);
    const float re = 2.0f * fmaxf(k.re_coeff * s, 0.1f);
    float c_sph = 0.424f;
    if (re <= 1000.0f) {
        const float c = dr_cbrt(re);
        const float r23 = c * c;
        const float lead = FAST ? 24.0f * dr_div<true>(1.0f, re) : 24.0f / re;
        c_sph = lead * (1.0f + r23 / 6.0f);
    }
    const float c_liu = c_sph * (1.0f + 2.632f * y);
    // (n >= n23 gives exactly 1, whatever the form: 1 - f is then exactly 0)
    const float f = n >= k.n23 ? 1.0f : (FAST ? n * k.inv_n23 : n / k.n23);
    const float g = 1.0f - f;
    const float cd = g * c_liu + f;
    const float rad = k.L + k.cbL * y;
    const float a_drop = 3.14159265358979323846f * (rad * rad);
    const float a_un = g * a_drop + f * k.d2;
    float w = 1.0f - q;
    w = w < DR_W_FLUSH ? 0.0f : (w > 1.0f ? 1.0f : w);
    const float num = (k.half_k_rho * s) * ((cd * w) * a_un);
    const float c = FAST ? num * dr_div<true>(1.0f, m) : num / m;
    o.ax = c * rx; o.ay = c * ry; o.az = c * rz;
    o.w = w; o.cd = cd; o.a_un = a_un; o.y = y;
}

#ifdef SPH_LAUNCH_FN   // ------------------------------------------------------------------ kernel translation units only

// v += dt a_drag behind the non-pressure phase, acc += a_drag where a non-pressure acceleration is kept; active fluid rows only (the
// walk wrote no other row of dr_acc)
__global__ void __launch_bounds__(256)
k_drag_apply(const Consts c, const int *__restrict__ meta, const float4 *__restrict__ a_drag, float4 *__restrict__ velm,
             float4 *__restrict__ acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n || !META_ACTIVE_FLUID(meta[i])) return;
    const float4 a = a_drag[i];
    float4 v = velm[i];
    v.x += c.dt * a.x; v.y += c.dt * a.y; v.z += c.dt * a.z;
    velm[i] = v;
    if (acc) { float4 q = acc[i]; q.x += a.x; q.y += a.y; q.z += a.z; acc[i] = q; }
}

// One mask-reusing light walk: one 16-byte record per candidate, (x, y, z, 1 fluid | 0 anything else), no B or C record.  Per pair one
// reciprocal square root and one dot product; the count is kept as a float (exact far beyond any neighbour count).  Writes two float4
// per active fluid row, in sorted order: acc = (a_drag, n_i), terms = (w, C_D, A_un, y); the row of a rigid particle keeps whatever
// it held.  Bytes / particle: R posv 16 + velm 16 -> W acc 16 + terms 16.
template <bool AF>
struct DragPass {
    static constexpr bool FLUID_BLOCKS_ONLY = true;   // active for fluid only, passive() empty
    static constexpr int BLOCK = 256, GROUPS = 3;
    static constexpr bool USES_J = false;
    static constexpr bool HAS_B = false, COUNT_PAIRS = true;
    static constexpr int PAIR_WEIGHT = 1;
    static constexpr bool HAS_REDUCE = false;
    typedef int BT;
    struct Own { float ex, ey, ez, n, q; };
    const float4 *posv, *velm; const int *meta;
    float4 *acc, *terms;
    DragConsts k;

    __device__ float4 stage_impl(int j) const {
        const float4 p = ldg_idx(posv, j);
        float fl = 1.0f;
        if (!AF && META_MAT(meta[j]) != 1) fl = 0.0f;
        return make_float4(p.x, p.y, p.z, fl);
    }
    __device__ float4 loadA(int j) const { return stage_impl(j); }
    __device__ BT loadB(int) const { return 0; }
    __device__ float4 stage(const Consts &, int j, BT &) const { return stage_impl(j); }
    __device__ bool begin(const Consts &c, int i, const float4 &, Own &o) const {
        bool ok = true;   // no early return: begin()'s loads go out with the rest of the prologue (k_nbr_pass)
        if (!AF || c.ghosts) ok = META_ACTIVE_FLUID(meta[i]);
        const float4 v = velm[i];
        drag_dir<SPH_FAST != 0>(k, v.x, v.y, v.z, o.ex, o.ey, o.ez);
        o.n = 0.0f; o.q = 0.0f;
        return ok;
    }
    __device__ void pair(const Consts &, Own &o, float dx, float dy, float dz, float r2, const float4 &a, const BT &, int) const {
#pragma clang fp contract(off)
        if (!AF && a.w == 0.0f) return;
        o.n += 1.0f;
        const float dot = (o.ex * dx + o.ey * dy) + o.ez * dz;
#if SPH_FAST
        const float qq = dot * __builtin_amdgcn_rsqf(fmaxf(r2, 1e-30f));
#else
        const float qq = r2 > 0.0f ? dot / __builtin_sqrtf(r2) : 0.0f;
#endif
        o.q = fmaxf(o.q, qq);
    }
    __device__ float finish(const Consts &, int i, const float4 &, Own &o) const {
        const float4 v = velm[i];
        DragOut r;
        drag_finish<SPH_FAST != 0>(k, v.x, v.y, v.z, v.w, o.n, o.q, r);
        acc[i] = make_float4(r.ax, r.ay, r.az, o.n);
        terms[i] = make_float4(r.w, r.cd, r.a_un, r.y);
        return 0.0f;
    }
    __device__ void passive(const Consts &, int, const float4 &) const {}
};

#endif   // SPH_LAUNCH_FN
