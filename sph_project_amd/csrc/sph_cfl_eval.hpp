// sph_cfl_eval.hpp -- adaptive time stepping (SphCflParams, include/sph_hip.h): the rule that turns the largest particle
// speed into the next step size, and the per-particle part of the reduce -- which particles count and how a speed is squared.  ONE source
// for the reduce kernel (sph_cfl.hpp), the host side of a step and the host entries sph_cfl_dt_host / sph_cfl_speed2_host
// (sph_cfl_api.hpp), and the stand-alone check (tools/check_cfl.cpp).  The rule is host arithmetic in double: sqrt, /, * and ceil are
// exactly rounded, so a float64 model restates it bit for bit.  The speed is float32 with every product and sum rounded in the order
// written (no contraction in either build).  Needs <math.h>, <stdint.h>, <string.h> and include/sph_hip.h before it.
#pragma once

#if defined(__HIPCC__)
#define CFL_HD __host__ __device__ static inline
#else
#define CFL_HD static inline
#endif
#if defined(__clang__)
#define CFL_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CFL_NO_CONTRACT   /* (build with -ffp-contract=off) */
#endif

// a scene time t counts as t_end when t_end - t <= CFL_REACHED * dt_max
#define CFL_REACHED (1.0 / 1048576.0)   /* 2^-20 */

// does the particle with this meta word take part (the word's layout: sph_common.hpp META_*): active fluid (material 1, no ghost), or a
// rigid particle (material 2) of a dynamic body -- k_renew_rigid stores v + w x r there; never a ghost, never the dead
CFL_HD int cfl_counted(int m) {
    if ((m >> 12) & 1) return 0;                      // dead
    if (((m >> 8) & 0xB) == 1) return 1;              // active fluid
    return (((m >> 8) & 0x3) == 2 && ((m >> 10) & 1) && !((m >> 11) & 1)) ? 1 : 0;
}

// |v|^2 = (vx vx + vy vy) + vz vz, five roundings
// Plain operators under the pragma, on the device as on the host: __fmul_rn / __fadd_rn are plain products and sums inside the HIP
// headers, outside any pragma, and the fast build (-ffp-contract=fast-honor-pragmas) fused them into v_fmac_f32.
CFL_HD float cfl_speed2(float vx, float vy, float vz) {
    CFL_NO_CONTRACT
    const float xx = vx * vx, yy = vy * vy, zz = vz * vz;
    const float s = xx + yy;
    return s + zz;
}

// the bit pattern of a float32; non-negative floats order like these unsigned integers
CFL_HD unsigned cfl_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    unsigned u; memcpy(&u, &f, sizeof(u)); return u;
#endif
}
// inf or NaN (a NaN may carry a sign)
CFL_HD int cfl_nonfinite(unsigned bits) { return (bits & 0x7fffffffu) >= 0x7f800000u ? 1 : 0; }

// the rule (host).  d: the particle diameter; vmax2: the float32 maximum of |v|^2 (finite, >= 0); remaining: t_end - t while a time target is
// set, anything not finite otherwise.  A remaining time within the tolerance counts as reached: no landing.  Returns the step as the
// float32 the kernels take, widened, and SPH_CFL_* flags.
static inline double cfl_rule(const SphCflParams *p, double d, float vmax2, double remaining, int *flags) {
    CFL_NO_CONTRACT
    const double v = sqrt((double)vmax2);
    const double lim = p->factor * 0.4 * d;
    int f = 0;
    double dt;
    if (v * p->max_dt > lim) dt = lim / v;   // (v > 0 here: no division by zero)
    else { dt = p->max_dt; f |= SPH_CFL_CLAMPED_MAX; }
    if (dt < p->min_dt) { dt = p->min_dt; f |= SPH_CFL_CLAMPED_MIN; }
    if (isfinite(remaining) && remaining > CFL_REACHED * p->max_dt) {
        const double n = ceil(remaining / dt);   // >= 1
        dt = remaining / n;                      // never above the CFL step; never below half of it while remaining >= it
        f |= SPH_CFL_LANDING;
    }
    if (flags) *flags = f;
    return (double)(float)dt;
}

// the reduce on the host: the maximum of |v|^2 over the particles that count, non-finite squares left out and reported
static inline void cfl_speed2_max(int64_t n, const float *vel, const int32_t *meta, float *vmax2, int *nonfinite) {
    unsigned best = 0u; int bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!cfl_counted(meta[i])) continue;
        const unsigned b = cfl_bits(cfl_speed2(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]));
        if (cfl_nonfinite(b)) bad = 1; else if (b > best) best = b;
    }
    float out; memcpy(&out, &best, sizeof(out));
    *vmax2 = out; *nonfinite = bad;
}
