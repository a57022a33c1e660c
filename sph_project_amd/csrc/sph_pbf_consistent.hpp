// sph_pbf_consistent.hpp -- the consistent PBF variant (Macklin & Mueller 2013 with the project's cubic spline): pair
// functors for k_nbr_pass, the predict / finish kernels and their launchers; included by sph_kernels.hip inside the per-build namespace.
//
// Access pattern.  posv keeps the positions of the step's sort for the whole step; the predicted positions x* live in a buffer of their
// own (State::pbf_old, with State::pbf_pos as the Jacobi pass's second buffer).  The neighbours of i are the particles j != i with
// |x_i - x_j| < h at the SORTED positions -- the set PcisphRhoStarPass walks, fixed for the step -- so both walks of an iteration are
// tiled passes on the masks the step's density pass stored; kernel values are taken at x* (a rigid neighbour stays at its own position).
#pragma once

// W and grad W of the cubic spline at a predicted offset d = x*_i - x*_j, which may exceed h: both vanish there (the accepted-pair
// forms of the fast build, kernW<true> / kernGradScale, carry no such test).  Fast build: grad W = gs d, the scalar goes into the
// pair's coefficient and the gradient never exists as a vector (see WcsphForcePass::pair); strict build: kernel_gradient as written.
#if SPH_FAST
__device__ __forceinline__ void pbfc_kernel(const Consts &c, float r2, float &w, float &gs) {
    const Geom g = geom(c, r2);
    w = kernW<false>(c, g);
    gs = g.q <= 1.0f ? kernGradScale(c, g) : 0.0f;
}
#endif

// ---------------------------------------------------------------------------------------
// Walk A: density and lambda.  D_i = V_i W(0) + sum_j V_j W(x*_ij) (rho_i = rho0 D_i: m_j = rho0 V_j for fluid, rho0 V_b for rigid),
// G_ij = V_j grad W(x*_ij), C_i = max(D_i - 1, 0), lambda_i = -C_i / (sum |G_ij|^2 + |sum G_ij|^2 + eps).  The reduction leaves the
// partial sums of C.  Staged: x*_j (a rigid neighbour: its position), 12 bytes.
// Bytes / particle: R posv 16 + x* 16 -> W rho 4 + lambda 4.
template <bool AF>
struct PbfcDensityLambdaPass {
    static constexpr bool FLUID_BLOCKS_ONLY = true;   // active for fluid only, passive() empty
    static constexpr int BLOCK = 256, GROUPS = 3;
    static constexpr bool USES_J = !AF;   // pair() looks at j only for rigid neighbours
    static constexpr bool HAS_B = true, COUNT_PAIRS = true, HAS_REDUCE = true;
    static constexpr int PAIR_WEIGHT = 2;   // a density and a lambda pass
    // the all-fluid walk on stored masks needs 97-98 VGPRs in the fast build (eight accumulators under the medium functors' staging
    // batches): one or two over the 96 of five waves per SIMD, so it takes four (128) rather than spill
    static constexpr int MAX_WAVES = (SPH_FAST && AF) ? 4 : 8;
    struct BT { float x, y, z; };
    struct Own { float px, py, pz, sum, gx, gy, gz, s2; };
    const float4 *posv, *xs; const int *meta;
    float *rho, *lambda; float eps; float *red_out;

    __device__ float4 loadA(int j) const { return posv[j]; }
    __device__ float4 stage(const Consts &, int j, BT &bj) const {
        const float4 p = ldg_idx(posv, j);
        float4 q;
        if (!AF && META_MAT(meta[j]) != 1) q = p;
        else q = ldg_idx(xs, j);
        bj.x = q.x; bj.y = q.y; bj.z = q.z;
        return p;
    }
    __device__ bool begin(const Consts &c, int i, const float4 &, Own &o) const {
        bool ok = true;   // no early return: begin()'s loads go out with the rest of the prologue (k_nbr_pass)
        if (!AF || c.ghosts) ok = META_ACTIVE_FLUID(meta[i]);
        const float4 q = xs[i];
        o.px = q.x; o.py = q.y; o.pz = q.z;
        o.sum = o.gx = o.gy = o.gz = o.s2 = 0.0f;
        return ok;
    }
    __device__ void pair(const Consts &c, Own &o, float, float, float, float, const float4 &a, const BT &bj, int) const {
        const float dx = o.px - bj.x, dy = o.py - bj.y, dz = o.pz - bj.z;
        const float r2 = dx * dx + dy * dy + dz * dz;
#if SPH_FAST
        float w, gs;
        pbfc_kernel(c, r2, w, gs);
        o.sum += a.w * w;
        const float k = a.w * gs;   // G_ij = k d, |G_ij|^2 = k^2 r^2
        o.s2 += (k * k) * r2;
        o.gx += k * dx; o.gy += k * dy; o.gz += k * dz;
#else
        const Geom g = geom(c, r2);
        o.sum += a.w * kernW<false>(c, g);
        float gx, gy, gz;
        kernGrad(c, dx, dy, dz, g, gx, gy, gz);
        gx *= a.w; gy *= a.w; gz *= a.w;
        o.s2 += gx * gx + gy * gy + gz * gz;
        o.gx += gx; o.gy += gy; o.gz += gz;
#endif
    }
    __device__ float finish(const Consts &c, int i, const float4 &pi, Own &o) const {
        const float d = pi.w * c.W0 + o.sum;
        rho[i] = d * c.rho0;
        const float cc = fmaxf(d - 1.0f, 0.0f);
        const float den = o.s2 + (o.gx * o.gx + o.gy * o.gy + o.gz * o.gz) + eps;
        lambda[i] = -fdiv(cc, den);
        return cc;
    }
    __device__ void passive(const Consts &, int, const float4 &) const {}
};

// Walk B: the correction, Jacobi.  x*_i += sum_fluid (lambda_i + lambda_j) G_ij + lambda_i sum_rigid G_ib, written to the second x*
// buffer (the launcher swaps).  Staged: (x*_j, lambda_j), 16 bytes; a rigid neighbour: (its position, 0).
// Bytes / particle: R posv 16 + x* 16 + lambda 4 -> W x* 16.
template <bool AF>
struct PbfcDeltaPass {
    static constexpr bool FLUID_BLOCKS_ONLY = true;   // active for fluid only, passive() empty
    static constexpr int BLOCK = 256, GROUPS = 3;
    static constexpr bool USES_J = !AF;   // pair() looks at j only for rigid neighbours
    static constexpr bool HAS_B = true, COUNT_PAIRS = true, HAS_REDUCE = false;
    static constexpr int PAIR_WEIGHT = 1;
    struct BT { float x, y, z, l; };
    struct Own { float px, py, pz, l, ax, ay, az; };
    const float4 *posv, *xs; const int *meta; const float *lambda;
    float4 *xs_out;

    __device__ float4 stage_impl(int j, BT &bj) const {
        const float4 p = ldg_idx(posv, j);
        if (!AF && META_MAT(meta[j]) != 1) { bj.x = p.x; bj.y = p.y; bj.z = p.z; bj.l = 0.0f; return p; }
        const float4 q = ldg_idx(xs, j);
        bj.x = q.x; bj.y = q.y; bj.z = q.z; bj.l = ldg_idx(lambda, j);
        return p;
    }
    __device__ float4 loadA(int j) const { return posv[j]; }
    __device__ BT loadB(int j) const { BT b; stage_impl(j, b); return b; }
    __device__ float4 stage(const Consts &, int j, BT &bj) const { return stage_impl(j, bj); }
    __device__ bool begin(const Consts &c, int i, const float4 &, Own &o) const {
        bool ok = true;   // no early return: begin()'s loads go out with the rest of the prologue (k_nbr_pass)
        if (!AF || c.ghosts) ok = META_ACTIVE_FLUID(meta[i]);
        const float4 q = xs[i];
        o.px = q.x; o.py = q.y; o.pz = q.z;
        o.l = lambda[i];
        o.ax = o.ay = o.az = 0.0f;
        return ok;
    }
    __device__ void pair(const Consts &c, Own &o, float, float, float, float, const float4 &a, const BT &bj, int) const {
        const float dx = o.px - bj.x, dy = o.py - bj.y, dz = o.pz - bj.z;
        const float r2 = dx * dx + dy * dy + dz * dz;
#if SPH_FAST
        float w, gs;
        pbfc_kernel(c, r2, w, gs);
        const float k = ((o.l + bj.l) * a.w) * gs;
        o.ax += k * dx; o.ay += k * dy; o.az += k * dz;
#else
        float gx, gy, gz;
        kernGrad(c, dx, dy, dz, geom(c, r2), gx, gy, gz);
        const float k = (o.l + bj.l) * a.w;
        o.ax += k * gx; o.ay += k * gy; o.az += k * gz;
#endif
    }
    __device__ float finish(const Consts &, int i, const float4 &, Own &o) const {
        xs_out[i] = make_float4(o.px + o.ax, o.py + o.ay, o.pz + o.az, 0.0f);
        return 0.0f;
    }
    __device__ void passive(const Consts &, int, const float4 &) const {}
};

// x*_i = x_i + dt v*_i + boundary for fluid; every other particle's x* is its position, in both buffers (the correction pass writes
// fluid particles only).  posv and the velocities stay as they are.
__global__ void __launch_bounds__(256)
k_pbfc_predict(const Consts c, const float4 *posv, const float4 *velm, const int *meta, float4 *xs, float4 *xs2, int all_fluid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    const float4 p = posv[i];
    const int m = all_fluid ? META_PACK(0, 1, 1) : meta[i];
    if (META_MAT(m) == 1) {
        float4 v = velm[i];
        float x = p.x + c.dt * v.x, y = p.y + c.dt * v.y, z = p.z + c.dt * v.z;
        if (META_DYN(m)) enforce_boundary(c, x, y, z, v.x, v.y, v.z);
        xs[i] = make_float4(x, y, z, 0.0f);
    } else {
        xs[i] = xs2[i] = make_float4(p.x, p.y, p.z, 0.0f);
    }
}

// x_i = boundary(x*_i), v_i = (x_i - x_old_i) / dt for fluid (posv held x_old until here: k_pbf_finish's velocity); then the emitter
// branch of update_fluid_position (base_solver.py:660-666) for the particles above gravitationUpper: one that turns fluid here takes
// part from the next step on.
__global__ void __launch_bounds__(256)
k_pbfc_finish(const Consts c, float4 *posv, float4 *velm, int *meta, const float4 *xs, const RigidPose *pose, int all_fluid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    const int m = all_fluid ? META_PACK(0, 1, 1) : meta[i];
    float4 p = posv[i];
    float4 v = velm[i];
    if (META_MAT(m) == 1) {
        const float4 q = xs[i];
        float x = q.x, y = q.y, z = q.z;
        if (META_DYN(m)) enforce_boundary(c, x, y, z, v.x, v.y, v.z);
#if SPH_FAST
        v.x = (x - p.x) * c.inv_dt; v.y = (y - p.y) * c.inv_dt; v.z = (z - p.z) * c.inv_dt;
#else
        v.x = (x - p.x) / c.dt; v.y = (y - p.y) / c.dt; v.z = (z - p.z) / c.dt;
#endif
        posv[i] = make_float4(x, y, z, p.w);
        velm[i] = v;
    } else if (up_coord(c, p) > c.g_upper) {
        const int obj = META_OBJ(m);
        if (obj >= 0 && pose->material[obj] == 1) {
            p.x += c.dt * v.x; p.y += c.dt * v.y; p.z += c.dt * v.z;
            if (up_coord(c, p) <= c.g_upper) {
                meta[i] = META_SET_MAT(m, 1);
                if (META_DYN(m)) enforce_boundary(c, p.x, p.y, p.z, v.x, v.y, v.z);
                velm[i] = v;
            }
            posv[i] = p;
        }
    }
}

static void l_pbfc_predict(State &s) {
    if (s.c.n == 0) return;
    hipLaunchKernelGGL(k_pbfc_predict, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, s.posv.cur(), s.velm.cur(), s.meta.cur(),
                       s.pbf_old, s.pbf_pos, s.c.all_fluid);
}

// the partial sums of C are finished by l_pbfc_delta: the iteration that meets the stop test still applies its correction, so inside
// a device-controlled loop the stop flag must not rise before the second walk has run (as PCISPH's, l_pcisph_rho_star)
// (reduce: a lone SPH_PH_PBFC_DENSITY_LAMBDA phase, which reports its own sum)
static void l_pbfc_density_lambda(State &s, int reduce) {
    launch_pass_af(s, 2, [&](auto af) {
        return PbfcDensityLambdaPass<af>{s.posv.cur(), s.pbf_old, s.meta.cur(), s.rho.cur(), s.pbf_lambda, s.pbf_eps, s.red_partial};
    });
    if (reduce && s.c.n > 0) l_reduce_sum(s, 3, cdiv(s.c.n, NBR_BLOCK));
}

// the corrected x* go to the second buffer, which then takes the first one's place; reduce: this walk closes an iteration whose walk
// A left partial sums (a lone SPH_PH_PBFC_DELTA phase has none to finish)
static void l_pbfc_delta(State &s, int reduce) {
    launch_pass_af(s, 2, [&](auto af) { return PbfcDeltaPass<af>{s.posv.cur(), s.pbf_old, s.meta.cur(), s.pbf_lambda, s.pbf_pos}; });
    std::swap(s.pbf_old, s.pbf_pos);
    if (reduce && s.c.n > 0 && !s.skip_residual) l_reduce_sum(s, 3, cdiv(s.c.n, NBR_BLOCK));   // (State::last_pass_listed is still walk A's)
}

static void l_pbfc_finish(State &s) {
    if (s.c.n == 0) return;
    s.masks_valid = 0;  // positions move
    hipLaunchKernelGGL(k_pbfc_finish, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, s.posv.cur(), s.velm.cur(), s.meta.cur(),
                       s.pbf_old, s.pose, s.c.all_fluid);
}

static void register_pbfc_launchers(Launch &L) {
    L.pbfc_predict = l_pbfc_predict;
    L.pbfc_density_lambda = l_pbfc_density_lambda;
    L.pbfc_delta = l_pbfc_delta;
    L.pbfc_finish = l_pbfc_finish;
}
