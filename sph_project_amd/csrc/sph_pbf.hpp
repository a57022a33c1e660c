// sph_pbf.hpp -- PBF (SPH/fluid_solvers/PBF.py, Position Based Fluids): kernels and launchers; included by sph_kernels.hip inside
// the per-build namespace.
//
// Access pattern.  The five refine() iterations of a step (PBF.py:62-66) walk the cell lists of the sort at the START of the step while
// the positions move: base_container.py:550 for_all_neighbors takes the centre cell from particle i's CURRENT position and tests the
// distance with the current positions of both particles, but the particle ranges of the 27 cells are the step-start sort's.  The tiled
// neighbour pass (k_nbr_pass) stages the candidate runs of a workgroup from the cells its particles were SORTED into, which is the
// wrong candidate set for a particle that x += dt v or fix_position has moved across a cell face.  The refine walks below therefore
// walk per particle: the 27 cells around the current cell (9 runs of 3 z-cells, cells outside the grid skipped), candidates in
// ascending sorted index -- the reference's order (ox, oy, oz) with oz fastest.  A particle whose current cell differs from its sorted
// cell (x_old.w holds it) is counted ("recentred walks", SphStats::pbf_recentred); it takes the same code path.
//
// Two deviations, both forced:
//   D1  fix_position is Jacobi: every delta is computed from the positions at the start of the pass, then all are applied (the reference
//       updates particle_positions[p_i] in place while other iterations read it as pos_j: a race on a GPU, Gauss-Seidel on a serial one);
//   D2  old positions and lambdas are sized particle_max_num (the reference allocates them with particle_num[None], still 0 then).
#pragma once

__device__ __forceinline__ int pbf_lin(const Consts &c, int cx, int cy, int cz) { return (cx * c.ny + cy) * c.nz + cz; }
// base_container.py:468 pos_to_index, one axis, NOT clamped: (int)(x / grid_size) truncates like the reference's cast.  During refine
// a particle can sit outside the domain (the boundary is enforced before and after the iterations only); its centre cell is then
// outside the grid and only the in-grid cells around it are walked.  (The quotient is bounded first: any value beyond the grid's
// first layer outside gives no cell to walk, and a NaN position walks nothing.)
__device__ __forceinline__ int pbf_coord(float x, float gs, int n) {
    const float t = fminf(fmaxf(x / gs, -2.0f), (float)(n + 1));
    return (int)t;
}

// one wave's share of the step statistics: pairs (weighted by the reference passes the walk stands for) and recentred walks
__device__ __forceinline__ void pbf_count(const Consts &c, DevScalars *scal, unsigned long long *recentred, int npairs, int wp, bool moved) {
    const float fp = wave_sum((float)npairs);
    const unsigned long long mv = __ballot(moved);
    if ((threadIdx.x & 63) == 0) {
        const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) & (SPH_STAT_SLOTS - 1);
        if (fp > 0.0f) {
            atomicAdd(&scal->pairs[c.stat_bank][slot], (unsigned long long)fp * (unsigned long long)wp);
            atomicAdd(&scal->evals[c.stat_bank][slot], (unsigned long long)fp);
        }
        if (mv) atomicAdd(&recentred[c.stat_bank], (unsigned long long)__popcll(mv));
    }
}

// The walk of base_container.py:550-560 around particle i's current position p: the body runs for every j != i with |x_i - x_j| < dh
// (q = posv[j], dx dy dz = x_i - x_j, r2), runs in (ox, oy) order, particles ascending; np counts the accepted pairs.  (A macro, not a
// function taking a lambda: the closure of the rigid-aware forms was left on the stack, 64 bytes of scratch per lane.)
#define PBF_WALK_BEGIN(c, cell_start, pos, i, p, np)                                                                                   \
    {                                                                                                                                \
        const int cx_ = pbf_coord((p).x, (c).grid_size, (c).nx), cy_ = pbf_coord((p).y, (c).grid_size, (c).ny);                     \
        const int cz_ = pbf_coord((p).z, (c).grid_size, (c).nz);                                                                     \
        const int z0_ = cz_ > 0 ? cz_ - 1 : 0, z1_ = cz_ < (c).nz - 1 ? cz_ + 1 : (c).nz - 1;                                          \
        if (z0_ <= z1_)                                                                                                              \
        for (int ox_ = -1; ox_ <= 1; ++ox_) {                                                                                        \
            const int x_ = cx_ + ox_;                                                                                                \
            if (x_ < 0 || x_ >= (c).nx) continue;                                                                                    \
            for (int oy_ = -1; oy_ <= 1; ++oy_) {                                                                                    \
                const int y_ = cy_ + oy_;                                                                                            \
                if (y_ < 0 || y_ >= (c).ny) continue;                                                                                \
                const int b_ = (cell_start)[pbf_lin(c, x_, y_, z0_)], e_ = (cell_start)[pbf_lin(c, x_, y_, z1_) + 1];                \
                for (int j = b_; j < e_; ++j) {                                                                                      \
                    if (j == (i)) continue;                                                                                          \
                    const float4 q = ldg_idx(pos, j);                                                                                \
                    const float dx = (p).x - q.x, dy = (p).y - q.y, dz = (p).z - q.z;                                                \
                    const float r2 = dx * dx + dy * dy + dz * dz;                                                                    \
                    if (!(r2 < (c).h2)) continue;                                                                                    \
                    ++(np);
#define PBF_WALK_END \
                }    \
            }        \
        }            \
    }

__device__ __forceinline__ bool pbf_moved(const Consts &c, const float4 &p, const float4 &old) {
    const int cx = pbf_coord(p.x, c.grid_size, c.nx), cy = pbf_coord(p.y, c.grid_size, c.ny), cz = pbf_coord(p.z, c.grid_size, c.nz);
    const bool inside = cx >= 0 && cx < c.nx && cy >= 0 && cy < c.ny && cz >= 0 && cz < c.nz;
    return !inside || pbf_lin(c, cx, cy, cz) != __float_as_int(old.w);
}

// PBF.py:151-152 save_old_position + update_fluid_position (base_solver.py:652, emitter branch included) + :154 enforce_domain_boundary.
// x_old = (position at the sort, sorted cell id).  The fluid velocity is not written: recompute_fluid_velocity overwrites it.
__global__ void __launch_bounds__(256)
k_pbf_predict(const Consts c, float4 *posv, float4 *velm, int *meta, float4 *old, const RigidPose *pose, int all_fluid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    float4 p = posv[i];
    const int lin = pbf_lin(c, cell_coord(p.x, c.grid_size, c.nx), cell_coord(p.y, c.grid_size, c.ny), cell_coord(p.z, c.grid_size, c.nz));
    old[i] = make_float4(p.x, p.y, p.z, __int_as_float(lin));
    float4 v = velm[i];
    const int m = all_fluid ? META_PACK(0, 1, 1) : meta[i];
    if (META_MAT(m) == 1) {
        p.x += c.dt * v.x; p.y += c.dt * v.y; p.z += c.dt * v.z;
        if (META_DYN(m)) enforce_boundary(c, p.x, p.y, p.z, v.x, v.y, v.z);
        posv[i] = p;
    } else if (up_coord(c, p) > c.g_upper) {  // emitter branch base_solver.py:660-666
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

// PBF.py:62 compute_density (base_solver.py:522, self term V_i W(0) = 0) + :68 compute_lambda (+task :84), one walk: lambda_i needs
// only its own rho_i.  A rigid neighbour's gradient carries rho_i / rho0 (:95-101), which is known after the walk: its sums are kept
// apart and scaled in the epilogue.  Writes rho (fluid), lambda (fluid).
template <bool AF>
__global__ void __launch_bounds__(256)
k_pbf_density_lambda(const Consts c, const int *cell_start, const float4 *posv, const float4 *velm, const int *meta, const float4 *old,
                     float *rho, float *lambda, DevScalars *scal, unsigned long long *recentred) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int np = 0;
    bool moved = false;
    if (i < c.n && (AF || META_MAT(meta[i]) == 1)) {
        const float4 p = posv[i];
        moved = pbf_moved(c, p, old[i]);
        float d = 0.0f, fx = 0.0f, fy = 0.0f, fz = 0.0f, f2 = 0.0f, rx = 0.0f, ry = 0.0f, rz = 0.0f, r2s = 0.0f;
        PBF_WALK_BEGIN(c, cell_start, posv, i, p, np)
            const Geom g = geom(c, r2);
            d += q.w * Poly6Kernel::W(c, g);
            float gx, gy, gz;
            Poly6Kernel::grad(c, dx, dy, dz, g, gx, gy, gz);
            const int mj = AF ? 1 : META_MAT(meta[j]);
            if (mj == 1) {
                const float s = fdiv(ldg_idx(velm, j).w, c.rho0);
                gx *= s; gy *= s; gz *= s;
                f2 += gx * gx + gy * gy + gz * gz;
                fx += gx; fy += gy; fz += gz;
            } else if (mj == 2) {
                gx *= q.w; gy *= q.w; gz *= q.w;
                r2s += gx * gx + gy * gy + gz * gz;
                rx += gx; ry += gy; rz += gz;
            }
        PBF_WALK_END
        const float r = d * c.rho0;
        rho[i] = r;
        if (!AF) {
            const float s = fdiv(r, c.rho0);
            fx += s * rx; fy += s * ry; fz += s * rz;
            f2 += (s * s) * r2s;
        }
        const float den = f2 + (fx * fx + fy * fy + fz * fz) + SPH_PBF_LAMBDA_EPS;
        lambda[i] = -fdiv(fdiv(r, c.rho0) - 1.0f, den);
    }
    pbf_count(c, scal, recentred, np, 2, moved);   // compute_density + compute_lambda
}

// PBF.py:104 fix_position (+task :113), Jacobi (D1): reads the positions at the start of the pass, writes pos_out (every particle:
// the launcher swaps it in).  s_corr = -corrK (W(r) / W(0.3 h))^4 (:50-58).
template <bool AF>
__global__ void __launch_bounds__(256)
k_pbf_fix_position(const Consts c, const int *cell_start, const float4 *posv, const float4 *velm, const int *meta, const float4 *old,
                   const float *lambda, float4 *pos_out, DevScalars *scal, unsigned long long *recentred) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int np = 0;
    bool moved = false;
    if (i < c.n) {
        float4 p = posv[i];
        if (AF || META_MAT(meta[i]) == 1) {
            moved = pbf_moved(c, p, old[i]);
            const float li = lambda[i];
            const float wq = poly6W(c, SPH_PBF_CORR_DQ * c.h);
            float ax = 0.0f, ay = 0.0f, az = 0.0f;
            PBF_WALK_BEGIN(c, cell_start, posv, i, p, np)
                const Geom g = geom(c, r2);
                float gx, gy, gz;
                Poly6Kernel::grad(c, dx, dy, dz, g, gx, gy, gz);
                float x = fdiv(Poly6Kernel::W(c, g), wq);
                x = x * x; x = x * x;
                const float sc = -SPH_PBF_CORR_K * x;
                const int mj = AF ? 1 : META_MAT(meta[j]);
                if (mj == 1) {
                    const float k = li + ldg_idx(lambda, j) + sc, m = ldg_idx(velm, j).w;
                    ax += ((k * gx) * m); ay += ((k * gy) * m); az += ((k * gz) * m);
                } else if (mj == 2) {
                    const float k = (li + li) + sc, m = q.w * c.rho0;
                    ax += ((k * gx) * m); ay += ((k * gy) * m); az += ((k * gz) * m);
                }
            PBF_WALK_END
            p.x += fdiv(ax, c.rho0); p.y += fdiv(ay, c.rho0); p.z += fdiv(az, c.rho0);
        }
        pos_out[i] = p;
    }
    pbf_count(c, scal, recentred, np, 1, moved);
}

// PBF.py:156 enforce_domain_boundary + :158 recompute_fluid_velocity: v = (x - x_old) / dt for fluid (the boundary's velocity response
// is overwritten, as in the reference)
__global__ void __launch_bounds__(256)
k_pbf_finish(const Consts c, float4 *posv, float4 *velm, const int *meta, const float4 *old, int all_fluid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    const int m = all_fluid ? META_PACK(0, 1, 1) : meta[i];
    if (META_MAT(m) != 1) return;
    float4 p = posv[i];
    float4 v = velm[i];
    if (META_DYN(m)) {
        const float4 p_in = p;
        enforce_boundary(c, p.x, p.y, p.z, v.x, v.y, v.z);
        if (p.x != p_in.x || p.y != p_in.y || p.z != p_in.z) posv[i] = p;
    }
    const float4 o = old[i];
#if SPH_FAST
    v.x = (p.x - o.x) * c.inv_dt; v.y = (p.y - o.y) * c.inv_dt; v.z = (p.z - o.z) * c.inv_dt;
#else
    v.x = (p.x - o.x) / c.dt; v.y = (p.y - o.y) / c.dt; v.z = (p.z - o.z) / c.dt;
#endif
    velm[i] = v;
}

static void l_pbf_predict(State &s) {
    if (s.c.n == 0) return;
    s.masks_valid = 0;  // positions move
    hipLaunchKernelGGL(k_pbf_predict, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, s.posv.cur(), s.velm.cur(), s.meta.cur(),
                       s.pbf_old, s.pose, s.c.all_fluid);
}

static void l_pbf_density_lambda(State &s) {
    if (s.c.n == 0) return;
    dispatch_bool(s.c.all_fluid, [&](auto af) {
        hipLaunchKernelGGL(k_pbf_density_lambda<af>, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, s.cell_start, s.posv.cur(),
                           s.velm.cur(), s.meta.cur(), s.pbf_old, s.rho.cur(), s.pbf_lambda, s.scal, s.pbf_recentred);
    });
}

// the new positions go to the scratch buffer, which then takes the place of the current one (the old one is the next scratch)
static void l_pbf_fix_position(State &s) {
    if (s.c.n == 0) return;
    s.masks_valid = 0;
    dispatch_bool(s.c.all_fluid, [&](auto af) {
        hipLaunchKernelGGL(k_pbf_fix_position<af>, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, s.cell_start, s.posv.cur(),
                           s.velm.cur(), s.meta.cur(), s.pbf_old, s.pbf_lambda, s.pbf_pos, s.scal, s.pbf_recentred);
    });
    float4 *t = s.posv.b[s.posv.c]; s.posv.b[s.posv.c] = s.pbf_pos; s.pbf_pos = t;
}

static void l_pbf_finish(State &s) {
    if (s.c.n == 0) return;
    hipLaunchKernelGGL(k_pbf_finish, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, s.posv.cur(), s.velm.cur(), s.meta.cur(),
                       s.pbf_old, s.c.all_fluid);
}

static void register_pbf_launchers(Launch &L) {
    L.pbf_predict = l_pbf_predict;
    L.pbf_density_lambda = l_pbf_density_lambda;
    L.pbf_fix_position = l_pbf_fix_position;
    L.pbf_finish = l_pbf_finish;
}
