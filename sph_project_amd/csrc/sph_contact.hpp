// sph_contact.hpp -- rigid contact detection (the host's "contact" rigid backend): kernel and launcher; included by sph_kernels.hip
// inside the per-build namespace.  Semantics in include/sph_hip.h (sph_set_rigid_contact), design in DESIGN.md 13.
//
// Targets are the particles of dynamic rigid objects: a sparse, spatially clustered subset of the sorted order.  The pass is launched
// over the whole particle range; a workgroup without a target leaves behind one barrier (the sorted order keeps a body's particles in
// neighbouring cells, so most workgroups are all-or-nothing).  A target walks the 27 cells around its sorted cell -- 9 runs of 3 z-cells
// from the step's cell lists, as the PBF refine walks do -- and accepts rigid particles of other objects closer than D (D <= the cell
// size, so the 27 cells hold every partner).  Rigid particles have not moved since the sort when the pass runs, so their cells are exact.
//
// Accumulation.  Every accepted pair is converted to 64-bit fixed point (2^-32 per unit, as DevScalars::wrench) BEFORE it is summed:
//   * into a workgroup table in LDS, 64 slots opened by atomicCAS on the key (linear probing), ds_add_u64 / ds_max_u64 per value;
//   * behind a barrier every open slot goes out as 7 global 64-bit integer adds + 1 integer max onto the key's row.
// Integer addition commutes and every pair is rounded on its own, so the table is bit-reproducible whatever order lanes, waves and
// workgroups run in.  A pair whose workgroup table is full goes straight to the global row (same integers, same result).
#pragma once

#define SPH_CT_SLOTS 64
#define SPH_CT_SCALE 4294967296.0

__device__ __forceinline__ unsigned long long ct_fix(float v) { return (unsigned long long)__double2ll_rn((double)v * SPH_CT_SCALE); }

// one contact onto key `key`: midpoint m, depth * n (dx, dy, dz), depth d
__device__ __forceinline__ void ct_add(int *s_key, unsigned long long (*s_val)[SPH_CT_VALUES], unsigned long long *table, int key,
                                       float mx, float my, float mz, float dx, float dy, float dz, float d) {
    const unsigned long long v1 = ct_fix(mx), v2 = ct_fix(my), v3 = ct_fix(mz), v4 = ct_fix(dx), v5 = ct_fix(dy), v6 = ct_fix(dz);
    const unsigned long long v7 = ct_fix(d);
    unsigned long long *row = nullptr;
    for (int t = 0; t < SPH_CT_SLOTS; ++t) {
        const int slot = (key + t) & (SPH_CT_SLOTS - 1);
        const int old = atomicCAS(&s_key[slot], -1, key);
        if (old == -1 || old == key) { row = s_val[slot]; break; }
    }
    if (!row) row = table + (size_t)key * SPH_CT_VALUES;   // workgroup table full: the global row directly
    atomicAdd(row + 0, 1ull);
    atomicAdd(row + 1, v1); atomicAdd(row + 2, v2); atomicAdd(row + 3, v3);
    atomicAdd(row + 4, v4); atomicAdd(row + 5, v5); atomicAdd(row + 6, v6);
    atomicMax(row + 7, v7);
}

// bin of a direction: 2 * dominant axis (the first of equal magnitudes) + (that component < 0)
__device__ __forceinline__ int ct_bin(float x, float y, float z) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    if (ax >= ay && ax >= az) return x < 0.0f ? 1 : 0;
    if (ay >= az) return y < 0.0f ? 3 : 2;
    return z < 0.0f ? 5 : 4;
}

__global__ void __launch_bounds__(256)
k_rigid_contact(const Consts c, const ContactArgs a, const int *cell_start, const float4 *posv, const int *meta,
                unsigned long long *table, float4 *part, unsigned long long *pairs) {
    __shared__ int s_key[SPH_CT_SLOTS];
    __shared__ unsigned long long s_val[SPH_CT_SLOTS][SPH_CT_VALUES];
    __shared__ unsigned s_pairs;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int mi = 0;
    bool tgt = false;
    if (i < live_n(c)) {
        mi = meta[i];
        tgt = META_MAT(mi) == 2 && META_DYN(mi) && !META_GHOST(mi) && !META_DEAD(mi) && META_OBJ(mi) >= 0 &&
              META_OBJ(mi) < SPH_NOBJ;
    }
    if (!__syncthreads_or(tgt)) return;   // workgroup-uniform
    if (threadIdx.x < SPH_CT_SLOTS) {
        s_key[threadIdx.x] = -1;
        for (int q = 0; q < SPH_CT_VALUES; ++q) s_val[threadIdx.x][q] = 0ull;
    }
    if (threadIdx.x == 0) s_pairs = 0u;
    __syncthreads();
    if (tgt) {
        const int A = META_OBJ(mi);
        const float4 p = posv[i];
        const float D = a.D, D2 = a.D * a.D;
        int np = 0;
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
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
                    if (!(r2 < D2)) continue;
                    const int mj = ldg_idx(meta, j);
                    const int B = META_OBJ(mj);
                    if (META_MAT(mj) != 2 || B == A || B >= SPH_NOBJ) continue;
                    const float r = sqrtf(r2);
                    if (!(r > 1e-6f && r < D)) continue;
                    const float d = D - r, k = d / r;
                    const float nx_ = dx * k, ny_ = dy * k, nz_ = dz * k;   // depth * n
                    const int bin = ct_bin(dx, dy, dz);
                    const int part_b = B >= 0 ? B : 20 + bin;               // the domain box (object id -1): one partner per bin
                    ct_add(s_key, s_val, table, (A * SPH_CT_PARTNERS + part_b) * SPH_CT_BINS + bin,
                           0.5f * (p.x + q.x), 0.5f * (p.y + q.y), 0.5f * (p.z + q.z), nx_, ny_, nz_, d);
                    sx += nx_; sy += ny_; sz += nz_;
                    ++np;
                }
            }
        }
        if (a.walls) {   // the six domain planes: partner 20 + bin, contact point = the projection onto the plane
            const float half = 0.5f * D;
            const float pc[3] = {p.x, p.y, p.z};
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    const float dist = side == 0 ? pc[ax] - a.lo[ax] : a.hi[ax] - pc[ax];
                    if (!(dist < half)) continue;
                    const float d = half - dist, sg = side == 0 ? 1.0f : -1.0f;
                    const int bin = 2 * ax + side;
                    const float m0 = ax == 0 ? pc[0] - sg * dist : pc[0], m1 = ax == 1 ? pc[1] - sg * dist : pc[1];
                    const float m2 = ax == 2 ? pc[2] - sg * dist : pc[2];
                    const float n0 = ax == 0 ? sg * d : 0.0f, n1 = ax == 1 ? sg * d : 0.0f, n2 = ax == 2 ? sg * d : 0.0f;
                    ct_add(s_key, s_val, table, (A * SPH_CT_PARTNERS + 20 + bin) * SPH_CT_BINS + bin, m0, m1, m2, n0, n1, n2, d);
                    sx += n0; sy += n1; sz += n2;
                    ++np;
                }
            }
        }
        part[i] = make_float4(sx, sy, sz, (float)np);
        if (np) atomicAdd(&s_pairs, (unsigned)np);
    }
    __syncthreads();
    if (threadIdx.x < SPH_CT_SLOTS) {
        const int key = s_key[threadIdx.x];
        if (key >= 0) {
            unsigned long long *row = table + (size_t)key * SPH_CT_VALUES;
            for (int q = 0; q < SPH_CT_VALUES - 1; ++q) atomicAdd(row + q, s_val[threadIdx.x][q]);
            atomicMax(row + SPH_CT_VALUES - 1, s_val[threadIdx.x][SPH_CT_VALUES - 1]);
        }
    }
    if (threadIdx.x == 0 && s_pairs) atomicAdd(pairs, (unsigned long long)s_pairs);
}

// the pass counts into `pairs` from zero (sph_get_rigid_contact_pairs: the last pass); the table accumulates until the host resets it
static void l_rigid_contact(State &s) {
    if (s.c.n == 0 || !s.contact_on) return;
    hipMemsetAsync(s.contact_pairs, 0, sizeof(unsigned long long), s.stream);
    hipLaunchKernelGGL(k_rigid_contact, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, s.contact, s.cell_start, s.posv.cur(),
                       s.meta.cur(), s.contact_table, s.contact_part, s.contact_pairs);
}

static void register_contact_launchers(Launch &L) { L.rigid_contact = l_rigid_contact; }
