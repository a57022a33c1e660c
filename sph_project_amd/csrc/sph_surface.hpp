// sph_surface.hpp -- surface reconstruction (fluid particles -> triangle mesh): kernels and launchers; included by sph_kernels.hip inside
// the per-build namespace.  Method in DESIGN.md 14, semantics in include/sph_hip.h (sph_surface_create), float64 restatement in
// tests/surface_model.py.
//
// Passes (one stream, the host reads three counts in between: particles' coarse bounds, active bricks, vertices / triangles):
//   bin     coarse cell per particle (edge B e >= h), histogram, scan, scatter, then a rank inside each cell by the bit pattern of (x, y, z):
//           the binned order is a function of the particle SET; V_j = 1 / sum_k W over the 27 cells in a fixed order
//   flags   a coarse cell is an active brick when its 3x3x3 neighbourhood holds a particle; scan -> brick ids in coarse linear order
//   field   one workgroup per brick (per part of PPT * 256 points): the 27 cells' particles (xyz + V) staged in LDS in chunks, every
//           thread owns PPT grid points and sums V_j W(x - x_j) in the staging order.  Every point is owned by one brick: one value.
//   count   per point: its cube's case (8 corners, neighbour bricks through brick_id, 0 outside active bricks) and the crossings of the
//           3 edges it owns; workgroup scans in point order -> per-brick counts -> scans over the bricks
//   emit    vertices in (brick, point, axis) order by linear interpolation, triangles in (brick, cube, table) order; an edge's vertex is
//           found through its owner point's word, in whichever brick that point lies
//   normals one thread per vertex: -grad phi / |grad phi| from the 27 cells around it
// No float atomics: the only atomics count (histogram slots, compaction slots, pair tests), and every float sum runs in a fixed order.
#pragma once
#include "sph_mc_table.hpp"

#define SURF_CHUNK 1024   // float4 particles per LDS chunk of the field pass (16 KiB)

// cube edge e -> owner point offset and axis (sph_project_amd/mc_table.py EDGES); entry 12 = padding
__constant__ const signed char surf_edge_off[13][3] = {{0, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 1, 1}, {0, 0, 0}, {1, 0, 0}, {0, 0, 1},
                                                       {1, 0, 1}, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {0, 0, 0}};
__constant__ const signed char surf_edge_axis[13] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 0};

__device__ __forceinline__ int surf_coord(const SurfDev &d, float x, int axis) {
#if SPH_FAST
    return (int)floorf(x * (1.0f / d.be)) - d.cmin[axis];
#else
    return (int)floorf(x / d.be) - d.cmin[axis];
#endif
}
__device__ __forceinline__ int surf_lin(const SurfDev &d, int x, int y, int z) { return (x * d.cn[1] + y) * d.cn[2] + z; }

// the project's cubic spline (base_solver.py:57) with support h: W(r) for r < h
__device__ __forceinline__ float surf_w(const SurfDev &d, float r2) {
    const float r = __builtin_sqrtf(r2);
#if SPH_FAST
    const float q = r * (1.0f / d.h);
#else
    const float q = r / d.h;
#endif
    if (q <= 0.5f) { const float q2 = q * q; return d.kW * (6.0f * q2 * q - 6.0f * q2 + 1.0f); }
    const float t = 1.0f - q;
    return q <= 1.0f ? d.kW * 2.0f * (t * t * t) : 0.0f;
}

// exclusive scan of one value per thread over a 256-thread workgroup (every thread calls it); *total = the workgroup's sum
__device__ __forceinline__ int surf_block_scan(int v, int *s, int *total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int a = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    const int incl = s[t];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

// --- exclusive scan of int a[0, n) in place, a[n] = the total (tiles of 1024, one workgroup over the tile sums, add back) --------------
__global__ void __launch_bounds__(256) k_surf_scan_tile(int *a, int n, int *tile_sum) {
    __shared__ int s[256];
    const int base = blockIdx.x * 1024 + threadIdx.x * 4;
    int v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = base + k < n ? a[base + k] : 0; sum += v[k]; }
    int total;
    int run = surf_block_scan(sum, s, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (base + k < n) a[base + k] = run; run += v[k]; }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
__global__ void __launch_bounds__(256) k_surf_scan_top(int *tile_sum, int tiles, int *a, int n) {
    __shared__ int s[256];
    int carry = 0;
    for (int b = 0; b < tiles; b += 256) {
        const int i = b + threadIdx.x;
        const int v = i < tiles ? tile_sum[i] : 0;
        int total;
        const int ex = surf_block_scan(v, s, &total);
        if (i < tiles) tile_sum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) a[n] = carry;
}
__global__ void __launch_bounds__(256) k_surf_scan_add(int *a, int n, const int *tile_sum) {
    const int base = blockIdx.x * 1024;
    const int off = tile_sum[blockIdx.x];
    for (int k = threadIdx.x; k < 1024; k += 256)
        if (base + k < n) a[base + k] += off;
}
static void surf_scan(SurfDev &d, int *a, int n) {
    const int tiles = cdiv(n > 0 ? n : 1, 1024);
    hipLaunchKernelGGL(k_surf_scan_tile, dim3(tiles), dim3(256), 0, d.stream, a, n, d.scan_tmp);
    hipLaunchKernelGGL(k_surf_scan_top, dim3(1), dim3(256), 0, d.stream, d.scan_tmp, tiles, a, n);
    hipLaunchKernelGGL(k_surf_scan_add, dim3(tiles), dim3(256), 0, d.stream, a, n, (const int *)d.scan_tmp);
}

// --- input ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_surf_compact(const float4 *posv, const int *meta, int n, int obj, float4 *xin, int *counter) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int m = meta[i];
    if (META_OBJ(m) != obj || META_GHOST(m) || META_DEAD(m)) return;
    const float4 p = posv[i];
    xin[atomicAdd(counter, 1)] = make_float4(p.x, p.y, p.z, 0.0f);   // slot order is irrelevant: the bin pass orders by key
}
static void l_surf_compact(SurfDev &d, const float4 *posv, const int *meta, int n, int obj) {
    hipMemsetAsync(d.counter, 0, sizeof(int), d.stream);
    if (n > 0) hipLaunchKernelGGL(k_surf_compact, dim3(cdiv(n, 256)), dim3(256), 0, d.stream, posv, meta, n, obj, d.xin, d.counter);
}

// min / max coarse coordinates: reduced in LDS first, then 7 global atomics per workgroup (1.23 M threads on the same 6 global words
// took 1.3 ms on C2)
__global__ void __launch_bounds__(256) k_surf_bounds(SurfDev d) {
    __shared__ int s[7];
    if (threadIdx.x < 7) s[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : threadIdx.x < 6 ? INT_MIN : 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < d.n) {
        const float4 p = d.xin[i];
        const float v[3] = {p.x, p.y, p.z};
        bool bad = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) bad |= !(fabsf(v[a]) < 1e8f * d.be);   // non-finite or absurd: the host refuses the input
        if (bad) atomicOr(&s[6], 1);
        else {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int c = surf_coord(d, v[a], a);   // (cmin = 0 here: absolute coarse coordinates)
                atomicMin(&s[a], c);
                atomicMax(&s[3 + a], c);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&d.bounds[threadIdx.x], s[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&d.bounds[threadIdx.x], s[threadIdx.x]);
    else if (threadIdx.x == 6 && s[6]) atomicOr(&d.bounds[6], 1);
}
static void l_surf_bounds(SurfDev &d) {
    if (d.n > 0) hipLaunchKernelGGL(k_surf_bounds, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d);
}

// --- bin, key order, volumes ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int surf_cell_of(const SurfDev &d, float4 p) {
    return surf_lin(d, surf_coord(d, p.x, 0), surf_coord(d, p.y, 1), surf_coord(d, p.z, 2));
}
__global__ void __launch_bounds__(256) k_surf_hist(SurfDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const int c = surf_cell_of(d, d.xin[i]);
    d.pcell[i] = c;
    d.pslot[i] = atomicAdd(&d.cell_start[c], 1);
}
__global__ void __launch_bounds__(256) k_surf_scatter(SurfDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    d.xtmp[d.cell_start[d.pcell[i]] + d.pslot[i]] = d.xin[i];
}
// key order inside a cell: (bits of x, bits of y, bits of z), ties (bit-identical positions) by arrival slot -- they are interchangeable
__global__ void __launch_bounds__(256) k_surf_rank(SurfDev d) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d.n) return;
    const float4 p = d.xtmp[j];
    const int c = surf_cell_of(d, p);
    const int b = d.cell_start[c], e = d.cell_start[c + 1];
    const unsigned kx = __float_as_uint(p.x), ky = __float_as_uint(p.y), kz = __float_as_uint(p.z);
    int rank = 0;
    for (int k = b; k < e; ++k) {
        const float4 q = d.xtmp[k];
        const unsigned qx = __float_as_uint(q.x), qy = __float_as_uint(q.y), qz = __float_as_uint(q.z);
        const bool less = qx != kx ? qx < kx : qy != ky ? qy < ky : qz != kz ? qz < kz : k < j;
        rank += less;
    }
    d.xs[b + rank] = p;
}
// V_j = 1 / sum_k W(x_j - x_k) over the 27 cells (9 runs of 3 z-cells), self included; writes (xyz, V) into out
__global__ void __launch_bounds__(256) k_surf_volume(SurfDev d, const float4 *xs, float4 *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const float4 p = xs[i];
    const int cx = surf_coord(d, p.x, 0), cy = surf_coord(d, p.y, 1), cz = surf_coord(d, p.z, 2);   // 1 .. cn - 2 (empty margin)
    float sum = 0.0f;
    for (int ox = -1; ox <= 1; ++ox)
        for (int oy = -1; oy <= 1; ++oy) {
            const int b = d.cell_start[surf_lin(d, cx + ox, cy + oy, cz - 1)], e = d.cell_start[surf_lin(d, cx + ox, cy + oy, cz + 1) + 1];
            for (int k = b; k < e; ++k) {
                const float4 q = xs[k];
                const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
                const float r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < d.h2) sum += surf_w(d, r2);
            }
        }
    out[i] = make_float4(p.x, p.y, p.z, 1.0f / sum);
}
static void l_surf_bin(SurfDev &d) {
    hipMemsetAsync(d.cell_start, 0, sizeof(int) * ((size_t)d.G + 1), d.stream);
    const int g = cdiv(d.n, 256);
    hipLaunchKernelGGL(k_surf_hist, dim3(g), dim3(256), 0, d.stream, d);
    surf_scan(d, d.cell_start, d.G);
    hipLaunchKernelGGL(k_surf_scatter, dim3(g), dim3(256), 0, d.stream, d);
    hipLaunchKernelGGL(k_surf_rank, dim3(g), dim3(256), 0, d.stream, d);
    // xs (key order, w = 0) -> xtmp (key order, w = V); the two swap so that xs holds the result
    hipLaunchKernelGGL(k_surf_volume, dim3(g), dim3(256), 0, d.stream, d, (const float4 *)d.xs, d.xtmp);
    float4 *t = d.xs; d.xs = d.xtmp; d.xtmp = t;
}

// --- active bricks ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_surf_flags(SurfDev d) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d.G) return;
    const int cz = c % d.cn[2], cy = (c / d.cn[2]) % d.cn[1], cx = c / (d.cn[2] * d.cn[1]);
    int f = 0;
    for (int ox = -1; ox <= 1 && !f; ++ox)
        for (int oy = -1; oy <= 1 && !f; ++oy)
            for (int oz = -1; oz <= 1 && !f; ++oz) {
                const int x = cx + ox, y = cy + oy, z = cz + oz;
                if (x < 0 || y < 0 || z < 0 || x >= d.cn[0] || y >= d.cn[1] || z >= d.cn[2]) continue;
                const int l = surf_lin(d, x, y, z);
                f = d.cell_start[l + 1] > d.cell_start[l];
            }
    d.flag[c] = f;
}
static void l_surf_flags(SurfDev &d) {
    hipLaunchKernelGGL(k_surf_flags, dim3(cdiv(d.G, 256)), dim3(256), 0, d.stream, d);
    surf_scan(d, d.flag, d.G);
}
__global__ void __launch_bounds__(256) k_surf_bricks(SurfDev d) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d.G) return;
    const int f = d.flag[c];
    const bool on = d.flag[c + 1] != f;
    d.brick_id[c] = on ? f : -1;
    if (on) d.brick_cell[f] = c;
}

// --- the field (hot pass) ------------------------------------------------------------------------------------------------------------
// blockIdx.x = brick, blockIdx.y = part: points [part * 256 PPT, (part + 1) * 256 PPT) of the brick's B^3, point p = part * 256 PPT +
// k * 256 + tid at local (p / B^2, p / B % B, p % B).  Every point sums its particles in the staging order: 9 runs (x, y, z-1..z+1)
// of the 27 cells, each run in key order, in chunks of SURF_CHUNK.
template <int PPT>
__global__ void __launch_bounds__(256) k_surf_field(SurfDev d) {
    __shared__ float4 s_x[SURF_CHUNK];
    __shared__ int s_run[9][2];
    const int brick = blockIdx.x;
    const int c = d.brick_cell[brick];
    const int cz = c % d.cn[2], cy = (c / d.cn[2]) % d.cn[1], cx = c / (d.cn[2] * d.cn[1]);
    if (threadIdx.x < 9) {
        const int x = cx + (int)threadIdx.x / 3 - 1, y = cy + (int)threadIdx.x % 3 - 1;
        int b = 0, e = 0;
        if (x >= 0 && y >= 0 && x < d.cn[0] && y < d.cn[1]) {
            const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz < d.cn[2] - 1 ? cz + 1 : d.cn[2] - 1;
            b = d.cell_start[surf_lin(d, x, y, z0)];
            e = d.cell_start[surf_lin(d, x, y, z1) + 1];
        }
        s_run[threadIdx.x][0] = b;
        s_run[threadIdx.x][1] = e;
    }
    float px[PPT], py[PPT], pz[PPT], acc[PPT];
    const int p0 = blockIdx.y * 256 * PPT + (int)threadIdx.x;
    const int gx = (d.cmin[0] + cx) * d.B, gy = (d.cmin[1] + cy) * d.B, gz = (d.cmin[2] + cz) * d.B;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = p0 + k * 256;
        acc[k] = 0.0f;
        if (p < d.P) {
            px[k] = (float)(gx + p / (d.B * d.B)) * d.e;
            py[k] = (float)(gy + (p / d.B) % d.B) * d.e;
            pz[k] = (float)(gz + p % d.B) * d.e;
        } else {
            px[k] = py[k] = pz[k] = 1e30f;   // beyond every particle's support: r2 < h2 never holds
        }
    }
    __syncthreads();
    long long tests = 0;
    for (int r = 0; r < 9; ++r) {
        const int rb = s_run[r][0], re = s_run[r][1];
        for (int base = rb; base < re; base += SURF_CHUNK) {
            const int cnt = min(SURF_CHUNK, re - base);
            for (int k = threadIdx.x; k < cnt; k += 256) s_x[k] = d.xs[base + k];
            __syncthreads();
            for (int j = 0; j < cnt; ++j) {
                const float4 q = s_x[j];   // every lane reads the same word: an LDS broadcast
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const float dx = px[k] - q.x, dy = py[k] - q.y, dz = pz[k] - q.z;
                    const float r2 = dx * dx + dy * dy + dz * dz;
                    if (r2 < d.h2) acc[k] += q.w * surf_w(d, r2);
                }
            }
            tests += cnt;
            __syncthreads();
        }
    }
    float *out = d.phi + (size_t)brick * d.P;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = p0 + k * 256;
        if (p < d.P) out[p] = acc[k];
    }
    if (threadIdx.x == 0) {
        const int pts = min(d.P - (int)blockIdx.y * 256 * PPT, 256 * PPT);
        atomicAdd(d.pairs, (unsigned long long)(tests * pts));
    }
}
static void l_surf_field(SurfDev &d) {
    hipLaunchKernelGGL(k_surf_bricks, dim3(cdiv(d.G, 256)), dim3(256), 0, d.stream, d);
    hipMemsetAsync(d.pairs, 0, sizeof(unsigned long long), d.stream);
    if (d.nb == 0) return;
    // points per thread: 4, 8 or 12, the smallest that covers the brick in as few parts as 12 would
    const int parts = cdiv(d.P, 256 * 12);
    const int need = cdiv(d.P, 256 * parts);
    const dim3 grid(d.nb, parts);
    if (need <= 4) hipLaunchKernelGGL(k_surf_field<4>, dim3(d.nb, cdiv(d.P, 1024)), dim3(256), 0, d.stream, d);
    else if (need <= 8) hipLaunchKernelGGL(k_surf_field<8>, dim3(d.nb, cdiv(d.P, 2048)), dim3(256), 0, d.stream, d);
    else hipLaunchKernelGGL(k_surf_field<12>, grid, dim3(256), 0, d.stream, d);
}

// --- cubes and edges -----------------------------------------------------------------------------------------------------------------
// the point at brick-local (lx, ly, lz), each in [0, B]: its brick (-1: not an active brick) and index inside the brick
__device__ __forceinline__ int surf_locate(const SurfDev &d, int cx, int cy, int cz, int brick, int lx, int ly, int lz, int *idx) {
    if (lx >= d.B || ly >= d.B || lz >= d.B) {
        const int x = cx + (lx >= d.B), y = cy + (ly >= d.B), z = cz + (lz >= d.B);
        if (lx >= d.B) lx -= d.B;
        if (ly >= d.B) ly -= d.B;
        if (lz >= d.B) lz -= d.B;
        brick = (x < d.cn[0] && y < d.cn[1] && z < d.cn[2]) ? d.brick_id[surf_lin(d, x, y, z)] : -1;
    }
    *idx = (lx * d.B + ly) * d.B + lz;
    return brick;
}
__device__ __forceinline__ float surf_phi_at(const SurfDev &d, int cx, int cy, int cz, int brick, int lx, int ly, int lz) {
    int idx;
    const int b = surf_locate(d, cx, cy, cz, brick, lx, ly, lz, &idx);
    return b >= 0 ? d.phi[(size_t)b * d.P + idx] : 0.0f;
}
__device__ __forceinline__ int surf_case(const SurfDev &d, int cx, int cy, int cz, int brick, int lx, int ly, int lz, float *f0) {
    int cs = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float f = surf_phi_at(d, cx, cy, cz, brick, lx + (k & 1), ly + ((k >> 1) & 1), lz + ((k >> 2) & 1));
        if (k == 0) *f0 = f;
        cs |= (f > d.iso ? 1 : 0) << k;
    }
    return cs;
}
__device__ __forceinline__ unsigned surf_mask(int cs) {
    return (unsigned)(((cs ^ (cs >> 1)) & 1) | (((cs ^ (cs >> 2)) & 1) << 1) | (((cs ^ (cs >> 4)) & 1) << 2));
}

__global__ void __launch_bounds__(256) k_surf_count(SurfDev d) {
    __shared__ int s[256];
    const int brick = blockIdx.x;
    const int c = d.brick_cell[brick];
    const int cz = c % d.cn[2], cy = (c / d.cn[2]) % d.cn[1], cx = c / (d.cn[2] * d.cn[1]);
    int vcarry = 0, tcarry = 0;
    for (int base = 0; base < d.P; base += 256) {
        const int p = base + (int)threadIdx.x;
        int nv = 0, nt = 0;
        unsigned word = 0;
        if (p < d.P) {
            float f0;
            const int cs = surf_case(d, cx, cy, cz, brick, p / (d.B * d.B), (p / d.B) % d.B, p % d.B, &f0);
            const unsigned m = surf_mask(cs);
            nv = __popc(m);
            nt = sph_mc_ntri[cs];
            word = ((unsigned)cs << 3) | m;
        }
        int vt, tt;
        const int vo = surf_block_scan(nv, s, &vt);
        surf_block_scan(nt, s, &tt);
        if (p < d.P) d.edge[(size_t)brick * d.P + p] = ((unsigned)(vcarry + vo) << 11) | word;
        vcarry += vt;
        tcarry += tt;
    }
    if (threadIdx.x == 0) { d.vbase[brick] = vcarry; d.tbase[brick] = tcarry; }
}
static void l_surf_count(SurfDev &d) {
    if (d.nb > 0) hipLaunchKernelGGL(k_surf_count, dim3(d.nb), dim3(256), 0, d.stream, d);
    surf_scan(d, d.vbase, d.nb);
    surf_scan(d, d.tbase, d.nb);
}

__global__ void __launch_bounds__(256) k_surf_emit(SurfDev d) {
    __shared__ int s[256];
    const int brick = blockIdx.x;
    const int c = d.brick_cell[brick];
    const int cz = c % d.cn[2], cy = (c / d.cn[2]) % d.cn[1], cx = c / (d.cn[2] * d.cn[1]);
    const int gx = (d.cmin[0] + cx) * d.B, gy = (d.cmin[1] + cy) * d.B, gz = (d.cmin[2] + cz) * d.B;
    const int vb = d.vbase[brick];
    int tcarry = d.tbase[brick];
    for (int base = 0; base < d.P; base += 256) {
        const int p = base + (int)threadIdx.x;
        int nt = 0;
        unsigned word = 0;
        int lx = 0, ly = 0, lz = 0;
        if (p < d.P) {
            word = d.edge[(size_t)brick * d.P + p];
            nt = sph_mc_ntri[(word >> 3) & 0xff];
            lx = p / (d.B * d.B); ly = (p / d.B) % d.B; lz = p % d.B;
            const unsigned m = word & 7u;
            if (m) {
                const float f0 = d.phi[(size_t)brick * d.P + p];
                int v = vb + (int)(word >> 11);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (!(m & (1u << a))) continue;
                    const float f1 = surf_phi_at(d, cx, cy, cz, brick, lx + (a == 0), ly + (a == 1), lz + (a == 2));
                    const float t = (d.iso - f0) / (f1 - f0);
                    float g[3] = {(float)(gx + lx), (float)(gy + ly), (float)(gz + lz)};
                    g[a] += t;
                    d.vert[3 * (size_t)v + 0] = g[0] * d.e;
                    d.vert[3 * (size_t)v + 1] = g[1] * d.e;
                    d.vert[3 * (size_t)v + 2] = g[2] * d.e;
                    ++v;
                }
            }
        }
        int tt;
        const int to = surf_block_scan(nt, s, &tt);
        if (nt) {
            const int cs = (word >> 3) & 0xff;
            int *out = d.tri + 3 * (size_t)(tcarry + to);
            for (int k = 0; k < 3 * nt; ++k) {
                const int e = sph_mc_tri[cs][k];
                const int a = surf_edge_axis[e];
                int idx;
                const int ob = surf_locate(d, cx, cy, cz, brick, lx + surf_edge_off[e][0], ly + surf_edge_off[e][1], lz + surf_edge_off[e][2], &idx);
                int v = -1;   // (an edge with a crossing never leaves the active bricks: DESIGN.md 14)
                if (ob >= 0) {
                    const unsigned w = d.edge[(size_t)ob * d.P + idx];
                    v = d.vbase[ob] + (int)(w >> 11) + __popc(w & 7u & ((1u << a) - 1u));
                }
                out[k] = v;
            }
        }
        tcarry += tt;
    }
}
static void l_surf_emit(SurfDev &d) {
    if (d.nb > 0) hipLaunchKernelGGL(k_surf_emit, dim3(d.nb), dim3(256), 0, d.stream, d);
}

// --- normals -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_surf_normals(SurfDev d, int nv) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const float x = d.vert[3 * (size_t)v], y = d.vert[3 * (size_t)v + 1], z = d.vert[3 * (size_t)v + 2];
    const int cx = surf_coord(d, x, 0), cy = surf_coord(d, y, 1), cz = surf_coord(d, z, 2);
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    for (int ox = -1; ox <= 1; ++ox)
        for (int oy = -1; oy <= 1; ++oy) {
            const int xx = cx + ox, yy = cy + oy;
            const int z0 = max(cz - 1, 0), z1 = min(cz + 1, d.cn[2] - 1);
            if (xx < 0 || yy < 0 || xx >= d.cn[0] || yy >= d.cn[1] || z0 > z1) continue;
            const int b = d.cell_start[surf_lin(d, xx, yy, z0)], e = d.cell_start[surf_lin(d, xx, yy, z1) + 1];
            for (int k = b; k < e; ++k) {
                const float4 q = d.xs[k];
                const float dx = x - q.x, dy = y - q.y, dz = z - q.z;
                const float r2 = dx * dx + dy * dy + dz * dz;
                if (!(r2 < d.h2) || r2 <= 0.0f) continue;
                const float r = __builtin_sqrtf(r2);
#if SPH_FAST
                const float qq = r * (1.0f / d.h);
#else
                const float qq = r / d.h;
#endif
                const float f = 1.0f - qq;
                const float dw = d.kG * (qq <= 0.5f ? qq * (3.0f * qq - 2.0f) : -f * f);   // dW/dr
                const float s = q.w * dw / r;
                gx += s * dx; gy += s * dy; gz += s * dz;
            }
        }
    const float len = __builtin_sqrtf(gx * gx + gy * gy + gz * gz);
    const float inv = len > 0.0f ? -1.0f / len : 0.0f;
    d.nrm[3 * (size_t)v] = gx * inv;
    d.nrm[3 * (size_t)v + 1] = gy * inv;
    d.nrm[3 * (size_t)v + 2] = gz * inv;
}
static void l_surf_normals(SurfDev &d, int nv) {
    if (nv > 0) hipLaunchKernelGGL(k_surf_normals, dim3(cdiv(nv, 256)), dim3(256), 0, d.stream, d, nv);
}

static void register_surface_launchers(Launch &L) {
    L.surf_compact = l_surf_compact;
    L.surf_bounds = l_surf_bounds;
    L.surf_bin = l_surf_bin;
    L.surf_flags = l_surf_flags;
    L.surf_field = l_surf_field;
    L.surf_count = l_surf_count;
    L.surf_emit = l_surf_emit;
    L.surf_normals = l_surf_normals;
}
