// sph_surface_post.hpp -- post-processing of a reconstructed surface (vertex adjacency, smoothing weights, Laplacian smoothing, normal
// smoothing): kernels and launchers; included by sph_kernels.hip inside the per-build namespace after sph_surface.hpp.  Method in
// DESIGN.md 16, float32 restatement in tests/surface_post_model.py, host sequence in sph_surface_api.hpp (surf_post).
//
// Passes (one stream, one host read: the adjacency total and the largest degree):
//   adjacency  2 slots per triangle corner (integer atomics), scan, fill, then per vertex: sort its slots, drop duplicates and itself,
//              scan the unique counts, compact -> CSR (off, adj).  Neighbours ascending, so the result is free of the atomics' order.
//   weights    c_j = sum_{k != j, r < h} (1 - r^2 / h^2) per particle over the 27 coarse cells in the binned order; per vertex
//              w_i = min(1, max_{r < h} c_j / normalization).  The max is order-free.
//   smoothing  Jacobi on a float4 copy of the vertices, ping-pong: P' = (1 - w) P + w (sum_{j ascending} P_j) / deg
//   normals    n' = s / |s|, s = n_i + sum_{j ascending} n_j (a zero sum stays as it is)
// No float atomics; every float sum runs in a fixed order.
#pragma once

// --- adjacency -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_post_adj_count(SurfPost p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.nt) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&p.raw[p.tri[3 * (size_t)t + k]], 2);
}
__global__ void __launch_bounds__(256) k_post_adj_fill(SurfPost p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.nt) return;
    const int v[3] = {p.tri[3 * (size_t)t], p.tri[3 * (size_t)t + 1], p.tri[3 * (size_t)t + 2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int at = p.raw[v[k]] + atomicAdd(&p.cnt[v[k]], 2);   // slot order is irrelevant: the next pass sorts
        p.slot[at] = v[(k + 1) % 3];
        p.slot[at + 1] = v[(k + 2) % 3];
    }
}
// insertion sort of the vertex's slots in place (any length: a high degree is slow, not wrong), then unique values != the vertex itself
// to the front of its range; cnt[i] = their number
__global__ void __launch_bounds__(256) k_post_adj_sort(SurfPost p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.nv) return;
    int *s = p.slot;
    const int b = p.raw[i], e = p.raw[i + 1];
    for (int k = b + 1; k < e; ++k) {
        const int x = s[k];
        int m = k - 1;
        while (m >= b && s[m] > x) { s[m + 1] = s[m]; --m; }
        s[m + 1] = x;
    }
    int u = 0, last = -1;
    for (int k = b; k < e; ++k) {
        const int x = s[k];
        if (x != last && x != i) s[b + u++] = x;   // (b + u <= k: never ahead of the read)
        last = x;
    }
    p.cnt[i] = u;
    atomicMax(p.maxdeg, u);
}
__global__ void __launch_bounds__(256) k_post_adj_compact(SurfPost p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.nv) return;
    const int b = p.raw[i], o = p.cnt[i], u = p.cnt[i + 1] - o;
    for (int k = 0; k < u; ++k) p.adj[o + k] = p.slot[b + k];
}
// up to the scanned unique counts (the host reads the total and allocates adj in between)
static void l_surf_post_adjacency(SurfDev &d, SurfPost &p) {
    hipMemsetAsync(p.raw, 0, sizeof(int) * ((size_t)p.nv + 1), d.stream);
    hipMemsetAsync(p.cnt, 0, sizeof(int) * ((size_t)p.nv + 1), d.stream);
    hipMemsetAsync(p.maxdeg, 0, sizeof(int), d.stream);
    if (p.nt > 0) hipLaunchKernelGGL(k_post_adj_count, dim3(cdiv(p.nt, 256)), dim3(256), 0, d.stream, p);
    surf_scan(d, p.raw, p.nv);
    if (p.nt > 0) hipLaunchKernelGGL(k_post_adj_fill, dim3(cdiv(p.nt, 256)), dim3(256), 0, d.stream, p);
    if (p.nv > 0) hipLaunchKernelGGL(k_post_adj_sort, dim3(cdiv(p.nv, 256)), dim3(256), 0, d.stream, p);
    surf_scan(d, p.cnt, p.nv);
}
static void l_surf_post_compact(SurfDev &d, SurfPost &p) {
    if (p.nv > 0) hipLaunchKernelGGL(k_post_adj_compact, dim3(cdiv(p.nv, 256)), dim3(256), 0, d.stream, p);
}

// --- smoothing weights -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float post_wterm(const SurfDev &d, float r2) {
#if SPH_FAST
    return 1.0f - r2 * (1.0f / d.h2);
#else
    return 1.0f - r2 / d.h2;
#endif
}
// c_j over the 9 runs of 3 z-cells, as k_surf_volume walks them (binned particles lie 1 .. cn - 2: the grid keeps an empty margin)
__global__ void __launch_bounds__(256) k_post_pcount(SurfDev d, SurfPost p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const float4 q0 = d.xs[i];
    const int cx = surf_coord(d, q0.x, 0), cy = surf_coord(d, q0.y, 1), cz = surf_coord(d, q0.z, 2);
    float c = 0.0f;
    for (int ox = -1; ox <= 1; ++ox)
        for (int oy = -1; oy <= 1; ++oy) {
            const int b = d.cell_start[surf_lin(d, cx + ox, cy + oy, cz - 1)], e = d.cell_start[surf_lin(d, cx + ox, cy + oy, cz + 1) + 1];
            for (int k = b; k < e; ++k) {
                const float4 q = d.xs[k];
                const float dx = q0.x - q.x, dy = q0.y - q.y, dz = q0.z - q.z;
                const float r2 = dx * dx + dy * dy + dz * dz;
                if (k != i && r2 < d.h2) c += post_wterm(d, r2);
            }
        }
    p.pc[i] = c;
}
// w_i = min(1, max c_j / normalization) over the particles within h of the (unsmoothed) vertex, 0 when there are none
__global__ void __launch_bounds__(256) k_post_vweight(SurfDev d, SurfPost p) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= p.nv) return;
    const float x = d.vert[3 * (size_t)v], y = d.vert[3 * (size_t)v + 1], z = d.vert[3 * (size_t)v + 2];
    const int cx = surf_coord(d, x, 0), cy = surf_coord(d, y, 1), cz = surf_coord(d, z, 2);
    float m = 0.0f;
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
                if (r2 < d.h2) m = fmaxf(m, p.pc[k]);
            }
        }
#if SPH_FAST
    p.w[v] = fminf(1.0f, m * (1.0f / p.norm));
#else
    p.w[v] = fminf(1.0f, m / p.norm);
#endif
}
static void l_surf_post_weights(SurfDev &d, SurfPost &p) {
    if (d.n > 0) hipLaunchKernelGGL(k_post_pcount, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d, p);
    if (p.nv > 0) hipLaunchKernelGGL(k_post_vweight, dim3(cdiv(p.nv, 256)), dim3(256), 0, d.stream, d, p);
}

// --- f32[3] <-> float4 working copies ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_post_to4(const float *src, float4 *dst, int nv) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < nv) dst[v] = make_float4(src[3 * (size_t)v], src[3 * (size_t)v + 1], src[3 * (size_t)v + 2], 0.0f);
}
__global__ void __launch_bounds__(256) k_post_from4(const float4 *src, float *dst, int nv) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const float4 q = src[v];
    dst[3 * (size_t)v] = q.x; dst[3 * (size_t)v + 1] = q.y; dst[3 * (size_t)v + 2] = q.z;
}

// --- Laplacian smoothing: one Jacobi iteration src -> dst ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_post_smooth(const int *__restrict__ off, const int *__restrict__ adj, const float *__restrict__ w,
                                                     const float4 *__restrict__ src, float4 *__restrict__ dst, int nv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int b = off[i], e = off[i + 1];
    const float4 q = src[i];
    if (e == b) { dst[i] = q; return; }   // no neighbour: the vertex stays
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int k = b; k < e; ++k) {
        const float4 r = src[adj[k]];
        sx += r.x; sy += r.y; sz += r.z;
    }
    const float deg = (float)(e - b);
#if SPH_FAST
    const float inv = 1.0f / deg;
    const float mx = sx * inv, my = sy * inv, mz = sz * inv;
#else
    const float mx = sx / deg, my = sy / deg, mz = sz / deg;
#endif
    const float wi = w ? w[i] : 1.0f, wo = 1.0f - wi;
    dst[i] = make_float4(wo * q.x + wi * mx, wo * q.y + wi * my, wo * q.z + wi * mz, 0.0f);
}

// --- normal smoothing: one iteration src -> dst ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_post_nsmooth(const int *__restrict__ off, const int *__restrict__ adj, const float4 *__restrict__ src,
                                                      float4 *__restrict__ dst, int nv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int b = off[i], e = off[i + 1];
    const float4 q = src[i];
    float sx = q.x, sy = q.y, sz = q.z;
    for (int k = b; k < e; ++k) {
        const float4 r = src[adj[k]];
        sx += r.x; sy += r.y; sz += r.z;
    }
    const float len = __builtin_sqrtf(sx * sx + sy * sy + sz * sz);
    if (len > 0.0f) {
#if SPH_FAST
        const float inv = 1.0f / len;
        sx *= inv; sy *= inv; sz *= inv;
#else
        sx /= len; sy /= len; sz /= len;
#endif
    }
    dst[i] = make_float4(sx, sy, sz, 0.0f);
}

// K Jacobi iterations of the positions; the result goes back into d.vert
static void l_surf_post_smooth(SurfDev &d, SurfPost &p, int iters) {
    if (p.nv == 0 || iters <= 0) return;
    const dim3 g(cdiv(p.nv, 256));
    const int *off = p.cnt;
    hipLaunchKernelGGL(k_post_to4, g, dim3(256), 0, d.stream, (const float *)d.vert, p.a, p.nv);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(k_post_smooth, g, dim3(256), 0, d.stream, off, (const int *)p.adj, (const float *)p.w, (const float4 *)p.a, p.b, p.nv);
        float4 *t = p.a; p.a = p.b; p.b = t;
    }
    hipLaunchKernelGGL(k_post_from4, g, dim3(256), 0, d.stream, (const float4 *)p.a, d.vert, p.nv);
}
// L iterations of the normals; the result goes back into d.nrm
static void l_surf_post_nsmooth(SurfDev &d, SurfPost &p, int iters) {
    if (p.nv == 0 || iters <= 0) return;
    const dim3 g(cdiv(p.nv, 256));
    hipLaunchKernelGGL(k_post_to4, g, dim3(256), 0, d.stream, (const float *)d.nrm, p.a, p.nv);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(k_post_nsmooth, g, dim3(256), 0, d.stream, (const int *)p.cnt, (const int *)p.adj, (const float4 *)p.a, p.b, p.nv);
        float4 *t = p.a; p.a = p.b; p.b = t;
    }
    hipLaunchKernelGGL(k_post_from4, g, dim3(256), 0, d.stream, (const float4 *)p.a, d.nrm, p.nv);
}

static void register_surface_post_launchers(Launch &L) {
    L.surf_post_adjacency = l_surf_post_adjacency;
    L.surf_post_compact = l_surf_post_compact;
    L.surf_post_weights = l_surf_post_weights;
    L.surf_post_smooth = l_surf_post_smooth;
    L.surf_post_nsmooth = l_surf_post_nsmooth;
}
