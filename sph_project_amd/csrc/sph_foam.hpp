// sph_foam.hpp -- diffuse particles (spray, foam, bubbles) generated from the fluid state: kernels and launchers; included by
// sph_kernels.hip inside the per-build namespace.  Method in DESIGN.md 26, semantics in include/sph_hip.h (sph_foam_create), float64
// restatement in tests/foam_model.py.
//
// Passes of one step (one stream; the host reads the counters once, at the end):
//   grid        cell per fluid particle (edge h), histogram, scan, scatter, then a rank inside each cell by particle id: the binned order
//               is a function of the particle SET, so every sum below runs in an order that the input order cannot change
//   advect      one lane per diffuse particle: N and v_f over the 27 cells (9 runs of 3 z-cells), class, motion, survivor flag; scan;
//               survivors compacted into the other bank in their old order
//   normals     one lane per fluid particle in grid order: g_i, n_i
//   potentials  one lane per fluid particle: ta, wc, e, n_d, child count
//   generate    scan of the counts; children written behind the survivors in (grid order, child) order; counters
// The walks are the plain per-particle walks of sph_pbf.hpp / sph_contact.hpp (no LDS staging).  No float atomics: the only atomics count.
#pragma once

__device__ __forceinline__ int foam_coord(const FoamDev &d, float x, int a) {
    // border cell 0 below the domain, cn - 1 above it; NaN files into cell 0 (fmaxf drops it)
    const float c = floorf((x - d.glo[a]) / d.h) + 1.0f;
    return (int)fminf(fmaxf(c, 0.0f), (float)(d.cn[a] - 1));
}
__device__ __forceinline__ int foam_lin(const FoamDev &d, int x, int y, int z) { return (x * d.cn[1] + y) * d.cn[2] + z; }
__device__ __forceinline__ int foam_cell_of(const FoamDev &d, float4 p) {
    return foam_lin(d, foam_coord(d, p.x, 0), foam_coord(d, p.y, 1), foam_coord(d, p.z, 2));
}

// f(k) for every grid-order index k of the 27 cells around p (cells outside the grid do not exist)
template <class F> __device__ __forceinline__ void foam_walk(const FoamDev &d, float4 p, F &&f) {
    const int cx = foam_coord(d, p.x, 0), cy = foam_coord(d, p.y, 1), cz = foam_coord(d, p.z, 2);
    const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz < d.cn[2] - 1 ? cz + 1 : d.cn[2] - 1;
    for (int ox = -1; ox <= 1; ++ox) {
        const int x = cx + ox;
        if (x < 0 || x >= d.cn[0]) continue;
        for (int oy = -1; oy <= 1; ++oy) {
            const int y = cy + oy;
            if (y < 0 || y >= d.cn[1]) continue;
            const int b = d.cell_start[foam_lin(d, x, y, z0)], e = d.cell_start[foam_lin(d, x, y, z1) + 1];
            for (int k = b; k < e; ++k) f(k);
        }
    }
}

// one add per wave to counter word w
__device__ __forceinline__ void foam_count(const FoamDev &d, int w, unsigned v) {
    unsigned long long s = v;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&d.ctr[w], s);
}

// --- the random numbers: a counter-based integer hash of (seed, id, foam step, child, stream); tests/foam_model.py restates it bit for bit
__device__ __forceinline__ unsigned foam_mix(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float foam_rand(const FoamDev &d, unsigned id, unsigned k, unsigned stream) {
    unsigned h = foam_mix(d.seed_lo ^ 0x9e3779b9u);
    h = foam_mix(h ^ d.seed_hi);
    h = foam_mix(h ^ id);
    h = foam_mix(h ^ d.t);
    h = foam_mix(h ^ k);
    h = foam_mix(h ^ stream);
    return (float)(h >> 8) * 5.9604644775390625e-8f;   // top 24 bits * 2^-24: [0, 1)
}

// --- input from a handle: the active fluid particles in the handle's order -------------------------------------------------------------
__global__ void __launch_bounds__(256) k_foam_flag(const int *meta, int n_all, int *flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_all) return;
    const int m = meta[i];
    flag[i] = (META_ACTIVE_FLUID(m) && !META_DEAD(m)) ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_foam_take(FoamDev d, const float4 *posv, const float4 *velm, const int *pid, int n_all, const int *flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_all) return;
    const int j = flag[i];
    if (flag[i + 1] == j) return;
    const float4 p = posv[i], v = velm[i];
    d.xin[j] = make_float4(p.x, p.y, p.z, 0.0f);
    d.vin[j] = make_float4(v.x, v.y, v.z, 0.0f);
    d.idin[j] = pid[i];
}
static void foam_scan(FoamDev &d, int *a, int n) {
    const int tiles = cdiv(n > 0 ? n : 1, 1024);
    hipLaunchKernelGGL(k_surf_scan_tile, dim3(tiles), dim3(256), 0, d.stream, a, n, d.scan_tmp);
    hipLaunchKernelGGL(k_surf_scan_top, dim3(1), dim3(256), 0, d.stream, d.scan_tmp, tiles, a, n);
    hipLaunchKernelGGL(k_surf_scan_add, dim3(tiles), dim3(256), 0, d.stream, a, n, (const int *)d.scan_tmp);
}
static void l_foam_compact(FoamDev &d, const float4 *posv, const float4 *velm, const int *pid, const int *meta, int n_all, int *flag) {
    if (n_all <= 0) { hipMemsetAsync(flag, 0, sizeof(int), d.stream); return; }
    const int g = cdiv(n_all, 256);
    hipLaunchKernelGGL(k_foam_flag, dim3(g), dim3(256), 0, d.stream, meta, n_all, flag);
    foam_scan(d, flag, n_all);
    hipLaunchKernelGGL(k_foam_take, dim3(g), dim3(256), 0, d.stream, d, posv, velm, pid, n_all, (const int *)flag);
}

// --- grid ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_foam_hist(FoamDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const int c = foam_cell_of(d, d.xin[i]);
    d.pcell[i] = c;
    d.pslot[i] = atomicAdd(&d.cell_start[c], 1);
}
__global__ void __launch_bounds__(256) k_foam_scatter(FoamDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const int j = d.cell_start[d.pcell[i]] + d.pslot[i];
    d.xt[j] = d.xin[i]; d.vt[j] = d.vin[i]; d.idt[j] = d.idin[i]; d.srct[j] = i;
}
// id order inside a cell; equal ids (a caller's mistake) by the bits of the position, then by arrival
__global__ void __launch_bounds__(256) k_foam_rank(FoamDev d) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d.n) return;
    const float4 p = d.xt[j];
    const int c = foam_cell_of(d, p);
    const int b = d.cell_start[c], e = d.cell_start[c + 1];
    const unsigned id = (unsigned)d.idt[j], kx = __float_as_uint(p.x), ky = __float_as_uint(p.y), kz = __float_as_uint(p.z);
    int rank = 0;
    for (int k = b; k < e; ++k) {
        const unsigned qi = (unsigned)d.idt[k];
        bool less;
        if (qi != id) less = qi < id;
        else {
            const float4 q = d.xt[k];
            const unsigned qx = __float_as_uint(q.x), qy = __float_as_uint(q.y), qz = __float_as_uint(q.z);
            less = qx != kx ? qx < kx : qy != ky ? qy < ky : qz != kz ? qz < kz : k < j;
        }
        rank += less;
    }
    const int o = b + rank;
    d.xs[o] = p; d.vs[o] = d.vt[j]; d.ids[o] = (int)id; d.src[o] = d.srct[j];
}
static void l_foam_grid(FoamDev &d) {
    hipMemsetAsync(d.cell_start, 0, sizeof(int) * ((size_t)d.G + 1), d.stream);
    if (d.n == 0) return;   // (the scan of zeros is zeros)
    const int g = cdiv(d.n, 256);
    hipLaunchKernelGGL(k_foam_hist, dim3(g), dim3(256), 0, d.stream, d);
    foam_scan(d, d.cell_start, d.G);
    hipLaunchKernelGGL(k_foam_scatter, dim3(g), dim3(256), 0, d.stream, d);
    hipLaunchKernelGGL(k_foam_rank, dim3(g), dim3(256), 0, d.stream, d);
}

// --- advection of the existing diffuse particles -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_foam_advect(FoamDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < d.nd;
    unsigned visited = 0, accepted = 0;
    int cls = -1, kept = 0;
    if (on) {
        float4 p = d.dx[0][i], v = d.dv[0][i];
        int N = 0;
        float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
        foam_walk(d, p, [&](int k) {
            const float4 q = d.xs[k];
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float r = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
            ++visited;
            if (r < d.h) {
                const float4 u = d.vs[k];
                const float w = 1.0f - r / d.h;
                ++N; ++accepted;
                sw += w; sx += w * u.x; sy += w * u.y; sz += w * u.z;
            }
        });
        const float fx = sw > 0.0f ? sx / sw : v.x, fy = sw > 0.0f ? sy / sw : v.y, fz = sw > 0.0f ? sz / sw : v.z;
        if (N < d.n_spray) {
            cls = 0;
            v.x += d.dt * d.g[0]; v.y += d.dt * d.g[1]; v.z += d.dt * d.g[2];
        } else if (N <= d.n_bubble) {
            cls = 1;
            v.x = fx; v.y = fy; v.z = fz;
            p.w -= d.dt;
        } else {
            cls = 2;
            v.x += -d.k_b * d.dt * d.g[0] + d.k_d * (fx - v.x);
            v.y += -d.k_b * d.dt * d.g[1] + d.k_d * (fy - v.y);
            v.z += -d.k_b * d.dt * d.g[2] + d.k_d * (fz - v.z);
        }
        p.x += d.dt * v.x; p.y += d.dt * v.y; p.z += d.dt * v.z;
        kept = (p.w > 0.0f && p.x >= d.lo[0] && p.x <= d.hi[0] && p.y >= d.lo[1] && p.y <= d.hi[1] && p.z >= d.lo[2] && p.z <= d.hi[2]) ? 1 : 0;
        v.w = __int_as_float(cls);
        d.dx[0][i] = p; d.dv[0][i] = v;
        d.keep[i] = kept;
    }
    foam_count(d, FC_VISIT + 0, visited);
    foam_count(d, FC_ACCEPT + 0, accepted);
    foam_count(d, FC_CLASS + 0, kept && cls == 0);
    foam_count(d, FC_CLASS + 1, kept && cls == 1);
    foam_count(d, FC_CLASS + 2, kept && cls == 2);
    foam_count(d, FC_DIED, on && !kept);
}
__global__ void __launch_bounds__(256) k_foam_survivors(FoamDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.nd) return;
    const int j = d.keep[i];
    if (d.keep[i + 1] == j) return;
    d.dx[1][j] = d.dx[0][i]; d.dv[1][j] = d.dv[0][i]; d.dkey[1][j] = d.dkey[0][i];
}
// leaves the survivors in bank 1 and keep[nd] = their number
static void l_foam_advect(FoamDev &d) {
    if (d.nd == 0) { hipMemsetAsync(d.keep, 0, sizeof(int), d.stream); return; }
    const int g = cdiv(d.nd, 256);
    hipLaunchKernelGGL(k_foam_advect, dim3(g), dim3(256), 0, d.stream, d);
    foam_scan(d, d.keep, d.nd);
    hipLaunchKernelGGL(k_foam_survivors, dim3(g), dim3(256), 0, d.stream, d);
}

// --- normals -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_foam_normals(FoamDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned visited = 0, accepted = 0;
    if (i < d.n) {
        const float4 p = d.xs[i];
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        foam_walk(d, p, [&](int k) {
            const float4 q = d.xs[k];
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float r = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
            ++visited;
            if (k != i && r < d.h) {
                const float w = 1.0f - r / d.h;
                ++accepted;
                gx += dx * w; gy += dy * w; gz += dz * w;
            }
        });
        const float gl = __builtin_sqrtf(gx * gx + gy * gy + gz * gz);
        d.nrm[i] = gl >= d.nmin_h ? make_float4(gx / gl, gy / gl, gz / gl, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    foam_count(d, FC_VISIT + 1, visited);
    foam_count(d, FC_ACCEPT + 1, accepted);
}
static void l_foam_normals(FoamDev &d) {
    if (d.n > 0) hipLaunchKernelGGL(k_foam_normals, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d);
}

// --- potentials and child counts -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float foam_phi(float I, float lo, float hi) { return (fminf(I, hi) - fminf(I, lo)) / (hi - lo); }

__global__ void __launch_bounds__(256) k_foam_potentials(FoamDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned visited = 0, accepted = 0;
    if (i < d.n) {
        const float4 p = d.xs[i], v = d.vs[i], ni = d.nrm[i];
        float ta = 0.0f, wc = 0.0f;
        foam_walk(d, p, [&](int k) {
            const float4 q = d.xs[k];
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float r = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
            ++visited;
            if (k != i && r < d.h) {
                const float4 u = d.vs[k];
                const float w = 1.0f - r / d.h;
                ++accepted;
                const float ux = v.x - u.x, uy = v.y - u.y, uz = v.z - u.z;
                const float um = __builtin_sqrtf(ux * ux + uy * uy + uz * uz);
                if (um >= 1e-6f && r >= 1e-6f) ta += um * (1.0f - (ux * dx + uy * dy + uz * dz) / (um * r)) * w;
                if (ni.w != 0.0f && r >= 1e-6f) {
                    const float4 nj = d.nrm[k];
                    // xhat_ji . n_i < 0: j lies behind i's outward normal
                    if (nj.w != 0.0f && -(dx * ni.x + dy * ni.y + dz * ni.z) / r < 0.0f)
                        wc += (1.0f - (ni.x * nj.x + ni.y * nj.y + ni.z * nj.z)) * w;
                }
            }
        });
        const float v2 = v.x * v.x + v.y * v.y + v.z * v.z, vm = __builtin_sqrtf(v2);
        if (!(ni.w != 0.0f && vm >= 1e-6f && (v.x * ni.x + v.y * ni.y + v.z * ni.z) / vm >= 0.6f)) wc = 0.0f;
        const float e = 0.5f * v2;
        const float nd = foam_phi(e, d.e_lo, d.e_hi) * (d.k_ta * foam_phi(ta, d.ta_lo, d.ta_hi) + d.k_wc * foam_phi(wc, d.wc_lo, d.wc_hi)) * d.dt;
        d.pot[i] = make_float4(ta, wc, e, nd);
        const float c = floorf(nd + foam_rand(d, (unsigned)d.ids[i], 0u, 0u));
        d.cnt[i] = (int)fminf(fmaxf(c, 0.0f), (float)d.max_pp);   // (NaN: none)
    }
    foam_count(d, FC_VISIT + 2, visited);
    foam_count(d, FC_ACCEPT + 2, accepted);
}
static void l_foam_potentials(FoamDev &d) {
    if (d.n > 0) hipLaunchKernelGGL(k_foam_potentials, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d);
    else hipMemsetAsync(d.cnt, 0, sizeof(int), d.stream);
}

// --- generation ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_foam_emit(FoamDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const int b = d.cnt[i], nc = d.cnt[i + 1] - b;
    if (nc <= 0) return;
    const int base = d.keep[d.nd] + b;   // behind the survivors
    if (base >= d.cap) return;
    const float4 p = d.xs[i], v = d.vs[i];
    const unsigned id = (unsigned)d.ids[i];
    const float vm = __builtin_sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    float hx = 1.0f, hy = 0.0f, hz = 0.0f;
    if (vm >= 1e-6f) { hx = v.x / vm; hy = v.y / vm; hz = v.z / vm; }
    // e1 = (vhat x a) / |vhat x a| with a = y where vhat is near x, else x; e2 = vhat x e1
    float ax = 1.0f, ay = 0.0f;
    if (fabsf(hx) > 0.9f) { ax = 0.0f; ay = 1.0f; }
    float e1x = -hz * ay, e1y = hz * ax, e1z = hx * ay - hy * ax;   // (a.z = 0)
    const float el = __builtin_sqrtf(e1x * e1x + e1y * e1y + e1z * e1z);
    e1x /= el; e1y /= el; e1z /= el;
    const float e2x = hy * e1z - hz * e1y, e2y = hz * e1x - hx * e1z, e2z = hx * e1y - hy * e1x;
    for (int k = 0; k < nc && base + k < d.cap; ++k) {
        const float r = d.pr * __builtin_sqrtf(foam_rand(d, id, (unsigned)k, 1u));
        const float th = 6.2831853071795864769f * foam_rand(d, id, (unsigned)k, 2u);
        const float s = foam_rand(d, id, (unsigned)k, 3u) * vm * d.dt;
        const float life = d.life_lo + foam_rand(d, id, (unsigned)k, 4u) * (d.life_hi - d.life_lo);
        const float c = r * cosf(th), sn = r * sinf(th);
        const float ox = c * e1x + sn * e2x, oy = c * e1y + sn * e2y, oz = c * e1z + sn * e2z;
        d.dx[1][base + k] = make_float4(p.x + ox + s * hx, p.y + oy + s * hy, p.z + oz + s * hz, life);
        d.dv[1][base + k] = make_float4(v.x + ox, v.y + oy, v.z + oz, __int_as_float(3));
        d.dkey[1][base + k] = (unsigned long long)(d.t & 0x7fffffu) << 40 | (unsigned long long)id << 8 | (unsigned long long)k;
    }
}
__global__ void k_foam_finish(FoamDev d) {
    const long long surv = d.keep[d.nd], total = d.cnt[d.n];
    const long long room = (long long)d.cap - surv;
    const long long born = total < room ? total : room;
    d.ctr[FC_BORN] = (unsigned long long)born;
    d.ctr[FC_DROPPED] = (unsigned long long)(total - born);
    d.ctr[FC_COUNT] = (unsigned long long)(surv + born);
}
static void l_foam_generate(FoamDev &d) {
    if (d.n > 0) {
        foam_scan(d, d.cnt, d.n);
        hipLaunchKernelGGL(k_foam_emit, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d);
    }
    hipLaunchKernelGGL(k_foam_finish, dim3(1), dim3(1), 0, d.stream, d);
}

// --- the renderer's source (sph_render_set_foam): id 0x80000000 | 31 bits of a hash of the key, colour by class ------------------------------
__global__ void __launch_bounds__(256) k_foam_render_source(const unsigned long long *key, const float4 *dv, int n, int *id, unsigned *col,
                                                            unsigned c0, unsigned c1, unsigned c2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    const unsigned hsh = foam_mix(foam_mix((unsigned)k ^ 0x9e3779b9u) ^ (unsigned)(k >> 32));
    unsigned v = 0x80000000u | (hsh & 0x7fffffffu);
    if (v >= 0xFFFFFFE0u) v -= 32u;   // (the top 16 ids are the box lines', -2 .. -17 in the id image: diffuse ids lie below -17 there)
    id[i] = (int)v;
    const int cls = __float_as_int(dv[i].w);
    col[i] = cls == 0 ? c0 : cls == 2 ? c2 : c1;   // (born this step: drawn as foam)
}
static void l_foam_render_source(const FoamDev &d, int n, int *id, unsigned *col, const unsigned rgb[3]) {
    if (n > 0) hipLaunchKernelGGL(k_foam_render_source, dim3(cdiv(n, 256)), dim3(256), 0, d.stream, (const unsigned long long *)d.dkey[0],
                                  (const float4 *)d.dv[0], n, id, col, rgb[0], rgb[1], rgb[2]);
}

static void register_foam_launchers(Launch &L) {
    L.foam_compact = l_foam_compact;
    L.foam_grid = l_foam_grid;
    L.foam_advect = l_foam_advect;
    L.foam_normals = l_foam_normals;
    L.foam_potentials = l_foam_potentials;
    L.foam_generate = l_foam_generate;
    L.foam_render_source = l_foam_render_source;
}
