// sph_surface_aniso.hpp -- anisotropic kernels of the surface reconstruction (opt-in): kernels and launchers; included by sph_kernels.hip
// after sph_surface.hpp, inside the per-build namespace.  Method in DESIGN.md 29, semantics in include/sph_hip.h
// (sph_surface_set_anisotropy), float64 restatement in tests/surface_aniso_model.py.
//
// Passes, after the bin pass of sph_surface.hpp has left the key-ordered particles in xs (their isotropic V in w is not used here):
//   moments  per particle, over its 27 coarse cells in the bin pass's order: N_i, sum w, sum w d, sum w d d^T (d = x_k - x_i,
//            w = 1 - (|d| / h)^3) in float64, the covariance about the weighted mean rounded to f32, then surf_aniso_matrix in f32
//            -> A_i, det A_i
//   volume   V_j = 1 / sum_k det A_k W(|A_k (x_j - x_k)|), the same walk
//   field    k_surf_field with three staged records per particle: (xyz, V det A), (Axx, Axy, Axz, Ayy), (Ayz, Azz)
//   normals  k_surf_normals with grad w_j = det A_j W'(|y|) / |y| A_j y, y = A_j (x - x_j)
// Every a_k >= 1, so kernel j vanishes outside the ball of radius h around x_j: r2 < h2 stays the prefilter, and bins, bricks, count and
// emit are those of sph_surface.hpp.  No float atomics; every sum runs in the staging order.
#pragma once
#include "sph_surface_aniso_eig.hpp"

#define SURF_ANISO_CHUNK 512   // particles per LDS chunk of the anisotropic field pass: 40 B each, 20 KiB

// y = A d for the staged matrix (m = xx xy xz yy, yz / zz apart)
#define SURF_ANISO_MUL(m, yz, zz, dx, dy, dz, y0, y1, y2)             \
    const float y0 = (m).x * (dx) + (m).y * (dy) + (m).z * (dz);      \
    const float y1 = (m).y * (dx) + (m).w * (dy) + (yz) * (dz);       \
    const float y2 = (m).z * (dx) + (yz) * (dy) + (zz) * (dz)

__global__ void __launch_bounds__(256) k_surf_aniso_moments(SurfDev d, SurfAniso a) {
    __shared__ int s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < d.n) {
        const float4 p = d.xs[i];
        const int cx = surf_coord(d, p.x, 0), cy = surf_coord(d, p.y, 1), cz = surf_coord(d, p.z, 2);   // 1 .. cn - 2 (empty margin)
        // The moments are accumulated in float64 from the f32 positions (differences and products are then exact, the sums good to
        // 2^-53 N): C_i reaches the f32 eigen routine correctly rounded, whatever the neighbour count.
        int nb = 0;
        double sw = 0.0, mx = 0.0, my = 0.0, mz = 0.0, xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
        for (int ox = -1; ox <= 1; ++ox)
            for (int oy = -1; oy <= 1; ++oy) {
                const int b = d.cell_start[surf_lin(d, cx + ox, cy + oy, cz - 1)], e = d.cell_start[surf_lin(d, cx + ox, cy + oy, cz + 1) + 1];
                for (int k = b; k < e; ++k) {
                    const float4 q = d.xs[k];
                    const float fx = q.x - p.x, fy = q.y - p.y, fz = q.z - p.z;
                    if (!(fx * fx + fy * fy + fz * fz < d.h2)) continue;   // the f32 test of every other pass decides who is a neighbour
                    nb += k != i;
                    const double dx = (double)q.x - (double)p.x, dy = (double)q.y - (double)p.y, dz = (double)q.z - (double)p.z;
                    const double t = __builtin_sqrt(dx * dx + dy * dy + dz * dz) / a.h;
                    const double w = 1.0 - t * t * t;   // (the particle itself: d = 0, w = 1)
                    sw += w;
                    const double wx = w * dx, wy = w * dy, wz = w * dz;
                    mx += wx; my += wy; mz += wz;
                    xx += wx * dx; xy += wx * dy; xz += wx * dz; yy += wy * dy; yz += wy * dz; zz += wz * dz;
                }
            }
        // covariance about the weighted mean, from the moments about x_i
        const double ex = mx / sw, ey = my / sw, ez = mz / sw;
        const float C[6] = {(float)(xx / sw - ex * ex), (float)(xy / sw - ex * ey), (float)(xz / sw - ex * ez),
                            (float)(yy / sw - ey * ey), (float)(yz / sw - ey * ez), (float)(zz / sw - ez * ez)};
        float A[6], det;
        const int code = surf_aniso_matrix(C, nb, a.prm, A, &det);
        a.am[i] = make_float4(A[0], A[1], A[2], A[3]);
        a.an[i] = make_float4(A[4], A[5], det, __int_as_float(nb));
        if (code) atomicAdd(&s_cnt[code - 1], 1);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&a.cnt[threadIdx.x], s_cnt[threadIdx.x]);
}
static void l_surf_aniso_moments(SurfDev &d, SurfAniso &a) {
    hipMemsetAsync(a.cnt, 0, 2 * sizeof(int), d.stream);
    if (d.n > 0) hipLaunchKernelGGL(k_surf_aniso_moments, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d, a);
}

// V_j: k_surf_volume's walk with every neighbour's own kernel (A = I, det = 1 everywhere gives k_surf_volume's bits)
__global__ void __launch_bounds__(256) k_surf_aniso_volume(SurfDev d, SurfAniso a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const float4 p = d.xs[i];
    const int cx = surf_coord(d, p.x, 0), cy = surf_coord(d, p.y, 1), cz = surf_coord(d, p.z, 2);
    float sum = 0.0f;
    for (int ox = -1; ox <= 1; ++ox)
        for (int oy = -1; oy <= 1; ++oy) {
            const int b = d.cell_start[surf_lin(d, cx + ox, cy + oy, cz - 1)], e = d.cell_start[surf_lin(d, cx + ox, cy + oy, cz + 1) + 1];
            for (int k = b; k < e; ++k) {
                const float4 q = d.xs[k];
                const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
                const float r2 = dx * dx + dy * dy + dz * dz;
                if (!(r2 < d.h2)) continue;
                const float4 m = a.am[k], t = a.an[k];
                SURF_ANISO_MUL(m, t.x, t.y, dx, dy, dz, y0, y1, y2);
                sum += t.z * surf_w(d, y0 * y0 + y1 * y1 + y2 * y2);
            }
        }
    a.vol[i] = 1.0f / sum;   // (the particle's own term det A_i W(0) > 0)
}
static void l_surf_aniso_volume(SurfDev &d, SurfAniso &a) {
    if (d.n > 0) hipLaunchKernelGGL(k_surf_aniso_volume, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d, a);
}

// --- the field: k_surf_field's grid, points, staging order and pair count; see there ----------------------------------------------------
template <int PPT>
__global__ void __launch_bounds__(256) k_surf_field_aniso(SurfDev d, SurfAniso a) {
    __shared__ float4 s_x[SURF_ANISO_CHUNK];   // xyz, V det A
    __shared__ float4 s_m[SURF_ANISO_CHUNK];   // xx xy xz yy
    __shared__ float2 s_t[SURF_ANISO_CHUNK];   // yz zz
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
        for (int base = rb; base < re; base += SURF_ANISO_CHUNK) {
            const int cnt = min(SURF_ANISO_CHUNK, re - base);
            for (int k = threadIdx.x; k < cnt; k += 256) {
                const float4 q = d.xs[base + k], t = a.an[base + k];
                s_x[k] = make_float4(q.x, q.y, q.z, a.vol[base + k] * t.z);
                s_m[k] = a.am[base + k];
                s_t[k] = make_float2(t.x, t.y);
            }
            __syncthreads();
            for (int j = 0; j < cnt; ++j) {
                const float4 q = s_x[j], m = s_m[j];   // every lane reads the same words: LDS broadcasts
                const float2 t = s_t[j];
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const float dx = px[k] - q.x, dy = py[k] - q.y, dz = pz[k] - q.z;
                    const float r2 = dx * dx + dy * dy + dz * dz;
                    if (r2 < d.h2) {
                        SURF_ANISO_MUL(m, t.x, t.y, dx, dy, dz, y0, y1, y2);
                        acc[k] += q.w * surf_w(d, y0 * y0 + y1 * y1 + y2 * y2);   // (0 from |y| >= h on)
                    }
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
static void l_surf_field_aniso(SurfDev &d, SurfAniso &a) {
    hipLaunchKernelGGL(k_surf_bricks, dim3(cdiv(d.G, 256)), dim3(256), 0, d.stream, d);
    hipMemsetAsync(d.pairs, 0, sizeof(unsigned long long), d.stream);
    if (d.nb == 0) return;
    // points per thread as l_surf_field chooses them
    const int parts = cdiv(d.P, 256 * 12);
    const int need = cdiv(d.P, 256 * parts);
    if (need <= 4) hipLaunchKernelGGL(k_surf_field_aniso<4>, dim3(d.nb, cdiv(d.P, 1024)), dim3(256), 0, d.stream, d, a);
    else if (need <= 8) hipLaunchKernelGGL(k_surf_field_aniso<8>, dim3(d.nb, cdiv(d.P, 2048)), dim3(256), 0, d.stream, d, a);
    else hipLaunchKernelGGL(k_surf_field_aniso<12>, dim3(d.nb, parts), dim3(256), 0, d.stream, d, a);
}

// --- normals -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_surf_normals_aniso(SurfDev d, SurfAniso a, int nv) {
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
                if (!(r2 < d.h2)) continue;
                const float4 m = a.am[k], t = a.an[k];
                SURF_ANISO_MUL(m, t.x, t.y, dx, dy, dz, y0, y1, y2);
                const float s2 = y0 * y0 + y1 * y1 + y2 * y2;
                if (s2 <= 0.0f) continue;
                const float r = __builtin_sqrtf(s2);
#if SPH_FAST
                const float qq = r * (1.0f / d.h);
#else
                const float qq = r / d.h;
#endif
                if (!(qq < 1.0f)) continue;   // outside the shrunk support
                const float f = 1.0f - qq;
                const float dw = d.kG * (qq <= 0.5f ? qq * (3.0f * qq - 2.0f) : -f * f);   // dW/dr at |y|
                const float s = a.vol[k] * t.z * dw / r;
                SURF_ANISO_MUL(m, t.x, t.y, y0, y1, y2, g0, g1, g2);   // A y = A^2 d
                gx += s * g0; gy += s * g1; gz += s * g2;
            }
        }
    const float len = __builtin_sqrtf(gx * gx + gy * gy + gz * gz);
    const float inv = len > 0.0f ? -1.0f / len : 0.0f;
    d.nrm[3 * (size_t)v] = gx * inv;
    d.nrm[3 * (size_t)v + 1] = gy * inv;
    d.nrm[3 * (size_t)v + 2] = gz * inv;
}
static void l_surf_normals_aniso(SurfDev &d, SurfAniso &a, int nv) {
    if (nv > 0) hipLaunchKernelGGL(k_surf_normals_aniso, dim3(cdiv(nv, 256)), dim3(256), 0, d.stream, d, a, nv);
}

static void register_surface_aniso_launchers(Launch &L) {
    L.surf_aniso_moments = l_surf_aniso_moments;
    L.surf_aniso_volume = l_surf_aniso_volume;
    L.surf_field_aniso = l_surf_field_aniso;
    L.surf_normals_aniso = l_surf_normals_aniso;
}
