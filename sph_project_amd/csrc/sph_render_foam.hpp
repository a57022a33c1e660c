// sph_render_foam.hpp -- diffuse particles in the surface frames (white water over and under the surface): kernels and launchers; included
// by sph_kernels.hip inside the per-build namespace, behind sph_render_thickness.hpp whose splat sequence, counter banks and composite it
// restates.  The image is defined in DESIGN.md 28, semantics in include/sph_hip.h (sph_render_set_surface_foam), numpy restatement in
// tests/render_foam_model.py.  No k_render_*, k_rsurf_*, k_rthick_* or k_foam_* kernel is touched: everything here is a sibling.
//
// Passes (the renderer's stream, no host read in between):
//   splat   diffuse spheres only (radius rf): per covered pixel centre the chord [t0, t1] of the ray, its far end cut at the pixel's limit
//           L -- the frame's own depth in the opaque surface mode, the opaque layer's in thickness mode -- as an integer in units of u, added
//           with an integer atomicAdd to the plane `fo` (over the surface) or, thickness mode, on a surface pixel, behind t_w + bias, to
//           `fu` (under it), whose nearest start below the surface goes to `du` with an integer atomicMin.  No float is ever added: the
//           three planes are functions of the particle SETS.  The float sequence is rthick_pixel's, contraction off, IEEE / and sqrt.
//   under   thickness mode, surface pixels with fu > 0: k_rthick_shade restated with the fluid column split at du and the foam between.
//   over    every pixel with fo > 0: the bytes the pixel holds mixed with the foam colour by I(fo).
// The splat runs with the frame (sph_render_handle), while the diffuse set is the one that was drawn; under and over in sph_render_surface,
// behind its shade.
#pragma once

#define RFOAM_OVER 1u
#define RFOAM_UNDER 2u
#define RFOAM_CUT 4u
#define RFOAM_REMOVED 8u

__device__ __forceinline__ unsigned long long *rfoam_bank(const RenderFoamDev &f, int group, unsigned block) {
    return f.cnt + 8u * ((unsigned)group * RSURF_CNT_BANKS + (block & (RSURF_CNT_BANKS - 1)));
}

// one pixel of one diffuse sphere (d: the frame's RenderDev with r / r2 those of the diffuse spheres).  Returns the pair's flags:
// RFOAM_OVER / RFOAM_UNDER an add was issued to that plane, RFOAM_CUT ... of a chord the limit cut short, RFOAM_REMOVED the limit removed it
__device__ __forceinline__ unsigned rfoam_pixel(const RenderDev &d, const RenderSurfDev &s, const RenderFoamDev &f, const RenderView &v, int i,
                                                int j) {
#pragma clang fp contract(off)
    const float X = ((float)(2 * i + 1) / (float)d.W - 1.0f) * d.tx;
    const float Y = (1.0f - (float)(2 * j + 1) / (float)d.H) * d.ty;
    const float dd = (X * X + Y * Y) + 1.0f;
    const float k = ((X * v.xs + Y * v.ys) + v.z) / dd;
    const float wx = v.xs - k * X, wy = v.ys - k * Y, wz = v.z - k;
    const float h = d.r2 - ((wx * wx + wy * wy) + wz * wz);
    if (!(h >= 0.0f)) return 0u;
    const float root = sqrtf(h / dd);
    const float t0 = k - root, t1 = k + root;
    if (!(t0 > d.zn)) return 0u;
    const size_t p = (size_t)j * d.W + i;
    const unsigned long long kw = f.key0[p];
    const unsigned long long kl = f.okey ? f.okey[p] : kw;
    float b = t1;
    bool cut = false;
    if (kl != ~0ull) {
        const float top = __uint_as_float((unsigned)(kl >> 32));
        if (top < t1) { b = top; cut = true; }
    }
    if (!(b > t0)) return RFOAM_REMOVED;
    const unsigned c = (unsigned)((b - t0) * s.inv_u);
    if (f.okey && (s.base[p] & RSURF_FLAG)) {
        const float tw = __uint_as_float((unsigned)(kw >> 32));
        if (t0 >= tw + f.bias) {
            atomicAdd(&f.fu[p], c);
            atomicMin(&f.du[p], (unsigned)((t0 - tw) * s.inv_u));
            return cut ? RFOAM_UNDER | RFOAM_CUT : RFOAM_UNDER;
        }
    }
    atomicAdd(&f.fo[p], c);
    return cut ? RFOAM_OVER | RFOAM_CUT : RFOAM_OVER;
}

#define RFOAM_TALLY(w) do { const unsigned w_ = (w); over += w_ & 1u; under += (w_ >> 1) & 1u; cuts += (w_ >> 2) & 1u; removed += w_ >> 3; } while (0)

__device__ __forceinline__ void rfoam_count(const RenderFoamDev &f, unsigned block, unsigned over, unsigned under, unsigned cuts, unsigned removed) {
    over = render_wave_sum(over);
    under = render_wave_sum(under);
    cuts = render_wave_sum(cuts);
    removed = render_wave_sum(removed);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *cnt = rfoam_bank(f, 0, block);
        if (over) atomicAdd(&cnt[0], (unsigned long long)over);
        if (under) atomicAdd(&cnt[1], (unsigned long long)under);
        if (cuts) atomicAdd(&cnt[2], (unsigned long long)cuts);
        if (removed) atomicAdd(&cnt[3], (unsigned long long)removed);
    }
}

// one lane per diffuse particle; spheres above RENDER_LARGE_PX go to the mode's own large list
__global__ void __launch_bounds__(256) k_rfoam_splat_small(RenderDev d, RenderSurfDev s, RenderFoamDev f) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned over = 0, under = 0, cuts = 0, removed = 0;
    if (i < f.n) {
        const float4 p = f.pos[i];
        if (!(render_bad(p.x) || render_bad(p.y) || render_bad(p.z))) {
            const RenderView v = rthick_view(d, p);
            RenderBox b;
            if (render_bounds(d, v, b)) {
                if ((b.i1 - b.i0 + 1) * (b.j1 - b.j0 + 1) > RENDER_LARGE_PX) f.large[atomicAdd(f.nlarge, 1ull)] = i;
                else
                    for (int j = b.j0; j <= b.j1; ++j)
                        for (int x = b.i0; x <= b.i1; ++x) RFOAM_TALLY(rfoam_pixel(d, s, f, v, x, j));
            }
        }
    }
    rfoam_count(f, blockIdx.x, over, under, cuts, removed);
}

// one workgroup per sphere of the mode's large list
__global__ void __launch_bounds__(256) k_rfoam_splat_large(RenderDev d, RenderSurfDev s, RenderFoamDev f) {
    const int nl = (int)*f.nlarge;
    unsigned over = 0, under = 0, cuts = 0, removed = 0;
    for (int k = blockIdx.x; k < nl; k += gridDim.x) {
        const int i = f.large[k];
        const RenderView v = rthick_view(d, f.pos[i]);
        RenderBox b;
        if (!render_bounds(d, v, b)) continue;
        const int bw = b.i1 - b.i0 + 1, np = bw * (b.j1 - b.j0 + 1);
        for (int q = threadIdx.x; q < np; q += 256) RFOAM_TALLY(rfoam_pixel(d, s, f, v, b.i0 + q % bw, b.j0 + q / bw));
    }
    rfoam_count(f, blockIdx.x, over, under, cuts, removed);
}

// I(F) = 1 - exp2(-(density F / 256)): how much of the pixel a diffuse chord sum of F units takes
__device__ __forceinline__ float rfoam_intensity(const RenderFoamDev &f, unsigned F) {
#pragma clang fp contract(off)
    const float x = f.density * ((float)F / 256.0f);
    return 1.0f - __builtin_amdgcn_exp2f(-x);
}

// --- under layer: k_rthick_shade restated for the surface pixels with fu > 0, the fluid column split at du ---------------------------------
__global__ void __launch_bounds__(256) k_rfoam_under(RenderDev d, RenderSurfDev s, RenderThickDev t, RenderFoamDev f, const unsigned *__restrict__ Q,
                                                     const unsigned *__restrict__ T) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)d.W * d.H) return;
    const unsigned word = s.base[p];
    if (!(word & RSURF_FLAG)) return;
    const unsigned Fu = f.fu[p];
    if (Fu == 0u) return;
    const float Iu = rfoam_intensity(f, Fu);
    if (Iu == 0.0f) return;
    const int i = (int)(p % (size_t)d.W), j = (int)(p / (size_t)d.W);
    const unsigned qi = Q[p];
    const unsigned ql = i > 0 ? Q[p - 1] : RSURF_SENT, qr = i + 1 < d.W ? Q[p + 1] : RSURF_SENT;
    const unsigned qu = j > 0 ? Q[p - d.W] : RSURF_SENT, qd = j + 1 < d.H ? Q[p + d.W] : RSURF_SENT;
    const float X = render_X(d, i), Y = render_Y(d, j);
    const float z = (float)qi * s.u;
    const int sx = rsurf_side(qi, ql, qr), sy = rsurf_side(qi, qu, qd);
    const float Px = z * X, Py = z * Y, Pz = z;
    const float pl = sqrtf(Px * Px + Py * Py + Pz * Pz);
    const float ex = -Px / pl, ey = -Py / pl, ez = -Pz / pl;   // towards the eye
    float nx = ex, ny = ey, nz = ez;
    if (sx != 0 && sy != 0) {
        float ax, ay, az, bx, by, bz;
        if (sx > 0) {
            const float dz = (float)((int)qr - (int)qi) * s.u;
            ax = dz * render_X(d, i + 1) + z * s.dX; ay = dz * Y; az = dz;
        } else {
            const float dz = (float)((int)qi - (int)ql) * s.u;
            ax = dz * X + ((float)ql * s.u) * s.dX; ay = dz * Y; az = dz;
        }
        if (sy > 0) {
            const float dz = (float)((int)qd - (int)qi) * s.u;
            bx = dz * X; by = dz * render_Y(d, j + 1) + z * s.dY; bz = dz;
        } else {
            const float dz = (float)((int)qi - (int)qu) * s.u;
            bx = dz * X; by = dz * Y + ((float)qu * s.u) * s.dY; bz = dz;
        }
        const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const float cl = sqrtf(cx * cx + cy * cy + cz * cz);
        if (cl > 0.0f) {
            nx = cx / cl; ny = cy / cl; nz = cz / cl;
            if (nx * Px + ny * Py + nz * Pz > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        }
    }
    float lx = d.light[0] - Px, ly = d.light[1] - Py, lz = d.light[2] - Pz;
    const float ll = sqrtf(lx * lx + ly * ly + lz * lz);
    lx = lx / ll; ly = ly / ll; lz = lz / ll;
    const float ndl = fmaxf(nx * lx + ny * ly + nz * lz, 0.0f);
    const float hx = lx + ex, hy = ly + ey, hz = lz + ez;
    const float hl = sqrtf(hx * hx + hy * hy + hz * hz);
    const float ndh = hl > 0.0f ? fmaxf((nx * hx + ny * hy + nz * hz) / hl, 0.0f) : 0.0f;
    const float sp = ndh > 0.0f ? s.spec * __builtin_amdgcn_exp2f(s.shin * __builtin_amdgcn_logf(ndh)) : 0.0f;
    const unsigned Tm = max(T[p], 1u), m = min(Tm, f.du[p]);
    const float T1 = (float)m / 256.0f, T2 = (float)(Tm - m) / 256.0f;   // particle radii of fluid in front of the foam, behind it
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float base = (float)((word >> (8 * c)) & 0xffu) / 255.0f;
        const float lit = base * (d.amb + ndl * d.lrgb[c]);
        const float hi = sp * d.lrgb[c];
        const float kc = t.absorb * (1.0f - base) + t.scatter;
        const float a1 = __builtin_amdgcn_exp2f(-(kc * T1)), a2 = __builtin_amdgcn_exp2f(-(kc * T2));
        const float behind = (float)t.orgb[3 * p + c] / 255.0f;
        const float fc = (float)((f.rgb >> (8 * c)) & 0xffu) / 255.0f;
        const float deep = lit * (1.0f - a2) + a2 * behind;
        const float mid = fc * Iu + (1.0f - Iu) * deep;
        d.rgb[3 * p + c] = rsurf_byte((lit * (1.0f - a1) + a1 * mid) + hi);
    }
}

// --- over layer: per pixel, on the bytes the pixel holds; counts the pixels of both layers ------------------------------------------------
__global__ void __launch_bounds__(256) k_rfoam_over(RenderDev d, RenderFoamDev f) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = p < (size_t)d.W * d.H;
    const unsigned Fo = in ? f.fo[p] : 0u;
    const unsigned Fu = (in && f.okey) ? f.fu[p] : 0u;
    if (Fo) {
        const float Io = rfoam_intensity(f, Fo);
        if (Io != 0.0f) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float cur = (float)d.rgb[3 * p + c] / 255.0f;
                const float fc = (float)((f.rgb >> (8 * c)) & 0xffu) / 255.0f;
                d.rgb[3 * p + c] = rsurf_byte(cur * (1.0f - Io) + fc * Io);
            }
        }
    }
    const unsigned long long po = __ballot(Fo != 0u), pu = __ballot(Fu != 0u);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *cnt = rfoam_bank(f, 1, blockIdx.x);
        if (po) atomicAdd(&cnt[0], (unsigned long long)__popcll(po));
        if (pu) atomicAdd(&cnt[1], (unsigned long long)__popcll(pu));
    }
}

// d: the frame's RenderDev; the diffuse spheres' radius goes into a copy
static void l_render_foam_splat(RenderDev &d, RenderSurfDev &s, RenderFoamDev &f) {
    const size_t px = (size_t)d.W * d.H;
    hipMemsetAsync(f.fo, 0, px * 4, d.stream);
    hipMemsetAsync(f.fu, 0, px * 4, d.stream);
    hipMemsetAsync(f.du, 0xff, px * 4, d.stream);
    hipMemsetAsync(f.cnt, 0, RSURF_CNT_BANKS * 64, d.stream);   // group 0
    hipMemsetAsync(f.nlarge, 0, 8, d.stream);
    if (f.n > 0) {
        RenderDev l = d;
        l.r = f.rf; l.r2 = f.rf2;
        hipLaunchKernelGGL(k_rfoam_splat_small, dim3(cdiv(f.n, 256)), dim3(256), 0, d.stream, l, s, f);
        hipLaunchKernelGGL(k_rfoam_splat_large, dim3(RENDER_LARGE_GRID), dim3(256), 0, d.stream, l, s, f);
    }
}
static void l_render_foam_under(RenderDev &d, RenderSurfDev &s, RenderThickDev &t, RenderFoamDev &f, const unsigned *Q, const unsigned *T) {
    const size_t px = (size_t)d.W * d.H;
    hipLaunchKernelGGL(k_rfoam_under, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d, s, t, f, Q, T);
}
static void l_render_foam_over(RenderDev &d, RenderFoamDev &f) {
    const size_t px = (size_t)d.W * d.H;
    hipMemsetAsync(f.cnt + (size_t)RSURF_CNT_BANKS * 8, 0, RSURF_CNT_BANKS * 64, d.stream);   // group 1
    hipLaunchKernelGGL(k_rfoam_over, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d, f);
}

static void register_render_foam_launchers(Launch &L) {
    L.render_foam_splat = l_render_foam_splat;
    L.render_foam_under = l_render_foam_under;
    L.render_foam_over = l_render_foam_over;
}
