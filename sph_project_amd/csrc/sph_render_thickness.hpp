// sph_render_thickness.hpp -- thickness mode of the screen-space surface frames (a surface frame -> a translucent one): kernels and
// launchers; included by sph_kernels.hip inside the per-build namespace, behind sph_render_surface.hpp whose planes and counter banks it
// uses.  The image is defined in DESIGN.md 25, semantics in include/sph_hip.h (sph_render_set_thickness), numpy restatement in
// tests/render_thickness_model.py.
//
// Passes (the renderer's stream, no host read in between):
//   opaque    the ordinary splat and shade walks once more (siblings of k_render_small / k_render_large, whose code is untouched), filtered
//             by !rsurf_particle, on a RenderDev copy whose key / rgb / counters / large list are the opaque layer's; k_render_lines and
//             k_render_finish run on that copy as they are.  What lies behind the fluid, as the ordinary renderer would draw it.
//   splat     surface particles only: per covered pixel centre the chord of the sphere along the ray, cut at the opaque depth, as an
//             integer in units of u, added with an integer atomicAdd.  No float is ever added: the plane is a function of the particle set.
//             The float sequence runs with contraction off and IEEE division / square root: the same bits in both builds and in np.float32.
//   smooth    Jacobi steps on the thickness plane: the integer tent of the depth smoothing, its half-width taken from the final smoothed
//             depth of the pixel, every surface pixel in the window a tap.  One workgroup per 16 x 16 tile, T and Q staged in LDS.
//   shade     the composite per surface pixel: the surface shade of k_rsurf_shade restated, its Lambert term mixed with the opaque layer's
//             colour by the transmittance exp2(-tau) of the pixel's thickness.  Contraction off: both builds give the same bytes.
// The opaque and splat passes run with the frame, while the particle source is the one that was drawn; smooth and shade in
// sph_render_surface, in place of k_rsurf_shade.
#pragma once

__device__ __forceinline__ unsigned long long *rthick_bank(const RenderThickDev &t, int group, unsigned block) {
    return t.cnt + 8u * ((unsigned)group * RSURF_CNT_BANKS + (block & (RSURF_CNT_BANKS - 1)));
}

// --- opaque layer: k_render_small / k_render_large restated with the filter; o is the copy that points at the opaque planes ---------------
template <bool SHADE>
__global__ void __launch_bounds__(256) k_rthick_opaque_small(RenderDev o, RenderSurfDev s) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned issued = 0;
    bool drawn = false, bad = false;
    if (i < o.n && render_take(o, i) && !rsurf_particle(o, s, i)) {
        const float4 p = o.pos[i];
        if (render_bad(p.x) || render_bad(p.y) || render_bad(p.z)) bad = true;
        else {
            const RenderView v = render_view(o, p);
            RenderBox b;
            if (render_bounds(o, v, b)) {
                drawn = true;
                const unsigned id = (unsigned)o.id[i];
                if ((b.i1 - b.i0 + 1) * (b.j1 - b.j0 + 1) > RENDER_LARGE_PX) {
                    if (!SHADE) o.large[atomicAdd(&o.cnt[2], 1ull)] = i;
                } else {
                    const unsigned col = SHADE ? render_colour(o, i, id) : 0u;
                    for (int j = b.j0; j <= b.j1; ++j)
                        for (int x = b.i0; x <= b.i1; ++x) render_pixel<SHADE>(o, v, x, j, id, col, issued);
                }
            }
        }
    }
    if (SHADE) return;
    const unsigned long long dr = __ballot(drawn), bd = __ballot(bad);
    issued = render_wave_sum(issued);
    if ((threadIdx.x & 63) == 0) {
        if (dr) atomicAdd(&o.cnt[0], (unsigned long long)__popcll(dr));
        if (bd) atomicAdd(&o.cnt[1], (unsigned long long)__popcll(bd));
        if (issued) atomicAdd(&o.cnt[3], (unsigned long long)issued);
    }
}

template <bool SHADE>
__global__ void __launch_bounds__(256) k_rthick_opaque_large(RenderDev o) {   // (the list holds opaque particles only)
    const int nl = (int)o.cnt[2];
    unsigned issued = 0;
    for (int k = blockIdx.x; k < nl; k += gridDim.x) {
        const int i = o.large[k];
        const RenderView v = render_view(o, o.pos[i]);
        RenderBox b;
        if (!render_bounds(o, v, b)) continue;
        const unsigned id = (unsigned)o.id[i];
        const unsigned col = SHADE ? render_colour(o, i, id) : 0u;
        const int bw = b.i1 - b.i0 + 1, np = bw * (b.j1 - b.j0 + 1);
        for (int q = threadIdx.x; q < np; q += 256) render_pixel<SHADE>(o, v, b.i0 + q % bw, b.j0 + q / bw, id, col, issued);
    }
    if (SHADE) return;
    issued = render_wave_sum(issued);
    if ((threadIdx.x & 63) == 0 && issued) atomicAdd(&o.cnt[3], (unsigned long long)issued);
}

// --- thickness splat ----------------------------------------------------------------------------------------------------------------------
// render_view, render_X / render_Y and render_hit restated: one rounding per operation, sums from the left
__device__ __forceinline__ RenderView rthick_view(const RenderDev &d, float4 p) {
#pragma clang fp contract(off)
    const float vx = p.x - d.E[0], vy = p.y - d.E[1], vz = p.z - d.E[2];
    RenderView v;
    v.xs = (d.s[0] * vx + d.s[1] * vy) + d.s[2] * vz;
    v.ys = (d.u[0] * vx + d.u[1] * vy) + d.u[2] * vz;
    v.z = (d.f[0] * vx + d.f[1] * vy) + d.f[2] * vz;
    return v;
}

// one pixel of one surface sphere: the chord [t0, t1] of the ray, its far end cut at the opaque depth, in units of u.  Returns the pair's
// flags: RTHICK_ADD an add was issued, RTHICK_CUT ... of a chord the opaque depth cut short, RTHICK_REMOVED the opaque depth removed it
#define RTHICK_ADD 1u
#define RTHICK_CUT 2u
#define RTHICK_REMOVED 4u
__device__ __forceinline__ unsigned rthick_pixel(const RenderDev &d, const RenderSurfDev &s, const RenderThickDev &t, const RenderView &v, int i,
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
    const unsigned long long ko = t.okey[p];
    float b = t1;
    bool cut = false;
    if (ko != ~0ull) {
        const float top = __uint_as_float((unsigned)(ko >> 32));
        if (top < t1) { b = top; cut = true; }
    }
    if (!(b > t0)) return RTHICK_REMOVED;
    atomicAdd(&t.T[0][p], (unsigned)((b - t0) * s.inv_u));
    return cut ? RTHICK_ADD | RTHICK_CUT : RTHICK_ADD;
}

#define RTHICK_TALLY(w) do { const unsigned w_ = (w); adds += w_ & 1u; cuts += (w_ >> 1) & 1u; removed += w_ >> 2; } while (0)

__device__ __forceinline__ void rthick_count(const RenderThickDev &t, unsigned block, unsigned adds, unsigned cuts, unsigned removed) {
    adds = render_wave_sum(adds);
    cuts = render_wave_sum(cuts);
    removed = render_wave_sum(removed);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *cnt = rthick_bank(t, 0, block);
        if (adds) atomicAdd(&cnt[0], (unsigned long long)adds);
        if (cuts) atomicAdd(&cnt[1], (unsigned long long)cuts);
        if (removed) atomicAdd(&cnt[2], (unsigned long long)removed);
    }
}

// one thread per particle (the walk of k_render_small); large spheres are left to the large pass
__global__ void __launch_bounds__(256) k_rthick_splat_small(RenderDev d, RenderSurfDev s, RenderThickDev t) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned adds = 0, cuts = 0, removed = 0;
    if (i < d.n && render_take(d, i) && rsurf_particle(d, s, i)) {
        const float4 p = d.pos[i];
        if (!(render_bad(p.x) || render_bad(p.y) || render_bad(p.z))) {
            const RenderView v = rthick_view(d, p);
            RenderBox b;
            if (render_bounds(d, v, b) && (b.i1 - b.i0 + 1) * (b.j1 - b.j0 + 1) <= RENDER_LARGE_PX)
                for (int j = b.j0; j <= b.j1; ++j)
                    for (int x = b.i0; x <= b.i1; ++x) RTHICK_TALLY(rthick_pixel(d, s, t, v, x, j));
        }
    }
    rthick_count(t, blockIdx.x, adds, cuts, removed);
}

// one workgroup per sphere of the frame's large list (surface and opaque particles: the list and its length are the ordinary splat's)
__global__ void __launch_bounds__(256) k_rthick_splat_large(RenderDev d, RenderSurfDev s, RenderThickDev t) {
    const int nl = (int)d.cnt[2];
    unsigned adds = 0, cuts = 0, removed = 0;
    for (int k = blockIdx.x; k < nl; k += gridDim.x) {
        const int i = d.large[k];
        if (!rsurf_particle(d, s, i)) continue;
        const RenderView v = rthick_view(d, d.pos[i]);
        RenderBox b;
        if (!render_bounds(d, v, b)) continue;
        const int bw = b.i1 - b.i0 + 1, np = bw * (b.j1 - b.j0 + 1);
        for (int q = threadIdx.x; q < np; q += 256) RTHICK_TALLY(rthick_pixel(d, s, t, v, b.i0 + q % bw, b.j0 + q / bw));
    }
    rthick_count(t, blockIdx.x, adds, cuts, removed);
}

// --- smoothing: k_rsurf_smooth's tile and window, with the half-width and the taps' validity read off the depth plane Q -------------------
__global__ void __launch_bounds__(256) k_rthick_smooth(int W, int H, RenderSurfDev s, RenderThickDev t, const unsigned *__restrict__ Q,
                                                       const unsigned *__restrict__ in, unsigned *__restrict__ out) {
    __shared__ unsigned tq[RSURF_LDS_W * RSURF_LDS_W];
    __shared__ unsigned tt[RSURF_LDS_W * RSURF_LDS_W];
    __shared__ int halo;
    const int tx = threadIdx.x & (RSURF_TILE - 1), ty = threadIdx.x / RSURF_TILE;
    const int gx = (int)blockIdx.x * RSURF_TILE + tx, gy = (int)blockIdx.y * RSURF_TILE + ty;
    const unsigned qi = (gx < W && gy < H) ? Q[(size_t)gy * W + gx] : RSURF_SENT;
    const bool surf = qi != RSURF_SENT;
    const unsigned raw = qi ? s.rnum / qi : (unsigned)s.rmax + 1u;
    const int Ri = (int)min(max(raw, 1u), (unsigned)s.rmax);
    if (threadIdx.x == 0) halo = 0;
    __syncthreads();
    if (surf) atomicMax(&halo, Ri);
    __syncthreads();
    const int R = halo;   // 0: a tile without a surface pixel
    if (R == 0) return;
    const int TW = RSURF_TILE + 2 * R;
    const int x0 = (int)blockIdx.x * RSURF_TILE - R, y0 = (int)blockIdx.y * RSURF_TILE - R;
    for (int c = threadIdx.x; c < TW * TW; c += 256) {
        const int cx = x0 + c % TW, cy = y0 + c / TW;
        const bool inside = cx >= 0 && cx < W && cy >= 0 && cy < H;
        tq[c] = inside ? Q[(size_t)cy * W + cx] : RSURF_SENT;
        tt[c] = inside ? in[(size_t)cy * W + cx] : 0u;
    }
    __syncthreads();
    unsigned visited = 0;
    if (surf) {
        unsigned long long num = 0;
        unsigned den = 0;
        for (int dy = -Ri; dy <= Ri; ++dy) {
            const unsigned wy = (unsigned)(Ri + 1 - abs(dy));
            const int row = (ty + R + dy) * TW + tx + R;
            for (int dx = -Ri; dx <= Ri; ++dx) {
                if (tq[row + dx] != RSURF_SENT) {
                    const unsigned w = wy * (unsigned)(Ri + 1 - abs(dx));
                    num += (unsigned long long)w * tt[row + dx];
                    den += w;
                }
            }
        }
        visited = (unsigned)((2 * Ri + 1) * (2 * Ri + 1));
        out[(size_t)gy * W + gx] = (unsigned)((num + (den >> 1)) / den);   // the centre tap always counts: den > 0
    }
    visited = render_wave_sum(visited);
    if ((threadIdx.x & 63) == 0 && visited)
        atomicAdd(&rthick_bank(t, 1, blockIdx.y * gridDim.x + blockIdx.x)[0], (unsigned long long)visited);
}

// --- composite: k_rsurf_shade restated up to its two terms, then the mix with the opaque layer ---------------------------------------------
__global__ void __launch_bounds__(256) k_rthick_shade(RenderDev d, RenderSurfDev s, RenderThickDev t, const unsigned *__restrict__ Q,
                                                      const unsigned *__restrict__ T) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned word = p < (size_t)d.W * d.H ? s.base[p] : 0u;
    const bool surf = (word & RSURF_FLAG) != 0u;
    unsigned Ti = 0u;
    bool empty = false;
    if (surf) {
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
        Ti = T[p];
        empty = t.T[0][p] == 0u;
        const float Tr = (float)max(Ti, 1u) / 256.0f;   // particle radii of fluid along the ray; a surface pixel is never empty
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float base = (float)((word >> (8 * c)) & 0xffu) / 255.0f;
            const float lit = base * (d.amb + ndl * d.lrgb[c]);
            const float hi = sp * d.lrgb[c];
            const float tau = (t.absorb * (1.0f - base) + t.scatter) * Tr;
            const float a = __builtin_amdgcn_exp2f(-tau);
            const float behind = (float)t.orgb[3 * p + c] / 255.0f;
            d.rgb[3 * p + c] = rsurf_byte((behind * a + lit * (1.0f - a)) + hi);
        }
    }
    const unsigned long long em = __ballot(empty);
    unsigned tm = Ti;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tm = max(tm, (unsigned)__shfl_xor((int)tm, o, 64));
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *cnt = rthick_bank(t, 1, blockIdx.x);
        if (em) atomicAdd(&cnt[1], (unsigned long long)__popcll(em));
        if (tm) atomicMax(&cnt[2], (unsigned long long)tm);
    }
}

// the copy of the frame's RenderDev that draws into the opaque layer (no id image)
static RenderDev rthick_opaque_dev(const RenderDev &d, const RenderThickDev &t) {
    RenderDev o = d;
    o.key = t.okey; o.rgb = t.orgb; o.ids = nullptr; o.cnt = t.ocnt; o.large = t.olarge;
    return o;
}

static void l_render_thick_opaque(RenderDev &d, RenderSurfDev &s, RenderThickDev &t) {
    RenderDev o = rthick_opaque_dev(d, t);
    const size_t px = (size_t)d.W * d.H;
    hipMemsetAsync(t.okey, 0xff, px * 8, d.stream);
    hipMemsetAsync(t.ocnt, 0, 64, d.stream);
    if (d.n > 0) {
        hipLaunchKernelGGL(k_rthick_opaque_small<false>, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, o, s);
        hipLaunchKernelGGL(k_rthick_opaque_large<false>, dim3(RENDER_LARGE_GRID), dim3(256), 0, d.stream, o);
    }
    if (d.draw_box) hipLaunchKernelGGL(k_render_lines<false>, dim3(12), dim3(256), 0, d.stream, o);
    if (d.n > 0) {
        hipLaunchKernelGGL(k_rthick_opaque_small<true>, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, o, s);
        hipLaunchKernelGGL(k_rthick_opaque_large<true>, dim3(RENDER_LARGE_GRID), dim3(256), 0, d.stream, o);
    }
    if (d.draw_box) hipLaunchKernelGGL(k_render_lines<true>, dim3(12), dim3(256), 0, d.stream, o);
    hipLaunchKernelGGL(k_render_finish, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, o);
}
static void l_render_thick_splat(RenderDev &d, RenderSurfDev &s, RenderThickDev &t) {
    hipMemsetAsync(t.T[0], 0, (size_t)d.W * d.H * 4, d.stream);
    hipMemsetAsync(t.cnt, 0, RSURF_CNT_BANKS * 64, d.stream);   // group 0
    if (d.n > 0) {
        hipLaunchKernelGGL(k_rthick_splat_small, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d, s, t);
        hipLaunchKernelGGL(k_rthick_splat_large, dim3(RENDER_LARGE_GRID), dim3(256), 0, d.stream, d, s, t);
    }
}
static void l_render_thick_smooth(RenderDev &d, RenderSurfDev &s, RenderThickDev &t, const unsigned *Q, const unsigned *in, unsigned *out) {
    hipLaunchKernelGGL(k_rthick_smooth, dim3(cdiv(d.W, RSURF_TILE), cdiv(d.H, RSURF_TILE)), dim3(256), 0, d.stream, d.W, d.H, s, t, Q, in, out);
}
static void l_render_thick_shade(RenderDev &d, RenderSurfDev &s, RenderThickDev &t, const unsigned *Q, const unsigned *T) {
    const size_t px = (size_t)d.W * d.H;
    hipLaunchKernelGGL(k_rthick_shade, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d, s, t, Q, T);
}

static void register_render_thickness_launchers(Launch &L) {
    L.render_thick_opaque = l_render_thick_opaque;
    L.render_thick_splat = l_render_thick_splat;
    L.render_thick_smooth = l_render_thick_smooth;
    L.render_thick_shade = l_render_thick_shade;
}
