// sph_render_surface.hpp -- screen-space surface mode of the particle renderer (a particle frame -> a smoothed, lit liquid surface):
// kernels and launchers; included by sph_kernels.hip inside the per-build namespace, behind sph_render.hpp whose walk and camera it uses.
// The image is defined in DESIGN.md 24, semantics in include/sph_hip.h (sph_render_set_surface), integer restatement in
// tests/render_surface_model.py.
//
// Passes (the renderer's stream, no host read in between):
//   base      the shade walk of sph_render.hpp once more (a sibling of k_render_small / k_render_large<true>, whose code is untouched): a
//             pixel whose final key carries the particle's id gets the particle's unshaded colour, plus RSURF_FLAG when the particle
//             belongs to a surface object.  Runs with the frame, while the particle source is still the one that was drawn.
//   quantise  per pixel: q = min((u32)(t * inv_u), 2^24 - 1) where the flag is set, the sentinel elsewhere; written to both q planes.
//   smooth    `iterations` Jacobi steps between the two planes: one workgroup per 16 x 16 tile, the tile + a halo of its largest window
//             staged in LDS, integer tent weights over a window whose half-width follows the depth; no float anywhere.
//   shade     per flagged pixel: one-sided differences towards the nearer neighbour (chosen on integers), normal, Lambert + Blinn-Phong,
//             plain stores into the frame's rgb.  Contraction is off in this pass: both builds give the same bytes.
#pragma once

#define RSURF_TILE 16
#define RSURF_LDS_W (RSURF_TILE + 2 * RSURF_RMAX_CAP)

// a surface particle: handle path by object mask (and, with fluid_only, by material), points path by the per-point flag
__device__ __forceinline__ bool rsurf_particle(const RenderDev &d, const RenderSurfDev &s, int i) {
    if (d.meta) {
        const int m = d.meta[i], o = META_OBJ(m);
        if (s.fluid_only && META_MAT(m) != 1) return false;
        return o >= 0 && o < 32 && ((s.omask >> o) & 1u);
    }
    return !s.pmask || s.pmask[i] != 0;
}

// the counter bank of a workgroup
__device__ __forceinline__ unsigned long long *rsurf_bank(const RenderSurfDev &s, unsigned block) {
    return s.cnt + 8u * (block & (RSURF_CNT_BANKS - 1));
}

__device__ __forceinline__ void rsurf_base_pixel(const RenderDev &d, const RenderSurfDev &s, int i, int j, unsigned id, unsigned word) {
    const size_t p = (size_t)j * d.W + i;
    if ((unsigned)d.key[p] == id) s.base[p] = word;
}

// one thread per particle (the walk of k_render_small<true>); large spheres are left to the large pass
__global__ void __launch_bounds__(256) k_rsurf_base_small(RenderDev d, RenderSurfDev s) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n || !render_take(d, i)) return;
    const float4 p = d.pos[i];
    if (render_bad(p.x) || render_bad(p.y) || render_bad(p.z)) return;
    const RenderView v = render_view(d, p);
    RenderBox b;
    if (!render_bounds(d, v, b)) return;
    if ((b.i1 - b.i0 + 1) * (b.j1 - b.j0 + 1) > RENDER_LARGE_PX) return;
    const unsigned id = (unsigned)d.id[i];
    const unsigned word = (render_colour(d, i, id) & 0xffffffu) | (rsurf_particle(d, s, i) ? RSURF_FLAG : 0u);
    for (int j = b.j0; j <= b.j1; ++j)
        for (int x = b.i0; x <= b.i1; ++x) rsurf_base_pixel(d, s, x, j, id, word);
}

// one workgroup per listed sphere (the list and its length are the splat's of this frame)
__global__ void __launch_bounds__(256) k_rsurf_base_large(RenderDev d, RenderSurfDev s) {
    const int nl = (int)d.cnt[2];
    for (int k = blockIdx.x; k < nl; k += gridDim.x) {
        const int i = d.large[k];
        const RenderView v = render_view(d, d.pos[i]);
        RenderBox b;
        if (!render_bounds(d, v, b)) continue;
        const unsigned id = (unsigned)d.id[i];
        const unsigned word = (render_colour(d, i, id) & 0xffffffu) | (rsurf_particle(d, s, i) ? RSURF_FLAG : 0u);
        const int bw = b.i1 - b.i0 + 1, np = bw * (b.j1 - b.j0 + 1);
        for (int q = threadIdx.x; q < np; q += 256) rsurf_base_pixel(d, s, b.i0 + q % bw, b.j0 + q / bw, id, word);
    }
}

// one rounded multiply and a truncation: the same integer in both builds and in numpy float32
__global__ void __launch_bounds__(256) k_rsurf_quantise(RenderDev d, RenderSurfDev s) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool surf = false;
    if (p < (size_t)d.W * d.H) {
        unsigned q = RSURF_SENT;
        if (s.base[p] & RSURF_FLAG) {
            const float v = __uint_as_float((unsigned)(d.key[p] >> 32)) * s.inv_u;
            q = v >= (float)RSURF_QMAX ? RSURF_QMAX : (unsigned)v;
            surf = true;
        }
        s.q[0][p] = q;
        s.q[1][p] = q;
    }
    const unsigned long long c = __ballot(surf);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&rsurf_bank(s, blockIdx.x)[0], (unsigned long long)__popcll(c));
}

// One Jacobi step.  Every thread first reads its own pixel and takes its window half-width R_i; the tile's largest R_i (one LDS atomic per
// surface pixel) is the halo that is staged with the tile in LDS -- at most rmax, far less where the surface is distant -- and a tile
// without a surface pixel leaves before it stages anything.  Out-of-frame cells hold the sentinel, which no tap accepts.  Every thread
// then walks its own (2 R_i + 1)^2 window.  R_i differs across a wave: the loops simply diverge -- the hardware runs the wave to its
// largest R with the finished lanes masked, which is what an explicit wave maximum plus a mask would do, without the cross-lane step.
// Non-surface pixels hold the sentinel in both planes since the quantise pass, so only surface pixels are written.
__global__ void __launch_bounds__(256) k_rsurf_smooth(int W, int H, RenderSurfDev s, const unsigned *__restrict__ in, unsigned *__restrict__ out,
                                                      int first) {
    __shared__ unsigned tile[RSURF_LDS_W * RSURF_LDS_W];
    __shared__ int halo;
    const int tx = threadIdx.x & (RSURF_TILE - 1), ty = threadIdx.x / RSURF_TILE;
    const int gx = (int)blockIdx.x * RSURF_TILE + tx, gy = (int)blockIdx.y * RSURF_TILE + ty;
    const unsigned qi = (gx < W && gy < H) ? in[(size_t)gy * W + gx] : RSURF_SENT;
    const bool surf = qi != RSURF_SENT;
    const unsigned raw = qi ? s.rnum / qi : (unsigned)s.rmax + 1u;   // (the sentinel gives 0; unused there)
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
        tile[c] = (cx >= 0 && cx < W && cy >= 0 && cy < H) ? in[(size_t)cy * W + cx] : RSURF_SENT;
    }
    __syncthreads();
    unsigned visited = 0, accepted = 0;
    bool clamped = false;
    if (surf) {
        clamped = raw > (unsigned)s.rmax;
        unsigned long long num = 0;
        unsigned den = 0;
        for (int dy = -Ri; dy <= Ri; ++dy) {
            const unsigned wy = (unsigned)(Ri + 1 - abs(dy));
            const unsigned *row = tile + (ty + R + dy) * TW + tx + R;
            for (int dx = -Ri; dx <= Ri; ++dx) {
                const unsigned qj = row[dx];
                const unsigned diff = qj > qi ? qj - qi : qi - qj;
                if (qj != RSURF_SENT && diff <= s.dq) {
                    const unsigned w = wy * (unsigned)(Ri + 1 - abs(dx));
                    num += (unsigned long long)w * qj;
                    den += w;
                    ++accepted;
                }
            }
        }
        visited = (unsigned)((2 * Ri + 1) * (2 * Ri + 1));
        out[(size_t)gy * W + gx] = (unsigned)((num + (den >> 1)) / den);   // the centre tap always counts: den > 0
    }
    const unsigned long long cl = __ballot(clamped);
    visited = render_wave_sum(visited);
    accepted = render_wave_sum(accepted);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *cnt = rsurf_bank(s, blockIdx.y * gridDim.x + blockIdx.x);
        if (visited) atomicAdd(&cnt[1], (unsigned long long)visited);
        if (accepted) atomicAdd(&cnt[2], (unsigned long long)accepted);
        if (first && cl) atomicAdd(&cnt[3], (unsigned long long)__popcll(cl));
    }
}

__device__ __forceinline__ unsigned char rsurf_byte(float x) {
#pragma clang fp contract(off)
    x = fminf(fmaxf(x, 0.0f), 1.0f);
    const float y = 255.0f * x;
    return (unsigned char)floorf(y + 0.5f);
}

// the neighbour of the one-sided difference along one axis: +1 the neighbour at index + 1, -1 the one before, 0 none.  The smaller
// |dq| wins, a tie goes to the + side.
__device__ __forceinline__ int rsurf_side(unsigned qi, unsigned qm, unsigned qp) {
    const bool vm = qm != RSURF_SENT, vp = qp != RSURF_SENT;
    const unsigned dm = qm > qi ? qm - qi : qi - qm, dp = qp > qi ? qp - qi : qi - qp;
    if (vp && (!vm || dp <= dm)) return 1;
    return vm ? -1 : 0;
}

// Per flagged pixel.  P = z (X, Y, 1), z = q u.  The difference to a neighbour is formed without cancellation:
// P_j - P_i = (dz X_j + z_i dX, dz Y, dz) with dz = (q_j - q_i) u from the exact integer difference.
__global__ void __launch_bounds__(256) k_rsurf_shade(RenderDev d, RenderSurfDev s, const unsigned *__restrict__ Q) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)d.W * d.H) return;
    const unsigned word = s.base[p];
    if (!(word & RSURF_FLAG)) return;
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
    // ndh^shininess through the hardware's log2 / exp2 (the same instructions in both builds)
    const float sp = ndh > 0.0f ? s.spec * __builtin_amdgcn_exp2f(s.shin * __builtin_amdgcn_logf(ndh)) : 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float base = (float)((word >> (8 * c)) & 0xffu) / 255.0f;
        const float lit = d.amb + ndl * d.lrgb[c];
        const float hi = sp * d.lrgb[c];
        d.rgb[3 * p + c] = rsurf_byte(base * lit + hi);
    }
}

static void l_render_surface_base(RenderDev &d, RenderSurfDev &s) {
    hipMemsetAsync(s.base, 0, (size_t)d.W * d.H * 4, d.stream);
    if (d.n > 0) {
        hipLaunchKernelGGL(k_rsurf_base_small, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d, s);
        hipLaunchKernelGGL(k_rsurf_base_large, dim3(RENDER_LARGE_GRID), dim3(256), 0, d.stream, d, s);
    }
}
static void l_render_surface_quantise(RenderDev &d, RenderSurfDev &s) {
    const size_t px = (size_t)d.W * d.H;
    hipLaunchKernelGGL(k_rsurf_quantise, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d, s);
}
static void l_render_surface_smooth(RenderDev &d, RenderSurfDev &s, int it) {
    hipLaunchKernelGGL(k_rsurf_smooth, dim3(cdiv(d.W, RSURF_TILE), cdiv(d.H, RSURF_TILE)), dim3(256), 0, d.stream, d.W, d.H, s,
                       (const unsigned *)s.q[it & 1], s.q[1 - (it & 1)], it == 0 ? 1 : 0);
}
static void l_render_surface_shade(RenderDev &d, RenderSurfDev &s, int plane) {
    const size_t px = (size_t)d.W * d.H;
    hipLaunchKernelGGL(k_rsurf_shade, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d, s, (const unsigned *)s.q[plane]);
}

static void register_render_surface_launchers(Launch &L) {
    L.render_surface_base = l_render_surface_base;
    L.render_surface_quantise = l_render_surface_quantise;
    L.render_surface_smooth = l_render_surface_smooth;
    L.render_surface_shade = l_render_surface_shade;
}
