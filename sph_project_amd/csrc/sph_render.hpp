// sph_render.hpp -- particle rendering (particles -> one RGB frame): kernels and launchers; included by sph_kernels.hip inside the per-build
// namespace.  The image is defined in DESIGN.md 15, semantics in include/sph_hip.h (sph_render_create), float64 restatement in
// tests/render_model.py.  Replaces the GGUI frame of the reference's run_simulation.py:116-135 (scene.particles + scene.lines, then
// window.save_image).
//
// Passes (one stream, no host read in between):
//   splat   one thread per particle: object mask / ghost / dead, non-finite (counted), cull, conservative pixel bounds, then per covered
//           pixel centre the ray-sphere test and an atomicMin of the u64 key (float_bits(t) << 32 | id) -- after a plain load of the
//           current key says it would lower it.  Keys only decrease, so a stale load costs an extra atomic, never a lost one.  Spheres
//           whose bounds exceed RENDER_LARGE_PX pixels go to a list that one workgroup per sphere handles.  The box lines step along
//           their screen major axis (geometry clipped and projected on the host, in double).
//   shade   the same walk: a pixel whose final key carries the particle's id (line id) is that particle's (line's) alone, so it writes
//           the colour with plain stores; depth comes back from the key.  Then per pixel: background, the id image, covered pixels.
// The image is a function of the particle SET: the winner of a pixel is the smallest key, whatever the order the atomics ran in.
#pragma once

#define RENDER_LARGE_PX 4096   // pixels of a sphere's screen bounds above which one workgroup (not one thread) walks them
#define RENDER_LARGE_GRID 512  // workgroups of the large-sphere passes (grid-stride over the list, whose length stays on the device)

struct RenderView { float xs, ys, z; };   // c - E in (s, u, f) coordinates
struct RenderBox { int i0, i1, j0, j1; };

__device__ __forceinline__ bool render_bad(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// object mask, ghosts and dead slots of the handle path (meta null: the points path, every particle)
__device__ __forceinline__ bool render_take(const RenderDev &d, int i) {
    if (!d.meta) return true;
    const int m = d.meta[i];
    if (META_GHOST(m) || META_DEAD(m)) return false;
    const int o = META_OBJ(m);
    return o >= 0 && o < 32 && ((d.mask >> o) & 1u);
}

__device__ __forceinline__ RenderView render_view(const RenderDev &d, float4 p) {
    const float vx = p.x - d.E[0], vy = p.y - d.E[1], vz = p.z - d.E[2];
    RenderView v;
    v.xs = d.s[0] * vx + d.s[1] * vy + d.s[2] * vz;
    v.ys = d.u[0] * vx + d.u[1] * vy + d.u[2] * vz;
    v.z = d.f[0] * vx + d.f[1] * vy + d.f[2] * vz;
    return v;
}

// screen coordinate (X or Y, image plane at depth 1) -> continuous pixel index whose integer part + 0.5 is a pixel centre
__device__ __forceinline__ float render_col(const RenderDev &d, float X) { return (X / d.tx + 1.0f) * (0.5f * (float)d.W) - 0.5f; }
__device__ __forceinline__ float render_row(const RenderDev &d, float Y) { return (1.0f - Y / d.ty) * (0.5f * (float)d.H) - 0.5f; }

// the sphere's shadow on one screen axis: tangents from the eye in the plane of that axis and f (exact for a sphere, z > r)
__device__ __forceinline__ void render_span(float a, float z, float r, float &lo, float &hi) {
    const float den = z * z - r * r;
    const float q = r * sqrtf(fmaxf(a * a + den, 0.0f));
    lo = (a * z - q) / den;
    hi = (a * z + q) / den;
}

// conservative pixel bounds (one pixel of margin), clipped to the screen; false: nothing to draw
__device__ __forceinline__ bool render_bounds(const RenderDev &d, const RenderView &v, RenderBox &b) {
    if (!(v.z + d.r > d.zn)) return false;   // wholly behind the near plane
    float c0 = -1.0f, c1 = (float)d.W, r0 = -1.0f, r1 = (float)d.H;   // straddles the near plane or holds the eye: the whole screen
    if (v.z - d.r > d.zn) {
        float xl, xh, yl, yh;
        render_span(v.xs, v.z, d.r, xl, xh);
        render_span(v.ys, v.z, d.r, yl, yh);
        const float lim = 4.0f * (float)(d.W > d.H ? d.W : d.H);
        c0 = fminf(fmaxf(render_col(d, xl), -lim), lim);
        c1 = fminf(fmaxf(render_col(d, xh), -lim), lim);
        r0 = fminf(fmaxf(render_row(d, yh), -lim), lim);
        r1 = fminf(fmaxf(render_row(d, yl), -lim), lim);
    }
    b.i0 = max((int)floorf(c0) - 1, 0);
    b.i1 = min((int)ceilf(c1) + 1, d.W - 1);
    b.j0 = max((int)floorf(r0) - 1, 0);
    b.j1 = min((int)ceilf(r1) + 1, d.H - 1);
    return b.i0 <= b.i1 && b.j0 <= b.j1;
}

// pixel (i, j)'s ray d = (X, Y, 1) in (s, u, f) coordinates
__device__ __forceinline__ float render_X(const RenderDev &d, int i) { return ((float)(2 * i + 1) / (float)d.W - 1.0f) * d.tx; }
__device__ __forceinline__ float render_Y(const RenderDev &d, int j) { return (1.0f - (float)(2 * j + 1) / (float)d.H) * d.ty; }

// ray-sphere: disc = b^2 - (d.d)(|v|^2 - r^2) evaluated as (d.d)(r^2 - |w|^2), w = v - (b / d.d) d the part of v across the ray
// (no cancellation of two |v|^2-sized terms); t = b / d.d - sqrt(disc) / d.d.  Hit: disc >= 0 and t > zn.
__device__ __forceinline__ bool render_hit(const RenderDev &d, const RenderView &v, float X, float Y, float &t) {
    const float dd = X * X + Y * Y + 1.0f;
    const float k = (X * v.xs + Y * v.ys + v.z) / dd;
    const float wx = v.xs - k * X, wy = v.ys - k * Y, wz = v.z - k;
    const float h = d.r2 - (wx * wx + wy * wy + wz * wz);
    if (!(h >= 0.0f)) return false;
    t = k - sqrtf(h / dd);
    return t > d.zn;
}

__device__ __forceinline__ unsigned char render_byte(float x) {
    x = fminf(fmaxf(x, 0.0f), 1.0f);
    return (unsigned char)floorf(255.0f * x + 0.5f);
}

// the colour of the winner at depth t: ambient + Lambert from the point light, per channel
__device__ __forceinline__ void render_shade_px(const RenderDev &d, const RenderView &v, float X, float Y, float t, unsigned col,
                                                unsigned char *out) {
    const float inv_r = 1.0f / d.r;
    const float nx = (t * X - v.xs) * inv_r, ny = (t * Y - v.ys) * inv_r, nz = (t - v.z) * inv_r;
    const float lx = d.light[0] - t * X, ly = d.light[1] - t * Y, lz = d.light[2] - t;   // light in (s, u, f) coordinates
    const float ln = sqrtf(lx * lx + ly * ly + lz * lz);
    const float ndl = fmaxf((nx * lx + ny * ly + nz * lz) / ln, 0.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float base = (float)((col >> (8 * c)) & 0xffu) / 255.0f;
        out[c] = render_byte(base * (d.amb + ndl * d.lrgb[c]));
    }
}

__device__ __forceinline__ unsigned render_colour(const RenderDev &d, int i, unsigned id) {
    return d.col_home ? d.col_home[id] : d.col ? d.col[i] : 0xffffffu;
}

// one pixel of one sphere: SPLAT lowers the key (counting the atomics issued), SHADE writes the colour where the key is this sphere's
template <bool SHADE>
__device__ __forceinline__ void render_pixel(const RenderDev &d, const RenderView &v, int i, int j, unsigned id, unsigned col, unsigned &issued) {
    const float X = render_X(d, i), Y = render_Y(d, j);
    const size_t p = (size_t)j * d.W + i;
    if (SHADE) {
        const unsigned long long k = d.key[p];
        if ((unsigned)k == id) render_shade_px(d, v, X, Y, __uint_as_float((unsigned)(k >> 32)), col, d.rgb + 3 * p);
    } else {
        float t;
        if (!render_hit(d, v, X, Y, t)) return;
        const unsigned long long k = ((unsigned long long)__float_as_uint(t) << 32) | id;
        if (k < d.key[p]) { atomicMin(&d.key[p], k); ++issued; }
    }
}

__device__ __forceinline__ unsigned render_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one thread per particle; large spheres are listed (splat) or left to the large pass (shade)
template <bool SHADE>
__global__ void __launch_bounds__(256) k_render_small(RenderDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned issued = 0;
    bool drawn = false, bad = false;
    if (i < d.n && render_take(d, i)) {
        const float4 p = d.pos[i];
        if (render_bad(p.x) || render_bad(p.y) || render_bad(p.z)) bad = true;
        else {
            const RenderView v = render_view(d, p);
            RenderBox b;
            if (render_bounds(d, v, b)) {
                drawn = true;
                const unsigned id = (unsigned)d.id[i];
                if ((b.i1 - b.i0 + 1) * (b.j1 - b.j0 + 1) > RENDER_LARGE_PX) {
                    if (!SHADE) d.large[atomicAdd(&d.cnt[2], 1ull)] = i;
                } else {
                    const unsigned col = SHADE ? render_colour(d, i, id) : 0u;
                    for (int j = b.j0; j <= b.j1; ++j)
                        for (int x = b.i0; x <= b.i1; ++x) render_pixel<SHADE>(d, v, x, j, id, col, issued);
                }
            }
        }
    }
    if (SHADE) return;
    const unsigned long long dr = __ballot(drawn), bd = __ballot(bad);
    issued = render_wave_sum(issued);
    if ((threadIdx.x & 63) == 0) {
        if (dr) atomicAdd(&d.cnt[0], (unsigned long long)__popcll(dr));
        if (bd) atomicAdd(&d.cnt[1], (unsigned long long)__popcll(bd));
        if (issued) atomicAdd(&d.cnt[3], (unsigned long long)issued);
    }
}

// one workgroup per listed sphere: its 256 threads stride over the bounds' pixels
template <bool SHADE>
__global__ void __launch_bounds__(256) k_render_large(RenderDev d) {
    const int nl = (int)d.cnt[2];
    unsigned issued = 0;
    for (int k = blockIdx.x; k < nl; k += gridDim.x) {
        const int i = d.large[k];
        const RenderView v = render_view(d, d.pos[i]);
        RenderBox b;
        if (!render_bounds(d, v, b)) continue;
        const unsigned id = (unsigned)d.id[i];
        const unsigned col = SHADE ? render_colour(d, i, id) : 0u;
        const int bw = b.i1 - b.i0 + 1, np = bw * (b.j1 - b.j0 + 1);
        for (int q = threadIdx.x; q < np; q += 256) render_pixel<SHADE>(d, v, b.i0 + q % bw, b.j0 + q / bw, id, col, issued);
    }
    if (SHADE) return;
    issued = render_wave_sum(issued);
    if ((threadIdx.x & 63) == 0 && issued) atomicAdd(&d.cnt[3], (unsigned long long)issued);
}

// box lines: one workgroup per edge, one thread per step along the screen major axis (RenderDev::line, set by the host)
template <bool SHADE>
__global__ void __launch_bounds__(256) k_render_lines(RenderDev d) {
    const int e = blockIdx.x;
    if (d.line_axis[e] < 0) return;
    const float *g = d.line[e];
    const int k0 = (int)g[6], k1 = (int)g[7];
    const unsigned id = RENDER_LINE_ID0 + (unsigned)e;
    for (int k = k0 + (int)threadIdx.x; k <= k1; k += 256) {
        const float s = ((float)k + 0.5f - g[0]) / (g[2] - g[0]);   // screen-linear parameter of this step's pixel centre
        const int m = (int)floorf(g[1] + s * (g[3] - g[1]));         // nearest pixel on the minor axis
        const int i = d.line_axis[e] == 0 ? k : m, j = d.line_axis[e] == 0 ? m : k;
        if (i < 0 || i >= d.W || j < 0 || j >= d.H) continue;
        const size_t p = (size_t)j * d.W + i;
        if (SHADE) {
            if ((unsigned)d.key[p] == id) {
                d.rgb[3 * p] = d.box & 0xffu; d.rgb[3 * p + 1] = (d.box >> 8) & 0xffu; d.rgb[3 * p + 2] = (d.box >> 16) & 0xffu;
            }
        } else {
            const float t = 1.0f / (g[4] + s * (g[5] - g[4]));        // 1/z is linear on the screen
            if (!(t > d.zn)) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | id;
            if (key < d.key[p]) atomicMin(&d.key[p], key);
        }
    }
}

// per pixel: background colour where nothing won, the id image, covered (sphere) pixels
__global__ void __launch_bounds__(256) k_render_finish(RenderDev d) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = p < (size_t)d.W * d.H;
    bool sphere = false;
    if (in) {
        const unsigned long long k = d.key[p];
        const unsigned lo = (unsigned)k;
        if (k == ~0ull) {
            d.rgb[3 * p] = d.bg & 0xffu; d.rgb[3 * p + 1] = (d.bg >> 8) & 0xffu; d.rgb[3 * p + 2] = (d.bg >> 16) & 0xffu;
            if (d.ids) d.ids[p] = -1;
        } else if (lo >= RENDER_LINE_ID0) {
            if (d.ids) d.ids[p] = -2 - (int)(lo - RENDER_LINE_ID0);
        } else {
            sphere = true;
            if (d.ids) d.ids[p] = (int)lo;
        }
    }
    const unsigned long long c = __ballot(sphere);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&d.cnt[4], (unsigned long long)__popcll(c));
}

// Sort-last compositing: another layer of the same frame -- key and rgb planes of a renderer with the same parameters, drawn
// from other particles -- folded into this one: per pixel the smaller key wins and brings its colour.  Pure streaming, so every lane
// takes four pixels: two 16-byte key loads and one 12-byte rgb load per side, the colours chosen by byte masks, stores only where
// something changed.  The last lane walks the W H % 4 pixels of the tail one by one.
struct RenderRgb4 { unsigned a, b, c; };   // 4 pixels x 3 channels

__global__ void __launch_bounds__(256) k_render_merge(RenderDev d, const unsigned long long *__restrict__ key_in,
                                                      const unsigned char *__restrict__ rgb_in) {
    const size_t px = (size_t)d.W * d.H, groups = px >> 2;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g < groups) {
        ulonglong2 *mk = (ulonglong2 *)d.key + 2 * g;
        const ulonglong2 *ik = (const ulonglong2 *)key_in + 2 * g;
        ulonglong2 m0 = mk[0], m1 = mk[1];
        const ulonglong2 i0 = ik[0], i1 = ik[1];
        const bool t0 = i0.x < m0.x, t1 = i0.y < m0.y, t2 = i1.x < m1.x, t3 = i1.y < m1.y;
        if (!(t0 || t1 || t2 || t3)) return;
        if (t0 || t1) { if (t0) m0.x = i0.x; if (t1) m0.y = i0.y; mk[0] = m0; }
        if (t2 || t3) { if (t2) m1.x = i1.x; if (t3) m1.y = i1.y; mk[1] = m1; }
        RenderRgb4 *mc = (RenderRgb4 *)d.rgb + g;
        const RenderRgb4 in = ((const RenderRgb4 *)rgb_in)[g];
        RenderRgb4 c = *mc;
        // bytes 0-2 pixel 0, 3-5 pixel 1, 6-8 pixel 2, 9-11 pixel 3
        const unsigned ma = (t0 ? 0x00ffffffu : 0u) | (t1 ? 0xff000000u : 0u);
        const unsigned mb = (t1 ? 0x0000ffffu : 0u) | (t2 ? 0xffff0000u : 0u);
        const unsigned mcw = (t2 ? 0x000000ffu : 0u) | (t3 ? 0xffffff00u : 0u);
        c.a = (c.a & ~ma) | (in.a & ma);
        c.b = (c.b & ~mb) | (in.b & mb);
        c.c = (c.c & ~mcw) | (in.c & mcw);
        *mc = c;
    } else if (g == groups) {
        for (size_t p = groups << 2; p < px; ++p)
            if (key_in[p] < d.key[p]) {
                d.key[p] = key_in[p];
                d.rgb[3 * p] = rgb_in[3 * p]; d.rgb[3 * p + 1] = rgb_in[3 * p + 1]; d.rgb[3 * p + 2] = rgb_in[3 * p + 2];
            }
    }
}

static void l_render_splat(RenderDev &d) {
    if (d.n > 0) {
        hipLaunchKernelGGL(k_render_small<false>, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d);
        hipLaunchKernelGGL(k_render_large<false>, dim3(RENDER_LARGE_GRID), dim3(256), 0, d.stream, d);
    }
    if (d.draw_box) hipLaunchKernelGGL(k_render_lines<false>, dim3(12), dim3(256), 0, d.stream, d);
}
static void l_render_shade(RenderDev &d) {
    if (d.n > 0) {
        hipLaunchKernelGGL(k_render_small<true>, dim3(cdiv(d.n, 256)), dim3(256), 0, d.stream, d);
        hipLaunchKernelGGL(k_render_large<true>, dim3(RENDER_LARGE_GRID), dim3(256), 0, d.stream, d);
    }
    if (d.draw_box) hipLaunchKernelGGL(k_render_lines<true>, dim3(12), dim3(256), 0, d.stream, d);
    const size_t px = (size_t)d.W * d.H;
    hipLaunchKernelGGL(k_render_finish, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d);
}

// a layer folded in (both planes complete on the stream before the call); l_render_finish afterwards: the per-pixel pass of l_render_shade
// once more -- it leaves the colour of every keyed pixel alone, rewrites background and ids, and ADDS to cnt[4], which the caller clears
static void l_render_merge(RenderDev &d, const unsigned long long *key_in, const unsigned char *rgb_in) {
    const size_t px = (size_t)d.W * d.H, lanes = (px >> 2) + ((px & 3) ? 1 : 0);
    hipLaunchKernelGGL(k_render_merge, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, d.stream, d, key_in, rgb_in);
}
static void l_render_finish(RenderDev &d) {
    const size_t px = (size_t)d.W * d.H;
    hipLaunchKernelGGL(k_render_finish, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d);
}

static void register_render_launchers(Launch &L) {
    L.render_splat = l_render_splat;
    L.render_shade = l_render_shade;
    L.render_merge = l_render_merge;
    L.render_finish = l_render_finish;
}

#include "sph_render_mesh.hpp"
#include "sph_render_trace.hpp"
