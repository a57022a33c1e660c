// sph_render_mesh.hpp -- mesh rendering (an ordered list of triangle meshes -> one RGB frame): kernels and launchers; included at the end
// of sph_render.hpp inside the per-build namespace, whose camera helpers, box lines and k_render_finish it shares.  The image is defined in
// DESIGN.md 17, semantics in include/sph_hip.h (sph_render_mesh_begin), float64 restatement in tests/render_mesh_model.py.  Stands in for
// the reference's render.py + rendering_script.py (every .obj of a frame directory through a Blender scene -> render.png).
//
// Passes (one stream, no host read in between):
//   depth   one thread per triangle (global index g, mesh found by bisection of the mesh table): three gathered vertices into view
//           coordinates, put in one canonical order (lexicographic by view position), the three edge planes m = p x q of the ordered pairs,
//           the face plane N, the screen bounds of the projected vertices plus one pixel; then per pixel centre of the bounds the hit test
//           and an atomicMin of (float_bits(t) << 32 | g) after a plain load says it would lower the key.  Triangles whose bounds exceed
//           RENDER_LARGE_PX pixels go to a list that one workgroup per triangle walks.
//   shade   the same walk: the pixel whose final key carries g is written with plain stores.  Then the box lines and k_render_finish.
//
// Watertight by construction: an edge's plane is computed from its two vertices in the canonical order whichever triangle asks, and every
// operation of the set-up and of the edge functions is an explicit fma or a lone multiply / subtract that no contraction can change -- so
// the two triangles of a shared edge get the SAME bits for its edge function, in the small and large kernels and in both builds, and a
// pixel centre cannot be strictly outside both.  The same ordering makes depth a function of the triangle's vertex positions as a set:
// coincident triangles tie exactly, whatever their winding, and the smaller global index wins.
#pragma once

struct MeshVert { float x, y, z; int slot; };   // view coordinates (s, u, f) and the vertex's slot in the frame's vertex array
struct MeshTri {
    float m12[3], m02[3], m01[3];   // p1 x p2, p0 x p2, p0 x p1 of the ordered vertices
    float N[3], aN;                 // (p1 - p0) x (p2 - p0), p0 . N
    int slot[3];
    unsigned col;
    int smooth;
};
enum { MESH_OK = 0, MESH_NONFINITE = 1, MESH_DEGENERATE = 2, MESH_BAD_INDEX = 3, MESH_CULLED = 4 };

__device__ __forceinline__ void mesh_cross(const float *p, const float *q, float *o) {
    o[0] = __builtin_fmaf(p[1], q[2], -(p[2] * q[1]));
    o[1] = __builtin_fmaf(p[2], q[0], -(p[0] * q[2]));
    o[2] = __builtin_fmaf(p[0], q[1], -(p[1] * q[0]));
}
// d . m for the pixel ray d = (X, Y, 1)
__device__ __forceinline__ float mesh_plane(const float *m, float X, float Y) { return __builtin_fmaf(X, m[0], __builtin_fmaf(Y, m[1], m[2])); }

__device__ __forceinline__ MeshVert mesh_view(const RenderDev &d, const float *p, int slot) {
    const float vx = p[0] - d.E[0], vy = p[1] - d.E[1], vz = p[2] - d.E[2];
    MeshVert v;
    v.x = __builtin_fmaf(d.s[0], vx, __builtin_fmaf(d.s[1], vy, d.s[2] * vz));
    v.y = __builtin_fmaf(d.u[0], vx, __builtin_fmaf(d.u[1], vy, d.u[2] * vz));
    v.z = __builtin_fmaf(d.f[0], vx, __builtin_fmaf(d.f[1], vy, d.f[2] * vz));
    v.slot = slot;
    return v;
}
__device__ __forceinline__ bool mesh_before(const MeshVert &a, const MeshVert &b) {
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    if (a.z != b.z) return a.z < b.z;
    return a.slot < b.slot;
}
__device__ __forceinline__ void mesh_order(MeshVert &a, MeshVert &b) {
    if (mesh_before(b, a)) { const MeshVert t = a; a = b; b = t; }
}

// the mesh of global triangle g: the last record whose first triangle is <= g (empty meshes share their successor's start and lose)
__device__ __forceinline__ int mesh_of(const MeshDev &m, long long g) {
    int lo = 0, hi = m.nm - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (m.rec[mid].t0 <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// set-up of triangle g; MESH_OK: T and the pixel bounds b are valid
__device__ __forceinline__ int mesh_setup(const RenderDev &d, const MeshDev &m, long long g, MeshTri &T, RenderBox &b) {
    const MeshRec rec = m.rec[mesh_of(m, g)];
    MeshVert v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = m.tri[3 * g + k];
        if (i < 0 || i >= rec.nv) return MESH_BAD_INDEX;
        const long long slot = rec.v0 + i;
        const float p[3] = {m.vert[3 * slot], m.vert[3 * slot + 1], m.vert[3 * slot + 2]};
        if (render_bad(p[0]) || render_bad(p[1]) || render_bad(p[2])) return MESH_NONFINITE;
        v[k] = mesh_view(d, p, (int)slot);
    }
    mesh_order(v[0], v[1]); mesh_order(v[1], v[2]); mesh_order(v[0], v[1]);
    const float p0[3] = {v[0].x, v[0].y, v[0].z}, p1[3] = {v[1].x, v[1].y, v[1].z}, p2[3] = {v[2].x, v[2].y, v[2].z};
    // two corners at one position (neighbours in the order): zero area exactly, while the fma of the cross product would leave rounding dust
    if ((p0[0] == p1[0] && p0[1] == p1[1] && p0[2] == p1[2]) || (p1[0] == p2[0] && p1[1] == p2[1] && p1[2] == p2[2])) return MESH_DEGENERATE;
    const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    mesh_cross(e1, e2, T.N);
    if (render_bad(T.N[0]) || render_bad(T.N[1]) || render_bad(T.N[2])) return MESH_NONFINITE;   // (finite vertices, overflowing products)
    if (T.N[0] == 0.0f && T.N[1] == 0.0f && T.N[2] == 0.0f) return MESH_DEGENERATE;
    T.aN = __builtin_fmaf(p0[0], T.N[0], __builtin_fmaf(p0[1], T.N[1], p0[2] * T.N[2]));
    mesh_cross(p1, p2, T.m12); mesh_cross(p0, p2, T.m02); mesh_cross(p0, p1, T.m01);
    T.slot[0] = v[0].slot; T.slot[1] = v[1].slot; T.slot[2] = v[2].slot;
    T.col = rec.col; T.smooth = rec.smooth;
    // bounds: every point of the triangle has a view depth between its vertices'
    const float zmax = fmaxf(p0[2], fmaxf(p1[2], p2[2])), zmin = fminf(p0[2], fminf(p1[2], p2[2]));
    if (!(zmax > d.zn)) return MESH_CULLED;
    float c0 = -1.0f, c1 = (float)d.W, r0 = -1.0f, r1 = (float)d.H;   // a vertex not in front of the near plane: the whole screen
    if (zmin > d.zn) {
        const float lim = 4.0f * (float)(d.W > d.H ? d.W : d.H);
        const float ca = render_col(d, p0[0] / p0[2]), cb = render_col(d, p1[0] / p1[2]), cc = render_col(d, p2[0] / p2[2]);
        const float ra = render_row(d, p0[1] / p0[2]), rb = render_row(d, p1[1] / p1[2]), rc = render_row(d, p2[1] / p2[2]);
        c0 = fminf(fmaxf(fminf(ca, fminf(cb, cc)), -lim), lim); c1 = fminf(fmaxf(fmaxf(ca, fmaxf(cb, cc)), -lim), lim);
        r0 = fminf(fmaxf(fminf(ra, fminf(rb, rc)), -lim), lim); r1 = fminf(fmaxf(fmaxf(ra, fmaxf(rb, rc)), -lim), lim);
    }
    b.i0 = max((int)ceilf(c0 - 1.0f), 0); b.i1 = min((int)floorf(c1 + 1.0f), d.W - 1);
    b.j0 = max((int)ceilf(r0 - 1.0f), 0); b.j1 = min((int)floorf(r1 + 1.0f), d.H - 1);
    return b.i0 <= b.i1 && b.j0 <= b.j1 ? MESH_OK : MESH_CULLED;
}

// unit normal of the face plane (scaled first: the squares of a tiny N would underflow)
__device__ __forceinline__ void mesh_flat_normal(const MeshTri &T, float *n) {
    const float s = fmaxf(fabsf(T.N[0]), fmaxf(fabsf(T.N[1]), fabsf(T.N[2])));
    const float x = T.N[0] / s, y = T.N[1] / s, z = T.N[2] / s;
    const float l = sqrtf(x * x + y * y + z * z);
    n[0] = x / l; n[1] = y / l; n[2] = z / l;
}

// the colour of triangle T at pixel ray (X, Y, 1), depth t: flat or blended normal, turned to the viewer, ambient + Lambert
__device__ __forceinline__ void mesh_shade_px(const RenderDev &d, const MeshDev &m, const MeshTri &T, float X, float Y, float t,
                                              unsigned char *out) {
    float n[3];
    bool have = false;
    if (T.smooth) {   // weights: the edge function opposite each ordered vertex (one sign inside the triangle)
        const float w0 = mesh_plane(T.m12, X, Y), w1 = -mesh_plane(T.m02, X, Y), w2 = mesh_plane(T.m01, X, Y);
        const float *a = m.nrm + 3 * (size_t)T.slot[0], *b = m.nrm + 3 * (size_t)T.slot[1], *c = m.nrm + 3 * (size_t)T.slot[2];
        const float bx = w0 * a[0] + w1 * b[0] + w2 * c[0], by = w0 * a[1] + w1 * b[1] + w2 * c[1], bz = w0 * a[2] + w1 * b[2] + w2 * c[2];
        const float s = fmaxf(fabsf(bx), fmaxf(fabsf(by), fabsf(bz)));
        if (s > 0.0f && !render_bad(s) && !render_bad(bx) && !render_bad(by) && !render_bad(bz)) {
            const float wx = bx / s, wy = by / s, wz = bz / s;
            const float vx = d.s[0] * wx + d.s[1] * wy + d.s[2] * wz, vy = d.u[0] * wx + d.u[1] * wy + d.u[2] * wz,
                        vz = d.f[0] * wx + d.f[1] * wy + d.f[2] * wz;
            const float l = sqrtf(vx * vx + vy * vy + vz * vz);
            if (l > 0.0f) { n[0] = vx / l; n[1] = vy / l; n[2] = vz / l; have = true; }
        }
    }
    if (!have) mesh_flat_normal(T, n);
    if (n[0] * X + n[1] * Y + n[2] > 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    const float lx = d.light[0] - t * X, ly = d.light[1] - t * Y, lz = d.light[2] - t;
    const float ln = sqrtf(lx * lx + ly * ly + lz * lz);
    const float ndl = fmaxf((n[0] * lx + n[1] * ly + n[2] * lz) / ln, 0.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float base = (float)((T.col >> (8 * c)) & 0xffu) / 255.0f;
        out[c] = render_byte(base * (d.amb + ndl * d.lrgb[c]));
    }
}

// one pixel of one triangle: depth lowers the key (counting the atomics issued), SHADE writes the colour where the key is this triangle's
template <bool SHADE>
__device__ __forceinline__ void mesh_pixel(const RenderDev &d, const MeshDev &m, const MeshTri &T, int i, int j, unsigned g, unsigned &issued,
                                           bool &hit) {
    const float X = render_X(d, i), Y = render_Y(d, j);
    const size_t p = (size_t)j * d.W + i;
    if (SHADE) {
        const unsigned long long k = d.key[p];
        if ((unsigned)k == g) mesh_shade_px(d, m, T, X, Y, __uint_as_float((unsigned)(k >> 32)), d.rgb + 3 * p);
    } else {
        const float a = mesh_plane(T.m12, X, Y), b = mesh_plane(T.m02, X, Y), c = mesh_plane(T.m01, X, Y);   // b: of p0 x p2, sign reversed
        if (!((a >= 0.0f && b <= 0.0f && c >= 0.0f) || (a <= 0.0f && b >= 0.0f && c <= 0.0f))) return;
        const float t = T.aN / mesh_plane(T.N, X, Y);
        if (!(t > d.zn) || render_bad(t)) return;
        hit = true;
        const unsigned long long k = ((unsigned long long)__float_as_uint(t) << 32) | g;
        if (k < d.key[p]) { atomicMin(&d.key[p], k); ++issued; }
    }
}

// one thread per triangle; large ones are listed (depth) or left to the large pass (shade)
template <bool SHADE>
__global__ void __launch_bounds__(256) k_mesh_small(RenderDev d, MeshDev m) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned issued = 0;
    bool hit = false;
    int st = MESH_CULLED;
    if (g < m.nt) {
        MeshTri T;
        RenderBox b;
        st = mesh_setup(d, m, g, T, b);
        if (st == MESH_OK) {
            if ((b.i1 - b.i0 + 1) * (b.j1 - b.j0 + 1) > RENDER_LARGE_PX) {
                if (!SHADE) m.large[atomicAdd(&d.cnt[2], 1ull)] = (unsigned)g;
            } else {
                for (int j = b.j0; j <= b.j1; ++j)
                    for (int x = b.i0; x <= b.i1; ++x) mesh_pixel<SHADE>(d, m, T, x, j, (unsigned)g, issued, hit);
            }
        }
    }
    if (SHADE) return;
    // counters: summed per wave, then per workgroup in LDS, so that one atomic per workgroup and counter reaches the shared line of d.cnt
    // (one per wave made the pass wait on that line: profiles/render_mesh_rocprofv3_c2_summary.txt)
    __shared__ unsigned sh[5];
    if (threadIdx.x < 5) sh[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned long long h = __ballot(hit), nf = __ballot(st == MESH_NONFINITE), dg = __ballot(st == MESH_DEGENERATE),
                             bi = __ballot(st == MESH_BAD_INDEX);
    issued = render_wave_sum(issued);
    if ((threadIdx.x & 63) == 0) {
        if (h) atomicAdd(&sh[0], (unsigned)__popcll(h));
        if (nf) atomicAdd(&sh[1], (unsigned)__popcll(nf));
        if (issued) atomicAdd(&sh[2], issued);
        if (dg) atomicAdd(&sh[3], (unsigned)__popcll(dg));
        if (bi) atomicAdd(&sh[4], (unsigned)__popcll(bi));
    }
    __syncthreads();
    if (threadIdx.x < 5 && sh[threadIdx.x]) {
        const int slot = threadIdx.x == 0 ? 0 : threadIdx.x == 1 ? 1 : threadIdx.x == 2 ? 3 : threadIdx.x == 3 ? 5 : 6;
        atomicAdd(&d.cnt[slot], (unsigned long long)sh[threadIdx.x]);
    }
}

// one workgroup per listed triangle: its 256 threads stride over the bounds' pixels (every thread repeats the set-up: same bits)
template <bool SHADE>
__global__ void __launch_bounds__(256) k_mesh_large(RenderDev d, MeshDev m) {
    const long long nl = (long long)d.cnt[2];
    unsigned issued = 0;
    for (long long k = blockIdx.x; k < nl; k += gridDim.x) {
        const unsigned g = m.large[k];
        MeshTri T;
        RenderBox b;
        bool hit = false;
        if (mesh_setup(d, m, (long long)g, T, b) == MESH_OK) {
            const int bw = b.i1 - b.i0 + 1, np = bw * (b.j1 - b.j0 + 1);
            for (int q = threadIdx.x; q < np; q += 256) mesh_pixel<SHADE>(d, m, T, b.i0 + q % bw, b.j0 + q / bw, g, issued, hit);
        }
        if (!SHADE) {
            const int any = __syncthreads_or(hit ? 1 : 0);
            if (threadIdx.x == 0 && any) atomicAdd(&d.cnt[0], 1ull);
        }
    }
    if (SHADE) return;
    issued = render_wave_sum(issued);
    if ((threadIdx.x & 63) == 0 && issued) atomicAdd(&d.cnt[3], (unsigned long long)issued);
}

static void l_render_mesh_depth(RenderDev &d, MeshDev &m) {
    if (m.nt > 0) {
        hipLaunchKernelGGL(k_mesh_small<false>, dim3((unsigned)((m.nt + 255) / 256)), dim3(256), 0, d.stream, d, m);
        hipLaunchKernelGGL(k_mesh_large<false>, dim3(RENDER_LARGE_GRID), dim3(256), 0, d.stream, d, m);
    }
    if (d.draw_box) hipLaunchKernelGGL(k_render_lines<false>, dim3(12), dim3(256), 0, d.stream, d);
}
static void l_render_mesh_shade(RenderDev &d, MeshDev &m) {
    if (m.nt > 0) {
        hipLaunchKernelGGL(k_mesh_small<true>, dim3((unsigned)((m.nt + 255) / 256)), dim3(256), 0, d.stream, d, m);
        hipLaunchKernelGGL(k_mesh_large<true>, dim3(RENDER_LARGE_GRID), dim3(256), 0, d.stream, d, m);
    }
    if (d.draw_box) hipLaunchKernelGGL(k_render_lines<true>, dim3(12), dim3(256), 0, d.stream, d);
}
static void l_render_mesh_finish(RenderDev &d) {
    const size_t px = (size_t)d.W * d.H;
    hipLaunchKernelGGL(k_render_finish, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d);
}

static void register_render_mesh_launchers(Launch &L) {
    L.render_mesh_depth = l_render_mesh_depth;
    L.render_mesh_shade = l_render_mesh_shade;
    L.render_mesh_finish = l_render_mesh_finish;
}
