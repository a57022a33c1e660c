// sph_render_trace.hpp -- traced mesh frames (an ordered list of triangle meshes -> one RGB frame with shadows and refracting water):
// kernels and launchers; included behind sph_render_mesh.hpp by sph_render.hpp, inside the per-build namespace, whose camera helpers, box lines and
// mesh table it shares.  The image is defined in DESIGN.md 30, semantics in include/sph_hip.h (sph_render_set_trace).
//
// Stages (one stream, no host read in between; n, the number of kept triangles, is read from the counters on the device):
//   set-up     one thread per triangle: three gathered world corners in one canonical order (lexicographic by position), the triangles
//              mesh_setup would skip left out and counted, the centroids' bounds by integer atomicMin / atomicMax of an order-keeping
//              code; then the key morton30(centroid) << 32 | g.
//   sort       LSD radix sort, 8 bits a pass, over the code bits alone: the keys start in the order of g, the passes are stable, so the
//              result is the order of the whole 64-bit key.  Keys are distinct, so the hierarchy's depth is at most 64 whatever the input.
//   hierarchy  Karras 2012, one thread per inner node.
//   fit        one thread per leaf climbs: the first arrival at an inner node leaves, the second unites the two boxes and goes on.  The
//              hand-off crosses workgroups, CUs and XCDs (an XCD's L2 is not coherent with another's, a CU's L1 with nobody's): the
//              arriving thread releases at AGENT scope before its counter atomic, the second arrival acquires at AGENT scope after it and
//              reads the sibling's box with agent-scope loads.  min / max do not round: every box is the exact union of its children.
//              Then the skip links (where a ray goes when it is done with a subtree) and the depth, one thread per node.
//   shade      one thread per pixel, one path of at most max_depth segments, no recursion: closest hit per segment, any hit per shadow
//              ray, both without a stack (left child first, then the skip link) and under a visit cap of 2 nt nodes.
//   finish     the box lines by depth against the primary hit (k_render_lines), the id image.
// No loop waits on another thread: every bound follows from the data (64 levels, 2 nt visits, max_depth segments).
//
// Culling never changes the winner, by construction: a triangle is hit only if the ray passes the slab test of the
// triangle's OWN box, the same routine that tests the nodes, and its t is clamped into that test's [t_near, t_far].  The triangle test is
// conservative (edge functions inside down to minus their error bound, the box widened): a ray that meets the exact triangle is never refused.  Subtraction, the
// multiplication by one fixed reciprocal, min and max are monotone in floating point, so a box that contains another yields t_near not
// larger and t_far not smaller, bit for bit: whatever rejects an enclosing node rejects every triangle below it.
#pragma once

struct TV3 { float x, y, z; };
__device__ __forceinline__ TV3 tv3(float x, float y, float z) { TV3 v; v.x = x; v.y = y; v.z = z; return v; }
__device__ __forceinline__ TV3 tv_sub(TV3 a, TV3 b) { return tv3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float tv_dot(TV3 a, TV3 b) { return __builtin_fmaf(a.x, b.x, __builtin_fmaf(a.y, b.y, a.z * b.z)); }
__device__ __forceinline__ TV3 tv_cross(TV3 p, TV3 q) {
    return tv3(__builtin_fmaf(p.y, q.z, -(p.z * q.y)), __builtin_fmaf(p.z, q.x, -(p.x * q.z)), __builtin_fmaf(p.x, q.y, -(p.y * q.x)));
}
__device__ __forceinline__ TV3 tv_at(TV3 o, float t, TV3 d) { return tv3(__builtin_fmaf(t, d.x, o.x), __builtin_fmaf(t, d.y, o.y), __builtin_fmaf(t, d.z, o.z)); }
__device__ __forceinline__ bool tv_bad(TV3 a) { return render_bad(a.x) || render_bad(a.y) || render_bad(a.z); }
// a / |a|, scaled first (the squares of a tiny vector would underflow); false: zero or non-finite
__device__ __forceinline__ bool tv_unit(TV3 a, TV3 &n) {
    const float s = fmaxf(fabsf(a.x), fmaxf(fabsf(a.y), fabsf(a.z)));
    if (!(s > 0.0f) || render_bad(s) || tv_bad(a)) return false;
    const TV3 b = tv3(a.x / s, a.y / s, a.z / s);
    const float l = sqrtf(tv_dot(b, b));
    n = tv3(b.x / l, b.y / l, b.z / l);
    return true;
}

// floats in an unsigned code that keeps their order
__device__ __forceinline__ unsigned trace_code(float f) { const unsigned b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float trace_uncode(unsigned c) { return __uint_as_float((c & 0x80000000u) ? (c & 0x7fffffffu) : ~c); }

__device__ __forceinline__ bool trace_before(const float4 &a, const float4 &b) {
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    if (a.z != b.z) return a.z < b.z;
    return __float_as_int(a.w) < __float_as_int(b.w);
}
__device__ __forceinline__ void trace_order(float4 &a, float4 &b, int &odd) {
    if (trace_before(b, a)) { const float4 t = a; a = b; b = t; odd ^= 1; }
}

__device__ __forceinline__ unsigned trace_wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned trace_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// --- set-up ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_trace_setup(MeshDev m, TraceDev t) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    int st = MESH_CULLED;   // (beyond the list)
    unsigned lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
    if (g < m.nt) {
        const int mi = mesh_of(m, g);
        const MeshRec rec = m.rec[mi];
        float4 c[3];
        st = MESH_OK;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = m.tri[3 * g + k];
            if (i < 0 || i >= rec.nv) { st = MESH_BAD_INDEX; break; }
            const long long slot = rec.v0 + i;
            c[k] = make_float4(m.vert[3 * slot], m.vert[3 * slot + 1], m.vert[3 * slot + 2], __int_as_float((int)slot));
            if (render_bad(c[k].x) || render_bad(c[k].y) || render_bad(c[k].z)) { st = MESH_NONFINITE; break; }
        }
        int odd = 0;
        if (st == MESH_OK) {
            trace_order(c[0], c[1], odd); trace_order(c[1], c[2], odd); trace_order(c[0], c[1], odd);
            if ((c[0].x == c[1].x && c[0].y == c[1].y && c[0].z == c[1].z) || (c[1].x == c[2].x && c[1].y == c[2].y && c[1].z == c[2].z))
                st = MESH_DEGENERATE;
        }
        if (st == MESH_OK) {
            const TV3 p0 = tv3(c[0].x, c[0].y, c[0].z), p1 = tv3(c[1].x, c[1].y, c[1].z), p2 = tv3(c[2].x, c[2].y, c[2].z);
            const TV3 N = tv_cross(tv_sub(p1, p0), tv_sub(p2, p0));
            if (tv_bad(N)) st = MESH_NONFINITE;
            else if (N.x == 0.0f && N.y == 0.0f && N.z == 0.0f) st = MESH_DEGENERATE;
        }
        if (st == MESH_OK) {
            t.corner[3 * g] = c[0]; t.corner[3 * g + 1] = c[1]; t.corner[3 * g + 2] = c[2];
            t.st[g] = (mi << 1) | odd;
            const float q = 1.0f / 3.0f;
            const float cx = (c[0].x + c[1].x + c[2].x) * q, cy = (c[0].y + c[1].y + c[2].y) * q, cz = (c[0].z + c[1].z + c[2].z) * q;
            lo[0] = hi[0] = trace_code(cx); lo[1] = hi[1] = trace_code(cy); lo[2] = hi[2] = trace_code(cz);
        } else
            t.st[g] = -1;
    }
    __shared__ unsigned sh[4], sb[6];
    if (threadIdx.x < 4) sh[threadIdx.x] = 0u;
    if (threadIdx.x < 6) sb[threadIdx.x] = threadIdx.x < 3 ? ~0u : 0u;
    __syncthreads();
    const unsigned long long ok = __ballot(st == MESH_OK), nf = __ballot(st == MESH_NONFINITE), dg = __ballot(st == MESH_DEGENERATE),
                             bi = __ballot(st == MESH_BAD_INDEX);
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = trace_wave_min(lo[k]); hi[k] = trace_wave_max(hi[k]); }
    if ((threadIdx.x & 63) == 0) {
        if (ok) atomicAdd(&sh[0], (unsigned)__popcll(ok));
        if (nf) atomicAdd(&sh[1], (unsigned)__popcll(nf));
        if (dg) atomicAdd(&sh[2], (unsigned)__popcll(dg));
        if (bi) atomicAdd(&sh[3], (unsigned)__popcll(bi));
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { atomicMin(&sb[k], lo[k]); atomicMax(&sb[3 + k], hi[k]); }
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && sh[threadIdx.x]) atomicAdd(&t.ctr[TC_KEPT + threadIdx.x], (unsigned long long)sh[threadIdx.x]);
    if (threadIdx.x < 6 && sh[0]) {
        if (threadIdx.x < 3) atomicMin(&t.bnd[threadIdx.x], sb[threadIdx.x]); else atomicMax(&t.bnd[threadIdx.x], sb[threadIdx.x]);
    }
}

// 10 bits -> every third bit
__device__ __forceinline__ unsigned trace_spread(unsigned v) {
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ unsigned trace_cell(float c, float lo, float hi) {
    if (!(hi > lo)) return 0u;
    const float q = (c - lo) / (hi - lo) * 1024.0f;
    return (unsigned)fminf(fmaxf(q, 0.0f), 1023.0f);
}

__global__ void __launch_bounds__(256) k_trace_keys(MeshDev m, TraceDev t) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= m.nt) return;
    unsigned code = 0x40000000u;
    if (t.st[g] >= 0) {
        const float4 a = t.corner[3 * g], b = t.corner[3 * g + 1], c = t.corner[3 * g + 2];
        const float q = 1.0f / 3.0f;
        const float cx = (a.x + b.x + c.x) * q, cy = (a.y + b.y + c.y) * q, cz = (a.z + b.z + c.z) * q;   // (the set-up's expression: inside the bounds)
        const unsigned ix = trace_cell(cx, trace_uncode(t.bnd[0]), trace_uncode(t.bnd[3])), iy = trace_cell(cy, trace_uncode(t.bnd[1]), trace_uncode(t.bnd[4])),
                       iz = trace_cell(cz, trace_uncode(t.bnd[2]), trace_uncode(t.bnd[5]));
        code = (trace_spread(ix) << 2) | (trace_spread(iy) << 1) | trace_spread(iz);
    }
    t.key[0][g] = ((unsigned long long)code << 32) | (unsigned long long)(unsigned)g;
}

// --- sort: one 8-bit pass = count per tile, scan over the tiles, stable scatter ---------------------------------------------------------
__global__ void __launch_bounds__(256) k_trace_sort_count(TraceDev t, long long nt, int pass, int shift) {
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned long long *in = t.key[pass & 1];
    const long long base = (long long)blockIdx.x * TRACE_SORT_TILE;
    for (int q = threadIdx.x; q < TRACE_SORT_TILE; q += 256) {
        const long long i = base + q;
        if (i < nt) atomicAdd(&h[(unsigned)(in[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    t.hist[(size_t)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

// one workgroup, thread = digit: the counts of its digit become exclusive over the tiles; the digits' bases go to the row behind the last tile
__global__ void __launch_bounds__(256) k_trace_sort_scan(TraceDev t, int tiles) {
    __shared__ unsigned tot[256];
    unsigned run = 0u;
    for (int b = 0; b < tiles; ++b) {
        const size_t k = (size_t)b * 256 + threadIdx.x;
        const unsigned c = t.hist[k];
        t.hist[k] = run;
        run += c;
    }
    tot[threadIdx.x] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0u;
        for (int d = 0; d < 256; ++d) { const unsigned c = tot[d]; tot[d] = s; s += c; }
    }
    __syncthreads();
    t.hist[(size_t)tiles * 256 + threadIdx.x] = tot[threadIdx.x];
}

// the tile's keys in chunks of 256, in order: a key's place is its digit's running offset + the keys of that digit in the waves before
// its own + those in the lanes before its own (the lanes that agree on all eight digit bits: eight ballots)
__global__ void __launch_bounds__(256) k_trace_sort_scatter(TraceDev t, long long nt, int tiles, int pass, int shift) {
    __shared__ unsigned off[256], wc[4][256];
    const unsigned long long *in = t.key[pass & 1];
    unsigned long long *out = t.key[1 - (pass & 1)];
    off[threadIdx.x] = t.hist[(size_t)tiles * 256 + threadIdx.x] + t.hist[(size_t)blockIdx.x * 256 + threadIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) wc[w][threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * TRACE_SORT_TILE;
    for (int q = 0; q < TRACE_SORT_TILE; q += 256) {   // (uniform: every thread runs every chunk and meets every barrier)
        const long long i = base + q + threadIdx.x;
        const bool valid = i < nt;
        const unsigned long long key = valid ? in[i] : 0ull;
        const unsigned dg = (unsigned)(key >> shift) & 255u;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bb = __ballot((dg >> b) & 1u);
            same &= ((dg >> b) & 1u) ? bb : ~bb;
        }
        const unsigned before = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && before == 0u) wc[wave][dg] = (unsigned)__popcll(same);
        __syncthreads();
        if (valid) {
            unsigned pos = off[dg] + before;
            for (int w = 0; w < wave; ++w) pos += wc[w][dg];
            if (pos < (unsigned long long)nt) out[pos] = key;   // (a permutation by construction; the guard keeps a bug inside the buffer)
        }
        __syncthreads();
        off[threadIdx.x] += wc[0][threadIdx.x] + wc[1][threadIdx.x] + wc[2][threadIdx.x] + wc[3][threadIdx.x];
#pragma unroll
        for (int w = 0; w < 4; ++w) wc[w][threadIdx.x] = 0u;
        __syncthreads();
    }
}

// --- hierarchy (Karras 2012) ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int trace_delta(const unsigned long long *k, long long n, long long i, long long j) {
    if (j < 0 || j >= n) return -1;
    return __clzll((long long)(k[i] ^ k[j]));   // (distinct keys: never 64)
}

__global__ void __launch_bounds__(256) k_trace_hierarchy(MeshDev m, TraceDev t) {
    const long long n = (long long)t.ctr[TC_KEPT];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && n >= 1) t.parent[0] = -1;
    if (n > m.nt || i >= n - 1) return;
    const unsigned long long *k = t.key[0];
    const int d = trace_delta(k, n, i, i + 1) > trace_delta(k, n, i, i - 1) ? 1 : -1;
    const int dmin = trace_delta(k, n, i, i - d);
    long long lmax = 2;
    for (int it = 0; it < 40 && trace_delta(k, n, i, i + lmax * d) > dmin; ++it) lmax <<= 1;
    long long l = 0;
    for (long long s = lmax >> 1; s >= 1; s >>= 1)
        if (trace_delta(k, n, i, i + (l + s) * d) > dmin) l += s;
    const long long j = i + l * d;
    const int dnode = trace_delta(k, n, i, j);
    long long s = 0, q = l;
    for (int it = 0; it < 64; ++it) {
        q = (q + 1) >> 1;
        if (trace_delta(k, n, i, i + (s + q) * d) > dnode) s += q;
        if (q <= 1) break;
    }
    const long long gamma = i + s * d + (d < 0 ? -1 : 0);
    const long long lo = i < j ? i : j, hi = i < j ? j : i;
    const int L = (int)(lo == gamma ? n - 1 + gamma : gamma), R = (int)(hi == gamma + 1 ? n - 1 + gamma + 1 : gamma + 1);
    if (L < 1 || R < 1 || L >= 2 * n - 1 || R >= 2 * n - 1) return;   // (never for sorted distinct keys; a bug stays inside the buffers)
    t.left[i] = L; t.right[i] = R;
    t.parent[L] = (int)i; t.parent[R] = (int)i;
}

// --- fit ----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float trace_load_agent(const float *p) {
    return __uint_as_float(__hip_atomic_load((const unsigned *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

__global__ void __launch_bounds__(256) k_trace_fit(MeshDev m, TraceDev t) {
    const long long n = (long long)t.ctr[TC_KEPT];
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n > m.nt || j >= n) return;
    const unsigned g = (unsigned)t.key[0][j];
    if ((long long)g >= m.nt) return;
    const float4 a = t.corner[3 * (size_t)g], b = t.corner[3 * (size_t)g + 1], c = t.corner[3 * (size_t)g + 2];
    float lx = fminf(a.x, fminf(b.x, c.x)), ly = fminf(a.y, fminf(b.y, c.y)), lz = fminf(a.z, fminf(b.z, c.z));
    float hx = fmaxf(a.x, fmaxf(b.x, c.x)), hy = fmaxf(a.y, fmaxf(b.y, c.y)), hz = fmaxf(a.z, fmaxf(b.z, c.z));
    int node = (int)(n - 1 + j);
    for (int level = 0; level < 66; ++level) {   // (at most 64 levels: the keys are 64 distinct bit strings)
        float *bx = t.box + 6 * (size_t)node;
        bx[0] = lx; bx[1] = ly; bx[2] = lz; bx[3] = hx; bx[4] = hy; bx[5] = hz;
        const int p = t.parent[node];
        if (p < 0 || p >= n - 1) return;
        // publish the box to whoever arrives second, on any XCD: agent-scope release, its wait, then the counter.  The explicit
        // s_waitcnt behind each fence is deliberate: the compiler has been seen to drop a fence's own wait when a waited load or
        // a used atomic stands before it, and a box published a moment late is a wrong box, silently
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = atomicAdd(&t.arrive[p], 1);
        if (old != 1) return;   // first arrival (0) leaves; anything else would be a bug: leave as well
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int Lc = t.left[p], Rc = t.right[p];
        const int sib = Lc == node ? Rc : Lc;
        if (sib < 0 || sib >= 2 * n - 1) return;
        const float *sx = t.box + 6 * (size_t)sib;
        lx = fminf(lx, trace_load_agent(sx)); ly = fminf(ly, trace_load_agent(sx + 1)); lz = fminf(lz, trace_load_agent(sx + 2));
        hx = fmaxf(hx, trace_load_agent(sx + 3)); hy = fmaxf(hy, trace_load_agent(sx + 4)); hz = fmaxf(hz, trace_load_agent(sx + 5));
        node = p;
    }
}

// per node: the skip link (the right sibling of the nearest ancestor-or-self that is a left child); per leaf: its depth
__global__ void __launch_bounds__(256) k_trace_links(MeshDev m, TraceDev t) {
    const long long n = (long long)t.ctr[TC_KEPT];
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    int depth = 0;
    if (n <= m.nt && x < 2 * n - 1) {
        int c = (int)x, skip = -1;
        bool found = false;
        for (int level = 0; level < 66; ++level) {
            const int p = t.parent[c];
            if (p < 0 || p >= n - 1) break;
            if (!found && t.left[p] == c) { skip = t.right[p]; found = true; }
            c = p;
            ++depth;
        }
        t.skip[x] = skip;
    }
    depth = (int)trace_wave_max((unsigned)depth);
    if ((threadIdx.x & 63) == 0 && depth) atomicMax(&t.ctr[TC_DEPTH], (unsigned long long)depth);
}

// --- rays ---------------------------------------------------------------------------------------------------------------------------------
struct TraceRay {
    TV3 O, d, inv;      // inv: 1 / d per axis; an axis with d = 0 (or a reciprocal that is not finite) is tested by containment
    float tmin;         // a hit needs t > tmin
    unsigned self;      // the id the ray starts on (never hit), ~0u: none
};
struct TraceCount { unsigned visits, tests, aborted; };

__device__ __forceinline__ TraceRay trace_ray(TV3 O, TV3 d, float tmin, unsigned self) {
    TraceRay r;
    r.O = O; r.d = d; r.tmin = tmin; r.self = self;
    r.inv = tv3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    return r;
}

__device__ __forceinline__ void trace_slab_axis(float lo, float hi, float o, float inv, float &tn, float &tf) {
    if (fabsf(inv) <= 3.0e38f) {
        // the box seen from the origin, widened by 2^-21 of each distance (more than the u of the corners' own P - O in trace_tri)
        const float l = lo - o, h = hi - o;
        const float a = __builtin_fmaf(-fabsf(l), 4.8e-7f, l) * inv, b = __builtin_fmaf(fabsf(h), 4.8e-7f, h) * inv;
        tn = fmaxf(tn, fminf(a, b)); tf = fminf(tf, fmaxf(a, b));
    } else {
        const float l = lo - o, h = hi - o;
        if (!(__builtin_fmaf(-fabsf(l), 4.8e-7f, l) <= 0.0f && 0.0f <= __builtin_fmaf(fabsf(h), 4.8e-7f, h))) { tn = INFINITY; tf = -INFINITY; }
    }
}
// the slab test of box [lo, hi]: [tn, tf] with tf padded upwards (Ize 2013); every operation is monotone in lo (downwards) and hi
__device__ __forceinline__ bool trace_slab(const TraceRay &r, float lx, float ly, float lz, float hx, float hy, float hz, float &tn, float &tf) {
    tn = -INFINITY; tf = INFINITY;
    trace_slab_axis(lx, hx, r.O.x, r.inv.x, tn, tf);
    trace_slab_axis(ly, hy, r.O.y, r.inv.y, tn, tf);
    trace_slab_axis(lz, hz, r.O.z, r.inv.z, tn, tf);
    tf = __builtin_fmaf(fabsf(tf), 4.0e-7f, tf);
    return tn <= tf && tf > r.tmin;
}

// an edge function d . (p x q) and a bound of its rounding error: each component of the cross product is one multiplication and one fma
// (<= 2 u (|p_j q_k| + |p_k q_j|)), the dot product one multiplication and two fmas (<= 3 u sum |d_i m_i|, and |m_i| is itself at most the
// bracket): |error| <= 5 u sum_i |d_i| (|p_j q_k| + |p_k q_j|); 8 u is taken (u = 2^-24: 4.8e-7)
__device__ __forceinline__ float trace_edge(TV3 d, TV3 p, TV3 q, float &eps) {
    const float ax = __builtin_fmaf(fabsf(p.y), fabsf(q.z), fabsf(p.z) * fabsf(q.y)), ay = __builtin_fmaf(fabsf(p.z), fabsf(q.x), fabsf(p.x) * fabsf(q.z)),
                az = __builtin_fmaf(fabsf(p.x), fabsf(q.y), fabsf(p.y) * fabsf(q.x));
    eps = 4.8e-7f * __builtin_fmaf(fabsf(d.x), ax, __builtin_fmaf(fabsf(d.y), ay, fabsf(d.z) * az));
    return tv_dot(d, tv_cross(p, q));
}

// triangle g against the ray: its own box's slab test, the three edge functions about the ray's origin (each from its edge's two corners
// in the canonical order: the same bits for both triangles of a shared edge), t = ((p0 - O) . N) / (d . N) clamped into the slab's range.
// Conservative: an edge function counts as inside down to minus its own error bound, and the box is widened by more than the rounding of
// the corners, so a ray that meets the exact triangle is never refused -- no ray passes between two triangles of a closed mesh, whatever
// the boxes' faces.  Near an edge both neighbours may accept; a SOFT hit (inside only by the bound) yields to the closest
// hard one unless it lies in front of it by more than 2^-12 of its t (trace_pick): the neighbour whose edge functions hold the ray by
// sign keeps the hit, as in section 17, and a path goes on from the triangle it really left through.
template <bool ANY>
__device__ __forceinline__ bool trace_tri(const MeshDev &m, const TraceDev &t, const TraceRay &r, unsigned g, float &th, bool &soft) {
    if (g == r.self) return false;
    const int st = t.st[g];
    if (st < 0) return false;
    if (ANY && (m.rec[st >> 1].mat & 1)) return false;   // water does not block light
    const float4 a = t.corner[3 * (size_t)g], b = t.corner[3 * (size_t)g + 1], c = t.corner[3 * (size_t)g + 2];
    float tn, tf;
    if (!trace_slab(r, fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z)),
                    fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z)), tn, tf)) return false;
    const TV3 A = tv3(a.x, a.y, a.z), B = tv3(b.x, b.y, b.z), C = tv3(c.x, c.y, c.z);
    const TV3 p0 = tv_sub(A, r.O), p1 = tv_sub(B, r.O), p2 = tv_sub(C, r.O);
    float s0, s1, s2;
    const float e0 = trace_edge(r.d, p1, p2, s0), e1 = trace_edge(r.d, p0, p2, s1), e2 = trace_edge(r.d, p0, p1, s2);
    if (!((e0 >= -s0 && e1 <= s1 && e2 >= -s2) || (e0 <= s0 && e1 >= -s1 && e2 <= s2))) return false;
    soft = !((e0 >= 0.0f && e1 <= 0.0f && e2 >= 0.0f) || (e0 <= 0.0f && e1 >= 0.0f && e2 <= 0.0f));   // inside only by the error bound
    const TV3 N = tv_cross(tv_sub(B, A), tv_sub(C, A));
    const float tt = tv_dot(p0, N) / tv_dot(r.d, N);
    if (render_bad(tt)) return false;
    th = fminf(fmaxf(tt, tn), tf);
    return th > r.tmin && !render_bad(th);
}

// the closest hard key and the closest soft key of a ray -> its hit
__device__ __forceinline__ unsigned long long trace_pick(unsigned long long hard, unsigned long long soft) {
    if (soft == ~0ull) return hard;
    if (hard == ~0ull) return soft;
    const float th = __uint_as_float((unsigned)(hard >> 32)), ts = __uint_as_float((unsigned)(soft >> 32));
    return ts < __builtin_fmaf(-th, 0.000244140625f, th) ? soft : hard;
}

// closest hit (ANY = false): the smallest key float_bits(t) << 32 | g below `best` (the floor's, or all ones); any hit (ANY = true): 0 as
// soon as a triangle that blocks light is hit at t < tmax, else all ones.  Left child first, then the skip link; at most 2 nt visits.
template <bool ANY>
__device__ __forceinline__ unsigned long long trace_walk(const MeshDev &m, const TraceDev &t, const TraceRay &r, unsigned long long best, float tmax,
                                                         TraceCount &cn) {
    const long long n = (long long)t.ctr[TC_KEPT];
    if (n > m.nt) return best;
    float tb = ANY ? tmax : __uint_as_float((unsigned)(best >> 32));   // (all ones: a NaN, which no comparison below takes for a bound)
    const bool bounded = ANY || best != ~0ull;
    bool have = bounded;
    unsigned long long bsoft = ~0ull;   // (soft hits never bound the walk: one behind the final hard hit cannot win, one before it is never culled)
    if (!t.use_bvh) {
        for (long long g = 0; g < m.nt; ++g) {
            float th;
            bool soft;
            ++cn.tests;
            if (!trace_tri<ANY>(m, t, r, (unsigned)g, th, soft)) continue;
            if (ANY) { if (th < tmax) return 0ull; continue; }
            const unsigned long long k = ((unsigned long long)__float_as_uint(th) << 32) | (unsigned long long)(unsigned)g;
            if (soft) { if (k < bsoft) bsoft = k; }
            else if (k < best) best = k;
        }
        return trace_pick(best, bsoft);
    }
    const long long cap = 2 * m.nt;
    long long visits = 0;
    int node = n > 0 ? 0 : -1;
    while (node >= 0) {
        if (++visits > cap) { cn.aborted = 1u; return ~0ull; }
        ++cn.visits;
        if (node >= n - 1) {   // a leaf: the triangle's own test holds its box
            const unsigned g = (unsigned)t.key[0][node - (n - 1)];
            float th;
            bool soft;
            ++cn.tests;
            if ((long long)g < m.nt && trace_tri<ANY>(m, t, r, g, th, soft)) {
                if (ANY) { if (th < tmax) return 0ull; }
                else {
                    const unsigned long long k = ((unsigned long long)__float_as_uint(th) << 32) | (unsigned long long)g;
                    if (soft) { if (k < bsoft) bsoft = k; }
                    else if (k < best) { best = k; tb = th; have = true; }
                }
            }
            node = t.skip[node];
            continue;
        }
        const float *bx = t.box + 6 * (size_t)node;
        float tn, tf;
        bool in = trace_slab(r, bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], tn, tf);
        if (in && have) in = ANY ? tn < tb : tn <= tb;
        node = in ? t.left[node] : t.skip[node];
        if (node >= 2 * n - 1) { cn.aborted = 1u; return ~0ull; }
    }
    return ANY ? best : trace_pick(best, bsoft);
}

// --- surfaces ---------------------------------------------------------------------------------------------------------------------------
struct TraceSurf {
    int water;          // material
    unsigned col;       // r | g << 8 | b << 16
    TV3 Ng;             // the geometric normal of the stored winding (turned round for a mesh wound inwards), not normalised
    TV3 ns;             // the shading normal (unit): the blend of the vertex normals, or Ng / |Ng|
    int blended;        // ns is a blend
};

__device__ __forceinline__ TraceSurf trace_surface(const RenderDev &d, const MeshDev &m, const TraceDev &t, unsigned id, TV3 O, TV3 dir, TV3 P) {
    TraceSurf s;
    s.blended = 0;
    if (id == TRACE_FLOOR_ID) {
        const int ix = (int)floorf((P.x - t.floor_lo[0]) / t.cell), iz = (int)floorf((P.z - t.floor_lo[1]) / t.cell);
        const unsigned tone = ((ix + iz) & 1) ? 128u : 204u;
        s.water = 0; s.col = tone | tone << 8 | tone << 16;
        s.Ng = tv3(0.0f, 1.0f, 0.0f); s.ns = s.Ng;
        return s;
    }
    const int st = t.st[id];
    const MeshRec rec = m.rec[st >> 1];
    s.water = rec.mat & 1; s.col = rec.col;
    const float4 a = t.corner[3 * (size_t)id], b = t.corner[3 * (size_t)id + 1], c = t.corner[3 * (size_t)id + 2];
    const TV3 A = tv3(a.x, a.y, a.z), B = tv3(b.x, b.y, b.z), C = tv3(c.x, c.y, c.z);
    TV3 N = tv_cross(tv_sub(B, A), tv_sub(C, A));
    const bool turn = ((st & 1) != 0) != ((rec.mat & 2) != 0);
    s.Ng = turn ? tv3(-N.x, -N.y, -N.z) : N;
    if (!tv_unit(s.Ng, s.ns)) s.ns = tv3(0.0f, 1.0f, 0.0f);   // (N is finite and non-zero: the set-up kept the triangle)
    if (rec.smooth) {   // weights: the edge function opposite each ordered corner (one sign inside the triangle)
        const TV3 p0 = tv_sub(A, O), p1 = tv_sub(B, O), p2 = tv_sub(C, O);
        const float w0 = tv_dot(dir, tv_cross(p1, p2)), w1 = -tv_dot(dir, tv_cross(p0, p2)), w2 = tv_dot(dir, tv_cross(p0, p1));
        const float *na = m.nrm + 3 * (size_t)__float_as_int(a.w), *nb = m.nrm + 3 * (size_t)__float_as_int(b.w), *nc = m.nrm + 3 * (size_t)__float_as_int(c.w);
        const TV3 bl = tv3(w0 * na[0] + w1 * nb[0] + w2 * nc[0], w0 * na[1] + w1 * nb[1] + w2 * nc[1], w0 * na[2] + w1 * nb[2] + w2 * nc[2]);
        TV3 u;
        if (tv_unit(bl, u)) {
            if (w0 + w1 + w2 < 0.0f) u = tv3(-u.x, -u.y, -u.z);   // (the weights share a sign: the blend keeps the normals' side)
            s.ns = u; s.blended = 1;
        }
    }
    return s;
}

// ambient + Lambert x visibility of a diffuse surface point, per channel in [0, ...): the rule of mesh_shade_px in world coordinates
__device__ __forceinline__ TV3 trace_diffuse(const RenderDev &d, const MeshDev &m, const TraceDev &t, const TraceSurf &s, TV3 dir, TV3 P, unsigned id,
                                             TraceCount &cn, unsigned &shadow_rays, int &shadow, TV3 &n) {
    n = s.ns;
    if (tv_dot(n, dir) > 0.0f) n = tv3(-n.x, -n.y, -n.z);
    const TV3 L = tv3(t.light[0] - P.x, t.light[1] - P.y, t.light[2] - P.z);
    const float ln = sqrtf(tv_dot(L, L));
    float ndl = fmaxf(tv_dot(n, L) / ln, 0.0f);
    shadow = -1;
    if (t.shadows && ndl > 0.0f) {
        const TraceRay r = trace_ray(P, L, 0.0f, id);
        ++shadow_rays;
        shadow = trace_walk<true>(m, t, r, ~0ull, 1.0f, cn) == 0ull ? 1 : 0;
        if (shadow) ndl = 0.0f;
    }
    TV3 c;
    c.x = (float)(s.col & 0xffu) / 255.0f * __builtin_fmaf(ndl, d.lrgb[0], d.amb);
    c.y = (float)((s.col >> 8) & 0xffu) / 255.0f * __builtin_fmaf(ndl, d.lrgb[1], d.amb);
    c.z = (float)((s.col >> 16) & 0xffu) / 255.0f * __builtin_fmaf(ndl, d.lrgb[2], d.amb);
    return c;
}

// the floor's key for the ray, or all ones
__device__ __forceinline__ unsigned long long trace_floor(const TraceDev &t, const TraceRay &r) {
    if (!t.floor || r.self == TRACE_FLOOR_ID) return ~0ull;
    const float tf = (t.floor_y - r.O.y) / r.d.y;
    if (render_bad(tf) || !(tf > r.tmin)) return ~0ull;
    const float x = __builtin_fmaf(tf, r.d.x, r.O.x), z = __builtin_fmaf(tf, r.d.z, r.O.z);
    if (!(x >= t.floor_lo[0] && x <= t.floor_hi[0] && z >= t.floor_lo[1] && z <= t.floor_hi[1])) return ~0ull;
    return ((unsigned long long)__float_as_uint(tf) << 32) | (unsigned long long)TRACE_FLOOR_ID;
}

__device__ __forceinline__ int trace_id_out(unsigned id) { return id == ~0u ? -1 : id == TRACE_FLOOR_ID ? -14 : (int)id; }

// --- the path of one pixel ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ TV3 trace_add(TV3 acc, TV3 w, TV3 c) {
    return tv3(__builtin_fmaf(w.x, c.x, acc.x), __builtin_fmaf(w.y, c.y, acc.y), __builtin_fmaf(w.z, c.z, acc.z));
}

__global__ void __launch_bounds__(256) k_trace_shade(RenderDev d, MeshDev m, TraceDev t) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = p < (size_t)d.W * d.H;
    TraceCount cn = {0u, 0u, 0u};
    unsigned rays_path = 0u, rays_refl = 0u, rays_shadow = 0u, truncated = 0u;
    if (in) {
        const int i = (int)(p % (size_t)d.W), j = (int)(p / (size_t)d.W);
        const float X = render_X(d, i), Y = render_Y(d, j);
        const TV3 bg = tv3((float)(d.bg & 0xffu) / 255.0f, (float)((d.bg >> 8) & 0xffu) / 255.0f, (float)((d.bg >> 16) & 0xffu) / 255.0f);
        // the path's ray, and the pending reflection of its last water hit
        TV3 O = tv3(d.E[0], d.E[1], d.E[2]);
        TV3 dir = tv3(__builtin_fmaf(X, d.s[0], __builtin_fmaf(Y, d.u[0], d.f[0])), __builtin_fmaf(X, d.s[1], __builtin_fmaf(Y, d.u[1], d.f[1])),
                      __builtin_fmaf(X, d.s[2], __builtin_fmaf(Y, d.u[2], d.f[2])));
        float tmin = d.zn;
        unsigned self = ~0u, rself = ~0u, wcol = 0u;
        TV3 rO = O, rdir = dir, rw = tv3(0.0f, 0.0f, 0.0f);
        bool refl = false, inside = false;
        TV3 thr = tv3(1.0f, 1.0f, 1.0f), acc = tv3(0.0f, 0.0f, 0.0f);
        int seg = 0;
        unsigned long long key0 = ~0ull;
        float *rec = nullptr;
        const float f0s = (t.ior - 1.0f) / (t.ior + 1.0f), F0 = f0s * f0s;
        for (int it = 0; it <= 2 * t.max_depth; ++it) {
            if (!refl && seg == t.max_depth) {   // cut: the background through what is left of the throughput
                acc = trace_add(acc, thr, bg);
                truncated = 1u;
                break;
            }
            const TraceRay r = refl ? trace_ray(rO, rdir, 0.0f, rself) : trace_ray(O, dir, tmin, self);
            if (refl) ++rays_refl; else if (seg) ++rays_path;
            const unsigned long long key = trace_walk<false>(m, t, r, trace_floor(t, r), 0.0f, cn);
            const unsigned id = key == ~0ull ? ~0u : (unsigned)key;
            const float th = __uint_as_float((unsigned)(key >> 32));
            if (!refl && seg == 0) key0 = key;
            if (!refl && t.rec) {
                rec = t.rec + ((size_t)p * t.max_depth + seg) * TRACE_REC_WORDS;
                rec[0] = r.O.x; rec[1] = r.O.y; rec[2] = r.O.z; rec[3] = r.d.x; rec[4] = r.d.y; rec[5] = r.d.z;
                rec[6] = __int_as_float(trace_id_out(id)); rec[7] = id == ~0u ? 0.0f : th;
                rec[8] = rec[9] = rec[10] = 0.0f;
                rec[11] = thr.x; rec[12] = thr.y; rec[13] = thr.z; rec[14] = rec[15] = rec[16] = 0.0f;
                rec[17] = rec[18] = rec[19] = 0.0f;
                rec[20] = __int_as_float(-1); rec[21] = __int_as_float(-1); rec[22] = 0.0f; rec[23] = __int_as_float(1 | (inside ? 8 : 0));
            }
            TV3 C = bg, P = r.O, nused = tv3(0.0f, 0.0f, 0.0f);
            TraceSurf s;
            s.water = 0;
            int shadow = -1;
            bool water_hit = false;
            if (id != ~0u) {
                P = tv_at(r.O, th, r.d);
                s = trace_surface(d, m, t, id, r.O, r.d, P);
                if (!refl && s.water) {   // a segment that ends leaving the fluid ran inside it, whatever was tracked (a camera in the fluid)
                    inside = !(tv_dot(r.d, s.Ng) < 0.0f);
                    if (inside) wcol = s.col;
                    if (rec) rec[23] = __int_as_float(1 | (inside ? 8 : 0));
                }
                if (!refl && inside) {   // Beer-Lambert along the segment's length (the primary direction is not a unit vector)
                    const float k = -(t.absorb * (seg == 0 ? th * sqrtf(tv_dot(r.d, r.d)) : th));
                    thr.x *= exp2f(k * (1.0f - (float)(wcol & 0xffu) / 255.0f));
                    thr.y *= exp2f(k * (1.0f - (float)((wcol >> 8) & 0xffu) / 255.0f));
                    thr.z *= exp2f(k * (1.0f - (float)((wcol >> 16) & 0xffu) / 255.0f));
                }
                if (!s.water) C = trace_diffuse(d, m, t, s, r.d, P, id, cn, rays_shadow, shadow, nused);
                else if (!refl) water_hit = true;   // (a reflection that meets water again is not followed: the background)
            }
            if (!water_hit) {
                const TV3 w = refl ? rw : thr;
                acc = trace_add(acc, w, C);
                if (rec) {
                    rec[17] = __builtin_fmaf(w.x, C.x, rec[17]); rec[18] = __builtin_fmaf(w.y, C.y, rec[18]); rec[19] = __builtin_fmaf(w.z, C.z, rec[19]);
                    if (refl) {
                        rec[21] = __int_as_float(trace_id_out(id));
                        rec[23] = __int_as_float(__float_as_int(rec[23]) | (shadow == 1 ? 16 : 0));
                    } else {
                        rec[8] = nused.x; rec[9] = nused.y; rec[10] = nused.z;
                        rec[20] = __int_as_float(shadow);
                    }
                }
                if (!refl) break;   // the path ends on a diffuse surface, the floor or the background
                refl = false;
                continue;
            }
            // water: enter or leave by the sign of d . Ng; the refraction normal; Snell, Schlick
            const float dng = tv_dot(r.d, s.Ng);
            const bool entering = dng < 0.0f;
            TV3 n = s.ns;
            if (s.blended && !(tv_dot(n, r.d) * dng > 0.0f)) tv_unit(s.Ng, n);
            if (tv_dot(n, r.d) > 0.0f) n = tv3(-n.x, -n.y, -n.z);
            TV3 du = r.d;
            tv_unit(r.d, du);
            const float cosi = fminf(fmaxf(-tv_dot(du, n), 0.0f), 1.0f);
            const float eta = entering ? 1.0f / t.ior : t.ior;
            const float k = __builtin_fmaf(-(eta * eta), __builtin_fmaf(-cosi, cosi, 1.0f), 1.0f);
            const TV3 rd = tv3(__builtin_fmaf(2.0f * cosi, n.x, du.x), __builtin_fmaf(2.0f * cosi, n.y, du.y), __builtin_fmaf(2.0f * cosi, n.z, du.z));
            int flags = 1 | (inside ? 8 : 0) | (entering ? 2 : 0);
            float F = 0.0f;
            if (k < 0.0f) {   // total internal reflection: the path follows the reflection with all of its throughput
                tv_unit(rd, dir);
                flags |= 4;
                inside = true; wcol = s.col;
            } else {
                const float ct = sqrtf(k), x = 1.0f - (entering ? cosi : ct), x2 = x * x;
                F = __builtin_fmaf(1.0f - F0, x2 * x2 * x, F0);
                const float q = __builtin_fmaf(eta, cosi, -ct);
                const TV3 td = tv3(__builtin_fmaf(eta, du.x, q * n.x), __builtin_fmaf(eta, du.y, q * n.y), __builtin_fmaf(eta, du.z, q * n.z));
                tv_unit(td, dir);
                rO = P; rself = id; rw = tv3(thr.x * F, thr.y * F, thr.z * F);
                tv_unit(rd, rdir);
                refl = true;
                thr = tv3(thr.x * (1.0f - F), thr.y * (1.0f - F), thr.z * (1.0f - F));
                inside = entering;
                wcol = s.col;
            }
            O = P; self = id; tmin = 0.0f; ++seg;
            if (rec) {
                rec[8] = n.x; rec[9] = n.y; rec[10] = n.z;
                rec[14] = thr.x; rec[15] = thr.y; rec[16] = thr.z;
                rec[22] = F; rec[23] = __int_as_float(flags);
            }
        }
        d.rgb[3 * p] = render_byte(acc.x); d.rgb[3 * p + 1] = render_byte(acc.y); d.rgb[3 * p + 2] = render_byte(acc.z);
        d.key[p] = key0;
    }
    // counters: one atomic per wave and counter that has something to add
    const unsigned long long pr = __ballot(in);
    const unsigned v[8] = {render_wave_sum(rays_path), render_wave_sum(rays_refl), render_wave_sum(rays_shadow), render_wave_sum(cn.visits),
                           render_wave_sum(cn.tests), render_wave_sum(truncated), render_wave_sum(cn.aborted), 0u};
    if ((threadIdx.x & 63) == 0) {
        if (pr) atomicAdd(&t.ctr[TC_RAYS_PRIMARY], (unsigned long long)__popcll(pr));
        if (v[0]) atomicAdd(&t.ctr[TC_RAYS_PATH], (unsigned long long)v[0]);
        if (v[1]) atomicAdd(&t.ctr[TC_RAYS_REFLECT], (unsigned long long)v[1]);
        if (v[2]) atomicAdd(&t.ctr[TC_RAYS_SHADOW], (unsigned long long)v[2]);
        if (v[3]) atomicAdd(&t.ctr[TC_VISITS], (unsigned long long)v[3]);
        if (v[4]) atomicAdd(&t.ctr[TC_TESTS], (unsigned long long)v[4]);
        if (v[5]) atomicAdd(&t.ctr[TC_TRUNCATED], (unsigned long long)v[5]);
        if (v[6]) atomicAdd(&t.ctr[TC_ABORTED], (unsigned long long)v[6]);
    }
}

// the id image of a traced frame (the colours are in place): -1 background, -2 - edge a box line, -14 the floor, else the primary hit's
// global triangle index; covered pixels counted as k_render_finish counts them (triangles)
__global__ void __launch_bounds__(256) k_trace_finish(RenderDev d) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool tri = false;
    if (p < (size_t)d.W * d.H) {
        const unsigned long long k = d.key[p];
        const unsigned lo = (unsigned)k;
        int id;
        if (k == ~0ull) id = -1;
        else if (lo >= RENDER_LINE_ID0) id = -2 - (int)(lo - RENDER_LINE_ID0);
        else if (lo == TRACE_FLOOR_ID) id = -14;
        else { id = (int)lo; tri = true; }
        if (d.ids) d.ids[p] = id;
    }
    const unsigned long long c = __ballot(tri);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&d.cnt[4], (unsigned long long)__popcll(c));
}

static void l_render_trace_setup(MeshDev &m, TraceDev &t, hipStream_t st) {
    if (m.nt <= 0) return;
    const unsigned grid = (unsigned)((m.nt + 255) / 256);
    hipLaunchKernelGGL(k_trace_setup, dim3(grid), dim3(256), 0, st, m, t);
    hipLaunchKernelGGL(k_trace_keys, dim3(grid), dim3(256), 0, st, m, t);
}
static void l_render_trace_sort(MeshDev &m, TraceDev &t, hipStream_t st) {
    if (m.nt <= 0) return;
    const int tiles = (int)((m.nt + TRACE_SORT_TILE - 1) / TRACE_SORT_TILE);
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 32 + 8 * pass;
        hipLaunchKernelGGL(k_trace_sort_count, dim3(tiles), dim3(256), 0, st, t, m.nt, pass, shift);
        hipLaunchKernelGGL(k_trace_sort_scan, dim3(1), dim3(256), 0, st, t, tiles);
        hipLaunchKernelGGL(k_trace_sort_scatter, dim3(tiles), dim3(256), 0, st, t, m.nt, tiles, pass, shift);
    }
}
static void l_render_trace_hierarchy(MeshDev &m, TraceDev &t, hipStream_t st) {
    if (m.nt <= 0) return;
    hipLaunchKernelGGL(k_trace_hierarchy, dim3((unsigned)((m.nt + 255) / 256)), dim3(256), 0, st, m, t);
}
static void l_render_trace_fit(MeshDev &m, TraceDev &t, hipStream_t st) {
    if (m.nt <= 0) return;
    hipLaunchKernelGGL(k_trace_fit, dim3((unsigned)((m.nt + 255) / 256)), dim3(256), 0, st, m, t);
    hipLaunchKernelGGL(k_trace_links, dim3((unsigned)((2 * m.nt + 255) / 256)), dim3(256), 0, st, m, t);
}
static void l_render_trace_shade(RenderDev &d, MeshDev &m, TraceDev &t) {
    const size_t px = (size_t)d.W * d.H;
    hipLaunchKernelGGL(k_trace_shade, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d, m, t);
}
static void l_render_trace_finish(RenderDev &d) {
    if (d.draw_box) {
        hipLaunchKernelGGL(k_render_lines<false>, dim3(12), dim3(256), 0, d.stream, d);
        hipLaunchKernelGGL(k_render_lines<true>, dim3(12), dim3(256), 0, d.stream, d);
    }
    const size_t px = (size_t)d.W * d.H;
    hipLaunchKernelGGL(k_trace_finish, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, d.stream, d);
}

static void register_render_trace_launchers(Launch &L) {
    L.render_trace_setup = l_render_trace_setup;
    L.render_trace_sort = l_render_trace_sort;
    L.render_trace_hierarchy = l_render_trace_hierarchy;
    L.render_trace_fit = l_render_trace_fit;
    L.render_trace_shade = l_render_trace_shade;
    L.render_trace_finish = l_render_trace_finish;
}
