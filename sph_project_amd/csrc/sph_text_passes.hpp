// sph_text_passes.hpp -- the device passes of the text export (the object is in sph_text_api.hpp, the number formats in
// sph_text.hpp).  Rows of a PLY ("x y z \n") or an OBJ ("v x y z\n", "vn x y z\n", "f a//a b//b c//c\n" or "f a b c\n") are numbered
// through the whole file; a piece is a run of at most piece_rows of them:
//   count   one thread per row: the row's bytes (the digits are computed, nothing is stored but the length), the longest row
//   scan    exclusive scan of the lengths (the surface reconstruction's three scan kernels), len[rows] = the piece's bytes
//   write   one workgroup per 256 rows: the rows' bytes are laid into LDS at (their offset - the workgroup's first offset), shifted by
//           the first offset's low 4 bits so that LDS and the output agree modulo 16; then the unaligned head goes out as bytes, the
//           body as aligned 16-byte stores (one global_store_dwordx4 per lane, a wave covers 1 KiB contiguous), the tail as bytes
// Integer code only: the strict and the fast build make the same bytes.
#pragma once
#include "sph_text.hpp"

#define TEXT_WG 256
#define TEXT_STAGE_VEC ((16 + TEXT_WG * TEXT_ROW_MAX + 15) / 16)   // uint4 words: the low-bits shift + 256 longest rows (18 208 bytes)

__device__ static inline int text_row_len(const TextDev &d, long long r) {
    if (d.kind == 0) {
        const unsigned *x = d.xyz + 3 * r;
        return text_f32_len(x[0]) + text_f32_len(x[1]) + text_f32_len(x[2]) + 4;
    }
    const long long nvn = d.nrm ? 2 * d.nv : d.nv;
    if (r < nvn) {
        const bool vn = r >= d.nv;
        const unsigned *x = (vn ? d.nrm : d.xyz) + 3 * (vn ? r - d.nv : r);
        return (vn ? 2 : 1) + text_f32_len(x[0]) + text_f32_len(x[1]) + text_f32_len(x[2]) + 4;
    }
    const int *t = d.tri + 3 * (r - nvn);
    const int a = text_index_len(t[0]), b = text_index_len(t[1]), c = text_index_len(t[2]);
    return d.nrm ? 1 + 2 * (a + b + c) + 3 * 3 + 1 : 1 + (a + b + c) + 3 + 1;
}

__device__ static inline void text_row_put(const TextDev &d, long long r, char *p) {
    int n = 0;
    if (d.kind == 0) {
        const unsigned *x = d.xyz + 3 * r;
#pragma unroll 1
        for (int c = 0; c < 3; ++c) { n += text_f32(x[c], p + n); p[n++] = ' '; }
        p[n] = '\n';
        return;
    }
    const long long nvn = d.nrm ? 2 * d.nv : d.nv;
    if (r < nvn) {
        const bool vn = r >= d.nv;
        const unsigned *x = (vn ? d.nrm : d.xyz) + 3 * (vn ? r - d.nv : r);
        p[n++] = 'v';
        if (vn) p[n++] = 'n';
#pragma unroll 1
        for (int c = 0; c < 3; ++c) { p[n++] = ' '; n += text_f32(x[c], p + n); }
        p[n] = '\n';
        return;
    }
    const int *t = d.tri + 3 * (r - nvn);
    p[n++] = 'f';
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        p[n++] = ' ';
        n += text_index(t[c], p + n);
        if (d.nrm) { p[n++] = '/'; p[n++] = '/'; n += text_index(t[c], p + n); }
    }
    p[n] = '\n';
}

__global__ void __launch_bounds__(TEXT_WG) k_text_count(TextDev d) {
    __shared__ int longest;
    if (threadIdx.x == 0) longest = 0;
    __syncthreads();
    const int i = blockIdx.x * TEXT_WG + threadIdx.x;
    if (i < d.rows) {
        const int n = text_row_len(d, d.row0 + i);
        d.len[i] = n;
        atomicMax(&longest, n);
    }
    __syncthreads();
    if (threadIdx.x == 0 && longest > 0) atomicMax(d.longest, longest);
}

__global__ void __launch_bounds__(TEXT_WG) k_text_write(TextDev d) {
    __shared__ uint4 stage[TEXT_STAGE_VEC];
    char *s = reinterpret_cast<char *>(stage);
    const int first = blockIdx.x * TEXT_WG;
    const int last = min(first + TEXT_WG, d.rows);
    const unsigned g0 = (unsigned)d.len[first], g1 = (unsigned)d.len[last];   // this workgroup's bytes [g0, g1) of the piece
    if (g1 < g0 || g1 - g0 > (unsigned)(TEXT_WG * TEXT_ROW_MAX)) return;      // (never: the scan is of lengths <= TEXT_ROW_MAX)
    const unsigned a0 = g0 & ~15u;   // s[b - a0] is byte b of the piece
    const int i = first + (int)threadIdx.x;
    if (i < last) {
        const unsigned o = (unsigned)d.len[i];
        if (o >= g0 && o + (unsigned)TEXT_ROW_MAX <= a0 + 16u * TEXT_STAGE_VEC) text_row_put(d, d.row0 + i, s + (o - a0));
    }
    __syncthreads();
    const unsigned head_end = min(g1, (g0 + 15u) & ~15u);
    const unsigned body_end = max(head_end, g1 & ~15u);
    for (unsigned b = g0 + threadIdx.x; b < head_end; b += TEXT_WG) d.out[b] = (unsigned char)s[b - a0];
    for (unsigned b = head_end + 16u * threadIdx.x; b < body_end; b += 16u * TEXT_WG)
        *reinterpret_cast<uint4 *>(d.out + b) = stage[(b - a0) >> 4];
    for (unsigned b = body_end + threadIdx.x; b < g1; b += TEXT_WG) d.out[b] = (unsigned char)s[b - a0];
}

// triangle indices of a mesh: bad[0] = 1 if any lies outside [0, nv)
__global__ void __launch_bounds__(256) k_text_check_tri(const int *tri, long long n3, long long nv, int *bad) {
    __shared__ int any;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    int mine = 0;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n3; k += (long long)gridDim.x * 256) {
        const int v = tri[k];
        if (v < 0 || (long long)v >= nv) mine = 1;
    }
    if (mine) atomicOr(&any, 1);
    __syncthreads();
    if (threadIdx.x == 0 && any) atomicOr(bad, 1);
}

// the particles of one object in the handle's current order: flags, their exclusive scan, a gather to the scanned slots
__global__ void __launch_bounds__(256) k_text_obj_flag(const int *meta, int n, int obj, int *flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int m = meta[i];
    flag[i] = (META_OBJ(m) == obj && !META_GHOST(m) && !META_DEAD(m)) ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_text_obj_gather(const float4 *posv, const int *meta, int n, int obj, const int *slot, float *xyz) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int m = meta[i];
    if (META_OBJ(m) != obj || META_GHOST(m) || META_DEAD(m)) return;
    const float4 p = posv[i];
    float *o = xyz + 3 * (size_t)slot[i];
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
}

static void text_scan(int *a, int n, int *tmp, hipStream_t st) {
    const int tiles = cdiv(n > 0 ? n : 1, 1024);
    hipLaunchKernelGGL(k_surf_scan_tile, dim3(tiles), dim3(256), 0, st, a, n, tmp);
    hipLaunchKernelGGL(k_surf_scan_top, dim3(1), dim3(256), 0, st, tmp, tiles, a, n);
    hipLaunchKernelGGL(k_surf_scan_add, dim3(tiles), dim3(256), 0, st, a, n, (const int *)tmp);
}

static void l_text_count(TextDev &d) {
    if (d.rows > 0) hipLaunchKernelGGL(k_text_count, dim3(cdiv(d.rows, TEXT_WG)), dim3(TEXT_WG), 0, d.stream, d);
}
static void l_text_scan(TextDev &d) { text_scan(d.len, d.rows, d.scan_tmp, d.stream); }
static void l_text_write(TextDev &d) {
    if (d.rows > 0) hipLaunchKernelGGL(k_text_write, dim3(cdiv(d.rows, TEXT_WG)), dim3(TEXT_WG), 0, d.stream, d);
}
static void l_text_check_tri(TextDev &d, int *bad) {
    hipMemsetAsync(bad, 0, sizeof(int), d.stream);
    const long long n3 = 3 * d.nt;
    const long long wg = (n3 + 255) / 256;
    if (n3 > 0) hipLaunchKernelGGL(k_text_check_tri, dim3((int)(wg < 4096 ? wg : 4096)), dim3(256), 0, d.stream, d.tri, n3, d.nv, bad);
}
// slot[n + 1] (scratch), xyz[3 n]: afterwards slot[n] = the object's particles
static void l_text_compact(TextDev &d, const float4 *posv, const int *meta, int n, int obj, int *slot, float *xyz) {
    if (n > 0) hipLaunchKernelGGL(k_text_obj_flag, dim3(cdiv(n, 256)), dim3(256), 0, d.stream, meta, n, obj, slot);
    text_scan(slot, n, d.scan_tmp, d.stream);
    if (n > 0) hipLaunchKernelGGL(k_text_obj_gather, dim3(cdiv(n, 256)), dim3(256), 0, d.stream, posv, meta, n, obj, (const int *)slot, xyz);
}

static void register_text_launchers(Launch &L) {
    L.text_count = l_text_count;
    L.text_scan = l_text_scan;
    L.text_write = l_text_write;
    L.text_check_tri = l_text_check_tri;
    L.text_compact = l_text_compact;
}
