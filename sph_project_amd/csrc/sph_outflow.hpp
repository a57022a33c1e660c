// sph_outflow.hpp -- outflow: the two mark launches; included by sph_kernels.hip inside the per-build namespace.
// Semantics in include/sph_hip.h (sph_set_outflow), design in DESIGN.md 37.
//
// k_outflow_mark: one thread per live particle.  It loads the meta word and the position (20 bytes), runs the predicate
// (sph_outflow_eval.hpp, the source the host compiles too) over the active volumes, passed by value in index order, and sets the dead
// bit with a plain vector store.  The counts: one ballot per volume, and one atomic per wave and volume that has hits, on counters
// that sit on 128-byte lines of their own.  A wave without a hit -- nearly every wave -- issues no atomic and no store.
// k_outflow_mark_ids: the same for a removal by persistent id: a binary search in the sorted id list per particle.
// The sort that follows files the dead behind the grid (k_hash_count's meta_dead argument); nothing here moves a particle.  No LDS.
#pragma once

#define META_DEAD_BIT (1 << 12)

__global__ void __launch_bounds__(256)
k_outflow_mark(const Consts c, const OutflowArgs a, const float4 *__restrict__ posv, int *__restrict__ meta, unsigned *__restrict__ ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int hit = -1;
    if (i < live_n(c)) {
        const int m = meta[i];
        if (META_ACTIVE_FLUID(m) && !META_DEAD(m)) {
            const float4 p = posv[i];
            const int obj = META_OBJ(m);
            const unsigned obit = (obj >= 0 && obj < 32) ? (1u << obj) : 0u;
            for (int q = 0; q < a.nvol; ++q)
                if ((a.v[q].objects == 0xffffffffu || (a.v[q].objects & obit)) && of_inside(&a.v[q], p.x, p.y, p.z)) { hit = q; break; }
            if (hit >= 0) meta[i] = m | META_DEAD_BIT;
        }
    }
    if (!__any(hit >= 0)) return;   // (wave-uniform)
    for (int q = 0; q < a.nvol; ++q) {
        const unsigned long long b = __ballot(hit == q);
        if (b && lane == 0) atomicAdd(&ctr[a.v[q].index * SPH_OUTFLOW_CTR_STRIDE], (unsigned)__popcll(b));
    }
}

__global__ void __launch_bounds__(256)
k_outflow_mark_ids(const Consts c, const int *__restrict__ ids, int nids, const int *__restrict__ pid, int *__restrict__ meta,
                   unsigned *__restrict__ ctr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool hit = false;
    if (i < live_n(c)) {
        const int id = pid[i];
        int lo = 0, hi = nids;   // first entry >= id
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (ids[mid] < id) lo = mid + 1; else hi = mid; }
        if (lo < nids && ids[lo] == id) {
            const int m = meta[i];
            if (META_ACTIVE_FLUID(m) && !META_DEAD(m)) { meta[i] = m | META_DEAD_BIT; hit = true; }
        }
    }
    const unsigned long long b = __ballot(hit);
    if (b && lane == 0) atomicAdd(&ctr[SPH_MAX_OUTFLOWS * SPH_OUTFLOW_CTR_STRIDE], (unsigned)__popcll(b));
}

static void l_outflow_mark(State &s, const OutflowArgs &a) {
    if (a.nvol <= 0 || s.c.n <= 0 || !s.outflow_ctr) return;
    hipLaunchKernelGGL(k_outflow_mark, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, a, s.posv.cur(), s.meta.cur(), s.outflow_ctr);
}

static void l_outflow_mark_ids(State &s, int nids) {
    if (nids <= 0 || s.c.n <= 0 || !s.outflow_ctr || !s.outflow_ids) return;
    hipLaunchKernelGGL(k_outflow_mark_ids, dim3(cdiv(s.c.n, 256)), dim3(256), 0, s.stream, s.c, s.outflow_ids, nids, s.pid.cur(),
                       s.meta.cur(), s.outflow_ctr);
}

static void register_outflow_launchers(Launch &L) { L.outflow_mark = l_outflow_mark; L.outflow_mark_ids = l_outflow_mark_ids; }
