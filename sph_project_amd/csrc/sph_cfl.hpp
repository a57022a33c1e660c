// sph_cfl.hpp -- adaptive time stepping: the reduce that finds the largest particle speed; included by sph_kernels.hip inside the
// per-build namespace.  Semantics in include/sph_hip.h (sph_set_cfl), design in DESIGN.md 39.
//
// k_cfl_speed: one pass over the live slots.  A thread loads the meta word and, where the particle counts (sph_cfl_eval.hpp, the source
// the host compiles too), the velocity: 20 bytes per particle.  The grid is capped at CFL_MAX_BLOCKS workgroups and the threads stride,
// so a large scene issues a bounded number of atomics.  Each thread keeps the maximum of |v|^2 as its unsigned bit pattern (non-negative
// floats order like unsigned integers), the 64 lanes of a wave reduce it with shuffles, and one lane issues one atomicMax per wave --
// none where the word already holds as much.  A lane that squares to inf or NaN leaves that value out and the wave sets a flag word.
// The two words of a launch sit on 128-byte lines of their own.  There are two such pairs: a launch writes pair `bank` and clears the
// other one with plain stores, which the next launch then writes -- no memset launch in steady state.  No LDS.
#pragma once

#define CFL_MAX_BLOCKS 1024

__global__ void __launch_bounds__(256)
k_cfl_speed(const Consts c, const float4 *__restrict__ velm, const int *__restrict__ meta, unsigned *__restrict__ words, int bank) {
    unsigned *mine = words + bank * SPH_CFL_BANK_STRIDE, *other = words + (bank ^ 1) * SPH_CFL_BANK_STRIDE;
    if (blockIdx.x == 0 && threadIdx.x == 0) { other[0] = 0u; other[SPH_CFL_WORD_STRIDE] = 0u; }
    const int n = live_n(c);
    unsigned best = 0u;
    bool bad = false;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (!cfl_counted(meta[i])) continue;
        const float4 v = velm[i];
        const unsigned b = cfl_bits(cfl_speed2(v.x, v.y, v.z));
        if (cfl_nonfinite(b)) bad = true; else best = max(best, b);
    }
    for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, off, 64));
    const bool any_bad = __any(bad);
    if ((threadIdx.x & 63) == 0) {
        if (best > 0u && best > __atomic_load_n(mine, __ATOMIC_RELAXED)) atomicMax(mine, best);
        if (any_bad) atomicOr(mine + SPH_CFL_WORD_STRIDE, 1u);
    }
}

static void l_cfl_speed(State &s, int bank) {
    if (!s.cfl_words) return;
    int blocks = cdiv(s.c.n, 256);
    if (blocks < 1) blocks = 1;   // (an empty handle still clears the other pair)
    if (blocks > CFL_MAX_BLOCKS) blocks = CFL_MAX_BLOCKS;
    hipLaunchKernelGGL(k_cfl_speed, dim3(blocks), dim3(256), 0, s.stream, s.c, s.velm.cur(), s.meta.cur(), s.cfl_words, bank & 1);
}

static void register_cfl_launchers(Launch &L) { L.cfl_speed = l_cfl_speed; }
