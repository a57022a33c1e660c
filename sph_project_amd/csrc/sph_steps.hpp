// sph_steps.hpp -- per-method step orchestration (included by sph_api.hip).
// Order of operations follows WCSPH.py:27, DFSPH.py:298, PCISPH.py:165 and base_solver.py:692.
#pragma once
#include <sched.h>

// reads scal->red[slot] (one small D2H copy + stream sync): the residual of the single IISPH iteration phase
static int read_red(SphHandle *h, int slot, float *out) {
    HIPCHK(h, hipMemcpyAsync(&h->scal_h->red[slot], &h->st.scal->red[slot], sizeof(float), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    *out = h->scal_h->red[slot];
    return SPH_OK;
}

static int implicit_viscosity_non_pressure(SphHandle *h);

// Read-back of a solver loop's batch (round 6).  hipMemcpyAsync D2H + hipStreamSynchronize cost 35-75 us of idle GPU per batch (the copy is a
// kernel of the runtime, the synchronise sleeps on an interrupt: profiles/r05_gaps_c3_motion.txt) -- two to three per solve, five to six per
// step of the buckling scene: a fifth of its step.  Instead a one-wave kernel behind the batch stores the residuals and the flags into pinned
// host memory, the batch number last (system-scope release), and the host spins on that number: the wait ends a few microseconds after the
// batch's last kernel.  (The same kernel -> pinned memory -> polling host pattern as the slab counts' mirror, sph_halo.hpp.)  Bounded: the host
// looks at hipStreamQuery every few microseconds and falls back to the copy when the stream is idle or broken.
struct LoopPub { float red[8]; int flags[4]; unsigned seq; unsigned pad[3]; };
static_assert(sizeof(LoopPub) == 64, "LoopPub layout");
__global__ void __launch_bounds__(64) k_publish_loop(DevScalars *scal, LoopPub *pub, unsigned seq) {
    const int t = threadIdx.x;
    const int stop = scal->flags[0];
    if (t < 8) __hip_atomic_store(&pub->red[t], scal->red[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if (t < 12) __hip_atomic_store(&pub->flags[t - 8], scal->flags[t - 8], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __syncthreads();
    if (t == 0) {
        // a loop that has stopped is over (the host launches nothing more for it): its flags are reset here, so that the next loop needs
        // no memset in front of it (a fill kernel + a launch boundary per solve)
        if (stop) { scal->flags[0] = 0; scal->flags[1] = 0; }
        __hip_atomic_store(&pub->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// host side of a publish: spin until the kernel's number shows up in pinned memory; false: the stream went idle or broke without it
static bool spin_for(State &s, const volatile unsigned *seq, unsigned want) {
    for (unsigned spins = 0;; ++spins) {
        if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == want) return true;
        if ((spins & 255u) == 255u) {
            const hipError_t q = hipStreamQuery(s.stream);
            if (q != hipErrorNotReady) return q == hipSuccess && __atomic_load_n(seq, __ATOMIC_ACQUIRE) == want;   // idle: one more look; or broken
            if (hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();   // "not yet" is no failure (check_async)
            if (spins > 4096u) sched_yield();   // a long wait (many steps queued): let whoever else wants this core have it; returns at once otherwise
        }
        __builtin_ia32_pause();
    }
}
// The pair statistics of one bank (3 x SPH_STAT_SLOTS striped 64-bit counters) added up on the device and published the same way: a D2H copy of
// the 97 KB DevScalars issued on an IDLE stream costs ~0.3 ms on this runtime (profiles/r06_sync_latency.txt)
struct StatsPub { unsigned long long pairs, evals, fallback; unsigned seq; unsigned pad[9]; };
static_assert(sizeof(StatsPub) == 64, "StatsPub layout");
__global__ void __launch_bounds__(256) k_publish_stats(const DevScalars *scal, int bank, StatsPub *pub, unsigned seq) {
    __shared__ unsigned long long s_w[3][4];
    unsigned long long a = 0, b = 0, c = 0;
    for (int k = threadIdx.x; k < SPH_STAT_SLOTS; k += 256) { a += scal->pairs[bank][k]; b += scal->evals[bank][k]; c += scal->fallback[bank][k]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); c += __shfl_down(c, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_w[0][threadIdx.x >> 6] = a; s_w[1][threadIdx.x >> 6] = b; s_w[2][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(&pub->pairs, s_w[0][0] + s_w[0][1] + s_w[0][2] + s_w[0][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&pub->evals, s_w[1][0] + s_w[1][1] + s_w[1][2] + s_w[1][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&pub->fallback, s_w[2][0] + s_w[2][1] + s_w[2][2] + s_w[2][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
        __hip_atomic_store(&pub->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// brings scal->red[0..8) and scal->flags[0..4) of the stream's current end into h->scal_h
static int loop_readback(SphHandle *h) {
    State &s = h->st;
    if (h->loop_pub) {
        const unsigned want = ++h->loop_seq;
        volatile LoopPub *pub = h->loop_pub;
        hipLaunchKernelGGL(k_publish_loop, dim3(1), dim3(64), 0, s.stream, s.scal, h->loop_pub, want);
        const bool got = spin_for(s, &pub->seq, want);
        if (got) {
            for (int k = 0; k < 8; ++k) h->scal_h->red[k] = pub->red[k];
            for (int k = 0; k < 4; ++k) h->scal_h->flags[k] = pub->flags[k];
            if (h->scal_h->flags[0] != 0) h->loop_flags_clean = true;   // (the kernel reset them behind the copy; else: as they were -- this is
                                                                        //  also the plain wait of sph_synchronize / sph_step, outside any loop)
            return SPH_OK;
        }
        h->loop_flags_clean = false;   // (whether the kernel ran is not known here)
    }
    hipError_t e = hipMemcpyAsync(h->scal_h->red, s.scal->red, 8 * sizeof(float) + 4 * sizeof(int), hipMemcpyDeviceToHost, s.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    if (e != hipSuccess) return fail(h, SPH_ERR_HIP, "solver loop read-back failed: %s", hipGetErrorString(e));
    return SPH_OK;
}

// particle_num the reference's residual means divide by (DFSPH.py:212, :293): the whole scene's, not this slab's
static long long dfsph_particle_num(SphHandle *h) { return h->st.slab_active ? h->comm_n_global : (long long)h->n; }

// A solve with a FIXED iteration count (SphParams::fixed_iterations: bench mode, sph_step_async) has no stop test, and nothing reads
// the residual of an iteration (SphStats::err_* report the reference's initial value in this mode): the walks still leave their
// per-workgroup partial sums, but the one-workgroup kernel that adds them up -- 5 us and a launch boundary per iteration, 2.4 % of a
// C3 step -- is not launched.  Unsharded only (a sharded solve all-reduces the residual either way).
struct SkipResidual {
    State &s;
    SkipResidual(SphHandle *h) : s(h->st) {
        s.skip_residual = (h->prm.fixed_iterations > 0 && !s.slab_active) ? 1 : 0;
    }
    ~SkipResidual() { s.skip_residual = 0; }
};

// What run_solve needs to know about one iterative solve.
struct SolveSpec {
    int slot;          // reduction slot of the residual (scal->red[slot]); also indexes loop_hint
    int kind;          // the reference's stop test, evaluated by the iteration's last reduction (State::loop_kind)
    double thr;        // its threshold
    float denom;       // residual = red[slot] / denom (0 when denom is not positive)
    int max_itr;       // iteration cap without fixed_iterations
    float fixed_err;   // residual reported with fixed_iterations: the reference's initial value
    int32_t *iter;     // where the iteration count and the residual go (h->last)
    float *err;
    void (*batch_end)(State &);   // optional: launched behind every batch, before its read-back (CG: cg_check)
};

// Solver loop.  `pre` launches the passes in front of the loop, `body` one iteration and returns the rc of its exchanges: the first
// non-zero rc ends the solve.  With fixed_iterations > 0: exactly that many iterations, no stop test, no read-back.  Otherwise the
// stop test runs on the device: the iteration's last reduction kernel evaluates the reference's criterion, counts the iteration and
// raises scal->flags[0]; every kernel of a later iteration starts with a look at that flag and returns.  Iterations go out in
// batches with ONE read-back per batch (loop_readback) instead of one per iteration (the reference synchronises with the host every
// iteration).  The state after the loop is the state after exactly the iteration the reference would have stopped at, whatever the
// batch sizes.
// Batch sizes (round 5): a solve takes about as many iterations as the same solve of the last step (C5: 41.5 +- 1 CG
// iterations; C3 in motion: 26.5 +- 1 density iterations), so the FIRST batch is last step's count less one and the
// loop then goes on in small batches -- two read-backs per solve instead of five to seven.  Every read-back is a
// stream drain plus the host's launch latency before the GPU has work again (~25-40 us of idle chip: the rocprofv3
// traces of round 5 show 188 us of kernels per DFSPH iteration in motion against 285 us of wall time, profiles/
// r05_rocprofv3_c3_motion_summary.txt).  Without a hint (first step): 2, 4, 8, 8, ...
// *launched (optional): the iterations enqueued; past the stop they are no-ops, so it can exceed *sp.iter by up to a batch.
template <class Pre, class Body>
static int run_solve(SphHandle *h, const SolveSpec &sp, Pre pre, Body body, int *launched = nullptr) {
    State &s = h->st;
    SkipResidual skip(h);
    pre();
    const int fixed = h->prm.fixed_iterations;
    int n = 0;
    if (fixed > 0) {
        for (; n < fixed; ++n) { int rc = body(); if (rc) return rc; }
        *sp.iter = fixed; *sp.err = sp.fixed_err;
    } else {
        if (!h->loop_flags_clean) HIPCHK(h, hipMemsetAsync(&s.scal->flags[0], 0, 2 * sizeof(int), s.stream));
        h->loop_flags_clean = false;
        s.loop_flag = &s.scal->flags[0];
        s.loop_slot = sp.slot; s.loop_kind = sp.kind; s.loop_denom = sp.denom; s.loop_thr = sp.thr;
        const int hint = h->loop_hint[sp.slot];
        int batch = hint > 3 ? hint - 1 : 2, rc = SPH_OK;
        bool predicted = hint > 3;
        // red[8] and flags[4] are neighbours in DevScalars: one 48-byte copy brings the residual and the flags
        static_assert(offsetof(DevScalars, flags) == offsetof(DevScalars, red) + 8 * sizeof(float), "red / flags layout");
        while (n < sp.max_itr) {
            const int nb = std::min(batch, sp.max_itr - n);
            for (int k = 0; k < nb && !rc; ++k) rc = body();
            if (rc) break;
            if (sp.batch_end) sp.batch_end(s);
            n += nb;
            rc = loop_readback(h);
            if (rc || h->scal_h->flags[0]) break;
            if (predicted) { batch = 2; predicted = false; }
            else if (batch < 8) batch *= 2;
        }
        s.loop_flag = nullptr;
        if (rc) return rc;
        *sp.iter = h->loop_hint[sp.slot] = h->scal_h->flags[1];
        *sp.err = sp.denom > 0 ? h->scal_h->red[sp.slot] / sp.denom : 0.0f;
    }
    if (launched) *launched = n;
    return SPH_OK;
}

// Akinci surface tension (sph_set_surface_tension): the colour-field normals the non-pressure pass reads, from the positions and
// densities as they are now, on the masks of the last sort.  Nothing without the mode.
static void ph_surface_normals(SphHandle *h) {
    if (!h->st.st_akinci) return;
    ProfScope p(h, SPH_K_SURFACE_NORMALS);
    h->L->surface_normals(h->st);
}

// Micropolar vorticity model (sph_set_micropolar): the walk reads positions, the step's starting velocities, densities and last step's
// w -- nothing the non-pressure pass writes -- so it runs in front of that pass; v += dt a_mp follows behind it (behind the end of the
// implicit-viscosity solve).  Nothing without the mode.
static void ph_micropolar(SphHandle *h) {
    if (!h->st.mp_on) return;
    ProfScope p(h, SPH_K_MICROPOLAR);
    h->L->micropolar(h->st);
}
static void ph_micropolar_apply(SphHandle *h) {
    if (!h->st.mp_on) return;
    ProfScope p(h, SPH_K_MISC);
    h->L->micropolar_apply(h->st);
}

// Elastic solids (sph_set_elastic_object): the passes read positions only, so they run in front of the non-pressure pass;
// v += dt a_el follows behind it, behind the micropolar model's.  Nothing while no object has been captured.
static void ph_elastic(SphHandle *h) {
    if (!h->st.el_nobj) return;
    ProfScope p(h, SPH_K_ELASTIC);
    h->L->elastic(h->st);
}
static void ph_elastic_apply(SphHandle *h) {
    if (!h->st.el_nobj) return;
    ProfScope p(h, SPH_K_MISC);
    h->L->elastic_apply(h->st);
}

// Air drag (sph_set_drag): the walk reads positions and the step's starting velocities -- nothing another pass of the phase writes --
// so it runs in front of the non-pressure pass; v += dt a_drag follows behind it, behind the elastic solids'.  Nothing without the mode.
static void ph_drag(SphHandle *h) {
    if (!h->st.dr_on) return;
    ProfScope p(h, SPH_K_DRAG);
    h->L->drag(h->st);
}
static void ph_drag_apply(SphHandle *h) {
    if (!h->st.dr_on) return;
    ProfScope p(h, SPH_K_MISC);
    h->L->drag_apply(h->st);
}

// Heat (sph_set_thermal): the gather and the walk read positions, densities and last step's T -- no velocity, nothing another pass of
// the phase writes -- so they run in front of the non-pressure pass (WCSPH's fused route: in front of its force pass); the buoyancy
// v += dt a_b follows behind it, behind the air drag's, and only with beta != 0.  Nothing without the mode.
static void ph_heat(SphHandle *h) {
    if (!h->st.heat_on) return;
    ProfScope p(h, SPH_K_HEAT);
    h->L->heat(h->st);
}
static void ph_heat_apply(SphHandle *h) {
    if (!h->st.heat_on || h->st.heat_beta == 0.0) return;
    ProfScope p(h, SPH_K_MISC);
    h->L->heat_apply(h->st);
}

// base_solver.py:190 compute_non_pressure_acceleration + :643 update_fluid_velocity
// walks = false (SPH_PH_NON_PRESSURE): the Akinci pass runs on the normals the last SPH_PH_SURFACE_NORMALS / step stored, and the
// micropolar model's a_mp is the one the last SPH_PH_MICROPOLAR / step stored (likewise a_el and a_drag)
static int run_non_pressure(SphHandle *h, bool walks = true) {
    if (walks) { ph_surface_normals(h); ph_micropolar(h); ph_elastic(h); ph_drag(h); ph_heat(h); }   // (positions and densities do not change under the CG solve: its end reads these too)
    if (h->prm.viscosity_implicit) {
        int rc = implicit_viscosity_non_pressure(h); if (rc) return rc;
        ph_micropolar_apply(h);
        ph_elastic_apply(h);
        ph_drag_apply(h);
        ph_heat_apply(h);
        return SPH_OK;
    }
    { ProfScope p(h, SPH_K_NON_PRESSURE); h->L->non_pressure(h->st, nullptr); }
    ph_micropolar_apply(h);
    ph_elastic_apply(h);
    ph_drag_apply(h);
    ph_heat_apply(h);
    return SPH_OK;
}

static int wcsph_step(SphHandle *h) {
    State &s = h->st;
    // sharded: + migration / ghost exchange; over the push transport a plain WCSPH step needs nothing back from the device
    // (slab_neighbor_search_push, "async"): implicit viscosity and the unfused force passes launch exact grids instead
    const bool fused = !h->prm.viscosity_implicit && !s.st_akinci && !s.mp_on && !s.el_marked && !s.dr_on && !(s.heat_on && s.heat_beta != 0.0);   // (heat without buoyancy adds nothing to v: the walk runs in front of the fused pass; the Akinci surface tension and the micropolar walk need the densities of ALL neighbours first; an elastic object adds a_el behind the non-pressure pass, the air drag a_drag)
    SortCarry carry;   // what the sort leaves to the density pass below (unsharded: that pass is the next launch and walks every tile)
    if (s.slab_active) { int rc = slab_neighbor_search(h, fused); if (rc) return rc; }
    else carry = ph_neighbor_search(h, true, true);                           // WCSPH.py:28 (the density pass below rewrites every rho: the sort need not move it)
    ph_rigid_volume(h);                                                       // base_solver.py:696 (see ph_rigid_volume)
    const bool books = fused && !getenv("SPH_FORCES_COUNT_OWN");   // (switch: the force pass counts its own pairs -- the counting instantiation any other caller of l_wcsph_forces gets)
    // Sharded over the push transport, fluid only: the density pass runs the slab's BOUNDARY tiles first, their rho / p go out to the
    // neighbours, and the INTERIOR tiles (everything more than two layers from a face) run while that message is in flight; only
    // then does the stream wait for the neighbours' (SURVEY 8e "compute interior cells while halos are in flight").
    const bool overlap = s.slab_active && s.push.on && s.tile_list[0] && s.c.all_fluid && s.tile_plan_n == s.c.n && (s.has_down || s.has_up);
    if (overlap) {
        const int hint = slab_field_hint(h);
        { ProfScope p(h, SPH_K_DENSITY); h->L->density(s, 1, {1, books}); }
        { ProfScope p(h, SPH_K_HALO); h->L->halo_push_fields(s, 2, nullptr, nullptr, hint); }
        { ProfScope p(h, SPH_K_DENSITY); h->L->density(s, 1, {2, books}); }
        { ProfScope p(h, SPH_K_HALO); h->L->halo_pull_fields(s, 2, nullptr, nullptr, hint); }
    } else if (s.slab_active && s.push.on) {
        // ghost rho, p: the density pass stores the values of its boundary particles straight into the neighbours' field message
        // (HaloFieldSend) -- no gather kernel, and the message travels while the pass is still running; then the usual wait + scatter
        const int hint = slab_field_hint(h);
        h->L->halo_fieldsend_begin(s);
        { ProfScope p(h, SPH_K_DENSITY); h->L->density(s, 1, {0, books}); }   // :29 + :33 (EOS fused)
        { ProfScope p(h, SPH_K_HALO); h->L->halo_pull_fields(s, 2, nullptr, nullptr, hint); }
    } else {
        { ProfScope p(h, SPH_K_DENSITY); h->L->density(s, 1, {0, books, carry}); }   // :29 + :33 (EOS fused)
        if (s.slab_active) { int rc = slab_exchange_fields(h); if (rc) return rc; }   // ghost rho, p
    }
    if (fused) {
        // Another step of this call follows (sph_step_async(n)) and nothing on the host happens in between: the force pass classifies its
        // own particles and stores the NEXT step's message into the neighbours' inboxes as its workgroups finish (HaloSend,
        // sph_halo_defs.hpp) -- the records travel while the pass is still running, and the next step starts with the hash alone.  Not
        // with an emitter or rigid bodies (they move particles after this pass) and not before a step that re-plans the cuts.
        const SlabComm &cm = h->comm;
        const bool rebalance_next = cm.rebalance_every > 0 && (h->steps + 1) % cm.rebalance_every == 0 && !h->any_rigid_object;
        if (s.slab_active && s.push.on && h->steps_to_follow > 0 && !rebalance_next && !s.has_emitter && !h->any_rigid_object &&
            !h->sort_dirty && !h->em_touch)
            h->L->halo_presend_begin(s);
        // Unsharded, all fluid, another step of this call queued right behind (nothing can touch the particles in between): the force pass
        // hashes the positions it stores for the next step's sort (NextHash) -- one launch less per step.
        // Not in a step whose slot holds or emits (fluid emitters: the slot moves / adds particles behind this pass; the host knows now).
        const bool hash_next = !s.slab_active && s.c.all_fluid && h->steps_to_follow > 0 && !s.has_emitter && !h->any_rigid_object &&
                               !h->sort_dirty && !h->em_touch;
        ph_heat(h);   // (heat with beta == 0: positions, densities and T only -- nothing the force pass has written yet)
        ProfScope p(h, SPH_K_WCSPH_FORCES); h->L->wcsph_forces(s, {books, hash_next});   // :30-31 + :34-36, :45 in one neighbour walk
        return SPH_OK;
    }
    int rc = run_non_pressure(h); if (rc) return rc;                          // :30-31
    { ProfScope p(h, SPH_K_PRESSURE_INTEGRATE); h->L->pressure_integrate(s); } // :34-36, :45
    return SPH_OK;
}

// DFSPH.py:139 correct_divergence_error.  Under slab sharding the ghosts' kappa_v goes out before the correction and their velocities
// after it, and the residual is summed over the ranks.
static int dfsph_divergence(SphHandle *h, bool first_derivative_done = false) {
    State &s = h->st;
    const SolveSpec sp{.slot = 0, .kind = 1, .thr = 0.001 * h->prm.density_0 / (double)s.c.dt,   // :150
                       .denom = (float)dfsph_particle_num(h), .max_itr = 1000, .fixed_err = 0.0f,   // :212 divides by particle_num
                       .iter = &h->last.iter_divergence, .err = &h->last.err_divergence, .batch_end = nullptr};
    int launched = 0;
    int rc = run_solve(h, sp, [&] {
        // DFSPH.py:140 compute_density_derivative before the loop (dfsph_step_end has it fused into the density + alpha walk)
        if (!first_derivative_done) { ProfScope p(h, SPH_K_DFSPH_RHO_ADV); h->L->dfsph_rho_adv(s, 0); }
    }, [&]() -> int {
        std::swap(s.kappa_v, s.kappa_v_next);  // DFSPH.py:133 compute_kappa_v: value of the last density-derivative pass
        if (s.slab_active) { int rc = slab_exchange_scalar(h, s.kappa_v); if (rc) return rc; }
        { ProfScope p(h, SPH_K_DFSPH_CORRECT); h->L->dfsph_correct(s, 0); }
        if (s.slab_active) { int rc = slab_exchange_vel(h); if (rc) return rc; }
        { ProfScope p(h, SPH_K_DFSPH_RHO_ADV); h->L->dfsph_rho_adv(s, 0); }
        return s.slab_active ? slab_finish_reduction(h, 0) : SPH_OK;
    }, &launched);
    if (rc) return rc;
    if ((launched - h->last.iter_divergence) & 1) std::swap(s.kappa_v, s.kappa_v_next);   // iterations past the stop did not run
    return SPH_OK;
}

// DFSPH.py:225 correct_density_error (sharded as the divergence solve)
static int dfsph_density(SphHandle *h) {
    State &s = h->st;
    const SolveSpec sp{.slot = 1, .kind = 1, .thr = 0.0001, .denom = (float)dfsph_particle_num(h), .max_itr = 1000,   // :239, :293
                       .fixed_err = 0.0f, .iter = &h->last.iter_density, .err = &h->last.err_density, .batch_end = nullptr};
    int launched = 0;
    int rc = run_solve(h, sp, [&] { ProfScope p(h, SPH_K_DFSPH_RHO_ADV); h->L->dfsph_rho_adv(s, 1); }, [&]() -> int {
        std::swap(s.kappa, s.kappa_next);      // DFSPH.py:218 compute_kappa
        if (s.slab_active) { int rc = slab_exchange_scalar(h, s.kappa); if (rc) return rc; }
        { ProfScope p(h, SPH_K_DFSPH_CORRECT); h->L->dfsph_correct(s, 1); }
        if (s.slab_active) { int rc = slab_exchange_vel(h); if (rc) return rc; }
        { ProfScope p(h, SPH_K_DFSPH_RHO_ADV); h->L->dfsph_rho_adv(s, 1); }
        return s.slab_active ? slab_finish_reduction(h, 1) : SPH_OK;
    }, &launched);
    if (rc) return rc;
    if ((launched - h->last.iter_density) & 1) std::swap(s.kappa, s.kappa_next);
    return SPH_OK;
}

// DFSPH.py:298 _step, first half: up to (not including) rigid_solver.step() / insert_object() at :305-:308
static int dfsph_step_begin(SphHandle *h) {
    State &s = h->st;
    if (h->sort_dirty) {
        // particles were appended outside a step (plain C-ABI use): the passes below walk the cell lists, so bring them
        // (and density / alpha, which the reference refreshes after every sort, DFSPH.py:316-318) up to date first.
        // Sharded: the re-sort invalidates the halo slot tables, so it has to be the full slab search (classify, exchange,
        // sort, tables) -- a COLLECTIVE: every rank of a sharded DFSPH scene that appends between steps gets here together
        // (the Python containers append mid-step and re-sort in step_end; this is the plain C-ABI path).
        if (s.slab_active) { int rc = slab_neighbor_search(h); if (rc) return rc; }
        else ph_neighbor_search(h);
        ph_rigid_volume(h);
        { ProfScope p(h, SPH_K_DFSPH_DENSITY_ALPHA); h->L->dfsph_density_alpha(s); }
        if (s.slab_active) { int rc = slab_exchange_scalar(h, s.rho.cur()); if (rc) return rc; }   // ghost densities, as in dfsph_step_end
    }
    int rc = run_non_pressure(h); if (rc) return rc;                          // DFSPH.py:299-300
    if (s.slab_active) { rc = slab_exchange_vel(h); if (rc) return rc; }      // the density solver reads v_j of the ghosts
    rc = dfsph_density(h); if (rc) return rc;                                 // :301
    // the sort of this step's second half follows at once when the whole step is one call (step_once): the position update hashes for it
    const bool hash_next = h->whole_step && !s.slab_active && s.c.all_fluid && !s.has_emitter && !h->any_rigid_object &&
                           !h->sort_dirty && !h->pose_dirty && !h->em_touch;
    { ProfScope p(h, SPH_K_MISC); h->L->advect_boundary(s, hash_next); }      // :303, :311-314 (boundary fused: it only looks at the particle itself)
    return SPH_OK;
}

// second half: :309 renew_rigid_particle_state and :311 boundary for what the host just inserted (step_insert_tail),
// then :316-:319
static int dfsph_step_end(SphHandle *h) {
    State &s = h->st;
    if (s.slab_active) { int rc = slab_neighbor_search(h); if (rc) return rc; }   // + migration / ghost exchange
    else ph_neighbor_search(h, true);                                         // :316 (the density pass below rewrites every rho: the sort need not move it)
    ph_rigid_volume(h);
    { ProfScope p(h, SPH_K_DFSPH_DENSITY_ALPHA); h->L->dfsph_density_alpha_div(s); }     // :317-318 + the D rho / Dt of :140
    if (s.slab_active) { int rc = slab_exchange_scalar(h, s.rho.cur()); if (rc) return rc; }   // ghost densities (kappa_j / rho_j, viscosity)
    return dfsph_divergence(h, true);                                         // :319
}

// PCISPH.py:110 refine.  Under slab sharding the ghosts' p / rho^2 goes out between the two passes of an
// iteration and their predicted positions after it; the density error is summed over the ranks.
static int pcisph_refine(SphHandle *h) {
    State &s = h->st;
    const SolveSpec sp{.slot = 2, .kind = 2, .thr = 0.001,                                                   // :122
                       .denom = (float)(s.slab_active ? h->comm_nfluid_global : (long long)h->n_fluid),   // :43-46 divides by fluid_particle_num
                       .max_itr = 1000, .fixed_err = 100.0f,                                              // :157
                       .iter = &h->last.iter_pcisph, .err = &h->last.err_pcisph, .batch_end = nullptr};
    return run_solve(h, sp, [] {}, [&]() -> int {
        { ProfScope p(h, SPH_K_PCISPH_RHO_STAR); h->L->pcisph_rho_star(s); }
        if (s.slab_active) { int rc = slab_exchange_scalar(h, s.ptm); if (rc) return rc; }
        { ProfScope p(h, SPH_K_PCISPH_PRESSURE_ACCEL); h->L->pcisph_pressure_accel(s); }
        if (s.slab_active) { int rc = slab_exchange_vel(h, s.ppos); if (rc) return rc; }
        return s.slab_active ? slab_finish_reduction(h, 2) : SPH_OK;
    });
}

static int pcisph_step(SphHandle *h) {
    State &s = h->st;
    SortCarry carry;
    if (s.slab_active) { int rc = slab_neighbor_search(h); if (rc) return rc; }   // + migration / ghost exchange
    else carry = ph_neighbor_search(h, true, true);                           // PCISPH.py:166 (:167 below rewrites every rho and moves what the sort leaves to it)
    ph_rigid_volume(h);
    { ProfScope p(h, SPH_K_DENSITY); h->L->density(s, 0, {0, false, carry}); } // :167
    if (s.slab_active) { int rc = slab_exchange_scalar(h, s.rho.cur()); if (rc) return rc; }   // ghost densities (viscosity)
    int rc = run_non_pressure(h); if (rc) return rc;                          // :168 (+ :174, v* kept aside)
    { ProfScope p(h, SPH_K_MISC); h->L->pcisph_init(s); }                     // :169
    if (s.slab_active) { rc = slab_exchange_vel(h, s.ppos); if (rc) return rc; }   // predicted positions of the ghosts
    rc = pcisph_refine(h); if (rc) return rc;                                 // :170
    { ProfScope p(h, SPH_K_PRESSURE_INTEGRATE); h->L->pressure_integrate(s); } // :175-177, :185
    return SPH_OK;
}

// IISPH.py:185 refine, one iteration (also the phase SPH_PH_IISPH_ITERATION)
static void iisph_iteration(SphHandle *h) {
    State &s = h->st;
    { ProfScope p(h, SPH_K_IISPH_DIJ_PJ); h->L->iisph_dij_pj(s); }     // :188
    { ProfScope p(h, SPH_K_IISPH_SUM_I); h->L->iisph_sum_i(s); }       // :189-190 (+ the error's partial sums)
}

// IISPH.py:185 refine: relaxed Jacobi, at least one iteration, stops when the average density error drops below eta (a negative
// error stops it too) or after max_iterations.  Stop test kind 2: error < (float)eta, error = sum / (fluid_particle_num rho0),
// :118-121.  fixed_iterations > 0: exactly that many, error reported 0.
static int iisph_refine(SphHandle *h) {
    const SolveSpec sp{.slot = 2, .kind = 2, .thr = SPH_IISPH_ETA, .denom = (float)h->n_fluid * (float)h->prm.density_0,   // :194-197
                       .max_itr = SPH_IISPH_MAX_ITER, .fixed_err = 0.0f, .iter = &h->last.iter_iisph, .err = &h->last.err_iisph,
                       .batch_end = nullptr};
    return run_solve(h, sp, [] {}, [h] { iisph_iteration(h); return (int)SPH_OK; });
}

// IISPH.py:203 _step up to the rigid solver: the sort, compute_density (no EOS), init_step + non-pressure forces + v* (:206-208, the
// pressures are cleared by the prepare pass), dii / aii / rho* (:210-213), refine (:215), pressure acceleration + v, x update +
// boundary (:218-220, :227: the same tail as PCISPH's)
static int iisph_step(SphHandle *h) {
    State &s = h->st;
    const SortCarry carry = ph_neighbor_search(h, true, true);                // :204 (:205 below rewrites every rho and moves what the sort leaves to it)
    ph_rigid_volume(h);
    { ProfScope p(h, SPH_K_DENSITY); h->L->density(s, 0, {0, false, carry}); } // :205
    int rc = run_non_pressure(h); if (rc) return rc;                          // :207-208
    { ProfScope p(h, SPH_K_IISPH_PREPARE); h->L->iisph_prepare(s); }          // :206, :210-213
    rc = iisph_refine(h); if (rc) return rc;                                  // :215
    { ProfScope p(h, SPH_K_PRESSURE_INTEGRATE); h->L->pressure_integrate(s); } // :218-220, :227
    return SPH_OK;
}

// PBF.py:145 _step, whole: the sort (it carries rho: compute_non_pressure_acceleration reads the densities the previous step's last
// refine iteration left, PBF.py:146-147), the non-pressure forces + v* with poly6 / spiky kernels (:147-148), save_old_position +
// x += dt v + boundary (:149-152), five refine iterations on the cell lists of this step's sort (:154, :62-66), boundary + v =
// (x - x_old) / dt (:156-158).  No rigid_solver.step(), no insert_object(), no renew_rigid_particle_state: PBF.py calls none of
// them.  Nothing is read back: fixed iteration count, asynchronous steps allowed.
static void pbf_begin_count(SphHandle *h) {
    State &s = h->st;
    h->pbf_bank = s.c.stat_bank;
    hipMemsetAsync(s.pbf_recentred + s.c.stat_bank, 0, sizeof(unsigned long long), s.stream);
}

static int pbf_step(SphHandle *h) {
    State &s = h->st;
    pbf_begin_count(h);
    ph_neighbor_search(h);                                                    // :146 (it carries rho, see above)
    ph_rigid_volume(h);
    int rc = run_non_pressure(h); if (rc) return rc;                          // :147-148
    { ProfScope p(h, SPH_K_PBF_UPDATE); h->L->pbf_predict(s); }               // :149-152
    for (int k = 0; k < SPH_PBF_ITERATIONS; ++k) {                            // :154 refine
        { ProfScope p(h, SPH_K_PBF_DENSITY_LAMBDA); h->L->pbf_density_lambda(s); }
        { ProfScope p(h, SPH_K_PBF_FIX_POSITION); h->L->pbf_fix_position(s); }
    }
    { ProfScope p(h, SPH_K_PBF_UPDATE); h->L->pbf_finish(s); }                // :156-158
    return SPH_OK;
}

// The consistent PBF variant, one iteration: walk A (rho, lambda, partial sums of C), walk B (the Jacobi correction of
// x*) and, with `reduce`, the reduction of A's sums behind B -- inside a device-controlled loop that is where the stop test runs, so
// the iteration that meets it still applies its correction.
static void pbfc_iteration(SphHandle *h, int reduce) {
    State &s = h->st;
    { ProfScope p(h, SPH_K_PBFC_DENSITY_LAMBDA); h->L->pbfc_density_lambda(s, 0); }
    { ProfScope p(h, SPH_K_PBFC_DELTA); h->L->pbfc_delta(s, reduce); }
}

// Stop after the first iteration k >= min_iterations with err_k = sum C / fluid_particle_num <= max_error (kind 1), or after
// max_iterations.  The first min_iterations - 1 iterations carry no stop test: they go out in front of the loop.  Reduction slot 3
// (the CG solve's elsewhere: PBF refuses implicit viscosity, so no other solve of a PBF handle uses it).
static int pbfc_solve(SphHandle *h) {
    State &s = h->st;
    const int fixed = h->prm.fixed_iterations;
    const int pre_n = fixed > 0 ? 0 : h->pbf.min_iterations - 1;
    const SolveSpec sp{.slot = 3, .kind = 1, .thr = (double)h->pbf.max_error, .denom = (float)h->n_fluid,
                       .max_itr = h->pbf.max_iterations - pre_n, .fixed_err = 0.0f,
                       .iter = &h->pbf_last.iterations, .err = &h->pbf_last.error, .batch_end = nullptr};
    int launched = 0;
    int rc = run_solve(h, sp, [&] { for (int k = 0; k < pre_n; ++k) pbfc_iteration(h, 0); },
                       [&]() -> int { pbfc_iteration(h, 1); return (int)SPH_OK; }, &launched);
    if (rc) return rc;
    if (fixed <= 0) {
        if ((launched - h->pbf_last.iterations) & 1) std::swap(s.pbf_old, s.pbf_pos);   // iterations past the stop did not run: their swaps go back
        h->pbf_last.iterations += pre_n;
    }
    return SPH_OK;
}

// One step: the sort, the rigid volumes, the density at the sorted positions (it stores the acceptance masks every later walk of the
// step reuses, and is the density the viscosity reads), v* = v + dt a with the cubic kernel, x* = x + dt v*, the solve, the finish.
// As under the reference variant: no rigid_solver.step(), no insert_object().
static int pbfc_step(SphHandle *h) {
    State &s = h->st;
    const SortCarry carry = ph_neighbor_search(h, true, true);
    ph_rigid_volume(h);
    { ProfScope p(h, SPH_K_DENSITY); h->L->density(s, 0, {0, false, carry}); }
    int rc = run_non_pressure(h); if (rc) return rc;
    { ProfScope p(h, SPH_K_PBF_UPDATE); h->L->pbfc_predict(s); }
    rc = pbfc_solve(h); if (rc) return rc;
    { ProfScope p(h, SPH_K_PBF_UPDATE); h->L->pbfc_finish(s); }
    return SPH_OK;
}

// host replica of PCISPH.py:129 compute_pcisph_k (same arithmetic as oracle/sph_ref.c)
static float host_pcisph_k(const SphParams &p) {
    const double hd = p.support_radius;
    const float hf = (float)hd;
    float kg = (float)(8.0 / M_PI);
    kg = 6.0f * kg / (float)(hd * hd * hd);
    const float diam = (float)(2.0 * p.particle_radius * 0.97);
    float sx = 0.f, sy = 0.f, sz = 0.f, s2 = 0.f;
    const int max_i = (int)(hf / diam) + 1;
    for (int i = -max_i; i <= max_i; i++)
        for (int j = -max_i; j <= max_i; j++)
            for (int k = -max_i; k <= max_i; k++) {
                const float rx = 0.0f - (float)i * diam, ry = 0.0f - (float)j * diam, rz = 0.0f - (float)k * diam;
                const float rn = sqrtf(rx * rx + ry * ry + rz * rz);
                if (rn < hf) {
                    float gx = 0.f, gy = 0.f, gz = 0.f;
                    const float q = rn / hf;
                    if (rn > 1e-5f && q <= 1.0f) {
                        const float den = rn * hf;
                        float sc;
                        if (q <= 0.5f) sc = kg * q * (3.0f * q - 2.0f);
                        else { const float f = 1.0f - q; sc = kg * (-f * f); }
                        gx = sc * (rx / den); gy = sc * (ry / den); gz = sc * (rz / den);
                    }
                    sx += gx; sy += gy; sz += gz;
                    s2 += gx * gx + gy * gy + gz * gz;
                }
            }
    const float dtV0 = (float)p.dt * (float)p.V0;
    return -0.5f / dtV0 / dtV0 / ((sx * sx + sy * sy + sz * sz) + s2);
}

static int method_prepare(SphHandle *h) {
    State &s = h->st;
    if (h->prm.method == SPH_METHOD_DFSPH) {  // DFSPH.py:321-324
        { ProfScope p(h, SPH_K_DFSPH_DENSITY_ALPHA); h->L->dfsph_density_alpha(s); }
        if (s.slab_active) { int rc = slab_exchange_scalar(h, s.rho.cur()); if (rc) return rc; }
    } else if (h->prm.method == SPH_METHOD_PCISPH) {  // PCISPH.py:188-190
        s.c.pcisph_k = host_pcisph_k(h->prm);
    }
    return SPH_OK;
}

static int method_run_phase(SphHandle *h, int phase) {
    State &s = h->st;
    if (h->prm.method == SPH_METHOD_DFSPH) {
        switch (phase) {
            case SPH_PH_DFSPH_ALPHA: { ProfScope p(h, SPH_K_DFSPH_DENSITY_ALPHA); h->L->dfsph_density_alpha(s); } return SPH_OK;
            case SPH_PH_DFSPH_DIVERGENCE: return dfsph_divergence(h);
            case SPH_PH_DFSPH_DENSITY: return dfsph_density(h);
            case SPH_PH_DFSPH_ALPHA_DIVERGENCE: {   // dfsph_step_end behind the sort and the rigid volumes (unsharded: no exchanges)
                { ProfScope p(h, SPH_K_DFSPH_DENSITY_ALPHA); h->L->dfsph_density_alpha_div(s); }
                return dfsph_divergence(h, true);
            }
            default: break;
        }
    } else if (h->prm.method == SPH_METHOD_PCISPH) {   // the passes of pcisph_step / pcisph_refine one by one (unsharded: no exchanges)
        switch (phase) {
            case SPH_PH_PCISPH_INIT: { ProfScope p(h, SPH_K_MISC); h->L->pcisph_init(s); } return SPH_OK;
            case SPH_PH_PCISPH_RHO_STAR: {   // the first walk of an iteration, no stop test; its density error is read back
                { ProfScope p(h, SPH_K_PCISPH_RHO_STAR); h->L->pcisph_rho_star(s); }
                { ProfScope p(h, SPH_K_REDUCE); h->L->pcisph_reduce_error(s); }   // (inside a step the second walk's launcher finishes these sums)
                float sum = 0.0f;
                int rc = read_red(h, 2, &sum); if (rc) return rc;
                h->last.iter_pcisph = 1; h->last.err_pcisph = h->n_fluid > 0 ? sum / (float)h->n_fluid : 0.0f;
                return SPH_OK;
            }
            case SPH_PH_PCISPH_PRESSURE_ACCEL: { ProfScope p(h, SPH_K_PCISPH_PRESSURE_ACCEL); h->L->pcisph_pressure_accel(s); } return SPH_OK;   // (adds the same partial sums up once more, as in a step)
            default: break;
        }
    } else if (h->prm.method == SPH_METHOD_IISPH) {
        switch (phase) {
            case SPH_PH_IISPH_PREPARE: { ProfScope p(h, SPH_K_IISPH_PREPARE); h->L->iisph_prepare(s); } return SPH_OK;
            case SPH_PH_IISPH_ITERATION: {   // one iteration of the step's refine, no stop test; its error is read back
                iisph_iteration(h);
                float sum = 0.0f;
                int rc = read_red(h, 2, &sum); if (rc) return rc;
                const float denom = (float)h->n_fluid * (float)h->prm.density_0;
                h->last.iter_iisph = 1; h->last.err_iisph = h->n_fluid > 0 ? sum / denom : 0.0f;
                return SPH_OK;
            }
            default: break;
        }
    } else if (h->prm.method == SPH_METHOD_PBF && h->pbf.variant == SPH_PBF_VARIANT_CONSISTENT) {
        switch (phase) {
            case SPH_PH_PBFC_PREDICT: { ProfScope p(h, SPH_K_PBF_UPDATE); h->L->pbfc_predict(s); } return SPH_OK;
            case SPH_PH_PBFC_DENSITY_LAMBDA: {   // its mean C is read back
                { ProfScope p(h, SPH_K_PBFC_DENSITY_LAMBDA); h->L->pbfc_density_lambda(s, 1); }
                float sum = 0.0f;
                int rc = read_red(h, 3, &sum); if (rc) return rc;
                h->pbf_last.iterations = 1; h->pbf_last.error = h->n_fluid > 0 ? sum / (float)h->n_fluid : 0.0f;
                return SPH_OK;
            }
            case SPH_PH_PBFC_DELTA: { ProfScope p(h, SPH_K_PBFC_DELTA); h->L->pbfc_delta(s, 0); } return SPH_OK;
            case SPH_PH_PBFC_FINISH: { ProfScope p(h, SPH_K_PBF_UPDATE); h->L->pbfc_finish(s); } return SPH_OK;
            default: break;
        }
    } else if (h->prm.method == SPH_METHOD_PBF) {   // one refine walk on the current positions and the last sort's cell lists
        switch (phase) {
            case SPH_PH_PBF_DENSITY_LAMBDA: { pbf_begin_count(h); ProfScope p(h, SPH_K_PBF_DENSITY_LAMBDA); h->L->pbf_density_lambda(s); } return SPH_OK;
            case SPH_PH_PBF_FIX_POSITION: { pbf_begin_count(h); ProfScope p(h, SPH_K_PBF_FIX_POSITION); h->L->pbf_fix_position(s); } return SPH_OK;
            case SPH_PH_PBF_PREDICT: { ProfScope p(h, SPH_K_PBF_UPDATE); h->L->pbf_predict(s); } return SPH_OK;
            case SPH_PH_PBF_FINISH: { ProfScope p(h, SPH_K_PBF_UPDATE); h->L->pbf_finish(s); } return SPH_OK;
            default: break;
        }
    }
    return fail(h, SPH_ERR_INVALID, "unknown phase %d for method %d", phase, h->prm.method);
}

#include "sph_cg_steps.hpp"
