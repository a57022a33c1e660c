// sph_cg_steps.hpp -- implicit viscosity (base_solver.py:509 implicit_viscosity_solve) orchestration
#pragma once

// The solve in pieces: implicit_viscosity_non_pressure() below is their sequence, and the phases SPH_PH_CG_* (cg_run_phase) run them one
// by one.  What one piece leaves for the next lives in State: cg_split, cg_fused_loop (the loop folds the p update into the next A p
// pass), cg_first (the next A p pass of the loop is the first one: nothing to fold in yet), cg_parity.

// Slab sharding: the ghosts are the neighbour ranks' rows of the system.  Their search direction goes out before every
// A p pass (12 B per ghost through the slot tables), the three dot products of an iteration are summed over the ranks
// (k_cg_fold + one 1-float and one 2-float all-reduce), and the solved velocities of the ghosts after the loop.
static int cg_refresh(SphHandle *h, float4 *arr) { return h->st.slab_active ? slab_exchange_vel(h, arr) : SPH_OK; }
static int cg_dots(SphHandle *h, int which) {
    State &s = h->st;
    if (!s.slab_active) return SPH_OK;
    { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_fold(s, which); }
    return which == 1 ? slab_allreduce_dev(h, &s.scal->red[7], 1) : slab_allreduce_dev(h, &s.scal->red[6], which == 0 ? 1 : 2);
}

// prepare_conjugate_gradient_solver1, the A p pass in front of the loop, prepare_conjugate_gradient_solver2 (:510-512) and |r0|^2.
// Returns through *fused_out whether the loop folds the p update into the next A p pass.
static int cg_solve_prepare(SphHandle *h, bool *fused_out) {
    State &s = h->st;
    // few fluid particles (the buckling sheet of C5: 106 k of 2.2 M particles = 416 tiles, one wave per SIMD): every A p pass is
    // pure latency; splitting it by x-offset group triples the waves in flight (PassSplit).  A scene that fills the chip
    // anyway (> ~1500 tiles) gains nothing from it and keeps the single launch.
    // (A two-way split, groups {0, 1} and {2}, was measured slower at C5: 1.639 -> 1.757 ms/step.)
    int split_limit = 400000;
    // One CG iteration = A p pass (+ combine when split), x / r update, p update.  Unsharded, the p update is folded into the
    // NEXT iteration's A p pass (CgApPass::fuse: p = r + beta p_old on the fly while staging; beta, the error and the stop flag
    // come from the x / r update's partials): two or three launches per iteration instead of three or four.  Sharded, the
    // ghosts' p has to exist in memory to be exchanged, so the p update stays a kernel of its own.
    bool fused = !s.slab_active && s.cg_p2;
#ifdef SPH_TEST_HOOKS
    // test-hook library only (tests/test_hip_implicit_viscosity.py): SPH_TEST_CG_SPLIT_LIMIT=k replaces the 400000 above (0: the
    // unsplit A p pass on a scene of any size); SPH_TEST_CG_SEPARATE_P makes the unsharded loop run the sharded one's launches
    // (k_cg_ap_combine inside the loop, k_cg_update_p2) -- launch forms no small unsharded scene reaches otherwise
    if (const char *e = getenv("SPH_TEST_CG_SPLIT_LIMIT")) split_limit = atoi(e);
    if (getenv("SPH_TEST_CG_SEPARATE_P")) fused = false;
#endif
    s.cg_split = (h->n_fluid > 0 && h->n_fluid <= split_limit) ? 3 : 0;
    s.cg_fused_loop = 0;   // (set for the loop only: the A p pass in front of it feeds prepare2 through cg_Ap)
    s.cg_first = 1;
    { ProfScope p(h, SPH_K_CG_PREPARE); h->L->cg_prepare(s); }                     // :510
    int rc = cg_refresh(h, s.cg_p); if (rc) return rc;                             // the ghosts' initial guess
    { ProfScope p(h, SPH_K_CG_AP); h->L->cg_ap(s, false); }                        // :511
    { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_prepare2(s); h->L->cg_alpha(s); }  // :512 (+ |r0|^2 for the first alpha)
    rc = cg_dots(h, 0); if (rc) return rc;
    *fused_out = fused;
    return SPH_OK;
}

// the three launches of one iteration (with cg_fused_loop set the third is none: the next A p pass does its work)
static int cg_iteration_ap(SphHandle *h) {
    State &s = h->st;
    int rc = cg_refresh(h, s.cg_p); if (rc) return rc;
    const bool fuse = s.cg_fused_loop && !s.cg_first;
    s.cg_first = 0;
    { ProfScope p(h, SPH_K_CG_AP); h->L->cg_ap(s, fuse); }
    return cg_dots(h, 1);
}
static int cg_iteration_xr(SphHandle *h) {
    State &s = h->st;
    { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_update_xr(s); }
    return cg_dots(h, 2);
}
static int cg_iteration_p(SphHandle *h) {
    State &s = h->st;
    if (!s.cg_fused_loop) { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_update_p(s); }
    return SPH_OK;
}

// :514-517 behind the loop
static int cg_solve_end(SphHandle *h) {
    State &s = h->st;
    s.cg_fused_loop = 0;
    int rc = cg_refresh(h, s.cg_x); if (rc) return rc;                             // solved velocities of the ghosts (:514)
    // :514-516: the explicit viscosity formula evaluated with the solved velocities gives the acceleration; the
    // fused pass adds gravity + surface tension and advances the ORIGINAL velocities (:470, :643)
    s.skip_viscosity = 0;
    { ProfScope p(h, SPH_K_NON_PRESSURE); h->L->non_pressure(s, s.cg_x); }
    { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_prepare_guess(s); }                // :517
    return SPH_OK;
}

// gravity + surface tension + implicit viscosity + v += dt a  (base_solver.py:190-198, :643)
static int implicit_viscosity_non_pressure(SphHandle *h) {
    State &s = h->st;
    bool fused = false;
    int rc = cg_solve_prepare(h, &fused); if (rc) return rc;
    auto iteration = [&]() -> int {
        int rc = cg_iteration_ap(h); if (rc) return rc;
        rc = cg_iteration_xr(h); if (rc) return rc;
        return cg_iteration_p(h);
    };
    // :445 conjugate_gradient_loop; tol starts at 1000 (:446), the residual reported with fixed_iterations
    const SolveSpec sp{.slot = 3, .kind = 3, .thr = 1e-6, .denom = 1.0f, .max_itr = 1000, .fixed_err = 1000.0f,
                       .iter = &h->last.iter_cg, .err = &h->last.err_cg, .batch_end = fused ? h->L->cg_check : nullptr};
    s.cg_fused_loop = fused ? 1 : 0;
    rc = run_solve(h, sp, [] {}, iteration);
    if (rc) { s.cg_fused_loop = 0; return rc; }
    return cg_solve_end(h);
}

// The pieces as phases (sph_hip.h SPH_PH_CG_*): the step's own launcher calls, one pass each, no stop test (as a solve with
// fixed_iterations: s.loop_flag is null).  Unsharded only.
static int cg_run_phase(SphHandle *h, int phase) {
    State &s = h->st;
    if (!h->prm.viscosity_implicit) return fail(h, SPH_ERR_INVALID, "phase %d needs viscosity_implicit", phase);
    if (s.slab_active) return fail(h, SPH_ERR_UNSUPPORTED, "phase %d: not under slab sharding", phase);
    switch (phase) {
        case SPH_PH_CG_PREPARE: {
            bool fused = false;
            int rc = cg_solve_prepare(h, &fused); if (rc) return rc;
            s.cg_fused_loop = fused ? 1 : 0;
            return SPH_OK;
        }
        case SPH_PH_CG_AP: return cg_iteration_ap(h);
        case SPH_PH_CG_UPDATE_XR: return cg_iteration_xr(h);
        case SPH_PH_CG_UPDATE_P: return cg_iteration_p(h);
        case SPH_PH_CG_END: return cg_solve_end(h);
        default: break;
    }
    return fail(h, SPH_ERR_INVALID, "unknown phase %d", phase);
}
