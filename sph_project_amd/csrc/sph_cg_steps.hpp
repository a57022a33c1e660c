// sph_cg_steps.hpp -- implicit viscosity (base_solver.py:509 implicit_viscosity_solve) orchestration
#pragma once

// gravity + surface tension + implicit viscosity + v += dt a  (base_solver.py:190-198, :643)
static int implicit_viscosity_non_pressure(SphHandle *h) {
    State &s = h->st;
    const bool slab = s.slab_active != 0;
    // few fluid particles (the buckling sheet of C5: 106 k of 2.2 M particles = 416 tiles, one wave per SIMD): every A p pass is
    // pure latency; splitting it by x-offset group triples the waves in flight (PassSplit).  A scene that fills the chip
    // anyway (> ~1500 tiles) gains nothing from it and keeps the single launch.
    // (A two-way split, groups {0, 1} and {2}, was measured slower at C5: 1.639 -> 1.757 ms/step.)
    s.cg_split = (h->n_fluid > 0 && h->n_fluid <= 400000) ? 3 : 0;
    // Slab sharding: the ghosts are the neighbour ranks' rows of the system.  Their search direction goes out before every
    // A p pass (12 B per ghost through the slot tables), the three dot products of an iteration are summed over the ranks
    // (k_cg_fold + one 1-float and one 2-float all-reduce), and the solved velocities of the ghosts after the loop.
    auto refresh = [&](float4 *arr) -> int { return slab ? slab_exchange_vel(h, arr) : SPH_OK; };
    auto dots = [&](int which) -> int {
        if (!slab) return SPH_OK;
        { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_fold(s, which); }
        return which == 1 ? slab_allreduce_dev(h, &s.scal->red[7], 1) : slab_allreduce_dev(h, &s.scal->red[6], which == 0 ? 1 : 2);
    };
    // One CG iteration = A p pass (+ combine when split), x / r update, p update.  Unsharded, the p update is folded into the
    // NEXT iteration's A p pass (CgApPass::fuse: p = r + beta p_old on the fly while staging; beta, the error and the stop flag
    // come from the x / r update's partials): two or three launches per iteration instead of three or four.  Sharded, the
    // ghosts' p has to exist in memory to be exchanged, so the p update stays a kernel of its own.
    const bool fused = !slab && s.cg_p2;
    s.cg_fused_loop = 0;   // (set for the loop only: the A p pass in front of it feeds prepare2 through cg_Ap)
    bool first = true;
    auto iteration = [&]() -> int {
        int rc = refresh(s.cg_p); if (rc) return rc;
        { ProfScope p(h, SPH_K_CG_AP); h->L->cg_ap(s, fused && !first); }
        rc = dots(1); if (rc) return rc;
        { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_update_xr(s); }
        rc = dots(2); if (rc) return rc;
        if (!fused) { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_update_p(s); }
        first = false;
        return SPH_OK;
    };
    { ProfScope p(h, SPH_K_CG_PREPARE); h->L->cg_prepare(s); }                     // :510
    int rc = refresh(s.cg_p); if (rc) return rc;                                   // the ghosts' initial guess
    { ProfScope p(h, SPH_K_CG_AP); h->L->cg_ap(s, false); }                        // :511
    { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_prepare2(s); h->L->cg_alpha(s); }  // :512 (+ |r0|^2 for the first alpha)
    rc = dots(0); if (rc) return rc;
    // :445 conjugate_gradient_loop; tol starts at 1000 (:446), the residual reported with fixed_iterations
    const SolveSpec sp{.slot = 3, .kind = 3, .thr = 1e-6, .denom = 1.0f, .max_itr = 1000, .fixed_err = 1000.0f,
                       .iter = &h->last.iter_cg, .err = &h->last.err_cg, .batch_end = fused ? h->L->cg_check : nullptr};
    s.cg_fused_loop = fused ? 1 : 0;
    rc = run_solve(h, sp, [] {}, iteration);
    s.cg_fused_loop = 0;
    if (rc) return rc;
    rc = refresh(s.cg_x); if (rc) return rc;                                       // solved velocities of the ghosts (:514)
    // :514-516: the explicit viscosity formula evaluated with the solved velocities gives the acceleration; the
    // fused pass adds gravity + surface tension and advances the ORIGINAL velocities (:470, :643)
    s.skip_viscosity = 0;
    { ProfScope p(h, SPH_K_NON_PRESSURE); h->L->non_pressure(s, s.cg_x); }
    { ProfScope p(h, SPH_K_CG_VECTOR); h->L->cg_prepare_guess(s); }                // :517
    return SPH_OK;
}
