/*
 * include/sph_hip.h -- C-ABI of libsph_hip.so, the MI355X (gfx950) SPH hot path.
 *
 * The reference (jason-huang03/SPH_Project) is 100 % Python + Taichi and has no FFI of its
 * own; this header is the boundary a reference-side binding would target (ctypes stub in
 * INTEGRATION.md).  Each entry point names the reference interface it replaces (paths
 * relative to the reference root).  Conventions:
 *   - plain pointers and sizes only; the caller owns every host buffer (C-contiguous
 *     f32 / i32), the library owns all device memory behind the opaque handle;
 *   - every call returns 0 or a negative SphStatus; text via sph_last_error();
 *     HIP / RCCL failures are captured, never fatal, nothing throws across the ABI;
 *   - one host thread per handle; one HIP compute stream (+ one comm stream) per handle;
 *   - python-side quantities of the reference are doubles here and are rounded to f32
 *     exactly where a reference Taichi kernel would consume them.
 */
#ifndef SPH_HIP_H
#define SPH_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SPH_MAX_OBJECTS 20 /* SPH/containers/base_container.py:52 max_num_object */
#define SPH_MAT_FLUID 1    /* base_container.py:30 */
#define SPH_MAT_RIGID 2    /* base_container.py:29 */

typedef enum {
    SPH_OK = 0,
    SPH_ERR_INVALID = -1,   /* bad argument / bad state */
    SPH_ERR_CAPACITY = -2,  /* particle_max_num exceeded */
    SPH_ERR_HIP = -3,       /* HIP runtime error (text in sph_last_error) */
    SPH_ERR_NO_DEVICE = -4, /* no gfx950 device visible */
    SPH_ERR_COMM = -5,      /* RCCL error */
    SPH_ERR_UNSUPPORTED = -6
} SphStatus;

/* SPH_METHOD_IISPH: SPH/fluid_solvers/IISPH.py as written (omega 0.2, eta 0.001, at most 20 relaxed-Jacobi iterations, :12-14),
   with ONE deviation: for a rigid neighbour, compute_dii (:40-44) divides by rho_i^2 -- the density this step's compute_density
   wrote for particle i -- where the reference reads particle_densities_star[p_i], which it has not computed yet in that step
   (zero on the first step: division by zero) and which its sort does not move (another particle's value afterwards).  rho_i
   is the d_ii of the IISPH paper and is defined at every step.  All-fluid scenes never take that branch.  Single GPU only:
   a sharded handle (sph_comm_set_slab) fails in sph_prepare with SPH_ERR_UNSUPPORTED. */
/* SPH_METHOD_PBF: SPH/fluid_solvers/PBF.py (Position Based Fluids; 5 refine iterations, lambda_eps 100, corrK 0.001, deltaQ 0.3 h,
   :11-13), poly6 W and spiky gradient in EVERY sum of its step (surface tension, viscosity, rigid volumes included).  The refine walks
   use the step-start cell lists with the centre cell and the distances taken from the CURRENT positions (base_container.py:550-560).
   Two deviations: fix_position is Jacobi (all deltas from the positions at the start of the pass, then applied: the reference's
   in-place update is a data race in parallel), and the PBF fields are sized particle_max_num (the reference sizes them with a
   particle_num that is still 0).  Under PBF, objects with a later entryTime are never inserted and rigid bodies never move (PBF.py's
   _step calls neither).  sph_prepare refuses (SPH_ERR_UNSUPPORTED) a sharded handle and viscosity_implicit.
   That is the "reference" variant, the default.  sph_set_pbf_variant selects the "consistent" one instead: the
   project's cubic spline in every sum, a density with its self term, the one-sided constraint C = max(rho / rho0 - 1, 0), lambda =
   -C / (sum |G|^2 + |sum G|^2 + eps), a Jacobi correction of predicted positions x* with the neighbour set fixed at the step's
   sort, and a stop test on the mean C.  The method id stays SPH_METHOD_PBF; what the reference variant refuses, this one refuses. */
typedef enum { SPH_METHOD_WCSPH = 0, SPH_METHOD_DFSPH = 1, SPH_METHOD_PCISPH = 2, SPH_METHOD_IISPH = 3, SPH_METHOD_PBF = 4 } SphMethod;

/* Scene / solver constants.  Mirrors what BaseContainer.__init__ (base_container.py:10-60)
   and BaseSolver.__init__ (SPH/fluid_solvers/base_solver.py:9-54) derive from the JSON. */
typedef struct {
    double domain_size[3];   /* base_container.py:23 (domainStart must be 0, run_simulation.py:11) */
    double particle_radius;  /* :33 dx */
    double support_radius;   /* :37 dh = 4 dx (or "supportRadius") = grid cell size :55 */
    double V0;               /* :49 0.8 * diameter^3 */
    double padding;          /* :58 */
    int32_t grid_num[3];     /* :56 ceil(domain_size / dh) */
    double gravity[3];       /* base_solver.py:16 */
    double g_upper;          /* :21-23 gravitationUpper (10000 if absent) */
    double viscosity;        /* :26 */
    double viscosity_b;      /* :27-29 */
    double density_0;        /* :31 */
    double surface_tension;  /* :32 (0.01) */
    double dt;               /* :36 timeStepSize */
    int32_t particle_max_num;/* base_container.py:116 */
    int32_t viscosity_implicit; /* base_solver.py:40 viscosityMethod == "implicit" */
    int32_t method;          /* SphMethod; run_simulation.py:46-63 */
    int32_t fixed_iterations;/* 0: reference stopping rules; >0: exactly this many DFSPH/PCISPH/IISPH/CG iterations */
    int32_t fast_math;       /* 0: IEEE div/sqrt, no FMA contraction; 1: v_rcp/v_rsq + FMA */
    int32_t device;          /* HIP device ordinal, -1: current */
    int32_t force_global;    /* debug mode of the neighbour passes: 0 normal; 1 every candidate run through the tile in chunks; 4 every group down the ordered walk; ... */
    int32_t deterministic;   /* 1: stable within-cell order (bit-reproducible sums) */
} SphParams;

typedef struct SphHandle SphHandle;

/* Per-particle fields addressable by sph_download / sph_upload.  Layouts are the reference's
   (base_container.py:138-185; dfsph_container.py:13-17; pcisph_container.py:15-19), in the
   current sorted order of the container (as BaseContainer.dump, base_container.py:599). */
typedef enum {
    SPH_F_POSITION = 0,      /* f32[n][3] particle_positions */
    SPH_F_VELOCITY = 1,      /* f32[n][3] particle_velocities */
    SPH_F_ACCELERATION = 2,  /* f32[n][3] particle_accelerations */
    SPH_F_DENSITY = 3,       /* f32[n]    particle_densities */
    SPH_F_PRESSURE = 4,      /* f32[n]    particle_pressures */
    SPH_F_REST_VOLUME = 5,   /* f32[n]    particle_rest_volumes */
    SPH_F_MASS = 6,          /* f32[n]    particle_masses */
    SPH_F_MATERIAL = 7,      /* i32[n]    particle_materials */
    SPH_F_OBJECT_ID = 8,     /* i32[n]    particle_object_ids */
    SPH_F_IS_DYNAMIC = 9,    /* i32[n]    particle_is_dynamic */
    SPH_F_COLOR = 10,        /* i32[n][3] particle_colors */
    SPH_F_PARTICLE_ID = 11,  /* i32[n]    insertion index (not in the reference; lets tests match particles) */
    SPH_F_GRID_ID = 12,      /* i32[n]    reference flat cell id (ix*ny+iy)*nz+iz, base_container.py:473 */
    SPH_F_DFSPH_ALPHA = 13,  /* f32[n] */
    SPH_F_DFSPH_KAPPA = 14,  /* f32[n] */
    SPH_F_DFSPH_KAPPA_V = 15,/* f32[n] */
    SPH_F_DENSITY_STAR = 16, /* f32[n] */
    SPH_F_DENSITY_DERIV = 17,/* f32[n] */
    SPH_F_PRESSURE_ACCEL = 18,   /* f32[n][3] pcisph particle_pressure_accelerations */
    SPH_F_PREDICTED_VEL = 19,    /* f32[n][3] */
    SPH_F_PREDICTED_POS = 20,    /* f32[n][3] (PCISPH; on a consistent-PBF handle: x*, download and upload) */
    SPH_F_CG_X = 21,             /* f32[n][3] base_solver.py:46 */
    SPH_F_ORIG_POSITION = 22,    /* f32[n][3] rigid_particle_original_positions */
    SPH_F_GHOST = 23,            /* i32[n]    1 for ghost copies of a neighbour slab's particles (multi-GPU), else 0 */
    /* solver scratch the per-term checks of tests/test_hip_solvers.py need (not fields of the reference: DFSPH.py:133 / :218 recompute
       kappa from density_star / density_derivative + alpha right before every correction; this library computes it in the pass that
       produces them and hands it to the next correction): */
    SPH_F_DFSPH_KAPPA_NEXT = 24,   /* f32[n] (rho*_i - 1) alpha_i / dt of the LAST density_star pass (pairs with SPH_F_DENSITY_STAR) */
    SPH_F_DFSPH_KAPPA_V_NEXT = 25, /* f32[n] D rho_i / Dt * alpha_i of the LAST density_derivative pass (pairs with SPH_F_DENSITY_DERIV) */
    SPH_F_DEBUG_CAPTURE = 26,      /* f32[n] libsph_hip_testhooks.so only: PCISPH pressure BEFORE the last executed update_pressure
                                      (PCISPH.py:66-73); the production library leaves the density pass's scratch there */
    /* IISPH (iisph_container.py:14-20; allocated for SPH_METHOD_IISPH only; rho* is SPH_F_DENSITY_STAR, IISPH.py:71): */
    SPH_F_IISPH_DII = 27,          /* f32[n][3] dii    (IISPH.py:18 compute_dii, rigid term: see SphMethod) */
    SPH_F_IISPH_AII = 28,          /* f32[n]    iisph_aii (IISPH.py:47 compute_aii) */
    SPH_F_IISPH_DIJ_PJ = 29,       /* f32[n][3] dij_pj (IISPH.py:125 compute_dij_pj, last executed iteration) */
    SPH_F_IISPH_SUM_I = 30,        /* f32[n]    sum_i  (IISPH.py:148 compute_sum_i, last executed iteration) */
    /* PBF (pbf_container.py:11-13; allocated for SPH_METHOD_PBF only, particle_max_num): */
    SPH_F_PBF_OLD_POSITION = 31,   /* f32[n][3] particle_old_positions (PBF.py:145 save_old_position: the positions at the step's sort) */
    SPH_F_PBF_LAMBDA = 32,         /* f32[n]    particle_pbf_lambdas (PBF.py:68 compute_lambda, last executed iteration; a consistent-PBF
                                                handle also takes it in sph_upload, and refuses SPH_F_PBF_OLD_POSITION: SPH_F_POSITION
                                                holds the old positions for the whole step) */
    /* rigid contact (allocated by sph_set_rigid_contact; written for contact targets only, zeroed by SPH_PH_RIGID_CONTACT): */
    SPH_F_RIGID_CONTACT_DN = 33,   /* f32[n][3] sum of depth * n over the target's contacts in the last contact pass */
    SPH_F_RIGID_CONTACT_COUNT = 34,/* f32[n]    the number of those contacts (partner particles + wall planes) */
    /* PCISPH only: the non-pressure acceleration the last SPH_PH_NON_PRESSURE stored (PCISPH.py:22 keeps it in particle_accelerations
       until the refine loop is over; this library keeps it in a buffer of its own, SPH_F_ACCELERATION is the pressure pass's): */
    SPH_F_NON_PRESSURE_ACCEL = 35, /* f32[n][3] gravity + surface tension + viscosity (base_solver.py:190), download only */
    /* implicit viscosity (viscosity_implicit handles only), download only: the vectors of the CG solve (base_solver.py:282-517) as the
       last launch left them.  Written on fluid rows only: any other row keeps what it held (zero, or a former occupant's value). */
    SPH_F_CG_B = 36,               /* f32[n][3] cg_b (:310) */
    SPH_F_CG_R = 37,               /* f32[n][3] cg_r */
    SPH_F_CG_P = 38,               /* f32[n][3] cg_p, the search direction of the running iteration */
    SPH_F_CG_AP = 39,              /* f32[n][3] cg_Ap.  NOT written by an A p walk that leaves its three parts only (the split walk inside the
                                      unsharded loop, SPH_F_CG_AP_PARTS): it then still holds the last combined A p */
    SPH_F_CG_V0 = 40,              /* f32[n][3] original_velocity (:298) */
    SPH_F_CG_DINV = 41,            /* f32[n][9] cg_diagnol_ii_inv, row-major (:303-308) */
    SPH_F_CG_AP_PARTS = 42,        /* f32[3][n][3] the per-x-offset-group parts of sum_j D_i^-1 (-A_ij) p_j of the last SPLIT A p walk, before
                                      dt / rho0 and + p_i: A p = ((part_0 + part_1) + part_2) dt / rho0 + p */
    /* Akinci surface tension (allocated when sph_set_surface_tension first switches the mode on), download only: the colour-field
       normals n_i = h sum_j (m_j / rho_j) gradW_ij the last SPH_PH_SURFACE_NORMALS (or step) stored.  Written on fluid rows only.  Not
       carried through the sort (recomputed every step): valid until the next sort, like SPH_F_NON_PRESSURE_ACCEL of a handle that is
       not PCISPH's (DFSPH sorts in the second half of its step: read both between sph_step_begin and sph_step_end). */
    SPH_F_SURFACE_NORMAL = 43,     /* f32[n][3] */
    /* Micropolar vorticity model (allocated when sph_set_micropolar first switches the mode on; SPH_ERR_UNSUPPORTED before).  The angular
       velocity belongs to the particle and follows it through every sort: download and upload in the CURRENT order, like every other field;
       particles appended later start at zero; rows that are not fluid read zero and an upload leaves them alone.  An axial vector:
       its sign follows the parity of the handle's axis order, as the rigid bodies' angular velocity does. */
    SPH_F_ANGULAR_VELOCITY = 44,   /* f32[n][3] */
    /* download only: a_mp of the last SPH_PH_MICROPOLAR (or step), written on active fluid rows only; valid until the next sort */
    SPH_F_MICROPOLAR_ACCEL = 45,   /* f32[n][3] */
    /* Elastic solids (allocated when sph_set_elastic_object first marks an object; SPH_ERR_UNSUPPORTED before).  All four in the CURRENT
       order like every field; rows that do not belong to a captured elastic object read zero.  The first three are download only: a_el of
       the last SPH_PH_ELASTIC (or step), valid until the next sort; the deformation gradient F (row-major) and the stress
       (xx, xy, xz, yy, yz, zz) that pass stored.  The rotation is the unit quaternion (x, y, z, w) the next pass warm-starts from:
       up- and downloadable (an upload leaves rows outside captured elastic objects alone). */
    SPH_F_ELASTIC_ACCEL = 46,      /* f32[n][3] */
    SPH_F_ELASTIC_DEFGRAD = 47,    /* f32[n][9] */
    SPH_F_ELASTIC_STRESS = 48,     /* f32[n][6] */
    SPH_F_ELASTIC_ROTATION = 49,   /* f32[n][4] */
    /* Air drag (allocated when sph_set_drag first switches the mode on; SPH_ERR_UNSUPPORTED before).  Download only, in the CURRENT
       order: what the last SPH_PH_DRAG (or step) stored, written on active fluid rows only; valid until the next sort. */
    SPH_F_DRAG_ACCEL = 50,         /* f32[n][3]: a_drag */
    SPH_F_DRAG_TERMS = 51,         /* f32[n][5]: n_i, w, C_D, A_un, y */
    /* Heat (allocated when sph_set_thermal first switches the mode on; SPH_ERR_UNSUPPORTED before).  The temperature belongs to the
       particle and follows it through every sort: download and upload in the CURRENT order, like every other field.  A row that is not
       fluid reads the temperature its object is held at (the reference temperature where it has none); an upload writes fluid rows only. */
    SPH_F_TEMPERATURE = 52,        /* f32[n] */
    /* download only: dT/dt of the last SPH_PH_HEAT (or step), written on active fluid rows only; valid until the next sort */
    SPH_F_TEMPERATURE_RATE = 53,   /* f32[n] */
    SPH_F_COUNT_
} SphField;

/* Individually callable phases (tests, profiling).  sph_step() runs them in the order of the
   reference's _step() (WCSPH.py:27, DFSPH.py:298, PCISPH.py:165) followed by step() :692. */
typedef enum {
    SPH_PH_NEIGHBOR_SEARCH = 0,  /* base_container.py:544 prepare_neighborhood_search */
    SPH_PH_RIGID_VOLUME = 1,     /* base_solver.py:106 */
    SPH_PH_DENSITY = 2,          /* :522 (+ WCSPH.py:17 EOS when method == wcsph) */
    SPH_PH_NON_PRESSURE = 3,     /* :190 + :643 (gravity, surface tension, viscosity, v += dt a) */
    SPH_PH_PRESSURE_INTEGRATE = 4, /* :136 + :643 + :652 + :575 */
    SPH_PH_DFSPH_ALPHA = 5,      /* DFSPH.py:23 */
    SPH_PH_DFSPH_DIVERGENCE = 6, /* DFSPH.py:139 */
    SPH_PH_DFSPH_DENSITY = 7,    /* DFSPH.py:225 */
    SPH_PH_IISPH_PREPARE = 8,    /* IISPH.py:93 init_step + :18 compute_dii + :47 compute_aii + :71 compute_density_star */
    SPH_PH_IISPH_ITERATION = 9,  /* one iteration of IISPH.py:185 refine: compute_dij_pj, compute_sum_i, update_pressure (+ error) */
    SPH_PH_PBF_DENSITY_LAMBDA = 10, /* PBF.py:64-65 compute_density + compute_lambda on the current positions and the last sort's cells */
    SPH_PH_PBF_FIX_POSITION = 11,   /* PBF.py:66 fix_position (Jacobi) on the same */
    SPH_PH_PBF_PREDICT = 12,        /* PBF.py:150-154 save_old_position + update_fluid_position + enforce_domain_boundary */
    SPH_PH_PBF_FINISH = 13,         /* PBF.py:156-158 enforce_domain_boundary + recompute_fluid_velocity */
    SPH_PH_RIGID_CONTACT = 14,      /* the rigid contact pass (sph_set_rigid_contact) on the current positions and the last sort's cells;
                                       the per-particle contact fields are zeroed first; the table accumulates as in a step */
    /* consistent PBF variant (sph_set_pbf_variant), on the masks and cell lists of the last sort: */
    SPH_PH_PBFC_PREDICT = 15,        /* x* = x + dt v + boundary (SPH_F_PREDICTED_POS); SPH_F_POSITION stays */
    SPH_PH_PBFC_DENSITY_LAMBDA = 16, /* walk A: rho, lambda at x*; SphPbfStats::error = mean C of this walk, iterations = 1 */
    SPH_PH_PBFC_DELTA = 17,          /* walk B: the Jacobi correction of x* */
    SPH_PH_PBFC_FINISH = 18,         /* x = boundary(x*), v = (x - x_old) / dt, emitter branch */
    /* PCISPH, the passes of the step one by one (after SPH_PH_NON_PRESSURE, on the cell lists of the last sort): */
    SPH_PH_PCISPH_INIT = 19,           /* PCISPH.py:154 init_step: p = 0, predicted velocity and position without a pressure term */
    SPH_PH_PCISPH_RHO_STAR = 20,       /* first walk of an iteration of PCISPH.py:110 refine: :33 compute_density_star + :66 update_pressure;
                                          SphStats::err_pcisph = density_error of this walk, iter_pcisph = 1 */
    SPH_PH_PCISPH_PRESSURE_ACCEL = 21, /* second walk: :75 compute_temp_pressure_acceleration + :19, :26 predicted velocity and position */
    SPH_PH_DFSPH_ALPHA_DIVERGENCE = 22, /* the end of a DFSPH step behind the sort and the rigid volumes, as the step runs it: density + alpha + the
                                           first D rho / Dt in ONE walk (DFSPH.py:317-318, :140), then the loop of :139.  The fast build's fused walk
                                           evaluates that first D rho / Dt in another order than the pass SPH_PH_DFSPH_DIVERGENCE starts with */
    /* Implicit viscosity (viscosity_implicit handles of any method, unsharded), the launches of the CG solve inside SPH_PH_NON_PRESSURE one
       pass each, with no stop test.  SPH_PH_CG_PREPARE, k x (AP, UPDATE_XR, UPDATE_P), SPH_PH_CG_END is SPH_PH_NON_PRESSURE with
       fixed_iterations = k, bit for bit. */
    SPH_PH_CG_PREPARE = 23,    /* base_solver.py:510-512: prepare_conjugate_gradient_solver1, the first compute_Ap, prepare_..._solver2, |r0|^2 */
    SPH_PH_CG_AP = 24,         /* :374 compute_Ap as the loop's next A p pass runs it: from the second one on it also applies the p update of
                                  the iteration before, where the step folds that update into it (every unsharded solve) */
    SPH_PH_CG_UPDATE_XR = 25,  /* :394 alpha, :409 update_cg_x, :415 update_cg_r_and_beta (the sums) */
    SPH_PH_CG_UPDATE_P = 26,   /* :427-437 beta, error, update_p.  Where the step folds the p update into the next A p pass this phase launches
                                  NOTHING and returns SPH_OK: cg_p, beta and the error change only with the next SPH_PH_CG_AP */
    SPH_PH_CG_END = 27,        /* :514-517: the viscous acceleration from the solved velocities + gravity + surface tension, v += dt a on the
                                  original velocities, the reaction on dynamic bodies, prepare_guess */
    /* Akinci surface tension (sph_set_surface_tension; SPH_ERR_INVALID while the mode is off): the normal pass alone, on the masks of
       the last sort.  In this mode SPH_PH_NON_PRESSURE (and SPH_PH_CG_END) run the Akinci pass on the STORED normals, without
       recomputing them; a step computes them in front of its non-pressure pass. */
    SPH_PH_SURFACE_NORMALS = 28,
    /* Micropolar vorticity model (sph_set_micropolar; SPH_ERR_INVALID while the mode is off): the walk alone, on the masks of the last
       sort: it stores a_mp (SPH_F_MICROPOLAR_ACCEL) and the new angular velocities and adds the reaction on dynamic bodies.  In this
       mode SPH_PH_NON_PRESSURE (and SPH_PH_CG_END) add the STORED a_mp behind their pass, v += dt a_mp, without walking again; a
       step walks in front of its non-pressure pass. */
    SPH_PH_MICROPOLAR = 29,
    /* Elastic solids (sph_set_elastic_object; SPH_ERR_INVALID while no object is marked): the scatter and the passes A and B alone, on
       the order of the last sort: they store a_el (SPH_F_ELASTIC_ACCEL), F, the stress and the new rotations.  SPH_PH_NON_PRESSURE
       (and SPH_PH_CG_END) then add the STORED a_el behind their pass, v += dt a_el; a step runs the passes in front of its
       non-pressure pass. */
    SPH_PH_ELASTIC = 30,
    /* Fluid emitters (sph_set_emitter; SPH_ERR_INVALID while none is set): the hold and the emission of the CURRENT step count alone --
       what sph_prepare's emission did for count 0 -- i.e. the held layers are put on their closed form at T_steps and the layers
       born(steps) not emitted yet are emitted.  Idempotent: a second run emits nothing. */
    SPH_PH_EMIT = 31,
    /* Air drag (sph_set_drag; SPH_ERR_INVALID while the mode is off): the walk alone, on the masks of the last sort: it stores a_drag
       (SPH_F_DRAG_ACCEL) and its terms (SPH_F_DRAG_TERMS) and nothing else.  In this mode SPH_PH_NON_PRESSURE (and SPH_PH_CG_END) add
       the STORED a_drag behind their pass, v += dt a_drag, without walking again; a step walks in front of its non-pressure pass. */
    SPH_PH_DRAG = 32,
    /* Outflow (sph_set_outflow; SPH_ERR_INVALID while no volume is set): the mark and the count of the CURRENT step count alone -- every
       active fluid particle inside a volume whose time window holds T_steps gets its dead bit, the per-volume counters are read back.  No
       sort: the particle count shrinks in the next SPH_PH_NEIGHBOR_SEARCH (or step). */
    SPH_PH_OUTFLOW = 33,
    /* Adaptive time stepping (sph_set_cfl; SPH_ERR_INVALID while the mode is off): the reduce alone -- the maximum of |v|^2 over the
       particles that count is read back into SphTimeState::vmax2; the step size does not change.  A non-finite square:
       SPH_ERR_INVALID ("non-finite velocity"). */
    SPH_PH_CFL = 34,
    /* Heat (sph_set_thermal; SPH_ERR_INVALID while the mode is off): the gather and the walk alone, on the masks of the last sort: they
       store the new temperatures (SPH_F_TEMPERATURE) and dT/dt (SPH_F_TEMPERATURE_RATE) and nothing else.  In this mode, with
       beta != 0, SPH_PH_NON_PRESSURE (and SPH_PH_CG_END) add the buoyancy of the GATHERED temperatures -- those the last walk read --
       behind their pass, v += dt a_b, without walking again; a step walks in front of its non-pressure pass. */
    SPH_PH_HEAT = 35,
    SPH_PH_COUNT_
} SphPhase;

typedef struct {
    int64_t steps;               /* steps executed since create */
    int64_t pair_interactions;   /* accepted (i fluid, j != i, |x_ij| < dh) pairs summed over the
                                    neighbour passes of the LAST step (SURVEY 8d metric) */
    int32_t particle_num;
    int32_t fluid_particle_num;
    int32_t iter_divergence, iter_density, iter_pcisph, iter_cg; /* last step */
    float   err_divergence, err_density, err_pcisph, err_cg;
    int64_t lds_fallback_blocks; /* neighbour-pass workgroups that overflowed the LDS tile (last step) */
    double  total_time;          /* container.total_time, base_solver.py:694 */
    int64_t pair_evaluations;    /* the same accepted pairs counted once per neighbour walk the library actually makes
                                    (a fused kernel that does the work of k reference passes adds k to
                                    pair_interactions and 1 here), last step */
    int64_t hash_launches;       /* launches of the cell-id / histogram kernel (init_grid, base_container.py:496) since create */
    int64_t prehashed_sorts;     /* sorts since create whose init_grid was done by the force pass of the step before (inside one
                                    sph_step_async(n) call of an unsharded all-fluid WCSPH scene): hash_launches + prehashed_sorts
                                    = sorts.  Lets a test assert which path a timed region really took. */
    int64_t list_sorts;          /* deterministic sorts since create that ranked the particles from per-cell run lists filed by whoever
                                    hashed them (reorder_particles, base_container.py:506-515, in two launches: rank + gather with the
                                    per-tile preparation of the neighbour passes fused in) instead of run records filed after the scan */
    int64_t carried_sorts;       /* list sorts since create whose gather left velocity + mass, meta word and particle id to the density
                                    pass launched behind it (all-fluid unsharded WCSPH / PCISPH / IISPH steps; SPH_NO_SORT_CARRY=1: 0) */
    int32_t iter_iisph;          /* IISPH.py:185 refine: iterations of the last step (last SPH_PH_IISPH_ITERATION phase: 1) */
    float   err_iisph;           /* its density_error (IISPH.py:118-121; 0 with fixed_iterations > 0, as err_* of the others) */
    int64_t pbf_recentred;       /* PBF: refine walks of the last step (or phase) whose particle's current cell differed from its sorted cell
                                    (base_container.py:550: the 27 cells around the current cell, not the sorted one) */
} SphStats;

/* Kernel ids for the HIP-event profiler (sph_profile_*). */
typedef enum {
    SPH_K_HASH_COUNT = 0, SPH_K_SCAN = 1, SPH_K_SCATTER = 2, SPH_K_DENSITY = 3,
    SPH_K_NON_PRESSURE = 4, SPH_K_PRESSURE_INTEGRATE = 5, SPH_K_RIGID_VOLUME = 6,
    SPH_K_DFSPH_DENSITY_ALPHA = 7, SPH_K_DFSPH_RHO_ADV = 8, SPH_K_DFSPH_CORRECT = 9,
    SPH_K_REDUCE = 10, SPH_K_PCISPH_RHO_STAR = 11, SPH_K_PCISPH_PRESSURE_ACCEL = 12,
    SPH_K_CG_PREPARE = 13, SPH_K_CG_AP = 14, SPH_K_CG_VECTOR = 15, SPH_K_MISC = 16,
    SPH_K_HALO = 17, SPH_K_WCSPH_FORCES = 18,
    SPH_K_IISPH_PREPARE = 19, SPH_K_IISPH_DIJ_PJ = 20, SPH_K_IISPH_SUM_I = 21,
    SPH_K_PBF_DENSITY_LAMBDA = 22, SPH_K_PBF_FIX_POSITION = 23, SPH_K_PBF_UPDATE = 24,
    SPH_K_RIGID_CONTACT = 25, SPH_K_RIGID_INTEGRATE = 26, SPH_K_RIGID_CONTACT_SOLVE = 27,
    SPH_K_PBFC_DENSITY_LAMBDA = 28, SPH_K_PBFC_DELTA = 29,   /* consistent PBF: walk A, walk B (predict / finish: SPH_K_PBF_UPDATE) */
    SPH_K_RIGID_MOTION = 30,   /* scripted rigid bodies: the launch that evaluates their motion programs (sph_set_rigid_motion);
                                  sph_kernel_name's table ends at 29 and answers "?" for this id */
    SPH_K_SURFACE_NORMALS = 31, /* Akinci surface tension: the normal pass (the Akinci force pass itself is SPH_K_NON_PRESSURE); "?" as well */
    SPH_K_MICROPOLAR = 32,      /* micropolar vorticity model: the gather of the angular velocities + the walk (v += dt a_mp: SPH_K_MISC); "?" as well */
    SPH_K_ELASTIC = 33,         /* elastic solids: the scatter + pass A + pass B (v += dt a_el: SPH_K_MISC; the capture: SPH_K_MISC); "?" as well */
    SPH_K_EMIT = 34,            /* fluid emitters: the hold launch and the emit launch (sph_set_emitter); "?" as well */
    SPH_K_DRAG = 35,            /* air drag: the walk (v += dt a_drag: SPH_K_MISC); "?" as well */
    SPH_K_OUTFLOW = 36,         /* outflow: the mark launch (by volume, or by id for sph_remove_particles); "?" as well */
    SPH_K_CFL = 37,             /* adaptive time stepping: the reduce of the largest speed (sph_set_cfl); "?" as well */
    SPH_K_HEAT = 38,            /* heat: the gather of the temperatures + the walk (v += dt a_b and the fills: SPH_K_MISC); "?" as well */
    SPH_K_COUNT_
} SphKernelId;

/* --- lifetime -------------------------------------------------------------------------- */
/* replaces XContainer.__init__ allocation (base_container.py:129-185) + XSolver.__init__.
   particle_max_num <= 268,435,455 per handle (SPH_ERR_CAPACITY beyond: shard the scene over GPUs) */
int sph_create(const SphParams *params, SphHandle **out);
void sph_destroy(SphHandle *h);
/* message of the last failure on this handle (h == NULL: last failure of sph_create) */
const char *sph_last_error(SphHandle *h);

/* --- scene upload ---------------------------------------------------------------------- */
/* replaces BaseContainer._add_particles (base_container.py:441): append n particles of one object.
   pos/vel: f32[n][3]; density/pressure: f32[n]; material/is_dynamic: i32[n]; color: i32[n][3]. */
int sph_append_particles(SphHandle *h, int object_id, int n, const float *pos, const float *vel,
                         const float *density, const float *pressure, const int32_t *material,
                         const int32_t *is_dynamic, const int32_t *color);
/* persistent ids (SPH_F_PARTICLE_ID) of the n particles appended last; default = insertion index on this handle.  A rank
   of a sharded scene passes global insertion indices. */
int sph_set_appended_ids(SphHandle *h, int n, const int32_t *ids);
/* object_materials / rigid_body_is_dynamic (base_container.py:150,156; insert_object :237,:317,:332).  On a sharded scene
   (sph_comm_set_slab) EVERY rank registers every object, whether or not it holds any of its particles: the halo records of a
   scene with a dynamic rigid body carry the rest positions (64 instead of 48 bytes); sph_prepare agrees on that over all ranks,
   and a later mismatch fails the exchange on both sides (record size in the message header). */
int sph_set_object(SphHandle *h, int object_id, int material, int is_dynamic);
/* pose written by the host rigid solver (SPH/rigid_solver/bullet_solver.py:158-167); rot9 row-major.  Like the reference's
   rigid_body_* fields it is only READ at the renew_rigid_particle_state point of a step (inside sph_step_end / the second half of
   sph_step), wherever before that it was written: a pose pushed between two steps moves the particles after the fluid passes of
   the next step, not before them (base_solver.py:616, WCSPH.py:43). */
int sph_set_rigid_pose(SphHandle *h, int object_id, const float *com, const float *rot9,
                       const float *vel, const float *angvel, const float *com0);
/* rigid_body_forces / rigid_body_torques read by bullet_solver.py:150-156; reset != 0 zeroes them.  On a sharded scene
   (sph_comm_set_slab) this is a collective: every rank calls it at the same point of the step and gets the sum over the ranks. */
int sph_get_rigid_wrench(SphHandle *h, float *force, float *torque, int reset);

/* Rigid contact (opt-in; the host's "contact" rigid backend).  Once per step, right after the method's passes of the first half
   (where sph_get_rigid_wrench is read; rigid particles have not moved since the last sort), a pass walks the 27 cells around every
   particle of a DYNAMIC rigid object and accepts every rigid particle j of ANOTHER object (dynamic, static, the domain box; ghosts
   included, fluid skipped) with 1e-6 < |x_i - x_j| < distance.  Without a domain box the six planes wall_lo / wall_hi are partners too:
   a particle touches a plane when it is closer than distance / 2 (depth = distance / 2 - its signed distance, contact point = its
   projection onto the plane).  Per pair: n = (x_i - x_j) / |x_i - x_j|, depth = distance - |x_i - x_j|, bin = 2 * (dominant axis of n,
   first of equal ones) + (that component < 0).  The pass files every pair under the key (A = i's object, B, bin), B = j's object id,
   or 20 + bin for the domain box (object id -1) and the wall planes.  Per key the table holds
     [0] pairs  [1..3] sum of the midpoints (x_i + x_j) / 2  [4..6] sum of depth * n  [7] maximum depth
   accumulated as 64-bit fixed point (2^-32 per unit): bit-reproducible, and summed until read with reset != 0.
   sph_set_rigid_contact: distance <= the grid cell size; wall_lo / wall_hi (3-vectors, scene frame) both null in a scene with a domain
   box.  on = 0 turns the pass off.  SPH_ERR_UNSUPPORTED on a PBF handle (PBF moves no rigid body).
   sph_get_rigid_contacts: table = double[SPH_MAX_OBJECTS][SPH_CONTACT_PARTNERS][SPH_CONTACT_BINS][SPH_CONTACT_VALUES] in the scene frame
   (bins and vectors mapped back under SPH_SLAB_LAYOUT=slow).  On a sharded scene a collective like sph_get_rigid_wrench: every rank
   walks its own targets (ghosts are partners) and gets the sum over the ranks (maximum for [7]). */
#define SPH_CONTACT_PARTNERS 26
#define SPH_CONTACT_BINS 6
#define SPH_CONTACT_VALUES 8
int sph_set_rigid_contact(SphHandle *h, int on, float distance, const float *wall_lo, const float *wall_hi);
int sph_get_rigid_contacts(SphHandle *h, double *table, int reset);
/* accepted contacts (partner particles + wall planes) of the last contact pass on this handle (this rank's targets).  A query of its
   own rather than a SphStats field: the statistics struct ends at pbf_recentred by contract. */
int sph_get_rigid_contact_pairs(SphHandle *h, int64_t *pairs);

/* PBF variant.  variant 0 = reference (PBF.py as written, the default), 1 = consistent.  For the consistent variant:
   the solve runs at least min_iterations (>= 1) and at most max_iterations (>= min_iterations) iterations and stops after the first
   one whose mean constraint error sum_i C_i / fluid_particle_num is <= max_error (> 0, finite); epsilon (> 0, finite) is the
   relaxation term of lambda's denominator.  SphParams::fixed_iterations > 0 runs exactly that many and reports error 0.
   Legal between sph_create and sph_prepare only.  SPH_ERR_UNSUPPORTED: not a PBF handle.  SPH_ERR_INVALID: after sph_prepare, or a
   bad field (the message names it).  sph_step_async on a consistent handle needs fixed_iterations > 0: the stop test reads back. */
typedef struct { int32_t variant, min_iterations, max_iterations; float max_error, epsilon; } SphPbfParams;
#define SPH_PBF_VARIANT_REFERENCE 0
#define SPH_PBF_VARIANT_CONSISTENT 1
int sph_set_pbf_variant(SphHandle *h, const SphPbfParams *params);
/* the variant of a PBF handle, the iterations of its last step's solve and that solve's last mean constraint error (reference variant:
   its fixed 5, and 0).  A query of its own: the statistics struct ends at pbf_recentred by contract. */
typedef struct { int32_t variant, iterations; float error; } SphPbfStats;
int sph_get_pbf_stats(SphHandle *h, SphPbfStats *out);

/* Surface tension model (opt-in).  method 0 = reference (the reference's pairwise -sigma m_j / m_i R W(r) with
   SphParams::surface_tension, the default), 1 = akinci: Akinci, Akinci, Teschner 2013.  With h the support radius, W the cubic spline,
   rho the density the viscous term of the method reads, j fluid and k boundary neighbours of an active fluid particle i:
     n_i = h sum_j (m_j / rho_j) gradW_ij,   K_ij = 2 rho0 / (rho_i + rho_j),   Psi_k = rho0 V_k
     a_i = -gamma sum_j K_ij (m_j C(r) (x_i - x_j) / r + n_i - n_j)  -  beta sum_k Psi_k A(r) (x_i - x_k) / r
     C(r) = 32 / (pi h^9) { (h-r)^3 r^3 : h/2 < r <= h;  2 (h-r)^3 r^3 - h^6 / 64 : 0 < r <= h/2 },
     A(r) = 0.007 / h^3.25 (-4 r^2 / h + 6 r - 2 h)^(1/4) : h/2 < r <= h   (radicand clamped at 0)
   in the place of the reference's term; gravity, viscosity and v += dt a stay.  A dynamic rigid neighbour k receives
   +m_i beta Psi_k A(r) (x_i - x_k) / r at x_k.  WCSPH takes its unfused route in this mode (density, normals, non-pressure,
   pressure: SPH_K_WCSPH_FORCES does not run).  Legal at any time between steps; switching back to 0 restores the reference path
   bit for bit.  gamma, beta are kept while the method is 0.
   SPH_ERR_UNSUPPORTED: a PBF handle (either variant), a sharded handle (and sph_comm_set_slab while the mode is on).  This library
   has no 2-D handles; the Python front end refuses 2-D scenes.  SPH_ERR_INVALID: gamma or beta negative or not finite, an unknown method.
   sph_surface_tension_kernels_host: C(r) and A(r) of the kernels' source on the CPU, strict (fast = 0) or fast form.  No device. */
#define SPH_SURFACE_TENSION_REFERENCE 0
#define SPH_SURFACE_TENSION_AKINCI 1
typedef struct { int32_t method; double gamma, beta; } SphSurfaceTensionParams;
int sph_set_surface_tension(SphHandle *h, const SphSurfaceTensionParams *params);
int sph_get_surface_tension(SphHandle *h, SphSurfaceTensionParams *out);
int sph_surface_tension_kernels_host(double h, const float *r, int64_t n, float *C_out, float *A_out, int fast);

/* Micropolar vorticity model (opt-in).  method 0 = none (the default), 1 = micropolar: Bender, Koschier, Kugelstadt,
   Weiler 2017.  Every fluid particle carries an angular velocity w (SPH_F_ANGULAR_VELOCITY, zero when inserted).  With R = x_i - x,
   gradW = gradW(R), W the cubic spline, rho the density the viscous term of the method reads, j fluid and k boundary neighbours of an
   active fluid particle i, Psi_k = rho0 V_k:
     a_mp_i  = nu_t / rho_i [ sum_j m_j (w_i - w_j) x gradW_ij + sum_k Psi_k w_i x gradW_ik ]
     alpha_i = theta_inv { nu_t / rho_i [ sum_j m_j (v_i - v_j) x gradW_ij + sum_k Psi_k (v_i - v_k) x gradW_ik ]
                           - 2 nu_t w_i - zeta sum_j (m_j / rho_j) (w_i - w_j) W_ij }
     v_i <- v_i + dt (a_np_i + a_mp_i),   w_i <- w_i + dt alpha_i
   All sums read the state at the start of the non-pressure phase (the w update is Jacobi).  A dynamic rigid neighbour k receives
   -m_i nu_t / rho_i Psi_k w_i x gradW_ik at x_k.  a_mp also enters the non-pressure acceleration, which every method keeps in this
   mode (SPH_F_NON_PRESSURE_ACCEL).  WCSPH takes its unfused route (SPH_K_WCSPH_FORCES does not run).  Legal at any time between
   steps; switching back to 0 restores the plain path bit for bit and keeps w and the three values.
   The angular velocities are stored by persistent particle id, which has to be the append order: while the mode is on
   sph_set_appended_ids and an upload of SPH_F_PARTICLE_ID are refused with SPH_ERR_UNSUPPORTED, and so is the mode once either has
   been used.  SPH_ERR_UNSUPPORTED too: a PBF handle (either variant), a sharded handle (and sph_comm_set_slab while the mode is on).
   This library has no 2-D handles; the Python front end refuses 2-D scenes.  SPH_ERR_INVALID: nu_t, zeta or theta_inv negative or
   not finite, an unknown method.
   sph_micropolar_pair_host: the kernels' pair arithmetic on the CPU, strict (fast = 0) or fast form.  in: n records of 24 floats
   (v_i[3], w_i[3], nu_t / rho_i, m_j, v_j[3], w_j[3], m_j / rho_j, zeta, R[3], gs, gradW[3], W; gradW = gs R: the fast form reads gs and
   R, the strict form gradW); out: n records of 6 floats, the pair's share of the two sums (sph_micropolar.hpp MpSums).  No device. */
#define SPH_VORTICITY_NONE 0
#define SPH_VORTICITY_MICROPOLAR 1
typedef struct { int32_t method; double nu_t, zeta, theta_inv; } SphMicropolarParams;
int sph_set_micropolar(SphHandle *h, const SphMicropolarParams *params);
int sph_get_micropolar(SphHandle *h, SphMicropolarParams *out);
int sph_micropolar_pair_host(const float *in, int64_t n, float *out, int fast);

/* Elastic solids (opt-in, per fluid object): corotated linear SPH elasticity on a kernel-corrected rest configuration
   (Becker, Ihmsen, Teschner 2009; the rotation extraction of Mueller et al. 2016).  The object's particles stay fluid: every other pass
   treats them as before, and one more acceleration is added where a_mp is.  With x0 the positions at capture, x0_ji = x0_j - x0_i,
   gradW0_ij = gradW(x0_i - x0_j), V0 the rest volume, N0_i the particles j != i of the SAME object that the step's neighbour test
   accepts at capture (symmetric bit for bit):
     capture:  M_i = sum_{j in N0_i} V0 x0_ji (x) gradW0_ij;  g0_ij = M_i^-1 gradW0_ij (float64, rounded to f32);  q_i = identity
     step:     F_i = sum_j V0 (x_j - x_i) (x) g0_ij;  R_i = rotation of F_i (10 warm-started iterations on q_i, which is stored)
               eps_i = 1/2 (F_i R_i^T + R_i F_i^T) - I;  sig_i = 2 mu eps_i + lambda tr(eps_i) I
               a_el_i = (V0^2 / m_i) sum_j (sig_i R_i g0_ij - sig_j R_j g0_ji);  v_i <- v_i + dt (a_np_i + a_mp_i + a_el_i)
     mu = E / (2 (1 + nu)), lambda = E nu / ((1 + nu)(1 - 2 nu)).  All sums read the positions at the start of the non-pressure phase.
   sph_set_elastic_object marks the object; the NEXT neighbour search that holds particles of it captures it (sph_prepare, or the first
   step after a late entry) and that call returns the capture's error: SPH_ERR_CAPACITY when a list would exceed
   SPH_ELASTIC_MAX_NEIGHBOURS entries (no list is ever truncated), SPH_ERR_INVALID when a particle is degenerate (the smallest
   eigenvalue of M below 1e-3 of the largest: a sheet, fewer than three non-coplanar neighbours; the message names the object and the
   count), SPH_ERR_UNSUPPORTED when the object's ids are not one contiguous append range.  A refused object stays plain fluid.  Marking
   a captured object again changes its parameters only.  a_el also enters the non-pressure acceleration where a method keeps one.
   WCSPH takes its unfused route while an object is marked.  The lists are stored by persistent particle id, which has to be the
   append order: while an object is marked sph_set_appended_ids and an upload of SPH_F_PARTICLE_ID are refused with
   SPH_ERR_UNSUPPORTED, and so is marking once either has been used.  SPH_ERR_UNSUPPORTED too: a PBF handle, a sharded handle (and
   sph_comm_set_slab while an object is marked), particles appended to an object after its capture (sph_append_particles).
   SPH_ERR_INVALID: E <= 0 or not finite, nu outside [0, 0.49], an object that is unknown or not fluid.
   sph_get_elastic_rest: the captured lists, row r = particle id first_id + r: nbr int32[count][SPH_ELASTIC_MAX_NEIGHBOURS] (ascending
   ids, -1 behind the end), g0_ij and g0_ji f32[count][SPH_ELASTIC_MAX_NEIGHBOURS][3] in the scene's frame (zero behind the end).
   sph_elastic_particle_host: passes A and B of ONE particle from the kernels' own source on the CPU, strict (fast = 0) or fast form,
   no device.  nnb list entries: xj[nnb][3], g0_ij[nnb][3], g0_ji[nnb][3], the neighbours' pass-A results q_j[nnb][4] and
   sigma_j[nnb][6]; xi[3], the warm start q_prev[4]; out: F[9], q[4], sigma[6] (pass A) and a_el[3] (pass B on them). */
#define SPH_ELASTIC_MAX_NEIGHBOURS 64
typedef struct { double youngs_modulus, poisson_ratio; } SphElasticParams;
typedef struct {
    int32_t captured;        /* 0: not marked, 1: marked and waiting for its capture, 2: captured, 3: refused at capture */
    int32_t count, first_id; /* particles of the object and the first of their ids (captured objects) */
    int32_t longest_list;
    float min_eig_ratio;     /* smallest eigenvalue ratio of M over the object's particles */
    SphElasticParams params;
} SphElasticObjectInfo;
int sph_set_elastic_object(SphHandle *h, int object_id, const SphElasticParams *params);
int sph_get_elastic_object(SphHandle *h, int object_id, SphElasticObjectInfo *out);
int sph_get_elastic_rest(SphHandle *h, int object_id, int32_t *nbr, float *g0_ij, float *g0_ji);
int sph_elastic_particle_host(int nnb, const float *xi, const float *xj, const float *g0_ij, const float *g0_ji, const float *q_prev,
                              const float *q_j, const float *sigma_j, double V0, double mass, double mu, double lambda, float *F_out,
                              float *q_out, float *sigma_out, float *a_out, int fast);

/* Air drag and wind (opt-in).  method 0 = none (the default), 1 = gissler: Gissler, Band, Peer, Ihmsen, Teschner 2017,
   "Approximate air-fluid interactions for SPH".  The air is not simulated: a constant wind u (air_velocity) of density rho_air acts
   on every active fluid particle; nothing receives a reaction, momentum is not conserved, by design.
   Constants (water in air): sigma = 0.0724, mu_l = 0.00102, mu_a = 1.845e-5, C_F = 1/3, C_k = 8, C_d = 5, C_b = 0.5, n_full = 38.
   Per handle, once on the host in double, d = 2 r the particle diameter, rho_l = density_0:
     L       = cbrt(3 / (4 pi)) d
     1/t_d   = C_d mu_l / (2 rho_l L^2)
     omega^2 = C_k sigma / (rho_l L^3) - 1/t_d^2          (refused if <= 0)
     t_max   = -2 (atan(sqrt(t_d^2 omega^2)) - pi) / omega
     c_def   = 1 - exp(-t_max / t_d) (cos(omega t_max) + sin(omega t_max) / (omega t_d))
     y_coeff = C_F (rho_air L / sigma) c_def / (C_k C_b)
     n23     = 2 n_full / 3
   Per active fluid particle i with velocity v_i at the start of the non-pressure phase and mass m_i; j ranges over its fluid
   neighbours (material fluid, any object, r_ij < h, self excluded: the pairs every other walk accepts); rigid and boundary particles
   neither count nor shield:
     v_rel = u - v_i ;  s2 = |v_rel|^2 ;  if s2 < 1e-6: a_drag_i = 0, all terms 0, done
     s = sqrt(s2) ;  e = v_rel / s
     y     = min(s2 y_coeff, 1)
     Re    = 2 max(rho_air s L / mu_a, 0.1)
     C_sph = Re <= 1000 ? 24 / Re (1 + Re^(2/3) / 6) : 0.424
     C_liu = C_sph (1 + 2.632 y)
     n_i   = number of j ;  f = min(n23, n_i) / n23
     C_D   = (1 - f) C_liu + f                                  (n_i = 0: C_liu)
     A_drop = pi (L + C_b L y)^2 ;  A_un = (1 - f) A_drop + f d^2
     q     = max over j of  e . (x_i - x_j) / |x_i - x_j|       (0 when n_i = 0; never below 0)
     w     = clamp(1 - q, 0, 1)                                 (a w below 2^-20, the roundoff q carries, is stored as 0)
     a_drag_i = k (1 / (2 m_i)) rho_air s v_rel C_D w A_un
     v_i <- v_i + dt (a_np_i + ... + a_drag_i)
   a_drag also enters the non-pressure acceleration, which every method keeps in this mode (SPH_F_NON_PRESSURE_ACCEL).  WCSPH takes its
   unfused route (SPH_K_WCSPH_FORCES does not run).  Legal at any time between steps; switching back to 0 restores the plain path bit
   for bit and keeps the values.  SPH_ERR_UNSUPPORTED: a PBF handle (either variant), a sharded handle (and sph_comm_set_slab while
   the mode is on).  This library has no 2-D handles; the Python front end refuses 2-D scenes.  SPH_ERR_INVALID: an unknown method,
   k or rho_air negative or not finite, a wind component that is not finite, omega^2 <= 0 for the handle's radius and density.
   sph_drag_particle_host: everything behind the walk (drag_finish of csrc/sph_drag.hpp) from the kernels' own source on the CPU,
   strict (fast = 0) or fast form.  in: n records of 6 floats (v_i[3], m_i, n_i, q); out: n records of 7 floats (a_drag[3], w, C_D,
   A_un, y).  sph_drag_constants_host: the per-handle constants above, out[8] = L, 1/t_d, omega^2, t_max, c_def, y_coeff, n23,
   rho_air L / mu_a; SPH_ERR_INVALID (and only the first three filled) where omega^2 <= 0.  Neither touches a device. */
#define SPH_DRAG_NONE 0
#define SPH_DRAG_GISSLER 1
typedef struct { int32_t method; double k, rho_air, air_velocity[3]; } SphDragParams;
int sph_set_drag(SphHandle *h, const SphDragParams *params);
int sph_get_drag(SphHandle *h, SphDragParams *out);
int sph_drag_particle_host(const SphDragParams *params, double radius, double rho0, int64_t n, const float *in, float *out, int fast);
int sph_drag_constants_host(const SphDragParams *params, double radius, double rho0, double *out);

/* Heat: a temperature per fluid particle, conduction and Boussinesq buoyancy (opt-in).  method 0 = none (the default),
   1 = conduction: Cleary and Monaghan 1999 with constant conductivity.  With R = x_i - x, gradW = gradW(R),
   F = (R . gradW) / (|R|^2 + 0.01 h^2), j the fluid and k the boundary neighbours of an active fluid particle i (r < h, self excluded:
   the pairs every other walk accepts; domain box, static, scripted and dynamic bodies, held emitter particles), rho the density the
   method's viscous term reads (WCSPH: before the clamp of the equation of state), at the start of the non-pressure phase:
     dT_i/dt = 2 alpha (rho0 / rho_i) [ sum_j (m_j / rho_j) (T_i - T_j) F_ij + sum_k c_k (T_i - T_k) F_ik ]
               c_k = V_k (rest volume) where k's object has a temperature T_k (sph_set_object_temperature), else 0: adiabatic
     T_i <- T_i + dt dT_i/dt                  (Jacobi: every sum reads the T of the previous step)
     a_b_i = -beta (T_i - t_ref) g            (T_i: the previous step's);   v_i <- v_i + dt (a_np_i + ... + a_b_i)
   A body is never heated or cooled by the fluid, and nothing receives a reaction.  alpha in m^2 / s (0: T is only carried), beta in
   1 / K.  With beta == 0 nothing is added to v and WCSPH keeps its fused force pass (SPH_K_WCSPH_FORCES); with beta != 0 it takes its
   unfused route and a_b enters the non-pressure acceleration where one is kept.  The update is explicit: it stays a convex combination
   of neighbour temperatures while dt 2 alpha (rho0 / rho_i) sum c |F| <= 1; nothing here checks that.
   Temperatures are stored by particle id, which must be the append order: SPH_ERR_UNSUPPORTED after sph_set_appended_ids / an upload of
   SPH_F_PARTICLE_ID, and both are refused while the mode is on.  New particles (sph_append_particles, an emitter's layers) start at
   their object's temperature, or at t_ref where it has none; so does every particle present when the mode is first switched on.
   sph_set_thermal: legal at any time between steps; a null pointer or method 0 switches the mode off, restores the plain path bit for
   bit and keeps the temperatures.  SPH_ERR_UNSUPPORTED: a PBF handle (either variant), a sharded handle (and sph_comm_set_slab while
   the mode is on).  This library has no 2-D handles; the Python front end refuses 2-D scenes.  SPH_ERR_INVALID: an unknown method,
   alpha or beta negative or not finite, t_ref not finite.
   sph_set_object_temperature: object -1 (the domain box) .. SPH_MAX_OBJECTS - 1; has_T = 0 takes the temperature away.  Legal in either
   mode and before the object exists.  A fluid object's (an emitter's) temperature is what its particles are inserted with from then
   on -- and what its held layers, which are boundary particles, are held at.
   sph_heat_pair_host: the walk's pair arithmetic (heat_pair of csrc/sph_thermal.hpp) from the kernels' own source on the CPU, strict
   (fast = 0) or fast form.  in: n records of 12 floats (T_i, c_j, T_j, dx, dy, dz, r2, eps, gs, gx, gy, gz; the strict form reads the
   gradient, the fast form gs with gradW = gs R); out: n floats, c_j (T_i - T_j) F_ij.  sph_heat_finish_host (an addition): what follows
   the sum, and the buoyancy.  in: n records of 12 floats (sum, 2 alpha, rho0, rho_i, dt, T_i, -beta, t_ref, g[3], unused); out: n
   records of 5 floats (dT/dt, T_new, a_b[3]).  Neither touches a device. */
#define SPH_THERMAL_NONE 0
#define SPH_THERMAL_CONDUCTION 1
typedef struct { int32_t method; double alpha, beta, t_ref; } SphThermal;
int sph_set_thermal(SphHandle *h, const SphThermal *params);
int sph_get_thermal(SphHandle *h, SphThermal *out);
int sph_set_object_temperature(SphHandle *h, int object_id, double temperature, int has_T);
int sph_heat_pair_host(const float *in, int64_t n, float *out, int fast);
int sph_heat_finish_host(const float *in, int64_t n, float *out, int fast);

/* Device rigid integrator (opt-in; the host's "device" rigid backend).  The physics of the host's native backend
   (SPH/rigid_solver/host_rigid_solver.py integrate: semi-implicit Euler in float64 under gravity and the fluid wrench, gyroscopic
   term, rotation by exp([dt w]x), re-orthonormalisation, inelastic wall contact of the body's axis-aligned extent) in one kernel
   launch between the two halves of every step, one workgroup per registered body.  With it sph_step / sph_step_async carry dynamic
   bodies without any host work.  All arguments float64, scene frame, rot9 / inertia_body row-major.
   sph_set_rigid_integrator stands in for PyBulletSolver.__init__ (bullet_solver.py:19-71: gravity, time step, the wall boxes);
   wall_lo / wall_hi are the planes no part of a body may cross.  on = 0 turns the launch off.
   sph_set_rigid_body stands in for insert_rigid_object (bullet_solver.py:75-131: mass, inertia, base position, orientation and
   velocity of a body): it registers body object_id or replaces it, uploads its body-frame points (float64[npoints][3]) and marks
   the pose dirty, so the next renew_rigid_particle_state applies it; com0 (may be NULL) is the rest centre of mass, as in
   sph_set_rigid_pose.
   sph_get_rigid_state stands in for the read-back of bullet_solver.py:158-167 and get_rigid_body_states (:169-176); it drains the
   stream first.  Any output may be NULL.
   sph_rigid_integrate stands in for PyBulletSolver.step (bullet_solver.py:144-167) of a host that drives the halves itself: the
   launch on its own, valid only between sph_step_begin and sph_step_end; exactly what sph_step runs between its halves (after the
   contact pass, if that is on).  The launch reads the wrench as sph_get_rigid_wrench returns it (rounded through float32) and
   clears the whole wrench array, as sph_get_rigid_wrench(reset = 1) does.
   SPH_ERR_UNSUPPORTED: a PBF handle (PBF.py moves no body), a sharded handle (the wrench would need an all-reduce inside the step),
   a handle whose axis order is not "xyz".  SPH_ERR_INVALID: a bad object id, a singular inertia, mass <= 0, npoints < 0,
   sph_get_rigid_state of an unregistered body, sph_rigid_integrate outside a step or with the integrator off -- and
   sph_set_rigid_pose on a registered body while the integrator is on (one master per body). */
int sph_set_rigid_integrator(SphHandle *h, int on, const double *gravity, const double *wall_lo, const double *wall_hi);
int sph_set_rigid_body(SphHandle *h, int object_id, double mass, const double *inertia_body, const double *com, const double *rot9,
                       const double *vel, const double *angvel, const double *com0, const double *points, int npoints);
int sph_get_rigid_state(SphHandle *h, int object_id, double *com, double *rot9, double *vel, double *angvel);
int sph_rigid_integrate(SphHandle *h);

/* Device contact solver (opt-in; the host's "device_contact" rigid backend).  The physics of the host's "contact" backend
   (SPH/rigid_solver/host_rigid_solver.py: contacts_from_table, then ContactSolver.step -- the integrator's velocity half, one contact per
   non-empty table key of a registered body in ascending (A, B, bin) order, `iterations` sweeps of sequential impulses with restitution,
   Coulomb friction and rolling resistance, `iterations` sweeps of split impulses, positions) in ONE kernel launch of one workgroup, in
   float64.  While it is on, that launch takes the place of the integrator's in sph_step / sph_step_async / sph_rigid_integrate: it runs
   after the contact pass, reads the wrench as the integrator does and the table as sph_get_rigid_contacts returns it, and clears both
   (as reset = 1 does); it does NOT apply the integrator's extent wall rule -- a body meets the walls through the contact pass (the
   domain box's particles or the six wall planes).  sph_get_rigid_contact_pairs is left alone.
   sph_set_rigid_contact_solver stands in for ContactSolver.__init__ and the two attributes the backend sets: restitution, friction,
   sweeps, beta (the share of the depth the split impulses remove per step), slop (the depth a resting contact keeps) and patch (the
   rolling-resistance radius), the last two in scene units.  on = 0 returns the launch to the integrator; turning the integrator
   (sph_set_rigid_integrator) or the contact pass (sph_set_rigid_contact) off turns the solver off too.
   SPH_ERR_UNSUPPORTED: as sph_set_rigid_integrator (PBF, a sharded handle, an axis order other than "xyz").  SPH_ERR_INVALID: the
   integrator or the contact pass is off, iterations outside 1..64, a parameter that is negative or not finite.
   sph_get_rigid_contact_rows: the rows of the last solve (diagnostics, tests); drains the stream first.  It always writes *count (the
   rows of the last solve) and copies min(count, capacity) rows of SPH_CONTACT_ROW_VALUES doubles:
     [0] A  [1] B (-1: an infinite-mass partner)  [2..4] point  [5..7] normal (from B towards A)  [8] depth  [9] normal impulse
     [10..11] friction impulses  [12..13] rolling impulses  [14] split impulse  [15] the table's partner index (20 + bin: box / wall plane)
   rows may be NULL with capacity 0. */
#define SPH_CONTACT_ROW_VALUES 16
int sph_set_rigid_contact_solver(SphHandle *h, int on, double restitution, double friction, int iterations, double beta, double slop,
                                 double patch);
int sph_get_rigid_contact_rows(SphHandle *h, double *rows, int capacity, int *count);

/* Scripted rigid bodies (opt-in; the scene key "motion" of a RigidBodies entry).  A scripted body is neither frozen nor
   free: its pose is a function of time, the superposition of up to three blocks -- keyframes, a harmonic oscillation, a constant drift.
   The program is given in canonical form (angles in radians, directions and axes normalised or zero, end = +infinity for "never"):
     dt  = (double)(float)timeStepSize,  t_k = k * dt  (k = steps completed since sph_prepare: a product, never a running sum)
     tau = clamp(t, start, end) - start
     h   = min(1, tau / ramp) * sin(2 pi frequency tau + phase)                                        (ramp = 0: no ramp)
     d     = key_translation(tau) + (h * amplitude) * direction + tau * drift_velocity
     theta = key_rotation(tau) + ((h * angle) * axis + (tau * drift_rate) * drift_axis)                (a rotation vector, radians)
     E = exp([theta]x),  rot(t) = E rot_rest,  com(t) = com_rest + rot_rest pivot + d - E rot_rest pivot
   key_*: the piecewise interpolant (linear, or smooth: s <- s s (3 - 2 s)) of the key values at tau mapped into [0, T] by the repeat mode
   (hold, loop, pingpong), T the last key time; zero without keys.  All of it in float64 with every product rounded, in both builds.
   The velocities of step k -> k + 1 are the step's backward differences, so that every particle of the body moves by dt times the
   velocity the fluid passes saw:  vel = (com(t_k+1) - com(t_k)) / dt;  M = rot(t_k+1) rot(t_k)^T, a = vee(M - M^T) / 2, s = |a|,
   c = (tr M - 1) / 2, angvel = (atan2(s, c) / s) a / dt  (a / dt for s <= 1e-12).
   sph_set_rigid_motion registers (or replaces) the program of object_id and its rest pose (com_rest, rot_rest row-major; com0, may be NULL,
   the rest centre of mass as in sph_set_rigid_pose).  Legal before and after sph_prepare.  The body takes the zero-velocity pose of the
   time the running step ends at (between sph_step_begin and sph_step_end: t_k+1; otherwise t_k) and the pose is marked dirty, as by
   sph_set_rigid_body.  From then on ONE launch (SPH_K_RIGID_MOTION, one wave per scripted body) runs in every step where the device
   integrator's does -- in sph_step, sph_step_async and sph_rigid_integrate, before that launch, with or without sph_set_rigid_integrator:
   it writes the float64 record and the float32 pose, reads the body's six wrench words as sph_get_rigid_wrench returns them (rounded
   through float32), clears them and adds dt * force, dt * torque to float64 impulse sums.  A handle without scripted bodies launches
   nothing.  A scripted body is no registered body of the integrator or the contact solver: to them it is an infinite-mass partner.
   sph_get_rigid_motion_state drains the stream and returns the record.
   sph_rigid_motion_eval_host: the device's routine on the CPU (the same source): pose and velocities of step k -> k + 1 into
   out->com / rot / vel / angvel, out->steps = k + 1; the other fields are zeroed.  No device is touched.
   SPH_ERR_UNSUPPORTED: as sph_set_rigid_integrator (PBF, a sharded handle, an axis order other than "xyz").  SPH_ERR_INVALID, with a
   message that names the field: a bad object id, a bad program (more than SPH_RIGID_MOTION_MAX_KEYS keys, times that do not start at 0
   or do not increase strictly, a non-finite number, an unknown interpolation or repeat mode, a direction or axis that is neither zero
   nor of unit length, a negative frequency or ramp, end <= start), a body registered through sph_set_rigid_body -- and
   sph_set_rigid_body or sph_set_rigid_pose on a scripted body (one master per body). */
#define SPH_RIGID_MOTION_MAX_KEYS 64
typedef struct {
    double start, end;                 /* scene time, seconds; end = +infinity: never */
    double pivot[3];                   /* body frame: the point rotations turn about */
    int32_t nkeys;                     /* 0: no keyframes */
    int32_t interpolation;             /* 0 linear, 1 smooth */
    int32_t repeat;                    /* 0 hold, 1 loop, 2 pingpong */
    int32_t reserved;                  /* 0 */
    double key_times[SPH_RIGID_MOTION_MAX_KEYS];
    double key_translations[SPH_RIGID_MOTION_MAX_KEYS][3];
    double key_rotations[SPH_RIGID_MOTION_MAX_KEYS][3];   /* rotation vectors, radians */
    double frequency, phase, ramp;     /* Hz, radians, seconds */
    double direction[3], amplitude;    /* unit or zero, metres */
    double axis[3], angle;             /* unit or zero, radians */
    double drift_velocity[3];          /* m/s */
    double drift_axis[3], drift_rate;  /* unit or zero, rad/s */
} SphRigidMotion;
typedef struct {
    double com[3], rot[9], vel[3], angvel[3];   /* pose at t_steps, velocities of the step that led there */
    double force[3], torque[3];                 /* the wrench the last launch consumed */
    double impulse[3], angular_impulse[3];      /* sums of dt * force, dt * torque over the launches */
    int64_t steps;                              /* the step count the pose holds at */
} SphRigidMotionState;
int sph_set_rigid_motion(SphHandle *h, int object_id, const SphRigidMotion *program, const double *com_rest, const double *rot_rest,
                         const double *com0);
int sph_get_rigid_motion_state(SphHandle *h, int object_id, SphRigidMotionState *out);
int sph_rigid_motion_eval_host(const SphRigidMotion *program, const double *com_rest, const double *rot_rest, double dt, int64_t k,
                               SphRigidMotionState *out);

/* Fluid emitters (opt-in; the scene list "Emitters"): a nozzle -- a rectangle or a circle in a plane -- that emits layers
   of fluid particles on the device.  The program is given in canonical form: direction, tangent1, tangent2 an orthonormal basis computed
   once on the host, end = +infinity for "until the budget is spent".  With spacing = 2 particle_radius:
     lattice:  nu = floor(width / spacing), nv = floor(height / spacing) (circle: both floor(2 radius / spacing)); point (i, j) lies at
               ((i + 0.5 - nu / 2) spacing) tangent1 + ((j + 0.5 - nv / 2) spacing) tangent2; a circle keeps a^2 + b^2 <= radius^2;
               layer_n = the number of points; order j slow, i fast, the circle's gaps closed
     schedule: dt = (double)(float)timeStepSize, T_k = k dt (k = steps completed since sph_prepare: a product, never a running sum)
               s(k) = speed max(0, min(T_k, end) - start);  max_layers = floor(max_particles / layer_n)
               born(k) = 0 if T_k < start, else min(max_layers, floor(s(k) / spacing) + 1);  a_j(k) = s(k) - j spacing
               layer j < born(k) is HELD while a_j(k) < hold spacing and T_k <= end
   All of it in float64 with every product rounded, in both builds; a position  position + a_j direction + a tangent1 + b tangent2  is
   rounded to float32 once.  sph_prepare emits born(0); the step that takes the count from k - 1 to k emits the layers born(k - 1) ..
   born(k) - 1 at its insertion point (sph_step / sph_step_async: behind the rigid integrator's launch; sph_step_end: behind the
   boundary pass of what the host appended), ONE launch (k_emit, one thread per newborn particle of all emitters) that writes what
   sph_append_particles writes -- ids = the particle count at that moment + the index within the batch, emitters in index order --
   and applies the domain boundary; before it ONE elementwise launch (k_emit_hold) overwrites position and velocity of every held particle
   (found by id) with the closed form at T_k.  Both are profiled as SPH_K_EMIT; steps in which no layer is born / held launch
   neither.  The host evaluates the schedule itself: no read-back, no copy, no synchronisation per step.  The capacity
   max_layers layer_n of every emitter is reserved inside particle_max_num: sph_set_emitter returns SPH_ERR_CAPACITY when the budgets
   do not fit, sph_append_particles when an append would eat into them, emission never.
   sph_set_emitter: before sph_prepare only (SPH_ERR_INVALID after it); index 0 .. SPH_MAX_EMITTERS - 1 (a set index may be replaced).
   SPH_ERR_UNSUPPORTED, with a message that names the emitter: a sharded handle (and sph_comm_set_slab while an emitter is set), a PBF handle
   (either variant: PBF never inserts), a handle with g_upper set (gravitationUpper), an axis order other than "xyz"; and, once an
   emitter is set, sph_set_appended_ids, an upload of SPH_F_PARTICLE_ID, sph_set_elastic_object on an emitter's object and
   sph_append_particles into it.  SPH_ERR_INVALID, with a message that names the emitter and the field: an object id that is out of
   range, owns particles or belongs to another emitter, an unknown shape, a basis that is not orthonormal, a size, speed, density or
   max_particles that is not positive and finite, layer_n == 0, max_particles < layer_n, hold outside 0 .. SPH_EMITTER_MAX_HOLD,
   end <= start, speed dt > 0.5 spacing (so at most one layer per emitter is born per step).
   sph_get_emitter_state: what the host knows, no device access.  sph_emitter_eval_host: the kernels' routine on the CPU (the same
   source): the schedule after k steps and, with layer >= 0 and xyz != NULL, the float32 positions xyz[layer_n][3] of that layer at
   that count (the domain boundary not applied).  No device is touched. */
#define SPH_MAX_EMITTERS 8
#define SPH_EMITTER_MAX_HOLD 8
#define SPH_EMITTER_RECTANGLE 0
#define SPH_EMITTER_CIRCLE 1
typedef struct {
    int32_t object_id;                 /* a fluid object of its own */
    int32_t shape;                     /* SPH_EMITTER_RECTANGLE, SPH_EMITTER_CIRCLE */
    int32_t max_particles;             /* the emitter's budget */
    int32_t hold;                      /* layers kept kinematic behind the plane, 0 .. SPH_EMITTER_MAX_HOLD */
    double position[3];                /* centre of the nozzle plane */
    double direction[3], tangent1[3], tangent2[3];   /* orthonormal; tangent1 carries "width", tangent2 "height" */
    double width, height;              /* rectangle, metres */
    double radius;                     /* circle, metres */
    double speed;                      /* m/s along direction */
    double start, end;                 /* scene time, seconds; end = +infinity: until the budget is spent */
    double density;                    /* kg/m^3: mass = V0 density */
    int32_t color[3];                  /* 0 .. 255 */
    int32_t reserved;                  /* 0 */
} SphEmitter;
typedef struct {
    int32_t object_id, layer_particles, max_layers;
    int32_t layers;                    /* layers born so far */
    int32_t emitted;                   /* particles emitted so far = layers * layer_particles */
    int32_t held_layers;               /* layers the last slot held (the schedule at the current step count) */
    int32_t held_first;                /* index of the first of them */
    int32_t exhausted;                 /* layers == max_layers, or the current time is past `end` */
    int32_t held_id_base[SPH_EMITTER_MAX_HOLD + 1];   /* persistent id of the first particle of each held layer */
    int32_t reserved[3];
} SphEmitterState;
typedef struct {
    double T, s;                       /* T_k, s(k) */
    int32_t born;                      /* born(k) */
    int32_t held_first, held_layers;   /* the held range [held_first, held_first + held_layers) */
    int32_t layer_particles, max_layers, nu, nv;
    int32_t reserved;
    double layer_offset;               /* a_layer(k) of the layer asked for (0 when layer < 0) */
} SphEmitterEval;
int sph_set_emitter(SphHandle *h, int index, const SphEmitter *emitter);
int sph_get_emitter_state(SphHandle *h, int index, SphEmitterState *out);
int sph_emitter_eval_host(const SphEmitter *emitter, double dt, double spacing, int64_t k, int layer, SphEmitterEval *out, float *xyz);

/* Outflow (opt-in; the scene list "Outflows"): up to SPH_MAX_OUTFLOWS kill volumes -- an axis-aligned box or a sphere, in
   the scene frame -- that remove fluid on the device, and removal by persistent id from the host.
     predicate: float32, on the stored position.  The bounds are rounded to float32 once, at sph_set_outflow.  Box: min <= x <= max in
               every component (faces inclusive).  Sphere: dx = x - cx, ...; (dx dx + dy dy) + dz dz <= r r, every product and sum
               rounded (no contraction in either build).  invert negates the result (a keep-region).  A particle inside several volumes
               counts for the lowest index.  Only active fluid particles (SPH_MAT_FLUID) of the listed objects (n_objects == 0: of every
               object) are tested; rigid particles never leave.
     window:   T_k = k dt, dt = (double)(float)timeStepSize, k = the step count the running step ends at; a volume is active while
               start <= T_k <= end (end = +infinity: for ever).  Evaluated on the host; the kernel sees the active volumes only.
     slot:     the insertion point of a step, between the emitters' hold and their emission: newborn particles are first tested one step
               later, a held particle that is removed is gone (the hold pass finds ids; an id it does not find costs nothing).
   ONE elementwise launch (k_outflow_mark, profiled as SPH_K_OUTFLOW) sets the dead bit and counts per volume; the host reads the eight
   counters back once per step while a volume is active (one small copy into pinned memory and one stream wait).  The next neighbour
   search files the dead behind the grid (the graveyard cells a slab rank drops its ghosts into) and particle_num / fluid_particle_num
   shrink; sph_step and sph_step_end run that search before they return when their last slot removed something, so a caller never
   sees a dead particle.  Both sort modes (deterministic on or off) take the graveyard route for such a sort; every other sort is the
   one it was.  While a volume is set no step is pre-hashed by its own force pass / position update (SphStats::prehashed_sorts stays),
   and sph_step_async returns SPH_ERR_UNSUPPORTED (the count needs the host); sph_step(h, n) works for any n.
   Ids stop being slots with the first removal: new particles (sph_append_particles, emitters) get ids from a counter that only grows,
   and particle_max_num then bounds the particles EVER created (the arrays kept by id -- colours at home, micropolar angular velocities
   -- are indexed by it): SPH_ERR_CAPACITY from sph_append_particles / sph_set_emitter accordingly.  Ids are not recycled.
   SPH_F_CG_X (slot-indexed, not reordered by the sort) is only a warm start after a removal.
   sph_set_outflow: any time outside a step (between sph_step_begin and sph_step_end: SPH_ERR_INVALID); volume == NULL clears the index.
   SPH_ERR_UNSUPPORTED, with the reason: a PBF handle (either variant), a sharded handle (and sph_comm_set_slab while a volume is set),
   g_upper set, an axis order other than "xyz" (unreachable today: only sph_comm_set_slab permutes the axes, and a sharded handle is
   refused first), ids set from outside (sph_set_appended_ids / SPH_F_PARTICLE_ID; and those two while a
   volume is set), an elastic object present (and sph_set_elastic_object while a volume is set).  SPH_ERR_INVALID, naming the field:
   an unknown shape, a bound that is not finite, min >= max in a component, radius <= 0, end <= start, an object id outside the
   handle's objects or one that is not a fluid object.
   sph_get_outflow_state: what the host knows (no device access).
   sph_remove_particles: removal by persistent id, between steps or between sph_step_begin and sph_step_end (there the dead leave in
   sph_step_end, as what a volume marks in the slot).  Every id must name a live active fluid particle and appear once: otherwise
   SPH_ERR_INVALID and nothing is removed.  The device counts what it marks and the call checks that count against n.  The same
   refusals as sph_set_outflow.  A second kernel marks by binary search in the sorted
   id list (k_outflow_mark_ids, SPH_K_OUTFLOW).
   sph_outflow_test_host: the kernels' predicate on the CPU (the same source), one volume over n points xyz[n][3]: inside[k] = 0 / 1
   (geometry and invert; no window, no object list).  sph_outflow_active_host: the window test at step count k (0 / 1; < 0: an error).
   No device is touched. */
#define SPH_MAX_OUTFLOWS 8
#define SPH_OUTFLOW_MAX_OBJECTS 16
#define SPH_OUTFLOW_BOX 0
#define SPH_OUTFLOW_SPHERE 1
typedef struct {
    int32_t shape;                     /* SPH_OUTFLOW_BOX, SPH_OUTFLOW_SPHERE */
    int32_t invert;                    /* != 0: remove what is OUTSIDE the shape */
    double min[3], max[3];             /* box, scene frame, metres */
    double center[3], radius;          /* sphere */
    double start, end;                 /* scene time, seconds; end = +infinity: for ever */
    int32_t n_objects;                 /* 0: every fluid object; else objects[0 .. n_objects) */
    int32_t objects[SPH_OUTFLOW_MAX_OBJECTS];
    int32_t reserved;                  /* 0 */
} SphOutflow;
typedef struct {
    int64_t removed;                   /* particles this volume has removed since it was set */
    int32_t removed_last_step;         /* ... in the last slot (step or SPH_PH_OUTFLOW) */
    int32_t active;                    /* the window holds the current step count */
    int32_t reserved[4];
} SphOutflowState;
int sph_set_outflow(SphHandle *h, int index, const SphOutflow *volume);
int sph_get_outflow_state(SphHandle *h, int index, SphOutflowState *out);
int sph_remove_particles(SphHandle *h, const int32_t *ids, int n);
int sph_outflow_test_host(const SphOutflow *volume, const float *xyz, int n, uint8_t *inside);
int sph_outflow_active_host(const SphOutflow *volume, double dt, int64_t k);

/* Adaptive time stepping (opt-in; the scene keys cflMethod / cflFactor / cflMinTimeStepSize / cflMaxTimeStepSize): the
   device finds the largest particle speed at the end of every step and the library sets the next step's dt from it.
     who counts: active fluid particles that have not been removed, and the rigid particles of dynamic bodies (their stored velocity is
               v + w x r).  Static rigid particles, ghosts and the dead do not.
     speed:    float32, (vx vx + vy vy) + vz vz with every product and sum rounded: the same bits in the strict and the fast build.  ONE
               elementwise launch (k_cfl_speed, profiled as SPH_K_CFL) reduces it: a maximum per thread, across the 64 lanes of a wave,
               one atomic maximum per wave on the bit pattern; the host reads the maximum and a non-finite flag back once per step (one
               small copy into pinned memory and one stream wait).
     rule:     in double, d = 2 particle_radius, v = sqrt(vmax2):
                   dt = v max_dt > factor 0.4 d ? factor 0.4 d / v : max_dt;   dt = max(dt, min_dt);
                   with a time target: n = ceil(remaining / dt), dt = remaining / n;   dt = (double)(float)dt
               The landing step is never above the CFL step and, while the target is at least one CFL step away, never below half of it.
     slot:     the end of a step, behind everything that changes a velocity, before the scene time advances.  The first step size comes
               from a reduce in sph_prepare (or in sph_set_cfl on a prepared handle).  Particles appended and fields uploaded since the
               last reduce make the next step begin with one.
     time:     the scene time is the double sum of the float32 steps taken.  A target counts as reached when t_end - t <= 2^-20 max_dt.
   A non-finite square is SPH_ERR_INVALID ("non-finite velocity") from the call that stepped; the step size stays what it was.
   While the mode is on sph_step_async returns SPH_ERR_UNSUPPORTED (the maximum needs the host); sph_step(h, n) and the sph_step_begin /
   sph_step_end pair work.  A velocity criterion knows nothing of a sound speed: under WCSPH max_dt has to stay at the stiff limit.
   sph_set_time_step: a new step size between steps (SPH_ERR_INVALID inside one, and for a dt that is not positive and finite as a
   float32).  SPH_ERR_UNSUPPORTED while the CFL mode is on, and on every handle the mode refuses (below).
   sph_set_cfl: params == NULL or method SPH_CFL_NONE switches the mode off and restores the step size the handle was created with.
   SPH_ERR_INVALID, naming the field: an unknown method, a number that is not positive and finite, min_dt > max_dt.
   SPH_ERR_UNSUPPORTED, with the reason: an emitter, a motion program or an outflow volume is set (their programs are closed forms of
   k dt; and sph_set_emitter / sph_set_rigid_motion / sph_set_outflow while the mode is on), a PBF handle (either variant), a sharded
   handle (and sph_comm_set_slab while the mode is on), g_upper set (its frozen particles carry the rigid material).
   sph_get_cfl: the parameters (method SPH_CFL_NONE while the mode is off).
   sph_get_time_state: what the host knows (no device access).
   sph_set_time_target: the step sizes from now on land on t_end; a value that is not finite clears the target.  The pending dt is
   computed again from the stored maximum (host arithmetic only).  SPH_ERR_INVALID while the mode is off.
   sph_advance_until: sets the target, steps until it is reached or max_steps steps are done (SPH_OK both ways; steps_done says how
   many), then clears the target and restores the pending dt.
   sph_cfl_dt_host: the rule on the CPU (the same source).  remaining: not finite = no target.  sph_cfl_speed2_host: the reduce on the
   CPU (the same source) over vel[n][3]; meta[i]: material << 8 | (is_dynamic ? 1 << 10 : 0) | (ghost ? 1 << 11 : 0) | (removed ?
   1 << 12 : 0), the library's particle word.  No device is touched. */
#define SPH_CFL_NONE 0
#define SPH_CFL_VELOCITY 1
#define SPH_CFL_CLAMPED_MAX 1          /* SphTimeState::flags: the step is max_dt */
#define SPH_CFL_CLAMPED_MIN 2          /* ... is min_dt */
#define SPH_CFL_LANDING 4              /* ... was shortened to land on the time target */
#define SPH_CFL_STALE 8                /* ... will be computed again: the next step begins with a reduce */
typedef struct {
    int32_t method;                    /* SPH_CFL_NONE, SPH_CFL_VELOCITY */
    int32_t reserved;                  /* 0 */
    double factor;                     /* cflFactor */
    double min_dt, max_dt;             /* cflMinTimeStepSize, cflMaxTimeStepSize, seconds */
} SphCflParams;
typedef struct {
    double time;                       /* scene time, seconds */
    double dt_next;                    /* the step size the next step takes */
    double dt_last;                    /* ... the last step took (0 before the first) */
    double target;                     /* the time target (NaN: none) */
    float vmax2;                       /* the maximum of |v|^2 the last reduce found */
    int32_t flags;                     /* SPH_CFL_* of dt_next */
    int64_t steps;
    int32_t reserved[4];
} SphTimeState;
int sph_set_time_step(SphHandle *h, double dt);
int sph_set_cfl(SphHandle *h, const SphCflParams *params);
int sph_get_cfl(SphHandle *h, SphCflParams *out);
int sph_get_time_state(SphHandle *h, SphTimeState *out);
int sph_set_time_target(SphHandle *h, double t_end);
int sph_advance_until(SphHandle *h, double t_end, int max_steps, int *steps_done);
int sph_cfl_dt_host(const SphCflParams *params, double diameter, float vmax2, double remaining, double *dt, int32_t *flags);
int sph_cfl_speed2_host(int64_t n, const float *vel, const int32_t *meta, float *vmax2, int32_t *nonfinite);

/* --- time stepping --------------------------------------------------------------------- */
/* replaces XSolver.prepare() (base_solver.py:683, DFSPH.py:321, PCISPH.py:188); particles of
   entryTime <= 0 must have been appended */
int sph_prepare(SphHandle *h);
/* replaces XSolver.step() (base_solver.py:692) called nsteps times; synchronous on return */
int sph_step(SphHandle *h, int nsteps);
/* enqueue nsteps without the trailing host synchronisation (bench / overlap); only valid when no
   per-iteration host read-back is needed (wcsph, or fixed_iterations > 0) */
int sph_step_async(SphHandle *h, int nsteps);
int sph_synchronize(SphHandle *h);
/* One step in two halves, for hosts that act in the middle of _step() exactly where the reference does:
   sph_step_begin runs _step() up to (not including) `self.rigid_solver.step()` (WCSPH.py:39, DFSPH.py:305,
   PCISPH.py:179); the host then integrates rigid bodies (sph_get_rigid_wrench / sph_set_rigid_pose =
   bullet_solver.py:144-167) and appends objects whose entryTime has come (sph_append_particles =
   base_container.py:212-341); sph_step_end runs the rest: renew_rigid_particle_state + enforce_domain_boundary
   (+ for DFSPH the neighbour search, density, alpha and divergence solve, DFSPH.py:311-319) and step()'s tail
   (base_solver.py:694-696, including compute_rigid_particle_volume on the grid of the last sort).
   sph_step(h, 1) == sph_step_begin(h); sph_step_end(h). */
int sph_step_begin(SphHandle *h);
int sph_step_end(SphHandle *h);
/* one reference kernel group at a time (tests) */
int sph_run_phase(SphHandle *h, int phase);

/* --- state access ---------------------------------------------------------------------- */
/* replaces field.to_numpy() / BaseContainer.dump (base_container.py:599).  bytes must equal
   particle_num * element size of the field. */
int sph_download(SphHandle *h, int field, void *dst, size_t bytes);
int sph_upload(SphHandle *h, int field, const void *src, size_t bytes);
int sph_particle_num(SphHandle *h);       /* container.particle_num[None] */
int sph_fluid_particle_num(SphHandle *h); /* container.fluid_particle_num[None] */
int sph_get_stats(SphHandle *h, SphStats *out);
/* implicit viscosity: alpha, beta and error (base_solver.py:403, :428, :431) as the last launch that computes them left them on the
   device, out[0..2].  A query of its own rather than SphStats fields: the statistics struct ends at pbf_recentred by contract. */
int sph_get_cg_scalars(SphHandle *h, float *out);

/* The tables of the uniform grid as the last sort left them on the device (for tests and diagnosis).
   sph_download_grid_table waits for the stream and copies; sph_get_grid_layout reads what the host knows (an unsharded handle's counts
   are exact on the host).  Neither launches anything nor changes a state flag, so a step behaves the same whether or not they were
   called.  All of it is in the LIBRARY's frame: library axis k is scene axis axis_map[k], library x is the slowest axis of the
   cell order, lin = (cx * ny + cy) * nz + cz.  SPH_ERR_UNSUPPORTED on a sharded handle (sph_comm_set_slab: a slab's grid is local).
   SPH_ERR_INVALID: a NULL argument, an unknown table, bytes that differ from the table's size. */
typedef struct {
    int32_t nx, ny, nz;        /* cells per library axis */
    int32_t G;                 /* nx * ny * nz */
    int32_t scan_tile;         /* cells per tile of the prefix scan (2048) */
    int32_t axis_map[3];       /* scene axis of each library axis */
    float cell_size;           /* edge of a cell = the support radius, as the kernels divide by it */
    int32_t n;                 /* live particles */
    int32_t tiles;             /* tiles of 256 consecutive particle slots: ceil(n / 256) */
    int32_t tile_header_ints;  /* ints per tile header (20): first cell, last cell, 9 run starts, 9 run lengths */
    int32_t tiles_valid;       /* 1: tile headers, lane permutation and cell words were built for the current order of these n particles */
} SphGridLayout;
typedef enum {
    SPH_GRID_CELL_START = 0,   /* i32[G + 1]: exclusive prefix sum of the cell populations, [G] = n */
    SPH_GRID_TILE_HEADER = 1,  /* i32[tiles][tile_header_ints] */
    SPH_GRID_LANE_PERM = 2,    /* u8[tiles][256]: lane -> slot inside the tile */
    SPH_GRID_CELL_WORD = 3     /* u32[n]: per particle, bits 0-7 window entry of (.., .., z0), 8-10 z1 - z0 + 1, 11-19 column-exists bits */
} SphGridTable;
int sph_get_grid_layout(SphHandle *h, SphGridLayout *out);
int sph_download_grid_table(SphHandle *h, int which, void *dst, size_t bytes);

/* --- profiling (HIP events on the compute stream) -------------------------------------- */
/* record a HIP event pair around every launch of `kernel_id` (-1: all kernels); accumulates. */
int sph_profile_enable(SphHandle *h, int kernel_id, int on);
int sph_profile_reset(SphHandle *h);
/* resolves pending events; returns launches and total milliseconds of that kernel id */
int sph_profile_read(SphHandle *h, int kernel_id, int64_t *launches, double *total_ms);
const char *sph_kernel_name(int kernel_id);
/* device properties the bench reports: name (<=255 chars), CU count, HBM bytes */
int sph_device_info(SphHandle *h, char *name256, int *cu_count, int64_t *hbm_bytes);

/* device-to-device copy rate of this GPU, measured now (the second denominator of the bench's HBM roofline next to the
   8 TB/s spec): `reps` hipMemcpyAsync D2D copies of `bytes` bytes between two scratch buffers on the handle's
   stream, bracketed by HIP events; *gb_per_s = (read + written bytes) / time = 2 * bytes * reps / t.  The scratch is freed
   before returning. */
int sph_measure_copy_rate(SphHandle *h, size_t bytes, int reps, double *gb_per_s);

/* --- multi-GPU: z-slab sharding, one process per GPU, RCCL over xGMI ------------------- */
/* number of HIP devices this process sees (launchers map local rank -> device without any other runtime) */
int sph_device_count(void);
/* 128-byte RCCL unique id, created on rank 0 and distributed by the host launcher */
int sph_comm_unique_id(void *out128);
/* attach this handle to a communicator of `nranks` processes (RCCL ncclCommInitRank; SPH_COMM_TRANSPORT=shm:
   POSIX shared memory, several ranks may then share one GPU -- test rig) */
int sph_comm_init(SphHandle *h, int rank, int nranks, const void *id128);
/* what carries the halo messages of this handle: "rccl", "shm", "ipc-push+rccl", "ipc-push+shm" ("none" before sph_comm_init).
   Default (SPH_COMM_TRANSPORT unset / "auto"): RCCL for barriers and all-reduces; halo payload by device stores straight into the
   neighbour's inbox, mapped through hipIpc ("push"), if that can be set up and passes its self-test on EVERY rank, else RCCL
   ncclSend / ncclRecv.  "ipc": push or fail; "rccl": RCCL only; "shm" / "shm+ipc": shared-memory control plane (several ranks on
   one GPU, test rig) with host-staged mailboxes / with the push transport. */
const char *sph_comm_transport(SphHandle *h);
/* turn the handle into one z-slab: it owns the cell layers [z_lo, z_hi) of the SCENE's z (global grid) plus one ghost layer on each
   interior side; before any particle is appended.  Everything a caller hands over or reads back stays in the scene's frame.  Inside,
   the slabs are cut along the fastest axis of the cell order (default) or -- SPH_SLAB_LAYOUT=slow -- the scene's z is mapped onto the
   library's slowest axis at this boundary (positions, velocities, every 3-vector field, gravity, domain, rigid poses and wrenches are
   permuted).  Inside a multi-step call (sph_step_async(n)) a sharded WCSPH step lets its force pass write the NEXT step's
   halo message: between such steps the device state is half-classified, which no host call can observe (every read settles first). */
int sph_comm_set_slab(SphHandle *h, int z_lo, int z_hi);
int sph_comm_get_slab(SphHandle *h, int *z_lo, int *z_hi, int *n_owned, int *n_ghost);
/* slab cuts follow the fluid: every `every_steps` steps (default 64, env SPH_SLAB_REBALANCE; 0 = never) the ranks
   all-reduce their per-layer particle histograms and move each interior cut by at most one cell layer towards the
   balanced plan; the layer that changes hands migrates through the ordinary per-step exchange */
int sph_comm_set_rebalance(SphHandle *h, int every_steps);
/* late entry (base_container.py:218-221) under sharding: the object holds n particles in the whole scene, n_fluid of them
   fluid; every rank calls this next to its sph_append_particles of the slab's share (which may be empty) */
int sph_comm_add_global_count(SphHandle *h, int n, int n_fluid);
/* host-visible collectives over the communicator (what a launcher otherwise needs MPI / torch.distributed for):
   in-place all-reduce of <= 128 doubles, op 0 sum / 1 max / 2 min (ncclAllReduce); barrier = drain the stream,
   then all-reduce; both synchronous.  The solver residuals of a sharded DFSPH / PCISPH step use the same path. */
int sph_comm_allreduce(SphHandle *h, double *inout, int count, int op);
int sph_comm_barrier(SphHandle *h);
/* transport self-test: ring shift of n floats (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd; a self pair when
   the communicator has one rank), every word checked, plus an all-reduce check */
int sph_comm_selftest(SphHandle *h, int n);

/* --- mesh -> particles (host code, no GPU involved) ------------------------------------ */
/* replaces trimesh's mesh.voxelized(pitch).fill().points in BaseContainer.load_rigid_body (base_container.py:641-642):
   voxel centres (integer multiples of pitch) of the surface voxels plus the region they enclose, f32 xyz, x slowest.
   out_xyz == NULL: only *n_points is set. */
int sph_voxelize_mesh(const double *vertices, int n_vertices, const int32_t *faces, int n_faces, double pitch,
                      float *out_xyz, int64_t capacity_points, int64_t *n_points);
/* replaces mesh.contains(lattice) in BaseContainer.load_fluid_body (base_container.py:686-694): crossing parity along z;
   inside[(i * ny + j) * nz + k] for the point (xs[i], ys[j], zs[k]) */
int sph_points_in_mesh(const double *vertices, int n_vertices, const int32_t *faces, int n_faces, const double *xs, int nx,
                       const double *ys, int ny, const double *zs, int nz, uint8_t *inside);

/* --- frame export (host code, no GPU involved) ------------------------------------------ */
/* replaces ti.tools.PLYWriter(num_vertices = n).add_vertex_pos(x, y, z).export_ascii(path) of run_simulation.py:139-144: the ASCII PLY of
   one fluid object and frame (header as Taichi's python/taichi/tools/ply.py prints it, every value as str(np.float32) followed by a
   blank).  xyz: f32[n][3] in the scene's frame, e.g. what sph_download(SPH_F_POSITION) returned.  SPH_ERR_UNSUPPORTED: the file could
   not be written. */
int sph_write_ply_ascii(const char *path, const float *xyz, int64_t n);
/* the same file in parts (a sharded scene: every rank's owned particles, in rank order): first != 0 truncates the file and writes the
   header for n_total vertices, then this part's n rows; first == 0 appends n rows.  The parts of any split, concatenated, are byte for
   byte sph_write_ply_ascii of the concatenated array.  The caller keeps the parts in order (sph_comm_barrier between ranks). */
int sph_write_ply_ascii_part(const char *path, const float *xyz, int64_t n, int64_t n_total, int first);
/* str(np.float32(v)) -- the number format of that file -- into out (>= 48 bytes, no terminator); returns the length */
int sph_format_f32(float v, char *out);
/* the OBJ of one reconstructed surface (what splashsurf's `-o particle_object_{id}.obj` of surface_reconstruction.py:8 wrote): "v x y z"
   per vertex, "vn x y z" per normal (normals_or_NULL), then per triangle "f a//a b//b c//c" with 1-based indices ("f a b c" without
   normals); every number in sph_format_f32's format.  vertices / normals: f32[nv][3]; triangles: i32[nt][3] (0-based).
   SPH_ERR_UNSUPPORTED: the file could not be written. */
int sph_write_obj_ascii(const char *path, const float *vertices, int64_t nv, const float *normals_or_NULL, const int32_t *triangles,
                        int64_t nt);

/* --- surface reconstruction: fluid particles -> triangle mesh --------------- */
/* replaces `splashsurf reconstruct {ply} -o {obj} -r={radius} -l={smoothing_length} -c=0.5 -t=0.6 ... --normals=on` of
   surface_reconstruction.py:8 (run per frame and fluid object by surface_reconstruction.py:20-24).  Not splashsurf's algorithm: a
   Shepard colour field and marching cubes, defined here and in DESIGN.md 14 (no mesh cleanup; smoothing: see DESIGN.md 16 below):
     h = 2 smoothing_length radius (support of the project's cubic spline), V_j = 1 / sum_k W(x_j - x_k) over the input set,
     phi(x) = sum_j V_j W(x - x_j), surface phi = iso, inside phi > iso; grid points at integer multiples of e = cube_size radius from
     the origin; bricks of B^3 points, B = ceil(h / e), evaluated where a particle lies in the 3x3x3 coarse cells around them (phi = 0
     elsewhere); marching cubes with ambiguous faces resolved from their corners alone; a vertex per crossed grid edge (linear
     interpolation), shared by index; triangles counter-clockwise seen from outside; normals -grad phi / |grad phi| at the vertices.
   The mesh is a function of the particle SET (not of its order), bit for bit; vertices in (brick, point, axis) order, triangles in
   (brick, cube, case table) order.  One HIP stream per object; one host thread per object. */
typedef struct {
    double radius;           /* particle radius r (--radius; the scene's particleRadius) */
    double smoothing_length; /* -l, in multiples of r (3.5) */
    double cube_size;        /* -c, in multiples of r (0.5) */
    double iso;              /* -t, surface threshold (0.6) */
    int32_t normals;         /* --normals=on (1) */
    int32_t fast_math;       /* 0: IEEE div / sqrt, no FMA contraction; 1: the fast build */
    int32_t device;          /* HIP device ordinal, -1: current */
    int32_t reserved;        /* 0 */
    int64_t memory_cap_bytes;/* device bytes the object may hold at once (0: no cap); a frame that needs more fails with SPH_ERR_CAPACITY
                                before it allocates */
} SphSurfaceParams;

typedef struct {
    int64_t particles;        /* input particles of the last reconstruction */
    int64_t active_bricks;
    int64_t points_evaluated; /* active_bricks * B^3 */
    int64_t pair_tests;       /* (grid point, particle) candidates of the field pass: points x particles of their 27 coarse cells */
    int64_t vertices, triangles;
    int64_t bytes_allocated;  /* device bytes held by the object */
    int32_t B;                /* grid points per brick edge */
    int32_t reserved;
    double ms_bin;            /* HIP events: input, bounds, bin + key order + V_j */
    double ms_bricks;         /* active bricks */
    double ms_field;          /* phi (the hot pass) */
    double ms_mesh;           /* classify, count, scan, emit */
    double ms_normals;        /* -grad phi at the emitted vertices; ~0 when mesh smoothing is on (the normals are then taken at the
                                 smoothed positions, timed in SphSurfacePostStats.ms_normals) */
    double ms_total;          /* first event to last (host waits for the three counts included) */
} SphSurfaceStats;

typedef struct SphSurface SphSurface;
int sph_surface_create(const SphSurfaceParams *params, SphSurface **out);
void sph_surface_destroy(SphSurface *s);
const char *sph_surface_last_error(SphSurface *s);
/* host positions f32[n][3] (e.g. one frame's particle_object_{id}.ply, read by splashsurf from disk in the reference); synchronous */
int sph_surface_reconstruct(SphSurface *s, const float *xyz, int64_t n);
/* the particles of object_id (SPH_F_OBJECT_ID, ghosts excluded) of a live handle, compacted on the device with no host round trip
   (run_simulation.py:139-144 writes them to a PLY that surface_reconstruction.py then reads); the handle must be on the same device.
   SPH_ERR_UNSUPPORTED on a sharded handle (sph_comm_set_slab); synchronous. */
int sph_surface_reconstruct_object(SphSurface *s, SphHandle *h, int object_id);
int sph_surface_mesh_size(SphSurface *s, int64_t *n_vertices, int64_t *n_triangles);
/* vertices f32[nv][3], normals f32[nv][3] (NULL: skipped; SPH_ERR_INVALID when the object was created without normals),
   triangles i32[nt][3] */
int sph_surface_download(SphSurface *s, float *vertices, float *normals_or_NULL, int32_t *triangles);
int sph_surface_stats(SphSurface *s, SphSurfaceStats *out);

/* --- surface post-processing: smoothing of the reconstructed mesh ------------------------------------------------ */
/* replaces `--mesh-smoothing-weights=on --mesh-smoothing-iters=25 --normals=on --normals-smoothing-iters=10` of the splashsurf command in
   surface_reconstruction.py:8.  Not splashsurf's code: the method is defined here and in DESIGN.md 16.  Off by default (all zero); when
   mesh_smoothing_iters or normals_smoothing_iters is positive, every reconstruction that follows (both entry points above) runs, after
   the emit pass and inside the same synchronous call:
     N(i) = the vertices j != i that share a triangle with i, ascending, no duplicates;
     with mesh_smoothing_weights: c_j = sum over particles k != j with |x_j - x_k| < h of (1 - |x_j - x_k|^2 / h^2),
       w_i = min(1, max{c_j : |P_i - x_j| < h} / weights_normalization) (0 with no particle within h) at the unsmoothed positions;
       else w_i = 1;
     mesh_smoothing_iters Jacobi iterations P_i <- (1 - w_i) P_i + w_i (sum_{j in N(i), ascending} P_j) / |N(i)| (no neighbour: P_i stays);
     normals on and mesh_smoothing_iters > 0: the normals are taken at the smoothed positions (SphSurfaceStats.ms_normals is then ~0);
     normals_smoothing_iters iterations n_i <- s_i / |s_i|, s_i = n_i + sum_{j in N(i), ascending} n_j (|s_i| = 0: s_i stays).
   Triangles are not touched.  The mesh stays a function of the particle set, bit for bit.  New device buffers count under
   memory_cap_bytes (SPH_ERR_CAPACITY before they are allocated). */
typedef struct {
    int32_t mesh_smoothing_iters;    /* --mesh-smoothing-iters (reference: 25); 0: positions untouched */
    int32_t mesh_smoothing_weights;  /* --mesh-smoothing-weights=on (1) */
    double weights_normalization;    /* --mesh-smoothing-weights-normalization (13) */
    int32_t normals_smoothing_iters; /* --normals-smoothing-iters (reference: 10); needs an object created with normals */
    int32_t reserved;                /* 0 */
} SphSurfacePostParams;

typedef struct {
    int64_t adjacency_entries;  /* sum of |N(i)| of the last reconstruction */
    int32_t max_degree;         /* max |N(i)| */
    int32_t reserved;
    double ms_adjacency;        /* HIP events: slots, sort, scans, compaction (host read of the total included) */
    double ms_weights;
    double ms_smoothing;        /* all mesh_smoothing_iters iterations, float4 copies included */
    double ms_normals;          /* -grad phi at the smoothed positions */
    double ms_normal_smoothing;
    double ms_total;
} SphSurfacePostStats;

/* applies to the reconstructions that follow.  SPH_ERR_INVALID: a negative iteration count, a normalization that is not positive and
   finite (in f32 too), normal smoothing on an object created without normals. */
int sph_surface_set_postprocess(SphSurface *s, const SphSurfacePostParams *params);
/* zeros when the last reconstruction ran no post-processing */
int sph_surface_post_stats(SphSurface *s, SphSurfacePostStats *out);
/* the last reconstruction's N(i) as CSR, offsets i32[nv + 1], neighbours i32[offsets[nv]], and w_i f32[nv] (all 1 without
   mesh_smoothing_weights or with mesh_smoothing_iters = 0); any may be NULL.  SPH_ERR_INVALID when that reconstruction ran no
   post-processing. */
int sph_surface_download_post(SphSurface *s, int32_t *offsets, int32_t *neighbours, float *weights);

/* --- surface reconstruction with anisotropic kernels ----------------------------------------------------------------- */
/* Opt-in; off by default, and with the mode off every kernel launched and every byte written is what it is without this section.  The
   isotropic kernel's support h = 7 r meshes a one-particle sheet 4.2 r thick; here every particle gets a kernel shrunk along the
   directions in which its neighbourhood is thin (after Yu & Turk 2013, without their position smoothing: centres are not moved).  The
   project's own definition, with h, W, e, bricks, marching cubes and every order of section 14; for every input particle i:
     N_i = the number of k != i with |x_k - x_i| < h;  w_ik = 1 - (|x_k - x_i| / h)^3 over the same set, self included (w = 1);
     mean_i = sum w_ik x_k / sum w_ik;  C_i = sum w_ik (x_k - mean_i)(x_k - mean_i)^T / sum w_ik (accumulated relative to x_i);
     C_i = sum_k lambda_k v_k v_k^T, lambda_1 the largest (a fixed number of cyclic Jacobi sweeps in f32);
     N_i < min_neighbours or lambda_1 <= 0:  A_i = I / sparse_scale (the isolated rule);
     else a_k = 1 / max(lambda_k / lambda_1, 1 / max_ratio), A_i = sum a_k v_k v_k^T: symmetric, every a_k in [1, max_ratio], so
       kernels only shrink and kernel i vanishes outside the ball of radius h around x_i;
     w_j(x) = det(A_j) W(|A_j (x - x_j)|);  V_j = 1 / sum_k w_k(x_j);  phi(x) = sum_j V_j w_j(x);  normals -grad phi / |grad phi| with
       grad w_j = det(A_j) W'(|y|) / |y| A_j y, y = A_j (x - x_j).
   A = I everywhere gives section 14's V_j bit for bit.  The mesh stays a function of the particle set, bit for bit, in both builds; no
   float atomics.  New device buffers (36 bytes per particle) count under memory_cap_bytes (SPH_ERR_CAPACITY before they are
   allocated).  The smoothing of DESIGN.md 16 runs on the anisotropic mesh unchanged (its normals from the anisotropic field). */
typedef struct {
    int32_t enabled;         /* 0: off */
    int32_t min_neighbours;  /* below this N_i the isolated rule applies (25) */
    double max_ratio;        /* the largest a_k: >= 1 (2) */
    double sparse_scale;     /* the isolated rule's support in multiples of h: in (0, 1] (0.5) */
} SphSurfaceAnisoParams;

typedef struct {
    int64_t sparse_particles;   /* particles under the isolated rule in the last reconstruction */
    int64_t clamped_particles;  /* the others with at least one lambda_k / lambda_1 below 1 / max_ratio */
    double ms_moments;          /* HIP events: N_i, covariance, eigen-decomposition and clamp */
    double ms_volume;           /* V_j.  Both lie inside SphSurfaceStats.ms_bin; the anisotropic field is timed in ms_field */
} SphSurfaceAnisoStats;

/* applies from the next reconstruction on, through both entry points; NULL or enabled == 0 switches the mode off.  SPH_ERR_INVALID: a
   negative min_neighbours, a max_ratio below 1 or not finite (in f32 too), a sparse_scale outside (0, 1] or with 1 / scale not finite in
   f32 */
int sph_surface_set_anisotropy(SphSurface *s, const SphSurfaceAnisoParams *params_or_NULL);
/* zeros after a reconstruction without the mode */
int sph_surface_anisotropy_stats(SphSurface *s, SphSurfaceAnisoStats *out);
/* the last reconstruction's particles in the binned key order: xyz f32[n][3], A6 f32[n][6] = (xx, xy, xz, yy, yz, zz) of A_i,
   neighbours i32[n] = N_i, V f32[n]; n = SphSurfaceStats.particles; any may be NULL.  SPH_ERR_INVALID when that reconstruction ran
   without the mode. */
int sph_surface_download_anisotropy(SphSurface *s, float *xyz, float *A6, int32_t *neighbours, float *V);
/* the device's eigen and clamp routine, compiled from the same source, run on the host (no GPU involved): A6[i] from the covariance
   C6[i] (same six-entry layout) and neighbours[i] (NULL: every particle has enough); p->enabled is ignored.  SPH_ERR_INVALID as the
   setter. */
int sph_surface_aniso_matrix_host(const float *C6, int64_t n, const int32_t *neighbours, const SphSurfaceAnisoParams *p, float *A6);

/* --- particle rendering: particles -> one RGB frame ------------------------------------------------------------- */
/* replaces the GGUI frame of run_simulation.py:116-135 (scene.particles(x_vis_buffer, radius=dx, per_vertex_color=...), scene.lines of
   the domain box, scene.point_light, window.save_image -> raw_view.png).  Not GGUI's shaders: the image is defined here and in
   DESIGN.md 15.  Camera: f = normalize(target - eye), s = normalize(f x up), u = s x f; pixel column i (from the left), row j (from the
   top) looks along d = f + (2(i+.5)/W - 1) tan(fov/2) W/H s + (1 - 2(j+.5)/H) tan(fov/2) u (f.d = 1).  A sphere (centre c, radius r)
   covers the pixel where disc = b^2 - (d.d)(|c-E|^2 - r^2) >= 0, b = d.(c-E), and t = (b - sqrt(disc)) / (d.d) > z_near; the pixel's
   winner has the smallest (float_bits(t) << 32 | id) -- the image is a function of the particle SET.  Colour: col/255 (ambient +
   max(n.L, 0) light_rgb), clamped, floor(255 x + 0.5); P = E + t d, n = (P - c)/r, L = normalize(light - P).  Box: the 12 edges of
   [box_lo, box_hi], one pixel wide, unshaded, depth-tested with ids 0xFFFFFFF0 + edge: clipped at z_near, one pixel per step along the
   screen major axis, the nearest pixel on the minor axis, 1/z linear on the screen.  One HIP stream per object; synchronous calls. */
typedef struct {
    int32_t width, height;   /* pixels (1024 x 1024 in the reference); each 1..16384, width * height <= 2^26 */
    double eye[3];           /* camera position (5.5, 2.5, 4.0) */
    double target[3];        /* look-at (-1, 0, 0) */
    double up[3];            /* (0, 1, 0) */
    double fov_deg;          /* vertical field of view, (0, 180) (70) */
    double z_near;           /* > 0 (0.1) */
    double radius;           /* sphere radius, > 0 (the container's dx) */
    double light_pos[3];     /* point light (2, 2, 2) */
    double light_rgb[3];     /* (1, 1, 1) */
    double ambient;          /* >= 0 (0.1, our choice) */
    int32_t background_rgb[3]; /* 0..255 each (0, 0, 0) */
    int32_t draw_box;        /* 1: the 12 edges of [box_lo, box_hi] */
    double box_lo[3], box_hi[3];
    int32_t box_rgb[3];      /* 0..255 each ((0.99, 0.68, 0.28) -> (252, 173, 71)) */
    int32_t fast_math;       /* 0: IEEE div / sqrt, no FMA contraction; 1: the fast build */
    int32_t device;          /* HIP device ordinal, -1: current */
    int32_t reserved;        /* 0 */
} SphRenderParams;

typedef struct {
    int64_t particles;        /* particles given (points) / slots of the handle (handle) */
    int64_t drawn;            /* taken (object mask, no ghost or dead slot), finite and not culled */
    int64_t skipped_nonfinite;/* taken but with a non-finite coordinate: not drawn */
    int64_t large;            /* drawn spheres whose screen bounds exceed 4096 pixels (one workgroup each) */
    int64_t atomics;          /* 64-bit atomicMin issued by the sphere splat (after the plain load said the key would drop) */
    int64_t covered_pixels;   /* pixels won by a sphere */
    double ms_input;          /* HIP events: upload (points) / colour source (handle), clear of the depth keys */
    double ms_splat;          /* spheres (small, large) and box lines */
    double ms_shade;          /* the winners' colours, background and id image */
    double ms_total;
} SphRenderStats;

typedef struct SphRender SphRender;
int sph_render_create(const SphRenderParams *params, SphRender **out);
void sph_render_destroy(SphRender *r);
const char *sph_render_last_error(SphRender *r);
/* host particles: xyz f32[n][3], rgb_or_NULL u8[n][3] (NULL: white), ids_or_NULL u32[n] (distinct, < 0xFFFFFFF0; NULL: 0 .. n-1) */
int sph_render_points(SphRender *r, const float *xyz, const uint8_t *rgb_or_NULL, const uint32_t *ids_or_NULL, int64_t n);
/* the particles of a live handle whose object id has its bit set in object_mask (ghosts and dead slots never), each with its persistent
   id (SPH_F_PARTICLE_ID) and its colour as sph_download(SPH_F_COLOR) gives it; the handle's state is left untouched.  The handle must
   be on the same device and not between sph_step_begin and sph_step_end.
   A sharded handle (sph_comm_set_slab) makes the call COLLECTIVE over the handle's communicator: every rank calls it with
   the same renderer parameters and the same mask; each settles its asynchronous steps, draws its own particles, and the layers are
   merged down the rank chain (rank nranks-1 -> ... -> 0, neighbour transport, bounded waits: a lost rank ends in SPH_ERR_COMM).  Rank 0
   then holds the frame -- bit for bit the unsharded renderer's, persistent ids being global -- for sph_render_download and the
   encoders; on the other ranks sph_render_download is SPH_ERR_INVALID.  SPH_ERR_UNSUPPORTED: a handle whose library frame is permuted
   (SPH_SLAB_LAYOUT=slow). */
int sph_render_handle(SphRender *r, SphHandle *h, uint32_t object_mask);
/* the last frame: rgb u8[height][width][3] (rows from the top), ids_or_NULL i32[height][width]: the winner's id, -1 background,
   -2 - edge a box line */
int sph_render_download(SphRender *r, uint8_t *rgb, int32_t *ids_or_NULL);
int sph_render_stats(SphRender *r, SphRenderStats *out);

/* layers: what a particle frame holds per pixel -- the u64 key (float_bits(t) << 32 | id; ~0 where nothing was drawn) and
   the rgb.  Renderers with the same parameters that drew disjoint particle sets with distinct ids compose: per pixel the smaller key
   wins, and the result is the frame of the union.  key u64[height][width], rgb u8[height][width][3].
   _download: the layer of the last particle frame.  _merge: upload a layer, fold it into the current frame, then background, id image
   and covered_pixels again (sph_render_download / the encoders see the merged frame).  SPH_ERR_INVALID: no frame, or a mesh frame. */
int sph_render_layer_download(SphRender *r, uint64_t *key, uint8_t *rgb);
int sph_render_layer_merge(SphRender *r, const uint64_t *key, const uint8_t *rgb);

typedef struct {
    int32_t ranks;            /* ranks of the communicator the last sph_render_handle frame was composited over (1: not sharded) */
    int32_t hops;             /* hops of the chain this rank sent or received in */
    int64_t pieces_sent, pieces_recv;   /* messages (each at most the transport's message capacity) */
    int64_t bytes_sent, bytes_recv;
    int64_t drawn_global;     /* SphRenderStats.drawn summed over the ranks */
    double ms_composite;      /* HIP events: from this rank's first send or receive to the end of its last merge (or send) */
} SphRenderCompositeStats;
int sph_render_composite_stats(SphRender *r, SphRenderCompositeStats *out);

/* --- screen-space surface mode: a particle frame -> a smoothed, lit liquid surface --------------------------------- */
/* opt-in second stage of a particle frame, as real-time fluid renderers draw liquids without a mesh.  Surface pixels: those whose
   winner is a particle of a surface object (handle path: object_mask; points path: the per-point flag).  Depth stage, all integers:
   q = min((u32)(t * inv_u), 2^24 - 1) with u = radius / 256 and inv_u = 256 / radius rounded to f32 once; `iterations` Jacobi steps
   q_i' = (sum w q_j + (sum w >> 1)) / sum w over the taps (dx, dy) of the window |dx|, |dy| <= R_i that lie in the frame, are surface
   pixels and have |q_j - q_i| <= dq; R_i = clamp(Rnum / q_i, 1, rmax) (rmax where q_i = 0), w = (R_i + 1 - |dx|)(R_i + 1 - |dy|),
   Rnum = round(256 sigma H / (2 tan(fov / 2))), dq = round(256 range).  Colour stage (f32, contraction off: the same bytes in both
   builds): P = q u (X, Y, 1); per screen axis the one-sided difference towards the surface neighbour with the smaller |dq| (a tie: the
   + side; none: no difference, and the normal is the direction to the eye); n = normalised cross product turned to the eye;
   base (ambient + max(n.L, 0) light_rgb) + spec light_rgb max(n.h, 0)^shininess, h the half vector of the directions to the light and
   to the eye; clamped, floor(255 x + 0.5).  Every other pixel keeps the bytes of the particle frame.  While the mode is on,
   sph_render_points / _handle also fill the base plane (colour and flag per pixel); sph_render_surface then needs no particle.
   Thickness and absorption: sph_render_set_thickness below.
   Not done: refraction, Fresnel, the narrow-range filter's one-sided clamp, anti-aliasing, sharded frames. */
typedef struct {
    int32_t iterations;       /* 0..64 (3) */
    int32_t rmax;             /* largest window half-width in pixels, 1..16 (12) */
    double sigma;             /* smoothing half-width in particle radii, > 0 (1.5); Rnum must stay below 2^31 */
    double range;             /* depth range of a tap in particle radii, > 0 (2.0); dq in 1..2^24 */
    double spec;              /* >= 0 (0.35) */
    double shininess;         /* >= 1 (40) */
    int64_t object_mask;      /* handle path: bit o = object o is a surface object; -1: the fluid particles of every drawn object */
} SphRenderSurfaceParams;

typedef struct {
    int64_t surface_pixels;
    int64_t iterations;       /* smoothing iterations run */
    int64_t taps_visited;     /* (2 R_i + 1)^2 summed over surface pixels and iterations */
    int64_t taps_accepted;    /* of these: in the frame, a surface pixel, within dq */
    int64_t clamped_rmax;     /* surface pixels whose Rnum / q exceeded rmax in the first iteration */
    double ms_base;           /* HIP events: the base plane (part of the frame call) */
    double ms_smooth;         /* quantise and every iteration */
    double ms_shade;
} SphRenderSurfaceStats;

#define SPH_RENDER_SURFACE_SENTINEL 0xFFFFFFFFu   /* sph_render_surface_download_depth: not a surface pixel */

/* switches the mode on (params) or off (NULL); applies to the frames drawn afterwards.  SPH_ERR_INVALID, with a message that names the
   field: iterations outside 0..64, rmax outside 1..16, sigma / range not finite and positive (or too large, see above), spec negative
   or not finite, shininess below 1 or not finite, object_mask below -1 or above 2^32 - 1. */
int sph_render_set_surface(SphRender *r, const SphRenderSurfaceParams *params_or_NULL);
/* the per-point surface flag (u8[n], non-zero = surface) of the NEXT sph_render_points, whose n must equal this n; NULL: every point
   (the default, restored after that call) */
int sph_render_points_surface_mask(SphRender *r, const uint8_t *mask_or_NULL, int n);
/* runs quantise, smooth and shade on the frame last drawn by sph_render_points / _handle and overwrites its rgb in place
   (sph_render_download, sph_video_encode_render and sph_png_encode_render then see the surface frame; key plane and id image are
   untouched); synchronous.  SPH_ERR_INVALID: no particle frame held, a mesh frame, the mode off (or switched on after the frame was
   drawn), a frame changed by sph_render_layer_merge.  SPH_ERR_UNSUPPORTED: the frame was composited from a sharded handle. */
int sph_render_surface(SphRender *r);
/* the final integer depth plane of the last sph_render_surface: q u32[height][width], SPH_RENDER_SURFACE_SENTINEL elsewhere */
int sph_render_surface_download_depth(SphRender *r, uint32_t *q);
int sph_render_surface_stats(SphRender *r, SphRenderSurfaceStats *out);

/* --- thickness mode of the surface frames: what lies behind the fluid shows through -------------------------------- */
/* opt-in on top of the surface mode.  While it is on, sph_render_points / _handle also draw (1) the opaque layer: the frame the ordinary
   renderer would draw from the particles that are not surface particles plus the box lines, as a key plane (float_bits(t) << 32 | id,
   all ones where nothing won) with its rgb; (2) the thickness plane: every surface sphere, per pixel centre of its bounds, with the ray's
   chord [t0, t1] = k -+ sqrt(h / dd) (the quantities of the hit test, evaluated without contraction: the same bits in both builds),
   counted when h >= 0 and t0 > z_near, its far end b = min(t1, t_opaque), adds (u32)((b - t0) * inv_u) when b > t0 -- at most 512, summed
   in u32 with integer atomics, so the plane is a function of the particle set.  sph_render_surface then smooths it (`iterations` Jacobi
   steps, the depth stage's integer tent with R_i from the final smoothed depth, every surface pixel of the window a tap, no range test)
   and composites per surface pixel and channel, in f32 without contraction:
     Tr = max(T, 1) / 256,  tau = (absorb (1 - base / 255) + scatter) Tr,  a = exp2(-tau),
     out = byte((behind a + lit (1 - a)) + highlight),  behind = opaque rgb / 255,  lit and highlight the two terms of the surface mode.
   absorb = scatter = 0 and spec = 0: the opaque layer's bytes; a very large scatter: the bytes of the surface mode without thickness.
   A frame of more than 2^23 particles is refused while the mode is on (SPH_ERR_UNSUPPORTED, before any launch). */
typedef struct {
    float absorb;             /* per particle radius of fluid, scaled by 1 - base colour: what the fluid's colour takes away, >= 0 (0.05) */
    float scatter;            /* per particle radius of fluid, every channel alike, >= 0 (0.01) */
    int32_t iterations;       /* smoothing iterations of the thickness plane, 0..64 (2) */
} SphRenderThicknessParams;

typedef struct {
    int64_t adds;             /* (sphere, pixel) pairs that added to the plane: one integer atomic each */
    int64_t clipped;          /* of these: cut short by the opaque depth */
    int64_t removed;          /* pairs that hit but lay wholly behind the opaque depth (no atomic) */
    int64_t empty_pixels;     /* surface pixels whose summed thickness is 0 (they are composited with T = 1) */
    int64_t max_thickness;    /* the largest smoothed T */
    int64_t iterations;       /* smoothing iterations run */
    int64_t taps_visited;     /* (2 R_i + 1)^2 summed over surface pixels and iterations */
    double ms_opaque;         /* HIP events: the opaque layer and ... */
    double ms_splat;          /* ... the thickness splat (parts of the frame call) */
    double ms_smooth;         /* the thickness smoothing and ... */
    double ms_shade;          /* ... the composite (parts of sph_render_surface, within its ms_shade) */
} SphRenderThicknessStats;

/* switches the mode on (params) or off (NULL); applies to the frames drawn afterwards.  SPH_ERR_INVALID, with a message that names the
   field: absorb / scatter negative or not finite, iterations outside 0..64; also when the surface mode is off.  Switching the surface
   mode off switches this off too.  While it is on, sph_render_surface refuses a frame drawn before it was switched on. */
int sph_render_set_thickness(SphRender *r, const SphRenderThicknessParams *params_or_NULL);
/* of the last sph_render_surface: the smoothed plane T u32[height][width] in units of radius / 256 of view depth, 0 on non-surface
   pixels; raw != 0: the plane as the splat summed it */
int sph_render_surface_download_thickness(SphRender *r, uint32_t *T, int raw);
/* the opaque layer of the last particle frame, as sph_render_layer_download gives the frame's */
int sph_render_surface_download_opaque(SphRender *r, uint64_t *key, uint8_t *rgb);
int sph_render_thickness_stats(SphRender *r, SphRenderThicknessStats *out);

/* --- mesh rendering: an ordered list of triangle meshes -> one RGB frame ------------------------------------------ */
/* stands in for the reference's render.py + rendering_script.py (every .obj of a frame directory through a Blender scene ->
   {frame}/render.png).  Not Blender's path tracer: Lambert-shaded triangles, the camera, light, ambient, background, box lines and 8-bit
   rounding of the particle image above, one colour per mesh.  A frame: sph_render_mesh_begin, one sph_render_mesh_add /
   _add_surface per mesh, sph_render_mesh_end (draws; synchronous), then sph_render_download.  Triangles are numbered globally in list
   order (mesh 0's first); their total stays below 0xFFFFFFF0, the vertices' below 2^31.
   Hit of pixel ray d (f.d = 1) on triangle A B C, a = A - E, b = B - E, c = C - E: the edge functions d.(b x c), d.(c x a), d.(a x b) are
   all >= 0 or all <= 0 (no back-face culling), N = (B - A) x (C - A) is finite and non-zero, and t = (a.N) / (d.N) is finite and
   > z_near.  Each edge function is evaluated from the edge's two vertices in one canonical order, so the two triangles of a shared edge
   get the same bits for it (in both builds): no pixel centre falls between them.  Winner: the smallest (float_bits(t) << 32 | global
   triangle index); box lines take part with their keys as above.  Colour at P = E + t d: n = N / |N| for a mesh without normals, else the
   normalised blend of the three vertex normals weighted by the edge functions (the flat normal when the blend is zero or non-finite);
   n = -n if n.d > 0 (two-sided); col/255 (ambient + max(n.L, 0) light_rgb), clamped, floor(255 x + 0.5).  Skipped and counted: triangles
   with a non-finite vertex, with N = 0, or with an index outside [0, nv) -- the last makes sph_render_mesh_end return SPH_ERR_INVALID
   after the frame is drawn (nothing is read out of bounds; the frame can be downloaded).  SphRenderParams.radius is unused.
   sph_render_points / _handle are unchanged: a particle frame and a mesh frame are separate frames of one renderer. */
typedef struct {
    int64_t meshes, triangles, vertices;  /* of the list */
    int64_t large;              /* triangles whose screen bounds exceed 4096 pixels (one workgroup each) */
    int64_t skipped_nonfinite;  /* a non-finite vertex (or plane): not drawn */
    int64_t skipped_degenerate; /* N = 0: not drawn */
    int64_t bad_index;          /* an index outside [0, nv): not drawn, SPH_ERR_INVALID from sph_render_mesh_end */
    int64_t atomics;            /* 64-bit atomicMin issued by the depth pass (after the plain load said the key would drop) */
    int64_t covered_pixels;     /* pixels won by a triangle */
    int64_t hit;                /* triangles that passed the hit test at one pixel centre at least */
    double ms_depth;            /* HIP events: triangles (small, large) and box lines */
    double ms_shade;            /* the winners' colours */
    double ms_finish;           /* background and id image */
    double ms_total;            /* mesh table upload and clear of the keys included */
} SphRenderMeshStats;

/* SPH_ERR_INVALID: add / end without begin, negative counts, NULL arrays with non-zero counts, NULL rgb, too many triangles or vertices */
int sph_render_mesh_begin(SphRender *r);
/* host arrays: vertices f32[nv][3], normals_or_NULL f32[nv][3] (NULL: flat shading), triangles i32[nt][3] (0-based, local to this mesh) */
int sph_render_mesh_add(SphRender *r, const float *vertices, const float *normals_or_NULL, const int32_t *triangles, int64_t nv, int64_t nt,
                        const uint8_t rgb[3]);
/* the last mesh of a surface object (post-processed positions and normals when that stage is on), copied device to device; the
   surface object is left untouched and must be on the renderer's device */
int sph_render_mesh_add_surface(SphRender *r, SphSurface *s, const uint8_t rgb[3]);
/* draws the list; then sph_render_download: the id image holds the global triangle index (exact below 2^31 triangles), -1 background,
   -2 - edge a box line */
int sph_render_mesh_end(SphRender *r);
int sph_render_mesh_stats(SphRender *r, SphRenderMeshStats *out);

/* --- traced mesh frames: shadows and refracting water --------------------------------------------------------------- */
/* An opt-in mode of the mesh frames above: while it is on, sph_render_mesh_end traces the list instead of rasterising it -- a bounding
   volume hierarchy over the frame's triangles is built on the device (Morton codes of the centroids, radix sort, Karras 2012, boxes
   fitted bottom-up) and one Whitted-style path per pixel is followed through it: hard shadows from the point light, water meshes as a
   dielectric (Snell refraction, Schlick's Fresnel term with one reflection segment that is followed no further, Beer-Lambert absorption
   tinted by the mesh's colour), and the bottom face of the box as a checkered floor that takes the shadows.  Camera, pixel rays, near
   plane, light, ambient, background, box lines and 8-bit rounding are those of the mesh frames; without the mode every frame is what it
   was.  Deterministic: no random numbers, no float atomics; the winner of a ray is the smallest (float_bits(t) << 32 | global triangle
   index), so the image is a function of the mesh list.  A ray never hits the triangle it starts on (by index).  The id image holds the
   primary hit: a triangle index, SPH_RENDER_TRACE_FLOOR_ID for the floor, the line ids, -1.
   Not done: soft shadows, caustics (water does not block light), further reflection bounces, an environment map, anti-aliasing, sharded
   handles, particles in the same frame. */
#define SPH_RENDER_MATERIAL_DIFFUSE 0
#define SPH_RENDER_MATERIAL_WATER 1
#define SPH_RENDER_TRACE_FLOOR_ID (-14)
#define SPH_RENDER_TRACE_SEGMENT_WORDS 24
typedef struct {
    int32_t max_depth;          /* 1..64 segments of a path; a path cut there adds the background times its throughput */
    float ior;                  /* >= 1, the fluid's index of refraction */
    float absorb;               /* >= 0: a segment of length l in the fluid multiplies the throughput per channel by
                                   exp2(-absorb (1 - rgb / 255) l / radius), rgb the colour of the water mesh it entered */
    int32_t shadows;            /* 0 / 1: shadow rays towards the light */
    int32_t floor;              /* 0 / 1: the bottom face of the box (if the renderer draws one) as a diffuse checkered rectangle */
    float floor_cell;           /* > 0, the checker's cell in units of radius */
    int32_t use_bvh;            /* 0: every ray tests every triangle with the same routines (the check of the culling) */
    int32_t record;             /* 1: the segments of every path are kept for sph_render_trace_download_paths */
} SphRenderTraceParams;

typedef struct {
    int64_t triangles;          /* kept: leaves of the hierarchy */
    int64_t nodes;              /* 2 triangles - 1 */
    int64_t depth;              /* inner nodes above the deepest leaf (at most 64: the sort keys are distinct) */
    int64_t skipped_nonfinite, skipped_degenerate, bad_index;   /* left out, as the mesh frames count them */
    int64_t rays_primary, rays_path, rays_reflect, rays_shadow; /* pixels; refracted or totally reflected segments; reflection segments;
                                                                   shadow rays */
    int64_t node_visits, triangle_tests;
    int64_t truncated;          /* paths cut at max_depth */
    int64_t aborted_rays;       /* rays that reached the visit cap of 2 nt nodes (a miss; 0 unless the hierarchy is broken) */
    double ms_setup, ms_sort, ms_hierarchy, ms_fit, ms_trace, ms_finish, ms_total;   /* HIP events */
} SphRenderTraceStats;

/* the mode for the mesh frames that follow; NULL: off, and what it allocated is freed.  SPH_ERR_INVALID: a parameter outside its
   range, between mesh_begin and mesh_end; SPH_ERR_UNSUPPORTED: the renderer composites the layers of a sharded handle */
int sph_render_set_trace(SphRender *r, const SphRenderTraceParams *params_or_NULL);
/* the material of the mesh added last (between its _add and _end; default diffuse); flip = 1: the mesh is wound inwards.  Read by the
   traced frames only */
int sph_render_mesh_material(SphRender *r, int material, int flip);
/* of the traced frame held; SPH_ERR_INVALID while the mode is off or the frame held is not a traced one */
int sph_render_trace_stats(SphRender *r, SphRenderTraceStats *out);
/* the hierarchy of the traced frame held, n = triangles: left / right i32[n - 1] (node ids: inner node i is i, the leaf of sorted
   position j is n - 1 + j, the root is 0), boxes f32[2 n - 1][6] (lo xyz, hi xyz per node id), leaf_triangle i32[n] (the global
   triangle index of leaf j); each may be NULL */
int sph_render_trace_download_bvh(SphRender *r, int32_t *left, int32_t *right, float *boxes, int32_t *leaf_triangle);
/* the segments of a frame traced with record = 1: f32[height][width][max_depth][24].  Words: 0-2 origin, 3-5 direction, 6 hit id (i32:
   a triangle, the floor id, -1), 7 t, 8-10 the unit normal used (shading or refraction), 11-13 throughput at the start, 14-16
   throughput handed on (0: the path ends), 17-19 what the segment added to the pixel (its reflection included), 20 shadow ray of the
   hit (i32: -1 none, 0 lit, 1 blocked), 21 the reflection segment's hit id (i32, -1 none or a miss), 22 F, 23 flags (i32: 1 used,
   2 entering, 4 total internal reflection, 8 the segment ran inside the fluid, 16 the reflection's hit was in shadow) */
int sph_render_trace_download_paths(SphRender *r, float *segments);

/* --- video encoding: RGB frames -> baseline JPEG streams, the frames of a Motion-JPEG AVI ------------------------- */
/* stands in for the reference's make_video.py (imageio): every frame is compressed on the device it was rendered on; the AVI
   container around the frames is written on the host (sph_project_amd/video.py).  One frame is one complete .jpg file: baseline
   sequential DCT (SOF0), 8 bit, three components, JFIF header, full-range BT.601 YCbCr, chroma 4:2:0 or 4:4:4, the quantisation
   tables of T.81 Annex K scaled by `quality` with the IJG rule, the Annex K Huffman tables, a restart interval of 8 MCUs (DRI; the
   intervals are what the device codes in parallel).  A picture whose size is no multiple of the MCU is padded by repeating its last
   column and row.  The pixel-to-coefficient arithmetic is integer fixed point, so the bytes are a function of (pixels,
   width, height, quality, chroma): the same from both builds and from every call.  The device does colour conversion, DCT,
   quantisation, zigzag, run/size symbols, DC prediction, Huffman coding, bit packing, 0xFF stuffing and the restart markers; the host
   writes the fixed headers and EOI.  The output is sized from a counting pass: a stream is never truncated.  One HIP stream per
   object; synchronous calls.
   Two things beyond the minimum: `fast_math` selects the strict or the fast build's launchers as it does in the surface and render
   objects (the bytes do not depend on it; it is how one process reaches both builds to show that), and sph_video_header gives the
   fixed headers without a device, so that the tables and segment layout can be checked against the standard on a host that has
   no GPU (tests/test_video_host.py does) and a muxer can know the header length before the first frame. */
typedef struct {
    int32_t width, height;   /* pixels; each 1..16384, width * height <= 2^26 */
    int32_t quality;         /* 1..100 */
    int32_t chroma;          /* 420 or 444 */
    int32_t fast_math;       /* which build's launchers run (0 strict, 1 fast); the bytes are the same */
    int32_t device;          /* HIP device ordinal, -1: current */
    int32_t reserved;        /* 0 */
} SphVideoParams;

typedef struct {
    int64_t blocks;            /* 8 x 8 blocks coded (padding included) */
    int64_t scan_bytes;        /* entropy-coded bytes between SOS and EOI: stuffed zeros and restart markers included */
    int64_t stuffed_bytes;     /* zeros stuffed behind 0xFF bytes */
    int64_t restart_intervals;
    double ms_input;           /* HIP events: upload of a host image (~0 for a renderer's frame) */
    double ms_count;           /* first pass: bytes per restart interval */
    double ms_scan;            /* their scan, the total read by the host */
    double ms_write;           /* second pass: the bytes */
    double ms_total;
} SphVideoStats;

typedef struct SphVideo SphVideo;
/* SPH_ERR_INVALID (before any device is touched): a size, quality or chroma outside the ranges above, reserved != 0 */
int sph_video_create(const SphVideoParams *params, SphVideo **out);
void sph_video_destroy(SphVideo *v);
const char *sph_video_last_error(SphVideo *v);
/* the fixed headers (SOI ... SOS) of every stream of these parameters: *bytes their length, dst_or_NULL filled when given.  Host only. */
int sph_video_header(const SphVideoParams *params, uint8_t *dst_or_NULL, int64_t *bytes);
/* a host image u8[height][width][3], rows from the top */
int sph_video_encode_rgb(SphVideo *v, const uint8_t *rgb);
/* the renderer's last frame (particles or meshes), read from its device buffer: not downloaded, nothing of the renderer modified.
   SPH_ERR_INVALID with a message: no frame rendered yet, a frame of another size, a renderer on another device. */
int sph_video_encode_render(SphVideo *v, SphRender *r);
/* the last encoded frame: the length of the complete .jpg file, and the file (headers, scan, EOI) */
int sph_video_size(SphVideo *v, int64_t *bytes);
int sph_video_download(SphVideo *v, uint8_t *dst);
int sph_video_stats(SphVideo *v, SphVideoStats *out);

/* --- PNG encoding: RGB frames -> lossless .png files, the frames an exporting run stores -------------------------- */
/* stands in for the host's zlib pass over a downloaded frame: the file is made on the device the frame was rendered on.  One frame is
   one complete .png file: 8-bit RGB (colour type 2), not interlaced; signature, IHDR, one IDAT chunk per segment of 4096 filtered
   bytes, one IDAT chunk with the Adler-32, IEND.  The IDAT payloads are one zlib stream (header 78 01): per segment either one block
   in the fixed Huffman code, closed by an empty stored block that brings the next segment to a byte boundary, or one stored block,
   whichever is shorter (ties: fixed).  With sph_png_set_coding(SPH_PNG_CODING_DYNAMIC) a segment becomes a dynamic Huffman block
   (BTYPE 10, closed like a fixed one) where that takes strictly fewer bytes than the choice above: lit/len lengths are Huffman's over
   the segment's own tokens, the distance and code-length codes' come from package-merge (limits 4 and 7), all codes canonical, the
   header run-length coded by a fixed greedy rule; a file in dynamic coding is never longer than the fixed one.  With
   SPH_PNG_CODING_WINDOW every position also has one match candidate in the 32 KB before it -- the most recent earlier occurrence of
   its three bytes anywhere in the filtered stream, other segments included -- and a segment becomes one dynamic block of that parse
   (all 30 distance symbols, distance code by package-merge under 15) where that takes strictly fewer bytes than the dynamic coding's
   choice; a file in window coding is never longer than the dynamic one.  Tokens come from a fixed rule (candidate distances 1, 2, 3, 4, 6 inside the segment, longest
   match first, then the smallest distance, greedy from the segment's start), row filters from the least sum of |residual as int8|
   (ties: the lowest type) or one fixed type.  All of it is integer arithmetic, so the bytes are a function of (pixels, width, height,
   filter, coding): the same from both builds and from every call.  The device filters, matches, parses, codes, packs and computes the
   Adler-32 and every IDAT chunk's CRC-32, and writes the IDAT chunks whole; the host writes the signature, IHDR and IEND and never
   reads the payload.  The output is sized from a counting pass: a file is never truncated, and never longer than sph_png_bound.
   One HIP stream per object; synchronous calls.  `fast_math` selects the build whose launchers run, as in the video object. */
typedef struct {
    int32_t width, height;   /* pixels; each 1..16384, width * height <= 2^26 */
    int32_t filter;          /* -1: adaptive (per row), 0..4: that PNG filter type on every row */
    int32_t fast_math;       /* which build's launchers run (0 strict, 1 fast); the bytes are the same */
    int32_t device;          /* HIP device ordinal, -1: current */
    int32_t reserved;        /* 0 */
} SphPngParams;

typedef struct {
    int64_t raw_bytes;         /* the filtered stream: height * (1 + 3 * width) */
    int64_t zlib_bytes;        /* the zlib stream: header, blocks, Adler-32 */
    int64_t file_bytes;        /* the .png file */
    int64_t segments;
    int64_t stored_segments;   /* segments written as a stored block because every code would have been longer */
    int64_t literals;          /* tokens of the segments written in the fixed code or in a dynamic code */
    int64_t matches;
    int64_t filter_rows[5];    /* rows per filter type */
    double ms_input;           /* HIP events: upload of a host image (~0 for a renderer's frame) */
    double ms_filter;          /* row filters */
    double ms_count;           /* first pass: bytes per segment, Adler sums */
    double ms_scan;            /* their scan, the Adler-32, the total read by the host */
    double ms_write;           /* second pass: the chunks and their CRCs */
    double ms_total;
    int64_t dynamic_segments;     /* segments written as a dynamic Huffman block (0 in fixed coding) */
    int64_t dynamic_header_bits;  /* the sum of their headers' bits: HLIT, HDIST, HCLEN, the code-length code, the coded lengths */
} SphPngStats;

#define SPH_PNG_CODING_FIXED 0     /* per segment the fixed Huffman code or a stored block (the default) */
#define SPH_PNG_CODING_DYNAMIC 1   /* also a dynamic Huffman block where it is strictly shorter */
#define SPH_PNG_CODING_WINDOW 3    /* also a dynamic block of the parse with matches from a 32 KB window, where that is shorter still
                                      (2 is not a coding and stays refused) */

/* what the window coding adds to SphPngStats (a struct of its own: SphPngStats keeps its size); zeros after an encode in another coding */
typedef struct {
    int64_t window_segments;      /* segments written as a block of the window parse; their tokens are counted in literals / matches */
    int64_t window_matches;       /* the matches in them that came from the window candidate (no fixed distance gave that length) */
    int64_t window_far_matches;   /* the matches in them that reach back more than 4096 bytes */
    int64_t window_header_bits;   /* the sum of their headers' bits */
    double ms_candidates;         /* HIP events: the candidates of the whole stream (between ms_filter and ms_count) */
} SphPngWindowStats;

typedef struct SphPng SphPng;
/* SPH_ERR_INVALID (before any device is touched): a size or filter outside the ranges above, reserved != 0 */
int sph_png_create(const SphPngParams *params, SphPng **out);
void sph_png_destroy(SphPng *v);
const char *sph_png_last_error(SphPng *v);
/* the entropy coding of the encodes that follow; SPH_ERR_INVALID with a message for any other value */
int sph_png_set_coding(SphPng *v, int32_t coding);
/* the longest file these parameters can give: 8 + 25 + 17 * segments + raw_bytes + 2 + 16 + 12 with segments =
   ceil(raw_bytes / 4096).  The same in every coding: a dynamic or window block replaces a segment's block only where it is
   strictly shorter.  Host only: no device is touched. */
int sph_png_bound(const SphPngParams *params, int64_t *bytes);
/* a host image u8[height][width][3], rows from the top */
int sph_png_encode_rgb(SphPng *v, const uint8_t *rgb);
/* the renderer's last frame (particles or meshes), read from its device buffer: not downloaded, nothing of the renderer modified.
   SPH_ERR_INVALID with a message: no frame rendered yet, a frame of another size, a renderer on another device. */
int sph_png_encode_render(SphPng *v, SphRender *r);
/* the last encoded frame: the length of the complete .png file, and the file */
int sph_png_size(SphPng *v, int64_t *bytes);
int sph_png_download(SphPng *v, uint8_t *dst);
int sph_png_stats(SphPng *v, SphPngStats *out);
int sph_png_window_stats(SphPng *v, SphPngWindowStats *out);
/* for tests and diagnosis: the candidates of the last encode, which was in window coding (else SPH_ERR_INVALID): prev[i] is the most
   recent j < i with i - j <= 32768 and the same three bytes at j as at i in the filtered stream, 0xFFFFFFFF for none; n = raw_bytes */
int sph_png_download_candidates(SphPng *v, uint32_t *prev, size_t n);

/* --- Text export: ASCII PLY / OBJ frame files formatted on the device -------------------------------------------- */
/* stands in for a download followed by sph_write_ply_ascii / sph_write_obj_ascii: the same bytes, made where the particles or the
   mesh lie.  A source is bound by one call; sph_text_write / sph_text_read then produce the file of that source in pieces of at most
   piece_rows rows: per piece a count pass (bytes per row), a scan, and a write pass that lays the characters at the scanned offsets
   (offsets inside a piece fit 32 bits, totals are 64-bit).  Numbers: float32 as the shortest decimal digits that round-trip, laid
   out as sph_format_f32 does ("nan", "inf", "-0.0", positional with a digit behind the point for 1e-4 <= |v| < 1e16, else
   d[.ddd]e+XX; at most 19 characters); indices 1-based.  Integer arithmetic only: the same bytes from both builds and from the host
   writers.  The host writes the PLY header and copies finished pieces from two alternating pinned buffers into the file while the
   device makes the next piece; device memory is bounded by the source plus piece_rows * (71 + 4) bytes, pinned host memory by
   2 * 71 * piece_rows.  One HIP stream per object; synchronous calls. */
typedef struct {
    int32_t piece_rows;      /* rows per piece, 1..2^22; 0: the default 2^20 */
    int32_t fast_math;       /* which build's launchers run (0 strict, 1 fast); the bytes are the same */
    int32_t device;          /* HIP device ordinal, -1: current */
    int32_t reserved;        /* 0 */
} SphTextParams;

typedef struct {
    int64_t rows;            /* lines behind the header */
    int64_t values;          /* numbers written: 3 per point, vertex and normal; 3 per face, 6 with normals */
    int64_t bytes;           /* the file, header included */
    int64_t pieces;
    int64_t longest_row;     /* bytes, the line feed included */
    double ms_source;        /* HIP events: upload / compaction of the bound source (~0 for a surface read in place) */
    double ms_count;         /* the stages of the last write / read / size, summed over the pieces */
    double ms_scan;
    double ms_write;
    double ms_copy;          /* pieces to pinned host memory */
    double ms_file;          /* host clock: fwrite of the pieces (sph_text_write), memcpy into dst (sph_text_read) */
    double ms_total;         /* host clock: the whole call */
} SphTextStats;

typedef struct SphText SphText;
/* SPH_ERR_INVALID (before any device is touched): piece_rows outside the range, reserved != 0 */
int sph_text_create(const SphTextParams *params, SphText **out);
void sph_text_destroy(SphText *t);
const char *sph_text_last_error(SphText *t);
/* Sources.  Each call replaces the bound source; a failed call leaves none bound.
   PLY of host points xyz f32[n][3] (uploaded). */
int sph_text_ply_points(SphText *t, const float *xyz, int64_t n);
/* PLY of one object's particles of a live handle, ghosts and dead slots left out, in the handle's current (sorted) order -- the rows
   of sph_download(SPH_F_POSITION) whose object id matches; compacted on the device by a scan, the handle's state untouched.
   SPH_ERR_UNSUPPORTED: a sharded handle.  SPH_ERR_INVALID: another device, between sph_step_begin and sph_step_end, a bad id. */
int sph_text_ply_object(SphText *t, SphHandle *h, int object_id);
/* OBJ of a host mesh (uploaded): vertices f32[nv][3], normals f32[nv][3] or NULL, triangles i32[nt][3] 0-based.  The indices are
   checked on the device (0 <= index < nv) before anything is written: SPH_ERR_INVALID, as sph_write_obj_ascii. */
int sph_text_obj_mesh(SphText *t, const float *vertices, int64_t nv, const float *normals_or_NULL, const int32_t *triangles, int64_t nt);
/* OBJ of the surface's last mesh (smoothed vertices and normals included), read in place on the device: the surface must not
   reconstruct again or be destroyed before the file has been produced.  SPH_ERR_INVALID: no mesh yet, another device. */
int sph_text_obj_surface(SphText *t, SphSurface *surface);
/* the file of the bound source.  SPH_ERR_INVALID: no source bound; SPH_ERR_UNSUPPORTED: the path cannot be opened or written */
int sph_text_write(SphText *t, const char *path);
/* the same bytes in memory: their number (a count-only run), and the file into dst[cap] (SPH_ERR_CAPACITY if it does not fit) */
int sph_text_size(SphText *t, int64_t *bytes);
int sph_text_read(SphText *t, void *dst, int64_t cap);
int sph_text_stats(SphText *t, SphTextStats *out);
/* the device's number routine run on the host (no device is touched): the n floats' characters back to back in out[cap], their
   lengths in lengths[n].  For tests of the routine, not a product path.  SPH_ERR_CAPACITY: cap < the sum of the lengths. */
int sph_text_format_f32_host(const float *values, int64_t n, char *out, int64_t cap, int64_t *lengths);

/* --- Diffuse particles: spray, foam and bubbles from the fluid state ---------------------------------------------- */
/* A second particle set, generated from the fluid and carried by it, that never acts back on it (Ihmsen, Akinci, Akinci, Teschner
   2012, as the project states it in DESIGN.md 26).  One sph_foam_step_* call: the fluid set is binned into the object's own grid of
   edge h = 4 radius (ordered by id inside a cell), the diffuse particles are advected and classified by their fluid neighbours
   (spray ballistic, foam with the fluid and ageing, bubbles buoyant and dragged), normals and the potentials trapped air / wave
   crest / energy are summed per fluid particle with w(r) = 1 - r / h, children are generated from counter-based random numbers --
   a hash of (seed, id, foam step, child, stream), no state -- and written behind the compacted survivors at scanned offsets.  No
   float atomics: the same input gives the same bytes, and the order of the fluid input does not matter.  float32, the strict
   build's arithmetic unless fast_math.  One HIP stream per object; synchronous calls. */
typedef struct {
    double radius;             /* particle radius r > 0; support h = 4 r */
    double domain_lo[3], domain_hi[3];   /* the simulation domain: the grid covers it, with one border cell per side */
    double padding;            /* diffuse particles live in [domain_lo + padding, domain_hi - padding], the fluid's clamp box */
    double gravity[3];
    double ta_min, ta_max;     /* clamp limits of the trapped-air, wave-crest and energy potentials, each max > min */
    double wc_min, wc_max;
    double e_min, e_max;       /* energy per unit mass, 0.5 |v|^2 */
    double k_ta, k_wc;         /* children per second at full potential */
    double life_min, life_max; /* seconds; life_max >= life_min > 0 */
    double k_b, k_d;           /* bubbles: buoyancy and drag */
    double normal_min;         /* a particle has a normal where |g_i| >= normal_min h */
    int32_t n_spray;           /* fewer fluid neighbours: spray */
    int32_t n_bubble;          /* more: bubble; between the two: foam */
    int32_t max_per_particle;  /* children of one fluid particle per step, 0..255 */
    int32_t fast_math;         /* which build's kernels run (0 strict, 1 fast) */
    int32_t device;            /* HIP device ordinal, -1: current */
    int32_t reserved;          /* 0 */
    int64_t max_diffuse;       /* capacity of the diffuse set; 0: twice the fluid capacity seen at the first step */
    uint64_t seed;
} SphFoamParams;

typedef struct {
    int64_t step;              /* foam steps taken (the t of the keys born in the last one) */
    int64_t fluid;             /* fluid particles of the last step */
    int64_t diffuse;           /* diffuse particles now */
    int64_t spray, foam, bubble;   /* the survivors' classes of the last advection */
    int64_t born, died, dropped;   /* of the last step; dropped: children beyond max_diffuse */
    int64_t born_total, died_total, dropped_total;
    int64_t pairs_visited[3];  /* candidate pairs of the advect, normals and potentials walks */
    int64_t pairs_accepted[3]; /* of those, r < h */
    int64_t bytes_allocated;
    double ms_grid, ms_advect, ms_normals, ms_potentials, ms_generate, ms_total;   /* HIP events (ms_grid: input and grid) */
} SphFoamStats;

typedef struct SphFoam SphFoam;
/* SPH_ERR_INVALID (before any device is touched): non-finite or non-positive radius, an empty domain, limits with max <= min, negative
   rates or counts, max_per_particle > 255, a grid of more than 2^30 cells, reserved != 0. */
int sph_foam_create(const SphFoamParams *params, SphFoam **out);
void sph_foam_destroy(SphFoam *f);
const char *sph_foam_last_error(SphFoam *f);
/* One step of length dt > 0 from the active fluid particles of a live handle (ghosts and dead slots left out), read on the device in
   the handle's current order; the handle's state is untouched.  SPH_ERR_UNSUPPORTED: a sharded handle or one whose library frame is a
   permutation of the scene's.  SPH_ERR_INVALID: another device, between sph_step_begin and sph_step_end, dt not positive and finite. */
int sph_foam_step_handle(SphFoam *f, SphHandle *h, double dt);
/* The same from host arrays: xyz f32[n][3], vel f32[n][3], ids i32[n] (distinct; they take the place of the handle's particle ids in
   the random numbers and the keys).  n = 0 is legal: the diffuse particles are advected through empty space. */
int sph_foam_step_points(SphFoam *f, const float *xyz, const float *vel, const int32_t *ids, int64_t n, double dt);
/* The caller's own diffuse particles: xyz f32[n][3], vel f32[n][3], life f32[n].  Their keys are 2^63 | serial number (from 0, in
   call order).  SPH_ERR_CAPACITY: more than max_diffuse in all; SPH_ERR_INVALID: max_diffuse = 0 and no step has sized the set yet. */
int sph_foam_seed(SphFoam *f, const float *xyz, const float *vel, const float *life, int64_t n);
int sph_foam_count(SphFoam *f, int64_t *n);
/* The diffuse set in device order (unspecified; the key identifies a particle: foam step << 40 | id << 8 | child): xyz f32[n][3],
   vel f32[n][3], life f32[n], key u64[n], cls i32[n] -- the class of the last advection, 0 spray, 1 foam, 2 bubble, 3 born in the
   last step (children are not advected in their birth step) or seeded since.  Any output may be NULL. */
int sph_foam_download(SphFoam *f, float *xyz, float *vel, float *life, uint64_t *key, int32_t *cls);
/* The fluid quantities of the last step, one row per fluid particle of that step: in input order for sph_foam_step_points, in the
   handle's order (active fluid only) with their particle ids for sph_foam_step_handle.  ta, wc, e, nd f32[n], normal f32[n][3]
   (zero: no normal), ids i32[n]; any output may be NULL.  SPH_ERR_INVALID: no step yet. */
int sph_foam_download_potentials(SphFoam *f, float *ta, float *wc, float *e, float *nd, float *normal, int32_t *ids);
/* forget every diffuse particle (the step counter and the seed serial stay) */
int sph_foam_clear(SphFoam *f);
int sph_foam_stats(SphFoam *f, SphFoamStats *out);

/* Diffuse particles in particle frames.  While a foam object is set, sph_render_handle draws its diffuse particles from the device
   into the frame: spheres of radius_scale x the renderer's radius, coloured by class (rgb_* u8[3]; NULL: 250 250 255 / 255 255 255 /
   225 235 250), ids 0x80000000 | (low 31 bits of a hash of the key), folded into the key plane before the pixels are finished.  NULL
   clears it; without it no kernel argument or launch of sph_render_handle changes.  The object must outlive its use here.
   SPH_ERR_UNSUPPORTED: the surface mode is on (also when it is switched on later: sph_render_handle then refuses), at
   sph_render_handle for a sharded handle; SPH_ERR_INVALID: another device, radius_scale not positive, and at sph_render_handle a
   handle whose particle_max_num reaches 2^31 (its ids could not be told from diffuse ones). */
int sph_render_set_foam(SphRender *r, SphFoam *foam_or_NULL, double radius_scale, const uint8_t *rgb_spray, const uint8_t *rgb_foam,
                        const uint8_t *rgb_bubble);

/* --- Diffuse particles in the surface frames: white water over and under the surface ------------------------------- */
/* opt-in on top of the surface mode, entered through these calls only.  While a foam object is set, sph_render_handle -- behind the
   frame, the base plane and, thickness mode, the opaque layer and the thickness plane -- walks every diffuse sphere (radius rf =
   radius_scale x the renderer's) over the pixel centres of its bounds with the chord [t0, t1] of the thickness splat (counted when
   h >= 0 and t0 > z_near).  The limit L of a pixel is the frame's own depth t_w in the opaque surface mode and the opaque layer's depth
   in thickness mode (absent where that key is all ones); c = (u32)((min(t1, L) - t0) * inv_u) when min(t1, L) > t0.  Thickness mode, on a
   surface pixel with t0 >= t_w + depth_bias r: the pair is UNDER the surface -- fu += c, du = min(du, (u32)((t0 - t_w) * inv_u)) --
   otherwise OVER it: fo += c.  Integer atomics only: the three u32 planes are functions of the particle sets.  With raw_spheres the
   diffuse spheres are then also drawn into the particle frame as sph_render_set_foam draws them (its default class colours), after the
   frame's key plane has been copied; the frame's rgb is copied in either case, so that a repeated sph_render_surface starts from it.
   sph_render_surface then, behind its shade, with I(F) = 1 - exp2(-(density F / 256)) and f = rgb / 255, in f32 without contraction:
     under (thickness mode, surface pixels with fu > 0, I(fu) != 0): Tm = max(T, 1), T1 = min(Tm, du) / 256, T2 = (Tm - min(Tm, du)) / 256,
       k = absorb (1 - base) + scatter, a1 = exp2(-(k T1)), a2 = exp2(-(k T2)),
       out = byte((lit (1 - a1) + a1 (f I(fu) + (1 - I(fu)) (lit (1 - a2) + a2 behind))) + highlight);
     over (every pixel with fo > 0, I(fo) != 0): out = byte((cur / 255) (1 - I(fo)) + f I(fo)), cur the byte the pixel holds.
   The points path ignores the mode.  Without it no launch, allocation or byte of any call changes. */
typedef struct {
    double radius_scale;      /* the diffuse sphere's radius in renderer radii, > 0 (0.5) */
    double density;           /* per particle radius of diffuse chord, >= 0 (1.0) */
    double depth_bias;        /* particle radii behind the surface depth from which a chord counts as under it, >= 0 (1.0) */
    uint8_t rgb[3];           /* the white water's colour (255 255 255) */
    uint8_t raw_spheres;      /* != 0: the diffuse spheres are also drawn into the particle frame (1) */
    int32_t reserved;         /* 0 */
} SphRenderSurfaceFoamParams;

typedef struct {
    int64_t diffuse;          /* diffuse particles of the frame */
    int64_t large;            /* of these: walked by one workgroup each */
    int64_t adds_over;        /* (sphere, pixel) pairs that added to fo: one integer atomic each */
    int64_t adds_under;       /* ... to fu (and lowered du): two */
    int64_t clipped;          /* of both: cut short by the limit */
    int64_t removed;          /* pairs that hit but lay wholly behind the limit (no atomic) */
    int64_t pixels_over;      /* of the last sph_render_surface: pixels with fo > 0 */
    int64_t pixels_under;     /* ... with fu > 0 */
    double ms_splat;          /* HIP events: the copies and the splat, ... */
    double ms_raw;            /* ... the raw spheres' layer and its merge (parts of the frame call) */
    double ms_composite;      /* the under and over passes (part of sph_render_surface, behind its ms_shade) */
} SphRenderSurfaceFoamStats;

/* sets the diffuse set (params NULL: the defaults above) or clears it (foam NULL); applies to the frames sph_render_handle draws
   afterwards.  The object must outlive its use here.  SPH_ERR_INVALID, with a message that names the field: the surface mode is off,
   another device, radius_scale not positive or not finite, density / depth_bias negative or not finite, reserved not 0;
   SPH_ERR_UNSUPPORTED: sph_render_set_foam is set at the same time (which in turn stays refused while the surface mode is on).  At
   sph_render_handle: SPH_ERR_UNSUPPORTED for a sharded handle and, before any launch, for a diffuse count n with n ceil(512
   radius_scale) >= 2^32; SPH_ERR_INVALID with raw_spheres for a handle whose particle_max_num reaches 2^31.  sph_render_surface refuses
   (SPH_ERR_INVALID) a handle frame drawn before the set was given or its parameters changed, or before the thickness mode was
   switched.  Switching the surface mode off clears the set. */
int sph_render_set_surface_foam(SphRender *r, SphFoam *foam_or_NULL, const SphRenderSurfaceFoamParams *params_or_NULL);
/* a plane of the last sph_render_handle frame drawn with the set: plane 0 fo, 1 fu, 2 du (all ones: none), out u32[height][width] */
int sph_render_surface_download_foam(SphRender *r, int plane, uint32_t *out);
int sph_render_surface_foam_stats(SphRender *r, SphRenderSurfaceFoamStats *out);

#ifdef __cplusplus
}
#endif
#endif /* SPH_HIP_H */
