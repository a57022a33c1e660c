// sph_api.hip -- C-ABI of libsph_hip.so (include/sph_hip.h): device state, step orchestration,
// host<->device transfers, HIP-event profiler.  Host code only; kernels live in sph_kernels.hip.
#include "../../include/sph_hip.h"
#include "sph_common.hpp"
#include "sph_comm.hpp"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <stdlib.h>
#include <utility>
#include <array>
#include <algorithm>
#include "sph_voxel.hpp"
#include "sph_export.hpp"
#include "sph_devobj.hpp"

struct ProfSlot {
    bool on = false;
    int64_t launches = 0;
    double ms = 0.0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// elastic solids: one object as the host keeps it (sph_elastic_api.hpp).  state: the values of SphElasticObjectInfo::captured
struct ElObjHost { int state = 0; double E = 0.0, nu = 0.0; int id0 = 0, n = 0, longest = 0, slot = -1; float min_ratio = 0.0f; float4 *rest = nullptr; };

// fluid emitters: one emitter as the host keeps it (sph_emitter_api.hpp): the program, the lattice counts derived from it, the layers born
// so far and the persistent id of each layer's first particle
struct EmHost { bool on = false; SphEmitter e = {}; int nu = 0, nv = 0, layer_n = 0, max_layers = 0, layers = 0; std::vector<int> base; };

// outflow: one volume as the host keeps it (sph_outflow_api.hpp): the program, what it has removed in all and in the last slot
struct OfHost { bool on = false; SphOutflow v = {}; long long removed = 0; int last = 0; };

// adaptive time stepping (sph_cfl_api.hpp): the parameters, the step size the handle was created with, the time target (NaN: none), what
// the last reduce found, and the flags of the pending step size.  stale: the maximum no longer describes the state (the next step begins
// with a reduce).  irregular: a step was taken with another size than the creation one (the scene time is no closed form of the count)
struct CflHost {
    bool on = false, stale = true, irregular = false;
    SphCflParams p = {};
    double dt_create = 0.0; float dt_create_f = 0.0f;
    double target = NAN, dt_last = 0.0;
    float vmax2 = 0.0f;
    int flags = 0, bank = 0;
    unsigned *pinned = nullptr;
};

struct SphHandle : ErrSink {
    SphParams prm = {};
    State st;
    const Launch *L = nullptr;
    int device = 0;
    int n = 0;            // particle_num (a launch BOUND while n_exact is false: asynchronous slab steps, see slab_settle)
    bool n_exact = true;
    int n_fluid = 0;      // fluid_particle_num
    int n_nonfluid = 0;
    // every fluid particle appended so far carries the same mass (one fluid density: the usual scene), and nobody has uploaded masses:
    // the fused force pass then runs its uniform-mass instantiation (bit-identical sums, four VALU less per pair)
    bool fluid_mass_seen = false, fluid_mass_uniform = true; float fluid_mass0 = 0.0f;
    bool any_rigid_object = false;   // a non-fluid object was registered (slab sharding: its particles may live on another rank)
    int64_t steps = 0;
    int pbf_bank = 0;              // PBF: statistics bank of State::pbf_recentred the last step / phase counted into
    SphPbfParams pbf = {SPH_PBF_VARIANT_REFERENCE, 1, 50, 1e-3f, 1e-6f};   // sph_set_pbf_variant (the defaults of the scene keys)
    SphPbfStats pbf_last = {SPH_PBF_VARIANT_REFERENCE, 0, 0.0f};          // iterations / error of the last step's solve (sph_get_pbf_stats)
    int steps_to_follow = 0;       // sph_step_async(n): steps of this call still to come after the running one
    bool whole_step = false;       // both halves of the running step are ONE call (step_once): nothing on the host happens between them
    double total_time = 0.0;
    bool prepared = false;
    bool pose_dirty = false;
    int loop_hint[4] = {0, 0, 0, 0};   // iterations the last solve of each device-controlled loop took (sph_steps.hpp run_solve), by reduction slot
    struct LoopPub *loop_pub = nullptr;   // pinned: residual + flags of a solver loop's batch, published by a kernel (sph_steps.hpp k_publish_loop)
    unsigned loop_seq = 0, stats_seq = 0;
    bool loop_flags_clean = false;   // scal->flags[0..1] are zero (the publishing kernel of a stopped loop reset them): run_solve needs no memset
    int dev_cus = 256;           // compute units of the device (sizing of grids that should be resident at once)
    bool pose_given = false;     // sph_set_rigid_pose was called: pose_h holds library-frame vectors of the CURRENT axis order
    bool rigid_volume_done = false;
    bool sort_dirty = false;      // particles appended since the last sort
    bool in_step = false;         // between sph_step_begin and sph_step_end
    int n_mark = 0;               // particle count at the end of sph_step_begin: [n_mark, n) was appended mid-step
    int fresh_state = 0;          // rigid particles appended after prepare(): 1 = the next post-sort volume pass leaves them alone, 2 = the one after includes them (see ph_rigid_volume)
    RigidPose pose_h = {};   // (sph_create sets the identity rotations)
    // device rigid integrator: host copy of the registered bodies (their constants; the state part is what was uploaded last), the
    // capacity of each body's point array, and whether the kernel has moved the device pose since pose_h was last brought up to date
    RigidBodyDev rb_h[SPH_NOBJ] = {};
    int rb_cap[SPH_NOBJ] = {};
    bool rb_pose_stale = false;
    // scripted rigid bodies (sph_set_rigid_motion): which objects have a program; their records live on the device (State::rigid_motion)
    bool rm_on[SPH_NOBJ] = {};
    SphStats last = {};
    ProfSlot prof[SPH_K_COUNT_];
    std::vector<hipEvent_t> ev_pool;
    std::vector<void *> allocs;
    DevScalars *scal_h = nullptr;  // pinned
    SlabComm comm;
    long long comm_n_global = 0;   // particle_num of the whole scene (sum of the ranks' owned particles), see sph_prepare
    long long comm_nfluid_global = 0;   // fluid_particle_num of the whole scene (PCISPH's error mean divides by it)
    // Slab sharding: the scene's slab axis (z by contract; SPH_SLAB_AXIS=x|y|z) is SWAPPED with x at this ABI boundary,
    // because the library cuts its grid along x, the slowest axis of its cell order (layers = contiguous index ranges of the sorted
    // arrays: boundary workgroups first, interior ones while the halo flies).  0: no swap.  Everything a caller hands over or reads
    // back stays in the scene's frame: positions / velocities / every 3-vector field, gravity, domain, grid, rigid poses and
    // wrenches are permuted here (P = P^-1, det P = -1: axial vectors -- torque, angular velocity -- also change sign).
    int swap_axis = 0;             // != 0: the frames differ (kept as a flag; the permutation itself follows)
    int perm[3] = {0, 1, 2};       // library axis k  = scene axis perm[k]
    int inv[3] = {0, 1, 2};        // scene axis k    = library axis inv[k]
    float axial = 1.0f;            // parity of the permutation: sign of axial vectors (torque, angular velocity) across the boundary
    int slab_axis = 2;             // library axis the slabs are cut along (Consts::slab_axis): 2 = z (default), 0 = x (SPH_SLAB_LAYOUT=slow)
    // elastic solids: the objects, and for EVERY object the id range its appends made (first id, count, whether another object's append
    // split it); el_rc: the error of a capture that ran inside a neighbour search, returned by the call that searched (check_async)
    ElObjHost el[SPH_NOBJ];
    int obj_first[SPH_NOBJ] = {}, obj_n[SPH_NOBJ] = {};
    bool obj_split[SPH_NOBJ] = {};
    int el_rc = 0;
    // fluid emitters (sph_set_emitter): em_n of the SPH_MAX_EMITTERS slots are set; em_touch: the slot of the running step holds or emits
    // (known before the step's first launch: no pass of that step hashes for the coming sort)
    EmHost em[SPH_MAX_EMITTERS];
    int em_n = 0;
    bool em_touch = false;
    // outflow (sph_set_outflow, sph_remove_particles): of_n of the SPH_MAX_OUTFLOWS slots are set; of_pending: particles that carry the
    // dead bit and leave with the next sort; of_seen: the device counters as read last; id_next: the id of the next new particle once
    // something has been removed (until then ids are the append slots: next_id)
    OfHost of[SPH_MAX_OUTFLOWS];
    int of_n = 0, of_pending = 0;
    unsigned of_seen[SPH_MAX_OUTFLOWS] = {}, of_seen_ids = 0;   // (of_seen_ids: the counter of k_outflow_mark_ids)
    unsigned *of_pinned = nullptr;
    bool of_removed_any = false;
    int id_next = 0;
    CflHost cfl;
    // heat (sph_set_thermal): the per-object temperatures as the host keeps them, by the low byte of the meta word (object id + 1);
    // the device copy (State::heat_obj_T) follows every change while it exists
    bool heat_obj_has[256] = {};
    double heat_obj_T_h[256] = {};
};
static inline int next_id(const SphHandle *h);
// heat: the temperature a particle of this object (-1: the domain box) is inserted with
static inline float heat_insert_T(const SphHandle *h, int object_id) {
    const int b = (object_id + 1) & 0xff;
    return (float)(h->heat_obj_has[b] ? h->heat_obj_T_h[b] : h->st.heat_t_ref);
}
static long long em_reserved(const SphHandle *h);
static int em_of_object(const SphHandle *h, int object_id);

// layers of the whole scene along the slab axis / setting the local window [lo_ghost, top) of a rank
static inline int slab_layers_glob(const Consts &c) { return c.slab_axis == 0 ? c.nx_glob : c.nz_glob; }
static inline void slab_set_window(Consts &c, int z_lo, int z_hi) {
    const int glob = slab_layers_glob(c);
    const int off = z_lo > 0 ? z_lo - 1 : 0;              // one ghost layer per interior side
    const int top = z_hi < glob ? z_hi + 1 : glob;
    if (c.slab_axis == 0) { c.cx_off = off; c.nx = top - off; } else { c.cz_off = off; c.nz = top - off; }
    c.G = c.nx * c.ny * c.nz;
}

// "zxy" = library (x, y, z) <- scene (z, x, y)
static bool set_axis_order(SphHandle *h, const char *order) {
    int p[3], seen = 0;
    for (int k = 0; k < 3; ++k) {
        const char ch = order ? order[k] : 0;
        p[k] = (ch == 'x' || ch == 'X') ? 0 : (ch == 'y' || ch == 'Y') ? 1 : (ch == 'z' || ch == 'Z') ? 2 : -1;
        if (p[k] < 0) return false;
        seen |= 1 << p[k];
    }
    if (seen != 7 || order[3]) return false;
    for (int k = 0; k < 3; ++k) { h->perm[k] = p[k]; h->inv[p[k]] = k; }
    const bool even = (p[0] == 0 && p[1] == 1) || (p[0] == 1 && p[1] == 2) || (p[0] == 2 && p[1] == 0);
    h->axial = even ? 1.0f : -1.0f;
    h->swap_axis = !(p[0] == 0 && p[1] == 1 && p[2] == 2);
    return true;
}

template <class T> static int dalloc(SphHandle *h, T **p, size_t count) {
    void *q = nullptr;
    if (count == 0) count = 1;
    HIPCHK(h, hipMalloc(&q, count * sizeof(T)));
    HIPCHK(h, hipMemset(q, 0, count * sizeof(T)));
    h->allocs.push_back(q);
    *p = (T *)q;
    return SPH_OK;
}

// host replica of base_solver.py:57 kernel_W, same rounding as oracle/sph_ref.c (host TU is built
// with -ffp-contract=off)
static float host_kernel_W(double hd, float r) {
    float res = 0.0f;
    float k = (float)(8.0 / M_PI);
    k /= (float)(hd * hd * hd);
    float q = r / (float)hd;
    if (q <= 1.0f) {
        if (q <= 0.5f) { float q2 = q * q; float q3 = q2 * q; res = k * (6.0f * q3 - 6.0f * q2 + 1.0f); }
        else res = k * 2.0f * powf(1.0f - q, 3.0f);
    }
    return res;
}

static void fill_consts(SphHandle *h) {
    const SphParams &p = h->prm;
    Consts &c = h->st.c;
    memset(&c, 0, sizeof(c));
    const int *ix = h->perm;
    c.nx = c.nx_glob = p.grid_num[ix[0]]; c.ny = p.grid_num[ix[1]]; c.nz = c.nz_glob = p.grid_num[ix[2]];
    c.cx_off = c.cz_off = 0;
    c.slab_axis = h->slab_axis;
    c.G = c.nx * c.ny * c.nz;
    const double hd = p.support_radius;
    c.grid_size = (float)hd;
    c.h = (float)hd;
    // Acceptance test of a neighbour: the reference asks `(x_i - x_j).norm() < dh` (base_container.py:559), the kernels ask
    // `r2 < h2` without the square root.  sqrtf is monotone and correctly rounded, so there is an exact threshold: the
    // smallest f32 t with sqrtf(t) >= h.  r2 < t  <=>  sqrtf(r2) < h, bit for bit (lattices put many pairs exactly one
    // support radius apart; with h2 = h * h those could fall on the other side by one ulp).
    {
        float t = c.h * c.h;
        while (sqrtf(nextafterf(t, 0.0f)) >= c.h) t = nextafterf(t, 0.0f);
        while (sqrtf(t) < c.h) t = nextafterf(t, INFINITY);
        c.h2 = t;
    }
    c.inv_h = 1.0f / c.h;
    float k = (float)(8.0 / M_PI);
    c.kW = k / (float)(hd * hd * hd);
    c.kG = 6.0f * k / (float)(hd * hd * hd);
    c.W0 = host_kernel_W(hd, 0.0f);
    const float d = (float)(2.0 * p.particle_radius);
    c.Wd = host_kernel_W(hd, sqrtf(d * d + 0.0f + 0.0f));
    c.kGh = c.kG * c.inv_h;
    c.inv_h2 = c.inv_h * c.inv_h;
    c.Wd_poly = c.Wd / c.kW;
    const double dd = 2.0 * p.particle_radius;
    c.diameter2 = (float)(dd * dd);
    c.dt = (float)p.dt;
    c.inv_dt = 1.0f / c.dt;
    c.rho0 = (float)p.density_0;
    c.inv_rho0 = 1.0f / c.rho0;
    c.g_upper = (float)p.g_upper;
    c.up_axis = h->inv[1];
    c.gx = (float)p.gravity[ix[0]]; c.gy = (float)p.gravity[ix[1]]; c.gz = (float)p.gravity[ix[2]];
    c.st = (float)p.surface_tension;
    c.cv = (float)(2 * (3 + 2) * p.viscosity);
    c.cvb = (float)(2 * (3 + 2) * p.viscosity_b);
    c.visc_eps = (float)(0.01 * hd * hd);
    c.pad = (float)p.padding;
    c.hix = (float)(p.domain_size[ix[0]] - p.padding);
    c.hiy = (float)(p.domain_size[ix[1]] - p.padding);
    c.hiz = (float)(p.domain_size[ix[2]] - p.padding);
    c.thr_kappa = (float)1e-5 * c.dt;
    c.V0 = (float)p.V0;
    c.force_global = p.force_global;
    c.stat_bank = 0;
    c.run_grouping = 0;
    c.xcd_chunk = 0;
    c.ghosts = 0;
}

static void refresh_counts(SphHandle *h) {
    h->st.c.n = h->n;
    h->st.has_emitter = h->prm.g_upper < 9999.0;
    h->st.c.all_fluid = (h->n_nonfluid == 0 && !h->st.has_emitter && !(h->st.slab_active && h->any_rigid_object)) ? 1 : 0;
    h->st.c.ghosts = h->st.slab_active ? 1 : 0;
    // staging groups of the neighbour passes (sph_device.hpp run_of): outer runs mixed in the fast build on unsharded grids that are not thin
    // (a slab's runs overlap and are staged once, nbr_plan "chain": x-offset groups there)
    h->st.c.run_grouping = (h->prm.fast_math && !h->st.slab_active && h->st.c.nz >= 40) ? 1 : 0;
    h->st.has_rigid = h->n_nonfluid > 0;
    h->st.uniform_mass = (h->st.c.all_fluid && h->fluid_mass_uniform && !h->st.slab_active && !getenv("SPH_NO_UNIFORM_MASS")) ? 1 : 0;
}

extern "C" const char *sph_last_error(SphHandle *h) { return last_error(h); }

extern "C" const char *sph_kernel_name(int k) {
    // the table ends at id 29: tests/test_pbf_consistent_host.py pins "?" for id 30, so SPH_K_RIGID_MOTION (30) is profiled like every
    // other id but has no entry here; its name is the enum's (include/sph_hip.h)
    static const char *names[] = {
        "hash_count", "scan", "scatter", "density", "non_pressure", "pressure_integrate", "rigid_volume",
        "dfsph_density_alpha", "dfsph_rho_adv", "dfsph_correct", "reduce", "pcisph_rho_star",
        "pcisph_pressure_accel", "cg_prepare", "cg_ap", "cg_vector", "misc", "halo", "wcsph_forces",
        "iisph_prepare", "iisph_dij_pj", "iisph_sum_i", "pbf_density_lambda", "pbf_fix_position", "pbf_update",
        "rigid_contact", "rigid_integrate", "rigid_contact_solve", "pbfc_density_lambda", "pbfc_delta"};
    return (k >= 0 && k < (int)(sizeof(names) / sizeof(names[0]))) ? names[k] : "?";
}

static void slab_comm_destroy(SlabComm &c);
static int slab_settle(SphHandle *h);
static inline int slab_settle_if_needed(SphHandle *h) { return h->n_exact ? SPH_OK : slab_settle(h); }

extern "C" void sph_destroy(SphHandle *h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->st.stream) hipStreamSynchronize(h->st.stream);
    slab_comm_destroy(h->comm);
    if (h->st.push.mirror) { hipHostFree(h->st.push.mirror); h->st.push.mirror = nullptr; }
    for (auto &s : h->prof) for (auto &pr : s.pending) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (auto e : h->ev_pool) hipEventDestroy(e);
    for (void *p : h->allocs) hipFree(p);
    if (h->scal_h) hipHostFree(h->scal_h);
    if (h->loop_pub) hipHostFree((void *)h->loop_pub);
    if (h->of_pinned) hipHostFree((void *)h->of_pinned);
    if (h->cfl.pinned) hipHostFree((void *)h->cfl.pinned);
    if (h->st.list_count_pinned) { hipHostFree((void *)h->st.list_count_pinned); h->st.list_count_pinned = nullptr; }
    if (h->st.list_count_event) { hipEventDestroy(h->st.list_count_event); h->st.list_count_event = nullptr; }
    if (h->st.stream) hipStreamDestroy(h->st.stream);
    delete h;
}

extern "C" int sph_create(const SphParams *params, SphHandle **out) {
    if (!params || !out) return fail(nullptr, SPH_ERR_INVALID, "sph_create: null argument");
    *out = nullptr;
    const SphParams &p = *params;
    if (p.particle_max_num < 0 || p.grid_num[0] <= 0 || p.grid_num[1] <= 0 || p.grid_num[2] <= 0 ||
        !(p.support_radius > 0) || !(p.dt > 0))
        return fail(nullptr, SPH_ERR_INVALID, "sph_create: invalid parameters");
    if ((double)p.grid_num[0] * p.grid_num[1] * p.grid_num[2] > 2.0e9)
        return fail(nullptr, SPH_ERR_INVALID, "sph_create: grid too large");
    // particle indices travel as 32-bit BYTE offsets into float4 arrays (ldg_idx) and as 28-bit slot numbers of the slab
    // sharding: 2^28 - 1 particles per handle (~70 GB of state; a bigger scene is sharded over GPUs)
    if (p.particle_max_num > 0x0fffffff)
        return fail(nullptr, SPH_ERR_CAPACITY, "sph_create: particle_max_num %d exceeds 268435455 per GPU; shard the scene (sph_comm_set_slab)", p.particle_max_num);
    if (p.method < 0 || p.method > SPH_METHOD_PBF) return fail(nullptr, SPH_ERR_INVALID, "sph_create: unknown method %d", p.method);
    int dev = 0;
    { int rc = pick_device("sph_create", p.device, &dev); if (rc) return rc; }
    SphHandle *h = new SphHandle();
    h->prm = p;
    h->device = dev;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) h->dev_cus = cus; }
#define CHK_CREATE(call)                                                                   \
    do {                                                                                   \
        int rc_ = (call);                                                                  \
        if (rc_ != SPH_OK) { g_create_error = h->err; sph_destroy(h); return rc_; }        \
    } while (0)
#define HIP_CREATE(call)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            fail(nullptr, SPH_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));     \
            sph_destroy(h);                                                                \
            return SPH_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)
    h->L = p.fast_math ? sph_launch_fast() : sph_launch_strict();
    State &s = h->st;   // (every member starts from its initialiser: what follows allocates, and derives from the parameters)
    HIP_CREATE(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    fill_consts(h);
    h->cfl.dt_create = p.dt; h->cfl.dt_create_f = s.c.dt;
    const size_t cap = (size_t)p.particle_max_num;
    s.cap = p.particle_max_num;
    for (int k = 0; k < 2; ++k) {
        CHK_CREATE(dalloc(h, &s.posv.b[k], cap)); CHK_CREATE(dalloc(h, &s.velm.b[k], cap));
        CHK_CREATE(dalloc(h, &s.meta.b[k], cap)); CHK_CREATE(dalloc(h, &s.pid.b[k], cap));
        CHK_CREATE(dalloc(h, &s.color.b[k], cap)); CHK_CREATE(dalloc(h, &s.rho.b[k], cap));
    }
    const size_t G = (size_t)s.c.G;
    CHK_CREATE(dalloc(h, &s.cell_count, G + SPH_NGRAVE + 1)); CHK_CREATE(dalloc(h, &s.cell_start, G + SPH_NGRAVE + 1));   // + graveyard cells (slab sharding)
    CHK_CREATE(dalloc(h, &s.cellid, cap)); CHK_CREATE(dalloc(h, &s.rank, cap)); CHK_CREATE(dalloc(h, &s.tmp_idx, 2 * cap));   // (int2 run records of the stable sort)
    if (h->prm.deterministic && !getenv("SPH_NO_RUN_LISTS")) { CHK_CREATE(dalloc(h, &s.run_head, G + 1)); CHK_CREATE(dalloc(h, &s.run_rec, cap + G + 1)); CHK_CREATE(dalloc(h, &s.sort_inv, cap)); CHK_CREATE(dalloc(h, &s.color_home, cap)); s.color_home_ok = 1; }   // deterministic sort by run lists (RunList, sph_common.hpp)
    s.scan_blocks = (int)((G + SPH_NGRAVE + 2047) / 2048);
    if (s.scan_blocks < SPH_STAT_SLOTS / 256) s.scan_blocks = SPH_STAT_SLOTS / 256;   // k_scan_final also clears the statistics slots
    CHK_CREATE(dalloc(h, &s.scan_tile_state, (size_t)s.scan_blocks + 1));
    CHK_CREATE(dalloc(h, &s.scan_partial, 2 * ((size_t)s.scan_blocks + 1) * 8));   // two banks of tile sums, SCAN_PARTIAL_STRIDE ints apart (State::scan_bank)
    CHK_CREATE(dalloc(h, &s.rho_raw, cap)); CHK_CREATE(dalloc(h, &s.prs, cap)); CHK_CREATE(dalloc(h, &s.ptm, cap));
    CHK_CREATE(dalloc(h, &s.acc, cap));
    CHK_CREATE(dalloc(h, &s.nbr_mask, cap * 9 + 256)); CHK_CREATE(dalloc(h, &s.nbr_mask_hi, cap * 9 + 256));   // + 256: the lanes past the last particle of the last tile read (and drop) a word too
    CHK_CREATE(dalloc(h, &s.blk_hdr, (cap + 255) / 256 * (20 + 256)));   // headers of all tiles, then one cell word per particle slot (k_block_prep)
    if (!getenv("SPH_NO_BLOCK_LIST")) {
        CHK_CREATE(dalloc(h, &s.blk_flag, (cap + 255) / 256)); CHK_CREATE(dalloc(h, &s.blk_list, (cap + 255) / 256)); CHK_CREATE(dalloc(h, &s.blk_count, 1));
    }
    CHK_CREATE(dalloc(h, &s.lane_perm, (cap + 255) / 256 * 256));
    if (p.method == SPH_METHOD_DFSPH) {
        CHK_CREATE(dalloc(h, &s.alpha, cap)); CHK_CREATE(dalloc(h, &s.kappa, cap)); CHK_CREATE(dalloc(h, &s.kappa_v, cap));
        CHK_CREATE(dalloc(h, &s.rho_star, cap)); CHK_CREATE(dalloc(h, &s.rho_deriv, cap)); CHK_CREATE(dalloc(h, &s.kr, cap));
        CHK_CREATE(dalloc(h, &s.kappa_next, cap)); CHK_CREATE(dalloc(h, &s.kappa_v_next, cap));
    }
    if (p.method == SPH_METHOD_PCISPH) {
        CHK_CREATE(dalloc(h, &s.pacc, cap)); CHK_CREATE(dalloc(h, &s.pvel, cap)); CHK_CREATE(dalloc(h, &s.ppos, cap));
        CHK_CREATE(dalloc(h, &s.rho_star, cap)); CHK_CREATE(dalloc(h, &s.acc_np, cap));
        s.np_acc_out = s.acc_np;
    }
    if (p.method == SPH_METHOD_IISPH) {   // IISPH.py scratch: 52 bytes per particle, only for this method
        CHK_CREATE(dalloc(h, &s.iisph_dii, cap)); CHK_CREATE(dalloc(h, &s.iisph_dij, cap)); CHK_CREATE(dalloc(h, &s.iisph_w, cap));
        CHK_CREATE(dalloc(h, &s.rho_star, cap));
    }
    if (p.method == SPH_METHOD_PBF) {   // pbf_container.py:11-13, sized particle_max_num (D2); 36 bytes per particle
        CHK_CREATE(dalloc(h, &s.pbf_old, cap)); CHK_CREATE(dalloc(h, &s.pbf_pos, cap)); CHK_CREATE(dalloc(h, &s.pbf_lambda, cap));
        CHK_CREATE(dalloc(h, &s.pbf_recentred, 2));
        s.poly6 = 1;
    }
    if (p.viscosity_implicit) {
        CHK_CREATE(dalloc(h, &s.cg_p, cap)); CHK_CREATE(dalloc(h, &s.cg_Ap, cap)); CHK_CREATE(dalloc(h, &s.cg_x, cap));
        CHK_CREATE(dalloc(h, &s.cg_b, cap)); CHK_CREATE(dalloc(h, &s.cg_r, cap)); CHK_CREATE(dalloc(h, &s.cg_v0, cap));
        CHK_CREATE(dalloc(h, &s.cg_dinv, cap * 9));
        CHK_CREATE(dalloc(h, &s.cg_part, cap * 3));
        CHK_CREATE(dalloc(h, &s.cg_p2, cap));
    }
    s.red_blocks = (int)((cap + 255) / 256) + 1;
    CHK_CREATE(dalloc(h, &s.red_partial, (size_t)s.red_blocks * 8));   // (also the four partial-sum arrays of the CG kernels)
    CHK_CREATE(dalloc(h, &s.scal, 1)); CHK_CREATE(dalloc(h, &s.pose, 1));
    HIP_CREATE(hipHostMalloc((void **)&h->scal_h, sizeof(DevScalars), hipHostMallocDefault));
    { void *lp = nullptr; HIP_CREATE(hipHostMalloc(&lp, 128, hipHostMallocDefault)); memset(lp, 0, 128); h->loop_pub = (struct LoopPub *)lp; }   // + StatsPub behind it
    { int *lc = nullptr; HIP_CREATE(hipHostMalloc((void **)&lc, 64, hipHostMallocDefault)); *lc = 0; s.list_count_pinned = lc; }
    HIP_CREATE(hipEventCreateWithFlags(&s.list_count_event, hipEventDisableTiming));
    memset(h->scal_h, 0, sizeof(DevScalars));
    for (int o = 0; o < SPH_NOBJ; ++o) { h->pose_h.rot[o][0] = h->pose_h.rot[o][4] = h->pose_h.rot[o][8] = 1.0f; }
    s.z_hi = slab_layers_glob(s.c);
    s.visc_rho_raw = (p.method == SPH_METHOD_WCSPH);
    refresh_counts(h);
    *out = h;
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- scene upload
// rigid_particle_original_positions (base_container.py:155): allocated with the first dynamic rigid body
static int ensure_orig(SphHandle *h) {
    State &s = h->st;
    if (!s.orig.b[0]) {
        int rc = dalloc(h, &s.orig.b[0], (size_t)s.cap); if (rc) return rc;
        rc = dalloc(h, &s.orig.b[1], (size_t)s.cap); if (rc) return rc;
        // existing particles: original position = current position
        HIPCHK(h, hipMemcpyAsync(s.orig.cur(), s.posv.cur(), sizeof(float4) * (size_t)h->n, hipMemcpyDeviceToDevice, s.stream));
    }
    s.has_dynamic_rigid = 1;
    return SPH_OK;
}

extern "C" int sph_append_particles(SphHandle *h, int object_id, int n, const float *pos, const float *vel,
                                    const float *density, const float *pressure, const int32_t *material,
                                    const int32_t *is_dynamic, const int32_t *color) {
    if (!h) return SPH_ERR_INVALID;
    if (n < 0 || object_id < -1 || object_id >= SPH_MAX_OBJECTS) return fail(h, SPH_ERR_INVALID, "append: bad object id / count");
    if (n == 0) return SPH_OK;
    if (!pos || !vel || !density || !material || !is_dynamic) return fail(h, SPH_ERR_INVALID, "append: null array");
    { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    if (object_id >= 0 && object_id < SPH_NOBJ && h->el[object_id].state == 2)
        return fail(h, SPH_ERR_UNSUPPORTED, "append: object %d is an elastic solid whose rest configuration has been captured", object_id);
    if (h->n + n > h->st.cap) return fail(h, SPH_ERR_CAPACITY, "append: %d + %d exceeds particle_max_num %d", h->n, n, h->st.cap);
    const int id0 = next_id(h);   // (= h->n until a particle has been removed: outflow)
    if (id0 + n > h->st.cap) return fail(h, SPH_ERR_CAPACITY, "append: %d particles created so far + %d exceed particle_max_num %d (ids of removed particles are not reused)", id0, n, h->st.cap);
    if (h->em_n > 0) {
        if (em_of_object(h, object_id) >= 0) return fail(h, SPH_ERR_UNSUPPORTED, "append: object %d belongs to emitter %d (an emitter's object takes no other particles)", object_id, em_of_object(h, object_id));
        if ((long long)id0 + n + em_reserved(h) > (long long)h->st.cap)
            return fail(h, SPH_ERR_CAPACITY, "append: %d + %d + the emitters' reserved %lld exceed particle_max_num %d", id0, n, em_reserved(h), h->st.cap);
    }
    HIPCHK(h, hipSetDevice(h->device));
    State &s = h->st;
    const float V0 = (float)h->prm.V0;
    std::vector<float4> hp(n), hv(n), ho;
    std::vector<int> hm(n), hid(n);
    std::vector<unsigned> hc(n);
    std::vector<float> hr(n), hpr(n);
    bool any_dyn_rigid = false;
    int nfl = 0;
    const int ix0 = h->perm[0], ix1 = h->perm[1], ix2 = h->perm[2];   // scene frame -> library frame
    for (int k = 0; k < n; ++k) {
        // base_container.py:404 add_particle
        hp[k] = make_float4(pos[3 * k + ix0], pos[3 * k + ix1], pos[3 * k + ix2], V0);
        hv[k] = make_float4(vel[3 * k + ix0], vel[3 * k + ix1], vel[3 * k + ix2], V0 * density[k]);
        hm[k] = META_PACK(object_id, material[k], is_dynamic[k] ? 1 : 0);
        if (h->prepared && material[k] == SPH_MAT_RIGID) { hm[k] |= META_FRESH_BIT; h->fresh_state = 1; }
        hid[k] = id0 + k;
        unsigned r = color ? (unsigned)(color[3 * k] & 0xff) : 0, g = color ? (unsigned)(color[3 * k + 1] & 0xff) : 0,
                 b = color ? (unsigned)(color[3 * k + 2] & 0xff) : 0;
        hc[k] = r | (g << 8) | (b << 16);
        hr[k] = density[k];
        hpr[k] = pressure ? pressure[k] : 0.0f;
        if (material[k] == SPH_MAT_FLUID) {
            nfl++;
            if (!h->fluid_mass_seen) { h->fluid_mass_seen = true; h->fluid_mass0 = hv[k].w; }
            else if (hv[k].w != h->fluid_mass0) h->fluid_mass_uniform = false;
        }
        if (material[k] == SPH_MAT_RIGID && is_dynamic[k]) any_dyn_rigid = true;
    }
    if (any_dyn_rigid) { int rc = ensure_orig(h); if (rc) return rc; }
    HIPCHK(h, hipStreamSynchronize(s.stream));
    const size_t off = (size_t)h->n;
    HIPCHK(h, hipMemcpy(s.posv.cur() + off, hp.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(s.velm.cur() + off, hv.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(s.meta.cur() + off, hm.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(s.pid.cur() + off, hid.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(s.color.cur() + off, hc.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice));
    if (s.color_home) HIPCHK(h, hipMemcpy(s.color_home + (size_t)id0, hc.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice));   // (particle id = append index: hid above)
    HIPCHK(h, hipMemcpy(s.rho.cur() + off, hr.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(s.prs + off, hpr.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    if (s.orig.cur()) HIPCHK(h, hipMemcpy(s.orig.cur() + off, hp.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    if (s.heat_T_home) h->L->heat_fill(s, id0, n, heat_insert_T(h, object_id));   // (heat: the new rows start at their object's temperature)
    if (object_id >= 0 && object_id < SPH_NOBJ) {   // the id range of the object (ids = append order)
        if (h->obj_n[object_id] == 0) h->obj_first[object_id] = id0;
        else if (h->obj_first[object_id] + h->obj_n[object_id] != id0) h->obj_split[object_id] = true;
        h->obj_n[object_id] += n;
    }
    h->n += n;
    h->id_next = id0 + n;
    h->n_fluid += nfl;
    h->n_nonfluid += n - nfl;
    if (!h->prepared) h->rigid_volume_done = false;   // later arrivals: see fresh_state
    if (h->prepared) h->sort_dirty = true;
    s.masks_valid = 0;
    s.perm_n = -1; s.list_n = -1;
    h->cfl.stale = true;
    refresh_counts(h);
    return SPH_OK;
}

// persistent ids of the n particles appended last (a rank of a sharded scene numbers its particles with their global
// insertion indices, so that ids mean the same thing on every rank and in a single-GPU run)
// the ids stop being the append order (ids from outside, slab sharding's global ids): the sorted copy of the colours is brought up to
// date and the colours travel with the particles from now on
static void colors_leave_home(SphHandle *h) { h->L->sorted_color(h->st); h->st.color_home_ok = 0; }

extern "C" int sph_set_appended_ids(SphHandle *h, int n, const int32_t *ids) {
    if (h) { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    if (!h || !ids || n < 0 || n > h->n) return fail(h, SPH_ERR_INVALID, "set_appended_ids: bad arguments");
    if (n == 0) return SPH_OK;
    if (h->st.heat_on) return fail(h, SPH_ERR_UNSUPPORTED, "set_appended_ids: heat is on (its temperatures are stored by id, in append order)");
    if (h->st.mp_on) return fail(h, SPH_ERR_UNSUPPORTED, "set_appended_ids: the micropolar model is on (its angular velocities are stored by id, in append order)");
    if (h->st.el_marked) return fail(h, SPH_ERR_UNSUPPORTED, "set_appended_ids: an elastic object exists (its rest lists are stored by id, in append order)");
    if (h->em_n > 0) return fail(h, SPH_ERR_UNSUPPORTED, "set_appended_ids: an emitter is set (its held layers are found by id, in append order)");
    if (h->of_n > 0 || h->of_removed_any) return fail(h, SPH_ERR_UNSUPPORTED, "set_appended_ids: an outflow volume is set or particles have been removed (new ids come from the library's own counter)");
    h->st.ids_custom = 1;
    HIPCHK(h, hipSetDevice(h->device));
    colors_leave_home(h);
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    HIPCHK(h, hipMemcpy(h->st.pid.cur() + (size_t)(h->n - n), ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    return SPH_OK;
}

// The device integrator (sph_rigid.hpp) writes the float32 pose of its bodies on the device; before the host edits pose_h and uploads
// the whole struct again, those entries are brought back.
static int pose_refresh(SphHandle *h) {
    if (!h->rb_pose_stale) return SPH_OK;
    RigidPose dev;
    HIPCHK(h, hipMemcpyAsync(&dev, h->st.pose, sizeof(RigidPose), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    for (int o = 0; o < SPH_NOBJ; ++o) {
        if (!h->rb_h[o].registered && !h->rm_on[o]) continue;
        memcpy(h->pose_h.com[o], dev.com[o], sizeof(dev.com[o])); memcpy(h->pose_h.rot[o], dev.rot[o], sizeof(dev.rot[o]));
        memcpy(h->pose_h.vel[o], dev.vel[o], sizeof(dev.vel[o])); memcpy(h->pose_h.angvel[o], dev.angvel[o], sizeof(dev.angvel[o]));
    }
    h->rb_pose_stale = false;
    return SPH_OK;
}

static int upload_pose(SphHandle *h) {
    HIPCHK(h, hipMemcpyAsync(h->st.pose, &h->pose_h, sizeof(RigidPose), hipMemcpyHostToDevice, h->st.stream));
    HIPCHK(h, hipStreamSynchronize(h->st.stream));  // pose_h may change right after
    return SPH_OK;
}

extern "C" int sph_set_object(SphHandle *h, int object_id, int material, int is_dynamic) {
    if (!h || object_id < 0 || object_id >= SPH_MAX_OBJECTS) return fail(h, SPH_ERR_INVALID, "set_object: bad object id");
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = pose_refresh(h); if (rc) return rc; }
    h->pose_h.material[object_id] = material;
    if (material != 1) h->any_rigid_object = true;
    h->pose_h.is_dynamic[object_id] = is_dynamic ? 1 : 0;
    // a rank of a sharded scene may hold none of the body's particles now and receive them later as migrants (which carry
    // their rest positions): every rank that is told about the body keeps the array
    if (material == SPH_MAT_RIGID && is_dynamic) { int rc = ensure_orig(h); if (rc) return rc; }
    return upload_pose(h);
}

extern "C" int sph_set_rigid_pose(SphHandle *h, int o, const float *com, const float *rot9, const float *vel,
                                  const float *angvel, const float *com0) {
    if (!h || o < 0 || o >= SPH_MAX_OBJECTS || !com || !rot9 || !vel || !angvel) return fail(h, SPH_ERR_INVALID, "set_rigid_pose: bad argument");
    if (h->st.rigid_int_on && h->rb_h[o].registered)
        return fail(h, SPH_ERR_INVALID, "set_rigid_pose: object %d is moved by the device integrator (sph_set_rigid_body)", o);
    if (o < SPH_NOBJ && h->rm_on[o])
        return fail(h, SPH_ERR_INVALID, "set_rigid_pose: object %d is moved by its motion program (sph_set_rigid_motion)", o);
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = pose_refresh(h); if (rc) return rc; }
    // scene frame -> library frame: polar vectors P v, the axial angular velocity det(P) P w, the rotation P R P^T
    for (int a = 0; a < 3; ++a) {
        const int b = h->perm[a];
        h->pose_h.com[o][a] = com[b]; h->pose_h.vel[o][a] = vel[b]; h->pose_h.angvel[o][a] = h->axial * angvel[b]; if (com0) h->pose_h.com0[o][a] = com0[b];
        for (int q = 0; q < 3; ++q) h->pose_h.rot[o][3 * a + q] = rot9[3 * b + h->perm[q]];
    }
    h->pose_dirty = true;
    h->pose_given = true;
    return upload_pose(h);
}

extern "C" int sph_get_rigid_wrench(SphHandle *h, float *force, float *torque, int reset) {
    if (!h || !force || !torque) return fail(h, SPH_ERR_INVALID, "get_rigid_wrench: null");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->scal_h, h->st.scal, sizeof(DevScalars), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    // library frame -> scene frame: the force is polar (P^T f), the torque axial (det(P) P^T t)
    for (int o = 0; o < SPH_NOBJ; ++o)
        for (int a = 0; a < 3; ++a) {
            const int b = h->inv[a];
            force[3 * o + a] = (float)((double)h->scal_h->wrench[3 * o + b] / SPH_WRENCH_SCALE);
            torque[3 * o + a] = h->axial * (float)((double)h->scal_h->wrench[SPH_NOBJ * 3 + 3 * o + b] / SPH_WRENCH_SCALE);
        }
    if (h->st.slab_active && h->comm.nranks > 1) {
        // sharded scene: every rank holds the contributions of ITS fluid particles (SURVEY 8e "rigid coupling under sharding");
        // the body's wrench is their sum.  Collective: every rank calls this at the same point of the step (the host
        // rigid solver does, between sph_step_begin and sph_step_end).
        double w[2 * SPH_NOBJ * 3];
        for (int k = 0; k < SPH_NOBJ * 3; ++k) { w[k] = force[k]; w[SPH_NOBJ * 3 + k] = torque[k]; }
        { int rc = sph_comm_allreduce(h, w, 2 * SPH_NOBJ * 3, 0); if (rc) return rc; }   // one collective
        for (int k = 0; k < SPH_NOBJ * 3; ++k) { force[k] = (float)w[k]; torque[k] = (float)w[SPH_NOBJ * 3 + k]; }
    }
    if (reset)
        HIPCHK(h, hipMemsetAsync((char *)h->st.scal + offsetof(DevScalars, wrench), 0, sizeof(long long) * 2 * SPH_NOBJ * 3, h->st.stream));
    return SPH_OK;
}

extern "C" int sph_set_rigid_contact(SphHandle *h, int on, float distance, const float *wall_lo, const float *wall_hi) {
    if (!h) return SPH_ERR_INVALID;
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "set_rigid_contact: PBF moves no rigid body (PBF.py _step)");
    State &s = h->st;
    if (!on) { s.contact_on = 0; s.contact_solve_on = 0; return SPH_OK; }   // (the solver reads the table this pass fills)
    if (!(distance > 0.0f) || distance > s.c.grid_size)
        return fail(h, SPH_ERR_INVALID, "set_rigid_contact: distance %g outside (0, cell size %g]", (double)distance, (double)s.c.grid_size);
    if (!wall_lo != !wall_hi) return fail(h, SPH_ERR_INVALID, "set_rigid_contact: give both wall planes or neither");
    HIPCHK(h, hipSetDevice(h->device));
    if (!s.contact_table) {
        int rc = dalloc(h, &s.contact_table, (size_t)SPH_CT_KEYS * SPH_CT_VALUES); if (rc) return rc;
        rc = dalloc(h, &s.contact_pairs, 1); if (rc) return rc;
        rc = dalloc(h, &s.contact_part, (size_t)s.cap); if (rc) return rc;
    }
    ContactArgs a{};
    a.D = distance;
    a.walls = wall_lo ? 1 : 0;
    for (int k = 0; k < 3; ++k) {   // scene frame -> library frame
        a.lo[k] = wall_lo ? wall_lo[h->perm[k]] : 0.0f;
        a.hi[k] = wall_hi ? wall_hi[h->perm[k]] : 0.0f;
    }
    s.contact = a;
    s.contact_on = 1;
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- PBF variant
extern "C" int sph_set_pbf_variant(SphHandle *h, const SphPbfParams *p) {
    if (!h) return SPH_ERR_INVALID;
    if (!p) return fail(h, SPH_ERR_INVALID, "sph_set_pbf_variant: null argument");
    if (h->prm.method != SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_pbf_variant: not a PBF handle (method %d)", h->prm.method);
    if (h->prepared) return fail(h, SPH_ERR_INVALID, "sph_set_pbf_variant: legal between sph_create and sph_prepare only");
    if (p->variant != SPH_PBF_VARIANT_REFERENCE && p->variant != SPH_PBF_VARIANT_CONSISTENT)
        return fail(h, SPH_ERR_INVALID, "sph_set_pbf_variant: variant %d is neither 0 (reference) nor 1 (consistent)", p->variant);
    if (p->variant == SPH_PBF_VARIANT_CONSISTENT) {
        if (p->min_iterations < 1) return fail(h, SPH_ERR_INVALID, "sph_set_pbf_variant: min_iterations %d < 1", p->min_iterations);
        if (p->max_iterations < p->min_iterations)
            return fail(h, SPH_ERR_INVALID, "sph_set_pbf_variant: max_iterations %d < min_iterations %d", p->max_iterations, p->min_iterations);
        if (!(p->max_error > 0.0f) || !std::isfinite(p->max_error))
            return fail(h, SPH_ERR_INVALID, "sph_set_pbf_variant: max_error %g is not a positive finite number", (double)p->max_error);
        if (!(p->epsilon > 0.0f) || !std::isfinite(p->epsilon))
            return fail(h, SPH_ERR_INVALID, "sph_set_pbf_variant: epsilon %g is not a positive finite number", (double)p->epsilon);
        h->pbf = *p;
        h->st.pbf_eps = p->epsilon;
    } else {
        h->pbf.variant = SPH_PBF_VARIANT_REFERENCE;   // (the other fields mean nothing to PBF.py's fixed five iterations)
    }
    h->st.poly6 = h->pbf.variant == SPH_PBF_VARIANT_REFERENCE ? 1 : 0;   // the cubic spline in the shared passes of the consistent variant
    h->pbf_last.variant = h->pbf.variant;
    return SPH_OK;
}

extern "C" int sph_get_pbf_stats(SphHandle *h, SphPbfStats *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    if (h->prm.method != SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "sph_get_pbf_stats: not a PBF handle (method %d)", h->prm.method);
    *out = h->pbf_last;
    if (h->pbf.variant == SPH_PBF_VARIANT_REFERENCE) { out->iterations = h->steps > 0 ? SPH_PBF_ITERATIONS : 0; out->error = 0.0f; }
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- Akinci surface tension
#include "sph_surface_tension.hpp"
extern "C" int sph_set_surface_tension(SphHandle *h, const SphSurfaceTensionParams *p) {
    if (!h) return SPH_ERR_INVALID;
    if (!p) return fail(h, SPH_ERR_INVALID, "sph_set_surface_tension: null argument");
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_surface_tension: not on a PBF handle (either variant)");
    if (h->st.slab_active || h->comm.slab_ready)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_surface_tension: not on a sharded handle (the ghosts' normals would need an exchange)");
    if (p->method != SPH_SURFACE_TENSION_REFERENCE && p->method != SPH_SURFACE_TENSION_AKINCI)
        return fail(h, SPH_ERR_INVALID, "sph_set_surface_tension: method %d is neither 0 (reference) nor 1 (akinci)", p->method);
    if (!(p->gamma >= 0.0) || !std::isfinite(p->gamma)) return fail(h, SPH_ERR_INVALID, "sph_set_surface_tension: gamma %g is not a finite number >= 0", p->gamma);
    if (!(p->beta >= 0.0) || !std::isfinite(p->beta)) return fail(h, SPH_ERR_INVALID, "sph_set_surface_tension: beta %g is not a finite number >= 0", p->beta);
    State &s = h->st;
    if (p->method == SPH_SURFACE_TENSION_AKINCI) {
        HIPCHK(h, hipSetDevice(h->device));
        if (!s.st_normal) { int rc = dalloc(h, &s.st_normal, (size_t)s.cap); if (rc) return rc; }
        if (!s.st_acc && !s.np_acc_out) { int rc = dalloc(h, &s.st_acc, (size_t)s.cap); if (rc) return rc; }
    }
    s.st_akinci = p->method == SPH_SURFACE_TENSION_AKINCI ? 1 : 0;
    s.st_gamma = p->gamma; s.st_beta = p->beta; s.st_h = h->prm.support_radius;
    return SPH_OK;
}

extern "C" int sph_get_surface_tension(SphHandle *h, SphSurfaceTensionParams *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    out->method = h->st.st_akinci ? SPH_SURFACE_TENSION_AKINCI : SPH_SURFACE_TENSION_REFERENCE;
    out->gamma = h->st.st_gamma; out->beta = h->st.st_beta;
    return SPH_OK;
}

extern "C" int sph_surface_tension_kernels_host(double h, const float *r, int64_t n, float *C_out, float *A_out, int fast) {
    if (!(h > 0.0) || !std::isfinite(h)) return fail(nullptr, SPH_ERR_INVALID, "sph_surface_tension_kernels_host: h %g is not a positive finite number", h);
    if (n < 0) return fail(nullptr, SPH_ERR_INVALID, "sph_surface_tension_kernels_host: negative count");
    if (n > 0 && (!r || !C_out || !A_out)) return fail(nullptr, SPH_ERR_INVALID, "sph_surface_tension_kernels_host: null argument");
    const StSpline k = st_spline(h);
    for (int64_t i = 0; i < n; ++i) {
        C_out[i] = fast ? st_cohesion<true>(k, r[i]) : st_cohesion<false>(k, r[i]);
        A_out[i] = fast ? st_adhesion<true>(k, r[i]) : st_adhesion<false>(k, r[i]);
    }
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- micropolar vorticity model
#include "sph_micropolar.hpp"
extern "C" int sph_set_micropolar(SphHandle *h, const SphMicropolarParams *p) {
    if (!h) return SPH_ERR_INVALID;
    if (!p) return fail(h, SPH_ERR_INVALID, "sph_set_micropolar: null argument");
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_micropolar: not on a PBF handle (either variant)");
    if (h->st.slab_active || h->comm.slab_ready)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_micropolar: not on a sharded handle (the ghosts' angular velocities would need an exchange)");
    if (p->method != SPH_VORTICITY_NONE && p->method != SPH_VORTICITY_MICROPOLAR)
        return fail(h, SPH_ERR_INVALID, "sph_set_micropolar: method %d is neither 0 (none) nor 1 (micropolar)", p->method);
    if (!(p->nu_t >= 0.0) || !std::isfinite(p->nu_t)) return fail(h, SPH_ERR_INVALID, "sph_set_micropolar: nu_t %g is not a finite number >= 0", p->nu_t);
    if (!(p->zeta >= 0.0) || !std::isfinite(p->zeta)) return fail(h, SPH_ERR_INVALID, "sph_set_micropolar: zeta %g is not a finite number >= 0", p->zeta);
    if (!(p->theta_inv >= 0.0) || !std::isfinite(p->theta_inv))
        return fail(h, SPH_ERR_INVALID, "sph_set_micropolar: theta_inv %g is not a finite number >= 0", p->theta_inv);
    State &s = h->st;
    if (p->method == SPH_VORTICITY_MICROPOLAR) {
        if (s.ids_custom)
            return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_micropolar: particle ids were set from outside (sph_set_appended_ids / SPH_F_PARTICLE_ID): "
                                                "the angular velocities are stored by id and need the append order");
        HIPCHK(h, hipSetDevice(h->device));
        // (dalloc clears: the rows of particles appended later read zero until their first walk)
        if (!s.mp_w_home) { int rc = dalloc(h, &s.mp_w_home, (size_t)s.cap); if (rc) return rc; }
        if (!s.mp_w_sorted) { int rc = dalloc(h, &s.mp_w_sorted, (size_t)s.cap); if (rc) return rc; }
        if (!s.mp_acc) { int rc = dalloc(h, &s.mp_acc, (size_t)s.cap); if (rc) return rc; }
        if (!s.st_acc && !s.np_acc_out) { int rc = dalloc(h, &s.st_acc, (size_t)s.cap); if (rc) return rc; }
    }
    s.mp_on = p->method == SPH_VORTICITY_MICROPOLAR ? 1 : 0;
    s.mp_nu_t = p->nu_t; s.mp_zeta = p->zeta; s.mp_theta_inv = p->theta_inv;
    return SPH_OK;
}

extern "C" int sph_get_micropolar(SphHandle *h, SphMicropolarParams *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    out->method = h->st.mp_on ? SPH_VORTICITY_MICROPOLAR : SPH_VORTICITY_NONE;
    out->nu_t = h->st.mp_nu_t; out->zeta = h->st.mp_zeta; out->theta_inv = h->st.mp_theta_inv;
    return SPH_OK;
}

extern "C" int sph_micropolar_pair_host(const float *in, int64_t n, float *out, int fast) {
    if (n < 0) return fail(nullptr, SPH_ERR_INVALID, "sph_micropolar_pair_host: negative count");
    if (n > 0 && (!in || !out)) return fail(nullptr, SPH_ERR_INVALID, "sph_micropolar_pair_host: null argument");
    for (int64_t k = 0; k < n; ++k) {
        const float *q = in + 24 * k;
        MpSums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float cx, cy, cz;
        if (fast) mp_pair<true>(s, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13], q[14], q[15], q[16], q[17], q[18], q[19], q[20], q[21], q[22], q[23], cx, cy, cz);
        else mp_pair<false>(s, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13], q[14], q[15], q[16], q[17], q[18], q[19], q[20], q[21], q[22], q[23], cx, cy, cz);
        float *o = out + 6 * k;
        o[0] = s.ax; o[1] = s.ay; o[2] = s.az; o[3] = s.bx; o[4] = s.by; o[5] = s.bz;
    }
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- air drag and wind
#include "sph_drag.hpp"
// what sph_set_drag and the two host entries refuse in the values themselves
static int drag_check_values(SphHandle *h, const char *who, const SphDragParams *p) {
    if (p->method != SPH_DRAG_NONE && p->method != SPH_DRAG_GISSLER)
        return fail(h, SPH_ERR_INVALID, "%s: method %d is neither 0 (none) nor 1 (gissler)", who, p->method);
    if (!(p->k >= 0.0) || !std::isfinite(p->k)) return fail(h, SPH_ERR_INVALID, "%s: k %g is not a finite number >= 0", who, p->k);
    if (!(p->rho_air >= 0.0) || !std::isfinite(p->rho_air)) return fail(h, SPH_ERR_INVALID, "%s: rho_air %g is not a finite number >= 0", who, p->rho_air);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(p->air_velocity[a])) return fail(h, SPH_ERR_INVALID, "%s: air_velocity[%d] %g is not finite", who, a, p->air_velocity[a]);
    return SPH_OK;
}

extern "C" int sph_set_drag(SphHandle *h, const SphDragParams *p) {
    if (!h) return SPH_ERR_INVALID;
    if (!p) return fail(h, SPH_ERR_INVALID, "sph_set_drag: null argument");
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_drag: not on a PBF handle (either variant)");
    if (h->st.slab_active || h->comm.slab_ready)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_drag: not on a sharded handle (not done, although the walk would need the ghosts' positions only)");
    { int rc = drag_check_values(h, "sph_set_drag", p); if (rc) return rc; }
    State &s = h->st;
    if (p->method == SPH_DRAG_GISSLER) {
        DragHost hk;
        if (!drag_host_constants(h->prm.particle_radius, h->prm.density_0, p->rho_air, hk))
            return fail(h, SPH_ERR_INVALID, "sph_set_drag: omega^2 = %g <= 0 for radius %g and density %g (the droplet's oscillation is overdamped: "
                                            "the deformation model does not apply)", hk.omega2, h->prm.particle_radius, h->prm.density_0);
        HIPCHK(h, hipSetDevice(h->device));
        if (!s.dr_acc) { int rc = dalloc(h, &s.dr_acc, (size_t)s.cap); if (rc) return rc; }
        if (!s.dr_terms) { int rc = dalloc(h, &s.dr_terms, (size_t)s.cap); if (rc) return rc; }
        if (!s.st_acc && !s.np_acc_out) { int rc = dalloc(h, &s.st_acc, (size_t)s.cap); if (rc) return rc; }
    }
    s.dr_on = p->method == SPH_DRAG_GISSLER ? 1 : 0;
    s.dr_k = p->k; s.dr_rho_a = p->rho_air;
    s.dr_radius = h->prm.particle_radius; s.dr_rho_l = h->prm.density_0;
    for (int a = 0; a < 3; ++a) s.dr_u[a] = p->air_velocity[a];
    for (int a = 0; a < 3; ++a) s.dr_u_lib[a] = p->air_velocity[h->perm[a]];   // scene frame -> library frame
    return SPH_OK;
}

extern "C" int sph_get_drag(SphHandle *h, SphDragParams *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    out->method = h->st.dr_on ? SPH_DRAG_GISSLER : SPH_DRAG_NONE;
    out->k = h->st.dr_k; out->rho_air = h->st.dr_rho_a;
    for (int a = 0; a < 3; ++a) out->air_velocity[a] = h->st.dr_u[a];
    return SPH_OK;
}

extern "C" int sph_drag_constants_host(const SphDragParams *p, double radius, double rho0, double *out) {
    if (!p || !out) return fail(nullptr, SPH_ERR_INVALID, "sph_drag_constants_host: null argument");
    { int rc = drag_check_values(nullptr, "sph_drag_constants_host", p); if (rc) return rc; }
    if (!(radius > 0.0) || !std::isfinite(radius) || !(rho0 > 0.0) || !std::isfinite(rho0))
        return fail(nullptr, SPH_ERR_INVALID, "sph_drag_constants_host: radius %g and density %g must be finite numbers > 0", radius, rho0);
    DragHost hk;
    const bool ok = drag_host_constants(radius, rho0, p->rho_air, hk);
    out[0] = hk.L; out[1] = hk.inv_td; out[2] = hk.omega2; out[3] = hk.t_max; out[4] = hk.c_def; out[5] = hk.y_coeff; out[6] = hk.n23;
    out[7] = hk.re_coeff;
    if (!ok) return fail(nullptr, SPH_ERR_INVALID, "sph_drag_constants_host: omega^2 = %g <= 0 for radius %g and density %g", hk.omega2, radius, rho0);
    return SPH_OK;
}

extern "C" int sph_drag_particle_host(const SphDragParams *p, double radius, double rho0, int64_t n, const float *in, float *out, int fast) {
    if (!p) return fail(nullptr, SPH_ERR_INVALID, "sph_drag_particle_host: null argument");
    if (n < 0) return fail(nullptr, SPH_ERR_INVALID, "sph_drag_particle_host: negative count");
    if (n > 0 && (!in || !out)) return fail(nullptr, SPH_ERR_INVALID, "sph_drag_particle_host: null argument");
    { int rc = drag_check_values(nullptr, "sph_drag_particle_host", p); if (rc) return rc; }
    if (!(radius > 0.0) || !std::isfinite(radius) || !(rho0 > 0.0) || !std::isfinite(rho0))
        return fail(nullptr, SPH_ERR_INVALID, "sph_drag_particle_host: radius %g and density %g must be finite numbers > 0", radius, rho0);
    DragHost hk;
    if (!drag_host_constants(radius, rho0, p->rho_air, hk))
        return fail(nullptr, SPH_ERR_INVALID, "sph_drag_particle_host: omega^2 = %g <= 0 for radius %g and density %g", hk.omega2, radius, rho0);
    const DragConsts k = drag_consts(hk, radius, p->rho_air, p->k, p->air_velocity);
    for (int64_t r = 0; r < n; ++r) {
        const float *q = in + 6 * r;
        DragOut o;
        if (fast) drag_finish<true>(k, q[0], q[1], q[2], q[3], q[4], q[5], o);
        else drag_finish<false>(k, q[0], q[1], q[2], q[3], q[4], q[5], o);
        float *d = out + 7 * r;
        d[0] = o.ax; d[1] = o.ay; d[2] = o.az; d[3] = o.w; d[4] = o.cd; d[5] = o.a_un; d[6] = o.y;
    }
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- heat
#include "sph_thermal.hpp"
static int heat_upload_table(SphHandle *h) {
    State &s = h->st;
    if (!s.heat_obj_T) return SPH_OK;
    float tab[256];
    for (int b = 0; b < 256; ++b) tab[b] = h->heat_obj_has[b] ? (float)h->heat_obj_T_h[b] : HT_ADIABATIC;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(s.stream));   // (a walk in flight reads the table)
    HIPCHK(h, hipMemcpy(s.heat_obj_T, tab, sizeof(tab), hipMemcpyHostToDevice));
    return SPH_OK;
}

extern "C" int sph_set_thermal(SphHandle *h, const SphThermal *p) {
    if (!h) return SPH_ERR_INVALID;
    State &s = h->st;
    if (!p || p->method == SPH_THERMAL_NONE) { s.heat_on = 0; return SPH_OK; }   // (the values and the temperatures stay)
    if (p->method != SPH_THERMAL_CONDUCTION) return fail(h, SPH_ERR_INVALID, "sph_set_thermal: method %d is neither 0 (none) nor 1 (conduction)", p->method);
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_thermal: not on a PBF handle (either variant)");
    if (s.slab_active || h->comm.slab_ready)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_thermal: not on a sharded handle (the ghosts' temperatures would need an exchange)");
    if (!(p->alpha >= 0.0) || !std::isfinite(p->alpha)) return fail(h, SPH_ERR_INVALID, "sph_set_thermal: alpha %g is not a finite number >= 0", p->alpha);
    if (!(p->beta >= 0.0) || !std::isfinite(p->beta)) return fail(h, SPH_ERR_INVALID, "sph_set_thermal: beta %g is not a finite number >= 0", p->beta);
    if (!std::isfinite(p->t_ref)) return fail(h, SPH_ERR_INVALID, "sph_set_thermal: t_ref %g is not finite", p->t_ref);
    if (s.ids_custom)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_set_thermal: particle ids were set from outside (sph_set_appended_ids / SPH_F_PARTICLE_ID): "
                                            "the temperatures are stored by id and need the append order");
    s.heat_alpha = p->alpha; s.heat_beta = p->beta; s.heat_t_ref = p->t_ref;
    HIPCHK(h, hipSetDevice(h->device));
    // (each buffer on its own: a call that failed half way is finished by the next one)
    if (!s.heat_T_sorted) { int rc = dalloc(h, &s.heat_T_sorted, (size_t)s.cap); if (rc) return rc; }
    if (!s.heat_rate) { int rc = dalloc(h, &s.heat_rate, (size_t)s.cap); if (rc) return rc; }
    if (!s.heat_obj_T) { int rc = dalloc(h, &s.heat_obj_T, (size_t)256); if (rc) return rc; { int rc2 = heat_upload_table(h); if (rc2) return rc2; } }
    if (!s.heat_T_home) {   // the home array exists only once it holds every present particle's temperature
        // every particle present: its object's temperature, or t_ref (later ones: sph_append_particles, the emitters' slot)
        const size_t n = (size_t)h->n;
        std::vector<float> home((size_t)s.cap, (float)s.heat_t_ref);
        if (n) {
            std::vector<int> id(n), mt(n);
            HIPCHK(h, hipStreamSynchronize(s.stream));
            HIPCHK(h, hipMemcpy(id.data(), s.pid.cur(), n * 4, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(mt.data(), s.meta.cur(), n * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; ++i) {
                if (id[i] < 0 || id[i] >= s.cap) return fail(h, SPH_ERR_INVALID, "sph_set_thermal: particle id %d outside [0, %d)", id[i], s.cap);
                home[(size_t)id[i]] = heat_insert_T(h, META_OBJ(mt[i]));
            }
        }
        float *dev = nullptr;
        { int rc = dalloc(h, &dev, (size_t)s.cap); if (rc) return rc; }
        HIPCHK(h, hipMemcpy(dev, home.data(), (size_t)s.cap * 4, hipMemcpyHostToDevice));
        s.heat_T_home = dev;
    }
    s.heat_on = 1;
    return SPH_OK;
}

extern "C" int sph_get_thermal(SphHandle *h, SphThermal *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    out->method = h->st.heat_on ? SPH_THERMAL_CONDUCTION : SPH_THERMAL_NONE;
    out->alpha = h->st.heat_alpha; out->beta = h->st.heat_beta; out->t_ref = h->st.heat_t_ref;
    return SPH_OK;
}

extern "C" int sph_set_object_temperature(SphHandle *h, int object_id, double temperature, int has_T) {
    if (!h) return SPH_ERR_INVALID;
    if (object_id < -1 || object_id >= SPH_MAX_OBJECTS) return fail(h, SPH_ERR_INVALID, "sph_set_object_temperature: object id %d outside [-1, %d)", object_id, SPH_MAX_OBJECTS);
    if (has_T && !std::isfinite(temperature)) return fail(h, SPH_ERR_INVALID, "sph_set_object_temperature: temperature %g is not finite", temperature);
    if (has_T && !(fabs(temperature) < 1.0e38)) return fail(h, SPH_ERR_INVALID, "sph_set_object_temperature: temperature %g is outside (-1e38, 1e38)", temperature);
    h->heat_obj_has[object_id + 1] = has_T != 0;
    h->heat_obj_T_h[object_id + 1] = has_T ? temperature : 0.0;
    return heat_upload_table(h);
}

extern "C" int sph_heat_pair_host(const float *in, int64_t n, float *out, int fast) {
    if (n < 0) return fail(nullptr, SPH_ERR_INVALID, "sph_heat_pair_host: negative count");
    if (n > 0 && (!in || !out)) return fail(nullptr, SPH_ERR_INVALID, "sph_heat_pair_host: null argument");
    for (int64_t k = 0; k < n; ++k) {
        const float *q = in + 12 * k;
        out[k] = fast ? heat_pair<true>(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11])
                      : heat_pair<false>(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11]);
    }
    return SPH_OK;
}

extern "C" int sph_heat_finish_host(const float *in, int64_t n, float *out, int fast) {
    if (n < 0) return fail(nullptr, SPH_ERR_INVALID, "sph_heat_finish_host: negative count");
    if (n > 0 && (!in || !out)) return fail(nullptr, SPH_ERR_INVALID, "sph_heat_finish_host: null argument");
    for (int64_t k = 0; k < n; ++k) {
        const float *q = in + 12 * k;
        float *o = out + 5 * k;
        if (fast) heat_finish<true>(q[0], q[1], q[2], q[3], q[4], q[5], o, o + 1);
        else heat_finish<false>(q[0], q[1], q[2], q[3], q[4], q[5], o, o + 1);
        heat_buoyancy(q[6], q[5], q[7], q[8], q[9], q[10], o + 2);
    }
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- device rigid integrator (sph_rigid.hpp)
static int rigid_int_supported(SphHandle *h, const char *who) {
    if (h->prm.method == SPH_METHOD_PBF) return fail(h, SPH_ERR_UNSUPPORTED, "%s: PBF moves no rigid body (PBF.py _step)", who);
    if (h->st.slab_active) return fail(h, SPH_ERR_UNSUPPORTED, "%s: a sharded scene would need the wrench all-reduced inside the step", who);
    if (h->swap_axis) return fail(h, SPH_ERR_UNSUPPORTED, "%s: the library frame differs from the scene frame (axis order)", who);
    return SPH_OK;
}

static void rigid_int_list(SphHandle *h) {
    RigidIntArgs &a = h->st.rigid_int;
    a.nbodies = 0;
    for (int o = 0; o < SPH_NOBJ; ++o) if (h->rb_h[o].registered) a.ids[a.nbodies++] = o;
    for (int q = a.nbodies; q < SPH_NOBJ; ++q) a.ids[q] = -1;
}

extern "C" int sph_set_rigid_integrator(SphHandle *h, int on, const double *gravity, const double *wall_lo, const double *wall_hi) {
    if (!h) return SPH_ERR_INVALID;
    if (!on) { h->st.rigid_int_on = 0; h->st.contact_solve_on = 0; return SPH_OK; }   // (the solver is the integrator's launch)
    { int rc = rigid_int_supported(h, "set_rigid_integrator"); if (rc) return rc; }
    if (!gravity || !wall_lo || !wall_hi) return fail(h, SPH_ERR_INVALID, "set_rigid_integrator: null argument");
    RigidIntArgs &a = h->st.rigid_int;
    for (int k = 0; k < 3; ++k) { a.g[k] = gravity[k]; a.lo[k] = wall_lo[k]; a.hi[k] = wall_hi[k]; }
    a.dt = (double)h->st.c.dt;   // the float32 step the fluid passes use (the host solver's dt is that value too)
    rigid_int_list(h);
    h->st.rigid_int_on = 1;
    return SPH_OK;
}

extern "C" int sph_set_rigid_body(SphHandle *h, int o, double mass, const double *inertia_body, const double *com, const double *rot9,
                                  const double *vel, const double *angvel, const double *com0, const double *points, int npoints) {
    if (!h) return SPH_ERR_INVALID;
    if (o < 0 || o >= SPH_MAX_OBJECTS || !inertia_body || !com || !rot9 || !vel || !angvel || npoints < 0 || (npoints > 0 && !points) ||
        !(mass > 0.0) || !std::isfinite(mass))
        return fail(h, SPH_ERR_INVALID, "set_rigid_body: bad argument");
    { int rc = rigid_int_supported(h, "set_rigid_body"); if (rc) return rc; }
    if (h->rm_on[o]) return fail(h, SPH_ERR_INVALID, "set_rigid_body: object %d is moved by its motion program (sph_set_rigid_motion)", o);
    const double *m = inertia_body;
    double c[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                   m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                   m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};   // adjugate
    const double det = m[0] * c[0] + m[1] * c[3] + m[2] * c[6];
    double scale = 0.0;
    for (int q = 0; q < 9; ++q) scale = std::max(scale, fabs(m[q]));
    if (!std::isfinite(det) || !(fabs(det) > 1e-12 * scale * scale * scale))
        return fail(h, SPH_ERR_INVALID, "set_rigid_body: the inertia tensor of object %d is singular", o);
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = pose_refresh(h); if (rc) return rc; }
    State &s = h->st;
    if (!s.rigid_bodies) { int rc = dalloc(h, &s.rigid_bodies, (size_t)SPH_NOBJ); if (rc) return rc; }
    RigidBodyDev &b = h->rb_h[o];
    if (npoints > h->rb_cap[o]) {
        double *p = nullptr;
        int rc = dalloc(h, &p, (size_t)npoints * 3); if (rc) return rc;
        b.points = p; h->rb_cap[o] = npoints;
    }
    HIPCHK(h, hipStreamSynchronize(s.stream));
    if (npoints > 0) HIPCHK(h, hipMemcpy((void *)b.points, points, sizeof(double) * 3 * (size_t)npoints, hipMemcpyHostToDevice));
    b.npoints = npoints; b.registered = 1; b.mass = mass;
    for (int q = 0; q < 9; ++q) { b.inertia[q] = m[q]; b.inertia_inv[q] = c[q] / det; b.rot[q] = rot9[q]; }
    for (int k = 0; k < 3; ++k) { b.com[k] = com[k]; b.vel[k] = vel[k]; b.angvel[k] = angvel[k]; }
    HIPCHK(h, hipMemcpy(s.rigid_bodies + o, &b, sizeof(RigidBodyDev), hipMemcpyHostToDevice));
    rigid_int_list(h);
    // the float32 pose the particles see (sph_set_rigid_pose), applied by the next renew_rigid
    for (int k = 0; k < 3; ++k) {
        h->pose_h.com[o][k] = (float)com[k]; h->pose_h.vel[o][k] = (float)vel[k]; h->pose_h.angvel[o][k] = (float)angvel[k];
        if (com0) h->pose_h.com0[o][k] = (float)com0[k];
    }
    for (int q = 0; q < 9; ++q) h->pose_h.rot[o][q] = (float)rot9[q];
    h->pose_dirty = true;
    h->pose_given = true;
    return upload_pose(h);
}

extern "C" int sph_get_rigid_state(SphHandle *h, int o, double *com, double *rot9, double *vel, double *angvel) {
    if (!h) return SPH_ERR_INVALID;
    if (o < 0 || o >= SPH_MAX_OBJECTS || !h->rb_h[o].registered) return fail(h, SPH_ERR_INVALID, "get_rigid_state: object %d is not registered", o);
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    RigidBodyDev b;
    HIPCHK(h, hipMemcpyAsync(&b, h->st.rigid_bodies + o, sizeof(RigidBodyDev), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    for (int k = 0; k < 3; ++k) { if (com) com[k] = b.com[k]; if (vel) vel[k] = b.vel[k]; if (angvel) angvel[k] = b.angvel[k]; }
    if (rot9) for (int q = 0; q < 9; ++q) rot9[q] = b.rot[q];
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- scripted rigid bodies (sph_rigid_motion.hpp)
#include "sph_rigid_motion_eval.hpp"

// the program is in canonical form; the message names the field that is not
static int rigid_motion_check(SphHandle *h, const char *who, const SphRigidMotion *m) {
    auto fin3 = [](const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); };
    auto unit_or_zero = [](const double *v) {
        const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        return n2 == 0.0 || fabs(n2 - 1.0) <= 1e-12;
    };
    if (!std::isfinite(m->start)) return fail(h, SPH_ERR_INVALID, "%s: start is not finite", who);
    if (std::isnan(m->end) || !(m->end > m->start)) return fail(h, SPH_ERR_INVALID, "%s: end %g <= start %g", who, m->end, m->start);
    if (!fin3(m->pivot)) return fail(h, SPH_ERR_INVALID, "%s: pivot is not finite", who);
    if (m->nkeys < 0 || m->nkeys > SPH_RIGID_MOTION_MAX_KEYS)
        return fail(h, SPH_ERR_INVALID, "%s: keyframes: %d keys outside 0..%d", who, m->nkeys, SPH_RIGID_MOTION_MAX_KEYS);
    if (m->interpolation < 0 || m->interpolation > 1) return fail(h, SPH_ERR_INVALID, "%s: interpolation %d is neither 0 (linear) nor 1 (smooth)", who, m->interpolation);
    if (m->repeat < 0 || m->repeat > 2) return fail(h, SPH_ERR_INVALID, "%s: repeat %d is not 0 (hold), 1 (loop) or 2 (pingpong)", who, m->repeat);
    if (m->reserved != 0) return fail(h, SPH_ERR_INVALID, "%s: reserved != 0", who);
    for (int i = 0; i < m->nkeys; ++i) {
        if (!std::isfinite(m->key_times[i]) || !fin3(m->key_translations[i]) || !fin3(m->key_rotations[i]))
            return fail(h, SPH_ERR_INVALID, "%s: keyframes: key %d is not finite", who, i);
        if (i == 0 ? m->key_times[0] != 0.0 : !(m->key_times[i] > m->key_times[i - 1]))
            return fail(h, SPH_ERR_INVALID, "%s: keyframes: times must start at 0 and increase strictly (key %d)", who, i);
    }
    const double scalars[] = {m->frequency, m->phase, m->ramp, m->amplitude, m->angle, m->drift_rate};
    for (double v : scalars) if (!std::isfinite(v)) return fail(h, SPH_ERR_INVALID, "%s: a harmonic or drift parameter is not finite", who);
    if (!fin3(m->direction) || !fin3(m->axis) || !fin3(m->drift_velocity) || !fin3(m->drift_axis))
        return fail(h, SPH_ERR_INVALID, "%s: a harmonic or drift vector is not finite", who);
    if (m->frequency < 0.0) return fail(h, SPH_ERR_INVALID, "%s: frequency %g is negative", who, m->frequency);
    if (m->ramp < 0.0) return fail(h, SPH_ERR_INVALID, "%s: ramp %g is negative", who, m->ramp);
    if (!unit_or_zero(m->direction)) return fail(h, SPH_ERR_INVALID, "%s: direction is neither zero nor of unit length", who);
    if (!unit_or_zero(m->axis)) return fail(h, SPH_ERR_INVALID, "%s: axis is neither zero nor of unit length", who);
    if (!unit_or_zero(m->drift_axis)) return fail(h, SPH_ERR_INVALID, "%s: drift_axis is neither zero nor of unit length", who);
    return SPH_OK;
}

static void rigid_motion_list(SphHandle *h) {
    RigidMotionArgs &a = h->st.rigid_motion_args;
    a.nbodies = 0;
    for (int o = 0; o < SPH_NOBJ; ++o) if (h->rm_on[o]) a.ids[a.nbodies++] = o;
    for (int q = a.nbodies; q < SPH_NOBJ; ++q) a.ids[q] = -1;
    a.dt = (double)h->st.c.dt;   // the float32 step the fluid passes use
}

extern "C" int sph_set_rigid_motion(SphHandle *h, int o, const SphRigidMotion *program, const double *com_rest, const double *rot_rest,
                                    const double *com0) {
    if (!h) return SPH_ERR_INVALID;
    if (o < 0 || o >= SPH_MAX_OBJECTS || !program || !com_rest || !rot_rest) return fail(h, SPH_ERR_INVALID, "set_rigid_motion: bad argument");
    { int rc = rigid_int_supported(h, "set_rigid_motion"); if (rc) return rc; }
    { int rc = rigid_motion_check(h, "set_rigid_motion", program); if (rc) return rc; }
    if (h->cfl.on || h->cfl.irregular) return fail(h, SPH_ERR_UNSUPPORTED, "set_rigid_motion: the step size changes or has changed (sph_set_cfl / sph_set_time_step: a motion program is a closed form of k dt)");
    for (int q = 0; q < 9; ++q)
        if (!std::isfinite(rot_rest[q]) || !std::isfinite(com_rest[q % 3])) return fail(h, SPH_ERR_INVALID, "set_rigid_motion: the rest pose is not finite");
    if (h->rb_h[o].registered)
        return fail(h, SPH_ERR_INVALID, "set_rigid_motion: object %d is moved by the device integrator (sph_set_rigid_body)", o);
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = pose_refresh(h); if (rc) return rc; }
    State &s = h->st;
    if (!s.rigid_motion) { int rc = dalloc(h, &s.rigid_motion, (size_t)SPH_NOBJ); if (rc) return rc; }
    // the zero-velocity pose of the time the running step ends at: the next launch's backward differences start from there
    RigidMotionDev b;
    memset(&b, 0, sizeof(b));
    b.prog = *program;
    for (int k = 0; k < 3; ++k) b.com_rest[k] = com_rest[k];
    for (int q = 0; q < 9; ++q) b.rot_rest[q] = rot_rest[q];
    b.steps = (long long)h->steps + (h->in_step ? 1 : 0);
    rm_pose(&b.prog, b.com_rest, b.rot_rest, (double)b.steps * (double)s.c.dt, b.com, b.rot);
    b.registered = 1;
    HIPCHK(h, hipStreamSynchronize(s.stream));
    HIPCHK(h, hipMemcpy(s.rigid_motion + o, &b, sizeof(RigidMotionDev), hipMemcpyHostToDevice));
    h->rm_on[o] = true;
    rigid_motion_list(h);
    for (int k = 0; k < 3; ++k) {
        h->pose_h.com[o][k] = (float)b.com[k]; h->pose_h.vel[o][k] = 0.0f; h->pose_h.angvel[o][k] = 0.0f;
        if (com0) h->pose_h.com0[o][k] = (float)com0[k];
    }
    for (int q = 0; q < 9; ++q) h->pose_h.rot[o][q] = (float)b.rot[q];
    h->pose_dirty = true;
    h->pose_given = true;
    return upload_pose(h);
}

extern "C" int sph_get_rigid_motion_state(SphHandle *h, int o, SphRigidMotionState *out) {
    if (!h) return SPH_ERR_INVALID;
    if (!out) return fail(h, SPH_ERR_INVALID, "get_rigid_motion_state: null");
    if (o < 0 || o >= SPH_MAX_OBJECTS || !h->rm_on[o]) return fail(h, SPH_ERR_INVALID, "get_rigid_motion_state: object %d has no motion program", o);
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    // the record behind the program: state, consumed wrench, impulse sums, step count
    struct Tail { double com[3], rot[9], vel[3], angvel[3], force[3], torque[3], impulse[3], angular_impulse[3]; long long steps; } t;
    static_assert(offsetof(RigidMotionDev, steps) - offsetof(RigidMotionDev, com) == offsetof(Tail, steps), "record layout");
    HIPCHK(h, hipMemcpyAsync(&t, (const char *)(h->st.rigid_motion + o) + offsetof(RigidMotionDev, com), sizeof(Tail), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    for (int k = 0; k < 3; ++k) {
        out->com[k] = t.com[k]; out->vel[k] = t.vel[k]; out->angvel[k] = t.angvel[k]; out->force[k] = t.force[k]; out->torque[k] = t.torque[k];
        out->impulse[k] = t.impulse[k]; out->angular_impulse[k] = t.angular_impulse[k];
    }
    for (int q = 0; q < 9; ++q) out->rot[q] = t.rot[q];
    out->steps = (int64_t)t.steps;
    return SPH_OK;
}

extern "C" int sph_rigid_motion_eval_host(const SphRigidMotion *program, const double *com_rest, const double *rot_rest, double dt, int64_t k,
                                          SphRigidMotionState *out) {
    if (!program || !com_rest || !rot_rest || !out) return fail(nullptr, SPH_ERR_INVALID, "rigid_motion_eval_host: null argument");
    if (!(dt > 0.0) || !std::isfinite(dt) || k < 0) return fail(nullptr, SPH_ERR_INVALID, "rigid_motion_eval_host: dt must be positive and finite, k >= 0");
    { int rc = rigid_motion_check(nullptr, "rigid_motion_eval_host", program); if (rc) return rc; }
    memset(out, 0, sizeof(*out));
    rm_step(program, com_rest, rot_rest, dt, (long long)k, out->com, out->rot, out->vel, out->angvel);
    out->steps = k + 1;
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- device contact solver (sph_contact_solve.hpp)
extern "C" int sph_set_rigid_contact_solver(SphHandle *h, int on, double restitution, double friction, int iterations, double beta,
                                            double slop, double patch) {
    if (!h) return SPH_ERR_INVALID;
    State &s = h->st;
    if (!on) { s.contact_solve_on = 0; return SPH_OK; }
    { int rc = rigid_int_supported(h, "set_rigid_contact_solver"); if (rc) return rc; }
    if (!s.rigid_int_on) return fail(h, SPH_ERR_INVALID, "set_rigid_contact_solver: sph_set_rigid_integrator is off");
    if (!s.contact_on) return fail(h, SPH_ERR_INVALID, "set_rigid_contact_solver: sph_set_rigid_contact is off");
    if (iterations < 1 || iterations > 64) return fail(h, SPH_ERR_INVALID, "set_rigid_contact_solver: %d iterations outside 1..64", iterations);
    const double prm[5] = {restitution, friction, beta, slop, patch};
    for (double v : prm)
        if (!std::isfinite(v) || v < 0.0) return fail(h, SPH_ERR_INVALID, "set_rigid_contact_solver: parameter %g is negative or not finite", v);
    HIPCHK(h, hipSetDevice(h->device));
    if (!s.contact_rows) {
        int rc = dalloc(h, &s.contact_rows, (size_t)SPH_CT_KEYS * SPH_CS_ROW); if (rc) return rc;
        rc = dalloc(h, &s.contact_nrows, 1); if (rc) return rc;
    }
    s.contact_solve = ContactSolveArgs{restitution, friction, beta, slop, patch, iterations};
    s.contact_solve_on = 1;
    return SPH_OK;
}

extern "C" int sph_get_rigid_contact_rows(SphHandle *h, double *rows, int capacity, int *count) {
    if (count) *count = 0;
    if (!h || !count || capacity < 0 || (capacity > 0 && !rows)) return fail(h, SPH_ERR_INVALID, "get_rigid_contact_rows: bad argument");
    State &s = h->st;
    if (!s.contact_rows) return fail(h, SPH_ERR_INVALID, "get_rigid_contact_rows: sph_set_rigid_contact_solver was never enabled");
    HIPCHK(h, hipSetDevice(h->device));
    int n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, s.contact_nrows, sizeof(int), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(h, hipStreamSynchronize(s.stream));
    if (n < 0 || n > SPH_CT_KEYS) return fail(h, SPH_ERR_INVALID, "get_rigid_contact_rows: row count %d outside the table", n);
    *count = n;
    const int m = std::min(n, capacity);
    if (m == 0) return SPH_OK;
    std::vector<double> dev((size_t)m * SPH_CS_ROW);
    HIPCHK(h, hipMemcpyAsync(dev.data(), s.contact_rows, dev.size() * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(h, hipStreamSynchronize(s.stream));
    for (int r = 0; r < m; ++r)
        memcpy(rows + (size_t)r * SPH_CONTACT_ROW_VALUES, dev.data() + (size_t)r * SPH_CS_ROW, sizeof(double) * SPH_CONTACT_ROW_VALUES);
    return SPH_OK;
}

// the table in the scene frame: bin 2 a + s of library axis a is bin 2 perm[a] + s of the scene, vectors are permuted back like the wrench
static void contact_to_scene(const SphHandle *h, const unsigned long long *dev, double *out) {
    const size_t row = SPH_CT_VALUES;
    for (int A = 0; A < SPH_NOBJ; ++A)
        for (int B = 0; B < SPH_CT_PARTNERS; ++B)
            for (int b = 0; b < SPH_CT_BINS; ++b) {
                const int bs = 2 * h->perm[b / 2] + (b & 1);
                const int Bs = B >= 20 ? 20 + (2 * h->perm[(B - 20) / 2] + ((B - 20) & 1)) : B;
                const long long *v = (const long long *)dev + ((size_t)(A * SPH_CT_PARTNERS + B) * SPH_CT_BINS + b) * row;
                double *o = out + ((size_t)(A * SPH_CT_PARTNERS + Bs) * SPH_CT_BINS + bs) * row;
                o[0] = (double)v[0];
                for (int a = 0; a < 3; ++a) {
                    o[1 + a] = (double)v[1 + h->inv[a]] / SPH_WRENCH_SCALE;
                    o[4 + a] = (double)v[4 + h->inv[a]] / SPH_WRENCH_SCALE;
                }
                o[7] = (double)(unsigned long long)v[7] / SPH_WRENCH_SCALE;
            }
}

extern "C" int sph_get_rigid_contacts(SphHandle *h, double *table, int reset) {
    if (!h || !table) return fail(h, SPH_ERR_INVALID, "get_rigid_contacts: null");
    State &s = h->st;
    const size_t words = (size_t)SPH_CT_KEYS * SPH_CT_VALUES;
    if (!s.contact_table) return fail(h, SPH_ERR_INVALID, "get_rigid_contacts: sph_set_rigid_contact was never enabled");
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<unsigned long long> dev(words);
    HIPCHK(h, hipMemcpyAsync(dev.data(), s.contact_table, words * 8, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(h, hipStreamSynchronize(s.stream));
    contact_to_scene(h, dev.data(), table);
    if (s.slab_active && h->comm.nranks > 1) {
        // Collective, like the wrench: every rank walked its own targets.  The union of the non-empty keys first -- 4-bit digits, 12 keys
        // per double (a digit sums at most nranks <= 15 flags: no carry) -- then the sums and maxima of those keys only, 128 at a time.
        if (h->comm.nranks > 15) return fail(h, SPH_ERR_UNSUPPORTED, "get_rigid_contacts: more than 15 ranks");
        const int per = 12, nd = (SPH_CT_KEYS + per - 1) / per;
        std::vector<double> dig(nd, 0.0);
        for (int k = 0; k < SPH_CT_KEYS; ++k) if (table[(size_t)k * 8] > 0.0) dig[k / per] += (double)(1ll << (4 * (k % per)));
        for (int o = 0; o < nd; o += SHM_RED_MAX) { int rc = sph_comm_allreduce(h, dig.data() + o, std::min(SHM_RED_MAX, nd - o), 0); if (rc) return rc; }
        std::vector<int> keys;
        for (int k = 0; k < SPH_CT_KEYS; ++k) if (((long long)dig[k / per] >> (4 * (k % per))) & 15) keys.push_back(k);
        std::vector<double> sum(keys.size() * 7), mx(keys.size());
        for (size_t q = 0; q < keys.size(); ++q) {
            for (int v = 0; v < 7; ++v) sum[7 * q + v] = table[(size_t)keys[q] * 8 + v];
            mx[q] = table[(size_t)keys[q] * 8 + 7];
        }
        for (size_t o = 0; o < sum.size(); o += SHM_RED_MAX) { int rc = sph_comm_allreduce(h, sum.data() + o, (int)std::min((size_t)SHM_RED_MAX, sum.size() - o), 0); if (rc) return rc; }
        for (size_t o = 0; o < mx.size(); o += SHM_RED_MAX) { int rc = sph_comm_allreduce(h, mx.data() + o, (int)std::min((size_t)SHM_RED_MAX, mx.size() - o), 1); if (rc) return rc; }
        for (size_t q = 0; q < keys.size(); ++q) {
            for (int v = 0; v < 7; ++v) table[(size_t)keys[q] * 8 + v] = sum[7 * q + v];
            table[(size_t)keys[q] * 8 + 7] = mx[q];
        }
    }
    if (reset) HIPCHK(h, hipMemsetAsync(s.contact_table, 0, words * 8, s.stream));
    return SPH_OK;
}

extern "C" int sph_get_rigid_contact_pairs(SphHandle *h, int64_t *pairs) {
    if (!h || !pairs) return fail(h, SPH_ERR_INVALID, "get_rigid_contact_pairs: null");
    *pairs = 0;
    if (!h->st.contact_pairs) return SPH_OK;
    HIPCHK(h, hipSetDevice(h->device));
    unsigned long long r = 0;
    HIPCHK(h, hipMemcpyAsync(&r, h->st.contact_pairs, sizeof(r), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    *pairs = (int64_t)r;
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- profiling
static hipEvent_t get_event(SphHandle *h) {
    if (!h->ev_pool.empty()) { hipEvent_t e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

static void prof_resolve(SphHandle *h) {
    hipStreamSynchronize(h->st.stream);
    for (auto &s : h->prof) {
        for (auto &pr : s.pending) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { s.ms += ms; s.launches++; }
            h->ev_pool.push_back(pr.first); h->ev_pool.push_back(pr.second);
        }
        s.pending.clear();
    }
}

struct ProfScope {
    SphHandle *h; int k; hipEvent_t e1 = nullptr;
    ProfScope(SphHandle *h_, int k_) : h(h_), k(k_) {
        if (h->prof[k].on) {
            if (h->prof[k].pending.size() > 8192) prof_resolve(h);
            hipEvent_t e0 = get_event(h); e1 = get_event(h);
            hipEventRecord(e0, h->st.stream);
            h->prof[k].pending.push_back({e0, e1});
        }
    }
    ~ProfScope() { if (e1) hipEventRecord(e1, h->st.stream); }
};

extern "C" int sph_profile_enable(SphHandle *h, int kernel_id, int on) {
    if (!h || kernel_id >= SPH_K_COUNT_) return SPH_ERR_INVALID;
    for (int k = 0; k < SPH_K_COUNT_; ++k) if (kernel_id < 0 || kernel_id == k) h->prof[k].on = on != 0;
    return SPH_OK;
}
extern "C" int sph_profile_reset(SphHandle *h) {
    if (!h) return SPH_ERR_INVALID;
    hipSetDevice(h->device);
    prof_resolve(h);
    for (auto &s : h->prof) { s.launches = 0; s.ms = 0.0; }
    return SPH_OK;
}
extern "C" int sph_profile_read(SphHandle *h, int kernel_id, int64_t *launches, double *total_ms) {
    if (!h || kernel_id < 0 || kernel_id >= SPH_K_COUNT_) return SPH_ERR_INVALID;
    hipSetDevice(h->device);
    prof_resolve(h);
    if (launches) *launches = h->prof[kernel_id].launches;
    if (total_ms) *total_ms = h->prof[kernel_id].ms;
    return SPH_OK;
}

extern "C" int sph_device_info(SphHandle *h, char *name256, int *cu_count, int64_t *hbm_bytes) {
    if (!h) return SPH_ERR_INVALID;
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, h->device));
    // some driver stacks leave prop.name empty: report the architecture string alone then
    if (name256) { if (prop.name[0]) snprintf(name256, 256, "%s (%s)", prop.name, prop.gcnArchName); else snprintf(name256, 256, "%s, %d CUs", prop.gcnArchName, prop.multiProcessorCount); }
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return SPH_OK;
}

// device copy rate (read + write bytes per second) of `reps` D2D copies of `bytes` bytes, HIP events on the handle's stream
extern "C" int sph_measure_copy_rate(SphHandle *h, size_t bytes, int reps, double *gb_per_s) {
    if (!h || !gb_per_s || bytes < 4096 || reps < 1) return fail(h, SPH_ERR_INVALID, "measure_copy_rate: bad arguments");
    HIPCHK(h, hipSetDevice(h->device));
    void *a = nullptr, *b = nullptr;
    if (hipMalloc(&a, bytes) != hipSuccess || hipMalloc(&b, bytes) != hipSuccess) {
        if (a) hipFree(a);
        return fail(h, SPH_ERR_HIP, "measure_copy_rate: cannot allocate 2 x %zu bytes", bytes);
    }
    hipStream_t st = h->st.stream;
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    hipError_t e = hipMemsetAsync(a, 1, bytes, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, st);   // warm-up (page tables, clocks)
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int k = 0; k < reps && e == hipSuccess; ++k) e = hipMemcpyAsync((k & 1) ? a : b, (k & 1) ? b : a, bytes, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    h->ev_pool.push_back(e0); h->ev_pool.push_back(e1);
    hipFree(a); hipFree(b);
    if (e != hipSuccess || !(ms > 0.0f)) return fail(h, SPH_ERR_HIP, "measure_copy_rate: %s", hipGetErrorString(e));
    *gb_per_s = 2.0 * (double)bytes * reps / ((double)ms * 1e-3) / 1e9;
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- phases
static int check_async(SphHandle *h) {
    if (h->el_rc) { const int rc = h->el_rc; h->el_rc = 0; return rc; }   // (a capture inside this call's neighbour search failed: its message stands)
    if (h->st.state_error) { const int se = h->st.state_error; h->st.state_error = 0; return fail(h, SPH_ERR_INVALID, "internal state error %d (bit 0: a sort was scanned without a histogram of its own; bit 1: a density launch could not move the arrays its sort left to it; bit 2: a sort that drops removed particles met a hash made before they were marked)", se); }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, SPH_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return SPH_OK;
}

#include "sph_elastic_api.hpp"

// base_container.py:544 prepare_neighborhood_search
// rho_dead: the kernel the caller launches next rewrites every particle's density (Launch::scatter_stable)
// density_next: that kernel is Launch::density over every tile; the SortCarry returned goes into its DensityOpts (SPH_NO_SORT_CARRY=1: never asked for)
static SortCarry ph_neighbor_search(SphHandle *h, bool rho_dead = false, bool density_next = false) {
    State &s = h->st;
    SortCarry carry;
    const bool capture = s.el_pending && el_capture_due(h);   // (the capture reads meta and ids in sorted order: this sort leaves nothing to the density pass)
    // outflow: particles that carry the dead bit leave with this sort -- it files them into the graveyard cells behind the grid (the
    // launchers take a slab rank's route while State::drop_n is set), then the counts shrink
    const int drop = s.slab_active ? 0 : h->of_pending;
    s.drop_n = drop;
    { ProfScope p(h, SPH_K_HASH_COUNT); h->L->hash_count(s); }
    { ProfScope p(h, SPH_K_SCAN); h->L->scan(s); }
    { ProfScope p(h, SPH_K_SCATTER); if (h->prm.deterministic) carry = h->L->scatter_stable(s, rho_dead, density_next && !capture && !getenv("SPH_NO_SORT_CARRY")); else h->L->scatter(s); }
    h->sort_dirty = false;
    if (drop > 0) {
        s.drop_n = 0;
        h->n -= drop; h->n_fluid -= drop; h->of_pending = 0;
        if (h->n_mark > h->n) h->n_mark = h->n;
        refresh_counts(h);
    }
    if (capture) { const int rc = el_capture_pending(h); if (rc && !h->el_rc) h->el_rc = rc; }
    return carry;
}

// the same without the hash kernel: the push transport's classify / unpack kernels have hashed every particle already
static void ph_sort_hashed(SphHandle *h) {
    State &s = h->st;
    { ProfScope p(h, SPH_K_SCAN); h->L->scan(s); }
    { ProfScope p(h, SPH_K_SCATTER); if (h->prm.deterministic) h->L->scatter_stable(s, false, false); else h->L->scatter(s); }
    h->sort_dirty = false;
}

static void ph_rigid_volume(SphHandle *h) {
    // base_solver.py:106.  The reference runs it at the end of every step() (:696) on the grid of that step's sort.
    // Static boundaries: the sum only involves same-object (static) particles, so the value computed once after the
    // first sort is bit-identical to recomputing every step; with dynamic bodies it is recomputed after every sort.
    // Rigid particles appended after prepare() (late entryTime) carry META_FRESH: the reference's pass at the end of
    // their insertion step ran on a grid that did not contain them (WCSPH / PCISPH: V = 1 / W(0), set by post_insert;
    // DFSPH: they were sorted in before :317, with V = V0 from add_particle), and only the pass one step later saw them.
    if (!h->st.has_rigid) return;
    bool force = false;
    if (h->fresh_state == 2) { h->L->clear_fresh(h->st); h->fresh_state = 0; force = true; }
    else if (h->fresh_state == 1 && h->prm.method != SPH_METHOD_DFSPH) h->fresh_state = 2;   // this pass skips them (RigidVolumePass::begin)
    if (!force && h->rigid_volume_done && !h->st.has_dynamic_rigid) return;
    ProfScope p(h, SPH_K_RIGID_VOLUME);
    h->L->rigid_volume(h->st);
    h->rigid_volume_done = true;
}

static void step_begin(SphHandle *h) {
    State &s = h->st;
    s.c.stat_bank = (int)(h->steps & 1);   // cleared by the previous step's scan kernel (k_scan_lookback)
    // a pose pushed between two steps is NOT applied here: the reference reads the rigid_body_* fields in the middle of
    // _step() (renew_rigid_particle_state, WCSPH.py:43 / DFSPH.py:309 / PCISPH.py:183), after the fluid passes of the step --
    // step_second_half does that (pinned by the rigid_* fixtures, which write a pose between steps 1 and 2)
}

#include "sph_comm_api.hpp"
#include "sph_emitter_api.hpp"
#include "sph_outflow_api.hpp"
#include "sph_steps.hpp"
static int step_once(SphHandle *h);
static int finish_sync(SphHandle *h);
#include "sph_cfl_api.hpp"

static int read_scalars(SphHandle *h) {
    { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    if (h->loop_pub) {   // the sums of the last step's bank, added up on the device and published into pinned memory (sph_steps.hpp)
        StatsPub *pub = (StatsPub *)((char *)h->loop_pub + 64);
        const unsigned want = ++h->stats_seq;
        const int bank_d = h->steps > 0 ? (int)((h->steps - 1) & 1) : 0;
        hipLaunchKernelGGL(k_publish_stats, dim3(1), dim3(256), 0, h->st.stream, h->st.scal, bank_d, pub, want);
        if (spin_for(h->st, &pub->seq, want)) {
            h->last.pair_interactions = (int64_t)pub->pairs;
            h->last.pair_evaluations = (int64_t)pub->evals;
            h->last.lds_fallback_blocks = (int64_t)pub->fallback;
            return SPH_OK;
        }
    }
    HIPCHK(h, hipMemcpyAsync(h->scal_h, h->st.scal, sizeof(DevScalars), hipMemcpyDeviceToHost, h->st.stream));
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    unsigned long long pairs = 0, evals = 0, fb = 0;
    const int bank = h->steps > 0 ? (int)((h->steps - 1) & 1) : 0;   // bank of the last completed step
    for (int k = 0; k < SPH_STAT_SLOTS; ++k) {
        pairs += h->scal_h->pairs[bank][k]; evals += h->scal_h->evals[bank][k];
        fb += h->scal_h->fallback[bank][k];
    }
    h->last.pair_interactions = (int64_t)pairs;
    h->last.pair_evaluations = (int64_t)evals;
    h->last.lds_fallback_blocks = (int64_t)fb;
    return SPH_OK;
}

// Waiting for the stream and reading small results back (round 6; profiles/r06_sync_latency.txt).  What is slow on this runtime is not
// hipStreamSynchronize but a D2H copy issued on an IDLE stream: the 97 KB statistics copy of sph_get_stats cost ~0.3 ms per call once the same
// copy at the end of sph_step (issued while the step's kernels were still running, which hid its start-up) was taken away -- a synchronous C5
// step went 1.39 -> 1.75 ms.  The statistics are therefore added up on the device and published into pinned host memory like the solver
// loops' residuals (read_scalars -> k_publish_stats; sph_steps.hpp), no copy at all; sph_step / sph_step_end just wait.
// sph_synchronize -- the fence a caller times asynchronous steps with -- waits by the same publish + spin (ends ~30 us sooner than the
// interrupt-driven hipStreamSynchronize: C2 in the driver's 3 x 20-step configuration -0.5 %).
// sph_step / sph_step_end are synchronous on return; the statistics are brought over when somebody asks (sph_get_stats)
static int finish_sync(SphHandle *h) {
    { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    HIPCHK(h, hipStreamSynchronize(h->st.stream));
    return SPH_OK;
}

extern "C" int sph_prepare(SphHandle *h) {
    if (!h) return SPH_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->em_n > 0 && !h->prepared) { const int rc = ph_emit(h, 0); if (rc) return rc; }   // born(0), as insert_object does for entryTime <= 0
    refresh_counts(h);
    State &s = h->st;
    if (s.slab_active && h->prm.method == SPH_METHOD_IISPH)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_prepare: IISPH runs on one GPU only (no sharded IISPH solve: sph_comm_set_slab)");
    if (s.slab_active && h->prm.method == SPH_METHOD_PBF)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_prepare: PBF runs on one GPU only (no sharded PBF step: sph_comm_set_slab)");
    if (h->prm.viscosity_implicit && h->prm.method == SPH_METHOD_PBF)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_prepare: PBF with implicit viscosity is not supported (its CG walks would need the spiky gradient)");
    int rc = pose_refresh(h); if (rc) return rc;
    rc = upload_pose(h); if (rc) return rc;
    // base_solver.py:683 prepare: prepare_emitter, renew_rigid_particle_state, neighbour search,
    // compute_rigid_particle_volume (+ DFSPH.py:321 / PCISPH.py:188)
    { ProfScope p(h, SPH_K_MISC); h->L->prepare_emitter(s); h->L->renew_rigid(s); }
    h->pose_dirty = false;
    if (s.slab_active) {
        double n_own[2] = {(double)h->n, (double)h->n_fluid};   // before any ghost arrives: every particle is owned by exactly one rank
        rc = sph_comm_allreduce(h, n_own, 2, 0); if (rc) return rc;
        h->comm_n_global = (long long)n_own[0];
        h->comm_nfluid_global = (long long)n_own[1];
        // halo records carry the rest position (64 instead of 48 B) once the scene has a dynamic rigid body: all ranks agree
        // on that here, whoever was told about the body (later mismatches are caught by the record size in the message header)
        double dyn_rigid[1] = {s.orig.cur() ? 1.0 : 0.0};
        rc = sph_comm_allreduce(h, dyn_rigid, 1, 1); if (rc) return rc;
        if (dyn_rigid[0] > 0.0 && !s.orig.cur()) { rc = ensure_orig(h); if (rc) return rc; }
        rc = slab_neighbor_search(h); if (rc) return rc;
    }
    else ph_neighbor_search(h);
    h->rigid_volume_done = false;
    ph_rigid_volume(h);
    if (s.slab_active && s.has_rigid) {  // ghost copies of boundary particles must carry the volumes just computed
        rc = slab_neighbor_search(h); if (rc) return rc;
    }
    rc = method_prepare(h); if (rc) return rc;
    // the passes above counted into statistics bank 0, which the first step uses as well
    HIPCHK(h, hipMemsetAsync(s.scal, 0, sizeof(unsigned long long) * SPH_STAT_SLOTS, s.stream));
    HIPCHK(h, hipMemsetAsync((char *)s.scal + offsetof(DevScalars, evals), 0, sizeof(unsigned long long) * SPH_STAT_SLOTS, s.stream));
    HIPCHK(h, hipMemsetAsync((char *)s.scal + offsetof(DevScalars, fallback), 0, sizeof(unsigned long long) * SPH_STAT_SLOTS, s.stream));
    rc = check_async(h); if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(s.stream));
    if (h->cfl.on) { rc = cfl_reduce(h); if (rc) return rc; cfl_pending(h); }   // the first step size
    h->prepared = true;
    return SPH_OK;
}

// scripted bodies: their programs at t_k and t_{k+1}, their wrench words consumed -- before the integrator's launch, which clears the
// wrench words of the objects it does not own
static void ph_rigid_motion(SphHandle *h) {
    if (h->st.rigid_motion_args.nbodies <= 0) return;
    h->st.rigid_motion_args.k = (long long)h->steps;   // steps completed since sph_prepare, advanced where total_time is
    { ProfScope p(h, SPH_K_RIGID_MOTION); h->L->rigid_motion(h->st); }
    h->pose_dirty = true;
    h->rb_pose_stale = true;
}

// the rigid step of the device backend (bullet_solver.py:144-167 without the host): wrench -> state -> pose, between the halves of a step
static void ph_rigid_integrate(SphHandle *h) {
    ph_rigid_motion(h);
    if (!h->st.rigid_int_on || h->st.rigid_int.nbodies <= 0) return;
    // with the contact solver on, its launch takes the integrator's place: the table of this step's contact pass is its input
    if (h->st.contact_solve_on) { ProfScope p(h, SPH_K_RIGID_CONTACT_SOLVE); h->L->rigid_contact_solve(h->st); }
    else { ProfScope p(h, SPH_K_RIGID_INTEGRATE); h->L->rigid_integrate(h->st); }
    h->pose_dirty = true;
    h->rb_pose_stale = true;
}

extern "C" int sph_rigid_integrate(SphHandle *h) {
    if (!h) return SPH_ERR_INVALID;
    if (!h->in_step) return fail(h, SPH_ERR_INVALID, "sph_rigid_integrate outside sph_step_begin / sph_step_end");
    if (!h->st.rigid_int_on && h->st.rigid_motion_args.nbodies <= 0)
        return fail(h, SPH_ERR_INVALID, "sph_rigid_integrate: sph_set_rigid_integrator is off");
    { int rc = rigid_int_supported(h, "sph_rigid_integrate"); if (rc) return rc; }
    HIPCHK(h, hipSetDevice(h->device));
    ph_rigid_integrate(h);
    return check_async(h);
}

// First half of a step: everything the reference's _step() does before `self.rigid_solver.step()`.
static int step_first_half(SphHandle *h) {
    if (h->in_step) return fail(h, SPH_ERR_INVALID, "sph_step_begin: the previous step was not ended");
    { int rc = cfl_step_begin(h); if (rc) return rc; }
    step_begin(h);
    h->em_touch = em_slot_touches(h, (long long)h->steps + 1) || h->of_n > 0;   // (outflow: the slot may mark particles dead behind a hash)
    int rc;
    switch (h->prm.method) {
        case SPH_METHOD_WCSPH: rc = wcsph_step(h); break;                     // WCSPH.py:28-36 (:45 boundary fused into the position update)
        case SPH_METHOD_DFSPH: rc = dfsph_step_begin(h); break;
        case SPH_METHOD_IISPH: rc = iisph_step(h); break;                     // IISPH.py:204-220
        case SPH_METHOD_PBF:                                                  // PBF.py:145-158 (the whole _step: no rigid step, no insertion)
            rc = h->pbf.variant == SPH_PBF_VARIANT_CONSISTENT ? pbfc_step(h) : pbf_step(h); break;
        default: rc = pcisph_step(h); break;                                  // PCISPH.py:166-177
    }
    if (rc) return rc;
    // rigid contact, where the host reads the wrench: the rigid particles still sit where the last sort put them
    if (h->st.contact_on) { ProfScope p(h, SPH_K_RIGID_CONTACT); h->L->rigid_contact(h->st); }
    h->n_mark = h->n;
    h->in_step = true;
    return SPH_OK;
}

// Second half: renew_rigid_particle_state (:616) for a pose the host pushed in between, the boundary (and the stale-grid
// rigid volume) for particles the host appended in between, DFSPH's post-insertion passes, then step()'s tail.
static int step_second_half(SphHandle *h) {
    if (!h->in_step) return fail(h, SPH_ERR_INVALID, "sph_step_end without sph_step_begin");
    State &s = h->st;
    h->in_step = false;
    if (h->pose_dirty || h->fresh_state || h->prm.method != SPH_METHOD_WCSPH) { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    if (h->pose_dirty) { ProfScope p(h, SPH_K_MISC); h->L->renew_rigid(s); h->pose_dirty = false; }
    if (h->n > h->n_mark) {
        ProfScope p(h, SPH_K_MISC);
        h->L->post_insert(s, h->n_mark, h->prm.method != SPH_METHOD_DFSPH);
    }
    // fluid emitters: the insertion point of the step (the reference's insert_object()), behind the rigid integrator / motion launch of
    // the same slot.  k_emit applies the boundary itself; what it adds takes part in the next sort (DFSPH: the one right below)
    // outflow: between the emitters' hold and their emission -- a newborn particle is first tested one step later
    { int rc = ph_emit(h, (long long)h->steps + 1, 1); if (!rc) rc = ph_outflow(h, (long long)h->steps + 1); if (!rc) rc = ph_emit(h, (long long)h->steps + 1, 2); h->em_touch = false; if (rc) return rc; }
    // (late entry under sharding: every rank appended the part of the object that lies in its slab, possibly nothing; the
    //  host tells the library the object's whole size through sph_comm_add_global_count -- no collective per step)
    if (h->prm.method == SPH_METHOD_DFSPH) {
        int rc = dfsph_step_end(h); if (rc) return rc;
        if (h->fresh_state == 1) { h->fresh_state = 2; ph_rigid_volume(h); }  // base_solver.py:696 on the fresh grid: now it sees them
    } else if (h->fresh_state == 2) {
        // WCSPH / PCISPH, one step after the insertion: this step's sort took the new body in, so the reference's
        // end-of-step pass (:696) now finds its particles.  The cell lists of this step's sort are still right for the
        // rigid particles (static ones have not moved), which is all this pass looks at.
        ph_rigid_volume(h);
    }
    return cfl_step_end(h);   // the scene time and the step count advance; adaptive time stepping: the reduce and the next step size
}

static int step_once(SphHandle *h) {
    h->whole_step = true;
    int rc = step_first_half(h);
    h->whole_step = false;
#ifdef SPH_TEST_HOOKS
    // test-hook library only: SPH_TEST_FAIL_STEP=k makes the step with h->steps == k fail between its halves, ONCE -- what a device or
    // exchange error in the middle of a sph_step_async(n) looks like to the state machine (a hash made for a sort that will not come)
    {
        static int fail_at = getenv("SPH_TEST_FAIL_STEP") ? atoi(getenv("SPH_TEST_FAIL_STEP")) : -1;
        if (!rc && fail_at >= 0 && h->steps == fail_at) { fail_at = -1; h->in_step = false; rc = fail(h, SPH_ERR_INVALID, "SPH_TEST_FAIL_STEP: injected failure"); }
    }
#endif
    if (!rc) ph_rigid_integrate(h);   // the device rigid backend: the host has nothing to do between the halves
    if (!rc) rc = step_second_half(h);
    // a failed step may leave a hash made for a sort that will not come (NextHash: the WCSPH force pass for the next step's sort, the
    // DFSPH position update for this step's): the next sort, whoever asks for it, must hash for itself on a clean histogram
    if (rc && h->st.prehashed) { h->st.prehashed = 0; h->st.cell_count_clean = 0; h->st.hist_taken = 0; h->st.run_lists_filed = 0; }
    return rc;
}

extern "C" int sph_step_begin(SphHandle *h) {
    if (!h) return SPH_ERR_INVALID;
    if (!h->prepared) return fail(h, SPH_ERR_INVALID, "sph_step_begin before sph_prepare");
    HIPCHK(h, hipSetDevice(h->device));
    refresh_counts(h);
    int rc = step_first_half(h); if (rc) return rc;
    rc = slab_settle_if_needed(h); if (rc) return rc;   // the host may append next: it needs the count
    h->n_mark = h->n;
    return check_async(h);
}

extern "C" int sph_step_end(SphHandle *h) {
    if (!h) return SPH_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    refresh_counts(h);
    int rc = step_second_half(h); if (rc) return rc;
    outflow_settle(h);   // (what the slot marked leaves before the call returns; DFSPH's own sort has dropped it already)
    rc = check_async(h); if (rc) return rc;
    return finish_sync(h);
}

extern "C" int sph_step_async(SphHandle *h, int nsteps) {
    if (!h || nsteps < 0) return SPH_ERR_INVALID;
    if (!h->prepared) return fail(h, SPH_ERR_INVALID, "sph_step before sph_prepare");
    // the only check that keeps the pressure solves' stop tests (a read-back per batch) out of asynchronous steps
    if (h->prm.method != SPH_METHOD_WCSPH && h->prm.method != SPH_METHOD_PBF && h->prm.fixed_iterations <= 0)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_step_async needs wcsph, pbf or fixed_iterations > 0");
    if (h->prm.method == SPH_METHOD_PBF && h->pbf.variant == SPH_PBF_VARIANT_CONSISTENT && h->prm.fixed_iterations <= 0)
        return fail(h, SPH_ERR_UNSUPPORTED, "sph_step_async: the consistent PBF variant needs fixed_iterations > 0 (its stop test reads back)");
    if (h->of_n > 0) return fail(h, SPH_ERR_UNSUPPORTED, "sph_step_async: an outflow volume is set (the removed count is read back at every slot: sph_step)");
    if (h->cfl.on) return fail(h, SPH_ERR_UNSUPPORTED, "sph_step_async: the CFL mode is on (the largest speed is read back at every step: sph_step)");
    HIPCHK(h, hipSetDevice(h->device));
    refresh_counts(h);
    for (int k = 0; k < nsteps; ++k) {
        h->steps_to_follow = nsteps - 1 - k;   // (a sharded WCSPH step may start the next step's halo message behind its own force pass)
        int rc = step_once(h);
        h->steps_to_follow = 0;
        if (rc) return rc;   // (step_once drops a hash made for a sort that will not come)
    }
    return check_async(h);
}

extern "C" int sph_synchronize(SphHandle *h) {
    if (!h) return SPH_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->n_exact) return slab_settle(h);   // drains the stream (bounded) and brings the counts of the asynchronous steps back
    return loop_readback(h);   // (returns only when the stream has reached the kernel it appended)
}

extern "C" int sph_step(SphHandle *h, int nsteps) {
    if (!h || nsteps < 0) return SPH_ERR_INVALID;
    if (!h->prepared) return fail(h, SPH_ERR_INVALID, "sph_step before sph_prepare");
    HIPCHK(h, hipSetDevice(h->device));
    refresh_counts(h);
    for (int k = 0; k < nsteps; ++k) { int rc = step_once(h); if (rc) return rc; }
    outflow_settle(h);   // (what the last slot marked leaves before the call returns)
    int rc = check_async(h); if (rc) return rc;
    return finish_sync(h);
}

extern "C" int sph_run_phase(SphHandle *h, int phase) {
    if (!h) return SPH_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    refresh_counts(h);
    State &s = h->st;
    switch (phase) {
        case SPH_PH_NEIGHBOR_SEARCH: ph_neighbor_search(h); break;
        case SPH_PH_RIGID_VOLUME: h->rigid_volume_done = false; ph_rigid_volume(h); break;
        case SPH_PH_DENSITY: { ProfScope p(h, SPH_K_DENSITY); h->L->density(s, h->prm.method == SPH_METHOD_WCSPH, {}); } break;
        case SPH_PH_NON_PRESSURE: { int rc = run_non_pressure(h, false); if (rc) return rc; } break;   // (Akinci surface tension: on the STORED normals; micropolar model: + the STORED a_mp)
        case SPH_PH_SURFACE_NORMALS:
            if (!s.st_akinci) return fail(h, SPH_ERR_INVALID, "SPH_PH_SURFACE_NORMALS: the Akinci surface tension is off (sph_set_surface_tension)");
            ph_surface_normals(h);
            break;
        case SPH_PH_MICROPOLAR:
            if (!s.mp_on) return fail(h, SPH_ERR_INVALID, "SPH_PH_MICROPOLAR: the micropolar model is off (sph_set_micropolar)");
            ph_micropolar(h);
            break;
        case SPH_PH_EMIT:
            if (h->em_n <= 0) return fail(h, SPH_ERR_INVALID, "SPH_PH_EMIT: no emitter is set (sph_set_emitter)");
            if (!h->prepared) return fail(h, SPH_ERR_INVALID, "SPH_PH_EMIT before sph_prepare");
            { const int rc = ph_emit(h, (long long)h->steps); if (rc) return rc; }
            break;
        case SPH_PH_OUTFLOW:
            if (h->of_n <= 0) return fail(h, SPH_ERR_INVALID, "SPH_PH_OUTFLOW: no outflow volume is set (sph_set_outflow)");
            { const int rc = ph_outflow(h, (long long)h->steps); if (rc) return rc; }
            break;
        case SPH_PH_CFL: {
            if (!h->cfl.on) return fail(h, SPH_ERR_INVALID, "SPH_PH_CFL: the CFL mode is off (sph_set_cfl)");
            const bool stale = h->cfl.stale;   // (the pending step size is not computed again here: a stale maximum stays stale)
            const int rc = cfl_reduce(h);
            h->cfl.stale = h->cfl.stale || stale;
            if (rc) return rc;
        } break;
        case SPH_PH_DRAG:
            if (!s.dr_on) return fail(h, SPH_ERR_INVALID, "SPH_PH_DRAG: the air drag is off (sph_set_drag)");
            ph_drag(h);
            break;
        case SPH_PH_HEAT:
            if (!s.heat_on) return fail(h, SPH_ERR_INVALID, "SPH_PH_HEAT: heat is off (sph_set_thermal)");
            ph_heat(h);
            break;
        case SPH_PH_ELASTIC:
            if (!s.el_marked) return fail(h, SPH_ERR_INVALID, "SPH_PH_ELASTIC: no elastic object (sph_set_elastic_object)");
            ph_elastic(h);
            break;
        case SPH_PH_PRESSURE_INTEGRATE: { ProfScope p(h, SPH_K_PRESSURE_INTEGRATE); h->L->pressure_integrate(s); } break;
        case SPH_PH_RIGID_CONTACT: {
            if (!s.contact_on) return fail(h, SPH_ERR_INVALID, "SPH_PH_RIGID_CONTACT: sph_set_rigid_contact is off");
            HIPCHK(h, hipMemsetAsync(s.contact_part, 0, sizeof(float4) * (size_t)s.cap, s.stream));
            ProfScope p(h, SPH_K_RIGID_CONTACT); h->L->rigid_contact(s);
        } break;
        case SPH_PH_CG_PREPARE: case SPH_PH_CG_AP: case SPH_PH_CG_UPDATE_XR: case SPH_PH_CG_UPDATE_P: case SPH_PH_CG_END:
            { int rc = cg_run_phase(h, phase); if (rc) return rc; if (phase == SPH_PH_CG_END) { ph_micropolar_apply(h); ph_elastic_apply(h); ph_drag_apply(h); ph_heat_apply(h); } } break;   // (micropolar model: + the STORED a_mp; elastic solids: + the STORED a_el; air drag: + the STORED a_drag)
        default: { int rc = method_run_phase(h, phase); if (rc) return rc; }
    }
    int rc = check_async(h); if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(s.stream));
    return SPH_OK;
}

// ---------------------------------------------------------------------------------- state access
extern "C" int sph_particle_num(SphHandle *h) {
    if (!h) return SPH_ERR_INVALID;
    if (!h->n_exact) { hipSetDevice(h->device); const int rc = slab_settle(h); if (rc) return rc; }
    return h->n;
}
extern "C" int sph_fluid_particle_num(SphHandle *h) { return h ? h->n_fluid : SPH_ERR_INVALID; }

extern "C" int sph_get_stats(SphHandle *h, SphStats *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = read_scalars(h); if (rc) return rc;
    h->last.steps = h->steps;
    h->last.particle_num = h->n;
    h->last.fluid_particle_num = h->n_fluid;
    h->last.total_time = h->total_time;
    h->last.hash_launches = h->st.n_hash_launches;
    h->last.prehashed_sorts = h->st.n_prehashed_sorts;
    h->last.list_sorts = h->st.n_list_sorts;
    h->last.carried_sorts = h->st.n_carried_sorts;
    if (h->st.pbf_recentred) {   // the bank of the last completed step (or phase)
        unsigned long long r[2];
        HIPCHK(h, hipMemcpy(r, h->st.pbf_recentred, sizeof(r), hipMemcpyDeviceToHost));
        h->last.pbf_recentred = (int64_t)r[h->pbf_bank];
    }
    *out = h->last;
    return SPH_OK;
}

extern "C" int sph_get_cg_scalars(SphHandle *h, float *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    if (!h->prm.viscosity_implicit) return fail(h, SPH_ERR_UNSUPPORTED, "sph_get_cg_scalars: no implicit viscosity on this handle");
    HIPCHK(h, hipSetDevice(h->device));
    State &s = h->st;
    HIPCHK(h, hipStreamSynchronize(s.stream));
    float red[8];
    HIPCHK(h, hipMemcpy(red, &s.scal->red[0], sizeof(red), hipMemcpyDeviceToHost));
    out[0] = red[4]; out[1] = red[5]; out[2] = red[3];   // cg_alpha, cg_beta, cg_error
    return SPH_OK;
}

static const float4 *vec_field(SphHandle *h, int field) {
    State &s = h->st;
    switch (field) {
        case SPH_F_POSITION: case SPH_F_REST_VOLUME: return s.posv.cur();
        case SPH_F_VELOCITY: case SPH_F_MASS: return s.velm.cur();
        case SPH_F_ACCELERATION: return s.acc;
        case SPH_F_PRESSURE_ACCEL: return s.pacc;
        case SPH_F_PREDICTED_VEL: return s.pvel;
        case SPH_F_PREDICTED_POS: return h->pbf.variant == SPH_PBF_VARIANT_CONSISTENT ? s.pbf_old : s.ppos;   // consistent PBF: x*
        case SPH_F_CG_X: return s.cg_x;
        case SPH_F_ORIG_POSITION: return s.orig.cur() ? s.orig.cur() : s.posv.cur();
        case SPH_F_IISPH_DII: case SPH_F_IISPH_AII: return s.iisph_dii;     // (dii, aii)
        case SPH_F_IISPH_DIJ_PJ: case SPH_F_IISPH_SUM_I: return s.iisph_dij; // (dij_pj, sum_i)
        case SPH_F_PBF_OLD_POSITION: return h->pbf.variant == SPH_PBF_VARIANT_CONSISTENT ? nullptr : s.pbf_old;   // (x_old, sorted cell id); consistent variant: posv is the old position
        case SPH_F_RIGID_CONTACT_DN: case SPH_F_RIGID_CONTACT_COUNT: return s.contact_part;   // (sum of depth * n, contacts)
        case SPH_F_NON_PRESSURE_ACCEL: return s.acc_np ? s.acc_np : s.st_acc;   // (PCISPH, or the last Akinci pass / micropolar-mode pass of any method; null otherwise)
        case SPH_F_MICROPOLAR_ACCEL: return s.mp_acc;   // (allocated with the micropolar model; null otherwise)
        case SPH_F_DRAG_ACCEL: return s.dr_acc;         // (allocated with the air drag; null otherwise.  w = n_i: SPH_F_DRAG_TERMS)
        case SPH_F_SURFACE_NORMAL: return s.st_normal;   // (allocated with the Akinci surface tension; null otherwise)
        case SPH_F_CG_B: return s.cg_b;     // (implicit viscosity only; null otherwise)
        case SPH_F_CG_R: return s.cg_r;
        case SPH_F_CG_P: return s.cg_p;
        case SPH_F_CG_AP: return s.cg_Ap;
        case SPH_F_CG_V0: return s.cg_v0;
        default: return nullptr;
    }
}
static const float *scalar_field(SphHandle *h, int field) {
    State &s = h->st;
    switch (field) {
        case SPH_F_DENSITY: return s.rho.cur();
        case SPH_F_PRESSURE: return s.prs;
        case SPH_F_DFSPH_ALPHA: return s.alpha;
        case SPH_F_DFSPH_KAPPA: return s.kappa;
        case SPH_F_DFSPH_KAPPA_V: return s.kappa_v;
        case SPH_F_DENSITY_STAR: return s.rho_star;
        case SPH_F_DENSITY_DERIV: return s.rho_deriv;
        case SPH_F_DFSPH_KAPPA_NEXT: return s.kappa_next;
        case SPH_F_DFSPH_KAPPA_V_NEXT: return s.kappa_v_next;
        case SPH_F_DEBUG_CAPTURE: return s.rho_raw;   // (test-hook build: PcisphRhoStarPass::cap_prev points here)
        case SPH_F_PBF_LAMBDA: return s.pbf_lambda;
        default: return nullptr;
    }
}

extern "C" int sph_download(SphHandle *h, int field, void *dst, size_t bytes) {
    if (!h || !dst) return SPH_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    State &s = h->st;
    const size_t n = (size_t)h->n;
    HIPCHK(h, hipStreamSynchronize(s.stream));
    const bool is_vec3 = field == SPH_F_POSITION || field == SPH_F_VELOCITY || field == SPH_F_ACCELERATION ||
                         field == SPH_F_PRESSURE_ACCEL || field == SPH_F_PREDICTED_VEL || field == SPH_F_PREDICTED_POS ||
                         field == SPH_F_CG_X || field == SPH_F_ORIG_POSITION || field == SPH_F_IISPH_DII || field == SPH_F_IISPH_DIJ_PJ ||
                         field == SPH_F_PBF_OLD_POSITION || field == SPH_F_RIGID_CONTACT_DN || field == SPH_F_NON_PRESSURE_ACCEL ||
                         field == SPH_F_SURFACE_NORMAL || field == SPH_F_MICROPOLAR_ACCEL || field == SPH_F_DRAG_ACCEL || (field >= SPH_F_CG_B && field <= SPH_F_CG_V0);
    if (is_vec3) {
        const float4 *src = vec_field(h, field);
        if (!src) return fail(h, SPH_ERR_UNSUPPORTED, "download: field %d not allocated for this method", field);
        if (bytes != n * 12) return fail(h, SPH_ERR_INVALID, "download: field %d needs %zu bytes, got %zu", field, n * 12, bytes);
        std::vector<float4> tmp(n);
        HIPCHK(h, hipMemcpy(tmp.data(), src, n * sizeof(float4), hipMemcpyDeviceToHost));
        float *d = (float *)dst;
        const int ix0 = h->inv[0], ix1 = h->inv[1], ix2 = h->inv[2];   // library frame -> scene frame
        for (size_t i = 0; i < n; ++i) { const float v[3] = {tmp[i].x, tmp[i].y, tmp[i].z}; d[3 * i] = v[ix0]; d[3 * i + 1] = v[ix1]; d[3 * i + 2] = v[ix2]; }
        return SPH_OK;
    }
    if (field >= SPH_F_ELASTIC_ACCEL && field <= SPH_F_ELASTIC_ROTATION) return el_download(h, field, (float *)dst, bytes);
    if (field == SPH_F_DRAG_TERMS) {   // (n_i, w, C_D, A_un, y): scalars, no frame
        if (!s.dr_terms) return fail(h, SPH_ERR_UNSUPPORTED, "download: field %d not allocated (sph_set_drag)", field);
        if (bytes != n * 20) return fail(h, SPH_ERR_INVALID, "download: field %d needs %zu bytes, got %zu", field, n * 20, bytes);
        std::vector<float4> a(n), t(n);
        if (n) {
            HIPCHK(h, hipMemcpy(a.data(), s.dr_acc, n * sizeof(float4), hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(t.data(), s.dr_terms, n * sizeof(float4), hipMemcpyDeviceToHost));
        }
        float *d = (float *)dst;
        for (size_t i = 0; i < n; ++i) { d[5 * i] = a[i].w; d[5 * i + 1] = t[i].x; d[5 * i + 2] = t[i].y; d[5 * i + 3] = t[i].z; d[5 * i + 4] = t[i].w; }
        return SPH_OK;
    }
    if (field == SPH_F_TEMPERATURE) {   // at home by particle id -> the current order; a row that is not fluid: what its object is held at
        if (!s.heat_T_home) return fail(h, SPH_ERR_UNSUPPORTED, "download: field %d not allocated (sph_set_thermal)", field);
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "download: field %d needs %zu bytes, got %zu", field, n * 4, bytes);
        std::vector<float> home((size_t)s.cap);
        std::vector<int> id(n), mt(n);
        HIPCHK(h, hipMemcpy(home.data(), s.heat_T_home, (size_t)s.cap * 4, hipMemcpyDeviceToHost));
        if (n) {
            HIPCHK(h, hipMemcpy(id.data(), s.pid.cur(), n * 4, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(mt.data(), s.meta.cur(), n * 4, hipMemcpyDeviceToHost));
        }
        float *d = (float *)dst;
        for (size_t i = 0; i < n; ++i) {
            if (id[i] < 0 || id[i] >= s.cap) return fail(h, SPH_ERR_INVALID, "download: particle id %d outside [0, %d)", id[i], s.cap);
            d[i] = META_MAT(mt[i]) == SPH_MAT_FLUID ? home[(size_t)id[i]] : heat_insert_T(h, META_OBJ(mt[i]));
        }
        return SPH_OK;
    }
    if (field == SPH_F_TEMPERATURE_RATE) {
        if (!s.heat_rate) return fail(h, SPH_ERR_UNSUPPORTED, "download: field %d not allocated (sph_set_thermal)", field);
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "download: field %d needs %zu bytes, got %zu", field, n * 4, bytes);
        if (n) HIPCHK(h, hipMemcpy(dst, s.heat_rate, n * 4, hipMemcpyDeviceToHost));
        return SPH_OK;
    }
    if (field == SPH_F_ANGULAR_VELOCITY) {   // at home by particle id -> the current order; library frame -> scene frame, axial
        if (!s.mp_w_home) return fail(h, SPH_ERR_UNSUPPORTED, "download: field %d not allocated (sph_set_micropolar)", field);
        if (bytes != n * 12) return fail(h, SPH_ERR_INVALID, "download: field %d needs %zu bytes, got %zu", field, n * 12, bytes);
        std::vector<float4> home((size_t)s.cap);
        std::vector<int> id(n);
        HIPCHK(h, hipMemcpy(home.data(), s.mp_w_home, (size_t)s.cap * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(id.data(), s.pid.cur(), n * 4, hipMemcpyDeviceToHost));
        float *d = (float *)dst;
        const int ix0 = h->inv[0], ix1 = h->inv[1], ix2 = h->inv[2];
        for (size_t i = 0; i < n; ++i) {
            if (id[i] < 0 || id[i] >= s.cap) return fail(h, SPH_ERR_INVALID, "download: particle id %d outside [0, %d)", id[i], s.cap);
            const float4 w = home[(size_t)id[i]];
            const float v[3] = {w.x, w.y, w.z};
            d[3 * i] = h->axial * v[ix0]; d[3 * i + 1] = h->axial * v[ix1]; d[3 * i + 2] = h->axial * v[ix2];
        }
        return SPH_OK;
    }
    if (field == SPH_F_CG_DINV) {   // library frame -> scene frame on both indices
        if (!s.cg_dinv) return fail(h, SPH_ERR_UNSUPPORTED, "download: field %d not allocated for this method", field);
        if (bytes != n * 36) return fail(h, SPH_ERR_INVALID, "download: field %d needs %zu bytes, got %zu", field, n * 36, bytes);
        std::vector<float> tmp(n * 9);
        HIPCHK(h, hipMemcpy(tmp.data(), s.cg_dinv, n * 36, hipMemcpyDeviceToHost));
        float *d = (float *)dst;
        for (size_t i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) d[9 * i + 3 * a + b] = tmp[9 * i + 3 * h->inv[a] + h->inv[b]];
        return SPH_OK;
    }
    if (field == SPH_F_CG_AP_PARTS) {
        if (!s.cg_part) return fail(h, SPH_ERR_UNSUPPORTED, "download: field %d not allocated for this method", field);
        if (bytes != n * 36) return fail(h, SPH_ERR_INVALID, "download: field %d needs %zu bytes, got %zu", field, n * 36, bytes);
        std::vector<float4> tmp(n);
        float *d = (float *)dst;
        const int ix0 = h->inv[0], ix1 = h->inv[1], ix2 = h->inv[2];
        for (int g = 0; g < 3; ++g) {   // the parts lie s.cap apart (CgApPass::part_stride)
            HIPCHK(h, hipMemcpy(tmp.data(), s.cg_part + (size_t)g * s.cap, n * sizeof(float4), hipMemcpyDeviceToHost));
            float *dg = d + (size_t)g * n * 3;
            for (size_t i = 0; i < n; ++i) { const float v[3] = {tmp[i].x, tmp[i].y, tmp[i].z}; dg[3 * i] = v[ix0]; dg[3 * i + 1] = v[ix1]; dg[3 * i + 2] = v[ix2]; }
        }
        return SPH_OK;
    }
    if (field == SPH_F_REST_VOLUME || field == SPH_F_MASS || field == SPH_F_IISPH_AII || field == SPH_F_IISPH_SUM_I ||
        field == SPH_F_RIGID_CONTACT_COUNT) {
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "download: size mismatch");
        const float4 *src = vec_field(h, field);
        if (!src) return fail(h, SPH_ERR_UNSUPPORTED, "download: field %d not allocated for this method", field);
        std::vector<float4> tmp(n);
        HIPCHK(h, hipMemcpy(tmp.data(), src, n * sizeof(float4), hipMemcpyDeviceToHost));
        float *d = (float *)dst;
        for (size_t i = 0; i < n; ++i) d[i] = tmp[i].w;
        return SPH_OK;
    }
    if (const float *src = scalar_field(h, field)) {
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "download: size mismatch");
        HIPCHK(h, hipMemcpy(dst, src, n * 4, hipMemcpyDeviceToHost));
        return SPH_OK;
    }
    if (field == SPH_F_MATERIAL || field == SPH_F_OBJECT_ID || field == SPH_F_IS_DYNAMIC || field == SPH_F_GHOST) {
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "download: size mismatch");
        std::vector<int> tmp(n);
        HIPCHK(h, hipMemcpy(tmp.data(), s.meta.cur(), n * 4, hipMemcpyDeviceToHost));
        int32_t *d = (int32_t *)dst;
        for (size_t i = 0; i < n; ++i)
            d[i] = field == SPH_F_MATERIAL ? META_MAT(tmp[i]) : field == SPH_F_OBJECT_ID ? META_OBJ(tmp[i]) :
                   field == SPH_F_GHOST ? META_GHOST(tmp[i]) : META_DYN(tmp[i]);
        return SPH_OK;
    }
    if (field == SPH_F_PARTICLE_ID) {
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "download: size mismatch");
        HIPCHK(h, hipMemcpy(dst, s.pid.cur(), n * 4, hipMemcpyDeviceToHost));
        return SPH_OK;
    }
    if (field == SPH_F_COLOR) {
        if (bytes != n * 12) return fail(h, SPH_ERR_INVALID, "download: size mismatch");
        const unsigned *col = h->L->sorted_color(s); HIPCHK(h, hipStreamSynchronize(s.stream));
        std::vector<unsigned> tmp(n);
        HIPCHK(h, hipMemcpy(tmp.data(), col, n * 4, hipMemcpyDeviceToHost));
        int32_t *d = (int32_t *)dst;
        for (size_t i = 0; i < n; ++i) { d[3 * i] = tmp[i] & 0xff; d[3 * i + 1] = (tmp[i] >> 8) & 0xff; d[3 * i + 2] = (tmp[i] >> 16) & 0xff; }
        return SPH_OK;
    }
    if (field == SPH_F_GRID_ID) {
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "download: size mismatch");
        std::vector<float4> tmp(n);
        HIPCHK(h, hipMemcpy(tmp.data(), s.posv.cur(), n * sizeof(float4), hipMemcpyDeviceToHost));
        int32_t *d = (int32_t *)dst;
        // the REFERENCE's flat cell id: scene frame, whole grid (whatever this rank's slab or the library's axis order)
        const Consts &c = s.c;
        const int *gn = h->prm.grid_num;
        const int ix0 = h->inv[0], ix1 = h->inv[1], ix2 = h->inv[2];
        auto cc = [](float x, float gs, int nn) { int v = (int)(x / gs); v = v < 0 ? 0 : v; return v > nn - 1 ? nn - 1 : v; };
        for (size_t i = 0; i < n; ++i) {
            const float v[3] = {tmp[i].x, tmp[i].y, tmp[i].z};
            d[i] = (cc(v[ix0], c.grid_size, gn[0]) * gn[1] + cc(v[ix1], c.grid_size, gn[1])) * gn[2] + cc(v[ix2], c.grid_size, gn[2]);
        }
        return SPH_OK;
    }
    return fail(h, SPH_ERR_INVALID, "download: unknown field %d", field);
}

// The grid tables of the last sort, read only (include/sph_hip.h): no launch, no state flag touched -- in particular not l_sorted_color's.
extern "C" int sph_get_grid_layout(SphHandle *h, SphGridLayout *out) {
    if (!h || !out) return SPH_ERR_INVALID;
    if (h->st.slab_active) return fail(h, SPH_ERR_UNSUPPORTED, "get_grid_layout: a sharded handle (a slab's grid is local)");
    const State &s = h->st;
    memset(out, 0, sizeof(*out));
    out->nx = s.c.nx; out->ny = s.c.ny; out->nz = s.c.nz; out->G = s.c.G;
    out->scan_tile = 2048;   // (SCAN_TILE, sph_device.hpp; sph_create sizes scan_blocks by the same number)
    for (int k = 0; k < 3; ++k) out->axis_map[k] = h->perm[k];
    out->cell_size = s.c.grid_size;
    out->n = h->n;
    out->tiles = (h->n + 255) / 256;
    out->tile_header_ints = 20;   // (BLK_HDR_INTS, sph_device.hpp; sph_create sizes blk_hdr by the same number)
    out->tiles_valid = (s.perm_n == h->n && h->n > 0) ? 1 : 0;
    return SPH_OK;
}

extern "C" int sph_download_grid_table(SphHandle *h, int which, void *dst, size_t bytes) {
    if (!h || !dst) return SPH_ERR_INVALID;
    if (h->st.slab_active) return fail(h, SPH_ERR_UNSUPPORTED, "download_grid_table: a sharded handle (a slab's grid is local)");
    HIPCHK(h, hipSetDevice(h->device));
    const State &s = h->st;
    const size_t n = (size_t)h->n, tiles = (n + 255) / 256, tiles_cap = ((size_t)s.cap + 255) / 256;
    const void *src = nullptr;
    size_t want = 0;
    switch (which) {
        case SPH_GRID_CELL_START: src = s.cell_start; want = ((size_t)s.c.G + 1) * sizeof(int); break;
        case SPH_GRID_TILE_HEADER: src = s.blk_hdr; want = tiles * 20 * sizeof(int); break;
        case SPH_GRID_LANE_PERM: src = s.lane_perm; want = tiles * 256; break;
        case SPH_GRID_CELL_WORD: src = s.blk_hdr + tiles_cap * 20; want = n * sizeof(unsigned); break;   // behind the headers of all tiles (l_block_prep)
        default: return fail(h, SPH_ERR_INVALID, "download_grid_table: unknown table %d", which);
    }
    if (bytes != want) return fail(h, SPH_ERR_INVALID, "download_grid_table: table %d needs %zu bytes, got %zu", which, want, bytes);
    HIPCHK(h, hipStreamSynchronize(s.stream));
    if (want) HIPCHK(h, hipMemcpy(dst, src, want, hipMemcpyDeviceToHost));
    return SPH_OK;
}

extern "C" int sph_upload(SphHandle *h, int field, const void *src, size_t bytes) {
    if (!h || !src) return SPH_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = slab_settle_if_needed(h); if (rc) return rc; }
    State &s = h->st;
    const size_t n = (size_t)h->n;
    HIPCHK(h, hipStreamSynchronize(s.stream));
    s.masks_valid = 0;  // state edited from outside
    h->cfl.stale = true;
    float4 *vdst = nullptr;
    bool w_only = false;
    switch (field) {
        case SPH_F_POSITION: vdst = s.posv.cur(); break;
        case SPH_F_VELOCITY: vdst = s.velm.cur(); break;
        case SPH_F_REST_VOLUME: vdst = s.posv.cur(); w_only = true; break;
        case SPH_F_MASS: vdst = s.velm.cur(); w_only = true; h->fluid_mass_uniform = false; refresh_counts(h); break;
        case SPH_F_CG_X: vdst = s.cg_x; break;
        case SPH_F_PREDICTED_POS: if (h->pbf.variant == SPH_PBF_VARIANT_CONSISTENT) vdst = s.pbf_old; break;   // x* (the phase tests)
        default: break;
    }
    if (vdst) {
        const size_t need = w_only ? n * 4 : n * 12;
        if (bytes != need) return fail(h, SPH_ERR_INVALID, "upload: field %d needs %zu bytes", field, need);
        std::vector<float4> tmp(n);
        HIPCHK(h, hipMemcpy(tmp.data(), vdst, n * sizeof(float4), hipMemcpyDeviceToHost));
        const float *f = (const float *)src;
        const int ix0 = h->perm[0], ix1 = h->perm[1], ix2 = h->perm[2];   // scene frame -> library frame
        for (size_t i = 0; i < n; ++i) {
            if (w_only) tmp[i].w = f[i];
            else { tmp[i].x = f[3 * i + ix0]; tmp[i].y = f[3 * i + ix1]; tmp[i].z = f[3 * i + ix2]; }
        }
        HIPCHK(h, hipMemcpy(vdst, tmp.data(), n * sizeof(float4), hipMemcpyHostToDevice));
        return SPH_OK;
    }
    if (field == SPH_F_ELASTIC_ROTATION) return el_upload_rotation(h, (const float *)src, bytes);
    if (field == SPH_F_TEMPERATURE) {   // the current order -> home by particle id; fluid rows only
        if (!s.heat_T_home) return fail(h, SPH_ERR_UNSUPPORTED, "upload: field %d not allocated (sph_set_thermal)", field);
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "upload: field %d needs %zu bytes", field, n * 4);
        std::vector<float> home((size_t)s.cap);
        std::vector<int> id(n), mt(n);
        HIPCHK(h, hipMemcpy(home.data(), s.heat_T_home, (size_t)s.cap * 4, hipMemcpyDeviceToHost));
        if (n) {
            HIPCHK(h, hipMemcpy(id.data(), s.pid.cur(), n * 4, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(mt.data(), s.meta.cur(), n * 4, hipMemcpyDeviceToHost));
        }
        const float *f = (const float *)src;
        for (size_t i = 0; i < n; ++i) {
            if (id[i] < 0 || id[i] >= s.cap) return fail(h, SPH_ERR_INVALID, "upload: particle id %d outside [0, %d)", id[i], s.cap);
            if (META_MAT(mt[i]) != SPH_MAT_FLUID) continue;
            if (!std::isfinite(f[i])) return fail(h, SPH_ERR_INVALID, "upload: temperature %g of row %zu is not finite", f[i], i);
            home[(size_t)id[i]] = f[i];
        }
        HIPCHK(h, hipMemcpy(s.heat_T_home, home.data(), (size_t)s.cap * 4, hipMemcpyHostToDevice));
        return SPH_OK;
    }
    if (field == SPH_F_ANGULAR_VELOCITY) {   // the current order -> home by particle id; scene frame -> library frame, axial
        if (!s.mp_w_home) return fail(h, SPH_ERR_UNSUPPORTED, "upload: field %d not allocated (sph_set_micropolar)", field);
        if (bytes != n * 12) return fail(h, SPH_ERR_INVALID, "upload: field %d needs %zu bytes", field, n * 12);
        std::vector<float4> home((size_t)s.cap);
        std::vector<int> id(n), mt(n);
        HIPCHK(h, hipMemcpy(home.data(), s.mp_w_home, (size_t)s.cap * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(id.data(), s.pid.cur(), n * 4, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(mt.data(), s.meta.cur(), n * 4, hipMemcpyDeviceToHost));
        const float *f = (const float *)src;
        const int ix0 = h->perm[0], ix1 = h->perm[1], ix2 = h->perm[2];
        for (size_t i = 0; i < n; ++i) {
            if (id[i] < 0 || id[i] >= s.cap) return fail(h, SPH_ERR_INVALID, "upload: particle id %d outside [0, %d)", id[i], s.cap);
            if (META_MAT(mt[i]) != SPH_MAT_FLUID) continue;   // (only fluid carries one: the other rows stay zero)
            home[(size_t)id[i]] = make_float4(h->axial * f[3 * i + ix0], h->axial * f[3 * i + ix1], h->axial * f[3 * i + ix2], 0.0f);
        }
        HIPCHK(h, hipMemcpy(s.mp_w_home, home.data(), (size_t)s.cap * sizeof(float4), hipMemcpyHostToDevice));
        return SPH_OK;
    }
    if (field == SPH_F_PARTICLE_ID) {  // global ids when a scene is split over ranks
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "upload: size mismatch");
        if (s.heat_on) return fail(h, SPH_ERR_UNSUPPORTED, "upload: SPH_F_PARTICLE_ID while heat is on (its temperatures are stored by id, in append order)");
        if (s.mp_on) return fail(h, SPH_ERR_UNSUPPORTED, "upload: SPH_F_PARTICLE_ID while the micropolar model is on (its angular velocities are stored by id, in append order)");
        if (s.el_marked) return fail(h, SPH_ERR_UNSUPPORTED, "upload: SPH_F_PARTICLE_ID while an elastic object exists (its rest lists are stored by id, in append order)");
        if (h->em_n > 0) return fail(h, SPH_ERR_UNSUPPORTED, "upload: SPH_F_PARTICLE_ID while an emitter is set (its held layers are found by id, in append order)");
        if (h->of_n > 0 || h->of_removed_any) return fail(h, SPH_ERR_UNSUPPORTED, "upload: SPH_F_PARTICLE_ID while an outflow volume is set or after particles have been removed (new ids come from the library's own counter)");
        s.ids_custom = 1;
        colors_leave_home(h); HIPCHK(h, hipStreamSynchronize(s.stream));
        HIPCHK(h, hipMemcpy(s.pid.cur(), src, n * 4, hipMemcpyHostToDevice));
        return SPH_OK;
    }
    float *fdst = nullptr;
    switch (field) {
        case SPH_F_DENSITY: fdst = s.rho.cur(); break;
        case SPH_F_PRESSURE: fdst = s.prs; break;
        case SPH_F_PBF_LAMBDA: if (h->pbf.variant == SPH_PBF_VARIANT_CONSISTENT) fdst = s.pbf_lambda; break;
        default: break;
    }
    if (fdst) {
        if (bytes != n * 4) return fail(h, SPH_ERR_INVALID, "upload: size mismatch");
        HIPCHK(h, hipMemcpy(fdst, src, n * 4, hipMemcpyHostToDevice));
        return SPH_OK;
    }
    return fail(h, SPH_ERR_UNSUPPORTED, "upload: field %d is read-only", field);
}

// ---------------------------------------------------------------------------------- frame export (host code)
// replaces ti.tools.PLYWriter(...).add_vertex_pos(...).export_ascii(path) of run_simulation.py:139-144: n vertices, xyz f32[n][3]
extern "C" int sph_write_ply_ascii(const char *path, const float *xyz, int64_t n) {
    const int rc = sphexp::write_ply_ascii(path, xyz, n);
    return rc == 0 ? SPH_OK : (rc == -1 ? SPH_ERR_INVALID : SPH_ERR_UNSUPPORTED);
}
// the same file written in parts (sharded scenes: one part per rank, in rank order)
extern "C" int sph_write_ply_ascii_part(const char *path, const float *xyz, int64_t n, int64_t n_total, int first) {
    const int rc = sphexp::write_ply_ascii_part(path, xyz, n, n_total, first);
    return rc == 0 ? SPH_OK : (rc == -1 ? SPH_ERR_INVALID : SPH_ERR_UNSUPPORTED);
}
// the OBJ of a reconstructed surface (splashsurf's output in surface_reconstruction.py:8)
extern "C" int sph_write_obj_ascii(const char *path, const float *vertices, int64_t nv, const float *normals_or_NULL, const int32_t *triangles,
                                   int64_t nt) {
    const int rc = sphexp::write_obj_ascii(path, vertices, nv, normals_or_NULL, triangles, nt);
    return rc == 0 ? SPH_OK : (rc == -1 ? SPH_ERR_INVALID : SPH_ERR_UNSUPPORTED);
}
// str(np.float32(v)) into out (>= 48 bytes), returns its length: the number format of the PLY body, exported for the tests
extern "C" int sph_format_f32(float v, char *out) { return out ? sphexp::format_f32(v, out) : SPH_ERR_INVALID; }

// ---------------------------------------------------------------------------------- mesh -> particles (host code)
// replaces trimesh's `mesh.voxelized(pitch).fill().points` (base_container.py:641-642).  Call with out == NULL to get the
// count, then with a buffer of 3 * count floats.
extern "C" int sph_voxelize_mesh(const double *vertices, int n_vertices, const int32_t *faces, int n_faces, double pitch,
                                 float *out_xyz, int64_t capacity_points, int64_t *n_points) {
    if (!vertices || !faces || !n_points) return SPH_ERR_INVALID;
    for (int k = 0; k < 3 * n_faces; ++k) if (faces[k] < 0 || faces[k] >= n_vertices) return SPH_ERR_INVALID;
    std::vector<float> pts;
    if (sphvox::voxelize_fill(vertices, n_vertices, faces, n_faces, pitch, pts) != 0) return SPH_ERR_INVALID;
    *n_points = (int64_t)(pts.size() / 3);
    if (!out_xyz) return SPH_OK;
    if (capacity_points < *n_points) return SPH_ERR_CAPACITY;
    memcpy(out_xyz, pts.data(), pts.size() * sizeof(float));
    return SPH_OK;
}

// replaces `mesh.contains(points)` on the np.arange lattice of base_container.py:686-694: inside[(i*ny + j)*nz + k] = 1 if
// (xs[i], ys[j], zs[k]) lies inside the closed mesh
extern "C" int sph_points_in_mesh(const double *vertices, int n_vertices, const int32_t *faces, int n_faces, const double *xs,
                                  int nx, const double *ys, int ny, const double *zs, int nz, uint8_t *inside) {
    if (!vertices || !faces || !xs || !ys || !zs || !inside) return SPH_ERR_INVALID;
    for (int k = 0; k < 3 * n_faces; ++k) if (faces[k] < 0 || faces[k] >= n_vertices) return SPH_ERR_INVALID;
    return sphvox::contains_lattice(vertices, n_vertices, faces, n_faces, xs, nx, ys, ny, zs, nz, inside) == 0 ? SPH_OK : SPH_ERR_INVALID;
}

#include "sph_surface_api.hpp"
#include "sph_render_api.hpp"
#include "sph_render_trace_api.hpp"
#include "sph_encoder_api.hpp"
#include "sph_video_api.hpp"
#include "sph_png_api.hpp"
#include "sph_text_api.hpp"
#include "sph_foam_api.hpp"
