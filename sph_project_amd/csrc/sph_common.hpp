// sph_common.hpp -- host/device shared declarations of libsph_hip (gfx950 only).
//
// Data layout in HBM (all arrays have capacity particle_max_num, index = slot in the current
// cell-sorted order; cells linearised z-fastest as in the reference, lin = (cx*ny + cy)*nz + cz, so the
// 27 neighbour cells of a particle are 9 contiguous particle runs):
//   posv  float4  (x, y, z, rest volume V)       double-buffered (sort scatter / integration)
//   velm  float4  (vx, vy, vz, mass m)           double-buffered (sort scatter / v* update)
//   meta  int32   object_id+1 | material<<8 | is_dynamic<<10      } moved by the sort together with
//   pid   int32   insertion index (persistent particle id)        } color (r|g<<8|b<<16), rho and
//   rho   float   particle_densities                              } the rigid original positions
// Per-step scratch that the reference does not reorder either (base_container.py:506 list):
//   rho_raw, prs, ptm (= p / rho^2), acc, DFSPH alpha/kappa/..., PCISPH predicted state, CG vectors.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sph_hip.h"   // (SphRigidMotion: the program a scripted body's record holds)
#include <math.h>
#include "sph_outflow_eval.hpp"      // (OutflowDev: one outflow volume as the mark kernel takes it, by value)
#include <string.h>
#include "sph_cfl_eval.hpp"          // (adaptive time stepping: which particles count and how a speed is squared, kernel and host)

#define SPH_NOBJ 20
// IISPH.py:12-14: relaxation factor, stop threshold of the average density error, iteration cap
#define SPH_IISPH_OMEGA 0.2f
#define SPH_IISPH_ETA 0.001
#define SPH_IISPH_MAX_ITER 20
// PBF.py:11-13 (lambda_eps, corrK, corr_deltaQ_coeff) and :63 (refine iterations per step)
#define SPH_PBF_LAMBDA_EPS 100.0f
#define SPH_PBF_CORR_K 0.001f
#define SPH_PBF_CORR_DQ 0.3f
#define SPH_PBF_ITERATIONS 5

// meta packing
#define META_OBJ(m) (((m) & 0xff) - 1)
#define META_MAT(m) (((m) >> 8) & 0x3)
#define META_DYN(m) (((m) >> 10) & 0x1)
#define META_PACK(obj, mat, dyn) ((((obj) + 1) & 0xff) | (((mat) & 0x3) << 8) | (((dyn) & 1) << 10))
#define META_GHOST(m) (((m) >> 11) & 0x1)   /* slab sharding: copy of a neighbour rank's boundary particle */
#define META_DEAD(m) (((m) >> 12) & 0x1)    /* slab sharding: left this rank (or last step's ghost); sorted into the graveyard cell G */
#define META_FRESH(m) (((m) >> 13) & 0x1)   /* rigid particle appended after prepare(): the reference's end-of-step volume pass saw it on a stale grid */
#define META_FRESH_BIT (1 << 13)
#define META_ACTIVE_FLUID(m) ((((m) >> 8) & 0xB) == 1) /* material fluid and not a ghost */
#define META_SET_MAT(m, mat) (((m) & ~(0x3 << 8)) | (((mat) & 0x3) << 8))

struct Consts {
    int nx, ny, nz, G;      // grid the cell lists are built on (slab sharding: nx = own layers + ghost layers, see cx_off)
    // Slab sharding cuts the grid along ONE library axis (slab_axis) and builds the cell lists on the own layers + ghost layers only:
    //   slab_axis 2 (default): z, the FASTEST axis of the cell order lin = (cx ny + cy) nz + cz.  The three runs of an x-offset group of a
    //     thin slab overlap and are staged once (nbr_plan "chain"): at 12-24 layers per rank a step is 20-50 % cheaper than with
    //   slab_axis 0: x, the SLOWEST axis (the scene's z is mapped onto it at the C-ABI boundary, sph_api.hip set_axis_order): a rank's
    //     ghost / boundary / interior layers are contiguous index ranges, so boundary tiles can run first and interior ones while the halo
    //     flies -- built and measured in round 4 (profiles/r04_slab_layouts.txt): the split costs a workgroup lifetime per pass and the
    //     thin-slab staging advantage is lost; kept behind SPH_SLAB_LAYOUT=slow.
    // n?_glob = layers of the whole scene along the axis, c?_off = global layer of local layer 0 (0 for the axis that is not cut).
    int nx_glob, cx_off, nz_glob, cz_off, slab_axis;
    float grid_size;        // f32(dh): cell size
    float h, h2, inv_h;     // support radius, squared, reciprocal (fast build)
    float kW, kG;           // cubic spline constants (base_solver.py:57, :81)
    float kGh, Wd_poly;     // fast build: kG / h; kernel_W(particle diameter) / kW (the polynomial alone)
    float inv_h2;           // fast build: 1 / h^2
    float W0, Wd;           // kernel_W(0), kernel_W(particle diameter)
    float diameter2;
    float dt, inv_dt, rho0, inv_rho0, g_upper;
    int up_axis;            // library axis that holds the scene's y (gravitationUpper is a height: base_solver.py:18-23); 1 unless the axes are permuted
    float gx, gy, gz;
    float st;               // surface tension coefficient (0.01)
    float cv, cvb, visc_eps;// 2*(dim+2)*viscosity, ..*viscosity_b, 0.01*dh^2
    float pad, hix, hiy, hiz; // domain clamp
    float thr_kappa;        // DFSPH m_eps * dt
    float V0;
    float pcisph_k;
    int   n;                // particle_num
    int   all_fluid;        // no rigid / emitter particles in the container
    int   force_global;
    int   ghosts;           // slab sharding: ghost particles present (meta bit 11) even when all_fluid
    int   stat_bank;        // DevScalars bank the running step counts into (step parity)
    int   xcd_chunk;        // tile order of the neighbour passes (sph_device.hpp xcd_remap): 0 one contiguous eighth per XCD, C > 0 chunks of C tiles dealt round-robin
    int   run_grouping;     // which candidate runs form a staging group of k_nbr_pass (sph_device.hpp run_of): 0 x offsets, 1 outer runs mixed
    // slab sharding, device-resident counts (sph_halo.hpp SlabDyn): when set, the particle count lives in device memory
    // (the halo exchange changes it without the host looking) and `n` above is only the launch bound the grid was sized for
    const int *n_dev;
};

// particle_num as the kernels see it
__device__ __forceinline__ int live_n(const Consts &c) { return c.n_dev ? *c.n_dev : c.n; }

// z-slab sharding: per-step counts, kept on the device by the halo kernels (sph_halo.hpp) and mirrored into pinned host memory.
// status bits: see SLAB_ST_* below.
// Slab sharding files the particles a rank drops (last step's ghosts, migrants) behind its live particles: SPH_NGRAVE graveyard cells
// G .. G + SPH_NGRAVE - 1 behind the grid.  More than one because every run of dead lanes costs an atomic on its graveyard cell's
// counter, the dead sit in short runs all over the sorted order (the ghost cells at both ends of every z column), and atomics on ONE
// address are served one at a time: a single graveyard cell took the hash kernel from 8 to 50 us with two ranks (profiles/r04_two_ranks_*).
#define SPH_NGRAVE 64
// the three counters of a step message (records for the lower / upper rank, particles that die) sit in separate 128-byte lines of L2 and
// a bank (message parity) is HC_BANK ints: thousands of waves add to them per step, and atomics on one line are served one at a time
#define HC(k) ((k) * 32)
#define HC_BANK 128
struct SlabDyn {
    int n_app;       // particles while the step's sort runs: last step's + arrivals (dead ones still in)
    int n_live;      // after the sort: the dead ones (last step's ghosts, migrants that left) dropped
    int n_send[2];   // records sent to the lower / upper rank this step (migrants + boundary copies)
    int n_recv[2];   // records received from them
    int dropped;
    int longest;     // longest of the four messages (slot tables are reset up to here)
    int status;      // sticky: SLAB_ST_*
    unsigned seq;    // number of the step message these counts belong to
    int n_btiles;    // pinned mirror only: boundary tiles of the last sort (k_block_prep), sizes the boundary launches of the next steps
    unsigned wseq;   // pinned mirror only: 2 seq + 1 while the settle kernel writes the fields, 2 seq + 2 when they are complete (seqlock)
};
// Header of one step message.  TWO per inbox side, by message parity (round 5): the writer announces message m + 1 as soon as its own
// step is through -- it only needs the reader's message m for that, which the reader announced BEFORE consuming the writer's m.  With one
// header per side, a consuming kernel that is held up (a late workgroup; a process time-sliced off the GPU with 8 ranks on one device)
// met the number m + 1 and took m + 1's record count for the payload of m: records lost, or garbage appended
// (tests/test_hip_slab.py::test_c4_sharded_over_8_ranks..., 2 failures in ~35 runs, only inside the full suite).  The header of m is now
// overwritten by m + 2 only, which the lockstep argument of sph_halo.hpp already rules out while m is being consumed.
struct HaloRecHdr {
    unsigned seq;           // number of the message this header belongs to (stored last, system-scope release)
    int count, status, stride;   // records, the sender's status bits, float4 per record
};
struct HaloCtl {            // push transport: control block of one side of a rank's inbox, 256 bytes, written by that neighbour
    HaloRecHdr rec[2];      // step messages: header of message m in rec[m & 1]
    unsigned fld_seq;       // number of the last complete field message (its sizes are known to both sides: no header)
    int pad[55];
};
static_assert(sizeof(HaloCtl) == 256, "HaloCtl layout");
#define SLAB_ST_SEND_OVERFLOW 1   /* a face message of mine exceeds the message capacity */
#define SLAB_ST_PEER 2            /* a neighbour reported a failure in its message header */
#define SLAB_ST_STRIDE 4          /* the neighbour's record size differs from mine (dynamic rigid body not registered on every rank) */
#define SLAB_ST_CAPACITY 8        /* own + received particles exceed particle_max_num */
#define SLAB_ST_TIMEOUT 16        /* a neighbour's message did not arrive in time */
#define SLAB_ST_BOUND 32          /* particle count outran the launch bound of an asynchronous step */

// Device-side scalar block (zeroed / read back by the host)
#define SPH_STAT_SLOTS 2048  // statistics are striped over many words: ~20k same-address atomics per launch cost >200 us
struct DevScalars {
    // two banks: step k counts into bank k & 1 while its scan kernel clears the other one for step k + 1
    unsigned long long pairs[2][SPH_STAT_SLOTS];     // accepted pairs of a step weighted by the reference passes a walk stands for (sum over slots)
    unsigned long long evals[2][SPH_STAT_SLOTS];     // accepted pairs as evaluated (one per neighbour walk); separate 64-bit words: no carry between the two tallies
    unsigned long long fallback[2][SPH_STAT_SLOTS];  // neighbour runs that did not fit the LDS tile
    // rigid_body_forces, rigid_body_torques (base_container.py:161-162) as 64-bit FIXED POINT, 2^-32 N (N m) per unit: integer atomics
    // commute, so the accumulated wrench is bit-reproducible from run to run whatever order the workgroups finish in (the reference's f32
    // atomics -- and this code until round 3 -- are not); range +-2.1e9, resolution 2.3e-10.  Written by add_wrench (sph_passes.hpp).
    long long wrench[2 * SPH_NOBJ * 3];
#define SPH_WRENCH_SCALE 4294967296.0
    float red[8];                    // reduction results (errors, CG dots)
    int   flags[4];
};

struct RigidPose {  // rigid_body_* fields of the container (base_container.py:156-164)
    float com[SPH_NOBJ][3], com0[SPH_NOBJ][3], rot[SPH_NOBJ][9], vel[SPH_NOBJ][3], angvel[SPH_NOBJ][3];
    int   is_dynamic[SPH_NOBJ], material[SPH_NOBJ];
};

// slab sharding: what a pass needs to classify its own particles and store their records into the neighbours' inboxes (sph_halo_defs.hpp)
struct HaloSend {
    int on;                       // 0: the pass leaves the classification to k_halo_classify
    int z_lo, z_hi, has_down, has_up, cap, rs;
    float4 *dst[2];               // step-message regions of the neighbours' inboxes for the NEXT message
    int *counts;                  // its count bank: [0..1] records per side, [2] particles that die
    int *meta_w, *xidx;           // the particle's meta word (rewritten) and exchange tag
    const int *pid; const unsigned *color; const float4 *orig;
};

// What the WCSPH force pass needs to be the NEXT step's k_hash_count as well (round 5): it knows every particle's new position when it
// stores it, so it files the new cell id, takes the histogram atomic (one per run of equal cells among the tile's particles in sorted
// order, like k_hash_count) and leaves the arrival rank.  on = 0: the next step hashes as usual.
// Run lists of the deterministic sort (round 6, fourth session).  The lanes of a hashing wave are a few RUNS of particles that share a cell
// (wave_runs); whoever takes a run's histogram atomic also links the run into a per-cell list: one 64-bit exchange on head[cell] (sort epoch in
// the high word, so the heads are never reset: a head of another epoch is an empty list) and one record rec[first particle] = (previous head's
// first particle or -1, run length).  The sort then ranks every particle from its cell's list (k_sort_rank) -- the launch that used to file the
// records once the scan had said where (k_scatter_index) is gone.  The run that ARRIVES FIRST in its cell (its histogram atomic returned 0:
// at rest every run, in motion most) takes no second atomic: it leaves (first particle, length) in first[cell] by a plain store -- exactly one
// run per cell and sort does -- and only later arrivals chain themselves behind head[cell].  first[] needs no epoch: it is read for cells
// that hold several runs of this sort only, and such a cell has had its first arrival.  head == nullptr: off (slab sharding).
// ONE array holds both kinds of record -- rec[i] for i < first_off (the particle capacity), first[cell] = rec[first_off + cell] -- so that a
// hasher's store goes through one base pointer and an index chosen in registers (with two pointers in the kernel arguments the compiler
// fetched the chosen one by a dependent VECTOR load from the argument segment: one more round trip at the end of every force-pass workgroup).
struct RunList { unsigned long long *head; int2 *rec; int first_off; unsigned epoch; };
struct NextHash { int on; int *cellid, *rank, *cell_count, *tile_sum; RunList rl; };

// ... and what the WCSPH density pass needs to store (rho_raw, rho, p, p / rho^2) of its boundary particles straight into the field
// message of the neighbours' inboxes (the message k_halo_pack2<2> would gather afterwards): out[side] = that message's region, xidx = the
// exchange tags of this sort, dyn = this step's counts (the echo part of a message starts behind its n_send records)
struct HaloFieldSend { int on; float4 *out[2]; const int *xidx; const SlabDyn *dyn; };

// Rigid contact pass (sph_contact.hpp): contact distance D (the pitch bodies and box are sampled at), the domain planes of a scene
// without a domain box (library frame), and the table's shape: key = (A * SPH_CT_PARTNERS + B) * SPH_CT_BINS + bin, SPH_CT_VALUES words
#define SPH_CT_PARTNERS 26
#define SPH_CT_BINS 6
#define SPH_CT_VALUES 8
#define SPH_CT_KEYS (SPH_NOBJ * SPH_CT_PARTNERS * SPH_CT_BINS)
struct ContactArgs { float D; int walls; float lo[3], hi[3]; };

// Device rigid integrator (sph_rigid.hpp, the host's "device" rigid backend): the float64 state of one body, and what one launch needs --
// gravity, the walls no part of a body may cross, dt, and the object ids of the registered bodies (workgroup b integrates body ids[b])
struct RigidBodyDev {
    double com[3], rot[9], vel[3], angvel[3], mass, inertia[9], inertia_inv[9];
    const double *points;   // body-frame positions of the body's particles, 3 per point
    int npoints, registered;
};
struct RigidIntArgs { double g[3], lo[3], hi[3], dt; int nbodies; int ids[SPH_NOBJ]; };
// Device contact solver (sph_contact_solve.hpp, the host's "device_contact" rigid backend): ContactSolver's parameters -- restitution,
// friction, sweeps, the split impulses' share of the depth, the depth a resting contact keeps, the rolling-resistance radius
struct ContactSolveArgs { double e, mu, beta, slop, patch; int iterations; };
// one row of the solve, in doubles (layout: sph_contact_solve.hpp); its first SPH_CONTACT_ROW_VALUES are sph_get_rigid_contact_rows'
#define SPH_CS_ROW 36
// Scripted rigid bodies (sph_rigid_motion.hpp): the record of one body -- its program and rest pose, the float64 state the last launch
// left, the wrench it consumed and the impulse sums -- and what one launch needs: dt, the step count k (the launch evaluates t_k and
// t_{k+1}) and the object ids of the scripted bodies (wave b moves body ids[b])
struct RigidMotionDev {
    SphRigidMotion prog;
    double com_rest[3], rot_rest[9];
    double com[3], rot[9], vel[3], angvel[3];
    double force[3], torque[3], impulse[3], angular_impulse[3];
    long long steps;
    int registered, pad;
};
struct RigidMotionArgs { double dt; long long k; int nbodies; int ids[SPH_NOBJ]; };

// Fluid emitters (sph_emitter.hpp): the record of one emitter on the device -- its program and the lattice counts derived from it when it
// was set -- and the by-value tables of the two launches.  EmitArgs: the layers born in this slot, at most one per emitter (speed dt <=
// spacing / 2); first[q] = slot (= persistent id) of the layer's first particle, start[q] = its offset among the launch's threads.
// EmitHoldArgs: the held layers, at most SPH_EMITTER_MAX_HOLD per emitter, by the id of their first particle.
struct EmitterDev { SphEmitter e; int nu, nv, layer_n, max_layers; };
struct EmitArgs { double spacing; int nlayers, total; int emitter[SPH_MAX_EMITTERS], first[SPH_MAX_EMITTERS], id_first[SPH_MAX_EMITTERS], start[SPH_MAX_EMITTERS + 1]; double offset[SPH_MAX_EMITTERS]; };
#define SPH_EMIT_HOLD_ENTRIES (SPH_MAX_EMITTERS * SPH_EMITTER_MAX_HOLD)
// Outflow (sph_outflow.hpp): the volumes whose window holds the slot's step count, by value, in index order (the lowest index wins);
// the counters sit SPH_OUTFLOW_CTR_STRIDE unsigned apart (one 128-byte line each: atomics on one line are served one at a time), entry
// SPH_MAX_OUTFLOWS counts what k_outflow_mark_ids marked.  They only grow: the host keeps what it read last.
#define SPH_OUTFLOW_CTR_STRIDE 32
struct OutflowArgs { int nvol; OutflowDev v[SPH_MAX_OUTFLOWS]; };
// Adaptive time stepping (sph_cfl.hpp): two pairs of result words, SPH_CFL_BANK_STRIDE unsigned apart; in a pair the maximum of |v|^2 (its
// bit pattern) at 0 and the non-finite flag at SPH_CFL_WORD_STRIDE, each on a 128-byte line of its own.  A launch writes one pair and
// clears the other.
#define SPH_CFL_WORD_STRIDE 32
#define SPH_CFL_BANK_STRIDE 64
struct EmitHoldArgs { double spacing; int nlayers, id_lo, id_hi; int emitter[SPH_EMIT_HOLD_ENTRIES], id_base[SPH_EMIT_HOLD_ENTRIES]; double offset[SPH_EMIT_HOLD_ENTRIES]; };

// Surface reconstruction (sph_surface.hpp): the constants and device buffers of one SphSurface.  Coarse cells (= bricks of
// B^3 grid points) are counted from the absolute coarse coordinate cmin[] on a grid of cn[] cells that keeps one empty cell around the
// particles; coarse linear index (x * cn[1] + y) * cn[2] + z.
struct SurfDev {
    float h, h2, kW, kG, e, be, iso;   // support, support^2, 8 / (pi h^3), 6 kW / h, cube edge, coarse edge B e, iso value
    int B, P;                          // points per brick edge, B^3
    int cmin[3], cn[3], G;             // coarse grid frame
    int n, nb;                         // particles, active bricks
    float4 *xin;                       // [n] input positions (w unused)
    float4 *xtmp, *xs;                 // [n] binned in arrival order / in key order with w = V_j
    int *pcell, *pslot;                // [n] coarse cell and arrival slot of xin[i]
    int *cell_start;                   // [G + 1] particle counts -> their exclusive scan
    int *flag;                         // [G + 1] active-brick flags -> their exclusive scan (flag[G] = nb)
    int *brick_id;                     // [G] brick index of a coarse cell, -1 when inactive
    int *brick_cell;                   // [nb] coarse linear index of each brick (ascending)
    float *phi;                        // [nb * P] the field at every point of every active brick
    unsigned *edge;                    // [nb * P] (vertex offset inside the brick) << 11 | cube case << 3 | crossing mask of the point's 3 edges
    int *vbase, *tbase;                // [nb + 1] per-brick vertex / triangle counts -> their exclusive scans
    float *vert, *nrm;                 // [nv * 3]
    int *tri;                          // [nt * 3]
    int *bounds;                       // [7] min / max coarse coordinates of the particles, non-finite flag
    int *counter;                      // [1] particles compacted from a handle
    unsigned long long *pairs;         // [1] candidate pair tests of the field pass
    int *scan_tmp;                     // tile sums of surf_scan
    hipStream_t stream;
};
// Anisotropic kernels of the surface reconstruction (sph_surface_aniso.hpp): the clamp's constants and the per-particle
// kernel matrices, in the binned key order of SurfDev::xs.  A symmetric 3x3 is kept as (xx, xy, xz, yy, yz, zz).
struct SurfAnisoPrm { int min_nb; float inv_ratio, inv_scale; };   // min_neighbours, 1 / max_ratio, 1 / sparse_scale
struct SurfAniso {
    SurfAnisoPrm prm;
    double h;            // the support in double (the moments pass)
    float4 *am;          // [n] A: xx, xy, xz, yy
    float4 *an;          // [n] A: yz, zz; det A; the bits of N_i
    float *vol;          // [n] V_j = 1 / sum_k det A_k W(|A_k (x_j - x_k)|)
    int *cnt;            // [2] particles under the sparse rule, particles with a clamped ratio
};
// Surface post-processing (sph_surface_post.hpp): the mesh sizes and the buffers of the stage
struct SurfPost {
    int nv, nt;
    const int *tri;      // [nt * 3]
    int *raw;            // [nv + 1] 2 x incident triangles -> exclusive scan: a vertex's slot range
    int *cnt;            // [nv + 1] fill counters, then unique counts -> exclusive scan: the CSR offsets (off)
    int *slot;           // [6 nt] neighbour slots, sorted and deduplicated in place per vertex
    int *adj;            // [E] CSR neighbours
    int *maxdeg;         // [1]
    float *pc;           // [n] c_j per binned particle
    float *w;            // [nv] smoothing weight per vertex (null: 1)
    float norm;          // weights normalization
    float4 *a, *b;       // [nv] working copies (ping-pong)
};

// Diffuse particles (sph_foam.hpp): the constants and device buffers of one SphFoam.  The fluid set is binned into the
// object's own grid of edge h over the domain plus one border cell per side (cell coordinates are clamped into it); linear index
// (x * cn[1] + y) * cn[2] + z.  Inside a cell the particles are ordered by id, so the grid order is a function of the particle SET.
#define FOAM_CTR_WORDS 16
enum FoamCtr { FC_VISIT = 0, FC_ACCEPT = 3, FC_CLASS = 6, FC_DIED = 9, FC_BORN = 10, FC_DROPPED = 11, FC_COUNT = 12 };
struct FoamDev {
    float h, pr;                       // support radius 4 r, particle radius r
    float glo[3];                      // grid origin (the domain's lower corner)
    int cn[3], G;                      // cells per axis (border cells included), their product
    float lo[3], hi[3];                // the clamp box: a diffuse particle outside it is deleted
    float g[3];                        // gravity
    float ta_lo, ta_hi, wc_lo, wc_hi, e_lo, e_hi, k_ta, k_wc, life_lo, life_hi, k_b, k_d, nmin_h;
    int n_spray, n_bubble, max_pp;
    unsigned seed_lo, seed_hi, t;      // the random stream's seed, the foam step
    float dt;
    int n;                             // fluid particles of this step
    int nd, cap;                       // diffuse particles before this step, capacity
    float4 *xin, *vin; int *idin;      // [n] the fluid set in input order
    int *pcell, *pslot;                // [n] cell and arrival slot of input particle i
    int *cell_start;                   // [G + 1] counts -> their exclusive scan
    float4 *xt, *vt; int *idt, *srct;  // [n] binned, arrival order inside a cell (srct: input index)
    float4 *xs, *vs; int *ids, *src;   // [n] binned, id order inside a cell
    float4 *nrm;                       // [n] grid order: unit normal, w = 1 where the particle has one
    float4 *pot;                       // [n] grid order: ta, wc, e, n_d
    int *cnt;                          // [n + 1] children per fluid particle -> exclusive scan
    float4 *dx[2], *dv[2];             // [cap] diffuse particles: (xyz, life) and (velocity, class as int bits); [0] current, [1] compaction target
    unsigned long long *dkey[2];       // [cap]
    int *keep;                         // [cap + 1] survivor flags -> exclusive scan
    unsigned long long *ctr;           // [FOAM_CTR_WORDS] FoamCtr
    int *scan_tmp;                     // tile sums of the scans
    hipStream_t stream;
};

// Particle rendering (sph_render.hpp): camera, shading constants, the particle source and the frame buffers of one
// SphRender.  Source: pos[i] (xyz), id[i], colour col_home[id[i]] when col_home is set, else col[i] (r | g << 8 | b << 16; both null:
// white); meta null = every particle drawn, else object mask / ghosts / dead from META_*.  key[p] = (float_bits(t) << 32) | id.
#define RENDER_LINE_ID0 0xFFFFFFF0u
struct RenderDev {
    int W, H;
    float E[3], f[3], s[3], u[3];      // eye, forward, right, up (f x U normalised, s x f)
    float tx, ty;                      // tan(fov / 2) W / H, tan(fov / 2)
    float zn, r, r2;                   // near plane, sphere radius, r^2
    float light[3], lrgb[3], amb;      // point light - E in (s, u, f) coordinates, its colour, ambient
    unsigned bg, box;                  // background / box line colour (r | g << 8 | b << 16)
    int draw_box;
    float line[12][8];                 // box edge e, clipped at zn and projected (host, double): {major0, minor0, major1, minor1, 1/z0,
    int line_axis[12];                 //   1/z1, first step, last step} in continuous pixels (centre = integer + 0.5); axis 0: major = x,
                                       //   1: major = y, -1: not drawn
    int n;                             // particles of the source
    const float4 *pos;
    const int *meta, *id;
    const unsigned *col, *col_home;
    unsigned mask;                     // object mask (handle path)
    unsigned long long *key;           // [W H]
    unsigned char *rgb;                // [H][W][3]
    int *ids;                          // [W H] -1 background, -2 - edge, else the particle id
    int *large;                        // [n] particles whose screen bounds exceed RENDER_LARGE_PX pixels
    unsigned long long *cnt;           // [8] drawn, non-finite, large, atomics issued, covered pixels
    hipStream_t stream;
};

// Screen-space surface mode of a particle frame (sph_render_surface.hpp): the planes behind the frame's key plane and the
// integer constants of the depth stage.  base[p] = the winner's unshaded colour (r | g << 8 | b << 16) | RSURF_FLAG where the winner is a
// particle of a surface object, else 0.  q[k][p] = the quantised view depth of a surface pixel (units of u = r / 256, at most
// RSURF_QMAX), RSURF_SENT elsewhere.  cnt: [0] surface pixels, [1] window taps visited, [2] taps accepted, [3] pixels clamped at rmax --
// in RSURF_CNT_BANKS banks of 8 words, a workgroup adding to the bank of its index (thousands of waves adding to one word serialise in
// L2: the adds alone took longer than the passes); the host sums the banks.
#define RSURF_SENT 0xFFFFFFFFu
#define RSURF_QMAX 0x00FFFFFFu
#define RSURF_FLAG 0x01000000u
#define RSURF_RMAX_CAP 16
#define RSURF_CNT_BANKS 64
struct RenderSurfDev {
    unsigned *base;                    // [W H]
    unsigned *q[2];                    // [W H] each (ping-pong of the smoothing iterations)
    unsigned long long *cnt;           // [RSURF_CNT_BANKS][8]
    const unsigned char *pmask;        // points path: per-point surface flag (null: every point)
    unsigned omask;                    // handle path: surface objects
    int fluid_only;                    // handle path: ... and of these the fluid particles only (object_mask -1)
    float inv_u, u;                    // 256 / r and r / 256, each rounded to f32 once on the host
    unsigned rnum, dq;                 // R_i = clamp(rnum / q_i, 1, rmax); a tap counts when |q_j - q_i| <= dq
    int rmax;
    float dX, dY;                      // ray step per column / per row: 2 tx / W, -2 ty / H
    float spec, shin;
};

// Thickness mode of the surface frames (sph_render_thickness.hpp): the opaque layer -- a key / rgb plane pair with counters
// and a large list of its own, drawn from what is not a surface particle -- the thickness planes and the coefficients of the composite.
// T[0]: the splat's sums (units of u per pixel, view depth), T[1]: the first plane of the smoothing ping-pong, whose second is the idle
// depth plane of RenderSurfDev.  cnt: two groups of RSURF_CNT_BANKS banks of 8 words, banked as RenderSurfDev::cnt.  Group 0, the frame
// call: [0] adds issued, [1] pairs the opaque depth cut short, [2] pairs it removed.  Group 1, the surface call: [0] taps visited,
// [1] surface pixels whose summed thickness is 0, [2] the largest smoothed thickness (atomicMax).
#define RTHICK_MAX_PARTICLES (1 << 23)   // contributions of at most 512 each in a u32
struct RenderThickDev {
    unsigned long long *okey;          // [W H]
    unsigned char *orgb;               // [H][W][3]
    unsigned long long *ocnt;          // [8] the opaque layer's RenderDev::cnt
    int *olarge;                       // [n]
    unsigned *T[2];                    // [W H] each
    unsigned long long *cnt;           // [2][RSURF_CNT_BANKS][8]
    float absorb, scatter;
};

// Diffuse particles in the surface frames (sph_render_foam.hpp): the diffuse set, the three integer planes and the constants
// of the composite.  fo / fu: the summed chords of the diffuse spheres over / under the surface (units of u per pixel), du: the nearest
// start of an under chord below the surface (all ones: none).  key0: the frame's key plane as rend_run left it (a copy once the raw
// spheres are merged into the frame's), okey: the opaque layer's in thickness mode, else null.  cnt: two groups of RSURF_CNT_BANKS banks
// of 8 words, banked as RenderSurfDev::cnt.  Group 0, the frame call: [0] adds issued over, [1] under, [2] pairs the limit cut short,
// [3] pairs it removed.  Group 1, the surface call: [0] pixels with fo > 0, [1] with fu > 0.
struct RenderFoamDev {
    int n;                             // diffuse particles
    const float4 *pos;                 // [n] xyz
    int *large;                        // [n] spheres whose screen bounds exceed RENDER_LARGE_PX pixels
    unsigned long long *nlarge;        // [1] their number
    const unsigned long long *key0;    // [W H]
    const unsigned long long *okey;    // [W H] or null
    unsigned *fo, *fu, *du;            // [W H] each
    unsigned long long *cnt;           // [2][RSURF_CNT_BANKS][8]
    float rf, rf2;                     // the diffuse sphere's radius and its square
    float bias;                        // depth_bias r, rounded once on the host
    float density;
    unsigned rgb;                      // r | g << 8 | b << 16
};

// Mesh rendering (sph_render_mesh.hpp): the frame's meshes, concatenated.  Triangle g of the frame belongs to the last
// record with t0 <= g; its indices are local to that mesh's nv vertices, which start at slot v0 of vert / nrm.  The frame buffers,
// camera and counters are the RenderDev's: cnt[0] triangles that passed the hit test at some pixel centre (whether or not they won it), [1] non-finite, [2] large,
// [3] atomics issued, [4] covered pixels, [5] zero-area, [6] with an index outside [0, nv).
// mat: read by the traced frames only (TraceDev below): bit 0 water, bit 1 the mesh is wound inwards.
struct MeshRec { long long t0, v0; int nv; unsigned col; int smooth, mat; };
struct MeshDev {
    int nm;                            // meshes
    long long nt;                      // triangles of all meshes
    const MeshRec *rec;                // [nm]
    const float *vert, *nrm;           // [3 x vertices of all meshes] (nrm: read for the meshes with smooth = 1 only)
    const int *tri;                    // [3 nt]
    unsigned *large;                   // [nt] triangles whose screen bounds exceed RENDER_LARGE_PX pixels
};

// Traced mesh frames (sph_render_trace.hpp): the set-up triangles, the sort's keys, the hierarchy and the frame's constants.
// n = ctr[TC_KEPT] triangles are kept (read on the device: no host read between the stages).  Node ids: inner node i of the n - 1 is i,
// the leaf of sorted position j is n - 1 + j, the root is 0 (n = 1: the one leaf).  key = morton30 << 32 | g for a kept triangle g,
// 0x40000000 << 32 | g for a skipped one (sorted behind the kept).
#define TRACE_FLOOR_ID 0xFFFFFFEFu     // the floor's id in a key (below the line ids, above every triangle index)
#define TRACE_REC_WORDS 24             // words of one recorded segment (include/sph_hip.h, sph_render_trace_download_paths)
#define TRACE_SORT_TILE 2048           // keys of one workgroup of the sort
enum TraceCtr { TC_KEPT, TC_NONFINITE, TC_DEGENERATE, TC_BAD_INDEX, TC_DEPTH, TC_RAYS_PRIMARY, TC_RAYS_PATH, TC_RAYS_REFLECT,
                TC_RAYS_SHADOW, TC_VISITS, TC_TESTS, TC_TRUNCATED, TC_ABORTED, TC_COUNT_ = 16 };
struct TraceDev {
    float4 *corner;                    // [3 nt] world corners of triangle g in canonical order (w: the corner's vertex slot, as int bits)
    int *st;                           // [nt] -1 skipped, else mesh << 1 | (canonical order is an odd permutation of the stored one)
    unsigned long long *key[2];        // [nt] each (ping-pong of the radix sort; the sorted keys end in key[0])
    unsigned *hist;                    // [tiles + 1][256] digit counts per tile -> exclusive over the tiles; last row: the digits' bases
    int *left, *right;                 // [nt] children of inner node i
    int *parent, *skip;                // [2 nt] per node id: parent (-1 root); where a ray goes when it is done with the subtree (-1: out)
    int *arrive;                       // [nt] arrival counters of the fit (zeroed every frame)
    float *box;                        // [2 nt][6] lo xyz, hi xyz per node id
    unsigned *bnd;                     // [8] centroid bounds, floats in an order-keeping unsigned code: [0..2] min, [3..5] max
    unsigned long long *ctr;           // [TC_COUNT_]
    float *rec;                        // [W H][max_depth][TRACE_REC_WORDS] or null
    float light[3];                    // the point light, world coordinates
    float floor_y, floor_lo[2], floor_hi[2];   // the floor: y = floor_y, x and z inside [lo, hi]
    float cell;                        // checker cell (world units)
    float ior, absorb;                 // absorb: per world unit of length (the parameter / radius)
    int max_depth, shadows, floor, use_bvh;
};

// Video encoding (sph_video.hpp): one frame -> the scan of a baseline JPEG.  A restart interval is VIDEO_RI MCUs (the
// DRI segment says so) and the work of one workgroup.  Table entries: q the quantiser steps in natural order ([0] luminance, [1]
// chrominance); dc / ac the Huffman code of a symbol | its length << 16.
#define VIDEO_RI 8
struct VideoTables { unsigned short q[2][64]; unsigned dc[2][12]; unsigned ac[2][256]; };
struct VideoDev {
    int W, H, c420;                    // c420: 1 = 4:2:0 (MCU 16 x 16, 6 blocks), 0 = 4:4:4 (MCU 8 x 8, 3 blocks)
    int mw, nmcu, nint;                // MCUs across, in all; restart intervals
    const unsigned char *rgb;          // [H][W][3] the frame (the encoder's upload or a renderer's frame buffer)
    const VideoTables *tab;
    int *len;                          // [nint + 1] bytes per interval, stuffing and marker included -> their exclusive scan, [nint] the total
    unsigned long long *cnt;           // [2] stuffed bytes
    unsigned char *out;                // the scan's bytes
    hipStream_t stream;
};

// PNG encoding (sph_png.hpp): one frame -> the IDAT chunks of a PNG file.  The filtered stream (H rows of 1 + 3 W bytes) is
// cut into segments of PNG_SEG raw bytes, the work of one workgroup and one IDAT chunk each; PNG_DIST are the candidate match distances.
// cnt: [0..4] rows per filter type, [5] stored segments, [6] literals, [7] matches (the tokens of the segments coded with the fixed or a
// dynamic code), [8] dynamic segments, [9] the bits of their headers, [10] window segments, [11] the matches in them that the window
// candidate supplied, [12] those of their matches that reach back more than PNG_FAR bytes, [13] the bits of their headers.
#define PNG_SEG 4096
#define PNG_NCNT 14
#define PNG_SIDE 320                   // bytes per segment of the dynamic coding's side record (sph_png.hpp)
#define PNG_WSIDE 672                  // of the window coding's: the dynamic record, then the window block's lengths, choice and header bits
#define PNG_WINDOW 32768               // coding = window: how far back a match candidate may lie
#define PNG_FAR 4096
#define PNG_NONE 0xFFFFFFFFu           // prev: no candidate
#define PNG_SORT_TILE 4096             // positions per workgroup of the candidate sort
#define PNG_ND 5
#define PNG_DIST_LIST {1, 2, 3, 4, 6}
#define PNG_CRC_PIECE 17               // bytes per thread of a chunk's CRC: 256 pieces cover tag + prefix + stored header + PNG_SEG bytes
static_assert(256 * PNG_CRC_PIECE >= 4 + 2 + 5 + PNG_SEG, "the CRC pieces cover the longest chunk");
#define PNG_CRC_POLY 0xEDB88320u
// a b mod the CRC-32 polynomial, bit-reflected as the CRC register is: bit 31 is x^0
__host__ __device__ static inline unsigned png_crc_mul(unsigned a, unsigned b) {
    unsigned p = 0u;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b >> 1) ^ (PNG_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
struct PngDev {
    int W, H, filter;                  // filter: -1 adaptive, 0..4 that type on every row
    int stride, raw, nseg;             // 1 + 3 W; H stride; segments
    const unsigned char *rgb;          // [H][W][3] the frame (the encoder's upload or a renderer's frame buffer)
    unsigned char *flt;                // [raw] the filtered stream
    int *len;                          // [nseg + 1] bytes per segment's chunk (length, tag, payload, CRC) -> their exclusive scan, [nseg] the total
    unsigned *adler;                   // [2 nseg] per segment: sum of its bytes, sum of (bytes to its end) x byte, both mod 65521
    unsigned long long *cnt;           // [PNG_NCNT] see above
    unsigned *sum;                     // [1] the Adler-32 of the filtered stream (scan pass)
    unsigned crc_pow[8];               // x^(8 PNG_CRC_PIECE 2^j) mod the polynomial: joins two runs of 2^j pieces
    unsigned char *out;                // the chunks, then the Adler-32's own IDAT chunk
    hipStream_t stream;
    unsigned char *side;               // [nseg][PNG_SIDE] coding = dynamic: the count pass's code lengths and choice; nullptr: coding = fixed
    // coding = window (prev == nullptr otherwise; side then holds records of PNG_WSIDE bytes)
    unsigned *prev;                    // [nseg PNG_SEG] per position of the stream its candidate c(i), PNG_NONE: none ([raw, ...) is not written)
    unsigned *sort_key[2], *sort_pos[2];   // [raw] the candidate sort's two sides: 24-bit keys, positions
    int *hist;                         // [256][nsort] digit counts per sort workgroup -> their row-wise exclusive scans, then [256] the rows' totals
    int nsort;                         // workgroups of the sort: ceil((raw - 2) / PNG_SORT_TILE)
};

// Text export (sph_text_passes.hpp): the rows of an ASCII PLY or OBJ file, one piece of them at a time.
struct TextDev {
    int kind;                          // 0: PLY rows "x y z \n"; 1: OBJ rows (v, then vn, then f)
    const unsigned *xyz;               // [nv][3] the bits of the points (PLY) / vertices (OBJ)
    const unsigned *nrm;               // [nv][3] normals, or nullptr: no vn rows, faces as "f a b c"
    const int *tri;                    // [nt][3] 0-based
    long long nv, nt;
    long long row0;                    // the piece: rows [row0, row0 + rows) of the file
    int rows;
    int *len;                          // [rows + 1] bytes per row -> their exclusive scan, [rows] the piece's bytes (< 2^31)
    int *scan_tmp;                     // tile sums of the scans
    int *longest;                      // [1] the longest row so far
    unsigned char *out;                // the piece's bytes (16-byte aligned)
    hipStream_t stream;
};

// Elastic solids (sph_elastic.hpp).  One captured object as its two passes see it: rows = ids id0 .. id0 + n - 1 (a contiguous append
// range), the rest table rest[(2 k + plane) n + row] for k < kmax (k-major; plane 0 = (g0_ij, bits of j), plane 1 = (g0_ji, 0); j = -1
// ends a list), the Lame constants.
struct ElObjDev { int id0, n, kmax; float mu, lambda; float4 *rest; };
// one capture: the object, its id range, a table of all ELASTIC_MAX_NEIGHBOURS entries, the counters (k_elastic_capture)
struct ElCaptureArgs { int obj, id0, n; float4 *rest; unsigned *cnt; };

template <class T> struct DBuf {
    T *b[2] = {nullptr, nullptr};
    int c = 0;
    T *cur() const { return b[c]; }
    T *alt() const { return b[1 - c]; }
    void flip() { c = 1 - c; }
};

// The buffers and the carried bookkeeping of a handle.  Owned by SphHandle; every member initialises itself (sph_create allocates and
// derives from the parameters, nothing else).  What concerns ONE launch is an argument of that launch (Launch below), not a member.
struct State {
    Consts c = {};
    hipStream_t stream = nullptr;
    int cap = 0;         // particle_max_num
    // sorted, carried state
    DBuf<float4> posv, velm, orig;
    DBuf<int> meta, pid;
    DBuf<unsigned> color;   // the sorted copy of the colours: read through Launch::sorted_color (it may be out of date, see color_home)
    DBuf<float> rho;
    // grid
    int *cell_count = nullptr;     // G+1
    int *cell_start = nullptr;     // G+1 (exclusive scan, cell_start[G] = n)
    int *cellid = nullptr, *rank = nullptr;  // per particle (pre-sort)
    // deterministic sort by run lists (RunList above; unsharded scenes): list heads per cell (G + 1, never reset), the epoch of the histogram
    // being taken / last taken, "the hashers of the coming sort filed their runs", and the sort's gather index (dest slot -> source particle)
    unsigned long long *run_head = nullptr;
    int2 *run_rec = nullptr;       // cap + G + 1 records (RunList::rec)
    unsigned sort_epoch = 0u;
    int run_lists_filed = 0;
    int *sort_inv = nullptr;
    long long n_list_sorts = 0;   // sorts that went through k_sort_rank + k_gather_prep, since create (SphStats)
    long long n_carried_sorts = 0;   // ... whose velm / meta / pid the density pass behind them moved (SortCarry), since create (SphStats)
    // Bytes the sort's gather does not have to move (k_gather_prep, unsharded list sorts only):
    //  * a density that the kernel launched next recomputes for every particle: the caller of Launch::scatter_stable says so (rho_dead);
    //  * velocity + mass, meta word and particle id where the kernel launched next is a density pass over every tile of an all-fluid scene
    //    (density_next): that pass reads none of them, is far from any bandwidth limit and moves them itself (SortCarry);
    //  * colours stay AT HOME: color_home[particle id] is written when a particle is appended and never moves, while the ids are the append
    //    order (color_home_ok; ids set from outside or slab sharding end that).  color_stale: the sorted copy (State::color) is out of date --
    //    Launch::sorted_color brings it up to date for whoever needs it (download, a sort by run records, slab activation).
    unsigned *color_home = nullptr;
    int color_home_ok = 0, color_stale = 0;
    int *tmp_idx = nullptr;        // stable-sort scratch: int2 (first source index, length) per run, filed at the run's first slot (2 x cap ints)
    // Sums of the histogram over the scan's tiles of SCAN_TILE cells, two banks of scan_blocks + 1 ints.  Round 6: whoever takes the
    // histogram atomics (k_hash_count, the NextHash epilogue of the force pass, the slab kernels) adds its particles to the tile sums of
    // bank `scan_bank` as well -- one more atomic per WAVE, its lanes' cells lie in one tile nearly always -- so the scan is ONE launch:
    // k_scan_final reads that bank and clears the other one for the next histogram (like cell_count, which it clears behind itself).
    int *scan_partial = nullptr;
    int scan_blocks = 0;
    int *scan_tile_state = nullptr;   // per scan tile: (particles before it) + 1 if its cells hold that constant because it was EMPTY at the last scan, else 0 (k_scan_final)
    int scan_bank = 0;       // bank the hashers of the coming sort add to / the coming scan reads
    int skip_residual = 0;   // fixed-iteration solves (no stop test, nobody reads the residual): the walks leave their partial sums, k_reduce_partials is not launched
    int tile_sums_ready = 0; // ... and they did (else l_scan launches k_scan_reduce first: slab ranks)
    int cell_count_clean = 1;          // cell_count is all zero (the scan clears it behind itself)
    int hist_taken = 0;                // the histogram of the coming sort has been taken (by k_hash_count, a NextHash epilogue, the slab kernels) and not yet scanned
    int state_error = 0;               // sticky: a launcher met a state it must never see (l_scan without a histogram: ADVICE r05); reported by check_async
    // per-step scratch
    float *rho_raw = nullptr, *prs = nullptr, *ptm = nullptr;
    float4 *acc = nullptr;
    // DFSPH
    float *alpha = nullptr, *kappa = nullptr, *kappa_v = nullptr, *rho_star = nullptr, *rho_deriv = nullptr;
    float *kappa_next = nullptr, *kappa_v_next = nullptr;  // written by the rho_adv pass, consumed (after a swap) by the next correction
    float2 *kr = nullptr;          // (kappa, rho) staging pair for the correction pass
    // PCISPH
    float4 *pacc = nullptr, *pvel = nullptr, *ppos = nullptr, *acc_np = nullptr;
    // IISPH (allocated for that method only): (dii, aii), (dij_pj, sum_i), w = dii p + dij_pj; rho* in rho_star
    float4 *iisph_dii = nullptr, *iisph_dij = nullptr, *iisph_w = nullptr;
    // PBF (allocated for that method only, particle_max_num each): x_old = (position at the sort, sorted cell id), lambda, the second position
    // buffer of the Jacobi fix_position (swapped with posv.cur() behind every pass), recentred walks per statistics bank
    float4 *pbf_old = nullptr, *pbf_pos = nullptr; float *pbf_lambda = nullptr; unsigned long long *pbf_recentred = nullptr;
    int poly6 = 0;       // the shared passes (NonPressurePass, RigidVolumePass) use PBF.py's poly6 / spiky kernels
    // consistent PBF variant (sph_pbf_consistent.hpp): pbf_old / pbf_pos hold x* and the correction pass's second x* buffer, posv the old positions
    float pbf_eps = 1e-6f;   // SphPbfParams::epsilon, the relaxation term of lambda's denominator
    // rigid contact (sph_set_rigid_contact; allocated when first enabled): the per-key table (64-bit fixed point, sph_contact.hpp),
    // the per-particle (sum of depth * n, contacts) of the targets, the accepted contacts of the last pass
    int contact_on = 0;
    ContactArgs contact = {};
    unsigned long long *contact_table = nullptr, *contact_pairs = nullptr;
    float4 *contact_part = nullptr;
    // device rigid integrator (sph_set_rigid_integrator; the body array is allocated with the first sph_set_rigid_body)
    int rigid_int_on = 0;
    RigidIntArgs rigid_int = {};
    RigidBodyDev *rigid_bodies = nullptr;   // [SPH_NOBJ]
    // device contact solver (sph_set_rigid_contact_solver; allocated when first enabled): the rows of the last solve, one per table key at
    // most (sph_contact_solve.hpp), and their number
    int contact_solve_on = 0;
    ContactSolveArgs contact_solve = {};
    double *contact_rows = nullptr;
    int *contact_nrows = nullptr;
    // scripted rigid bodies (sph_set_rigid_motion; the record array is allocated with the first one)
    RigidMotionArgs rigid_motion_args = {};
    RigidMotionDev *rigid_motion = nullptr;   // [SPH_NOBJ]
    // fluid emitters (sph_set_emitter; the record array is allocated with the first one)
    EmitterDev *emitters = nullptr;           // [SPH_MAX_EMITTERS]
    // outflow (sph_set_outflow / sph_remove_particles; allocated with the first use): the counters of the mark kernels, the sorted id list
    // of a removal by id; drop_n: the COMING sort files that many dead particles into the graveyard cells behind the grid (the route of
    // a slab rank: hash with the meta words, scan over G + SPH_NGRAVE, run records; no run lists, no tile sums from the hasher)
    unsigned *outflow_ctr = nullptr;          // [(SPH_MAX_OUTFLOWS + 1) * SPH_OUTFLOW_CTR_STRIDE]
    int *outflow_ids = nullptr; int outflow_ids_cap = 0;
    int drop_n = 0;
    // adaptive time stepping (sph_set_cfl; allocated when the mode is first switched on): the result words of k_cfl_speed
    unsigned *cfl_words = nullptr;            // [2 * SPH_CFL_BANK_STRIDE]
    // CG (implicit viscosity)
    float4 *cg_p = nullptr, *cg_Ap = nullptr, *cg_x = nullptr, *cg_b = nullptr, *cg_r = nullptr, *cg_v0 = nullptr;
    float4 *cg_p2 = nullptr;   // second search-direction buffer (fused p update: the A p pass reads the old one and writes the new one)
    int cg_fused_loop = 0;     // this solve runs the two-launch iteration (A p [+ combine], x / r update)
    float *cg_dinv = nullptr;  // 9 floats per particle
    float4 *cg_part = nullptr; // 3 x cap: per-group parts of A p when the pass is split (CgApPass::SPLIT3)
    int cg_nocombine = 0;      // the last A p pass was split and left its dot-product shares itself: the x / r update adds the parts up (no k_cg_ap_combine)
    int cg_split = 0;          // this solve splits its A p passes (few fluid particles: see implicit_viscosity_non_pressure)
    int cg_parity = 0;         // which of the two |r|^2 partial arrays the next x / r update reads
    int cg_first = 1;          // the next A p pass of the loop is its first: no p update to fold into it (sph_cg_steps.hpp)
    // reductions
    float *red_partial = nullptr;  // per-block partial sums
    int red_blocks = 0;
    DevScalars *scal = nullptr;    // device
    RigidPose *pose = nullptr;     // device copy
    int has_dynamic_rigid = 0;
    int has_rigid = 0;
    // z-slab sharding (sph_halo.hpp): exchange tables and message buffers
    int *xidx[2] = {};   // carried through the sort: (kind << 29) | index, see HALO_KIND_*
    int xcur = 0;
    int *halo_tab[8] = {};   // slot tables, index = kind - 1 (sph_halo.hpp HALO_*): send, ghost, echo-send, echo-ghost x {down, up}
    float4 *sendbuf[2] = {}, *recvbuf[2] = {};     // 3 float4 per particle record
    int *halo_counts = nullptr;    // device, two banks of 4 (push transport: bank = message parity): [0..1] send counts, [2] dropped
    SlabDyn *dyn = nullptr;        // device-resident counts of a step, two banks (message parity): a kernel reads the last step's, writes this step's
    SlabDyn *dyn_cur = nullptr;    // the bank of the last step message (what c.n_dev and the field kernels look at)
    int tables_pending = 0;  // push transport: the next k_block_prep also fills the halo slot tables from xidx
    int async_counts = 0;    // the running step takes its counts from `dyn` (c.n_dev set, c.n = launch bound)
    // push transport (sph_halo.hpp): my inbox, the neighbours' inboxes mapped through hipIpc, message numbers
    struct PushState {
        int on = 0;                        // halo payload travels by device stores into the neighbour's inbox
        char *inbox = nullptr;             // mine (device memory the neighbours write)
        char *peer[2] = {};                // lower / upper neighbour's inbox in my address space (null: no neighbour)
        int rec_cap = 0;                   // records a step message can hold (normally the particle capacity)
        size_t rec_bytes = 0, fld_bytes = 0;   // size of one step-message / field-message region
        unsigned rec_seq = 0, fld_seq = 0;     // messages sent (= received) so far
        long long timeout_ticks = 0;       // bounded waits of the device (100 MHz wall clock)
        SlabDyn *mirror = nullptr;         // pinned host copy of `dyn`, written by the wait kernel
    } push;
    // slab sharding, compute / halo overlap: the layers of a slab are contiguous index ranges of the sorted arrays (x is the slowest axis of
    // the cell order), so the 256-particle tiles fall into a BOUNDARY set (anything within two own layers of a face, plus the ghost layers)
    // and an INTERIOR set; k_block_prep lists both once per sort.  A density pass launched with DensityOpts::tiles = 1 / 2 walks one set
    // only: boundary tiles first, their values go out, interior tiles run while the message is in flight.
    int *tile_list[2] = {};   // [0] boundary tiles, [1] interior tiles (XCD-remapped order), device
    int *tile_cnt = nullptr;  // their lengths (2 ints, device)
    unsigned char *tile_class = nullptr;   // per tile: 1 = boundary set.  The INTERIOR launch is an ordinary launch of every tile (no list: a list costs each
                                           // workgroup one more dependent load in front of its header) whose boundary tiles leave at once.
    int tile_plan_n = -1;     // particle count (launch bound) the lists were built for, -1: none
    int tile_bound_b = 0;     // workgroups a boundary launch gets: last known number of boundary tiles + margin (checked on the device: SLAB_ST_BOUND)
    HaloSend presend = {};    // on != 0: the next wcsph_forces launch classifies its particles and sends the next step message itself
    HaloFieldSend fieldsend = {};   // on != 0: the next WCSPH density launch stores its boundary values into the field message itself
    int preclassified = 0;    // ... and has done so: the next step's exchange starts with the hash alone
    int prehashed = 0;        // a force pass / position update has hashed for the coming sort (ForceOpts::hash_next, advect_boundary): that sort starts with the scan (l_hash_count returns at once)
    long long n_hash_launches = 0, n_prehashed_sorts = 0;   // k_hash_count launches / sorts that started from a NextHash hash, since create (SphStats)
    int halo_cap = 0;         // particles per message buffer
    int halo_longest = 0;     // longest halo message of the running step, in particles (sent or received)
    int slab_active = 0, z_lo = 0, z_hi = 0, has_down = 0, has_up = 0;
    unsigned *nbr_mask = nullptr;     // [9][cap]: acceptance mask of the first 32 candidates of every (particle, run), see process_run
    unsigned *nbr_mask_hi = nullptr;  // [9][cap]: candidates 32..63 of the runs that have them
    int masks_valid = 0;
    int uniform_mass = 0;     // all-fluid scene whose particles all carry the same mass (sph_api.hip refresh_counts): WcsphForcePass<true, true>
    // device-controlled solver loops (sph_steps.hpp device_loop): every kernel of an iteration starts with a look at
    // scal->flags[0] (stop) when loop_flag is set; the iteration's reduction kernel evaluates the stop criterion itself
    const int *loop_flag = nullptr;   // null outside such a loop
    int loop_slot = 0;            // reduction slot the criterion applies to
    int loop_kind = 0;            // 1: (double)(sum / denom) <= thr   2: (sum / denom) < (float)thr   3: CG, !(err > thr)
    float loop_denom = 1.0f; double loop_thr = 0.0;
    unsigned char *lane_perm = nullptr;  // [ceil(cap / 256) * 256]: lane -> particle map of every 256-particle workgroup (k_lane_perm)
    int *blk_flag = nullptr, *blk_list = nullptr, *blk_count = nullptr;   // per-workgroup 'holds fluid' flag, ascending list of those workgroups, its length (device)
    int list_n = -1;              // particle count the list was built for (-1: none)
    // Length of the list as the HOST knows it: k_compact_blocks stores it into pinned memory, an event behind it tells when it has landed.
    // A launch over the list then gets exactly that many workgroups (list_grid, sph_kernels.hip) instead of one per tile of the scene
    // with all but the listed ones leaving at once: the buckling scene has 8,496 tiles of which ~420 hold fluid, and the 24,000 empty
    // workgroups of a three-way split A p launch cost 16 % of the walk (round 5: C5 1.63 -> 1.47 ms/step).
    volatile int *list_count_pinned = nullptr;
    hipEvent_t list_count_event = nullptr;
    int list_count_known = -1;    // -1: not seen yet (the launches use the full grid until the event has passed)
    int last_pass_listed = 0;     // the last pass with a reduction ran the listed workgroups only: so must the sum of its partials
    int *blk_hdr = nullptr;       // [ceil(cap / 256)][BLK_HDR_INTS]: cell span and candidate-run windows of every workgroup
    int perm_n = -1;              // particle count blk_hdr / lane_perm were built for (-1: none)
    int has_emitter = 0;     // gravitationUpper set (base_solver.py:18-23)
    int visc_rho_raw = 0;    // viscosity reads rho_raw (WCSPH: density before the EOS clamp)
    int skip_viscosity = 0;  // implicit viscosity: explicit term not part of the fused pass
    float4 *np_acc_out = nullptr;  // non-pressure acceleration sink (PCISPH), else null
    // Akinci surface tension (sph_set_surface_tension; sph_surface_tension.hpp): off unless st_akinci; the buffers are allocated when the
    // mode is first switched on (normals: recomputed every step, not carried through the sort; st_acc: the non-pressure acceleration
    // of the last Akinci pass where the method keeps none of its own)
    int st_akinci = 0;
    double st_gamma = 1.0, st_beta = 0.0, st_h = 0.0;
    float4 *st_normal = nullptr, *st_acc = nullptr;
    // Micropolar vorticity model (sph_set_micropolar; sph_micropolar.hpp): off unless mp_on; the buffers are allocated when the mode is
    // first switched on.  mp_w_home[particle id]: the angular velocities AT HOME (no sort moves them; ids = append order, which
    // ids_custom ends: the mode and ids from outside exclude each other); mp_w_sorted: their copy in sorted order for the walk's
    // candidate records; mp_acc: a_mp of the last walk in sorted order (valid until the next sort).  With the mode on and no
    // non-pressure acceleration kept otherwise, st_acc takes it.
    int mp_on = 0, ids_custom = 0;
    double mp_nu_t = 0.01, mp_zeta = 0.1, mp_theta_inv = 0.5;
    float4 *mp_w_home = nullptr, *mp_w_sorted = nullptr, *mp_acc = nullptr;
    // Elastic solids (sph_set_elastic_object; sph_elastic.hpp): nothing is allocated or launched until an object is marked.  el_marked:
    // objects marked elastic, captured or waiting (WCSPH takes its unfused route while > 0); el_pending: those waiting for the next
    // sort that holds their particles; el_obj[0 .. el_nobj): the captured ones, el_mask: bit o = object o is among them.  At home by
    // particle id (ids = append order, as mp_w_home): positions and slots (the scatter's), q (double-buffered: pass A reads
    // el_q[el_qi] and writes the other, then el_qi flips), sigma (2 float4 per id), F (3 float4 per id).  el_acc: a_el of the last
    // pass B in sorted order (valid until the next sort).  el_cnt: the capture's counters (k_elastic_capture).
    int el_marked = 0, el_pending = 0, el_nobj = 0, el_qi = 0;
    unsigned el_mask = 0;
    ElObjDev el_obj[SPH_NOBJ] = {};
    float4 *el_x_home = nullptr, *el_q[2] = {nullptr, nullptr}, *el_sig = nullptr, *el_F = nullptr, *el_acc = nullptr;
    int *el_slot_home = nullptr;
    unsigned *el_cnt = nullptr;
    // Air drag (sph_set_drag; sph_drag.hpp): off unless dr_on; the two buffers are allocated when the mode is first switched on.
    // dr_acc = (a_drag, n_i), dr_terms = (w, C_D, A_un, y) of the last walk, in sorted order (valid until the next sort).  dr_u: the
    // wind in the scene's frame (what sph_get_drag returns), dr_u_lib: in the library's; dr_radius, dr_rho_l: the handle's particle
    // radius and rest density, from which the launcher derives the model's constants.  With the mode on and no non-pressure
    // acceleration kept otherwise, st_acc takes it.
    int dr_on = 0;
    double dr_k = 1.0, dr_rho_a = 1.2041, dr_u[3] = {0.0, 0.0, 0.0}, dr_u_lib[3] = {0.0, 0.0, 0.0}, dr_radius = 0.0, dr_rho_l = 0.0;
    float4 *dr_acc = nullptr, *dr_terms = nullptr;
    // Heat (sph_set_thermal; sph_thermal.hpp): off unless heat_on; the buffers are allocated when the mode is first switched on.
    // heat_T_home[particle id]: the temperatures AT HOME (no sort moves them; ids = append order, as mp_w_home: the mode and ids from
    // outside exclude each other); heat_T_sorted: their copy in sorted order, for the walk's candidate records and the buoyancy;
    // heat_rate: dT/dt of the last walk in sorted order (valid until the next sort); heat_obj_T: the per-object table on the device,
    // indexed by the low byte of the meta word (object id + 1; 0: the domain box), HT_ADIABATIC where the object has no temperature.
    int heat_on = 0;
    double heat_alpha = 1.0e-4, heat_beta = 0.0, heat_t_ref = 0.0;
    float *heat_T_home = nullptr, *heat_T_sorted = nullptr, *heat_rate = nullptr, *heat_obj_T = nullptr;
};

// Where the non-pressure acceleration is kept, or null where nobody keeps one: PCISPH's own buffer, else the buffer the Akinci pass
// writes and the micropolar model and the air drag make every method keep.  ONE statement of the rule for the non-pressure launcher
// and for every launch that adds an acceleration behind it.
static inline float4 *kept_np_acc(const State &s) {
    return s.np_acc_out ? s.np_acc_out : ((s.st_akinci || s.mp_on || s.dr_on) ? s.st_acc : nullptr);
}

// What a list sort's gather left behind for the density pass launched next (Launch::scatter_stable, density_next): thread d of a tile does
// out[d] = in[inv[d]] for velocity + mass, meta word and particle id -- exactly what k_gather_prep does otherwise -- in the prologue of
// k_nbr_pass<DensityPass<true, ...>>, on the memory round trips that prologue makes anyway.  Returned by the sort, handed to that ONE
// density launch (DensityOpts::carry); on = 0: the gather moved everything.
struct SortCarry {
    const int *inv = nullptr;      // destination slot -> source particle (State::sort_inv)
    const float4 *velm_in = nullptr; float4 *velm_out = nullptr;
    const int *meta_in = nullptr; int *meta_out = nullptr;
    const int *pid_in = nullptr; int *pid_out = nullptr;
    int on = 0;
};
// the functor's member, as an empty base where the instantiation has nothing to carry (its kernel arguments stay what they were)
template <bool ON> struct SortCarryOf { SortCarry carry; };
template <> struct SortCarryOf<false> {};

// Options of one launch (Launch::density, Launch::wcsph_forces)
struct DensityOpts {
    int tiles = 0;             // slab sharding, compute / halo overlap: 0 every tile, 1 the boundary set, 2 the interior set (State::tile_list)
    bool books_forces = false; // WCSPH step with the fused force pass: the density pass counts that pass's pairs too (it walks the same masks)
    SortCarry carry = {};      // the sort in front of this launch left velm / meta / pid for it to move (it said so: Launch::scatter_stable)
};
struct ForceOpts {
    bool booked_by_density = false;   // the density pass in front of this one has counted its pairs (DensityOpts::books_forces); else it counts its own
    bool hash_next = false;           // hash the positions it stores for the next step's sort (NextHash): the caller knows that nothing touches the particles before it
};

// Function table implemented twice (strict / fast math), see sph_kernels.hip.
struct Launch {
    unsigned *(*sorted_color)(State &);   // the colours in sorted order (State::color.cur()), materialised from color_home first if color_stale
    void (*hash_count)(State &);
    void (*scan)(State &);
    void (*scatter)(State &);                   // carries every array
    // rho_dead: the kernel launched next rewrites the density of every particle, so the gather need not carry it (list sorts of all-fluid
    // scenes drop it; the new rho.cur() then holds garbage until that kernel has run -- 0xFF bytes in the test-hook library)
    // density_next: the kernel launched next is a DensityPass over every tile (Launch::density with tiles = 0), so an all-fluid list sort
    // leaves velm / meta / pid to it.  The SortCarry returned says whether it did (on) and MUST then go into that launch's DensityOpts:
    // until that pass has run, velm.cur() / meta.cur() / pid.cur() hold garbage (0xFF bytes in the test-hook library).
    SortCarry (*scatter_stable)(State &, bool rho_dead, bool density_next);
    void (*density)(State &, int eos, DensityOpts o);
    void (*surface_normals)(State &);   // Akinci surface tension: the colour-field normals (State::st_normal), before non_pressure
    void (*micropolar)(State &);         // micropolar model: gather w, the walk (State::mp_acc, mp_w_home), before non_pressure
    void (*micropolar_apply)(State &);   // ... and v += dt a_mp (+ the kept non-pressure acceleration) behind it
    void (*elastic)(State &);            // elastic solids: scatter, pass A, pass B over the captured objects (State::el_acc), before non_pressure
    void (*elastic_apply)(State &);      // ... and v += dt a_el (+ the kept non-pressure acceleration) behind it
    void (*drag)(State &);               // air drag: the walk (State::dr_acc, dr_terms), before non_pressure
    void (*drag_apply)(State &);         // ... and v += dt a_drag (+ the kept non-pressure acceleration) behind it, behind the elastic solids'
    void (*heat)(State &);               // heat: gather T, the walk (State::heat_T_home, heat_rate), before non_pressure
    void (*heat_apply)(State &);         // ... and v += dt a_b (+ the kept non-pressure acceleration) behind it, behind the air drag's
    void (*heat_fill)(State &, int first_id, int count, float T);   // rows of new particles: heat_T_home[first_id, first_id + count) = T
    void (*elastic_capture)(State &, const ElCaptureArgs &);   // one object's rest configuration, on the cell lists of the sort that has just run
    void (*non_pressure)(State &, const float4 *visc_vel);   // visc_vel: velocities for the viscous term (implicit viscosity: cg_x), null: the particles' own
    void (*pressure_integrate)(State &);
    void (*wcsph_forces)(State &, ForceOpts o); // non_pressure + pressure_integrate in one neighbour walk (WCSPH)
    void (*rigid_volume)(State &);
    void (*renew_rigid)(State &);
    void (*prepare_emitter)(State &);
    void (*post_insert)(State &, int first, int stale_volume);   // appended particles [first, n): boundary (+ V = 1 / W(0) for rigid ones)
    void (*clear_fresh)(State &);
    // DFSPH
    void (*dfsph_density_alpha)(State &);
    void (*dfsph_density_alpha_div)(State &);   // + the first density derivative of the divergence solve (one neighbour walk less per step)
    void (*dfsph_rho_adv)(State &, int mode);   // 0: density derivative (+kappa_v), 1: density star (+kappa)
    void (*dfsph_correct)(State &, int mode);   // 0: divergence step, 1: density step
    void (*advect_boundary)(State &, bool hash_next);   // x += dt v, emitter, boundary (DFSPH position update); hash_next: + the hash of the sort that follows (NextHash)
    // PCISPH
    void (*pcisph_init)(State &);
    void (*pcisph_rho_star)(State &);
    void (*pcisph_pressure_accel)(State &);
    void (*pcisph_reduce_error)(State &);       // adds up the rho* walk's partial sums where no second walk follows (SPH_PH_PCISPH_RHO_STAR)
    // IISPH
    void (*iisph_prepare)(State &);             // dii + aii + rho* (IISPH.py:18-90), p = 0
    void (*iisph_dij_pj)(State &);              // first walk of an iteration (IISPH.py:125, + w = dii p + dij_pj)
    void (*iisph_sum_i)(State &);               // second walk: sum_i + update_pressure + the error's reduction (IISPH.py:148, :98)
    // PBF
    void (*pbf_predict)(State &);               // save_old_position + update_fluid_position + boundary (PBF.py:151-154)
    void (*pbf_density_lambda)(State &);        // compute_density + compute_lambda, one walk (PBF.py:64-65)
    void (*pbf_fix_position)(State &);          // fix_position, Jacobi (PBF.py:66, :104)
    void (*pbf_finish)(State &);                // boundary + recompute_fluid_velocity (PBF.py:156-158)
    // consistent PBF variant
    void (*pbfc_predict)(State &);              // x* = x + dt v* + boundary
    void (*pbfc_density_lambda)(State &, int reduce);   // walk A: rho, lambda, partial sums of C (reduce: summed at once, for a lone phase)
    void (*pbfc_delta)(State &, int reduce);    // walk B: the Jacobi correction of x* (+ the reduction that closes the iteration)
    void (*pbfc_finish)(State &);               // x = boundary(x*), v = (x - x_old) / dt, emitter branch
    // rigid contact: one walk over the dynamic rigid particles, per-key table + per-particle sums (sph_contact.hpp)
    void (*rigid_contact)(State &);
    // device rigid integrator: one workgroup per registered body (sph_rigid.hpp)
    void (*rigid_integrate)(State &);
    // device contact solver: one workgroup for the whole body system, in place of rigid_integrate (sph_contact_solve.hpp)
    void (*rigid_contact_solve)(State &);
    // scripted rigid bodies: one wave per body, before rigid_integrate / rigid_contact_solve (sph_rigid_motion.hpp)
    void (*rigid_motion)(State &);
    // fluid emitters (sph_emitter.hpp): the held layers onto their closed form (an elementwise pass over the n live particles), and the
    // newborn layers into the slots behind them (the caller raises the counts afterwards)
    void (*emit_hold)(State &, const EmitHoldArgs &);
    void (*emit)(State &, const EmitArgs &);
    // outflow (sph_outflow.hpp): the dead bit for every active fluid particle inside an active volume / whose id is in the sorted list
    void (*outflow_mark)(State &, const OutflowArgs &);
    void (*outflow_mark_ids)(State &, int nids);
    // adaptive time stepping (sph_cfl.hpp): the maximum of |v|^2 over the particles that count, into the result pair `bank`
    void (*cfl_speed)(State &, int bank);
    // z-slab sharding
    void (*halo_classify_pack)(State &, int n);
    void (*halo_unpack_append)(State &, int side, int count, int offset);
    void (*halo_build_tables)(State &);
    void (*halo_pack_fields)(State &, int side, int n_send, int n_recv);
    void (*halo_unpack_fields)(State &, int side, int n_recv, int n_send);
    void (*halo_pack_scalar)(State &, int side, int n_send, int n_recv, const float *src);
    void (*halo_unpack_scalar)(State &, int side, int n_recv, int n_send, float *dst);
    void (*halo_pack_vel)(State &, int side, int n_send, int n_recv, const float4 *arr);   // xyz of a float4 array
    void (*halo_unpack_vel)(State &, int side, int n_recv, int n_send, float4 *arr);
    void (*count_ghosts)(State &, int *out);
    // surface reconstruction (sph_surface.hpp)
    void (*surf_compact)(SurfDev &, const float4 *posv, const int *meta, int n, int object_id);   // one object's particles -> xin, counter
    void (*surf_bounds)(SurfDev &);             // coarse bounds of xin[0, n)
    void (*surf_bin)(SurfDev &);                // bin by coarse cell, order each cell by key, V_j (-> xs)
    void (*surf_flags)(SurfDev &);              // active bricks: flags and their scan (flag[G] = nb)
    void (*surf_field)(SurfDev &);              // brick list + phi at every point of every active brick (the hot pass)
    void (*surf_count)(SurfDev &);              // classify cubes and edges, per-brick vertex / triangle counts and their scans
    void (*surf_emit)(SurfDev &);               // vertices and triangles
    void (*surf_normals)(SurfDev &, int nv);    // -grad phi / |grad phi| at every vertex
    // anisotropic kernels (sph_surface_aniso.hpp)
    void (*surf_aniso_moments)(SurfDev &, SurfAniso &);           // N_i, weighted covariance, eigen-decomposition and clamp -> A_i, det A_i
    void (*surf_aniso_volume)(SurfDev &, SurfAniso &);            // V_j from the anisotropic kernels of the 27 cells
    void (*surf_field_aniso)(SurfDev &, SurfAniso &);             // surf_field with w_j(x) = det A_j W(|A_j (x - x_j)|)
    void (*surf_normals_aniso)(SurfDev &, SurfAniso &, int nv);   // surf_normals with the analytic gradient of w_j
    // surface post-processing (sph_surface_post.hpp)
    void (*surf_post_adjacency)(SurfDev &, SurfPost &);           // slots, sort + dedup, scan of the unique counts (cnt[nv] = entries)
    void (*surf_post_compact)(SurfDev &, SurfPost &);             // CSR neighbours into adj
    void (*surf_post_weights)(SurfDev &, SurfPost &);             // c_j per particle, w_i per vertex
    void (*surf_post_smooth)(SurfDev &, SurfPost &, int iters);   // Laplacian smoothing of d.vert
    void (*surf_post_nsmooth)(SurfDev &, SurfPost &, int iters);  // normal smoothing of d.nrm
    // particle rendering (sph_render.hpp)
    void (*render_splat)(RenderDev &);          // depth keys of spheres (small per thread, large per workgroup) and box lines
    void (*render_shade)(RenderDev &);          // the winners' colours, then background / ids / covered count per pixel
    void (*render_merge)(RenderDev &, const unsigned long long *, const unsigned char *);   // another layer's keys and colours folded in
    void (*render_finish)(RenderDev &);         // background / ids / covered count per pixel once more (after merges)
    // screen-space surface mode (sph_render_surface.hpp)
    void (*render_surface_base)(RenderDev &, RenderSurfDev &);      // the base plane: the shade walk once more, colour | surface flag
    void (*render_surface_quantise)(RenderDev &, RenderSurfDev &);  // key plane -> integer depth in both q planes, surface pixels counted
    void (*render_surface_smooth)(RenderDev &, RenderSurfDev &, int it);   // iteration it: q[it & 1] -> q[1 - (it & 1)]
    void (*render_surface_shade)(RenderDev &, RenderSurfDev &, int plane); // normals off q[plane], colour into rgb where the flag is set
    // thickness mode of the surface frames (sph_render_thickness.hpp)
    void (*render_thick_opaque)(RenderDev &, RenderSurfDev &, RenderThickDev &);   // the opaque layer: splat, shade, lines, finish on a copy
    void (*render_thick_splat)(RenderDev &, RenderSurfDev &, RenderThickDev &);    // T[0] = sum of the surface spheres' chords per pixel
    void (*render_thick_smooth)(RenderDev &, RenderSurfDev &, RenderThickDev &, const unsigned *Q, const unsigned *in, unsigned *out);
    void (*render_thick_shade)(RenderDev &, RenderSurfDev &, RenderThickDev &, const unsigned *Q, const unsigned *T);   // the composite
    // diffuse particles in the surface frames (sph_render_foam.hpp)
    void (*render_foam_splat)(RenderDev &, RenderSurfDev &, RenderFoamDev &);   // fo / fu / du from the diffuse spheres' chords
    void (*render_foam_under)(RenderDev &, RenderSurfDev &, RenderThickDev &, RenderFoamDev &, const unsigned *Q, const unsigned *T);
    void (*render_foam_over)(RenderDev &, RenderFoamDev &);                     // the over layer on the bytes held; both layers' pixels counted
    // mesh rendering (sph_render_mesh.hpp)
    void (*render_mesh_depth)(RenderDev &, MeshDev &);   // depth keys of triangles (small per thread, large per workgroup) and box lines
    void (*render_mesh_shade)(RenderDev &, MeshDev &);   // the winners' colours (triangles, lines)
    void (*render_mesh_finish)(RenderDev &);             // background / ids / covered count per pixel
    // traced mesh frames (sph_render_trace.hpp)
    void (*render_trace_setup)(MeshDev &, TraceDev &, hipStream_t);   // corners, skipped triangles counted, centroid bounds; then the keys
    void (*render_trace_sort)(MeshDev &, TraceDev &, hipStream_t);    // four 8-bit passes over the code bits
    void (*render_trace_hierarchy)(MeshDev &, TraceDev &, hipStream_t);   // Karras 2012: children and parents
    void (*render_trace_fit)(MeshDev &, TraceDev &, hipStream_t);     // boxes bottom-up, then the skip links and the depth
    void (*render_trace_shade)(RenderDev &, MeshDev &, TraceDev &);   // one path per pixel: rgb and the primary key
    void (*render_trace_finish)(RenderDev &);                         // box lines over the frame, the id image
    // video encoding (sph_video.hpp)
    void (*video_count)(VideoDev &);            // bytes per restart interval (transform, symbols, stuffing; nothing stored but the counts)
    void (*video_scan)(VideoDev &);             // their exclusive scan, the total behind it
    void (*video_write)(VideoDev &);            // the same bytes again, stored at the scanned offsets
    // PNG encoding (sph_png.hpp)
    void (*png_filter)(PngDev &);               // the filtered stream: one row filter per row, by the least sum of |residual|
    void (*png_candidates)(PngDev &);           // coding = window: prev[] of the whole filtered stream (sort by three-byte key, predecessors)
    void (*png_count)(PngDev &);                // bytes per segment's chunk (tokens, fixed or stored), the Adler sums
    void (*png_scan)(PngDev &);                 // their exclusive scan, the total behind it; the Adler-32
    void (*png_write)(PngDev &);                // the same bytes again, stored at the scanned offsets, with every chunk's CRC
    // text export (sph_text_passes.hpp)
    void (*text_count)(TextDev &);              // bytes per row of the piece, the longest row
    void (*text_scan)(TextDev &);               // their exclusive scan, the piece's bytes behind it
    void (*text_write)(TextDev &);              // the rows' characters at the scanned offsets (staged in LDS, aligned 16-byte stores)
    void (*text_check_tri)(TextDev &, int *bad);   // bad[0] = any triangle index outside [0, nv)
    void (*text_compact)(TextDev &, const float4 *posv, const int *meta, int n, int obj, int *slot, float *xyz);   // one object's particles, order kept
    // diffuse particles (sph_foam.hpp)
    void (*foam_compact)(FoamDev &, const float4 *posv, const float4 *velm, const int *pid, const int *meta, int n_all, int *flag);   // active fluid -> xin / vin / idin in the handle's order, flag[n_all] = n
    void (*foam_grid)(FoamDev &);               // hash + count, scan, scatter, id order inside each cell
    void (*foam_advect)(FoamDev &);             // the diffuse particles' walk, classes, survivors compacted into the other bank
    void (*foam_normals)(FoamDev &);
    void (*foam_potentials)(FoamDev &);         // ta, wc, e, n_d and the child counts
    void (*foam_generate)(FoamDev &);           // scan of the counts, children behind the survivors, the step's counters
    void (*foam_render_source)(const FoamDev &, int n, int *id, unsigned *col, const unsigned rgb[3]);   // renderer ids and class colours of the diffuse set
    void (*layer_hist)(State &, int *hist);      // owned particles per global cell layer
    void (*loop_criterion)(State &, int slot);   // stop test on an all-reduced residual (sharded solver loops)
    // push transport: the step message is written by halo_classify_pack itself; then
    // announce my message, wait for both neighbours', settle SlabDyn, append their records, reset the slot tables
    void (*halo_unpack2)(State &, int n_old, int bound_app, int bound_live, int count_hint);
    void (*halo_push_fields)(State &, int kind, float *f0, float4 *v, int count_hint);   // pack a field message per neighbour
    void (*halo_pull_fields)(State &, int kind, float *f0, float4 *v, int count_hint);   // announce, wait, scatter the neighbours' field messages
    void (*halo_selftest)(State &, int n, int tag, int tag_down, int tag_up, int *bad_dev);
    void (*halo_fieldsend_begin)(State &);   // begin a field message of kind 2: the density pass launched next fills it (State::fieldsend)
    void (*halo_presend_begin)(State &);   // begin the next step message: the force pass launched next fills it (State::presend)
    // implicit viscosity (CG)
    void (*cg_prepare)(State &);
    void (*cg_ap)(State &, bool fuse);   // fuse: apply the previous iteration's p update on the fly (CgApPass::fuse)
    void (*cg_prepare2)(State &);
    void (*cg_alpha)(State &);
    void (*cg_check)(State &);   // fused p update: stop test at the end of a batch of iterations
    void (*cg_update_xr)(State &);
    void (*cg_update_p)(State &);
    void (*cg_prepare_guess)(State &);
    void (*cg_fold)(State &, int which);   // slab sharding: local sums of the dot-product partials -> scal->red[6..7]
};

const Launch *sph_launch_strict();
const Launch *sph_launch_fast();
