// sph_rigid_motion.hpp -- scripted rigid bodies: the launch that evaluates their motion programs; included by sph_kernels.hip inside the
// per-build namespace.  Semantics in include/sph_hip.h (sph_set_rigid_motion), design in DESIGN.md 31.
//
// One wave per scripted body, in the slot of the device rigid integrator and before its launch (which clears the wrench words of the
// objects it does not own).  The program is a short serial piece of float64 arithmetic -- two evaluations of the pose (at t_k and
// t_{k+1}, products of the step count, never a running sum) and their backward differences -- so the wave's first lane runs it and the
// others leave: it costs what one lane costs, and a scene with a paddle still advances as one device call without a pose upload per
// step.  The lane then consumes the body's six wrench words (read as sph_get_rigid_wrench hands them out, rounded through float32),
// adds dt * force and dt * torque to the impulse sums, and writes the float64 record and the float32 pose k_renew_rigid reads.  The
// arithmetic is sph_rigid_motion_eval.hpp's, the same source the host entry compiles; keys are read from the record in global memory.
#pragma once
#include "sph_rigid_motion_eval.hpp"

__global__ void __launch_bounds__(64)
k_rigid_motion(const RigidMotionArgs a, RigidMotionDev *bodies, DevScalars *scal, RigidPose *pose) {
#pragma clang fp contract(off)
    const int o = a.ids[blockIdx.x];
    if (o < 0 || o >= SPH_NOBJ || threadIdx.x != 0) return;
    RigidMotionDev *b = bodies + o;
    double com[3], rot[9], vel[3], w[3];
    rm_step(&b->prog, b->com_rest, b->rot_rest, a.dt, a.k, com, rot, vel, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double f = (double)(float)((double)scal->wrench[3 * o + k] / SPH_WRENCH_SCALE);
        const double t = (double)(float)((double)scal->wrench[SPH_NOBJ * 3 + 3 * o + k] / SPH_WRENCH_SCALE);
        scal->wrench[3 * o + k] = 0;
        scal->wrench[SPH_NOBJ * 3 + 3 * o + k] = 0;
        b->force[k] = f; b->torque[k] = t;
        b->impulse[k] = b->impulse[k] + a.dt * f;
        b->angular_impulse[k] = b->angular_impulse[k] + a.dt * t;
        b->com[k] = com[k]; b->vel[k] = vel[k]; b->angvel[k] = w[k];
        pose->com[o][k] = (float)com[k]; pose->vel[o][k] = (float)vel[k]; pose->angvel[o][k] = (float)w[k];
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) { b->rot[q] = rot[q]; pose->rot[o][q] = (float)rot[q]; }
    b->steps = a.k + 1;
}

static void l_rigid_motion(State &s) {
    if (s.rigid_motion_args.nbodies <= 0 || !s.rigid_motion) return;
    hipLaunchKernelGGL(k_rigid_motion, dim3(s.rigid_motion_args.nbodies), dim3(64), 0, s.stream, s.rigid_motion_args, s.rigid_motion, s.scal,
                       s.pose);
}

static void register_rigid_motion_launchers(Launch &L) { L.rigid_motion = l_rigid_motion; }
