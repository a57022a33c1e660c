// check_rigid_motion.cpp -- the evaluator of the scripted rigid bodies (csrc/sph_rigid_motion_eval.hpp, the source the kernel and
// sph_rigid_motion_eval_host compile) on the CPU, under the host sanitizers: a few thousand random valid programs at random step
// indices, with the invariants the CPU tests check (tests/test_rigid_motion_host.py).
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_rigid_motion.cpp \
//       -o check_rigid_motion && ./check_rigid_motion > profiles/rigid_motion_host_check.txt
//   ./check_rigid_motion N SEED     N programs (default 4000), seed (default 1)
//
// Per program, 8 steps k (small ones, ones around `start` and `end`, large ones up to 10^7):
//   rot rot^T = I within 1e-12; com_k + dt * vel = com_{k+1} within 4 ulp of |com|; exp([dt angvel]x) rot_k = rot_{k+1} within 1e-12;
//   everything finite; a step that lies wholly before `start` or behind `end` has zero velocities.
// The programs turn a body by less than about 2.5 rad per step (the backward difference of a turn near pi is ill-conditioned, and a
// program that fast is its author's responsibility).
// Prints the worst value of each and the number of violations (0 = all hold); exits 1 if there is one.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include "../include/sph_hip.h"
#include "../sph_project_amd/csrc/sph_rigid_motion_eval.hpp"

static std::mt19937_64 rng;
static double uni(double a, double b) { return a + (b - a) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
static int pick(int n) { return (int)(rng() % (uint64_t)n); }
static void unit(double *v) {
    double n;
    do { for (int k = 0; k < 3; ++k) v[k] = uni(-1.0, 1.0); n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); } while (n < 0.1);
    for (int k = 0; k < 3; ++k) v[k] /= n;
}

static void random_program(SphRigidMotion *m, double dt) {
    memset(m, 0, sizeof(*m));
    m->start = pick(3) == 0 ? 0.0 : uni(0.0, 40.0) * dt;
    m->end = pick(3) == 0 ? INFINITY : m->start + uni(0.5, 400.0) * dt;
    for (int k = 0; k < 3; ++k) m->pivot[k] = uni(-0.2, 0.2);
    const int blocks = 1 + pick(7);   // bit 0 keyframes, 1 harmonic, 2 drift: at least one
    if (blocks & 1) {
        const int choices[] = {1, 2, 3, 17, 63, 64};
        m->nkeys = choices[pick(6)];
        m->interpolation = pick(2);
        m->repeat = pick(3);
        double t = 0.0;
        for (int i = 0; i < m->nkeys; ++i) {
            m->key_times[i] = t;
            t += uni(1.5, 30.0) * dt;
            for (int k = 0; k < 3; ++k) { m->key_translations[i][k] = uni(-0.1, 0.1); m->key_rotations[i][k] = uni(-0.5, 0.5); }
        }
    }
    if (blocks & 2) {
        m->frequency = pick(5) == 0 ? 0.0 : uni(0.1, 0.15 / dt);
        m->phase = uni(-3.2, 3.2);
        m->ramp = pick(2) ? 0.0 : uni(0.5, 200.0) * dt;
        if (pick(4)) { unit(m->direction); m->amplitude = uni(-0.1, 0.1); }
        if (pick(4)) { unit(m->axis); m->angle = uni(-0.5, 0.5); }
    }
    if (blocks & 4) {
        for (int k = 0; k < 3; ++k) m->drift_velocity[k] = uni(-2.0, 2.0);
        if (pick(4)) { unit(m->drift_axis); m->drift_rate = uni(-0.3, 0.3) / dt; }
    }
}

int main(int argc, char **argv) {
    const long n = argc > 1 ? atol(argv[1]) : 4000;
    rng.seed(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1ull);
    double worst_orth = 0.0, worst_com_ulp = 0.0, worst_rot = 0.0;
    long violations = 0, evaluated = 0, held = 0;
    // the program lives on the heap with nothing behind it: a read past the 64th key is the sanitizer's to find
    SphRigidMotion *m = (SphRigidMotion *)malloc(sizeof(SphRigidMotion));
    if (!m) return 2;
    for (long p = 0; p < n; ++p) {
        const double dt = (double)(float)uni(1e-4, 2e-3);
        random_program(m, dt);
        double c0[3], w0[3], R0[9];
        for (int k = 0; k < 3; ++k) { c0[k] = uni(0.0, 3.0); w0[k] = uni(-3.0, 3.0); }
        rm_skew_exp(w0, R0);
        const long long k_start = (long long)(m->start / dt), k_end = isfinite(m->end) ? (long long)(m->end / dt) : 1000;
        const long long ks[8] = {0, 1, (long long)pick(200), k_start > 0 ? k_start - 1 : 0, k_start, k_end, k_end + 2, (long long)pick(10000000)};
        for (int q = 0; q < 8; ++q) {
            const long long k = ks[q];
            double ca[3], Ra[9], com[3], rot[9], vel[3], w[3];
            rm_pose(m, c0, R0, (double)k * dt, ca, Ra);
            rm_step(m, c0, R0, dt, k, com, rot, vel, w);
            ++evaluated;
            bool bad = false;
            for (int j = 0; j < 3; ++j) bad = bad || !isfinite(com[j]) || !isfinite(vel[j]) || !isfinite(w[j]);
            double RRt[9], orth = 0.0;
            rm_mul_t(rot, rot, RRt);
            for (int j = 0; j < 9; ++j) { bad = bad || !isfinite(rot[j]); orth = fmax(orth, fabs(RRt[j] - (j % 4 == 0 ? 1.0 : 0.0))); }
            double cmax = 0.0;
            for (int j = 0; j < 3; ++j) cmax = fmax(cmax, fabs(com[j]));
            const double ulp = nextafter(cmax, INFINITY) - cmax;
            double com_ulp = 0.0;
            for (int j = 0; j < 3; ++j) com_ulp = fmax(com_ulp, fabs((ca[j] + dt * vel[j]) - com[j]) / ulp);
            const double dtw[3] = {dt * w[0], dt * w[1], dt * w[2]};
            double E[9], ER[9], drot = 0.0;
            rm_skew_exp(dtw, E);
            rm_mul(E, Ra, ER);
            for (int j = 0; j < 9; ++j) drot = fmax(drot, fabs(ER[j] - rot[j]));
            const bool outside = (double)(k + 1) * dt <= m->start || (double)k * dt >= m->end;
            if (outside) {
                ++held;
                for (int j = 0; j < 3; ++j) bad = bad || vel[j] != 0.0 || w[j] != 0.0;
            }
            worst_orth = fmax(worst_orth, orth); worst_com_ulp = fmax(worst_com_ulp, com_ulp); worst_rot = fmax(worst_rot, drot);
            if (bad || !(orth <= 1e-12) || !(com_ulp <= 4.0) || !(drot <= 1e-12)) {
                if (violations++ < 10)
                    fprintf(stderr, "program %ld step %lld: orth %.3e com %.2f ulp rot %.3e%s\n", p, k, orth, com_ulp, drot, bad ? " (not finite, or moving while held)" : "");
            }
        }
    }
    free(m);
    printf("check_rigid_motion: %ld random programs, %ld steps evaluated (%ld of them wholly before start or behind end)\n", n, evaluated, held);
    printf("  rot rot^T = I                          worst %.3e   (bound 1e-12)\n", worst_orth);
    printf("  com_k + dt vel = com_k+1               worst %.2f ulp of |com|   (bound 4)\n", worst_com_ulp);
    printf("  exp([dt angvel]x) rot_k = rot_k+1      worst %.3e   (bound 1e-12)\n", worst_rot);
    printf("  violations %ld\n", violations);
    return violations ? 1 : 0;
}
