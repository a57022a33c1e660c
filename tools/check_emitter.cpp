// check_emitter.cpp -- the evaluator of the fluid emitters (csrc/sph_emitter_eval.hpp, the source the kernels and sph_emitter_eval_host
// compile) on the CPU, under the host sanitizers: a few thousand random valid programs, with the invariants the CPU tests check on the
// model (tests/test_emitter_host.py).
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_emitter.cpp \
//       -o check_emitter && ./check_emitter > profiles/emitter_host_check.txt
//   ./check_emitter N SEED     N programs (default 4000), seed (default 1)
//
// Per program, the counts k = 0 .. 120 and a few large ones:
//   born(k) is monotone and grows by at most one per step; a newborn layer lies 0 <= a_j < speed dt in front of the plane; consecutive
//   layers are one spacing apart to 1e-12 relative; the held range lies inside [0, born], holds at most `hold` + 1 layers and is empty
//   past `end`; born(k) never exceeds max_layers; the lattice has layer_n points (the circle: counted by brute force), is centred, and
//   em_point walks it in order (j slow, i fast) without leaving the nozzle; every position is finite.
// Prints the worst value of each and the number of violations (0 = all hold); exits 1 if there is one.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include "../include/sph_hip.h"
#include "../sph_project_amd/csrc/sph_emitter_eval.hpp"

static std::mt19937_64 rng;
static double uni(double a, double b) { return a + (b - a) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
static int pick(int n) { return (int)(rng() % (uint64_t)n); }
static void unit(double *v) {
    double n;
    do { for (int k = 0; k < 3; ++k) v[k] = uni(-1.0, 1.0); n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); } while (n < 0.1);
    for (int k = 0; k < 3; ++k) v[k] /= n;
}

static void random_program(SphEmitter *e, double dt, double spacing) {
    memset(e, 0, sizeof(*e));
    e->object_id = pick(SPH_MAX_OBJECTS);
    e->shape = pick(5) < 2 ? SPH_EMITTER_CIRCLE : SPH_EMITTER_RECTANGLE;
    e->hold = pick(SPH_EMITTER_MAX_HOLD + 1);
    for (int k = 0; k < 3; ++k) e->position[k] = uni(0.1, 2.0);
    unit(e->direction);
    double up[3];
    for (;;) {
        unit(up);
        const double d = up[0] * e->direction[0] + up[1] * e->direction[1] + up[2] * e->direction[2];
        double n = 0.0;
        for (int k = 0; k < 3; ++k) { e->tangent2[k] = up[k] - d * e->direction[k]; n += e->tangent2[k] * e->tangent2[k]; }
        if (n < 0.01) continue;
        n = sqrt(n);
        for (int k = 0; k < 3; ++k) e->tangent2[k] /= n;
        break;
    }
    e->tangent1[0] = e->tangent2[1] * e->direction[2] - e->tangent2[2] * e->direction[1];
    e->tangent1[1] = e->tangent2[2] * e->direction[0] - e->tangent2[0] * e->direction[2];
    e->tangent1[2] = e->tangent2[0] * e->direction[1] - e->tangent2[1] * e->direction[0];
    if (e->shape == SPH_EMITTER_CIRCLE) e->radius = uni(0.55, 9.0) * spacing;
    else { e->width = uni(1.02, 14.0) * spacing; e->height = uni(1.02, 14.0) * spacing; }
    e->speed = uni(0.02, 0.5) * spacing / dt;
    e->start = pick(3) == 0 ? 0.0 : uni(0.0, 30.0) * dt;
    e->end = pick(3) == 0 ? INFINITY : e->start + uni(0.5, 90.0) * dt;
    e->density = uni(500.0, 2000.0);
}

int main(int argc, char **argv) {
    const long n = argc > 1 ? atol(argv[1]) : 4000;
    rng.seed(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1ull);
    double worst_gap = 0.0, worst_newborn = 0.0, worst_centre = 0.0;
    long violations = 0, evaluated = 0, layers = 0, points = 0, circles = 0;
    SphEmitter *e = (SphEmitter *)malloc(sizeof(SphEmitter));   // on the heap with nothing behind it
    if (!e) return 2;
    for (long p = 0; p < n; ++p) {
        const double dt = (double)(float)uni(1e-4, 2e-3), spacing = uni(0.004, 0.05);
        random_program(e, dt, spacing);
        int nu, nv;
        em_lattice(e, spacing, &nu, &nv);
        const int layer_n = em_layer_count(e, spacing);
        bool bad = nu < 1 || nv < 1 || layer_n < 1;
        // the lattice: brute-force count, order, centre
        int brute = 0;
        double ca = 0.0, cb = 0.0;
        for (int j = 0; j < nv && !bad; ++j)
            for (int i = 0; i < nu; ++i) {
                const double a = em_coord(i, nu, spacing), b = em_coord(j, nv, spacing);
                if (e->shape == SPH_EMITTER_CIRCLE && !(a * a + b * b <= e->radius * e->radius)) continue;
                double pa, pb;
                if (brute < layer_n) {
                    em_point(e, nu, nv, spacing, brute, &pa, &pb);
                    if (pa != a || pb != b) bad = true;
                }
                ca += a; cb += b; ++brute;
            }
        bad = bad || brute != layer_n;
        circles += e->shape == SPH_EMITTER_CIRCLE;
        points += layer_n;
        if (layer_n > 0) worst_centre = fmax(worst_centre, fmax(fabs(ca), fabs(cb)) / layer_n / spacing);
        e->max_particles = layer_n * (1 + pick(40)) + pick(layer_n > 0 ? layer_n : 1);
        const int max_layers = layer_n > 0 ? e->max_particles / layer_n : 0;
        int last = 0;
        for (long long k = 0; k <= 124 && !bad; ++k) {
            const long long kk = k <= 120 ? k : 1000 * (k - 120) + pick(1000000);
            EmSchedule sc;
            em_schedule(e, max_layers, dt, spacing, kk, &sc);
            ++evaluated;
            bad = bad || sc.born < 0 || sc.born > max_layers || sc.held_lo < 0 || sc.held_lo > sc.born || sc.born - sc.held_lo > e->hold + 1 ||
                  !isfinite(sc.s) || sc.s < 0.0;
            if (sc.T > e->end && sc.held_lo != sc.born) bad = true;
            if (k <= 120) {
                if (sc.born < last || sc.born - last > 1) bad = true;
                if (sc.born > last && k > 0) {   // a newborn layer
                    const double a = em_layer_offset(sc.s, sc.born - 1, spacing);
                    worst_newborn = fmax(worst_newborn, a / (e->speed * dt));
                    if (!(a >= 0.0) || !(a < e->speed * dt * (1.0 + 1e-12) + 1e-15)) bad = true;
                    ++layers;
                }
                if (sc.born >= 2) {
                    const double gap = em_layer_offset(sc.s, sc.born - 2, spacing) - em_layer_offset(sc.s, sc.born - 1, spacing);
                    worst_gap = fmax(worst_gap, fabs(gap - spacing) / spacing);
                    if (!(fabs(gap - spacing) <= 1e-12 * spacing)) bad = true;
                }
                last = sc.born;
            }
            if (sc.born > 0) {
                float x[3];
                double a, b;
                em_point(e, nu, nv, spacing, pick(layer_n), &a, &b);
                em_position(e, em_layer_offset(sc.s, sc.born - 1, spacing), a, b, x);
                bad = bad || !isfinite(x[0]) || !isfinite(x[1]) || !isfinite(x[2]) || fabs(a) > 0.5 * nu * spacing || fabs(b) > 0.5 * nv * spacing;
            }
        }
        if (bad && violations++ < 10) fprintf(stderr, "program %ld: shape %d nu %d nv %d layer_n %d (brute force %d)\n", p, e->shape, nu, nv, layer_n, brute);
    }
    free(e);
    printf("check_emitter: %ld random programs (%ld circles), %ld lattice points walked, %ld schedules evaluated, %ld newborn layers\n", n, circles,
           points, evaluated, layers);
    printf("  newborn layer: a_j / (speed dt)              worst %.6f   (must lie in [0, 1))\n", worst_newborn);
    printf("  consecutive layers: |gap - spacing| / spacing   worst %.3e   (bound 1e-12)\n", worst_gap);
    printf("  lattice centre / spacing                        worst %.3e\n", worst_centre);
    printf("  violations %ld\n", violations);
    return violations ? 1 : 0;
}
