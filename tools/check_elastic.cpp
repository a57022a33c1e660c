// check_elastic.cpp -- the rotation extraction of the elastic solids (el_extract_rotation of csrc/sph_elastic.hpp, the source the
// kernels and sph_elastic_particle_host compile) on the CPU, under the host sanitizers: a few thousand random deformation gradients
// F = rotation x stretch, iterated to convergence, against the float64 polar factor.  A stand-alone program: never loaded into
// python, never run on a GPU.
//
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       --offload-arch=gfx950 tools/check_elastic.cpp -o check_elastic && ./check_elastic > profiles/elastic_host_check.txt
//   (or, the host compiler alone:  g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all ...)
//   ./check_elastic N SEED     N matrices (default 4000), seed (default 1)
//
// Per matrix: a rotation by a uniform angle in [0, 170] degrees about a uniform axis, times a symmetric stretch with eigenvalues in
// [0.6, 1.5] about random axes, rounded to f32.  From the identity quaternion, rounds of ELASTIC_ROT_ITERS iterations until a round
// moves q by less than 1e-6 (the sum of the four changes: a few f32 ulp; at most 200 rounds).  Then R = mat(q):
//   R R^T = I within 1e-5; det R = +1 within 1e-5; |R - polar(F)| (largest entry) within 1e-5, polar(F) by Newton's iteration
//   R <- (R + R^-T) / 2 in float64; everything finite; pass-A's stress of (F, R) symmetric by construction and finite.
// Prints the worst value of each, the largest number of rounds, and the number of violations (0 = all hold); exits 1 if there is one.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include "../sph_project_amd/csrc/sph_elastic.hpp"

static std::mt19937_64 rng;
static double uni(double a, double b) { return a + (b - a) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }

static void axis_angle(const double ax[3], double ang, double R[9]) {
    const double c = cos(ang), s = sin(ang), t = 1.0 - c, x = ax[0], y = ax[1], z = ax[2];
    const double r[9] = {t * x * x + c, t * x * y - s * z, t * x * z + s * y, t * x * y + s * z, t * y * y + c, t * y * z - s * x,
                         t * x * z - s * y, t * y * z + s * x, t * z * z + c};
    memcpy(R, r, sizeof(r));
}
static void random_axis(double ax[3]) {
    double n;
    do { for (int k = 0; k < 3; ++k) ax[k] = uni(-1.0, 1.0); n = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]); } while (n < 0.1 || n > 1.0);
    for (int k = 0; k < 3; ++k) ax[k] /= n;
}
static void mul(const double A[9], const double B[9], double C[9]) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[3 * a + b] = A[3 * a] * B[b] + A[3 * a + 1] * B[3 + b] + A[3 * a + 2] * B[6 + b];
}
static double det3(const double M[9]) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
static void inv_transpose(const double M[9], double O[9]) {   // (M^-1)^T = cofactors / det
    const double d = 1.0 / det3(M);
    O[0] = (M[4] * M[8] - M[5] * M[7]) * d; O[1] = (M[5] * M[6] - M[3] * M[8]) * d; O[2] = (M[3] * M[7] - M[4] * M[6]) * d;
    O[3] = (M[2] * M[7] - M[1] * M[8]) * d; O[4] = (M[0] * M[8] - M[2] * M[6]) * d; O[5] = (M[1] * M[6] - M[0] * M[7]) * d;
    O[6] = (M[1] * M[5] - M[2] * M[4]) * d; O[7] = (M[2] * M[3] - M[0] * M[5]) * d; O[8] = (M[0] * M[4] - M[1] * M[3]) * d;
}
static void polar(const double F[9], double R[9]) {
    memcpy(R, F, 9 * sizeof(double));
    for (int it = 0; it < 60; ++it) {
        double T[9], delta = 0.0;
        inv_transpose(R, T);
        for (int k = 0; k < 9; ++k) { const double n = 0.5 * (R[k] + T[k]); delta = fmax(delta, fabs(n - R[k])); R[k] = n; }
        if (delta < 1e-15) break;
    }
}

int main(int argc, char **argv) {
    const long n = argc > 1 ? atol(argv[1]) : 4000;
    rng.seed(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
    double worst_orth = 0.0, worst_det = 0.0, worst_polar = 0.0, worst_angle = 0.0;
    int worst_rounds = 0;
    long bad = 0;
    for (long t = 0; t < n; ++t) {
        double ax[3], Rot[9], Q[9], S[9], D[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, QD[9], Qt[9], Fd[9];
        random_axis(ax);
        const double ang = uni(0.0, 170.0) * M_PI / 180.0;
        axis_angle(ax, ang, Rot);
        random_axis(ax);
        axis_angle(ax, uni(0.0, M_PI), Q);
        D[0] = uni(0.6, 1.5); D[4] = uni(0.6, 1.5); D[8] = uni(0.6, 1.5);
        mul(Q, D, QD);
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) Qt[3 * a + b] = Q[3 * b + a];
        mul(QD, Qt, S);
        mul(Rot, S, Fd);
        float F[9], q[4] = {0.0f, 0.0f, 0.0f, 1.0f};
        for (int k = 0; k < 9; ++k) { F[k] = (float)Fd[k]; Fd[k] = (double)F[k]; }
        int rounds = 0;
        for (; rounds < 200; ++rounds) {
            const float p[4] = {q[0], q[1], q[2], q[3]};
            el_extract_rotation(q, F, ELASTIC_ROT_ITERS);
            const double d = fabs((double)q[0] - p[0]) + fabs((double)q[1] - p[1]) + fabs((double)q[2] - p[2]) + fabs((double)q[3] - p[3]);
            if (d < 1e-6) { ++rounds; break; }
        }
        float Rf[9], sig[6];
        el_quat_matrix(q, Rf);
        el_stress(F, Rf, 1.0f, 1.5f, sig);
        double R[9], P[9], orth = 0.0, dist = 0.0;
        for (int k = 0; k < 9; ++k) R[k] = (double)Rf[k];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                orth = fmax(orth, fabs(R[3 * a] * R[3 * b] + R[3 * a + 1] * R[3 * b + 1] + R[3 * a + 2] * R[3 * b + 2] - (a == b ? 1.0 : 0.0)));
        const double dd = fabs(det3(R) - 1.0);
        polar(Fd, P);
        for (int k = 0; k < 9; ++k) dist = fmax(dist, fabs(R[k] - P[k]));
        bool finite = true;
        for (int k = 0; k < 4; ++k) finite = finite && isfinite(q[k]);
        for (int k = 0; k < 6; ++k) finite = finite && isfinite(sig[k]);
        if (!finite || orth > 1e-5 || dd > 1e-5 || dist > 1e-5) {
            if (++bad <= 5) fprintf(stderr, "matrix %ld: angle %.2f deg, rounds %d, orthonormality %.3e, det - 1 %.3e, distance %.3e, finite %d\n", t, ang * 180.0 / M_PI, rounds, orth, dd, dist, (int)finite);
        }
        worst_orth = fmax(worst_orth, orth); worst_det = fmax(worst_det, dd);
        if (dist > worst_polar) { worst_polar = dist; worst_angle = ang * 180.0 / M_PI; }
        if (rounds > worst_rounds) worst_rounds = rounds;
    }
    printf("check_elastic: %ld random F = rotation (0 .. 170 degrees) x stretch (0.6 .. 1.5), el_extract_rotation from the identity to convergence\n", n);
    printf("  worst |R R^T - I|            %.3e   (bound 1e-5)\n", worst_orth);
    printf("  worst |det R - 1|            %.3e   (bound 1e-5)\n", worst_det);
    printf("  worst |R - polar(F)|         %.3e   (bound 1e-5; at a rotation of %.1f degrees)\n", worst_polar, worst_angle);
    printf("  most rounds of %d iterations  %d\n", ELASTIC_ROT_ITERS, worst_rounds);
    printf("  violations                   %ld\n", bad);
    return bad ? 1 : 0;
}
