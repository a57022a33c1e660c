// check_drag.cpp -- the per-particle arithmetic of the air drag (csrc/sph_drag.hpp: drag_host_constants, dr_cbrt, drag_dir, drag_finish,
// the source the kernels and sph_drag_particle_host compile) on the CPU, under the host sanitizers: a few hundred thousand random
// records, both forms, over random radii, densities, winds and scales.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_drag.cpp \
//       -o check_drag && ./check_drag > profiles/drag_host_check.txt
//   ./check_drag N SEED     N records per form (default 300000), seed (default 1)
//
// Per record (speeds 1e-5 ... 60 m / s, any direction, n_i 0 ... 80, q 0 ... 1 with the ends, masses over two decades):
//   every output is finite; 0 <= w <= 1; below the threshold everything is 0, above it C_D > 0, A_un > 0, 0 <= y <= 1 and a_drag is
//   parallel to v_rel (|a x v_rel| <= 1e-5 |a| |v_rel|) and points along it; the direction of drag_dir is a unit vector to 1e-6; the two
//   forms agree to 1e-5 relative.  The cube root: 1e5 arguments over 0.2 ... 1000 against cbrt in double, worst error in units of 2^-24.
// Prints the worst value of each and the number of violations (0 = all hold); exits 1 if there is one.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../sph_project_amd/csrc/sph_drag.hpp"

static std::mt19937_64 rng;
static double uni(double a, double b) { return a + (b - a) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
static double logu(double a, double b) { return exp(uni(log(a), log(b))); }

int main(int argc, char **argv) {
    const long N = argc > 1 ? atol(argv[1]) : 300000;
    rng.seed(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
    long bad = 0, below = 0, refused = 0;
    double worst_cross = 0.0, worst_unit = 0.0, worst_forms = 0.0, min_cd = 1e30, max_cd = 0.0, max_a = 0.0, worst_cbrt = 0.0;
    for (int i = 0; i < 100000; ++i) {
        const float x = (float)logu(0.2, 1000.0);
        const double e = fabs((double)dr_cbrt(x) / cbrt((double)x) - 1.0) / ldexp(1.0, -24);
        if (e > worst_cbrt) worst_cbrt = e;
        if (!(e <= 7.0)) ++bad;
    }
    DragHost hk;
    if (drag_host_constants(1e-9, 1000.0, 1.2041, hk)) ++bad;   // overdamped: must be refused
    for (long r = 0; r < N; ++r) {
        const double radius = logu(1e-3, 0.1), rho_l = uni(500.0, 2000.0), rho_a = uni(0.0, 3.0), k = uni(0.0, 50.0);
        if (!drag_host_constants(radius, rho_l, rho_a, hk)) { ++refused; continue; }
        double u[3];
        const double us = (rng() & 1) ? 0.0 : logu(1e-3, 30.0);
        for (int c = 0; c < 3; ++c) u[c] = us * uni(-1.0, 1.0);
        const DragConsts kc = drag_consts(hk, radius, rho_a, k, u);
        const double s = logu(1e-5, 60.0);
        double d[3], dn;
        do { for (int c = 0; c < 3; ++c) d[c] = uni(-1.0, 1.0); dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); } while (dn < 0.1);
        const float v[3] = {(float)(u[0] - s * d[0] / dn), (float)(u[1] - s * d[1] / dn), (float)(u[2] - s * d[2] / dn)};
        const float m = (float)(rho_l * 0.8 * pow(2.0 * radius, 3.0) * logu(0.1, 10.0));
        const float n = (float)(rng() % 81);
        const int pick = (int)(rng() % 8);
        const float q = pick == 0 ? 0.0f : pick == 1 ? 1.0f : (float)uni(0.0, 1.0);
        DragOut o[2];
        drag_finish<false>(kc, v[0], v[1], v[2], m, n, q, o[0]);
        drag_finish<true>(kc, v[0], v[1], v[2], m, n, q, o[1]);
        const double rx = (double)kc.ux - v[0], ry = (double)kc.uy - v[1], rz = (double)kc.uz - v[2];
        const double rn = sqrt(rx * rx + ry * ry + rz * rz);
        for (int f = 0; f < 2; ++f) {
            const DragOut &p = o[f];
            const float all[7] = {p.ax, p.ay, p.az, p.w, p.cd, p.a_un, p.y};
            for (int c = 0; c < 7; ++c) if (!isfinite(all[c])) ++bad;
            if (!(p.w >= 0.0f && p.w <= 1.0f)) ++bad;
            float ex, ey, ez;
            if (f) drag_dir<true>(kc, v[0], v[1], v[2], ex, ey, ez); else drag_dir<false>(kc, v[0], v[1], v[2], ex, ey, ez);
            const double en = sqrt((double)ex * ex + (double)ey * ey + (double)ez * ez);
            if (p.cd == 0.0f) {   // below the threshold: everything is zero, the direction too
                if (f == 0) ++below;
                for (int c = 0; c < 7; ++c) if (all[c] != 0.0f) ++bad;
                if (en != 0.0 || rn * rn > 1.1e-6) ++bad;
                continue;
            }
            if (rn * rn < 0.9e-6) ++bad;
            if (fabs(en - 1.0) > worst_unit) worst_unit = fabs(en - 1.0);
            if (!(fabs(en - 1.0) <= 1e-6)) ++bad;
            if (!(p.cd > 0.0f) || !(p.a_un > 0.0f) || !(p.y >= 0.0f && p.y <= 1.0f)) ++bad;
            if (p.cd < min_cd) min_cd = p.cd;
            if (p.cd > max_cd) max_cd = p.cd;
            const double an = sqrt((double)p.ax * p.ax + (double)p.ay * p.ay + (double)p.az * p.az);
            if (an > max_a) max_a = an;
            if (an > 0.0) {
                const double cx = p.ay * rz - p.az * ry, cy = p.az * rx - p.ax * rz, cz = p.ax * ry - p.ay * rx;
                const double cr = sqrt(cx * cx + cy * cy + cz * cz) / (an * rn);
                if (cr > worst_cross) worst_cross = cr;
                if (!(cr <= 1e-5) || !(p.ax * rx + p.ay * ry + p.az * rz > 0.0)) ++bad;
            } else if (p.w != 0.0f && k != 0.0 && rho_a != 0.0 && an != 0.0) ++bad;
        }
        if (o[0].cd != 0.0f) {
            const double a0 = sqrt((double)o[0].ax * o[0].ax + (double)o[0].ay * o[0].ay + (double)o[0].az * o[0].az);
            const double da = sqrt(pow((double)o[0].ax - o[1].ax, 2) + pow((double)o[0].ay - o[1].ay, 2) + pow((double)o[0].az - o[1].az, 2));
            const double fr = fmax(a0 > 0.0 ? da / a0 : 0.0, fabs((double)o[0].cd - o[1].cd) / o[0].cd);
            if (fr > worst_forms) worst_forms = fr;
            if (!(fr <= 1e-5)) ++bad;
        }
    }
    printf("check_drag: %ld records per form (%ld below the threshold, %ld parameter sets refused as overdamped)\n", N - refused, below, refused);
    printf("  cube root: worst |dr_cbrt / cbrt - 1| = %.2f x 2^-24 over 100000 arguments in [0.2, 1000] (bound 7)\n", worst_cbrt);
    printf("  worst | |e| - 1 | = %.3g, worst |a x v_rel| / (|a| |v_rel|) = %.3g, worst strict - fast = %.3g relative\n", worst_unit, worst_cross, worst_forms);
    printf("  C_D in [%.4g, %.4g], largest |a_drag| = %.4g m / s^2\n", min_cd, max_cd, max_a);
    printf("  violations: %ld\n", bad);
    return bad ? 1 : 0;
}
