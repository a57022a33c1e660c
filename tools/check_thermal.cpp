// check_thermal.cpp -- the pair arithmetic, the finish and the buoyancy of the heat conduction (csrc/sph_thermal.hpp: heat_pair,
// heat_finish, heat_buoyancy, the source the kernels and sph_heat_pair_host / sph_heat_finish_host compile) on the CPU, under the host
// sanitizers: random particles with random neighbourhoods, both forms.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_thermal.cpp \
//       -o check_thermal && ./check_thermal > profiles/thermal_host_check.txt
//   ./check_thermal N SEED     N particles per form (default 100000), seed (default 1)
//
// Per particle: a support radius h over two decades, 1 ... 60 neighbours at 0.05 h ... h in any direction with the cubic spline's
// gradient in float64 rounded once, c_j over two decades (one in eight adiabatic: c_j = 0, T_j = 0), temperatures in -50 ... 400,
// rho_i = 0.5 ... 1.5 rho0, and the step at a random fraction 0 ... 1 of the particle's OWN limit 1 / (2 alpha (rho0 / rho_i) sum c |F|).
//   every term is finite; an adiabatic neighbour's term is exactly 0; a term's sign is that of T_j - T_i (F <= 0) or it is 0;
//   the two forms agree to 1e-5 of the sum of the term magnitudes; the new T lies within [min, max] of T_i and the conducting T_j, up to
//   4e-6 of the range's larger end (the convex combination, rounded); the buoyancy is -beta (T - T_ref) g to 4 units of 2^-24 and
//   points against g exactly when T > T_ref.
// Prints the worst value of each and the number of violations (0 = all hold); exits 1 if there is one.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../sph_project_amd/csrc/sph_thermal.hpp"

static std::mt19937_64 rng;
static double uni(double a, double b) { return a + (b - a) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
static double logu(double a, double b) { return exp(uni(log(a), log(b))); }

// kernel_gradient = s R for the cubic spline in 3-D
static double grad_scale(double r, double h) {
    const double kg = 6.0 * (8.0 / M_PI) / (h * h * h), q = r / h;
    if (!(r > 1e-5 * h) || q > 1.0) return 0.0;
    return (q <= 0.5 ? kg * q * (3.0 * q - 2.0) : -kg * (1.0 - q) * (1.0 - q)) / (r * h);
}

int main(int argc, char **argv) {
    const long N = argc > 1 ? atol(argv[1]) : 100000;
    rng.seed(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
    long bad = 0, pairs = 0, adiabatic = 0;
    double worst_forms = 0.0, worst_out = 0.0, worst_buoy = 0.0, max_rate = 0.0;
    for (long p = 0; p < N; ++p) {
        const double h = logu(0.004, 0.4), rho0 = uni(500.0, 2000.0), alpha = logu(1e-7, 1e-1);
        const float eps = (float)(0.01 * h * h), rho_i = (float)(rho0 * uni(0.5, 1.5)), Ti = (float)uni(-50.0, 400.0);
        const int nn = 1 + (int)(rng() % 60);
        float sum[2] = {0.0f, 0.0f};
        double mag = 0.0, weight = 0.0, lo = Ti, hi = Ti;
        for (int k = 0; k < nn; ++k) {
            double d[3], dn;
            do { for (int c = 0; c < 3; ++c) d[c] = uni(-1.0, 1.0); dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); } while (dn < 0.1);
            const double r = h * uni(0.05, 1.0);
            const float dx = (float)(r * d[0] / dn), dy = (float)(r * d[1] / dn), dz = (float)(r * d[2] / dn);
            const double r2d = (double)dx * dx + (double)dy * dy + (double)dz * dz;
            const float r2 = (float)r2d;
            const double s = grad_scale(sqrt(r2d), h);
            const bool wall_off = (rng() % 8) == 0;
            const float cj = wall_off ? 0.0f : (float)(h * h * h * logu(0.01, 1.0)), Tj = wall_off ? 0.0f : (float)uni(-50.0, 400.0);
            const float t0 = heat_pair<false>(Ti, cj, Tj, dx, dy, dz, r2, eps, 0.0f, (float)(s * dx), (float)(s * dy), (float)(s * dz));
            const float t1 = heat_pair<true>(Ti, cj, Tj, dx, dy, dz, r2, eps, (float)s, 0.0f, 0.0f, 0.0f);
            ++pairs;
            if (!isfinite(t0) || !isfinite(t1)) ++bad;
            if (wall_off) { ++adiabatic; if (t0 != 0.0f || t1 != 0.0f) ++bad; continue; }
            const float want = Tj - Ti;   // F <= 0: the term pulls T_i towards T_j
            if ((t0 != 0.0f && (t0 > 0.0f) != (want > 0.0f)) || (t1 != 0.0f && (t1 > 0.0f) != (want > 0.0f))) ++bad;
            sum[0] += t0; sum[1] += t1;
            mag += fabs((double)t0);
            weight += (double)cj * fabs(s * r2d / (r2d + (double)eps));
            if (Tj < lo) lo = Tj;
            if (Tj > hi) hi = Tj;
        }
        if (mag > 0.0) {
            const double fr = fabs((double)sum[0] - (double)sum[1]) / mag;
            if (fr > worst_forms) worst_forms = fr;
            if (!(fr <= 1e-5)) ++bad;
        }
        const float k2a = (float)(2.0 * alpha);
        const double own_limit = weight > 0.0 ? 1.0 / ((double)k2a * (rho0 / (double)rho_i) * weight) : 1.0;
        const float dt = (float)(own_limit * uni(0.0, 1.0) * (1.0 - 1e-5));
        for (int f = 0; f < 2; ++f) {
            float rate, Tn;
            if (f) heat_finish<true>(sum[f], k2a, (float)rho0, rho_i, dt, Ti, &rate, &Tn);
            else heat_finish<false>(sum[f], k2a, (float)rho0, rho_i, dt, Ti, &rate, &Tn);
            if (!isfinite(rate) || !isfinite(Tn)) { ++bad; continue; }
            if (fabs((double)rate) > max_rate) max_rate = fabs((double)rate);
            const double slack = 4e-6 * fmax(fabs(lo), fabs(hi));
            const double out = fmax(lo - (double)Tn, (double)Tn - hi) / fmax(fmax(fabs(lo), fabs(hi)), 1e-30);
            if (out > worst_out) worst_out = out;
            if ((double)Tn < lo - slack || (double)Tn > hi + slack) ++bad;
        }
        const double beta = uni(0.0, 1e-2), t_ref = uni(-20.0, 100.0), g[3] = {uni(-3.0, 3.0), uni(-12.0, -6.0), uni(-3.0, 3.0)};
        const HeatConsts hc = heat_consts(alpha, beta, t_ref);
        float a[3];
        heat_buoyancy(hc.kb, Ti, hc.t_ref, (float)g[0], (float)g[1], (float)g[2], a);
        for (int c = 0; c < 3; ++c) {
            const double want = (double)hc.kb * ((double)Ti - (double)hc.t_ref) * (double)(float)g[c];
            const double e = fabs((double)a[c] - want) / fmax(fabs(want), 1e-300) / ldexp(1.0, -24);
            if (want != 0.0 && e > worst_buoy) worst_buoy = e;
            if (!isfinite(a[c]) || (want != 0.0 && !(e <= 4.0))) ++bad;
        }
        if (beta > 0.0 && Ti > hc.t_ref && !(a[1] > 0.0f)) ++bad;   // hotter than the reference: up, against g
        if (beta > 0.0 && Ti < hc.t_ref && !(a[1] < 0.0f)) ++bad;
    }
    printf("check_thermal: %ld particles per form, %ld pairs (%ld adiabatic: every term exactly 0)\n", N, pairs, adiabatic);
    printf("  worst strict - fast = %.3g of sum |term| (bound 1e-5), largest |dT/dt| = %.4g K / s\n", worst_forms, max_rate);
    printf("  new T outside [min, max] of its neighbourhood by at most %.3g of the range's larger end (bound 4e-6; below the own limit)\n", worst_out);
    printf("  buoyancy: worst error %.2f x 2^-24 (bound 4)\n", worst_buoy);
    printf("  violations: %ld\n", bad);
    return bad ? 1 : 0;
}
