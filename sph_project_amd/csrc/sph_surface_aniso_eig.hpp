// sph_surface_aniso_eig.hpp -- the kernel matrix of one particle from its weighted covariance: a cyclic
// Jacobi eigen-decomposition of a symmetric 3x3 in f32 with a fixed number of sweeps, and the shrink-only clamp.  __host__ __device__:
// the moments kernel of sph_surface_aniso.hpp and sph_surface_aniso_matrix_host (sph_surface_api.hpp) compile this same source.
// Symmetric matrices are (xx, xy, xz, yy, yz, zz).
#pragma once

#define SURF_ANISO_SWEEPS 6   // f32 converges in 4 on every matrix of tests/test_surface_aniso_host.py; no data-dependent trip count

// one Jacobi rotation in the (P, Q) plane, R the third index: a[P][Q] -> 0 (Numerical Recipes' update; an exact zero is left alone)
#define SURF_JACOBI_ROTATE(P, Q, R)                                                          \
    do {                                                                                     \
        const float apq = a[P][Q];                                                           \
        if (apq != 0.0f) {                                                                   \
            const float theta = (a[Q][Q] - a[P][P]) / (2.0f * apq);                          \
            const float t = (theta >= 0.0f ? 1.0f : -1.0f) / (fabsf(theta) + __builtin_sqrtf(theta * theta + 1.0f)); \
            const float c = 1.0f / __builtin_sqrtf(t * t + 1.0f), s = t * c;                 \
            a[P][P] -= t * apq;                                                              \
            a[Q][Q] += t * apq;                                                              \
            a[P][Q] = a[Q][P] = 0.0f;                                                        \
            const float arp = a[R][P], arq = a[R][Q];                                        \
            a[R][P] = a[P][R] = c * arp - s * arq;                                           \
            a[R][Q] = a[Q][R] = s * arp + c * arq;                                           \
            _Pragma("unroll") for (int k_ = 0; k_ < 3; ++k_) {                               \
                const float vp = v[k_][P], vq = v[k_][Q];                                    \
                v[k_][P] = c * vp - s * vq;                                                  \
                v[k_][Q] = s * vp + c * vq;                                                  \
            }                                                                                \
        }                                                                                    \
    } while (0)

// A (and det A) of a particle with covariance C and nb neighbours.  Returns 0: anisotropic, every ratio inside the clamp; 1: the sparse
// rule (A = I / sparse_scale); 2: anisotropic with at least one ratio clamped.
__host__ __device__ inline int surf_aniso_matrix(const float C[6], int nb, const SurfAnisoPrm &p, float A[6], float *det) {
    const float m = fmaxf(C[0], fmaxf(C[3], C[5]));   // lambda_1 >= the largest diagonal entry: C = 0 (or not finite) <=> !(m > 0)
    bool sparse = nb < p.min_nb || !(m > 0.0f) || !(m < 3.0e38f);
    float a[3][3], v[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}}, lam = 0.0f;
    if (!sparse) {
        // the ratios do not depend on the scale: C / m keeps every product of the sweeps far from the ends of the f32 range
        a[0][0] = C[0] / m; a[1][1] = C[3] / m; a[2][2] = C[5] / m;
        a[0][1] = a[1][0] = C[1] / m; a[0][2] = a[2][0] = C[2] / m; a[1][2] = a[2][1] = C[4] / m;
#pragma unroll 1
        for (int sweep = 0; sweep < SURF_ANISO_SWEEPS; ++sweep) {
            SURF_JACOBI_ROTATE(0, 1, 2);
            SURF_JACOBI_ROTATE(0, 2, 1);
            SURF_JACOBI_ROTATE(1, 2, 0);
        }
        lam = fmaxf(a[0][0], fmaxf(a[1][1], a[2][2]));
        sparse = !(lam > 0.0f);
    }
    if (sparse) {
        A[0] = A[3] = A[5] = p.inv_scale;
        A[1] = A[2] = A[4] = 0.0f;
        *det = p.inv_scale * p.inv_scale * p.inv_scale;
        return 1;
    }
    bool clamped = false;
    float s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float ratio = a[k][k] / lam;
        clamped |= ratio < p.inv_ratio;
        s[k] = 1.0f / fmaxf(ratio, p.inv_ratio);   // in [1, max_ratio]
    }
    // A = sum_k s_k v_k v_k^T, v_k = column k of v, summed in the order k = 0, 1, 2
#define SURF_ANISO_ENTRY(I, J) (s[0] * v[I][0] * v[J][0] + s[1] * v[I][1] * v[J][1] + s[2] * v[I][2] * v[J][2])
    A[0] = SURF_ANISO_ENTRY(0, 0); A[1] = SURF_ANISO_ENTRY(0, 1); A[2] = SURF_ANISO_ENTRY(0, 2);
    A[3] = SURF_ANISO_ENTRY(1, 1); A[4] = SURF_ANISO_ENTRY(1, 2); A[5] = SURF_ANISO_ENTRY(2, 2);
#undef SURF_ANISO_ENTRY
    *det = s[0] * s[1] * s[2];
    return clamped ? 2 : 0;
}
