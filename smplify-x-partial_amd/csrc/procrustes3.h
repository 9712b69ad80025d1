// procrustes3.h -- the 3x3 solve of the orthogonal Procrustes problem (ProcrustesAlignment, smplifyx/utils.py:571-581), for the
// host and the device: no HIP runtime call, no global state, float64 throughout.
//
//   K = X1 X2^T = U S V^T,   R = V Z U^T,   Z = diag(1, 1, sign det(U V^T))        (utils.py:575-581)
//
// R is the rotation (det R = +1) that maximises tr(R K).  It needs the two leading singular pairs only: with K v_i = s_i u_i,
//   R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T
// is V Z U^T for either sign of det K (the third left vector of an SVD is +-(u1 x u2), and Z flips exactly the minus case), and
// stays the unique answer for a rank-2 K (coplanar points), where s_3 = 0 and u_3 is not defined by K.
// The pairs come from a one-sided (Hestenes) Jacobi SVD of K: plane rotations V from the right until the columns of G = K V are
// mutually orthogonal; then s_i = |g_i| and u_i = g_i / s_i.  No K^T K is formed, so small singular values keep their relative
// accuracy.  Sweeps run until one applies no rotation, at most P3_MAX_SWEEPS (3x3 matrices converge in 4 .. 6).
// Rank 1 (collinear points): R is not unique, any rotation that takes v1 to u1 gives the same aligned points; one is returned.
// K = 0 or a K that holds a non-finite value: the identity (the caller's scale is then 0 / 0 or non-finite, as the reference's).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define P3_HD __host__ __device__ inline
#else
#define P3_HD inline
#endif

#define P3_MAX_SWEEPS 30

P3_HD void p3_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// a unit vector orthogonal to the unit vector a
P3_HD void p3_any_orthogonal(const double* a, double* o) {
    const double ax = fabs(a[0]), ay = fabs(a[1]), az = fabs(a[2]);
    double e[3] = {0.0, 0.0, 0.0};
    e[(ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2)] = 1.0;      // the axis a leans on least
    p3_cross(a, e, o);
    const double n = sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
    o[0] /= n; o[1] /= n; o[2] /= n;
}

// K, R: row-major 3x3.  sv (or NULL): the singular values of K, descending.
P3_HD void procrustes3_rotation(const double* K, double* R, double* sv) {
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (sv) sv[0] = sv[1] = sv[2] = 0.0;
    double big = 0.0;
    bool finite = true;
    for (int i = 0; i < 9; ++i) { const double a = fabs(K[i]); if (!(a <= 1.7976931348623157e308)) finite = false; if (a > big) big = a; }
    if (!finite || big == 0.0) return;
    // columns of G = (K / big) V and of V, stored column by column
    double G[3][3], V[3][3];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) { G[c][r] = K[r * 3 + c] / big; V[c][r] = (r == c) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < P3_MAX_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double al = G[p][0] * G[p][0] + G[p][1] * G[p][1] + G[p][2] * G[p][2];
                const double be = G[q][0] * G[q][0] + G[q][1] * G[q][1] + G[q][2] * G[q][2];
                const double ga = G[p][0] * G[q][0] + G[p][1] * G[q][1] + G[p][2] * G[q][2];
                if (ga == 0.0 || fabs(ga) <= 1.1102230246251565e-16 * sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 3; ++r) {
                    const double gp = G[p][r], gq = G[q][r], vp = V[p][r], vq = V[q][r];
                    G[p][r] = c * gp - s * gq; G[q][r] = s * gp + c * gq;
                    V[p][r] = c * vp - s * vq; V[q][r] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double n[3];
    for (int c = 0; c < 3; ++c) n[c] = sqrt(G[c][0] * G[c][0] + G[c][1] * G[c][1] + G[c][2] * G[c][2]);
    int i0 = 0, i1 = 1, i2 = 2, tmp;                      // descending order of the column norms
    if (n[i1] > n[i0]) { tmp = i0; i0 = i1; i1 = tmp; }
    if (n[i2] > n[i0]) { tmp = i0; i0 = i2; i2 = tmp; }
    if (n[i2] > n[i1]) { tmp = i1; i1 = i2; i2 = tmp; }
    if (sv) { sv[0] = n[i0] * big; sv[1] = n[i1] * big; sv[2] = n[i2] * big; }
    double u1[3], u2[3], u3[3], v3[3];
    const double* v1 = V[i0];
    const double* v2 = V[i1];
    for (int r = 0; r < 3; ++r) u1[r] = G[i0][r] / n[i0];
    if (n[i1] > 0.0) {
        // u2 = g2 / |g2|, made orthogonal to u1 once more (the columns are orthogonal to ~1e-16 |g1||g2| only)
        const double d = u1[0] * G[i1][0] + u1[1] * G[i1][1] + u1[2] * G[i1][2];
        for (int r = 0; r < 3; ++r) u2[r] = G[i1][r] - d * u1[r];
        const double m = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
        if (m > 0.0) { for (int r = 0; r < 3; ++r) u2[r] /= m; } else p3_any_orthogonal(u1, u2);
    } else {
        p3_any_orthogonal(u1, u2);
    }
    p3_cross(u1, u2, u3);
    p3_cross(v1, v2, v3);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = v1[r] * u1[c] + v2[r] * u2[c] + v3[r] * u3[c];
}
