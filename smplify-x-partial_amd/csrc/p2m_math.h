// p2m_math.h -- the arithmetic of the point-to-triangle term (csrc/p2m.hip, sfx_p2m_forward / sfx_p2m_backward; the contract is
// in include/sfx.h), for the host and the device: no HIP runtime call, no global state.  The kernels and
// tests/p2m_math_check.cpp both include it.
//
//   closest point       p2m_closest(p, a, b, c): the region test of Ericson, Real-Time Collision Detection 5.1.5, in float32
//                       without a fused multiply-add (the units that include this header are compiled with -ffp-contract=off) and
//                       with the correctly rounded division.  dot(x, y) = (x0 y0 + x1 y1) + x2 y2;  ab = b - a, ac = c - a,
//                       ap = p - a, bp = p - b, cp = p - c;  d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp;
//                       vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.  The first condition that holds gives (v, w):
//                         1  d1 <= 0 and d2 <= 0                          (0, 0)                      vertex a
//                         2  d3 >= 0 and d4 <= d3                         (1, 0)                      vertex b
//                         3  vc <= 0 and d1 >= 0 and d3 <= 0              (d1 / (d1 - d3), 0)         edge ab
//                         4  d6 >= 0 and d5 <= d6                         (0, 1)                      vertex c
//                         5  vb <= 0 and d2 >= 0 and d6 <= 0              (0, d2 / (d2 - d6))         edge ac
//                         6  va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w   edge bc
//                         7  otherwise                                    den = 1 / ((va + vb) + vc), v = vb den, w = vc den
//                       u = (1 - v) - w;  q = (a + v ab) + w ac;  d = p - q;  s = dot(d, d).
//                       Every region has at most one division, so the branch-free form below selects a numerator and a
//                       denominator and divides once: the same operations on the same values, the same bits.  A comparison
//                       with a NaN is false, so a degenerate face falls through to 7 and gives a NaN s, which is never nearer.
//   staged form         p2m_closest_staged takes a, b, c and the differences ab, ac formed beforehand (the same subtractions)
//   gradient            c = ch_coef(g, w, s, r2) of chamfer_math.h; the point's row is c (p - q), corner k of the face receives
//                       -(c bary_k)(p - q), the difference in float64 from the float32 p and q.  The barycentrics minimise, so
//                       they carry no derivative (envelope theorem).
//   scatter             entry e = 3 i + k is corner k of point i; the inverted index over the vertices, the segment rule and the
//                       float64 order are those of chamfer_math.h (ch_invert, ch_rank, ch_seg_len)
#pragma once
#include "chamfer_math.h"

struct P2mHit {
    float s;            // squared distance
    float u, v, w;      // barycentrics of the closest point: q = u a + v b + w c
    float q[3];         // the closest point as the contract forms it: (a + v ab) + w ac
};

CH_HD float p2m_dot(const float* x, const float* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

CH_HD P2mHit p2m_closest_staged(const float* p, const float* a, const float* b, const float* c, const float* ab, const float* ac) {
    const float ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const float bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const float cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const float d1 = p2m_dot(ab, ap), d2 = p2m_dot(ac, ap), d3 = p2m_dot(ab, bp), d4 = p2m_dot(ac, bp);
    const float d5 = p2m_dot(ab, cp), d6 = p2m_dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    // the conditions, each evaluated whole (no short circuit: lanes of a wave sit in different regions, a branch would cost
    // every lane every path)
    const bool r1 = (d1 <= 0.f) & (d2 <= 0.f);
    const bool r2 = (d3 >= 0.f) & (d4 <= d3);
    const bool r3 = (vc <= 0.f) & (d1 >= 0.f) & (d3 <= 0.f);
    const bool r4 = (d6 >= 0.f) & (d5 <= d6);
    const bool r5 = (vb <= 0.f) & (d2 >= 0.f) & (d6 <= 0.f);
    const bool r6 = (va <= 0.f) & (e43 >= 0.f) & (e56 >= 0.f);
    // the one division of the region that decides (the first whose condition holds); 1 / 1 where it has none
    const bool k3 = r3 & !(r1 | r2), k5 = r5 & !(r1 | r2 | r3 | r4), k6 = r6 & !(r1 | r2 | r3 | r4 | r5);
    const bool k7 = !(r1 | r2 | r3 | r4 | r5 | r6);
    // (every operand is formed first and every choice is one select between two values at hand: written as nested
    // conditionals the compiler branches around single subtractions)
    const float den3 = d1 - d3, den5 = d2 - d6, den6 = e43 + e56, den7 = (va + vb) + vc;
    float num = 1.f, den = 1.f;
    den = k7 ? den7 : den;
    num = k6 ? e43 : num; den = k6 ? den6 : den;
    num = k5 ? d2 : num;  den = k5 ? den5 : den;
    num = k3 ? d1 : num;  den = k3 ? den3 : den;
    const float t = num / den;
    const float v6 = 1.f - t, v7 = vb * t, w7 = vc * t;
    float v = v7, w = w7;                       // the regions from the last to the first: the first that holds has the last word
    v = r6 ? v6 : v;   w = r6 ? t : w;
    v = r5 ? 0.f : v;  w = r5 ? t : w;
    v = r4 ? 0.f : v;  w = r4 ? 1.f : w;
    v = r3 ? t : v;    w = r3 ? 0.f : w;
    v = r2 ? 1.f : v;  w = r2 ? 0.f : w;
    v = r1 ? 0.f : v;  w = r1 ? 0.f : w;
    P2mHit h;
    h.v = v; h.w = w; h.u = (1.f - v) - w;
    h.q[0] = (a[0] + v * ab[0]) + w * ac[0]; h.q[1] = (a[1] + v * ab[1]) + w * ac[1]; h.q[2] = (a[2] + v * ab[2]) + w * ac[2];
    const float d[3] = {p[0] - h.q[0], p[1] - h.q[1], p[2] - h.q[2]};
    h.s = p2m_dot(d, d);
    return h;
}

CH_HD P2mHit p2m_closest(const float* p, const float* a, const float* b, const float* c) {
    const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const float ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    return p2m_closest_staged(p, a, b, c, ab, ac);
}

// corner k of point i in the scatter's entry numbering, and back
CH_HD int p2m_entry(int i, int k) { return 3 * i + k; }

// the float64 factor of a point's gradient and what entry k adds to its vertex row: -(c bary_k)(p - q)
CH_HD void p2m_point_term(const float* p, const P2mHit& h, double c, double (&out)[3]) {
    out[0] = c * ((double)p[0] - (double)h.q[0]); out[1] = c * ((double)p[1] - (double)h.q[1]); out[2] = c * ((double)p[2] - (double)h.q[2]);
}

CH_HD void p2m_corner_term(const float* p, const P2mHit& h, int k, double c, double (&acc)[3]) {
    const double cb = c * (double)(k == 0 ? h.u : k == 1 ? h.v : h.w);
    acc[0] += -(cb * ((double)p[0] - (double)h.q[0])); acc[1] += -(cb * ((double)p[1] - (double)h.q[1])); acc[2] += -(cb * ((double)p[2] - (double)h.q[2]));
}
