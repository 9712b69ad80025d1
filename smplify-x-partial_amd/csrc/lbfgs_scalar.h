// lbfgs_scalar.h -- the scalar layer of the on-device optimiser (lbfgs_body.h): the dual-typed arithmetic, the cubic step
// of the line search, the side view's flipped orientation and the per-frame scalar state.
//
// The reference mixes Python floats (double) and 0-d float32 tensors; PyTorch computes in
// float32 whenever a tensor takes part.  `Sc` carries that distinction so that every
// branch is decided on identically rounded numbers.  The specification is oracle/lbfgs_machine.py (same rounding rule).
//
// Pure scalar code, __host__ __device__ throughout: tests/lbfgs_scalar_check.cpp runs it on the CPU against the specification
// (tests/test_lbfgs_scalar_host.py).  Needs the HIP runtime header and libm only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
// every multiply-add in this file is written out: no implicit contraction (fused.hip is compiled without -ffp-contract=off)
#pragma clang fp contract(off)

enum { PH_ENTRY = 0, PH_BRACKET = 1, PH_ZOOM = 2 };
enum { A_NONE = 0, A_ENTRY, A_ITER_HEAD, A_ZOOM_NEXT, A_FINISH_LS, A_END_STEP, A_FINISH_STAGE };

struct Sc { double v; int t; };
__host__ __device__ __forceinline__ Sc P(double v) { Sc s; s.v = v; s.t = 0; return s; }
__host__ __device__ __forceinline__ Sc T(float v) { Sc s; s.v = (double)v; s.t = 1; return s; }
__host__ __device__ __forceinline__ Sc sc_add(Sc a, Sc b) { return (a.t | b.t) ? T((float)a.v + (float)b.v) : P(a.v + b.v); }
__host__ __device__ __forceinline__ Sc sc_sub(Sc a, Sc b) { return (a.t | b.t) ? T((float)a.v - (float)b.v) : P(a.v - b.v); }
__host__ __device__ __forceinline__ Sc sc_mul(Sc a, Sc b) { return (a.t | b.t) ? T((float)a.v * (float)b.v) : P(a.v * b.v); }
__host__ __device__ __forceinline__ Sc sc_div(Sc a, Sc b) { return (a.t | b.t) ? T((float)a.v / (float)b.v) : P(a.v / b.v); }
__host__ __device__ __forceinline__ bool sc_lt(Sc a, Sc b) { return (a.t | b.t) ? ((float)a.v < (float)b.v) : (a.v < b.v); }
__host__ __device__ __forceinline__ bool sc_le(Sc a, Sc b) { return (a.t | b.t) ? ((float)a.v <= (float)b.v) : (a.v <= b.v); }
__host__ __device__ __forceinline__ bool sc_gt(Sc a, Sc b) { return (a.t | b.t) ? ((float)a.v > (float)b.v) : (a.v > b.v); }
__host__ __device__ __forceinline__ bool sc_ge(Sc a, Sc b) { return (a.t | b.t) ? ((float)a.v >= (float)b.v) : (a.v >= b.v); }
__host__ __device__ __forceinline__ Sc sc_pmax(Sc a, Sc b) { return sc_gt(b, a) ? b : a; }   // Python max(a, b)
__host__ __device__ __forceinline__ Sc sc_pmin(Sc a, Sc b) { return sc_lt(b, a) ? b : a; }   // Python min(a, b)
__host__ __device__ __forceinline__ Sc sc_abs(Sc a) { a.v = fabs(a.v); return a; }
__host__ __device__ __forceinline__ Sc sc_neg(Sc a) { a.v = -a.v; return a; }
__host__ __device__ __forceinline__ Sc sc_sqrt(Sc a) { return a.t ? T(sqrtf((float)a.v)) : P(sqrt(a.v)); }

// lbfgs_ls.py:11-36
__host__ __device__ __forceinline__ Sc cubic_interpolate(Sc x1, Sc f1, Sc g1, Sc x2, Sc f2, Sc g2, bool has_bounds, Sc lo, Sc hi) {
    if (!has_bounds) {
        if (sc_le(x1, x2)) { lo = x1; hi = x2; } else { lo = x2; hi = x1; }
    }
    const Sc d1 = sc_sub(sc_add(g1, g2), sc_div(sc_mul(P(3.0), sc_sub(f1, f2)), sc_sub(x1, x2)));
    const Sc d2sq = sc_sub(sc_mul(d1, d1), sc_mul(g1, g2));
    if (sc_ge(d2sq, P(0.0))) {
        const Sc d2 = sc_sqrt(d2sq);
        Sc mp;
        if (sc_le(x1, x2))
            mp = sc_sub(x2, sc_mul(sc_sub(x2, x1), sc_div(sc_sub(sc_add(g2, d2), d1),
                                                          sc_add(sc_sub(g2, g1), sc_mul(P(2.0), d2)))));
        else
            mp = sc_sub(x1, sc_mul(sc_sub(x1, x2), sc_div(sc_sub(sc_add(g1, d2), d1),
                                                          sc_add(sc_sub(g1, g2), sc_mul(P(2.0), d2)))));
        return sc_pmin(sc_pmax(mp, lo), hi);
    }
    return sc_div(sc_add(lo, hi), P(2.0));
}

// cv2.Rodrigues semantics (fit_single_frame.py:528-535): rotvec -> R, R . R([0,pi,0]), -> rotvec
__host__ __device__ inline void flipped_orientation(const float* go, float* out) {
    const double r0 = go[0], r1 = go[1], r2 = go[2];
    const double a = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (a >= 1e-12) {
        const double k0 = r0 / a, k1 = r1 / a, k2 = r2 / a, s = sin(a), c = 1.0 - cos(a);
        const double K[9] = {0, -k2, k1, k2, 0, -k0, -k1, k0, 0};
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
            double kk = 0; for (int q = 0; q < 3; ++q) kk += K[i * 3 + q] * K[q * 3 + j];
            R[i * 3 + j] = (i == j ? 1.0 : 0.0) + s * K[i * 3 + j] + c * kk;
        }
    }
    // R . Ry(pi): Ry(pi) = diag(-1, 1, -1) up to rounding of sin(pi); use the exact Rodrigues value
    const double sp = sin(3.14159265358979323846), cp = 1.0 - cos(3.14159265358979323846);
    const double Y[9] = {1 - cp, 0, sp, 0, 1, 0, -sp, 0, 1 - cp};
    double M_[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        double v = 0; for (int q = 0; q < 3; ++q) v += R[i * 3 + q] * Y[q * 3 + j];
        M_[i * 3 + j] = v;
    }
    double cth = (M_[0] + M_[4] + M_[8] - 1.0) / 2.0;
    cth = cth < -1.0 ? -1.0 : (cth > 1.0 ? 1.0 : cth);
    const double ang = acos(cth);
    const double v0 = M_[7] - M_[5], v1 = M_[2] - M_[6], v2 = M_[3] - M_[1];
    const double sn = sqrt(v0 * v0 + v1 * v1 + v2 * v2) / 2.0;
    if (sn < 1e-10) {
        if (cth > 0) { out[0] = out[1] = out[2] = 0.f; return; }
        double d0 = sqrt(fmax((M_[0] + 1) / 2, 0.0)), d1 = sqrt(fmax((M_[4] + 1) / 2, 0.0)), d2 = sqrt(fmax((M_[8] + 1) / 2, 0.0));
        if (M_[1] < 0) d1 = -d1;
        if (M_[2] < 0) d2 = -d2;
        const double n = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        out[0] = (float)(d0 / n * ang); out[1] = (float)(d1 / n * ang); out[2] = (float)(d2 / n * ang);
        return;
    }
    out[0] = (float)(v0 / (2 * sn) * ang); out[1] = (float)(v1 / (2 * sn) * ang); out[2] = (float)(v2 / (2 * sn) * ang);
}

struct OptScal {
    int phase, outer, n_iter, n_iter_total, cur_evals, func_evals;
    int ls_evals, ls_iter, ls_done, insuf, low, high;
    int hist_n, hist_head, cache_valid, has_prev_outer;
    int evals, ref_evals, pad0, pad1;
    Sc t, t_prev, H_diag;
    Sc loss, prev_loss, orig_loss, f_prev, ls_f0;
    Sc gtd_prev, ls_gtd0, d_norm;
    Sc br0, br1, bf0, bf1, bgtd0, bgtd1;
    double prev_loss_outer;
};
// copied as dwords: tick_write_back (lbfgs_body.h) and the LDS-DMA fills of fused.hip
static_assert(sizeof(OptScal) == 360 && sizeof(OptScal) % 4 == 0, "OptScal is moved dword by dword");

__host__ __device__ __forceinline__ OptScal fresh_state() {
    OptScal s;
    s.phase = PH_ENTRY; s.outer = 0; s.n_iter = 0; s.n_iter_total = 0; s.cur_evals = 0; s.func_evals = 0;
    s.ls_evals = 0; s.ls_iter = 0; s.ls_done = 0; s.insuf = 0; s.low = 0; s.high = 1;
    s.hist_n = 0; s.hist_head = 0; s.cache_valid = 0; s.has_prev_outer = 0; s.evals = 0; s.ref_evals = 0;
    s.pad0 = 0; s.pad1 = 0;
    s.t = P(0.0); s.t_prev = P(0.0); s.H_diag = P(1.0);
    s.loss = P(0.0); s.prev_loss = P(0.0); s.orig_loss = P(0.0); s.f_prev = P(0.0); s.ls_f0 = P(0.0);
    s.gtd_prev = P(0.0); s.ls_gtd0 = P(0.0); s.d_norm = P(0.0);
    s.br0 = s.br1 = s.bf0 = s.bf1 = s.bgtd0 = s.bgtd1 = P(0.0);
    s.prev_loss_outer = 0.0;
    return s;
}

#pragma clang fp contract(fast)
