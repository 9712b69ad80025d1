// lbfgs_scalar.h -- the scalar layer of the on-device optimisers (lbfgs_body.h, lbfgs_wide.h): the dual-typed arithmetic, the
// cubic step of the line search, the side view's flipped orientation, the per-frame scalar state, and every transition of the
// state machine that is decided on scalars alone (the strong-Wolfe bracket and zoom phases, the LBFGS.step prologue and
// end-of-iteration tests, run_fitting's bookkeeping) -- the two ticks call these and keep the vector work between them.
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

// ---- The transitions of the state machine that read and write scalars only, stated once for both ticks (lbfgs_body.h: a frame's
// vectors in LDS, one wavefront; lbfgs_wide.h: rows in memory behind a vector layer).  A tick computes the reductions a
// transition wants, calls it, and does the vector work the returned value names.  Specification: oracle/lbfgs_machine.py;
// tests/lbfgs_scalar_check.cpp runs the line-search transitions against it on seeded states.

// c ? a : b on values (a ternary on members of the state would select between their addresses and keep the state in memory)
__host__ __device__ __forceinline__ Sc sc_pick(int c, const Sc a, const Sc b) { Sc r; r.v = c ? a.v : b.v; r.t = c ? a.t : b.t; return r; }

// the strong-Wolfe conditions at step t (lbfgs_ls.py:58, :73 and :134, :147)
__host__ __device__ __forceinline__ bool ls_armijo_fail(const OptScal& s, Sc f_new, Sc t) { return sc_gt(f_new, sc_add(s.ls_f0, sc_mul(sc_mul(P(1e-4), t), s.ls_gtd0))); }
__host__ __device__ __forceinline__ bool ls_curv_ok(const OptScal& s, Sc gtd_new) { return sc_le(sc_abs(gtd_new), sc_mul(P(-0.9), s.ls_gtd0)); }
__host__ __device__ __forceinline__ void ls_order_ends(OptScal& s) { const int swap = sc_le(s.bf0, s.bf1) ? 0 : 1; s.low = swap; s.high = 1 - swap; }
__host__ __device__ __forceinline__ void ls_set_bracket(OptScal& s, Sc b0, Sc b1, Sc f0, Sc f1, Sc gd0, Sc gd1, int done) {
    s.br0 = b0; s.br1 = b1; s.bf0 = f0; s.bf1 = f1; s.bgtd0 = gd0; s.bgtd1 = gd1;
    s.ls_done = done; s.insuf = 0;
    ls_order_ends(s);
}
__host__ __device__ __forceinline__ void ls_set_end(OptScal& s, int end, Sc b, Sc f, Sc gd) {
    if (end) { s.br1 = b; s.bf1 = f; s.bgtd1 = gd; } else { s.br0 = b; s.bf0 = f; s.bgtd0 = gd; }
}

// Bracket phase, one evaluation (f_in, gtd_new = g_in . d) at s.t (lbfgs_ls.py:54-100).  LS_EXTEND: the search goes on at the new
// s.t and the incoming gradient becomes the previous one.  Otherwise a bracket is set up -- scalars, order of the ends, ls_done,
// insuf -- whose gradient slot 1 is the incoming gradient and whose slot 0 is the one named; the zoom trial comes next.
enum { LS_EXTEND = 0, LS_G0_LSG0, LS_G0_GPREV, LS_G0_GIN };
__host__ __device__ __forceinline__ int ls_bracket_eval(OptScal& s, Sc f_in, Sc gtd_new, int max_ls) {
    s.ls_evals += 1;
    const Sc t = s.t;
    // loop budget exhausted: no tests on the last point, bracket = [0, t]
    if (s.ls_iter == max_ls) { ls_set_bracket(s, P(0.0), t, s.ls_f0, f_in, s.ls_gtd0, gtd_new, 0); return LS_G0_LSG0; }
    if (ls_armijo_fail(s, f_in, t) || (s.ls_iter > 1 && sc_ge(f_in, s.f_prev))) {
        ls_set_bracket(s, s.t_prev, t, s.f_prev, f_in, s.gtd_prev, gtd_new, 0); return LS_G0_GPREV; }
    // single-point bracket: the point itself is accepted
    if (ls_curv_ok(s, gtd_new)) { ls_set_bracket(s, t, t, f_in, f_in, gtd_new, gtd_new, 1); s.low = 0; s.high = 1; return LS_G0_GIN; }
    if (sc_ge(gtd_new, P(0.0))) { ls_set_bracket(s, s.t_prev, t, s.f_prev, f_in, s.gtd_prev, gtd_new, 0); return LS_G0_GPREV; }
    const Sc lo = sc_add(t, sc_mul(P(0.01), sc_sub(t, s.t_prev)));
    const Sc hi = sc_mul(t, P(10.0));
    const Sc t_next = cubic_interpolate(s.t_prev, s.f_prev, s.gtd_prev, t, f_in, gtd_new, true, lo, hi);
    s.t_prev = t; s.f_prev = f_in; s.gtd_prev = gtd_new;
    s.t = t_next; s.ls_iter += 1;
    return LS_EXTEND;
}

// Zoom phase, one evaluation at s.t (lbfgs_ls.py:132-161): the bracket's scalars and the order of its ends.  For the gradients:
// `end` receives the incoming one, after the other end has taken a copy of end's old gradient where copy_first is set.
// collapsed: the bracket is narrower than tol_change, the lower end is accepted; otherwise the zoom trial comes next.
struct ZoomMove { int end, copy_first, collapsed; };
__host__ __device__ __forceinline__ ZoomMove ls_zoom_eval(OptScal& s, Sc f_in, Sc gtd_new, double tol_change) {
    s.ls_evals += 1; s.ls_iter += 1;
    const Sc t = s.t;
    const int lo = s.low, hi = s.high;
    ZoomMove m; m.copy_first = 0;
    if (ls_armijo_fail(s, f_in, t) || sc_ge(f_in, sc_pick(lo, s.bf1, s.bf0))) {
        ls_set_end(s, hi, t, f_in, gtd_new); m.end = hi;
        ls_order_ends(s);
    } else {
        if (ls_curv_ok(s, gtd_new)) s.ls_done = 1;
        else if (sc_ge(sc_mul(gtd_new, sc_sub(sc_pick(hi, s.br1, s.br0), sc_pick(lo, s.br1, s.br0))), P(0.0))) {
            ls_set_end(s, hi, sc_pick(lo, s.br1, s.br0), sc_pick(lo, s.bf1, s.bf0), sc_pick(lo, s.bgtd1, s.bgtd0));
            m.copy_first = 1;
        }
        ls_set_end(s, lo, t, f_in, gtd_new); m.end = lo;
    }
    m.collapsed = sc_lt(sc_mul(sc_abs(sc_sub(s.br1, s.br0)), s.d_norm), P(tol_change)) ? 1 : 0;
    return m;
}

// The next zoom trial (lbfgs_ls.py:108-131).  false: the search is over (done, or out of iterations) and the lower end is
// accepted; true: s.t is the point to evaluate.
__host__ __device__ __forceinline__ bool ls_zoom_trial(OptScal& s, int max_iter) {
    if (s.ls_done || !(s.ls_iter < max_iter)) return false;
    Sc t = cubic_interpolate(s.br0, s.bf0, s.bgtd0, s.br1, s.bf1, s.bgtd1, false, P(0), P(0));
    const Sc bmax = sc_pick(sc_gt(s.br1, s.br0), s.br1, s.br0);      // Python max(list), min(list)
    const Sc bmin = sc_pick(sc_lt(s.br1, s.br0), s.br1, s.br0);
    const Sc eps = sc_mul(P(0.1), sc_sub(bmax, bmin));
    if (sc_lt(sc_pmin(sc_sub(bmax, t), sc_sub(t, bmin)), eps)) {
        if (s.insuf || sc_ge(t, bmax) || sc_le(t, bmin)) {
            if (sc_lt(sc_abs(sc_sub(t, bmax)), sc_abs(sc_sub(t, bmin)))) t = sc_sub(bmax, eps);
            else t = sc_add(bmin, eps);
            s.insuf = 0;
        } else s.insuf = 1;
    } else s.insuf = 0;
    s.t = t; s.phase = PH_ZOOM;
    return true;
}

// LBFGS.step prologue (lbfgs_ls.py:279-290); s.loss holds f at x, g_inf = |g|inf there.  Returns the next action.
__host__ __device__ __forceinline__ int step_entry(OptScal& s, float g_inf, double tol_grad) {
    s.cache_valid = 1; s.func_evals += 1;
    s.orig_loss = s.loss; s.cur_evals = 1; s.n_iter = 0;
    return sc_le(T(g_inf), P(tol_grad)) ? A_END_STEP : A_ITER_HEAD;
}
// One more iteration of LBFGS.step (lbfgs_ls.py:304-306)?  true: counted; n_iter_total == 1 marks the optimiser's first.
__host__ __device__ __forceinline__ bool step_iter_begin(OptScal& s, int max_iter) {
    if (!(s.n_iter < max_iter)) return false;
    s.n_iter += 1; s.n_iter_total += 1;
    return true;
}
// The first step length of an iteration (lbfgs_ls.py:375-381); g_asum = |g|_1, read in the optimiser's first iteration only.
__host__ __device__ __forceinline__ void step_first_length(OptScal& s, float g_asum, float lr) {
    s.prev_loss = s.loss;
    s.t = s.n_iter_total == 1 ? sc_mul(sc_pmin(P(1.0), sc_div(P(1.0), T(g_asum))), P((double)lr)) : P((double)lr);
}
// Directional derivative gtd = g . d: is d a descent direction worth a line search (lbfgs_ls.py:384-386)?
__host__ __device__ __forceinline__ bool step_descends(Sc gtd, double tol_change) { return !sc_gt(gtd, P(-tol_change)); }
// strong-Wolfe set-up (lbfgs_ls.py:39-52); d_inf = |d|inf
__host__ __device__ __forceinline__ void ls_setup(OptScal& s, Sc gtd, float d_inf) {
    s.ls_f0 = s.loss; s.ls_gtd0 = gtd; s.d_norm = T(d_inf);
    s.ls_evals = 0; s.ls_iter = 0;
    s.t_prev = P(0.0); s.f_prev = s.loss; s.gtd_prev = gtd; s.phase = PH_BRACKET;
}

// The line search is over: its lower end is the new point (lbfgs_ls.py:163-167, :398-404).  s.low still names the gradient;
// returns the accepted step length.  (The one place that selects between members, not values: the end is read once and
// nothing else of the bracket with it, and on values the fused tick kernels spill 4 to 20 bytes more per lane.)
__host__ __device__ __forceinline__ Sc ls_accept(OptScal& s) {
    const int lo = s.low;
    const Sc t = lo ? s.br1 : s.br0;
    s.loss = lo ? s.bf1 : s.bf0; s.t = t;
    s.cache_valid = 1;
    s.cur_evals += s.ls_evals; s.func_evals += s.ls_evals;
    return t;
}
// The ordered end-of-iteration tests (lbfgs_ls.py:409-434); g_inf = |g|inf at the new point, step_inf = |t d|inf.
__host__ __device__ __forceinline__ int step_iter_end(const OptScal& s, float g_inf, float step_inf, int max_iter, int max_eval,
                                                      double tol_grad, double tol_change) {
    const bool opt_cond = sc_le(T(g_inf), P(tol_grad));
    if (s.n_iter == max_iter) return A_END_STEP;
    if (s.cur_evals >= max_eval) return A_END_STEP;
    if (opt_cond) return A_END_STEP;
    if (sc_le(T(step_inf), P(tol_change))) return A_END_STEP;
    if (sc_lt(sc_abs(sc_sub(s.loss, s.prev_loss)), P(tol_change))) return A_END_STEP;
    return A_ITER_HEAD;
}

// run_fitting's bookkeeping after one LBFGS.step that returned `loss` (fitting.py:175-217), in two halves around the gtol
// test, whose per-group reduction is the caller's.  First half: the non-finite stop and the ftol test.
__host__ __device__ __forceinline__ bool fit_stops_on_loss(const OptScal& s, double loss, double ftol) {
    if (isnan(loss) || isinf(loss)) return true;
    if (s.outer > 0 && s.has_prev_outer && ftol > 0.0) {
        const double pv = s.prev_loss_outer;
        const double den = fmax(fmax(fabs(pv), fabs(loss)), 1.0);
        if ((pv - loss) / den <= ftol) return true;
    }
    return false;
}
// Second half: the outer counter and maxiters, then the re-entry.  A_FINISH_STAGE: run_fitting returns; A_ENTRY: the next
// LBFGS.step starts from the (loss, gradient) it already holds at the unchanged point (reuse); A_NONE: from an evaluation there.
__host__ __device__ __forceinline__ int fit_next_step(OptScal& s, bool stop, double loss, int maxiters, int reuse) {
    if (!stop) {
        s.prev_loss_outer = loss; s.has_prev_outer = 1; s.outer += 1;
        if (s.outer >= maxiters) stop = true;
    }
    if (stop) return A_FINISH_STAGE;
    s.phase = PH_ENTRY;
    if (reuse && s.cache_valid) { s.ref_evals += 1; return A_ENTRY; }
    return A_NONE;
}

#pragma clang fp contract(fast)
