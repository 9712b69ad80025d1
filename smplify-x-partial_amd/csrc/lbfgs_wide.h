// lbfgs_wide.h -- the optimiser's state machine for ONE problem of N variables, written against an abstract vector layer.
//
// Restates, for one problem whose loss and gradient come from outside:
//   FittingMonitor.run_fitting          smplifyx/fitting.py:147-217            (mode 0)
//   LBFGS.step                          smplifyx/optimizers/lbfgs_ls.py:256-445 (mode 1)
//   _strong_Wolfe / _cubic_interpolate  smplifyx/optimizers/lbfgs_ls.py:11-167
// with the transitions and the rounding rule of oracle/lbfgs_machine.py and the mode / resume semantics of
// lbfgs_tick_wave0<..., FIT = false> (lbfgs_body.h): one call of wide_tick consumes one evaluation and leaves the next point to
// evaluate in the row W_XT.  Every transition decided on scalars alone is lbfgs_scalar.h's, shared with lbfgs_tick_wave0 (the
// line search's bracket and zoom phases, the LBFGS.step prologue and end-of-iteration tests, run_fitting's bookkeeping); this
// file is the phase / action skeleton, the vector work between those calls, and the history with its plain recursion.
//
// The vector layer V (a template parameter) owns how a row of N floats is stored and who works on it: opt_wide.hip gives one
// workgroup of 1024 threads over rows in device memory, tests/lbfgs_wide_check.cpp a serial loop on the CPU.  The machine asks
// it for
//   row(k) / hist_y(slot) / hist_s(slot)    the working rows (enum below) and the history ring, as pointers the layer understands
//   dots(n, a[], b[], out[])                n <= 2 dot products in one pass, each accumulated in float64 and rounded once
//   axpy(dst, x, a, y)                      dst = fmaf(a, y, x), element by element
//   copy / neg / sub / scale                element-wise
//   asum(a), amax(a), amax_scaled(a, f)     |a|_1 (float64 accumulation, rounded once), |a|_inf, |a * f|_inf
//   gmax(a, off, len)                       signed maximum of a[off .. off + len)
//   Reg, r_load_neg / r_dot / r_axpy / r_scale / r_store      the vector the two-loop recursion keeps out of memory
//   al(), ro()                              per-problem tables: SFX_HIST_MAX alphas of one recursion; 1 / y.s per ring slot (SFX_HIST_MAX + 1)
//   scal()                                  where the scalar state (OptScal) lives during a tick
//   leader()                                true where the scalar state is written back (one thread; the CPU)
//   sync()                                  orders the leader's writes to al() / ro() before everybody's reads
//   trace(type, a, b, c)                    one record of the optimiser trace
// The machine itself is scalar code: whoever runs it (one wavefront on the device, whose lanes all compute the same scalars;
// the CPU) sees every reduction's result, and the layer spreads the vector work over whatever else it has.
//
// __host__ __device__ throughout, as lbfgs_scalar.h: the machine runs on the CPU over a serial layer, where it is tested
// (tests/test_opt_wide_host.py) and can be debugged.  Compile with -ffp-contract=off.
#pragma once
#include "lbfgs_scalar.h"
// every multiply-add in this file is written out: no implicit contraction
#pragma clang fp contract(off)

#ifndef SFX_HIST_MAX
#define SFX_HIST_MAX 400
#endif
#define SFX_WIDE_NMAX 32768
#define SFX_WIDE_MAX_GROUPS 256

// the working rows of one problem
enum { W_X = 0, W_XT, W_XINIT, W_D, W_G, W_PREVG, W_GPREV, W_BG0, W_BG1, W_LSG0, W_GIN, W_NROWS };
// status of a problem: 0 running, 1 run_fitting returned, 1000 one LBFGS.step returned (resumable)
enum { WIDE_RUNNING = 0, WIDE_DONE = 1, WIDE_PAUSED = 1000 };

struct WideCfg {
    int N, maxiters, max_iter, max_eval, hist_cap, reuse, ngroups;
    float lr;
    double ftol, gtol, tol_grad, tol_change;
    const int* g_off;          // [ngroups] the tensors of the caller's parameter list (run_fitting's gtol test, fitting.py:191)
    const int* g_len;
};

// What one problem keeps between ticks besides its rows.  OptScal is the fit loop's own (its size is pinned); the wide state
// goes around it.
struct WideState {
    OptScal s;
    int status, evals;         // evals: evaluations consumed since the last fresh begin
    float result;              // mode 0: what run_fitting returns (NaN for None); mode 1: the loss at entry
    int pad;
};

// The history ring has hist_cap + 1 slots: the candidate pair of an iteration is formed in the free slot and stays there when
// it is accepted (y.s > 1e-10), so no pair is copied and the oldest one is still whole when the candidate is refused.
__host__ __device__ __forceinline__ int wide_ring_slots(int hist_cap) { return hist_cap + 1; }

// init = 1: a fresh optimiser (lbfgs_ls.py:293-300) at the point the caller left in row W_X; init = 2: resume after a
// mode-1 run -- state, history and counters kept.  Either way the first point to evaluate is the current one.
template <class V>
__host__ __device__ __forceinline__ void wide_begin(V& v, WideState& st, int init) {
    if (v.leader()) {
        if (init == 1) { st.s = fresh_state(); st.status = WIDE_RUNNING; st.evals = 0; st.result = 0.f; st.pad = 0; }
        else if (st.status >= 900) st.status -= WIDE_PAUSED;
    }
    v.copy(v.row(W_XT), v.row(W_X));
}

// One evaluation: f_in and the gradient in row W_GIN, taken at row W_XT.  Returns the problem's status after it.
template <class V>
__host__ __device__ __forceinline__ int wide_tick(V& v, const WideCfg& C, WideState& st, int step_mode, float f_src) {
    int status = st.status;
    if (status > 0) return status;
    OptScal& s = v.scal();     // the layer's working copy of the scalar state (fast memory; written back below)
    s = st.s;
    int evals_total = st.evals + 1;
    float result = st.result;
    const double tol_change = C.tol_change, tol_grad = C.tol_grad;
    const int max_iter = C.max_iter, max_eval = C.max_eval, max_ls = 25, cap = C.hist_cap, slots = wide_ring_slots(C.hist_cap);
    typename V::Row X = v.row(W_X), XT = v.row(W_XT), XINIT = v.row(W_XINIT), D = v.row(W_D), G = v.row(W_G), PREVG = v.row(W_PREVG),
                    GPREV = v.row(W_GPREV), BG0 = v.row(W_BG0), BG1 = v.row(W_BG1), LSG0 = v.row(W_LSG0), GIN = v.row(W_GIN);

    const Sc f_in = P((double)f_src);
    int glast_cached = 0;
    s.evals += 1; s.ref_evals += 1;

#define W_TRIAL() v.axpy(XT, XINIT, (float)s.t.v, D)

    int act = A_NONE;
    // ---------------------------------------------------------------- consume the evaluation
    if (s.phase == PH_ENTRY) {
        v.copy(G, GIN);
        s.loss = f_in;
        act = A_ENTRY;
    } else if (s.phase == PH_BRACKET) {
        const int g0 = ls_bracket_eval(s, f_in, T(v.dot(GIN, D)), max_ls);
        if (g0 == LS_EXTEND) {
            v.copy(GPREV, GIN);
            W_TRIAL();
            act = A_NONE;
        } else {       // a bracket: gradient slot 0 = the row named, slot 1 = the incoming gradient
            v.copy(BG0, g0 == LS_G0_GIN ? GIN : g0 == LS_G0_LSG0 ? LSG0 : GPREV); v.copy(BG1, GIN);
            act = A_ZOOM_NEXT;
        }
    } else {   // PH_ZOOM
        const ZoomMove m = ls_zoom_eval(s, f_in, T(v.dot(GIN, D)), tol_change);
        if (m.copy_first) v.copy(m.end ? BG0 : BG1, m.end ? BG1 : BG0);
        v.copy(m.end ? BG1 : BG0, GIN);
        act = m.collapsed ? A_FINISH_LS : A_ZOOM_NEXT;
    }

    // ---------------------------------------------------------------- run until an evaluation is needed
    int guard = 0;
    while (act != A_NONE && guard++ < 4096) {
        switch (act) {
        case A_ENTRY: {          // LBFGS.step prologue (lbfgs_ls.py:279-290); (loss, G) hold f, g at x
            act = step_entry(s, v.amax(G), tol_grad);
            break;
        }
        case A_ITER_HEAD: {      // direction + first trial point (lbfgs_ls.py:304-397)
            if (!step_iter_begin(s, max_iter)) { act = A_END_STEP; break; }
            if (s.n_iter_total == 1) {
                v.neg(D, G);
                s.hist_n = 0; s.hist_head = 0; s.H_diag = P(1.0);
            } else {
                // the candidate pair, formed in the ring's free slot (D still holds the previous direction)
                const int fresh = (s.hist_head + s.hist_n) % slots;
                typename V::Row y = v.hist_y(fresh), sv = v.hist_s(fresh);
                v.sub(y, G, PREVG);
                v.scale(sv, D, (float)s.t.v);
                typename V::Row da[2] = {y, y}, db[2] = {sv, y};
                float r2[2];
                v.dots(2, da, db, r2);
                const float ys = r2[0];
                if (ys > 1e-10f) {
                    if (s.hist_n == cap) s.hist_head = (s.hist_head + 1) % slots;      // the oldest pair leaves
                    else s.hist_n += 1;
                    if (v.leader()) v.ro()[fresh] = 1.0f / ys;
                    s.H_diag = T(ys / r2[1]);
                }
                // two-loop recursion (lbfgs_ls.py:352-370), plain and sequential: newest to oldest, then back
                const int n = s.hist_n, head = s.hist_head;
                const float hd = (float)s.H_diag.v;
                typename V::Reg q;
                v.r_load_neg(q, G);
                v.sync();                  // the leader's ro[fresh] before everybody reads it
                for (int i = n - 1; i >= 0; --i) {
                    const int slot = (head + i) % slots;
                    const float a = v.r_dot(q, v.hist_s(slot)) * v.ro()[slot];
                    if (v.leader()) v.al()[i] = a;
                    v.r_axpy(q, -a, v.hist_y(slot));
                }
                v.r_scale(q, hd);
                v.sync();                  // the leader's al[] likewise
                for (int i = 0; i < n; ++i) {
                    const int slot = (head + i) % slots;
                    const float be = v.r_dot(q, v.hist_y(slot)) * v.ro()[slot];
                    v.r_axpy(q, v.al()[i] - be, v.hist_s(slot));
                }
                v.r_store(D, q);
            }
            v.copy(PREVG, G);
            step_first_length(s, s.n_iter_total == 1 ? v.asum(G) : 0.f, C.lr);
            const Sc gtd = T(v.dot(G, D));
            if (!step_descends(gtd, tol_change)) { act = A_END_STEP; break; }
            // strong-Wolfe set-up (lbfgs_ls.py:39-52)
            v.copy(XINIT, X);
            v.copy(LSG0, G);
            v.copy(GPREV, G);
            ls_setup(s, gtd, v.amax(D));
            W_TRIAL();
            act = A_NONE;
            break;
        }
        case A_ZOOM_NEXT: {      // next zoom trial (lbfgs_ls.py:108-131)
            if (!ls_zoom_trial(s, max_iter)) { act = A_FINISH_LS; break; }
            W_TRIAL();
            act = A_NONE;
            break;
        }
        case A_FINISH_LS: {      // accept the lowest bracket end (lbfgs_ls.py:163-167,398-434)
            v.copy(G, s.low ? BG1 : BG0);
            const Sc t = ls_accept(s);
            v.axpy(X, XINIT, (float)t.v, D);
            v.trace(0, t.v, s.loss.v, s.ls_evals);
            const float g_inf = v.amax(G);
            act = step_iter_end(s, g_inf, v.amax_scaled(D, (float)t.v), max_iter, max_eval, tol_grad, tol_change);
            break;
        }
        case A_END_STEP: {       // run_fitting bookkeeping (fitting.py:175-217)
            const double loss = s.orig_loss.v;
            v.trace(1, loss, s.func_evals, s.n_iter_total);
            if (step_mode) {         // one LBFGS.step per call: hand control back, keep the state
                result = (float)loss;
                status = WIDE_PAUSED;
                s.phase = PH_ENTRY;
                v.copy(XT, X);
                act = A_NONE;
                break;
            }
            bool stop = fit_stops_on_loss(s, loss, C.ftol);
            if (!stop) {         // the gtol test (fitting.py:191) on the last gradient the closure returned
                typename V::Row gl = glast_cached ? G : GIN;
                bool all_small = true;     // (one group that is not small decides: the others need no look)
                for (int gi = 0; gi < C.ngroups && all_small; ++gi) {
                    const float m = v.gmax(gl, C.g_off[gi], C.g_len[gi]);
                    if (!((double)fabsf(m) < C.gtol)) all_small = false;
                }
                if (all_small) stop = true;
            }
            act = fit_next_step(s, stop, loss, C.maxiters, C.reuse);
            if (act == A_ENTRY) glast_cached = 1;          // (loss, G) already hold f, g at the unchanged x
            else if (act == A_NONE) v.copy(XT, X);
            break;
        }
        case A_FINISH_STAGE: {
            result = s.has_prev_outer ? (float)s.prev_loss_outer : (float)NAN;      // (None)
            v.trace(2, result, s.evals, 0);
            status = WIDE_DONE;
            s = fresh_state();
            v.copy(XT, X);
            act = A_NONE;
            break;
        }
        default: act = A_NONE; break;
        }
    }
    if (v.leader()) { st.s = s; st.status = status; st.evals = evals_total; st.result = result; }
    return status;
#undef W_TRIAL
}

#pragma clang fp contract(fast)
