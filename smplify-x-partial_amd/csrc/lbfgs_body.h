// lbfgs_body.h -- batched on-device optimiser: one wavefront per frame advances that frame's
// run_fitting / L-BFGS / strong-Wolfe state machine by ONE closure evaluation per launch.
//
// Replaces (per frame, with all Python-side control flow moved on device):
//   FittingMonitor.run_fitting        smplifyx/fitting.py:147-217
//   LBFGS.step                        smplifyx/optimizers/lbfgs_ls.py:256-445
//   _strong_Wolfe / _cubic_interpolate smplifyx/optimizers/lbfgs_ls.py:11-167
//   per-stage optimiser re-creation   smplifyx/fit_single_frame.py:553-564
// The specification is oracle/lbfgs_machine.py (same transitions, same rounding rule).
//
// This file: the tick (lbfgs_tick_wave0), its entry for a workgroup (lbfgs_tick_body) and the workgroup-wide write-back
// (tick_write_back).  The tick is the phase / action skeleton, the vector work (Lane3 in registers, rows in LDS) and the fit's
// stage sequencing; every transition decided on scalars alone -- the line search's bracket and zoom phases, the LBFGS.step
// prologue and end-of-iteration tests, run_fitting's bookkeeping -- is lbfgs_scalar.h, with the dual-typed scalars, the cubic
// step and the scalar state; the history and the blocked two-loop recursion are lbfgs_two_loop.h.  Compile with -ffp-contract=off (see there).
#pragma once
#include "lbfgs_scalar.h"
#include "lbfgs_two_loop.h"
// every multiply-add in this file is written out: no implicit contraction
#pragma clang fp contract(off)

// One tick of frame b's optimiser, executed by ONE wavefront (lanes 0..63).  f_in / g_in: the
// closure result (global D.f/D.g, or LDS copies in fused kernels).  s_al[SFX_HIST_MAX + 2 * LB_BS], s_state and
// s_work[2048] (the tick's working copies; may alias any LDS that is dead during the tick)
// are LDS scratch owned by the caller.
// FIT: the fit's stage sequencing -- the side-view test at the start of a run, the camera stage's orientation kept for it and
// the second pass from the flipped orientation (A_FINISH_STAGE).  false: one run of one stage over a BatchDev that has none of
// M, D.gt, D.try_both, D.orient_pass, D.gocam, D.X0, D.stage_loss2 (opt_ext.hip); none of them is read then.
// PF: the caller has the working set (vectors, X, Xt in s_work, the scalar state in s_state) and both variable lists (vls
// points to LDS copies) in place already -- k_tick_dense requests them with its entry's LDS-DMA batch, a whole loss /
// adjoint pass before the tick wants them -- and takes the frame's stage after the tick from *stage_out.  stage_in (PF): the
// frame's stage where the caller knows it -- a workgroup that ran this frame's previous tick has it from that tick's *stage_out,
// and its working set is what that tick left in s_work / s_state (everything a tick changes there it also writes back) --; -2: D.stage.
template <int SETS, bool PF = false, bool WB = true, bool FIT = true>
__device__ __forceinline__ void lbfgs_tick_wave0(const DevModel& M, const BatchDev& D, const VarList* __restrict__ vls,
                                                 int first_stage, int last_stage, int init, int step_mode,
                                                 const int b, const int lane, float* s_al, OptScal& s_state, float* s_work,
                                                 const float* f_src, const float* g_src, int* stage_out = nullptr,
                                                 const int stage_in = -2) {
    const BatchCfgDev& C = D.cfg;
    OptState* gst = reinterpret_cast<OptState*>(D.opt) + b;
    int stage = (PF && stage_in != -2) ? stage_in : D.stage[b];
    float* Xg = D.X + (size_t)b * SFX_NPAR_MAX;          // global homes of the parameters, the trial point and the vectors;
    float* Xtg = D.Xt + (size_t)b * SFX_NPAR_MAX;        // a tick works on LDS copies (below)
    float* vecg = D.vec + (size_t)b * NVEC * SFX_NVAR_MAX;
#ifdef SFX_RING_CONST                                   // (measurement: the ring's size as the compile-time constant it was until round 5)
    const int R = SFX_HIST, hrows = R + 8;
#else
    const int R = C.hist_ring, hrows = R + 8;          // slots of the history ring (SFX_HIST unless history_size is larger)
#endif
    float* hY = D.hist + (size_t)b * 2 * hrows * SFX_NVAR_MAX;
    float* hS = hY + (size_t)hrows * SFX_NVAR_MAX;
#define VEC(k) (vec + (k) * SFX_NVAR_MAX)

    // ---------------------------------------------------------------- (re)initialisation
    if (init == 1) {
        const OptScal s = fresh_state();
        stage = first_stage;
        if (lane == 0) {
            D.stage[b] = stage;
            gst->s = s;            // ro[] needs no initialisation (guarded by hist_n)
            if constexpr (FIT) {
                D.orient_pass[b] = 0;
                int both = 0;
                if (C.side_thsh > 0.f) {     // torch.dist of the 2-D shoulders (fit_single_frame.py:461-463)
                    const float* g2 = D.gt + (size_t)b * M.K * 2;
                    const float dx = g2[2 * C.lsh] - g2[2 * C.rsh], dy = g2[2 * C.lsh + 1] - g2[2 * C.rsh + 1];
                    both = sqrtf(dx * dx + dy * dy) < C.side_thsh;
                }
                D.try_both[b] = both;
            }
        }
        for (int i = lane; i < hrows * LB_BROW; i += 64) { gst->syb[i] = 0.f; gst->syt[i] = 0.f; }     // (columns 0..8 stay zero)
        for (int q = lane; q < 1 + SFX_MAX_STAGES; q += 64) {
            if (q >= first_stage + 1 && q <= last_stage + 1) {
                D.stage_evals[(size_t)b * (1 + SFX_MAX_STAGES) + q] = 0;
                D.stage_ref_evals[(size_t)b * (1 + SFX_MAX_STAGES) + q] = 0;
            }
        }
        for (int i = lane; i < SFX_NPAR_MAX; i += 64) Xtg[i] = Xg[i];
        return;
    }
    if (init == 2) {           // resume after a pause (optimizer.step granularity): keep the state
        if (stage >= 900 && lane == 0) D.stage[b] = stage - 1000;   // camera stage -1 pauses as 999
        for (int i = lane; i < SFX_NPAR_MAX; i += 64) Xtg[i] = Xg[i];
        return;
    }
    if (stage > last_stage) { if (PF && lane == 0) *stage_out = stage; return; }
    // debug: frame 0 accumulates shader-clock deltas between TMARKs into dbg[32+i], tick count in dbg[63]
    long long tm_prev = 0;
#define TMARK(i) do { if (D.dbg && b == 0 && lane == 0) { const long long c_ = clock64();                 \
        if (i) D.dbg[32 + (i)] += c_ - tm_prev; else D.dbg[63] += 1; tm_prev = c_; } } while (0)
    TMARK(0);

    // Working set in LDS for the duration of the tick, fetched in ONE round trip and written back at the end: the scalar
    // state (every lane reads -- broadcast -- and writes -- identical values -- the same words, so the single wavefront
    // stays uniform), the NVEC optimiser vectors, the parameters X and the trial point Xt.  The state machine below
    // stores a vector and reads it back a few lines later many times per tick: through global memory each of those is
    // an L2 round trip plus a fence (~10 of them in the common path), in LDS ~100 cycles.
    static_assert(NVEC * SFX_NVAR_MAX + 2 * SFX_NPAR_MAX <= 2048 && SFX_NPAR_MAX == 4 * 64, "s_work: 2048 floats");
    float* vec = s_work;
    float* X = s_work + NVEC * SFX_NVAR_MAX;
    float* Xt = X + SFX_NPAR_MAX;
    const VarList& vl = vls[stage < 0 ? 0 : 1];
    int N = vl.n;
    int idx3[NE3];           // this lane's parameter slots (vl.idx: 6 bytes per lane, once per tick)
    if constexpr (PF) {
#pragma unroll
        for (int e = 0; e < NE3; ++e) idx3[e] = vl.idx[3 * lane + e];
    } else {
        Lane3 wv_[NVEC];
#pragma unroll
        for (int k = 0; k < NVEC; ++k) wv_[k] = ld3_raw(vecg, (unsigned)k * SFX_NVAR_MAX, lane);
        const float4 x4 = reinterpret_cast<const float4*>(Xg)[lane], xt4 = reinterpret_cast<const float4*>(Xtg)[lane];
#pragma unroll
        for (int e = 0; e < NE3; ++e) idx3[e] = vl.idx[3 * lane + e];
        if (lane == 0) s_state = gst->s;
#pragma unroll
        for (int k = 0; k < NVEC; ++k) st3_full(vec + k * SFX_NVAR_MAX, wv_[k], lane);
        reinterpret_cast<float4*>(X)[lane] = x4; reinterpret_cast<float4*>(Xt)[lane] = xt4;
    }
    LB_SYNC();
    OptScal& s = s_state;
    const double tol_change = C.tol_change, tol_grad = C.tol_grad;      // (LBFGS defaults 1e-9 / 1e-5: optim_factory.py:27-65 never changes them)
    const int max_iter = C.lbfgs_max_iter, max_eval = C.max_eval, max_ls = 25;

    // incoming evaluation
    const Sc f_in = P((double)*f_src);
    Lane3 g_in = ld3(g_src, lane, N);
    int glast_cached = 0;
    s.evals += 1; s.ref_evals += 1;

    auto gather_x = [X, lane, N, &idx3]() { Lane3 r;
        for (int e = 0; e < NE3; ++e) { const int i = 3 * lane + e; r.v[e] = (i < N) ? X[idx3[e]] : 0.f; } return r; };
    auto write_trial = [X, Xt, vec, lane, N, &idx3](Sc t) {
        const Lane3 xi = ld3(VEC(VEC_XINIT), lane, N), d = ld3(VEC(VEC_D), lane, N);
        const Lane3 xt = axpy3(xi, (float)t.v, d);
        for (int i = lane; i < SFX_NPAR_MAX; i += 64) Xt[i] = X[i];
        LB_SYNC();
        for (int e = 0; e < NE3; ++e) { const int i = 3 * lane + e; if (i < N) Xt[idx3[e]] = xt.v[e]; }
    };
    // optimiser trace (sfx_batch_trace): one record per finished line search / LBFGS.step / stage
#define TRACE(ty, a_, b_, c_) do { if (D.trace && D.trace_n && lane == 0) { const int n_ = D.trace_n[b];                         \
        if (n_ < D.trace_cap) D.trace[(size_t)b * D.trace_cap + n_] = make_float4((float)(ty), (float)(a_), (float)(b_), (float)(c_)); \
        D.trace_n[b] = n_ + 1; } } while (0)
    if (D.trace && D.trace_evals) {      // (debug) every evaluation: trial step, loss, |g|inf  (the reduction is wave-wide: outside TRACE)
        const float ginf_ = absmax3(g_in, lane, N);
        TRACE(3, s.t.v, f_in.v, ginf_);
    }
    int act = A_NONE;
    TMARK(1);
    // ---------------------------------------------------------------- consume the evaluation
    if (s.phase == PH_ENTRY) {
        st3(VEC(VEC_G), g_in, lane, N);
        s.loss = f_in;
        act = A_ENTRY;
    } else if (s.phase == PH_BRACKET) {
        const Lane3 d = ld3(VEC(VEC_D), lane, N);
        const int g0 = ls_bracket_eval(s, f_in, T(dot3(g_in, d)), max_ls);
        if (g0 == LS_EXTEND) {
            st3(VEC(VEC_GPREV), g_in, lane, N);
            write_trial(s.t);
            act = A_NONE;
        } else {       // a bracket: gradient slot 0 = the one named, slot 1 = the incoming gradient
            const Lane3 G0 = g0 == LS_G0_GIN ? g_in : ld3(VEC(g0 == LS_G0_LSG0 ? VEC_LSG0 : VEC_GPREV), lane, N);
            st3(VEC(VEC_BG0), G0, lane, N); st3(VEC(VEC_BG1), g_in, lane, N);
            act = A_ZOOM_NEXT;
        }
    } else {   // PH_ZOOM
        const Lane3 d = ld3(VEC(VEC_D), lane, N);
        const ZoomMove m = ls_zoom_eval(s, f_in, T(dot3(g_in, d)), tol_change);
        if (m.copy_first) {
            const Lane3 tmp = ld3(VEC(m.end ? VEC_BG1 : VEC_BG0), lane, N);
            st3(VEC(m.end ? VEC_BG0 : VEC_BG1), tmp, lane, N);
        }
        st3(VEC(m.end ? VEC_BG1 : VEC_BG0), g_in, lane, N);
        act = m.collapsed ? A_FINISH_LS : A_ZOOM_NEXT;
    }

    TMARK(2);
    // ---------------------------------------------------------------- run until an evaluation is needed
    int guard = 0;
    while (act != A_NONE && guard++ < 4096) {
        switch (act) {
        case A_ENTRY: {          // LBFGS.step prologue (lbfgs_ls.py:279-290); (loss, G) hold f, g at x
            const Lane3 g = ld3(VEC(VEC_G), lane, N);
            act = step_entry(s, absmax3(g, lane, N), tol_grad);
            break;
        }
        case A_ITER_HEAD: {      // direction + first trial point (lbfgs_ls.py:304-397)
            if (!step_iter_begin(s, max_iter)) { act = A_END_STEP; break; }
            const Lane3 g = ld3(VEC(VEC_G), lane, N);
            Lane3 d;
            if (s.n_iter_total == 1) {
                for (int e = 0; e < NE3; ++e) d.v[e] = -g.v[e];
                s.hist_n = 0; s.hist_head = 0; s.H_diag = P(1.0);
            } else {
                const Lane3 pg = ld3(VEC(VEC_PREVG), lane, N), dold = ld3(VEC(VEC_D), lane, N);
                Lane3 y, sv;
                const float tf = (float)s.t.v;
                for (int e = 0; e < NE3; ++e) { y.v[e] = g.v[e] - pg.v[e]; sv.v[e] = dold.v[e] * tf; }
                const float ys = dot3(y, sv);
                if (ys > 1e-10f) {
                    int hn = s.hist_n, hh = s.hist_head;
                    lb_push_pair(hY, hS, gst, hn, hh, y, sv, ys, lane, C.hist_cap, R);
                    s.hist_n = hn; s.hist_head = hh;
                    s.H_diag = T(ys / dot3(y, y));
                }
                LB_SYNC();
                TMARK(3);
                Lane3 r;
                {
                    const int n = __builtin_amdgcn_readfirstlane(s.hist_n);
                    const float hd = (float)s.H_diag.v;
                    Lane3 q;
                    for (int e = 0; e < NE3; ++e) q.v[e] = -g.v[e];
                    if (n == 0) {
                        for (int e = 0; e < NE3; ++e) r.v[e] = q.v[e] * hd;
                    } else {
                        r = lb_two_loop<SETS>(hS, hY, gst, s_al, n, s.hist_head, hd, q, lane, R);
                    }
                }
                TMARK(5);
                d = r;
            }
            st3(VEC(VEC_D), d, lane, N);
            st3(VEC(VEC_PREVG), g, lane, N);
            float asum = 0.f;
            if (s.n_iter_total == 1) {
                for (int e = 0; e < NE3; ++e) asum = asum + fabsf(g.v[e]);
                asum = wsum(asum);
            }
            step_first_length(s, asum, C.lr);
            const Sc gtd = T(dot3(g, d));
            if (!step_descends(gtd, tol_change)) { act = A_END_STEP; break; }
            // strong-Wolfe set-up (lbfgs_ls.py:39-52)
            const Lane3 xi = gather_x();
            st3(VEC(VEC_XINIT), xi, lane, N);
            st3(VEC(VEC_LSG0), g, lane, N);
            st3(VEC(VEC_GPREV), g, lane, N);
            ls_setup(s, gtd, absmax3(d, lane, N));
            LB_SYNC();
            write_trial(s.t);
            act = A_NONE;
            break;
        }
        case A_ZOOM_NEXT: {      // next zoom trial (lbfgs_ls.py:108-131)
            if (!ls_zoom_trial(s, max_iter)) { act = A_FINISH_LS; break; }
            write_trial(s.t);
            act = A_NONE;
            break;
        }
        case A_FINISH_LS: {      // accept the lowest bracket end (lbfgs_ls.py:163-167,398-434)
            const Sc t = ls_accept(s);
            const Lane3 g = ld3(VEC(s.low ? VEC_BG1 : VEC_BG0), lane, N);
            st3(VEC(VEC_G), g, lane, N);
            const Lane3 xi = ld3(VEC(VEC_XINIT), lane, N), d = ld3(VEC(VEC_D), lane, N);
            const Lane3 xn = axpy3(xi, (float)t.v, d);
            for (int e = 0; e < NE3; ++e) { const int i = 3 * lane + e; if (i < N) X[idx3[e]] = xn.v[e]; }
            const float g_inf = absmax3(g, lane, N);
            TRACE(0, t.v, s.loss.v, s.ls_evals);
            Lane3 stp;
            const float tf = (float)t.v;
            for (int e = 0; e < NE3; ++e) stp.v[e] = d.v[e] * tf;
            act = step_iter_end(s, g_inf, absmax3(stp, lane, N), max_iter, max_eval, tol_grad, tol_change);
            if (act == A_ITER_HEAD) LB_SYNC();
            break;
        }
        case A_END_STEP: {       // run_fitting bookkeeping (fitting.py:175-217)
            const double loss = s.orig_loss.v;
            TRACE(1, loss, s.func_evals, s.n_iter_total);
            if (step_mode) {         // one LBFGS.step per call: hand control back, keep the state
                if (lane == 0) {
                    D.stage_loss[(size_t)b * (1 + SFX_MAX_STAGES) + stage + 1] = (float)loss;
                    D.stage[b] = stage + 1000;
                }
                s.phase = PH_ENTRY;
                for (int i = lane; i < SFX_NPAR_MAX; i += 64) Xt[i] = X[i];
                act = A_NONE;
                break;
            }
            bool stop = fit_stops_on_loss(s, loss, C.ftol);
            if (!stop) {         // the gtol test (fitting.py:191) on the last gradient the closure returned
                const Lane3 gl = glast_cached ? ld3(VEC(VEC_G), lane, N) : g_in;
                bool all_small = true;
                for (int gi = 0; gi < vl.ngroups; ++gi) {
                    if (!vl.g_has[gi]) continue;
                    float m = -INFINITY;
                    for (int e = 0; e < NE3; ++e) {
                        const int i = 3 * lane + e;
                        if (i >= vl.g_off[gi] && i < vl.g_off[gi] + vl.g_len[gi]) m = fmaxf(m, gl.v[e]);
                    }
                    m = wmax(m);
                    if (!((double)fabsf(m) < C.gtol)) all_small = false;
                }
                if (all_small) stop = true;
            }
            act = fit_next_step(s, stop, loss, C.maxiters, C.reuse);
            if (act == A_ENTRY) glast_cached = 1;          // (loss, G) already hold f, g at the unchanged x
            else if (act == A_NONE) { for (int i = lane; i < SFX_NPAR_MAX; i += 64) Xt[i] = X[i]; }
            break;
        }
        case A_FINISH_STAGE: {
            const int slot = stage + 1;     // camera stage -> 0
            const size_t so = (size_t)b * (1 + SFX_MAX_STAGES);
            int pass = 0;          // (of the side view: 0 = the first orientation, 1 = the flipped one)
            if constexpr (FIT) pass = D.orient_pass[b];
            const float res = s.has_prev_outer ? (float)s.prev_loss_outer : __int_as_float(0x7fc00000);
            TRACE(2, res, s.evals, stage);
            if (lane == 0) {
                (pass ? D.stage_loss2 : D.stage_loss)[so + slot] = res;
                D.stage_evals[so + slot] += s.evals;
                D.stage_ref_evals[so + slot] += s.ref_evals;
            }
            // camera stage done: remember the orientation the flipped candidate is derived from
            if constexpr (FIT) { if (stage < 0 && lane < 3) D.gocam[(size_t)b * 4 + lane] = X[D.L.go + lane]; }
            stage += 1;
            // side view (fit_single_frame.py:527-551): second fit from the orientation rotated by pi
            // about y; pose embedding and camera translation continue from the first fit, every
            // other body parameter is zeroed; the lower final loss wins (:662-667)
            if constexpr (FIT) {
            if (stage == C.n_stages && last_stage == C.n_stages - 1 && D.try_both[b]) {
                float* X0 = D.X0 + (size_t)b * SFX_NPAR_MAX;
                LB_SYNC();
                if (pass == 0) {
                    for (int i = lane; i < SFX_NPAR_MAX; i += 64) X0[i] = X[i];
                    LB_SYNC();
                    const ParLayout& L = D.L;
                    for (int i = lane; i < L.npar; i += 64) {
                        const bool keep = (i >= L.cam_t && i < L.cam_t + 3) || (i >= L.emb && i < L.emb + L.NEMB);
                        if (!keep) X[i] = 0.f;
                    }
                    LB_SYNC();
                    if (lane == 0) {
                        float fl[3];
                        flipped_orientation(D.gocam + (size_t)b * 4, fl);
                        X[L.go] = fl[0]; X[L.go + 1] = fl[1]; X[L.go + 2] = fl[2];
                        D.orient_pass[b] = 1;
                    }
                    if (L.has_bodyp && lane < 63) X[L.bodyp + lane] = X[L.emb + lane];
                    LB_SYNC();
                    stage = 0;
                } else {
                    const float l0 = D.stage_loss[so + C.n_stages], l1 = res;
                    if (l0 < l1) {                       // first orientation wins: restore it
                        for (int i = lane; i < SFX_NPAR_MAX; i += 64) X[i] = X0[i];
                    } else if (lane == 0) {
                        for (int q = 1; q <= C.n_stages; ++q) D.stage_loss[so + q] = D.stage_loss2[so + q];
                    }
                    if (lane == 0) D.orient_pass[b] = 2;
                    LB_SYNC();
                }
            }
            }
            if (lane == 0) D.stage[b] = stage;
            s = fresh_state();
            for (int i = lane; i < SFX_NPAR_MAX; i += 64) Xt[i] = X[i];
            act = A_NONE;
            break;
        }
        default: act = A_NONE; break;
        }
    }
    TMARK(6);
    LB_SYNC();
    // write the working set back (WB = false: the caller does, with tick_write_back below)
    if constexpr (WB) {
#pragma unroll
    for (int k = 0; k < NVEC; ++k) st3_full(vecg + k * SFX_NVAR_MAX, ld3_raw(vec, (unsigned)k * SFX_NVAR_MAX, lane), lane);
    reinterpret_cast<float4*>(Xg)[lane] = reinterpret_cast<const float4*>(X)[lane];
    reinterpret_cast<float4*>(Xtg)[lane] = reinterpret_cast<const float4*>(Xt)[lane];
    if (lane == 0) gst->s = s_state;     // ro[] and the band tables are written in place
    }
    if (PF && lane == 0) *stage_out = stage;
    TMARK(7);
#undef TMARK
#undef TRACE
#undef VEC
}

// The write-back of a PF tick's working set by the whole workgroup (CT threads, behind a barrier after the tick): vectors, X and Xt
// are one run of s_work, a 16-byte store per thread; the scalar state a dword per thread.  Same bytes as the tick's own write-back.
template <int CT>
__device__ __forceinline__ void tick_write_back(const BatchDev& D, const int b, const float* s_work, const OptScal& s_state, const int t) {
    constexpr int NV4 = NVEC * SFX_NVAR_MAX / 4, NX4 = SFX_NPAR_MAX / 4;
    for (int i = t; i < NV4 + 2 * NX4; i += CT) {
        const float4 v = reinterpret_cast<const float4*>(s_work)[i];
        float4* dst = i < NV4 ? reinterpret_cast<float4*>(D.vec + (size_t)b * NVEC * SFX_NVAR_MAX) + i
                    : i < NV4 + NX4 ? reinterpret_cast<float4*>(D.X + (size_t)b * SFX_NPAR_MAX) + (i - NV4)
                                    : reinterpret_cast<float4*>(D.Xt + (size_t)b * SFX_NPAR_MAX) + (i - NV4 - NX4);
        *dst = v;
    }
    int* gs = reinterpret_cast<int*>(&(reinterpret_cast<OptState*>(D.opt) + b)->s);
    const int* ls = reinterpret_cast<const int*>(&s_state);
    for (int i = t; i < (int)(sizeof(OptScal) / 4); i += CT) gs[i] = ls[i];
}

// Entry for a workgroup: wavefront 0 runs the state machine, the others pass through.  SETS: see lb_two_loop.
template <int SETS, bool PF = false, bool WB = true, bool FIT = true>
__device__ __forceinline__ void lbfgs_tick_body(const DevModel& M, const BatchDev& D, const VarList* __restrict__ vls,
                                                int first_stage, int last_stage, int init, int step_mode,
                                                const int b, const int tid, float* s_al, OptScal& s_state, float* s_work,
                                                const float* f_src, const float* g_src, int* stage_out = nullptr,
                                                const int stage_in = -2) {
    if (tid >= 64) return;
    lbfgs_tick_wave0<SETS, PF, WB, FIT>(M, D, vls, first_stage, last_stage, init, step_mode, b, tid, s_al, s_state, s_work, f_src, g_src, stage_out, stage_in);
}


#pragma clang fp contract(fast)
