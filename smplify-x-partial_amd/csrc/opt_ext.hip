// opt_ext.hip -- the optimiser of lbfgs_body.h for evaluations the CALLER supplies: sfx_opt_* (include/sfx.h).
//
// Replaces, for B independent problems of N <= 192 variables whose loss and gradient come from outside the library:
//   FittingMonitor.run_fitting          smplifyx/fitting.py:147-217            (mode 0)
//   LBFGS.step                          smplifyx/optimizers/lbfgs_ls.py:256-445 (mode 1)
//   _strong_Wolfe / _cubic_interpolate  smplifyx/optimizers/lbfgs_ls.py:11-167
// The state machine is lbfgs_tick_wave0 itself without the fit's stage sequencing (FIT = false), over a BatchDev that holds one
// "stage" (0), an identity variable list and none of the model's buffers: one wavefront per problem consumes one evaluation
// per launch and leaves the next point to evaluate in the caller's buffer.  (The tick's scalar transitions: lbfgs_scalar.h.)
// The host half of the C ABI that sfx_opt_wide_* shares -- argument checks, defaults, the trace's owner -- is opt_host.h.
// Specification: oracle/lbfgs_machine.py (x_trial, feed(f, g), done, records).
#include "../../include/sfx.h"
#include "lbfgs_body.h"
#include "opt_host.h"

#include <memory>

// One launch = one evaluation of every running problem (init = 0), or the start of a run (init = 1 fresh, 2 resumed).
// The caller's rows are N long and packed, the machine's 192 (gradient) and 256 (point) long: the three copies between them
// (gradient in -- also kept for sfx_opt_get --, x0 in at the start, trial point out) are element-wise and bounded by N.
__global__ __launch_bounds__(64)
void k_opt_tick(BatchDev D, const VarList* __restrict__ vls, int init, int step_mode, int N, const float* __restrict__ x0,
                const float* __restrict__ loss, const float* __restrict__ grad, float* __restrict__ x_trial, int* __restrict__ evals) {
    __shared__ float s_al[SFX_HIST_MAX + 2 * LB_BS];
    __shared__ OptScal s_state;
    __shared__ __align__(16) float s_work[2048];
    __shared__ __align__(16) float s_g[SFX_NVAR_MAX];
    const int b = blockIdx.x, lane = threadIdx.x;
    const DevModel M{};           // (FIT = false: not read)
    float* Xg = D.X + (size_t)b * SFX_NPAR_MAX;
    const float* Xtg = D.Xt + (size_t)b * SFX_NPAR_MAX;
    float* xt_out = x_trial + (size_t)b * N;
    if (init) {
        for (int i = lane; i < SFX_NPAR_MAX; i += 64) Xg[i] = i < N ? x0[(size_t)b * N + i] : 0.f;
        if (lane == 0) {
            if (init == 1) evals[b] = 0;
            if (b == 0) *D.n_active = D.cfg.B;      // (no problem ends in this launch: nothing counts down yet)
        }
        LB_SYNC();
        lbfgs_tick_wave0<3, /* PF */ false, /* WB */ true, /* FIT */ false>(M, D, vls, 0, 0, init, step_mode, b, lane, s_al, s_state, s_work, loss, s_g);
        LB_SYNC();
        for (int i = lane; i < N; i += 64) xt_out[i] = Xtg[i];
        return;
    }
    if (D.stage[b] > 0) return;      // finished (1: run_fitting returned; 1000: LBFGS.step returned): left alone
    Lane3 g;
#pragma unroll
    for (int e = 0; e < NE3; ++e) { const int i = 3 * lane + e; g.v[e] = i < N ? grad[(size_t)b * N + i] : 0.f; }
    st3_full(s_g, g, lane);
    st3_full(D.g + (size_t)b * SFX_NVAR_MAX, g, lane);
    if (lane == 0) evals[b] += 1;
    LB_SYNC();
    lbfgs_tick_wave0<3, /* PF */ false, /* WB */ true, /* FIT */ false>(M, D, vls, 0, 0, 0, step_mode, b, lane, s_al, s_state, s_work, loss + b, s_g);
    LB_SYNC();
    for (int i = lane; i < N; i += 64) xt_out[i] = Xtg[i];
    if (lane == 0 && D.stage[b] > 0) atomicSub(D.n_active, 1);
}

struct sfx_opt {
    DevAlloc mem;
    OptTrace trace;             // (D.trace / D.trace_n / D.trace_cap are its view)
    BatchDev D{};
    VarList* vl_dev = nullptr;
    int* evals = nullptr;
    int N = 0;
    int mode = -1;              // of the last sfx_opt_begin (-1: none yet)
    int* active_host = nullptr; // pinned: the 4-byte readback of sfx_opt_active
    ~sfx_opt() { if (active_host) (void)hipHostFree(active_host); }
};

extern "C" int sfx_opt_create(const sfx_opt_cfg* c, sfx_opt** out) {
    if (!c || !out) { sfx_set_error("null argument"); return -1; }
    *out = nullptr;
    if (const int rc = opt_check_cfg("sfx_opt_create", c, SFX_NVAR_MAX, SFX_MAX_GROUPS)) return rc;
    // every argument is accepted: from here on only the device can refuse, and ~sfx_opt releases whatever was acquired by then
    std::unique_ptr<sfx_opt> h(new sfx_opt());
    const int B = c->B, N = c->N;
    h->N = N;
    BatchDev& D = h->D;
    BatchCfgDev& C = D.cfg;
    const OptDefaults d = opt_defaults(c);
    C.B = B; C.n_stages = 1;
    C.maxiters = c->maxiters; C.ftol = c->ftol; C.gtol = c->gtol; C.lr = c->lr;
    C.lbfgs_max_iter = d.max_iter; C.max_eval = d.max_eval;
    C.tol_grad = d.tol_grad; C.tol_change = d.tol_change;
    C.hist_cap = d.hist_cap;
    C.hist_ring = std::max(C.hist_cap, SFX_HIST);
    C.reuse = d.reuse;
    C.side_thsh = 0.f;
    VarList vl{};                  // identity: optimiser index i = slot i of the problem's row
    vl.n = N;
    for (int i = 0; i < SFX_NVAR_MAX; ++i) vl.idx[i] = (short)(i < N ? i : 0);
    vl.ngroups = c->n_groups > 0 ? c->n_groups : 1;
    for (int i = 0, o = 0; i < vl.ngroups; ++i) {
        const int len = c->n_groups > 0 ? c->group_len[i] : N;
        vl.g_off[i] = (short)o; vl.g_len[i] = (short)len; vl.g_has[i] = 1; o += len;
    }
    const VarList vls[2] = {vl, vl};
    h->vl_dev = h->mem.up(vls, 2);
    const size_t ns = 1 + SFX_MAX_STAGES;
    D.X = h->mem.zeros<float>((size_t)B * SFX_NPAR_MAX);
    D.Xt = h->mem.zeros<float>((size_t)B * SFX_NPAR_MAX);
    D.g = h->mem.zeros<float>((size_t)B * SFX_NVAR_MAX);
    D.stage = h->mem.zeros<int>(B);
    D.opt = h->mem.zeros<char>((size_t)B * sizeof(OptState));
    D.vec = h->mem.zeros<float>((size_t)B * NVEC * SFX_NVAR_MAX);
    D.hist = h->mem.zeros<float>((size_t)B * 2 * (C.hist_ring + 8) * SFX_NVAR_MAX);
    D.n_active = h->mem.zeros<int>(4);
    D.stage_loss = h->mem.zeros<float>(B * ns);
    D.stage_evals = h->mem.zeros<int>(B * ns);
    D.stage_ref_evals = h->mem.zeros<int>(B * ns);
    h->evals = h->mem.zeros<int>(B);
    if (h->mem.failed) {
        sfx_set_error("sfx_opt_create: device memory for %d problems: %s", B, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    if (hipHostMalloc((void**)&h->active_host, sizeof(int)) != hipSuccess) { (void)hipGetLastError(); h->active_host = nullptr; }
    *out = h.release();
    return 0;
}

extern "C" void sfx_opt_destroy(sfx_opt* h) { delete h; }

extern "C" int sfx_opt_begin(sfx_opt* h, int32_t mode, int32_t resume, const float* x0_dev, float* x_trial_dev, void* stream) {
    if (const int rc = opt_check_begin("sfx_opt_begin", !h || !x0_dev || !x_trial_dev, mode, resume, h ? h->mode : -1)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const BatchDev& D = h->D;
    if (!resume) {
        // the rows of an earlier run left in the ring are skipped with a factor 0: exact only while they are finite, which an
        // evaluation supplied from outside does not promise
        SFX_CHECK(hipMemsetAsync(D.hist, 0, (size_t)D.cfg.B * 2 * (D.cfg.hist_ring + 8) * SFX_NVAR_MAX * sizeof(float), s));
        if (const int rc = h->trace.empty(D.cfg.B, s)) return rc;
    }
    h->mode = mode;
    hipLaunchKernelGGL(k_opt_tick, dim3(D.cfg.B), dim3(64), 0, s, D, h->vl_dev, resume ? 2 : 1, mode, h->N, x0_dev,
                       (const float*)nullptr, (const float*)nullptr, x_trial_dev, h->evals);
    SFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sfx_opt_tell(sfx_opt* h, const float* loss_dev, const float* grad_dev, float* x_trial_dev, void* stream) {
    if (const int rc = opt_check_tell("sfx_opt_tell", "sfx_opt_begin", !h || !loss_dev || !grad_dev || !x_trial_dev, h ? h->mode : -1)) return rc;
    const BatchDev& D = h->D;
    hipLaunchKernelGGL(k_opt_tick, dim3(D.cfg.B), dim3(64), 0, (hipStream_t)stream, D, h->vl_dev, 0, h->mode, h->N,
                       (const float*)nullptr, loss_dev, grad_dev, x_trial_dev, h->evals);
    SFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sfx_opt_active(sfx_opt* h, int32_t* n_active_host, void* stream) {
    if (!h || !n_active_host) { sfx_set_error("sfx_opt_active: null argument"); return -1; }
    if (h->mode < 0) { *n_active_host = 0; return 0; }
    hipStream_t s = (hipStream_t)stream;
    int* dst = h->active_host ? h->active_host : n_active_host;
    SFX_CHECK(hipMemcpyAsync(dst, h->D.n_active, sizeof(int), hipMemcpyDeviceToHost, s));
    SFX_CHECK(hipStreamSynchronize(s));
    *n_active_host = *dst;
    return 0;
}

extern "C" int sfx_opt_get(sfx_opt* h, float* x_dev, float* grad_dev, float* result_host, int32_t* evals_host, int32_t* status_host) {
    if (!h) { sfx_set_error("sfx_opt_get: null handle"); return -1; }
    const BatchDev& D = h->D;
    const int B = D.cfg.B, N = h->N;
    SFX_CHECK(hipDeviceSynchronize());
    if (x_dev) SFX_CHECK(hipMemcpy2D(x_dev, (size_t)N * 4, D.X, (size_t)SFX_NPAR_MAX * 4, (size_t)N * 4, B, hipMemcpyDeviceToDevice));
    if (grad_dev) SFX_CHECK(hipMemcpy2D(grad_dev, (size_t)N * 4, D.g, (size_t)SFX_NVAR_MAX * 4, (size_t)N * 4, B, hipMemcpyDeviceToDevice));
    if (result_host) {
        std::vector<float> l((size_t)B * (1 + SFX_MAX_STAGES));
        SFX_CHECK(hipMemcpy(l.data(), D.stage_loss, l.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < B; ++i) result_host[i] = l[(size_t)i * (1 + SFX_MAX_STAGES) + 1];
    }
    if (evals_host) SFX_CHECK(hipMemcpy(evals_host, h->evals, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
    if (status_host) {
        SFX_CHECK(hipMemcpy(status_host, D.stage, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < B; ++i) status_host[i] = (h->mode >= 0 && status_host[i] > 0) ? 1 : 0;
    }
    return 0;
}

extern "C" int sfx_opt_trace(sfx_opt* h, int32_t capacity) {
    if (!h || capacity < 0) { sfx_set_error("sfx_opt_trace: bad argument"); return -1; }
    const int rc = h->trace.attach("sfx_opt_trace", h->D.cfg.B, capacity);
    h->trace.view(h->D.trace, h->D.trace_n, h->D.trace_cap);
    return rc;
}

extern "C" int sfx_opt_get_trace(sfx_opt* h, float* records, int32_t* counts) {
    return OptTrace::read(h ? &h->trace : nullptr, "sfx_opt_trace", h ? h->D.cfg.B : 0, records, counts);
}
