// opt_host.h -- the host half that the two handles for caller-supplied evaluations share: sfx_opt_* (opt_ext.hip) and
// sfx_opt_wide_* (opt_wide.hip).  The argument checks with their messages (`fn` is the entry's name as the caller sees it), the
// defaults of optim_factory.py:50-52, the mode / resume rule of begin, and the owner of the optimiser trace.  Nothing here
// touches the device before every argument has passed.
#pragma once
#include "sfx_internal.h"

template <class T> static inline bool opt_is_null(const T* p) { return p == nullptr; }      // (sfx_opt_cfg.group_len is an array: never)

// sfx_*_create: the configuration (Cfg: sfx_opt_cfg or sfx_opt_wide_cfg -- the same field names), then the device.
// 0, or the entry's return code with the message set.
template <class Cfg>
static inline int opt_check_cfg(const char* fn, const Cfg* c, int n_max, int groups_max) {
    if (c->N < 1 || c->N > n_max) { sfx_set_error("%s: N = %d, supported 1..%d", fn, c->N, n_max); return -1; }
    if (c->B < 1) { sfx_set_error("%s: B = %d, at least 1 problem is needed", fn, c->B); return -1; }
    if (c->n_groups < 0 || c->n_groups > groups_max || (c->n_groups > 0 && opt_is_null(c->group_len))) {
        sfx_set_error("%s: %d parameter groups, at most %d", fn, c->n_groups, groups_max); return -1; }
    if (c->n_groups > 0) {
        long sum = 0;
        for (int i = 0; i < c->n_groups; ++i) {
            if (c->group_len[i] < 1) { sfx_set_error("%s: group %d has length %d", fn, i, c->group_len[i]); return -1; }
            sum += c->group_len[i];
        }
        if (sum != c->N) { sfx_set_error("%s: group lengths sum to %ld, N = %d", fn, sum, c->N); return -1; }
    }
    if (c->history_size < 0 || c->history_size > SFX_HIST_MAX) {
        sfx_set_error("%s: history_size %d, supported 1..%d (0 = %d)", fn, c->history_size, SFX_HIST_MAX, SFX_HIST); return -1; }
    if (c->maxiters < 1) { sfx_set_error("%s: maxiters = %d", fn, c->maxiters); return -1; }
    if (c->max_iter < 0 || c->max_eval < 0) { sfx_set_error("%s: negative max_iter / max_eval", fn); return -1; }
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        (void)hipGetLastError();
        sfx_set_error("%s: no HIP device (there is no CPU fallback)", fn); return -3;
    }
    return 0;
}

// what the configuration's zeros and negatives stand for
struct OptDefaults { int max_iter, max_eval, hist_cap, reuse; double tol_grad, tol_change; };
template <class Cfg>
static inline OptDefaults opt_defaults(const Cfg* c) {
    OptDefaults d;
    d.max_iter = c->max_iter > 0 ? c->max_iter : c->maxiters;
    d.max_eval = c->max_eval > 0 ? c->max_eval : d.max_iter * 5 / 4;
    d.tol_grad = c->tolerance_grad >= 0 ? c->tolerance_grad : 1e-5;
    d.tol_change = c->tolerance_change >= 0 ? c->tolerance_change : 1e-9;
    d.hist_cap = c->history_size > 0 ? c->history_size : SFX_HIST;
    d.reuse = c->reuse_entry_eval ? 1 : 0;
    return d;
}

// sfx_*_begin and sfx_*_tell; last_mode: of the handle's previous begin (-1: none)
static inline int opt_check_begin(const char* fn, bool null_arg, int mode, int resume, int last_mode) {
    if (null_arg) { sfx_set_error("%s: null argument", fn); return -1; }
    if (mode != 0 && mode != 1) { sfx_set_error("%s: mode %d (0 = run_fitting, 1 = one LBFGS.step)", fn, mode); return -1; }
    if (resume && (mode != 1 || last_mode != 1)) {
        sfx_set_error("%s: resume continues a mode-1 run (one LBFGS.step) with another; there is none", fn); return -1; }
    return 0;
}
static inline int opt_check_tell(const char* fn, const char* begin_fn, bool null_arg, int last_mode) {
    if (null_arg) { sfx_set_error("%s: null argument", fn); return -1; }
    if (last_mode < 0) { sfx_set_error("%s before %s", fn, begin_fn); return -1; }
    return 0;
}

// The optimiser trace of a handle: `cap` records per problem and the number written per problem.  The handle's device struct
// (BatchDev / WideDev: what the kernels see) holds copies of the three fields, refreshed with view() after every attach.
struct OptTrace {
    DevAlloc mem;
    float4* rec = nullptr; int* n = nullptr; int cap = 0;
    void view(float4*& d_rec, int*& d_n, int& d_cap) const { d_rec = rec; d_n = n; d_cap = cap; }
    // sfx_*_trace: capacity > 0 attaches, 0 detaches
    int attach(const char* fn, int B, int capacity) {
        SFX_CHECK(hipDeviceSynchronize());
        mem.clear(); rec = nullptr; n = nullptr; cap = 0;
        if (capacity == 0) return 0;
        // both buffers or neither: the kernel tests the records' pointer alone, so a half-attached trace must never be left behind
        DevAlloc fresh;
        float4* tr = fresh.alloc<float4>((size_t)B * capacity);
        int* tn = fresh.zeros<int>(B);
        if (fresh.failed) { sfx_set_error("%s: %s", fn, hipGetErrorString(hipGetLastError())); return -2; }
        std::swap(mem.ptrs, fresh.ptrs);
        rec = tr; n = tn; cap = capacity;
        return 0;
    }
    int empty(int B, hipStream_t s) {      // a fresh begin empties it
        if (n) SFX_CHECK(hipMemsetAsync(n, 0, (size_t)B * sizeof(int), s));
        return 0;
    }
    // sfx_*_get_trace (t: the handle's trace, null without a handle)
    static int read(const OptTrace* t, const char* attach_fn, int B, float* records, int32_t* counts) {
        if (!t || !t->rec) { sfx_set_error("no trace buffer attached (%s)", attach_fn); return -1; }
        SFX_CHECK(hipDeviceSynchronize());
        if (records) SFX_CHECK(hipMemcpy(records, t->rec, (size_t)B * t->cap * sizeof(float4), hipMemcpyDeviceToHost));
        if (counts) SFX_CHECK(hipMemcpy(counts, t->n, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        return 0;
    }
};
