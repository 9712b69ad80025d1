// inspect.hip -- looking at a batch from outside: debug reads of the dense path's buffers, the stand-alone two-loop recursion,
// the lab build's clocks and form switch (include/sfx_lab.h), the interpenetration term's diagnostics, trace and stage statistics.
#include "host.h"

#include <string>

#ifdef SFX_LAB       // include/sfx_lab.h
extern "C" int sfx_debug_phase_clocks(sfx_batch* b, int32_t stage, int64_t* out /* [32] */) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_debug_phase_clocks")) return -1;
    DevAlloc scratch;
    long long* d = scratch.zeros<long long>(64);
    if (scratch.failed) { (void)hipGetLastError(); sfx_set_error("out of device memory"); return -2; }
    { const long long freeze = 1 << 30; SFX_CHECK(hipMemcpy(d + 61, &freeze, sizeof(freeze), hipMemcpyHostToDevice)); }
    b->D.dbg = d;
    ClosureArgs a{}; a.stage_override = stage; a.from_X = 1;
    launch_closure(b->m->M, b->D, b->vl_dev, b->sw_dev, a, 0);
    launch_closure(b->m->M, b->D, b->vl_dev, b->sw_dev, a, 0);      // second launch: warm caches
    const hipError_t es = hipDeviceSynchronize();
    b->D.dbg = nullptr;         // (detached on every way out: the buffer goes with this call)
    SFX_CHECK(es);
    long long h[64];
    SFX_CHECK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < 32; ++i) out[i] = h[i];
    return 0;
}
#endif

// debug / tests: copy one of the dense path's device buffers of the most recent evaluation to the host.
// name -> floats per frame (rows are GEMM columns = frames while no compaction is in force):
//   "verts" V*3, "vposed" V*3, "pen_dverts" V*3, "pen_dfeat" 512, "pen_dA" 55*12, "pen_loss" 1,
//   "A" 12*55 (skinning transforms, [row*4+col][joint] gathered from the GEMM operand), "feat" 512,
//   "uvp" n_uniq*3 (blend offsets of the exported vertices as the dense GEMM wrote them), "uvp_self" n_uniq*3 (the same from
//   closure_lds.h self_blend_offsets on the current "feat": one launch of k_uvp_self into a scratch buffer),
//   "fwd" SFX_FWD_N = 6016 (rows are frames: the forward state each frame's latest export pass saved for its loss / adjoint pass)
extern "C" int sfx_batch_debug_read(sfx_batch* b, const char* name, float* out, int64_t n_out) {
    if (!b || !name || !out) { sfx_set_error("null argument"); return -1; }
    const BatchDev& D = b->D; const int B = D.cfg.B, V = b->m->M.V;
    const std::string k(name);
    SFX_CHECK(hipDeviceSynchronize());
    auto plain = [&](const float* src, size_t per) -> int {
        if (!src) { sfx_set_error("buffer '%s' is not allocated in this batch", name); return -1; }
        if ((int64_t)(per * B) != n_out) { sfx_set_error("'%s' holds %zu floats, caller asked for %lld", name, per * B, (long long)n_out); return -1; }
        SFX_CHECK(hipMemcpy(out, src, per * B * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    };
    if (k == "verts") return plain(D.verts, (size_t)V * 3);
    if (k == "vposed") return plain(D.vposed, (size_t)V * 3);
    if (k == "pen_dverts") return plain(D.pen_dverts, (size_t)V * 3);
    if (k == "pen_dfeat") return plain(D.pen_dfeat, SFX_KD_PAD);
    if (k == "pen_dA") return plain(D.pen_dA, (size_t)SFX_J * 12);
    if (k == "pen_loss") return plain(D.pen_loss, 1);
    if (k == "uvp") return plain(D.uvp, (size_t)b->m->M.n_uniq * 3);
    if (k == "fwd") return plain(D.fwd, SFX_FWD_N);
    if (k == "uvp_self") {
        const size_t n = (size_t)B * b->m->M.n_uniq * 3;
        if ((int64_t)n != n_out) { sfx_set_error("'%s' holds %zu floats, caller asked for %lld", name, n, (long long)n_out); return -1; }
        if (!n) return 0;
        if (!D.featR) { sfx_set_error("buffer '%s' is not allocated in this batch", name); return -1; }
        DevAlloc scratch;
        float* d = scratch.zeros<float>(n);
        if (!d) { (void)hipGetLastError(); sfx_set_error("out of device memory"); return -2; }
        launch_uvp_self(b->m->M, D, d, nullptr);
        SFX_CHECK(hipDeviceSynchronize());
        SFX_CHECK(hipMemcpy(out, d, n * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    if (k == "A" || k == "feat") {
        const size_t rows = k == "A" ? (size_t)12 * SFX_JPAD : SFX_KD_PAD, per = k == "A" ? (size_t)12 * SFX_J : SFX_KD_PAD;
        if ((int64_t)(per * B) != n_out) { sfx_set_error("'%s' holds %zu floats, caller asked for %lld", name, per * B, (long long)n_out); return -1; }
        std::vector<float> h(rows * D.Bpad);
        SFX_CHECK(hipMemcpy(h.data(), k == "A" ? D.AT : D.featR, h.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int i = 0; i < B; ++i) {
            if (k == "A") { for (int e = 0; e < 12; ++e) for (int j = 0; j < SFX_J; ++j) out[((size_t)i * 12 + e) * SFX_J + j] = h[((size_t)e * SFX_JPAD + j) * D.Bpad + i]; }
            else for (int q = 0; q < SFX_KD_PAD; ++q) out[(size_t)i * SFX_KD_PAD + q] = h[(size_t)i * SFX_KD_PAD + q];
        }
        return 0;
    }
    sfx_set_error("unknown buffer '%s'", name);
    return -1;
}

// Stand-alone operator: the direction the device's blocked two-loop recursion (lbfgs_two_loop.h lb_two_loop) computes from a history of `count`
// curvature pairs pushed in order (rows of SFX_NVAR_MAX = 192 floats, zero padded; the window keeps the last history_size,
// <= 0: 100) and a gradient g: d = -H g with H_diag = y.s / y.y of the last pair (lbfgs_ls.py:312-341).  Host pointers.
extern "C" int sfx_lbfgs_two_loop(const float* S, const float* Y, int32_t count, int32_t history_size, const float* g, float* d_out) {
    if (!S || !Y || !g || !d_out || count < 1 || history_size > SFX_HIST_MAX) { sfx_set_error("sfx_lbfgs_two_loop: bad arguments"); return -1; }
    const int rc = debug_two_loop(S, Y, count, history_size > 0 ? history_size : SFX_HIST, g, d_out);
    if (rc) { sfx_set_error("sfx_lbfgs_two_loop: HIP error"); return -1; }
    return 0;
}

#ifdef SFX_LAB       // include/sfx_lab.h
extern "C" int sfx_debug_lbs_dense_form(int32_t form) {
    const int prev = g_lbs_dense_form;
    if (form == 16 || form == 17 || form == 32) g_lbs_dense_form = form;
    return prev;
}

// debug: attach (enable=1) / read out and detach (enable=0) the 64-slot clock buffer; while attached,
// closure launches stamp dbg[0..18] and optimiser ticks of frame 0 accumulate dbg[32..63]
extern "C" int sfx_debug_clocks(sfx_batch* b, int32_t enable, int64_t* out /* [64] or NULL */) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (enable) {
        if (!b->dbg_buf && !(b->dbg_buf = b->mem.alloc<long long>(64))) { (void)hipGetLastError(); sfx_set_error("out of device memory"); return -2; }
        b->D.dbg = b->dbg_buf;
        SFX_CHECK(hipMemset(b->D.dbg, 0, 64 * sizeof(long long)));
        const long long freeze = enable > 1 ? enable : 40;      // k_tick_dense: stamps freeze after this launch
        SFX_CHECK(hipMemcpy(b->D.dbg + 61, &freeze, sizeof(freeze), hipMemcpyHostToDevice));
        return 0;
    }
    if (!b->D.dbg) { sfx_set_error("clock buffer not attached"); return -1; }
    SFX_CHECK(hipDeviceSynchronize());
    long long h[64];
    SFX_CHECK(hipMemcpy(h, b->D.dbg, sizeof(h), hipMemcpyDeviceToHost));
    b->D.dbg = nullptr;         // (the buffer stays with the batch for the next attach)
    if (out) for (int i = 0; i < 64; ++i) out[i] = h[i];
    return 0;
}
#endif

__global__ void k_count_grad_vertices(BatchDev D, int V) {
    __shared__ int cnt;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int n = 0;
    if (D.pen_want[b]) {
        const float* g = D.pen_dverts + (size_t)b * V * 3;
        for (int v = threadIdx.x; v < V; v += blockDim.x) n += (g[v * 3] != 0.f || g[v * 3 + 1] != 0.f || g[v * 3 + 2] != 0.f) ? 1 : 0;
    }
    atomicAdd(&cnt, n);
    __syncthreads();
    if (threadIdx.x == 0) D.ext_n[b] = cnt;
}

// the diagnostics of the interpenetration term: only where the term is
static int need_pen(const sfx_batch* b) { if (b->pen) return 0; sfx_set_error("batch was created without interpenetration"); return -1; }

extern "C" int sfx_batch_pen_stats(sfx_batch* b, int32_t* stats_host /* [B][4] */, int32_t* ext_n_host /* [B] or NULL */) {
    if (!b || !stats_host) { sfx_set_error("null argument"); return -1; }
    if (need_pen(b)) return -1;
    const int n = std::max(1, b->D.nact);
    int rc = b->pen_chunked ? sfx_pen_stats_from(b->pen_stats_all, n, stats_host)
                            : sfx_pen_stats(b->pen, std::min(n, sfx_pen_capacity(b->pen)), stats_host);
    if (rc) return rc;
    if (ext_n_host) {       // vertices that carry a gradient: counted on demand (it was an atomic per wavefront in every evaluation)
        hipLaunchKernelGGL(k_count_grad_vertices, dim3(n), dim3(256), 0, 0, b->D, b->m->M.V);
        SFX_CHECK(hipDeviceSynchronize());
        SFX_CHECK(hipMemcpy(ext_n_host, b->D.ext_n, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int sfx_batch_pen_pairs(sfx_batch* b, int32_t column, int32_t cap, int32_t* pairs_host, int32_t* n_out) {
    if (!b || !n_out) { sfx_set_error("null argument"); return -1; }
    if (need_pen(b)) return -1;
    if (b->pen_chunked) { sfx_set_error("the pair lists of a pooled batch's stand-alone evaluation are overwritten chunk by chunk"); return -1; }
    return sfx_pen_pairs(b->pen, column, cap, pairs_host, n_out);
}

extern "C" int sfx_batch_pen_launches(sfx_batch* b) {
    if (!b) { sfx_set_error("null argument"); return -1; }
    return b->pen_graph_nodes;
}

extern "C" int sfx_batch_pen_flags(sfx_batch* b, int32_t* flags_host /* [B] */) {
    if (!b || !flags_host) { sfx_set_error("null argument"); return -1; }
    if (need_pen(b)) return -1;
    SFX_CHECK(hipDeviceSynchronize());
    SFX_CHECK(hipMemcpy(flags_host, b->D.pen_flag, (size_t)b->D.cfg.B * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sfx_batch_trace(sfx_batch* b, int32_t capacity) {
    if (!b) { sfx_set_error("bad argument"); return -1; }
    if (refuse_f64(b, "sfx_batch_trace")) return -1;
    BatchDev& D = b->D;
    D.trace_evals = capacity < 0 ? 1 : 0;          // negative capacity: also one record per closure evaluation (debug)
    if (capacity < 0) capacity = -capacity;
    SFX_CHECK(hipDeviceSynchronize());
    b->trace_mem.clear(); D.trace = nullptr; D.trace_n = nullptr; D.trace_cap = 0;
    if (capacity == 0) return 0;
    // both buffers or neither: the kernels test D.trace alone, so a half-attached trace must never be left behind
    DevAlloc fresh;
    float4* tr = fresh.alloc<float4>((size_t)D.cfg.B * capacity);
    int* tn = fresh.zeros<int>(D.cfg.B);
    if (fresh.failed) { sfx_set_error("sfx_batch_trace: %s", hipGetErrorString(hipGetLastError())); return -2; }
    std::swap(b->trace_mem.ptrs, fresh.ptrs);
    D.trace = tr; D.trace_n = tn; D.trace_cap = capacity;
    return 0;
}

extern "C" int sfx_batch_get_trace(sfx_batch* b, float* records, int32_t* counts) {
    if (refuse_f64(b, "sfx_batch_get_trace")) return -1;
    if (!b || !b->D.trace) { sfx_set_error("no trace buffer attached (sfx_batch_trace)"); return -1; }
    const BatchDev& D = b->D;
    SFX_CHECK(hipDeviceSynchronize());
    if (records) SFX_CHECK(hipMemcpy(records, D.trace, (size_t)D.cfg.B * D.trace_cap * sizeof(float4), hipMemcpyDeviceToHost));
    if (counts) SFX_CHECK(hipMemcpy(counts, D.trace_n, (size_t)D.cfg.B * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sfx_batch_get_stats(sfx_batch* b, float* stage_loss, int32_t* stage_evals, int32_t* stage_ref_evals) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_batch_get_stats")) return -1;
    const int B = b->D.cfg.B, NS = b->D.cfg.n_stages + 1;
    std::vector<float> l((size_t)B * (1 + SFX_MAX_STAGES));
    std::vector<int> e(l.size()), r(l.size());
    SFX_CHECK(hipMemcpy(l.data(), b->D.stage_loss, l.size() * 4, hipMemcpyDeviceToHost));
    SFX_CHECK(hipMemcpy(e.data(), b->D.stage_evals, e.size() * 4, hipMemcpyDeviceToHost));
    SFX_CHECK(hipMemcpy(r.data(), b->D.stage_ref_evals, r.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < B; ++i)
        for (int q = 0; q < NS; ++q) {
            if (stage_loss) stage_loss[(size_t)i * NS + q] = l[(size_t)i * (1 + SFX_MAX_STAGES) + q];
            if (stage_evals) stage_evals[(size_t)i * NS + q] = e[(size_t)i * (1 + SFX_MAX_STAGES) + q];
            if (stage_ref_evals) stage_ref_evals[(size_t)i * NS + q] = r[(size_t)i * (1 + SFX_MAX_STAGES) + q];
        }
    return 0;
}
