// eval.hip -- one evaluation at a time: the interpenetration step with its graph capture, the closure of a batch and the readers
// of loss and gradient, the camera-depth guess, the forward of a batch, and the stand-alone LBS (sfx_lbs_forward / _backward)
// on the model's lazily made batch.
#include "host.h"

#include <cstdlib>
#include <cstring>

// The joints-only forward at X (forward_only = 1: joints, full pose, decoded body pose; no loss), of `stage`'s kind.
void forward_at_X(sfx_batch* b, int stage, int use_dense_verts, hipStream_t s) {
    ClosureArgs a{}; a.stage_override = stage; a.forward_only = 1; a.from_X = 1; a.use_dense_verts = use_dense_verts;
    launch_closure(b->m->M, b->D, b->vl_dev, b->sw_dev, a, s);
}

// The dense path's first half: the export pass writes the GEMM operands, the whole-grid GEMM every vertex.  D: the batch's own
// BatchDev or a caller's modified copy (sfx_lbs_backward); time_export: the export pass under a ProfScope of its own (eval_closure).
static void export_and_gemm(sfx_batch* b, const BatchDev& D, int stage_override, int from_X, bool time_export, hipStream_t s) {
    const DevModel& M = b->m->M;
    ClosureArgs e{}; e.stage_override = stage_override; e.from_X = from_X; e.export_dense = 1; e.forward_only = 2;
    if (time_export) { ProfScope p("export", s); launch_closure(M, D, b->vl_dev, b->sw_dev, e, s); }
    else launch_closure(M, D, b->vl_dev, b->sw_dev, e, s);
    { ProfScope p("lbs_dense", s, D.nact); launch_lbs_dense(M, D, s); }
}

// one closure evaluation of every (active) frame; stage_override = -2 -> per-frame stage[]
// penetration term of the pending evaluation of every active frame (after the dense LBS wrote the
// vertices, before the loss / adjoint pass reads pen_loss, pen_dverts and the vertex lists)
// which GEMM columns hold a frame whose pending evaluation carries a collision weight (fitting.py:437:
// the term is only evaluated while coll_loss_weight > 0)
__global__ void k_pen_want(BatchDev D, const StageW* __restrict__ sws, int stage_override) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= D.cfg.B) return;
    const int st = stage_override != -2 ? stage_override : D.stage[b];
    if (st >= 0 && st < D.cfg.n_stages && D.slot[b] >= 0) D.pen_want[D.slot[b]] = sws[st].coll > 0.f;
}

// want_ready: the fused tick kernel maintains pen_want[] itself (it knows every running frame's next stage when it exports
// the next trial point, and clears the flag of a frame that finishes): no launch for it inside the fitting loop
int eval_penetration(sfx_batch* b, int stage_override, hipStream_t s, bool want_ready) {
    const BatchDev& D = b->D;
    if (!b->pen || D.nact <= 0) return 0;
    ProfScope p("penetration", s, D.nact);
    if (!want_ready) {
        hipMemsetAsync(D.pen_want, 0, (size_t)D.cfg.B * sizeof(int), s);
        hipLaunchKernelGGL(k_pen_want, dim3((D.cfg.B + 63) / 64), dim3(64), 0, s, D, b->sw_dev, stage_override);
    }
    // the collision buffers hold one mesh per column of the POOL (cfg.slots); inside the fused loop nact never exceeds it.
    // A stand-alone call on a pooled batch (sfx_batch_closure / sfx_batch_step: one column per frame, nact = B) walks the
    // columns in chunks of the pool's size -- the buffers are scratch between launches, every result lands in per-frame arrays
    const int cap = sfx_pen_capacity(b->pen);
    const DevModel& M = b->m->M;
    const size_t V3 = (size_t)M.V * 3;
    b->pen_chunked = D.nact > cap;
    const int stride = sfx_pen_stats_stride();
    if (b->pen_chunked && !b->pen_stats_all) {
        b->pen_stats_all = b->mem.zeros<int>((size_t)D.cfg.B * stride);
        if (!b->pen_stats_all) { sfx_set_error("out of device memory"); return -2; }
    }
    // Fused loop: the step is a captured graph (SFX_PEN_GRAPH=0 switches it off).  The first evaluation of a process runs directly
    // (one-time attribute calls inside), every new column count is captured once on the loop's own stream.
#ifdef SFX_LAB
    static const bool graph_on = [] { const char* e = getenv("SFX_PEN_GRAPH"); return !e || atoi(e) != 0; }();
#else
    constexpr bool graph_on = true;
#endif
    static bool warmed = false;
    if (want_ready && graph_on && warmed && !b->pen_chunked) {
        auto it = b->pen_graphs.find(D.nact);
        if (it == b->pen_graphs.end()) {
            hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
            if (!b->cap_stream) SFX_CHECK(hipStreamCreateWithFlags(&b->cap_stream, hipStreamNonBlocking));
            hipStream_t cs = b->cap_stream;
            SFX_CHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
            PenAdjPrep ap{D.AT, M.Wsp_j, M.Wsp_w, M.W, D.adj_G, D.Bpad, M.Vpad};
            const int rc = sfx_pen_eval_masked(b->pen, D.nact, D.verts, b->pen_sigma, b->pen_outside, D.pen_loss, D.pen_dverts, D.pen_want, &ap, D.pen_over, cs);
            launch_pen_adjoint(M, D, cs);
            const hipError_t ec = hipStreamEndCapture(cs, &graph);
            if (rc || ec != hipSuccess || !graph) { if (graph) hipGraphDestroy(graph); (void)hipGetLastError(); sfx_set_error("capture of the interpenetration step failed"); return rc ? rc : -2; }
            {   // what one round launches for the term: counted on the captured graph, not written down
                size_t nn = 0;
                if (hipGraphGetNodes(graph, nullptr, &nn) == hipSuccess) {
                    std::vector<hipGraphNode_t> nodes(nn);
                    int nk = 0;
                    if (nn && hipGraphGetNodes(graph, nodes.data(), &nn) == hipSuccess)
                        for (size_t i = 0; i < nn; ++i) { hipGraphNodeType ty; if (hipGraphNodeGetType(nodes[i], &ty) == hipSuccess && ty == hipGraphNodeTypeKernel) ++nk; }
                    b->pen_graph_nodes = nk;
                }
            }
            const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            hipGraphDestroy(graph);
            if (ei != hipSuccess) { sfx_set_error("hipGraphInstantiate failed"); return -2; }
            it = b->pen_graphs.emplace(D.nact, exec).first;
        }
        sfx_pen_note_batch(b->pen, D.nact);
        SFX_CHECK(hipGraphLaunch(it->second, s));
        return 0;
    }
    warmed = true;
    for (int c0 = 0; c0 < D.nact; c0 += cap) {
        const int n = std::min(cap, D.nact - c0);
        // the lane that forms a vertex' gradient also writes d v_posed = T^T g, the adjoint GEMM's operand (column c0 + local index)
        PenAdjPrep ap{D.AT + c0, M.Wsp_j, M.Wsp_w, M.W, D.adj_G + (size_t)c0 * 3 * M.Vpad, D.Bpad, M.Vpad};
        int rc = sfx_pen_eval_masked(b->pen, n, D.verts + c0 * V3, b->pen_sigma, b->pen_outside, D.pen_loss + c0, D.pen_dverts + c0 * V3,
                                     D.pen_want + c0, &ap, D.pen_over + c0, s);
        if (rc) return rc;
        if (b->pen_chunked)     // keep this chunk's diagnostics: the next chunk reuses the rows
            SFX_CHECK(hipMemcpyAsync(b->pen_stats_all + (size_t)c0 * stride, sfx_pen_stats_dev(b->pen), (size_t)n * stride * sizeof(int), hipMemcpyDeviceToDevice, s));
    }
    launch_pen_adjoint(M, D, s);
    return 0;
}

int eval_closure(sfx_batch* b, int stage_override, int from_X, hipStream_t s) {
    const DevModel& M = b->m->M; const BatchDev& D = b->D;
    ClosureArgs a{};
    a.stage_override = stage_override; a.from_X = from_X;
    // the camera stage asks for return_verts=False (fit_single_frame.py:485): the reference
    // still evaluates every vertex there, so dense mode does too.
    if (D.cfg.lbs_mode == 1) {
        export_and_gemm(b, D, stage_override, from_X, true, s);
        if (int rc = eval_penetration(b, stage_override, s)) return rc;
        a.use_dense_verts = 1;
    }
    ProfScope p("closure", s);
    launch_closure(M, D, b->vl_dev, b->sw_dev, a, s);
    return 0;
}

// rows of SFX_NVAR_MAX values on the device (a batch's g / g64) -> out [B][n] on the host
template <class T>
static int read_rows(const T* rows_dev, int B, int n, T* out) {
    std::vector<T> g((size_t)B * SFX_NVAR_MAX);
    SFX_CHECK(hipMemcpy(g.data(), rows_dev, g.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (int i = 0; i < B; ++i) memcpy(out + (size_t)i * n, &g[(size_t)i * SFX_NVAR_MAX], (size_t)n * sizeof(T));
    return 0;
}
// the end of both closure entry points: wait for the stream, then loss [B] and gradient [B][n] of the stage's variable list
template <class T>
static int closure_out(sfx_batch* b, int stage, hipStream_t s, const T* f_dev, const T* g_dev, T* loss_out, T* grad_out) {
    SFX_CHECK(hipStreamSynchronize(s));
    SFX_CHECK(hipGetLastError());
    const int B = b->D.cfg.B, N = b->vl_host[stage < 0 ? 0 : 1].n;
    if (loss_out) SFX_CHECK(hipMemcpy(loss_out, f_dev, (size_t)B * sizeof(T), hipMemcpyDeviceToHost));
    return grad_out ? read_rows(g_dev, B, N, grad_out) : 0;
}

extern "C" int sfx_batch_closure(sfx_batch* b, int32_t stage, float* loss_out, float* grad_out, void* stream) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_batch_closure")) return -1;
    if (stage >= b->D.cfg.n_stages) { sfx_set_error("stage %d out of range", stage); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (int rc = eval_closure(b, stage < 0 ? -1 : stage, 1, s)) return rc;
    return closure_out(b, stage, s, b->D.f, b->D.g, loss_out, grad_out);
}

extern "C" int sfx_batch_closure_f64(sfx_batch* b, int32_t stage, double* loss_out, double* grad_out, void* stream) {
    if (need_f64(b, "sfx_batch_closure_f64")) return -1;
    if (stage >= b->D.cfg.n_stages) { sfx_set_error("stage %d out of range", stage); return -1; }
    hipStream_t s = (hipStream_t)stream;
    ClosureArgs a{};
    a.stage_override = stage < 0 ? -1 : stage; a.from_X = 1;
    { ProfScope p("closure", s); launch_closure64(b->m->M, b->D, b->vl_dev, b->sw64_dev, a, s); }
    return closure_out(b, stage, s, b->D.f64, b->D.g64, loss_out, grad_out);
}

extern "C" int sfx_batch_get_grad(sfx_batch* b, int32_t stage, float* grad_out) {
    if (!b || !grad_out) { sfx_set_error("null argument"); return -1; }
    if (refuse_f64(b, "sfx_batch_get_grad")) return -1;
    if (stage < -1 || stage >= b->D.cfg.n_stages) { sfx_set_error("stage %d out of range", stage); return -1; }
    return read_rows(b->D.g, b->D.cfg.B, b->vl_host[stage < 0 ? 0 : 1].n, grad_out);
}

extern "C" int sfx_batch_get_grad_f64(sfx_batch* b, int32_t stage, double* grad_out) {
    if (need_f64(b, "sfx_batch_get_grad_f64")) return -1;
    if (!grad_out) { sfx_set_error("null argument"); return -1; }
    if (stage < -1 || stage >= b->D.cfg.n_stages) { sfx_set_error("stage %d out of range", stage); return -1; }
    return read_rows(b->D.g64, b->D.cfg.B, b->vl_host[stage < 0 ? 0 : 1].n, grad_out);
}

__global__ void k_guess_init(BatchDev D, int K, const int* pairs, int n_pairs) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= D.cfg.B) return;
    const float* j3 = D.joints + (size_t)b * K * 3;
    const float* j2 = D.gt + (size_t)b * K * 2;
    float s3 = 0.f, s2 = 0.f;
    for (int p = 0; p < n_pairs; ++p) {
        const int a = pairs[2 * p], c = pairs[2 * p + 1];
        const float dx = j3[a * 3] - j3[c * 3], dy = j3[a * 3 + 1] - j3[c * 3 + 1], dz = j3[a * 3 + 2] - j3[c * 3 + 2];
        const float ex = j2[a * 2] - j2[c * 2], ey = j2[a * 2 + 1] - j2[c * 2 + 1];
        s3 += sqrtf(dx * dx + dy * dy + dz * dz);
        s2 += sqrtf(ex * ex + ey * ey);
    }
    const float est = D.cam[(size_t)b * 8 + 0] * ((s3 / n_pairs) / (s2 / n_pairs));
    float* x = D.X + (size_t)b * SFX_NPAR_MAX + D.L.cam_t;
    x[0] = 0.f; x[1] = 0.f; x[2] = est;
    float* xt = D.Xt + (size_t)b * SFX_NPAR_MAX + D.L.cam_t;
    xt[0] = 0.f; xt[1] = 0.f; xt[2] = est;
    D.cam[(size_t)b * 8 + 5] = est;
}

extern "C" int sfx_batch_guess_init(sfx_batch* b, const int32_t* pairs, int32_t n_pairs, void* stream) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_batch_guess_init")) return -1;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> pv(pairs, pairs + 2 * n_pairs);
    DevAlloc scratch;
    int* pd = scratch.alloc<int>(pv.size());
    if (!pd) { (void)hipGetLastError(); sfx_set_error("out of device memory"); return -2; }
    SFX_CHECK(hipMemcpyAsync(pd, pv.data(), pv.size() * sizeof(int), hipMemcpyHostToDevice, s));
    forward_at_X(b, -1, 0, s);
    hipLaunchKernelGGL(k_guess_init, dim3((b->D.cfg.B + 63) / 64), dim3(64), 0, s, b->D, b->K, pd, n_pairs);
    pack_fd(b, s);          // (est_tz changed)
    SFX_CHECK(hipStreamSynchronize(s));
    SFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sfx_batch_forward(sfx_batch* b, float* verts_dev, float* joints_dev, void* stream) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_batch_forward")) return -1;
    hipStream_t s = (hipStream_t)stream;
    const DevModel& M = b->m->M; const BatchDev& D = b->D;
    if (D.cfg.lbs_mode == 0 && !verts_dev) {       // needed-rows batch, joints only: the forward the rows closure runs
        forward_at_X(b, 0, 0, s);
        if (joints_dev) SFX_CHECK(hipMemcpyAsync(joints_dev, D.joints, (size_t)D.cfg.B * M.K * 3 * 4, hipMemcpyDeviceToDevice, s));
        SFX_CHECK(hipStreamSynchronize(s));
        SFX_CHECK(hipGetLastError());
        return 0;
    }
    export_and_gemm(b, D, 0, 1, false, s);
    forward_at_X(b, 0, 1, s);
    const size_t nv = (size_t)D.cfg.B * M.V * 3 * 4, nj = (size_t)D.cfg.B * M.K * 3 * 4;
    if (verts_dev) SFX_CHECK(hipMemcpyAsync(verts_dev, D.verts, nv, hipMemcpyDeviceToDevice, s));
    if (joints_dev) SFX_CHECK(hipMemcpyAsync(joints_dev, D.joints, nj, hipMemcpyDeviceToDevice, s));
    SFX_CHECK(hipStreamSynchronize(s));
    SFX_CHECK(hipGetLastError());
    return 0;
}

__global__ void k_pack_params(BatchDev D, const float* go, const float* bp, const float* betas, const float* expr,
                              const float* jaw, const float* leye, const float* reye, const float* lh, const float* rh) {
    const int b = blockIdx.x, t = threadIdx.x;
    const ParLayout& L = D.L;
    float* x = D.X + (size_t)b * SFX_NPAR_MAX;
    auto cp = [&](int off, int n, const float* src) { if (t < n) x[off + t] = src ? src[(size_t)b * n + t] : 0.f; };
    cp(L.cam_t, 3, nullptr); cp(L.go, 3, go); cp(L.betas, L.NB, betas); cp(L.lh, L.NPCA, lh); cp(L.rh, L.NPCA, rh);
    cp(L.expr, L.NE, expr); cp(L.jaw, 3, jaw); cp(L.leye, 3, leye); cp(L.reye, 3, reye); cp(L.emb, 63, bp);
}

// the batch behind sfx_lbs_forward / sfx_lbs_backward: made for the first call, remade when B changes
static int fwd_batch(sfx_model* m, int32_t B) {
    if (!m->fwd || m->fwd_B != B) {
        sfx_batch_destroy(m->fwd);
        m->fwd = nullptr; m->fwd_B = 0;      // (sfx_batch_create writes its result only on success)
        sfx_batch_cfg c{}; c.B = B; c.n_stages = 0; c.maxiters = 1; c.num_body_joints = m->M.K; c.lbs_mode = 1;   // forward only
        sfx_stage_weights w{};
        int rc = sfx_batch_create(m, &c, &w, &m->fwd);
        if (rc) return rc;
        m->fwd_B = B;
    }
    return 0;
}

extern "C" int sfx_lbs_forward(sfx_model* m, int32_t B, const float* go, const float* bp, const float* betas,
                               const float* expr, const float* jaw, const float* leye, const float* reye,
                               const float* lh, const float* rh, float* verts_out, float* joints_out,
                               float* full_pose_out, void* stream) {
    if (!m) { sfx_set_error("null model"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (int rc = fwd_batch(m, B)) return rc;
    sfx_batch* b = m->fwd;
    hipLaunchKernelGGL(k_pack_params, dim3(B), dim3(64), 0, s, b->D, go, bp, betas, expr, jaw, leye, reye, lh, rh);
    int rc = sfx_batch_forward(b, verts_out, joints_out, s);
    if (rc) return rc;
    if (full_pose_out) SFX_CHECK(hipMemcpyAsync(full_pose_out, b->D.fullpose, (size_t)B * SFX_POSE * 4, hipMemcpyDeviceToDevice, s));
    SFX_CHECK(hipStreamSynchronize(s));
    return 0;
}

// Buffers of sfx_lbs_backward, on first use.  All of a group or none: a failed group is released at once, the batch keeps what
// it had and stays usable (forward, and a backward that needs less).
static int bwd_buffers(sfx_batch* b, bool verts) {
    const int B = b->D.cfg.B; const DevModel& M = b->m->M;
    if (!b->bwd_gc) {
        DevAlloc fresh;
        float* gc = fresh.zeros<float>((size_t)B * SFX_NPAR_MAX);
        if (fresh.failed) { (void)hipGetLastError(); sfx_set_error("sfx_lbs_backward: out of device memory (%d meshes)", B); return -2; }
        b->mem.ptrs.insert(b->mem.ptrs.end(), fresh.ptrs.begin(), fresh.ptrs.end()); fresh.ptrs.clear();
        b->bwd_gc = gc;
    }
    if (verts && !b->bwd.adj_G) {
        DevAlloc fresh;
        auto w = b->bwd;
        w.vposed = fresh.zeros<float>((size_t)B * M.V * 3);
        w.adj_G = fresh.zeros<float>((size_t)b->D.Bpad * 3 * M.Vpad);
        w.adj_part = fresh.zeros<float>((size_t)sfx_adj_slices(M) * SFX_KD_PAD * b->D.Bpad);
        w.dfeat = fresh.zeros<float>((size_t)B * SFX_KD_PAD);
        w.dA = fresh.zeros<float>((size_t)B * SFX_J * 12);
        w.want = fresh.up(std::vector<int>((size_t)B, 1));      // every column carries a vertex gradient
        if (fresh.failed) { (void)hipGetLastError(); sfx_set_error("sfx_lbs_backward: out of device memory (%d meshes)", B); return -2; }
        b->mem.ptrs.insert(b->mem.ptrs.end(), fresh.ptrs.begin(), fresh.ptrs.end()); fresh.ptrs.clear();
        b->bwd = w;
    }
    return 0;
}

extern "C" int sfx_lbs_backward(sfx_model* m, int32_t B, const float* go, const float* bp, const float* betas,
                                const float* expr, const float* jaw, const float* leye, const float* reye,
                                const float* lh, const float* rh, const float* dverts, const float* djoints,
                                float* d_go, float* d_bp, float* d_betas, float* d_expr, float* d_jaw, float* d_leye,
                                float* d_reye, float* d_lh, float* d_rh, void* stream) {
    if (!m) { sfx_set_error("null model"); return -1; }
    if (!dverts && !djoints) { sfx_set_error("sfx_lbs_backward: dvertices and djoints are both NULL (no upstream gradient)"); return -1; }
    if (B <= 0) { sfx_set_error("sfx_lbs_backward: B=%d", B); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (int rc = fwd_batch(m, B)) return rc;
    sfx_batch* b = m->fwd;
    if (int rc = bwd_buffers(b, dverts != nullptr)) return rc;
    const DevModel& M = m->M;
    // stateless: the forward is evaluated again at the inputs of THIS call (nothing of an earlier sfx_lbs_forward is read)
    hipLaunchKernelGGL(k_pack_params, dim3(B), dim3(64), 0, s, b->D, go, bp, betas, expr, jaw, leye, reye, lh, rh);
    BatchDev D = b->D;       // (by value to every kernel: the adjoint's pointers are attached to this copy only)
    ClosureArgs a{}; a.stage_override = 0; a.from_X = 1;
    if (dverts) {
        D.vposed = b->bwd.vposed; D.adj_G = b->bwd.adj_G; D.adj_part = b->bwd.adj_part; D.pen_dfeat = b->bwd.dfeat;
        D.pen_dA = b->bwd.dA; D.pen_want = b->bwd.want; D.pen_dverts = const_cast<float*>(dverts);      // (only ever read)
        export_and_gemm(b, D, 0, 1, false, s);      // (the GEMM writes v_posed of every vertex as well: D.vposed)
        { ProfScope p("lbs_adjoint", s, D.nact); launch_adj_prep(M, D, s); launch_pen_adjoint(M, D, s); }
        a.use_dense_verts = 1;
    }
    // joints only: no GEMM in either direction -- the keypoints' blend-shape rows are evaluated by the sweep's own forward
    launch_closure_ext(M, D, b->vl_dev, b->sw_dev, a, djoints, dverts ? 1 : 0, b->bwd_gc, s);
    launch_scatter_gc(D, b->bwd_gc, LbsGradOut{d_go, d_bp, d_betas, d_expr, d_jaw, d_leye, d_reye, d_lh, d_rh}, s);
    SFX_CHECK(hipStreamSynchronize(s));
    SFX_CHECK(hipGetLastError());
    return 0;
}
