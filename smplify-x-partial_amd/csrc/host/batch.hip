// batch.hip -- a batch's life and its host-side I/O: sfx_batch_create / destroy (every device buffer of B frames), the frame
// data and parameter setters and getters with their float64 forms, stage weights and the GMM prior's upload.
#include "host.h"

#include <cmath>
#include <memory>

static void build_layout(ParLayout& L, int NB, int NE, int NPCA, int use_vposer, int latent) {
    L.NB = NB; L.NE = NE; L.NPCA = NPCA;
    L.cam_t = 0; L.go = 3; L.betas = 6; L.lh = L.betas + NB; L.rh = L.lh + NPCA; L.expr = L.rh + NPCA;
    L.jaw = L.expr + NE; L.leye = L.jaw + 3; L.reye = L.leye + 3; L.bodyp = L.reye + 3;
    L.has_bodyp = use_vposer ? 0 : 1;
    L.emb = L.bodyp + (L.has_bodyp ? 63 : 0);
    L.NEMB = use_vposer ? latent : 63;
    L.npar = L.emb + L.NEMB;
}

static void add_group(VarList& v, int off, int len, int has) {
    const int g = v.ngroups++;
    v.g_off[g] = (short)v.n; v.g_len[g] = (short)len; v.g_has[g] = (short)has;
    for (int i = 0; i < len; ++i, ++v.n) if (v.n < SFX_NVAR_MAX) v.idx[v.n] = (short)(off + i);     // (n > NVAR_MAX: rejected by the caller)
}

// One entry of opt_weights as the kernels read it: a StageW from float weights, a StageW64 from float (widened) or double ones.
// fit_single_frame.py:567-568: the bending weight, unless given, is a multiple of body_pose_weight, and the product is formed in
// the destination's type from the source's values -- fp32 in the reference's float run, double in its float64 run.
template <class W, class S>
static std::vector<W> stage_weights(const S* st, int n, bool coll) {
    using T = decltype(W::bpw);
    std::vector<W> out(std::max(1, n));
    for (int i = 0; i < n; ++i) {
        W& w = out[i];
        w.bpw = st[i].body_pose_weight; w.sw = st[i].shape_weight;
        w.bend = st[i].bending_prior_weight >= 0 ? (T)st[i].bending_prior_weight : (T)3.17 * (T)st[i].body_pose_weight;
        w.hpw = st[i].hand_prior_weight; w.epw = st[i].expr_prior_weight;
        for (int q = 0; q < 3; ++q) w.jaw[q] = st[i].jaw_prior_weight[q];
        w.hand_jw = st[i].hand_joint_weight; w.face_jw = st[i].face_joint_weight;
        w.coll = coll ? (T)st[i].coll_loss_weight : (T)0;       // (fitting.py:437; no interpenetration term in float64 mode)
    }
    return out;
}

extern "C" int sfx_batch_create(sfx_model* m, const sfx_batch_cfg* c, const sfx_stage_weights* st, sfx_batch** out) {
    if (!m || !c || !out) { sfx_set_error("null argument"); return -1; }
    if (c->n_stages < 0 || c->n_stages > SFX_MAX_STAGES) { sfx_set_error("n_stages=%d unsupported", c->n_stages); return -1; }
    if (c->use_vposer && m->M.vp_latent == 0) { sfx_set_error("use_vposer without sfx_model_set_vposer"); return -1; }
    if (c->high_precision == 2) {       // float64 end to end: the body-only needed-rows closure (FrameLDSSmall64) only
        const char* why = c->lbs_mode != 0 ? "lbs_mode must be 0 (needed rows)" : c->use_vposer ? "use_vposer" : c->use_hands ? "use_hands" :
                          c->use_face ? "use_face" : c->interpenetration ? "interpenetration" :
                          m->M.n_items > SFX_SMALL_ITEMS ? "a model whose keypoints need more than 32 vertex rows" : nullptr;
        if (why) { sfx_set_error("high_precision = 2 (float64) does not support %s", why); return -1; }
    }
    const int B = c->B, K = m->M.K;
    const bool pen_on = c->interpenetration != 0;
    // (round 5: a history_size beyond the default's 100 gets a ring of that many slots; the bound is the LDS array of the alphas)
    if (c->lbfgs_history_size > SFX_HIST_MAX) { sfx_set_error("history_size %d > %d", c->lbfgs_history_size, SFX_HIST_MAX); return -1; }
    if (pen_on && c->lbs_mode != 1) { sfx_set_error("interpenetration needs lbs_mode = 1 (the term reads every vertex)"); return -1; }
    if (pen_on && !(c->df_cone_height > 0.f)) { sfx_set_error("df_cone_height must be positive"); return -1; }
    if (c->side_view_thsh > 0.f && (c->left_shoulder_idx < 0 || c->left_shoulder_idx >= K || c->right_shoulder_idx < 0 || c->right_shoulder_idx >= K)) {
        sfx_set_error("shoulder indices out of range"); return -1; }
    ParLayout L{};
    build_layout(L, m->NB, m->NE, m->NPCA, c->use_vposer, m->M.vp_latent);
    if (L.npar > SFX_NPAR_MAX) { sfx_set_error("parameter block too large"); return -1; }
    VarList cam{}, body{};
    add_group(cam, L.cam_t, 3, 1); add_group(cam, L.go, 3, 1);
    // order of smplx.SMPLX.parameters() then pose_embedding (fit_single_frame.py:554-559)
    add_group(body, L.betas, L.NB, 1); add_group(body, L.go, 3, 1);
    // the dead body_pose parameter (zero gradient, never moves: SURVEY 7 quirk) takes 63 slots of the optimiser's vectors; with
    // all 45 + 45 hand variables (use_pca=False) the list would not fit, so it is left out there -- entries that are identically
    // zero in x, g, d, s and y contribute nothing to any dot product or norm of LBFGS.step / _strong_Wolfe
    const int n_live = L.NB + 3 + 2 * L.NPCA + 9 + L.NE + L.NEMB;
    if (L.has_bodyp && n_live + 63 <= SFX_NVAR_MAX) add_group(body, L.bodyp, 63, 0);
    add_group(body, L.lh, L.NPCA, 1); add_group(body, L.rh, L.NPCA, 1);
    add_group(body, L.jaw, 3, 1); add_group(body, L.leye, 3, 1); add_group(body, L.reye, 3, 1);
    add_group(body, L.expr, L.NE, 1); add_group(body, L.emb, L.NEMB, 1);
    if (body.n > SFX_NVAR_MAX) {
        // e.g. all 45 hand components: more optimisation variables than the optimiser's vectors hold.  Such a batch can
        // still evaluate the forward (sfx_lbs_forward / sfx_batch_forward); n_stages = 0 declares that intent
        if (c->n_stages > 0) { sfx_set_error("%d optimisation variables (limit %d): reduce num_pca_comps", body.n, SFX_NVAR_MAX); return -1; }
        body.n = SFX_NVAR_MAX;
    }
    // every argument is accepted: from here on only the device can refuse, and ~sfx_batch releases whatever was acquired by then
    std::unique_ptr<sfx_batch> b(new sfx_batch());
    b->m = m; b->K = K;
    BatchDev& D = b->D;
    D.L = L;
    D.cfg.B = B; D.cfg.n_stages = c->n_stages; D.cfg.use_vposer = c->use_vposer; D.cfg.use_hands = c->use_hands;
    D.cfg.use_face = c->use_face; D.cfg.use_conf = c->use_joints_conf; D.cfg.has_reg = c->has_regression_pose;
    D.cfg.use_conf_cam = c->use_conf_cam_init; D.cfg.nbj = c->num_body_joints; D.cfg.maxiters = c->maxiters;
    D.cfg.lbfgs_max_iter = c->lbfgs_max_iter > 0 ? c->lbfgs_max_iter : c->maxiters;
    D.cfg.max_eval = D.cfg.lbfgs_max_iter * 5 / 4; D.cfg.ftol = c->ftol; D.cfg.gtol = c->gtol;
    D.cfg.lr = c->lr; D.cfg.rho = c->rho; D.cfg.depth_w = c->depth_loss_weight; D.cfg.lbs_mode = c->lbs_mode;
    D.cfg.reuse = c->reuse_entry_eval;
    D.cfg.side_thsh = c->side_view_thsh; D.cfg.lsh = c->left_shoulder_idx; D.cfg.rsh = c->right_shoulder_idx;
    D.cfg.pen = pen_on ? 1 : 0;
    D.cfg.proj64 = c->high_precision ? 1 : 0;
    b->f64 = c->high_precision == 2;
    // negative = the reference's default; 0 is a legal value of lbfgs_ls.LBFGS (it disables the test) and reaches the device as 0
    D.cfg.tol_grad = c->lbfgs_tolerance_grad >= 0 ? c->lbfgs_tolerance_grad : 1e-5;
    D.cfg.tol_change = c->lbfgs_tolerance_change >= 0 ? c->lbfgs_tolerance_change : 1e-9;
    if (c->lbfgs_max_eval > 0) D.cfg.max_eval = c->lbfgs_max_eval;
    D.cfg.hist_cap = c->lbfgs_history_size > 0 ? c->lbfgs_history_size : SFX_HIST;
    D.cfg.hist_ring = std::max(D.cfg.hist_cap, SFX_HIST);
    {   // keypoints (and their vertex items: ascending in keypoint order) that are live while the hand / face joint weights are zero
        const int kl[3] = {std::min(K, c->num_body_joints), std::min(K, c->num_body_joints + 42), K};
        for (int q = 0; q < 3; ++q) {
            int n = 0;
            for (int i = 0; i < m->M.n_items; ++i) if (m->meta_host[MO_IK + i] < kl[q]) ++n;
            D.cfg.kl[q] = kl[q]; D.cfg.nil[q] = n;
        }
    }
    b->vl_host[0] = cam; b->vl_host[1] = body;
    std::vector<VarList> vls = {cam, body};
    b->vl_dev = b->mem.up(vls);
    b->sw_dev = b->mem.up(stage_weights<StageW>(st, c->n_stages, pen_on));
    if (b->f64) b->sw64_dev = b->mem.up(stage_weights<StageW64>(st, c->n_stages, false));      // (the float weights widened)
    D.Bpad = ((B + 127) / 128) * 128;
    D.X = b->mem.zeros<float>((size_t)B * SFX_NPAR_MAX);
    D.Xt = b->mem.zeros<float>((size_t)B * SFX_NPAR_MAX);
    if (b->f64) {       // the float64 mode's own buffers (typed twins; the fp32 ones stay, unused)
        D.X64 = b->mem.zeros<double>((size_t)B * SFX_NPAR_MAX);
        D.Xt64 = b->mem.zeros<double>((size_t)B * SFX_NPAR_MAX);
        D.f64 = b->mem.zeros<double>(B);
        D.g64 = b->mem.zeros<double>((size_t)B * SFX_NVAR_MAX);
        D.cam64 = b->mem.zeros<double>((size_t)B * 8);
    }
    D.gt = b->mem.zeros<float>((size_t)B * K * 2);
    D.conf = b->mem.zeros<float>((size_t)B * K);
    D.jw = b->mem.zeros<float>((size_t)B * K);
    D.cmask = b->mem.zeros<float>((size_t)B * K);
    D.cam = b->mem.zeros<float>((size_t)B * 8);
    D.camR = b->mem.zeros<float>((size_t)B * 9);
    D.regpose = b->mem.zeros<float>((size_t)B * 63);
    D.fd = b->mem.zeros<float>((size_t)B * FD_N);
    D.f = b->mem.zeros<float>(B);
    D.g = b->mem.zeros<float>((size_t)B * SFX_NVAR_MAX);
    D.bodypose = b->mem.zeros<float>((size_t)B * 63);
    D.featR = b->mem.zeros<float>((size_t)SFX_KD_PAD * D.Bpad);
    D.AT = b->mem.zeros<float>((size_t)12 * SFX_JPAD * D.Bpad);
    D.featR_w = D.featR; D.AT_w = D.AT;
    b->op_f[0] = D.featR; b->op_a[0] = D.AT;
    if (c->lbs_mode == 1 && !D.cfg.pen) {
        // the overlapped loop's further operand sets: two for the single rounds, a rotation of 2 x SFX_TICK_ROUNDS + 1 where the
        // multi-round form can run (host.h: 17 sets in all, 21 MB at 256 frames)
        b->n_sets = (m->M.n_uniq > 0 && m->M.n_uniq <= SFX_OV_SELF_UNIQ && sfx_small_closure(m->M, D)) ? OperandRing::kMaxSets : 3;
        for (int i = 1; i < b->n_sets; ++i) {
            b->op_f[i] = b->mem.zeros<float>((size_t)SFX_KD_PAD * D.Bpad);
            b->op_a[i] = b->mem.zeros<float>((size_t)12 * SFX_JPAD * D.Bpad);
        }
    }
    D.verts = b->mem.zeros<float>((size_t)B * m->M.V * 3);
    D.fwd = b->mem.zeros<float>((size_t)B * SFX_FWD_N);
    D.uvp = b->mem.zeros<float>((size_t)B * std::max(1, m->M.n_uniq) * 3);
    if (D.cfg.pen) {
        const int F = (int)(m->faces_host.size() / 3);
        const bool parts = !m->segm_host.empty();
        // collision buffers (partner lists, grid entries, pair list: ~45 MB per mesh at max_collisions 128) are indexed by
        // GEMM column, not by frame: a job that runs B frames through a pool of `slots` columns holds `slots` of them
        const int pen_cols = (c->slots > 0 && c->slots < B && c->lbs_mode == 1) ? std::min(B, ((c->slots + 31) / 32) * 32) : B;
        const int pen_cap = std::max(1, c->max_collisions);
        b->pen = m->pen_idle.take(pen_cols, pen_cap, m->parts_gen, &b->pen_cols);
        if (b->pen) sfx_pen_reuse(b->pen);
        else {
            int rc = sfx_pen_create(m->M.V, F, m->faces_host.data(), parts ? m->segm_host.data() : nullptr,
                                    parts ? m->parents_host.data() : nullptr, m->ign_host.empty() ? nullptr : m->ign_host.data(),
                                    (int)(m->ign_host.size() / 2), pen_cap, pen_cols, &b->pen);
            if (rc) return rc;
            b->pen_cols = pen_cols;
        }
        b->pen_cap = pen_cap; b->pen_gen = m->parts_gen;
        b->pen_sigma = c->df_cone_height; b->pen_outside = c->penalize_outside ? 1 : 0;
        (void)sfx_pen_set_point2plane(b->pen, c->point2plane);
        D.pen_loss = b->mem.zeros<float>(B);
        D.pen_dverts = b->mem.zeros<float>((size_t)B * m->M.V * 3);
        D.ext_n = b->mem.zeros<int>(B);
        D.pen_want = b->mem.zeros<int>(B);
        D.pen_over = b->mem.zeros<int>(B);
        D.pen_flag = b->mem.zeros<int>(B);
        D.vposed = b->mem.zeros<float>((size_t)B * m->M.V * 3);
        D.adj_G = b->mem.zeros<float>((size_t)D.Bpad * 3 * m->M.Vpad);
        D.adj_part = b->mem.zeros<float>((size_t)sfx_adj_slices(m->M) * SFX_KD_PAD * D.Bpad);
        D.pen_dfeat = b->mem.zeros<float>((size_t)B * SFX_KD_PAD);
        D.pen_dA = b->mem.zeros<float>((size_t)B * SFX_J * 12);
    }
    D.joints = b->mem.zeros<float>((size_t)B * K * 3);
    D.fullpose = b->mem.zeros<float>((size_t)B * SFX_POSE);
    D.stage = b->mem.zeros<int>(B);
    { std::vector<int> id(B); for (int i = 0; i < B; ++i) id[i] = i; D.slot = b->mem.up(id); D.nact = B; }
    b->act_dev = b->mem.zeros<int>(B); b->act_new_dev = b->mem.zeros<int>(B);
    b->slots = (c->slots > 0 && c->slots < B && c->lbs_mode == 1) ? ((c->slots + 31) / 32) * 32 : 0;
    if (b->slots >= B) b->slots = 0;
    D.opt = b->mem.zeros<char>((size_t)B * sfx_optstate_size());
    D.vec = b->mem.zeros<float>((size_t)B * NVEC * SFX_NVAR_MAX);
    D.hist = b->mem.zeros<float>((size_t)B * 2 * (D.cfg.hist_ring + 8) * SFX_NVAR_MAX);
    D.n_active = b->mem.zeros<int>(4);
    D.stage_loss = b->mem.zeros<float>((size_t)B * (1 + SFX_MAX_STAGES));
    D.stage_evals = b->mem.zeros<int>((size_t)B * (1 + SFX_MAX_STAGES));
    D.stage_ref_evals = b->mem.zeros<int>((size_t)B * (1 + SFX_MAX_STAGES));
    D.X0 = b->mem.zeros<float>((size_t)B * SFX_NPAR_MAX);
    D.gocam = b->mem.zeros<float>((size_t)B * 4);
    D.stage_loss2 = b->mem.zeros<float>((size_t)B * (1 + SFX_MAX_STAGES));
    D.try_both = b->mem.zeros<int>(B);
    D.orient_pass = b->mem.zeros<int>(B);
    if (b->mem.failed) { (void)hipGetLastError(); sfx_set_error("out of device memory (batch of %d frames)", B); return -2; }
    if (hipHostMalloc((void**)&b->stage_host, (size_t)SFX_POLL_BUFS * B * sizeof(int)) != hipSuccess) b->stage_host = nullptr;      // poll buffers
    if (hipHostMalloc((void**)&b->map_host, (size_t)SFX_POLL_BUFS * 3 * B * sizeof(int)) != hipSuccess) b->map_host = nullptr;
    if (c->lbs_mode == 1 && (!b->stage_host || !b->map_host)) {       // the fused dense loop polls through pinned memory
        sfx_set_error("out of pinned host memory"); return -2; }
    for (int i = 0; i < SFX_POLL_BUFS; ++i)
        if (hipEventCreateWithFlags(&b->poll_ev[i], hipEventDisableTiming) != hipSuccess) { sfx_set_error("event creation failed"); return -2; }
    *out = b.release();
    return 0;
}

sfx_batch::~sfx_batch() {
    for (auto& kv : pen_graphs) hipGraphExecDestroy(kv.second);
    if (cap_stream) hipStreamDestroy(cap_stream);
    if (s2) { (void)hipStreamSynchronize(s2); hipStreamDestroy(s2); }      // (DenseLoop::run drains it on every way out: nothing is pending)
    for (auto& ring : ov_ev) for (hipEvent_t e : ring) if (e) hipEventDestroy(e);
    if (pen) {             // the collision buffers go back to the model's idle slot (idle_slot.h), once nothing reads them any more
        (void)hipDeviceSynchronize();
        m->pen_idle.give(pen, pen_cols, pen_cap, pen_gen, m->parts_gen);
    }
    if (stage_host) hipHostFree(stage_host);
    if (map_host) hipHostFree(map_host);
    for (hipEvent_t e : poll_ev) if (e) hipEventDestroy(e);
}

extern "C" void sfx_batch_destroy(sfx_batch* b) { delete b; }

// gt | conf | jw | cmask | cam | camR | regpose of frame b -> its packed record D.fd[b] (what the closure workgroup
// loads in one 16-byte copy); launched after every host write to one of the seven arrays
__global__ void k_pack_fd(BatchDev D, int K) {
    const int b = blockIdx.x, t = threadIdx.x;
    float* fd = D.fd + (size_t)b * FD_N;
    for (int i = t; i < 2 * K; i += blockDim.x) fd[FD_GT + i] = D.gt[(size_t)b * K * 2 + i];
    for (int i = t; i < K; i += blockDim.x) {
        fd[FD_CONF + i] = D.conf[(size_t)b * K + i]; fd[FD_JW + i] = D.jw[(size_t)b * K + i]; fd[FD_CMASK + i] = D.cmask[(size_t)b * K + i]; }
    if (t < 8) fd[FD_CAM + t] = D.cam[(size_t)b * 8 + t];
    if (t < 9) fd[FD_CAMR + t] = D.camR[(size_t)b * 9 + t];
    if (t < 63) fd[FD_REG + t] = D.regpose[(size_t)b * 63 + t];
}
void pack_fd(sfx_batch* b, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_fd, dim3(b->D.cfg.B), dim3(128), 0, s, b->D, b->K);
}

// the camera record as the kernels read it: a frame's fx fy cx cy data_weight est_tz padded to 8 values
template <class T>
static std::vector<T> pad_cam(const T* cam, int B) {
    std::vector<T> c8((size_t)B * 8, T(0));
    for (int i = 0; i < B; ++i) for (int q = 0; q < 6; ++q) c8[(size_t)i * 8 + q] = cam[(size_t)i * 6 + q];
    return c8;
}

extern "C" int sfx_batch_set_frames(sfx_batch* b, const float* kp, const float* jw, const float* cmask,
                                    const float* cam, const float* camR) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    const int B = b->D.cfg.B, K = b->K;
    if (kp) {
        std::vector<float> gt((size_t)B * K * 2), cf((size_t)B * K);
        for (size_t i = 0; i < (size_t)B * K; ++i) { gt[2 * i] = kp[3 * i]; gt[2 * i + 1] = kp[3 * i + 1]; cf[i] = kp[3 * i + 2]; }
        SFX_CHECK(hipMemcpy(b->D.gt, gt.data(), gt.size() * 4, hipMemcpyHostToDevice));
        SFX_CHECK(hipMemcpy(b->D.conf, cf.data(), cf.size() * 4, hipMemcpyHostToDevice));
    }
    if (jw) SFX_CHECK(hipMemcpy(b->D.jw, jw, (size_t)B * K * 4, hipMemcpyHostToDevice));
    if (cmask) SFX_CHECK(hipMemcpy(b->D.cmask, cmask, (size_t)B * K * 4, hipMemcpyHostToDevice));
    if (cam) {
        const std::vector<float> c8 = pad_cam(cam, B);
        SFX_CHECK(hipMemcpy(b->D.cam, c8.data(), c8.size() * 4, hipMemcpyHostToDevice));
        if (b->f64) {       // (float64 batch: the float camera widened)
            std::vector<double> d8(c8.begin(), c8.end());
            SFX_CHECK(hipMemcpy(b->D.cam64, d8.data(), d8.size() * 8, hipMemcpyHostToDevice));
        }
    }
    if (camR) SFX_CHECK(hipMemcpy(b->D.camR, camR, (size_t)B * 9 * 4, hipMemcpyHostToDevice));
    pack_fd(b, 0);
    SFX_CHECK(hipDeviceSynchronize());
    return 0;
}

template <class T, class S>
static void put(std::vector<T>& X, int B, int off, int n, const S* src) {
    if (!src) return;
    for (int i = 0; i < B; ++i) for (int q = 0; q < n; ++q) X[(size_t)i * SFX_NPAR_MAX + off + q] = src[(size_t)i * n + q];
}
template <class T>
static void take(const std::vector<T>& X, int B, int off, int n, T* dst) {
    if (!dst) return;
    for (int i = 0; i < B; ++i) for (int q = 0; q < n; ++q) dst[(size_t)i * n + q] = X[(size_t)i * SFX_NPAR_MAX + off + q];
}

// Host parameters into the parameter block of a batch, X / Xt (floats) or X64 / Xt64 (doubles: float inputs are widened); NULL = keep
template <class T, class S>
static int scatter_params(sfx_batch* b, T* X_dev, T* Xt_dev, const S* cam_t, const S* go, const S* betas, const S* lh, const S* rh,
                          const S* expr, const S* jaw, const S* leye, const S* reye, const S* emb) {
    const int B = b->D.cfg.B; const ParLayout& L = b->D.L;
    std::vector<T> X((size_t)B * SFX_NPAR_MAX);
    SFX_CHECK(hipMemcpy(X.data(), X_dev, X.size() * sizeof(T), hipMemcpyDeviceToHost));
    put(X, B, L.cam_t, 3, cam_t); put(X, B, L.go, 3, go); put(X, B, L.betas, L.NB, betas);
    put(X, B, L.lh, L.NPCA, lh); put(X, B, L.rh, L.NPCA, rh); put(X, B, L.expr, L.NE, expr);
    put(X, B, L.jaw, 3, jaw); put(X, B, L.leye, 3, leye); put(X, B, L.reye, 3, reye);
    put(X, B, L.emb, L.NEMB, emb);
    // body_model.reset_params(body_pose=pose_embedding) also fills the (dead) body_pose parameter
    if (L.has_bodyp && emb) put(X, B, L.bodyp, 63, emb);
    SFX_CHECK(hipMemcpy(X_dev, X.data(), X.size() * sizeof(T), hipMemcpyHostToDevice));
    SFX_CHECK(hipMemcpy(Xt_dev, X.data(), X.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
// ... and back.  emb63: the embedding read as the 63 body-pose values (batches without VPoser)
template <class T>
static int gather_params(sfx_batch* b, const T* X_dev, T* cam_t, T* go, T* betas, T* lh, T* rh, T* expr, T* jaw, T* leye, T* reye,
                         T* emb, T* emb63) {
    const int B = b->D.cfg.B; const ParLayout& L = b->D.L;
    std::vector<T> X((size_t)B * SFX_NPAR_MAX);
    SFX_CHECK(hipMemcpy(X.data(), X_dev, X.size() * sizeof(T), hipMemcpyDeviceToHost));
    take(X, B, L.cam_t, 3, cam_t); take(X, B, L.go, 3, go); take(X, B, L.betas, L.NB, betas);
    take(X, B, L.lh, L.NPCA, lh); take(X, B, L.rh, L.NPCA, rh); take(X, B, L.expr, L.NE, expr);
    take(X, B, L.jaw, 3, jaw); take(X, B, L.leye, 3, leye); take(X, B, L.reye, 3, reye);
    take(X, B, L.emb, L.NEMB, emb); take(X, B, L.emb, 63, emb63);
    return 0;
}

extern "C" int sfx_batch_set_params(sfx_batch* b, const float* cam_t, const float* go, const float* betas,
                                    const float* lh, const float* rh, const float* expr, const float* jaw,
                                    const float* leye, const float* reye, const float* emb, const float* reg) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    const int B = b->D.cfg.B; const ParLayout& L = b->D.L;
    if (int rc = b->f64 ? scatter_params(b, b->D.X64, b->D.Xt64, cam_t, go, betas, lh, rh, expr, jaw, leye, reye, emb)
                        : scatter_params(b, b->D.X, b->D.Xt, cam_t, go, betas, lh, rh, expr, jaw, leye, reye, emb)) return rc;
    if (reg) {
        std::vector<float> r((size_t)B * 63, 0.f);
        for (int i = 0; i < B; ++i) for (int q = 0; q < L.NEMB; ++q) r[(size_t)i * 63 + q] = reg[(size_t)i * L.NEMB + q];
        SFX_CHECK(hipMemcpy(b->D.regpose, r.data(), r.size() * 4, hipMemcpyHostToDevice));
        pack_fd(b, 0);
        SFX_CHECK(hipDeviceSynchronize());
    }
    return 0;
}

extern "C" int sfx_batch_get_params(sfx_batch* b, float* cam_t, float* go, float* betas, float* lh, float* rh,
                                    float* expr, float* jaw, float* leye, float* reye, float* emb, float* body_pose) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_batch_get_params")) return -1;
    const bool decode = body_pose && b->D.cfg.use_vposer;
    if (int rc = gather_params(b, b->D.X, cam_t, go, betas, lh, rh, expr, jaw, leye, reye, emb, decode ? nullptr : body_pose)) return rc;
    if (decode) {       // the ACCEPTED latent decoded (fit_single_frame.py:653-657)
        forward_at_X(b, 0, 0, 0);
        SFX_CHECK(hipDeviceSynchronize());
        SFX_CHECK(hipMemcpy(body_pose, b->D.bodypose, (size_t)b->D.cfg.B * 63 * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}

// ---- float64 mode (high_precision = 2)
extern "C" int sfx_batch_set_stage_weights_f64(sfx_batch* b, const sfx_stage_weights_f64* st) {
    if (need_f64(b, "sfx_batch_set_stage_weights_f64")) return -1;
    if (!st) { sfx_set_error("null argument"); return -1; }
    const int n = b->D.cfg.n_stages;
    const std::vector<StageW64> w64 = stage_weights<StageW64>(st, n, false);
    SFX_CHECK(hipMemcpy(b->sw64_dev, w64.data(), (size_t)n * sizeof(StageW64), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int sfx_batch_set_frames_f64(sfx_batch* b, const double* kp, const double* jw, const double* cmask,
                                        const double* cam, const double* camR) {
    if (need_f64(b, "sfx_batch_set_frames_f64")) return -1;
    const int B = b->D.cfg.B, K = b->K;
    // the keypoint tables stay fp32 (the reference reads fp32 keypoints too): their values must be fp32 numbers
    if ((kp && !fp32_exact(kp, (size_t)B * K * 3)) || (jw && !fp32_exact(jw, (size_t)B * K)) ||
        (cmask && !fp32_exact(cmask, (size_t)B * K)) || (camR && !fp32_exact(camR, (size_t)B * 9))) {
        sfx_set_error("sfx_batch_set_frames_f64: keypoints, joint weights, masks and camera rotation must be fp32 values"); return -1; }
    auto narrow = [](const double* v, size_t n) { return std::vector<float>(v, v + n); };
    std::vector<float> k32, j32, m32, r32;
    if (kp) k32 = narrow(kp, (size_t)B * K * 3);
    if (jw) j32 = narrow(jw, (size_t)B * K);
    if (cmask) m32 = narrow(cmask, (size_t)B * K);
    if (camR) r32 = narrow(camR, (size_t)B * 9);
    std::vector<float> c32;
    if (cam) c32 = narrow(cam, (size_t)B * 6);      // (the fp32 record is only read by kernels the mode does not run)
    if (int rc = sfx_batch_set_frames(b, kp ? k32.data() : nullptr, jw ? j32.data() : nullptr, cmask ? m32.data() : nullptr,
                                      cam ? c32.data() : nullptr, camR ? r32.data() : nullptr)) return rc;
    if (cam) {
        const std::vector<double> d8 = pad_cam(cam, B);
        SFX_CHECK(hipMemcpy(b->D.cam64, d8.data(), d8.size() * 8, hipMemcpyHostToDevice));
    }
    return 0;
}

extern "C" int sfx_batch_set_params_f64(sfx_batch* b, const double* cam_t, const double* go, const double* betas,
                                        const double* lh, const double* rh, const double* expr, const double* jaw,
                                        const double* leye, const double* reye, const double* emb, const double* reg) {
    if (need_f64(b, "sfx_batch_set_params_f64")) return -1;
    const int B = b->D.cfg.B, nemb = b->D.L.NEMB;
    if (reg && !fp32_exact(reg, (size_t)B * nemb)) {
        sfx_set_error("sfx_batch_set_params_f64: the regression pose is kept in fp32 and must hold fp32 values"); return -1; }
    if (int rc = scatter_params(b, b->D.X64, b->D.Xt64, cam_t, go, betas, lh, rh, expr, jaw, leye, reye, emb)) return rc;
    if (reg) {
        std::vector<float> r(reg, reg + (size_t)B * nemb);
        return sfx_batch_set_params(b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, r.data());
    }
    return 0;
}

extern "C" int sfx_batch_get_params_f64(sfx_batch* b, double* cam_t, double* go, double* betas, double* lh, double* rh,
                                        double* expr, double* jaw, double* leye, double* reye, double* emb, double* body_pose) {
    if (need_f64(b, "sfx_batch_get_params_f64")) return -1;
    // (no VPoser in this mode: body_pose is the embedding)
    return gather_params(b, b->D.X64, cam_t, go, betas, lh, rh, expr, jaw, leye, reye, emb, body_pose);
}

extern "C" int sfx_batch_num_vars(sfx_batch* b, int32_t stage) {
    if (!b) return -1;
    return b->vl_host[stage < 0 ? 0 : 1].n;
}

// body_pose_prior = MaxMixturePrior (prior.py:100-231) for use_vposer=False fits without a regression
// prior (fitting.py:399-401).  means [M][D], precisions [M][D][D], nll_weights [M] (as the module's buffers)
extern "C" int sfx_batch_set_gmm_form(sfx_batch* b, int32_t M, int32_t Dm, const float* means, const float* precisions,
                                      const float* nll_weights, const float* comp_const) {
    if (!b || !means || !precisions || !nll_weights) { sfx_set_error("null argument"); return -1; }
    if (b->f64) { sfx_set_error("the mixture prior is fp32: not available on a float64 batch (high_precision = 2)"); return -1; }
    if (M < 1 || M > 2 * (256 / 64)) { sfx_set_error("1..8 mixture components supported, got %d", M); return -1; }
    if (b->D.cfg.use_vposer) { sfx_set_error("the mixture prior acts on body_pose: use_vposer must be off"); return -1; }
    if (Dm != b->D.L.NEMB) { sfx_set_error("mixture dimension %d != body pose dimension %d", Dm, b->D.L.NEMB); return -1; }
    std::vector<float> mu((size_t)M * 64, 0.f), P((size_t)M * 64 * 64, 0.f), lw(M);
    for (int m = 0; m < M; ++m) {
        if (!(nll_weights[m] > 0.f)) { sfx_set_error("nll_weights must be positive"); return -1; }
        lw[m] = logf(nll_weights[m]);
        for (int i = 0; i < Dm; ++i) {
            mu[(size_t)m * 64 + i] = means[(size_t)m * Dm + i];
            for (int j = 0; j < Dm; ++j)
                P[((size_t)m * 64 + j) * 64 + i] = 0.5f * (precisions[((size_t)m * Dm + i) * Dm + j] + precisions[((size_t)m * Dm + j) * Dm + i]);
        }
    }
    // merged form (prior.py:186-201): min_m [0.5 q_m - log w_m]; per-component form (:203-225): argmin_m [q_m + c_m], value + (-log w_m*)
    std::vector<float> csel(M), cadd(M);
    for (int m = 0; m < M; ++m) { csel[m] = comp_const ? comp_const[m] : -lw[m]; cadd[m] = comp_const ? -lw[m] : 0.f; }
    b->D.gmm_mean = b->mem.up(mu); b->D.gmm_prec = b->mem.up(P); b->D.gmm_lognw = b->mem.up(lw);
    b->D.gmm_csel = b->mem.up(csel); b->D.gmm_cadd = b->mem.up(cadd); b->D.gmm_scale = comp_const ? 1.f : 0.5f;
    if (!b->D.gmm_mean || !b->D.gmm_prec || !b->D.gmm_lognw || !b->D.gmm_csel || !b->D.gmm_cadd) { sfx_set_error("out of device memory"); return -2; }
    b->D.gmm_M = M;
    return 0;
}
extern "C" int sfx_batch_set_gmm(sfx_batch* b, int32_t M, int32_t Dm, const float* means, const float* precisions,
                                 const float* nll_weights) {
    return sfx_batch_set_gmm_form(b, M, Dm, means, precisions, nll_weights, nullptr);
}
