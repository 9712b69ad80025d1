// objective_ext.hip -- the fitting objective as a function of TENSORS the caller supplies: sfx_objective_eval and
// sfx_camera_init_eval (include/sfx.h).  Loss and gradient of every frame come from ONE launch.
//
// Replaces, for B frames whose joints were produced by anything (this library's LBS, a regressor of the caller's):
//   camera(joints)                     smplifyx/camera.py:93-117
//   SMPLifyLoss.forward                smplifyx/fitting.py:375-461 (without the interpenetration lines :437-455)
//   SMPLifyCameraInitLoss.forward      smplifyx/fitting.py:499-520
//   GMoF.forward                       smplifyx/utils.py:84-95
//   L2Prior / SMPLifyAnglePrior / MaxMixturePrior   smplifyx/prior.py:53-97, :100-231
//   total_loss.backward()              autograd from the total down to the tensors named above
//
// Work decomposition: one wavefront per frame, OBJ_WAVES frames per workgroup; no LDS, no barrier, no atomics.
//   keypoints      strided over the 64 lanes (pass p takes keypoints 64 p .. 64 p + 63); a lane keeps its partial sums of the
//                  loss, d translation (3) and d rotation (9) in registers over the passes, in pass order
//   priors         element i of a block in lane i % 64 (the 63 / 45 / 10 / 3 long blocks take one pass)
//   mixture        per component lane i forms z_i = (P_m^T d)_i from COLUMN i of the table (the 64 lanes read one row at a time:
//                  coalesced), d broadcast lane by lane (v_readlane); d^T P_m d = d . z is a DPP sum; the minimum over the
//                  components is kept as the loop over m goes (first minimum).  (P_m d)_i, which reads row i per lane (stride 63
//                  floats), is formed for the winner only: the gradient is scale (P + P^T) d
//   reductions     wave_sum_dpp (wave_ops.h): fixed order, so a frame's bits depend on its own inputs only
// A keypoint whose weight is 0 is skipped as a whole: it adds +0 to every sum and its row of d joints is +0, whatever its
// coordinates hold.
#include "../../include/sfx.h"
#include "closure_math.h"

#define OBJ_WAVES 4
#define OBJ_MAX_K 512        // keypoints per frame (the shipped joint maps: 25 .. 144)
#define OBJ_MAX_M 32         // mixture components
#define OBJ_GMM_D 63         // the mixture acts on the 21 body joints' axis-angle values

struct ObjArgs {
    int B, K, n_prior, nb, ne;
    float rho, dw, bpw, sw, bend, hpw, epw, jaw[3];
    int use_conf, use_hands, use_face, form;
    int M; const float* mu; const float* prec; const float* nllw; const float* cconst;
    const float* joints; const float* R; const float* t; const float* fx; const float* fy; const float* center;
    const float* gt; const float* conf; const float* jw;
    const float* body_pose; const float* prior; const float* target; const float* betas; const float* expr;
    const float* jawp; const float* lh; const float* rh;
    float* loss;
    float* d_joints; float* d_R; float* d_t; float* d_body_pose; float* d_prior; float* d_betas; float* d_expr; float* d_jaw;
    float* d_lh; float* d_rh;
};

// the value of lane j (wave-uniform j) in every lane
__device__ __forceinline__ float obj_lane(float x, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}

// sum x^2 over a block of n values (lane-strided), gradient 2 x w2 written when asked for; `on` = 0: the term is switched off,
// its gradient block is zeros
__device__ __forceinline__ float obj_l2_block(const float* __restrict__ x, float* __restrict__ dx, int n, float w2, bool on, int lane) {
    float a = 0.f;
    for (int i = lane; i < n; i += 64) {
        float g = 0.f;
        if (on) { const float v = x[i]; a += v * v; g = 2.f * v * w2; }
        if (dx) dx[i] = g;
    }
    return a;
}

// The data term's share of one keypoint, common to both objectives: given dL/du, dL/dv (pixels) the gradient with respect to the
// camera-frame point, accumulated into d translation / d rotation, and R^T of it = d joint.
__device__ __forceinline__ void obj_pixel_adjoint(float du, float dv, float fx, float fy, float pcx, float pcy, float pcz,
                                                  const float* Rc, const float* p, float* aT, float* aR, float* dj) {
    const float dix = du * fx, diy = dv * fy;
    const float d0 = dix / pcz, d1 = diy / pcz, d2 = -(dix * pcx + diy * pcy) / (pcz * pcz);
    aT[0] += d0; aT[1] += d1; aT[2] += d2;
#pragma unroll
    for (int c = 0; c < 3; ++c) { aR[c] += d0 * p[c]; aR[3 + c] += d1 * p[c]; aR[6 + c] += d2 * p[c]; }
    dj[0] = Rc[0] * d0 + Rc[3] * d1 + Rc[6] * d2;
    dj[1] = Rc[1] * d0 + Rc[4] * d1 + Rc[7] * d2;
    dj[2] = Rc[2] * d0 + Rc[5] * d1 + Rc[8] * d2;
}

__device__ __forceinline__ void obj_store_camera_grads(float* d_R, float* d_t, int b, const float* aT, const float* aR, float extra_tz,
                                                       int lane) {
    // (sums in every lane after the DPP reduction; lane 0 stores)
    float sT[3], sR[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) sT[i] = wave_sum_dpp(aT[i]);
#pragma unroll
    for (int i = 0; i < 9; ++i) sR[i] = wave_sum_dpp(aR[i]);
    if (lane == 0) {
        if (d_t) { d_t[b * 3 + 0] = sT[0]; d_t[b * 3 + 1] = sT[1]; d_t[b * 3 + 2] = sT[2] + extra_tz; }
        if (d_R) {
#pragma unroll
            for (int i = 0; i < 9; ++i) d_R[b * 9 + i] = sR[i];
        }
    }
}

__global__ __launch_bounds__(64 * OBJ_WAVES)
void k_objective(const ObjArgs A) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * OBJ_WAVES + (threadIdx.x >> 6);
    if (b >= A.B) return;        // (the whole wavefront leaves: every DPP sum below runs with 64 active lanes)
    const int K = A.K;
    float Rc[9], ct[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rc[i] = A.R[b * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) ct[i] = A.t[b * 3 + i];
    const float fx = A.fx[b], fy = A.fy[b], cx = A.center[b * 2], cy = A.center[b * 2 + 1];
    const float rho2 = A.rho * A.rho, dw2 = A.dw * A.dw;

    // ---- data term (fitting.py:378-388) -------------------------------------------------------------------------------
    float aL = 0.f, aT[3] = {0.f, 0.f, 0.f}, aR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = lane; k < K; k += 64) {
        const size_t bk = (size_t)b * K + k;
        float w = A.jw[bk];
        if (A.use_conf) w *= A.conf[bk];
        const float w2 = w * w;
        float dj[3] = {0.f, 0.f, 0.f};
        if (w2 != 0.f) {
            const float p[3] = {A.joints[bk * 3], A.joints[bk * 3 + 1], A.joints[bk * 3 + 2]};
            const fwd_t pd[3] = {(fwd_t)p[0], (fwd_t)p[1], (fwd_t)p[2]};
            float pcx, pcy, pcz, rx, ry;
            project_residual<float, float>(pd, Rc, ct, fx, fy, cx, cy, A.gt[bk * 2], A.gt[bk * 2 + 1], pcx, pcy, pcz, rx, ry);
            const float sx = rx * rx, sy = ry * ry;
            const float gmx = rho2 * (sx / (sx + rho2)), gmy = rho2 * (sy / (sy + rho2));      // utils.py:84-95
            aL += w2 * gmx + w2 * gmy;
            const float du = -(w2 * dw2) * gmof_grad(rx, rho2), dv = -(w2 * dw2) * gmof_grad(ry, rho2);
            obj_pixel_adjoint(du, dv, fx, fy, pcx, pcy, pcz, Rc, p, aT, aR, dj);
        }
        if (A.d_joints) { A.d_joints[bk * 3] = dj[0]; A.d_joints[bk * 3 + 1] = dj[1]; A.d_joints[bk * 3 + 2] = dj[2]; }
    }

    // ---- pose prior (fitting.py:390-401) --------------------------------------------------------------------------------
    const float bpw2 = A.bpw * A.bpw;
    float aPP = 0.f;
    if (A.form == SFX_PRIOR_MIXTURE) {
        // MaxMixturePrior (prior.py:186-201 merged, :203-225 per component) on the operand x [63]:
        //   merged         min_m [ 0.5 d_m^T P_m d_m - log w_m ]
        //   per component  m* = argmin_m [ d_m^T P_m d_m + c_m ],  value(m*) - log w_m*
        // with the tables as the module holds them (P_m not symmetrised: the gradient is scale (P_m + P_m^T) d_m)
        const float scale = A.cconst ? 1.f : 0.5f;
        const bool in = lane < OBJ_GMM_D;
        const float x = in ? A.prior[(size_t)b * OBJ_GMM_D + lane] : 0.f;
        float best = 0.f, best_z = 0.f, best_d = 0.f, best_add = 0.f;
        int best_m = 0;
        for (int m = 0; m < A.M; ++m) {
            const float d = in ? x - A.mu[m * OBJ_GMM_D + lane] : 0.f;
            const float* __restrict__ P = A.prec + (size_t)m * OBJ_GMM_D * OBJ_GMM_D;
            float z = 0.f;
            for (int j = 0; j < OBJ_GMM_D; ++j) {
                const float dj = obj_lane(d, j);
                if (in) z += P[j * OBJ_GMM_D + lane] * dj;
            }
            const float quad = wave_sum_dpp(d * z);
            const float nlw = -logf(A.nllw[m]);
            const float sel = scale * quad + (A.cconst ? A.cconst[m] : nlw);
            if (m == 0 || sel < best) { best = sel; best_m = m; best_z = z; best_d = d; best_add = A.cconst ? nlw : 0.f; }
        }
        if (lane == 0) aPP = best + best_add;
        if (A.d_prior) {
            const float* __restrict__ P = A.prec + (size_t)best_m * OBJ_GMM_D * OBJ_GMM_D;
            float y = 0.f;
            for (int j = 0; j < OBJ_GMM_D; ++j) {
                const float dj = obj_lane(best_d, j);
                if (in) y += P[lane * OBJ_GMM_D + j] * dj;
            }
            if (in) A.d_prior[(size_t)b * OBJ_GMM_D + lane] = scale * (y + best_z) * bpw2;
        }
    } else {
        const bool to_target = A.form == SFX_PRIOR_L2_TARGET;
        for (int i = lane; i < A.n_prior; i += 64) {
            const size_t bi = (size_t)b * A.n_prior + i;
            const float e = A.prior[bi];
            const float dlt = to_target ? e - A.target[bi] : e;
            aPP += dlt * dlt;
            if (A.d_prior) A.d_prior[bi] = 2.f * dlt * bpw2;
        }
    }

    // ---- the other priors (fitting.py:403-435) ----------------------------------------------------------------------
    const float sw2 = A.sw * A.sw, h2 = A.hpw * A.hpw, e2 = A.epw * A.epw;
    const float aSH = obj_l2_block(A.betas + (size_t)b * A.nb, A.d_betas ? A.d_betas + (size_t)b * A.nb : nullptr, A.nb, sw2, true, lane);
    float aANG = 0.f;
    if (lane < 63) {        // SMPLifyAnglePrior (prior.py:73-89): exp(pose[idx] * sign)^2 on the elbows and knees, idx - 3 of :61
        const float sg = (lane == 52) ? 1.f : (lane == 55 || lane == 9 || lane == 12) ? -1.f : 0.f;
        float g = 0.f;
        if (sg != 0.f) {
            const float e = expf(A.body_pose[(size_t)b * 63 + lane] * sg);
            aANG = e * e;
            g = 2.f * (e * e) * sg * A.bend;
        }
        if (A.d_body_pose) A.d_body_pose[(size_t)b * 63 + lane] = g;
    }
    const bool hands = A.use_hands != 0, face = A.use_face != 0;
    const float aLH = obj_l2_block(hands ? A.lh + (size_t)b * 45 : nullptr, A.d_lh ? A.d_lh + (size_t)b * 45 : nullptr, 45, h2, hands, lane);
    const float aRH = obj_l2_block(hands ? A.rh + (size_t)b * 45 : nullptr, A.d_rh ? A.d_rh + (size_t)b * 45 : nullptr, 45, h2, hands, lane);
    const float aEX = obj_l2_block(face ? A.expr + (size_t)b * A.ne : nullptr, A.d_expr ? A.d_expr + (size_t)b * A.ne : nullptr, A.ne, e2, face, lane);
    float aJW = 0.f;
    if (lane < 3) {
        float g = 0.f;
        if (face) {
            const float jwt = (lane == 0) ? A.jaw[0] : (lane == 1) ? A.jaw[1] : A.jaw[2];
            const float jv = A.jawp[b * 3 + lane] * jwt;       // jaw_pose.mul(jaw_prior_weight) (:434-435)
            aJW = jv * jv; g = 2.f * jv * jwt;
        }
        if (A.d_jaw) A.d_jaw[b * 3 + lane] = g;
    }

    // ---- reductions and the total, in the term order of fitting.py:457-460 ----------------------------------------------
    const float qL = wave_sum_dpp(aL), qPP = wave_sum_dpp(aPP), qSH = wave_sum_dpp(aSH), qANG = wave_sum_dpp(aANG);
    const float qJW = wave_sum_dpp(aJW), qEX = wave_sum_dpp(aEX), qLH = wave_sum_dpp(aLH), qRH = wave_sum_dpp(aRH);
    float total = qL * dw2 + qPP * bpw2 + qSH * sw2 + qANG * A.bend;
    if (face) total = total + qJW + qEX * e2;
    if (hands) total = total + qLH * h2 + qRH * h2;
    if (lane == 0) A.loss[b] = total;
    obj_store_camera_grads(A.d_R, A.d_t, b, aT, aR, 0.f, lane);
}

struct CamArgs {
    int B, K;
    float dw, depth_w; int use_conf;
    const float* joints; const float* R; const float* t; const float* fx; const float* fy; const float* center;
    const float* gt; const float* count; const float* conf; const float* est_tz;
    float* loss; float* d_joints; float* d_R; float* d_t;
};

__global__ __launch_bounds__(64 * OBJ_WAVES)
void k_camera_init(const CamArgs A) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * OBJ_WAVES + (threadIdx.x >> 6);
    if (b >= A.B) return;
    const int K = A.K;
    float Rc[9], ct[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rc[i] = A.R[b * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) ct[i] = A.t[b * 3 + i];
    const float fx = A.fx[b], fy = A.fy[b], cx = A.center[b * 2], cy = A.center[b * 2 + 1];
    const float dw2 = A.dw * A.dw;
    // use_conf (fitting.py:509-511): the double unsqueeze makes the term (sum_i conf_i^2) * (sum_j err_j) over the selected
    // keypoints -- every residual is weighted by the SUM of the squared confidences (oracle/objective.py:camera_init_loss)
    float csum = 1.f;
    if (A.use_conf) {
        float a = 0.f;
        for (int k = lane; k < K; k += 64) { const float c = A.conf[(size_t)b * K + k]; a += A.count[k] * (c * c); }
        csum = wave_sum_dpp(a);
    }
    float aL = 0.f, aT[3] = {0.f, 0.f, 0.f}, aR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = lane; k < K; k += 64) {
        const size_t bk = (size_t)b * K + k;
        const float n = A.count[k];        // times keypoint k appears in init_joints_idxs (index_select repeats it)
        float dj[3] = {0.f, 0.f, 0.f};
        if (n != 0.f) {
            const float p[3] = {A.joints[bk * 3], A.joints[bk * 3 + 1], A.joints[bk * 3 + 2]};
            const fwd_t pd[3] = {(fwd_t)p[0], (fwd_t)p[1], (fwd_t)p[2]};
            float pcx, pcy, pcz, rx, ry;
            project_residual<float, float>(pd, Rc, ct, fx, fy, cx, cy, A.gt[bk * 2], A.gt[bk * 2 + 1], pcx, pcy, pcz, rx, ry);
            aL += n * (rx * rx + ry * ry);
            const float s = n * csum * dw2;
            obj_pixel_adjoint(-2.f * rx * s, -2.f * ry * s, fx, fy, pcx, pcy, pcz, Rc, p, aT, aR, dj);
        }
        if (A.d_joints) { A.d_joints[bk * 3] = dj[0]; A.d_joints[bk * 3 + 1] = dj[1]; A.d_joints[bk * 3 + 2] = dj[2]; }
    }
    float joint = wave_sum_dpp(aL);
    if (A.use_conf) joint *= csum;
    joint *= dw2;
    float depth = 0.f, dtz = 0.f;
    if (A.depth_w > 0.f && A.est_tz) {        // fitting.py:515-519
        const float dz = ct[2] - A.est_tz[b], w2 = A.depth_w * A.depth_w;
        depth = w2 * (dz * dz); dtz = w2 * 2.f * dz;
    }
    if (lane == 0) A.loss[b] = joint + depth;
    obj_store_camera_grads(A.d_R, A.d_t, b, aT, aR, dtz, lane);
}

static int obj_check_shape(const char* fn, int B, int K) {
    if (B < 1) { sfx_set_error("%s: B = %d, at least 1 frame is needed", fn, B); return -1; }
    if (K < 1 || K > OBJ_MAX_K) { sfx_set_error("%s: K = %d keypoints, supported 1..%d", fn, K, OBJ_MAX_K); return -1; }
    return 0;
}

extern "C" int sfx_objective_eval(const sfx_objective_cfg* c, const sfx_objective_in* in, const sfx_objective_grads* g,
                                  float* loss_dev, void* stream) {
    if (!c || !in || !loss_dev) { sfx_set_error("sfx_objective_eval: null argument"); return -1; }
    if (int rc = obj_check_shape("sfx_objective_eval", in->B, in->K)) return rc;
    if (c->prior_form < SFX_PRIOR_L2_EMBEDDING || c->prior_form > SFX_PRIOR_MIXTURE) {
        sfx_set_error("sfx_objective_eval: pose-prior form %d (0 .. 3: SFX_PRIOR_*)", c->prior_form); return -1; }
    if (in->n_prior < 1 || in->num_betas < 0 || in->num_expr < 0) {
        sfx_set_error("sfx_objective_eval: block lengths n_prior = %d, num_betas = %d, num_expr = %d", in->n_prior, in->num_betas, in->num_expr);
        return -1; }
    if (c->prior_form == SFX_PRIOR_MIXTURE) {
        if (c->gmm_D != OBJ_GMM_D || in->n_prior != OBJ_GMM_D) {
            sfx_set_error("sfx_objective_eval: mixture dimension %d on an operand of %d values, supported: %d (the body pose)",
                          c->gmm_D, in->n_prior, OBJ_GMM_D); return -1; }
        if (c->gmm_M < 1 || c->gmm_M > OBJ_MAX_M) { sfx_set_error("sfx_objective_eval: %d mixture components, supported 1..%d", c->gmm_M, OBJ_MAX_M); return -1; }
        if (!c->gmm_means_dev || !c->gmm_precisions_dev || !c->gmm_nll_weights_dev) {
            sfx_set_error("sfx_objective_eval: the mixture form needs means, precisions and nll_weights"); return -1; }
    }
    if (!in->joints_dev || !in->cam_rot_dev || !in->cam_t_dev || !in->focal_x_dev || !in->focal_y_dev || !in->center_dev ||
        !in->gt_joints_dev || !in->joint_weights_dev || !in->body_pose_dev || !in->prior_dev || (in->num_betas > 0 && !in->betas_dev)) {
        sfx_set_error("sfx_objective_eval: a required input is NULL"); return -1; }
    if (c->use_joints_conf && !in->joints_conf_dev) { sfx_set_error("sfx_objective_eval: use_joints_conf without joints_conf"); return -1; }
    if (c->prior_form == SFX_PRIOR_L2_TARGET && !in->prior_target_dev) { sfx_set_error("sfx_objective_eval: the target form needs prior_target"); return -1; }
    if (c->use_hands && (!in->lhand_dev || !in->rhand_dev)) { sfx_set_error("sfx_objective_eval: use_hands without the hand poses"); return -1; }
    if (c->use_face && (!in->jaw_dev || (in->num_expr > 0 && !in->expression_dev))) { sfx_set_error("sfx_objective_eval: use_face without expression / jaw_pose"); return -1; }
    ObjArgs A{};
    A.B = in->B; A.K = in->K; A.n_prior = in->n_prior; A.nb = in->num_betas; A.ne = in->num_expr;
    A.rho = c->rho; A.dw = c->data_weight; A.bpw = c->body_pose_weight; A.sw = c->shape_weight; A.bend = c->bending_prior_weight;
    A.hpw = c->hand_prior_weight; A.epw = c->expr_prior_weight;
    for (int i = 0; i < 3; ++i) A.jaw[i] = c->jaw_prior_weight[i];
    A.use_conf = c->use_joints_conf ? 1 : 0; A.use_hands = c->use_hands ? 1 : 0; A.use_face = c->use_face ? 1 : 0; A.form = c->prior_form;
    A.M = c->gmm_M; A.mu = c->gmm_means_dev; A.prec = c->gmm_precisions_dev; A.nllw = c->gmm_nll_weights_dev; A.cconst = c->gmm_comp_const_dev;
    A.joints = in->joints_dev; A.R = in->cam_rot_dev; A.t = in->cam_t_dev; A.fx = in->focal_x_dev; A.fy = in->focal_y_dev;
    A.center = in->center_dev; A.gt = in->gt_joints_dev; A.conf = in->joints_conf_dev; A.jw = in->joint_weights_dev;
    A.body_pose = in->body_pose_dev; A.prior = in->prior_dev; A.target = in->prior_target_dev; A.betas = in->betas_dev;
    A.expr = in->expression_dev; A.jawp = in->jaw_dev; A.lh = in->lhand_dev; A.rh = in->rhand_dev;
    A.loss = loss_dev;
    if (g) {
        A.d_joints = g->d_joints_dev; A.d_R = g->d_cam_rot_dev; A.d_t = g->d_cam_t_dev; A.d_body_pose = g->d_body_pose_dev;
        A.d_prior = g->d_prior_dev; A.d_betas = g->d_betas_dev; A.d_expr = g->d_expression_dev; A.d_jaw = g->d_jaw_dev;
        A.d_lh = g->d_lhand_dev; A.d_rh = g->d_rhand_dev;
    }
    hipLaunchKernelGGL(k_objective, dim3((A.B + OBJ_WAVES - 1) / OBJ_WAVES), dim3(64 * OBJ_WAVES), 0, (hipStream_t)stream, A);
    SFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sfx_camera_init_eval(const sfx_camera_init_cfg* c, int32_t B, int32_t K,
                                    const float* joints_dev, const float* cam_rot_dev, const float* cam_t_dev,
                                    const float* focal_x_dev, const float* focal_y_dev, const float* center_dev,
                                    const float* gt_joints_dev, const float* init_count_dev, const float* joints_conf_dev,
                                    const float* est_tz_dev, float* loss_dev, float* d_joints_dev, float* d_cam_rot_dev,
                                    float* d_cam_t_dev, void* stream) {
    if (!c || !loss_dev) { sfx_set_error("sfx_camera_init_eval: null argument"); return -1; }
    if (int rc = obj_check_shape("sfx_camera_init_eval", B, K)) return rc;
    if (!joints_dev || !cam_rot_dev || !cam_t_dev || !focal_x_dev || !focal_y_dev || !center_dev || !gt_joints_dev || !init_count_dev) {
        sfx_set_error("sfx_camera_init_eval: a required input is NULL"); return -1; }
    if (c->use_conf && !joints_conf_dev) { sfx_set_error("sfx_camera_init_eval: use_conf without joints_conf"); return -1; }
    CamArgs A{};
    A.B = B; A.K = K; A.dw = c->data_weight; A.depth_w = c->depth_loss_weight; A.use_conf = c->use_conf ? 1 : 0;
    A.joints = joints_dev; A.R = cam_rot_dev; A.t = cam_t_dev; A.fx = focal_x_dev; A.fy = focal_y_dev; A.center = center_dev;
    A.gt = gt_joints_dev; A.count = init_count_dev; A.conf = joints_conf_dev; A.est_tz = est_tz_dev;
    A.loss = loss_dev; A.d_joints = d_joints_dev; A.d_R = d_cam_rot_dev; A.d_t = d_cam_t_dev;
    hipLaunchKernelGGL(k_camera_init, dim3((B + OBJ_WAVES - 1) / OBJ_WAVES), dim3(64 * OBJ_WAVES), 0, (hipStream_t)stream, A);
    SFX_CHECK(hipGetLastError());
    return 0;
}
