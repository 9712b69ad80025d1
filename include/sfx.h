/* sfx.h -- C ABI of libsfx.so, the MI355X (gfx950) SMPL-X fitting engine.
 *
 * The reference (xiyichen/smplify-x-partial) has no FFI seam: its hot path is a chain of
 * Python objects.  This header is the boundary the replacement defines
 * UNDER that Python surface; each entry point names the reference interface it stands
 * in for.  Plain pointers and sizes only -- no torch types.  Unless stated otherwise a
 * `const float*` / `const int32_t*` argument is a HOST pointer read during the call; a
 * `*_dev` argument is a DEVICE pointer (e.g. torch.Tensor.data_ptr()); `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  No ownership is transferred.
 * One model/batch handle per GPU; handles are thread-compatible, not thread-safe.
 * Every function returns 0 on success or a negative code; sfx_last_error() describes it.
 */
#ifndef SFX_H_
#define SFX_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfx_model sfx_model;   /* model constants resident in HBM            */
typedef struct sfx_batch sfx_batch;   /* B frames: parameters, data, optimiser state */

/* ---- model -------------------------------------------------------------------------
 * Replaces smplx.create(...) / smplx.SMPLX.__init__ (reference call site
 * smplifyx/main.py:109-127; file keys SURVEY.md appendix A.1).  Arrays use the .npz
 * layouts; the library re-lays them out for the GPU (k-major blend-shape matrix for the
 * dense MFMA GEMM, vertex-major copy for the needed-rows path, folded joint regressor). */
typedef struct sfx_model_desc {
    int32_t V, F, J;              /* 10475, 20908, 55                                  */
    int32_t num_betas, num_expr;  /* 10, 10                                            */
    int32_t num_pca;              /* hand PCA comps used (12); 0 = hands given as 45-D */
    const float*   v_template;    /* [V][3]                                            */
    const float*   shapedirs;     /* [V][3][num_betas+num_expr] (betas then expression)*/
    const float*   posedirs;      /* [V][3][9*(J-1)]                                   */
    const float*   J_regressor;   /* [J][V]                                            */
    const float*   lbs_weights;   /* [V][J]                                            */
    const int32_t* parents;       /* [J], parents[0] = -1                              */
    const float*   hands_comp_l;  /* [num_pca][45]                                     */
    const float*   hands_comp_r;  /* [num_pca][45]                                     */
    const float*   pose_mean;     /* [3*J]                                             */
    const int32_t* faces;         /* [F][3]                                            */
    int32_t        n_extra;       /* 21 vertex joints (VertexJointSelector)            */
    const int32_t* extra_vertex_ids;
    int32_t        n_lmk;         /* 51 static landmarks                               */
    const int32_t* lmk_faces_idx; /* [n_lmk]                                           */
    const float*   lmk_bary;      /* [n_lmk][3]                                        */
    int32_t        n_dyn_rows, n_dyn;  /* 79, 17 (0,0 = no face contour)               */
    const int32_t* dyn_lmk_faces_idx;  /* [n_dyn_rows][n_dyn]                          */
    const float*   dyn_lmk_bary;       /* [n_dyn_rows][n_dyn][3]                       */
    int32_t        K;             /* joints after joint_mapper                         */
    const int32_t* joint_map;     /* [K] indices into the 55+n_extra+n_lmk+n_dyn list
                                     (utils.JointMapper, smplifyx/utils.py:68-81)      */
} sfx_model_desc;

int  sfx_model_create(const sfx_model_desc* desc, sfx_model** out);
/* Releases the model's constants, the batch behind sfx_lbs_forward and the ONE collision handle the model retains (see
 * sfx_batch_destroy).  Destroy the model's batches first.                                */
void sfx_model_destroy(sfx_model* m);

/* VPoser-v1 decoder weights (human_body_prior cvpr19; reference call sites
 * fit_single_frame.py:241-245, fitting.py:236-238): fc1 [H][L], fc2 [H][H], out [126][H]. */
int  sfx_model_set_vposer(sfx_model* m, int32_t latent, int32_t hidden,
                          const float* fc1_w, const float* fc1_b,
                          const float* fc2_w, const float* fc2_b,
                          const float* out_w, const float* out_b);

/* ---- stand-alone VPoser decoder ---------------------------------------------------------
 * Replaces `vposer.decode(pose_embedding, output_type='aa')` of human_body_prior (cvpr19) wherever the reference calls it
 * outside the fitting closure (fitting.py:72,197,236, fit_single_frame.py:265,515,607,620,654, render_pkl.py:97) and what
 * autograd walks behind it, for B latents at once.  The handle is independent of any sfx_model, as the reference's `vposer`
 * is independent of `body_model`.  Weights are HOST pointers in the layouts of sfx_model_set_vposer and are refused like
 * there (hidden 512, latent a multiple of 4 and <= 60), before any device memory is touched.  decode / decode_backward take
 * DEVICE pointers to contiguous fp32 and only ENQUEUE on `stream`: they do not synchronise, allocate nothing and use no
 * scratch; B = 0 returns 0 without a launch.  decode_backward is stateless: it takes z again and re-evaluates the forward;
 * dz = d sum(dbody * body_pose) / d z.  A frame's result depends on its own latent only, bit for bit (not on B or its
 * position in the batch).                                                                  */
typedef struct sfx_vposer sfx_vposer;
int  sfx_vposer_create(int32_t latent, int32_t hidden,
                       const float* fc1_w, const float* fc1_b,
                       const float* fc2_w, const float* fc2_b,
                       const float* out_w, const float* out_b, sfx_vposer** out);
void sfx_vposer_destroy(sfx_vposer* v);
int  sfx_vposer_decode(sfx_vposer* v, int32_t B, const float* z_dev /* [B][latent] */,
                       float* body_pose_dev /* [B][63] */, void* stream);
int  sfx_vposer_decode_backward(sfx_vposer* v, int32_t B, const float* z_dev /* [B][latent] */,
                                const float* dbody_dev /* [B][63] */, float* dz_dev /* [B][latent] */, void* stream);

/* ---- stand-alone VPoser encoder ---------------------------------------------------------
 * Replaces `vposer.encode(full_pose_prior)` of human_body_prior (cvpr19; reference call site fit_single_frame.py:245: the
 * Normal the starting latent is sampled from) for B poses at once, with its backward: the pose prior
 * `vposer.encode(body_pose).mean.pow(2).sum()` of code that optimises the pose itself, and the manifold projection
 * decode(encode(p).mean).  A handle of its own -- a checkpoint may carry no encoder, and sfx_vposer stays as it is.
 * Weights are HOST pointers in the checkpoint's layouts ([out][in]): bn1 / bn2 [n_in] / [hidden] (weight, bias, running_mean,
 * running_var), fc1 [hidden][n_in], fc2 [hidden][hidden], mu and logvar [latent][hidden].  Eval-mode batch norm (eps 1e-5) is
 * folded into the linear layer behind it, in double.  n_in = 63: the first layer takes the axis-angle pose; n_in = 189: the
 * row-major rotation matrices of the 21 joints (plain Rodrigues, first-order below 1e-6 rad).  Refused before any device
 * memory is touched (-1): hidden != 512, latent not a multiple of 4 in 4 .. 60, n_in not 63 or 189, running_var + 1e-5 <= 0
 * or a non-finite value in a batch-norm table; -3: no HIP device; -2: out of device memory.
 * encode / encode_backward take DEVICE pointers to contiguous fp32 and only ENQUEUE on `stream`: they do not synchronise,
 * allocate nothing and use no global scratch (B = 0: nothing is launched).  mean = mu, sigma = softplus(logvar): the two
 * parameters of the Normal.  encode_backward is stateless (the forward is re-evaluated at pose_dev):
 * dpose = d (sum(dmean * mean) + sum(dsigma * sigma)) / d pose; one of dmean / dsigma may be NULL (= zeros), both NULL is
 * refused.  A frame's result depends on its own pose only, bit for bit (not on B or its position in the batch).  */
typedef struct sfx_vposer_encoder sfx_vposer_encoder;
int  sfx_vposer_encoder_create(int32_t latent, int32_t hidden, int32_t n_in,
                               const float* bn1_w, const float* bn1_b, const float* bn1_mean, const float* bn1_var,
                               const float* fc1_w, const float* fc1_b,
                               const float* bn2_w, const float* bn2_b, const float* bn2_mean, const float* bn2_var,
                               const float* fc2_w, const float* fc2_b,
                               const float* mu_w, const float* mu_b, const float* logvar_w, const float* logvar_b,
                               sfx_vposer_encoder** out);
void sfx_vposer_encoder_destroy(sfx_vposer_encoder* e);
int  sfx_vposer_encode(sfx_vposer_encoder* e, int32_t B, const float* pose_dev /* [B][63] */,
                       float* mean_dev /* [B][latent] */, float* sigma_dev /* [B][latent], may be NULL */, void* stream);
int  sfx_vposer_encode_backward(sfx_vposer_encoder* e, int32_t B, const float* pose_dev /* [B][63] */,
                                const float* dmean_dev /* [B][latent], may be NULL */,
                                const float* dsigma_dev /* [B][latent], may be NULL */,
                                float* dpose_dev /* [B][63] */, void* stream);

/* ---- stand-alone LBS forward ----------------------------------------------------------
 * Replaces body_model(return_verts=True, body_pose=..., return_full_pose=True)
 * (fitting.py:82,248; fit_single_frame.py:611).  All pointers are DEVICE pointers to
 * contiguous fp32; any output may be NULL.  `hands` are PCA coefficients [B][num_pca]. */
/* Per-face part labels of smplx_parts_segm.pkl and the part pairs that never collide
 * (fit_single_frame.py:316-328): used by batches created with interpenetration = 1.  segm /
 * parents [F]; ign_pairs [n_ign][2].  Without this call -- or after one with segm = parents = NULL,
 * which clears the labels -- no pair is filtered by part.                                      */
int  sfx_model_set_parts(sfx_model* m, const int32_t* segm, const int32_t* parents, const int32_t* ign_pairs,
                         int32_t n_ign);

int  sfx_lbs_forward(sfx_model* m, int32_t B,
                     const float* global_orient_dev,   /* [B][3]  */
                     const float* body_pose_dev,       /* [B][63] */
                     const float* betas_dev,           /* [B][num_betas] */
                     const float* expression_dev,      /* [B][num_expr]  */
                     const float* jaw_dev, const float* leye_dev, const float* reye_dev, /* [B][3] */
                     const float* lhand_dev, const float* rhand_dev,   /* [B][num_pca] */
                     float* vertices_out_dev,          /* [B][V][3]  or NULL */
                     float* joints_out_dev,            /* [B][K][3]  or NULL */
                     float* full_pose_out_dev,         /* [B][3J]    or NULL */
                     void* stream);

/* ---- backward pass of the stand-alone LBS ------------------------------------------------
 * Replaces autograd through smplx.SMPLX.forward / smplx.lbs.lbs (what `loss.backward()` walks in any
 * objective written on body_model(...).vertices / .joints): the gradient of
 *     sum(dvertices * vertices) + sum(djoints * joints)
 * with respect to the nine inputs of sfx_lbs_forward, for B meshes at once.  All pointers are DEVICE
 * pointers to contiguous fp32.  The call is stateless: it takes the nine inputs again and re-evaluates
 * the forward at them (the price of a vertex gradient is one more dense GEMM than a backward that kept
 * state would run), so nothing depends on which sfx_lbs_forward came before.  Either upstream may be
 * NULL (= zero); both NULL is an error (-1).  With dvertices NULL no GEMM runs in either direction.
 * Any output may be NULL.  The buffers of this path are allocated by its first call (-2: out of device
 * memory; the model keeps serving sfx_lbs_forward).  No gradient flows through the dynamic-contour
 * look-up (as in the reference); fp32 arithmetic, keypoint forward in fp64 as everywhere in the library. */
int  sfx_lbs_backward(sfx_model* m, int32_t B,
                      const float* global_orient_dev, const float* body_pose_dev, const float* betas_dev,
                      const float* expression_dev, const float* jaw_dev, const float* leye_dev, const float* reye_dev,
                      const float* lhand_dev, const float* rhand_dev,           /* as sfx_lbs_forward */
                      const float* dvertices_dev,       /* [B][V][3] or NULL */
                      const float* djoints_dev,         /* [B][K][3] or NULL */
                      float* d_global_orient_dev, float* d_body_pose_dev, float* d_betas_dev, float* d_expression_dev,
                      float* d_jaw_dev, float* d_leye_dev, float* d_reye_dev, float* d_lhand_dev, float* d_rhand_dev,
                      void* stream);

/* ---- a batch of independent frames -------------------------------------------------------
 * Replaces, for B frames at once, the objects fit_single_frame() wires together
 * (fit_single_frame.py:413-445: create_loss('camera_init'), create_loss('smplify'),
 * FittingMonitor, optim_factory.create_optimizer('lbfgsls')).                            */
typedef struct sfx_stage_weights {      /* one entry of opt_weights (fit_single_frame.py:330-353) */
    float body_pose_weight, shape_weight;
    float hand_prior_weight, expr_prior_weight;
    float jaw_prior_weight[3];
    float hand_joint_weight, face_joint_weight;   /* joint_weights slices (:569-572)    */
    float coll_loss_weight;                       /* coll_loss_weights[stage]; used when interpenetration = 1 */
    float bending_prior_weight;                   /* < 0: derive 3.17 * body_pose_weight (:567-568) */
} sfx_stage_weights;

typedef struct sfx_stage_weights_f64 {  /* the same fields in double: float64 batches (high_precision = 2), whose reference
                                           run carries weights like 57.4 unrounded and forms 3.17 * body_pose_weight in double */
    double body_pose_weight, shape_weight;
    double hand_prior_weight, expr_prior_weight;
    double jaw_prior_weight[3];
    double hand_joint_weight, face_joint_weight;
    double coll_loss_weight;                      /* (no interpenetration term in float64 mode: ignored) */
    double bending_prior_weight;                  /* < 0: derive 3.17 * body_pose_weight in double */
} sfx_stage_weights_f64;

typedef struct sfx_batch_cfg {
    int32_t B;
    int32_t n_stages;               /* body stages (3 or 5)                              */
    int32_t use_vposer;             /* pose_embedding = VPoser latent [32]                */
    int32_t use_hands, use_face;    /* SMPLifyLoss flags (fitting.py:331-339)             */
    int32_t use_joints_conf;        /* weights = joint_weights * conf (fitting.py:380)    */
    int32_t has_regression_pose;    /* pprior = |emb - regression_pose|^2 (:391-397)      */
    int32_t use_conf_cam_init;      /* use_conf quirk of camera-init loss (:509-511)      */
    int32_t num_body_joints;        /* 25 / 26 / 23: start of the hand keypoints          */
    int32_t maxiters;               /* run_fitting steps, and LBFGS max_iter unless lbfgs_max_iter says otherwise (cfg: 30) */
    double  ftol, gtol;             /* run_fitting tolerances (cfg: 1e-9, 1e-9)           */
    float   lr;                     /* cfg: 1.0                                           */
    float   rho;                    /* GMoF rho (cfg: 100)                                */
    float   depth_loss_weight;      /* camera-init depth term (default 1e2)               */
    int32_t lbs_mode;               /* 0: needed-rows LBS in the loop; 1: dense V-vertex
                                       LBS every closure (what the reference evaluates)   */
    int32_t reuse_entry_eval;       /* 1: serve LBFGS.step's entry evaluation from the
                                       value already computed at the same point           */
    float   side_view_thsh;         /* > 0: frames whose 2-D shoulder distance is below it are
                                       fitted twice (orientation flipped by pi about y) and the
                                       lower final loss kept (fit_single_frame.py:461-463,
                                       527-551,662-667); needs a fit over stages -1..n-1     */
    int32_t left_shoulder_idx, right_shoulder_idx;
    int32_t interpenetration;       /* 1: penetration term in the stages with coll_loss_weight > 0
                                       (fitting.py:437-455); needs lbs_mode 1 (all vertices)      */
    int32_t max_collisions;         /* partners kept per triangle (cfg: 8 / 128)                   */
    float   df_cone_height;         /* sigma of the cone distance field (cfg: 0.5 / 1e-4)          */
    int32_t penalize_outside;
    int32_t slots;                  /* dense mode: GEMM columns (frames resident in the fit loop at a time);
                                       0 or >= B: every frame has a column.  With slots < B the frames beyond
                                       the first `slots` wait in a queue and take over the columns of frames
                                       that finish (continuous batching): the reference's loop over frames
                                       (main.py:207) for jobs larger than one GEMM batch.  A frame's result does
                                       not depend on when it is admitted or which column it gets              */
    /* hyper-parameters of optimizers/lbfgs_ls.py's LBFGS that optim_factory.py:27-65 leaves at their defaults.  The two
       tolerances: NEGATIVE = default, 0 is passed through (legal in the reference: the test is disabled); the counts: 0 = default */
    double  lbfgs_tolerance_grad;   /* 1e-5                                                          */
    double  lbfgs_tolerance_change; /* 1e-9                                                          */
    int32_t lbfgs_max_eval;         /* maxiters * 5 / 4                                              */
    int32_t lbfgs_history_size;     /* 100; up to 400 (a larger history gets a ring of that many slots) */
    int32_t lbfgs_max_iter;         /* LBFGS(max_iter): iterations per LBFGS.step and bound of the zoom phase (lbfgs_ls.py:304,397);
                                       0 = maxiters, the one value optim_factory.py:15 hands to both; lbfgs_max_eval's default
                                       follows it (max_iter * 5 / 4, lbfgs_ls.py:203)                              */
    int32_t high_precision;         /* cfg float_dtype: float64 (main.py:99-105): besides the keypoint forward (always fp64) the
                                       projection up to the pixel residual is carried in fp64 in every stage -- gradient noise
                                       0.13 x torch fp32's, the fits behave like the reference's float64 run (LAB_NOTES.md §3.1);
                                       parameters, reverse sweep and optimiser stay fp32.
                                       Any nonzero value other than 2 selects this mode.
                                       2: the closure in float64 (the arithmetic of the reference's float_dtype: float64 run):
                                       parameters, rotations, blend-shape sums, projection, losses and the whole reverse
                                       sweep in double (model tables stay fp32: widening them is exact).  Body-only needed-rows
                                       batches: lbs_mode 0 without use_vposer, use_hands, use_face, interpenetration or the GMM
                                       prior (refused by sfx_batch_create / sfx_batch_set_gmm).  The batch is driven through the
                                       _f64 entry points below; float inputs (set_frames, set_params) are widened, float
                                       outputs are refused, and the device optimiser (fit, step, guess_init, stats, trace) and
                                       sfx_batch_forward are not available in this mode                             */
    int32_t point2plane;            /* DistanceFieldPenetrationLoss(point2plane=True) (cmd_parser.py:239): see
                                       sfx_pen_set_point2plane                                                     */
} sfx_batch_cfg;

/* Device memory of note: a dense batch without the interpenetration term keeps several sets of GEMM operand buffers for its
 * overlapped fitting loop, 4.7 KB per frame and set -- three sets in all; seventeen (21 MB at 256 frames, 82 MB at 1 024) where the
 * multi-round form of the loop can run: body-only keypoints without the VPoser decoder.                                     */
int  sfx_batch_create(sfx_model* m, const sfx_batch_cfg* cfg,
                      const sfx_stage_weights* stages /* [n_stages] */, sfx_batch** out);
/* Releases everything the batch owns, EXCEPT the collision buffers of a batch with interpenetration = 1 (about 45 MB per GEMM
 * column: 11.5 GB at 256): they go back to the model, which retains one such handle (the largest returned) for its next batch
 * until sfx_model_set_parts or sfx_model_destroy.  No other entry point releases that memory.                          */
void sfx_batch_destroy(sfx_batch* b);

/* Per-frame inputs (HOST pointers, copied):
 *  keypoints   [B][K][3]  x, y, confidence                (fit_single_frame.py:276-284)
 *  joint_weights [B][K]   after joints_to_ign and low-confidence zeroing (:285-287,574)
 *  cam_init_mask [B][K]   1 for the trimmed init_joints_idxs (:289-294)
 *  camera      [B][6]     focal_x, focal_y, center_x, center_y, data_weight(=1000/H), est_tz
 *  cam_rot     [B][9]     camera rotation (row-major; identity in the reference)
 */
int  sfx_batch_set_frames(sfx_batch* b, const float* keypoints, const float* joint_weights,
                          const float* cam_init_mask, const float* camera, const float* cam_rot);

/* Parameters (HOST pointers).  Names = the reference's result-pkl keys
 * (fit_single_frame.py:644-657).  `pose_embedding` is [B][63] or [B][latent];
 * `regression_pose` (may be NULL) is the clone taken at fit_single_frame.py:442.          */
int  sfx_batch_set_params(sfx_batch* b, const float* cam_translation, const float* global_orient,
                          const float* betas, const float* lhand, const float* rhand,
                          const float* expression, const float* jaw, const float* leye,
                          const float* reye, const float* pose_embedding,
                          const float* regression_pose);
int  sfx_batch_get_params(sfx_batch* b, float* cam_translation, float* global_orient,
                          float* betas, float* lhand, float* rhand, float* expression,
                          float* jaw, float* leye, float* reye, float* pose_embedding,
                          float* body_pose /* [B][63] decoded body pose */);

/* One closure evaluation for every frame at the CURRENT parameters (fitting.py:232-273:
 * forward + loss + adjoint).  stage = -1: camera-init loss over [cam_t, global_orient]
 * (N=6); stage >= 0: SMPLifyLoss with that stage's weights over the body variable vector
 * (order of body_model.parameters() + pose_embedding, N = sfx_batch_num_vars).
 * loss_out [B], grad_out [B][N]: HOST pointers (either may be NULL).                      */
int  sfx_batch_num_vars(sfx_batch* b, int32_t stage);
int  sfx_batch_closure(sfx_batch* b, int32_t stage, float* loss_out, float* grad_out, void* stream);

/* Camera translation guess of fitting.guess_init (fitting.py:36-110) for every frame:
 * one LBS forward, t_z = f * mean|d3D| / mean|d2D| over `n_pairs` keypoint pairs.
 * Writes cam_translation = (0,0,t_z) and est_tz.                                           */
int  sfx_batch_guess_init(sfx_batch* b, const int32_t* pairs /* [n_pairs][2] */, int32_t n_pairs,
                          void* stream);

/* The whole per-frame schedule of fit_single_frame.py:447-612 for all frames, on device:
 * camera stage, then n_stages body stages, each = FittingMonitor.run_fitting
 * (fitting.py:147-217) driving LBFGS.step with strong-Wolfe line search
 * (optimizers/lbfgs_ls.py:39-167,256-445).  first_stage/last_stage select a sub-range
 * (-1 = camera stage).  Blocks until done.                                                */
int  sfx_batch_fit(sfx_batch* b, int32_t first_stage, int32_t last_stage, void* stream);

/* ONE optimizer.step(closure) of LBFGS('lbfgsls') for every frame (lbfgs_ls.py:256-445), for
 * callers that drive run_fitting's outer loop themselves.  resume = 0 starts a fresh optimiser
 * (new stage), 1 continues the previous one (history kept).  loss_out [B] (HOST) receives what
 * step() returns: the loss at entry.                                                        */
int  sfx_batch_step(sfx_batch* b, int32_t stage, int32_t resume, float* loss_out, void* stream);

/* Gradient of the most recent closure evaluation of every frame, grad_out [B][num_vars(stage)]
 * (HOST): what `var.grad` holds after optimizer.step() in the reference, which run_fitting's
 * gtol test reads (fitting.py:191-193).                                                       */
int  sfx_batch_get_grad(sfx_batch* b, int32_t stage, float* grad_out);

/* Interpenetration diagnostics of the most recent evaluation (batches with interpenetration = 1),
 * per active GEMM column: stats as sfx_pen_stats; ext_n = vertices that carried a gradient.    */
int  sfx_batch_pen_stats(sfx_batch* b, int32_t* stats_host /* [B][4] */, int32_t* ext_n_host /* [B] or NULL */);
/* Per FRAME, sticky since the start of the last fit / step (HOST [B]): 1 = the frame consumed a collision evaluation in which
 * a bucket walk was cut short (a mesh folded into a few grid cells) -- pairs beyond the cut are missing and which ones depends
 * on arrival order (the package's BVH is traversal-order dependent in the same situation, fitting.py:445-447), so this frame's
 * result is not reproducible run to run.  0 on any sane mesh.  (A triangle with more than 2 x max_collisions partners is no
 * such case since round 4: its kept partners -- the lowest ids -- are derived from the grid again; with max_collisions > 1024,
 * or in a mesh with more than 4096 such triangles -- one that has collapsed onto itself -- it still is.)                                                                                                              */
int  sfx_batch_pen_flags(sfx_batch* b, int32_t* flags_host);
/* Kernel launches of ONE interpenetration step of the fitting loop (broad phase ... adjoint), counted on the graph the batch
 * captured for it most recently; 0 before the first fit with the term (measurement: bench.py roofline_pen.launches_per_round). */
int  sfx_batch_pen_launches(sfx_batch* b);
/* sfx_pen_pairs for GEMM column `column` of the batch's most recent evaluation (resident batches only). */
int  sfx_batch_pen_pairs(sfx_batch* b, int32_t column, int32_t cap, int32_t* pairs_host, int32_t* n_out);

/* Per-frame results of the last sfx_batch_fit (HOST pointers, any may be NULL):
 *  stage_loss [B][1+n_stages]  value run_fitting returns per stage (camera first)
 *  stage_evals [B][1+n_stages] closure evaluations performed per stage
 *  stage_ref_evals             evaluations the reference would have performed            */
int  sfx_batch_get_stats(sfx_batch* b, float* stage_loss, int32_t* stage_evals,
                         int32_t* stage_ref_evals);

/* Optimiser trace (tests of step-level parity with smplifyx/optimizers/lbfgs_ls.py:256-445 and
 * smplifyx/fitting.py:147-217): capacity > 0 attaches a buffer of `capacity` records per frame that every
 * later sfx_batch_fit / sfx_batch_step fills, capacity = 0 detaches it.  A record is 4 floats:
 *   (0, t, loss, ls_evals)                 a line search ended: accepted step length, loss there, its evaluations
 *   (1, entry loss, func_evals, n_iter)    one LBFGS.step returned (cumulative evaluations / iterations of the stage)
 *   (2, result, closure evaluations, stage) run_fitting returned for a stage (camera stage = -1)
 *   (3, trial step, loss, |gradient|inf)   (only with a NEGATIVE capacity, |capacity| records) every closure evaluation
 * sfx_batch_get_trace: records [B][capacity][4] and the number written per frame (HOST; counts may exceed capacity). */
int  sfx_batch_trace(sfx_batch* b, int32_t capacity);
int  sfx_batch_get_trace(sfx_batch* b, float* records, int32_t* counts);

/* ---- the optimiser for evaluations the CALLER supplies (csrc/opt_ext.hip) ----------------------------------
 * B independent problems of N <= 192 float32 variables each, advanced by the state machine of sfx_batch_fit / sfx_batch_step
 * (one wavefront per problem, one evaluation per launch), in reverse communication: the handle says where it wants each problem
 * evaluated, the caller evaluates loss and gradient there by any means (a torch loss and autograd, say) and hands them back.
 * No problem waits for a decision of another one, and nothing but sfx_opt_active synchronises.
 * Replaces FittingMonitor.run_fitting (smplifyx/fitting.py:147-217) over LBFGS(line_search_fn='strong_Wolfe').step
 * (smplifyx/optimizers/lbfgs_ls.py:256-445, _strong_Wolfe / _cubic_interpolate :11-167) for an arbitrary closure.          */
typedef struct sfx_opt sfx_opt;
typedef struct sfx_opt_cfg {
    int32_t B, N;
    int32_t n_groups; int32_t group_len[12];   /* the tensors of `params`: run_fitting's gtol test is per tensor
                                                  (fitting.py:191, abs(grad.max()) < gtol); 0 groups = one group of N */
    int32_t maxiters; double ftol, gtol;       /* run_fitting (fitting.py:147-217); maxiters >= 1 */
    float   lr;
    double  tolerance_grad, tolerance_change;  /* negative = default 1e-5 / 1e-9; 0 is passed through */
    int32_t max_iter, max_eval, history_size;  /* 0 = defaults, as in sfx_batch_cfg: maxiters, max_iter * 5 / 4, 100 */
    int32_t reuse_entry_eval;                  /* as sfx_batch_cfg.reuse_entry_eval (mode 0) */
} sfx_opt_cfg;
/* The optimiser object of optim_factory.py:50-52 and the monitor's tolerances, for B problems.  Refused before any device memory
 * is touched (-1): N outside 1..192, B < 1, more than 12 groups, group lengths that do not sum to N, history_size outside
 * 0..400.  -3: no HIP device.  -2: out of device memory (nothing stays allocated).                                       */
int  sfx_opt_create(const sfx_opt_cfg* cfg, sfx_opt** out);
void sfx_opt_destroy(sfx_opt* h);
/* Start a run.  mode 0: the whole run_fitting loop (fitting.py:174-217); mode 1: ONE LBFGS.step (lbfgs_ls.py:256-445) --
 * resume = 1 continues the optimiser of the previous mode-1 run (history and counters kept, as sfx_batch_step), 0 starts a
 * fresh one (lbfgs_ls.py:293-300) and empties the trace.  Copies x0_dev [B][N] (DEVICE) in and writes the first point to
 * evaluate to x_trial_dev [B][N] (DEVICE).  Enqueues only.                                                                */
int  sfx_opt_begin(sfx_opt* h, int32_t mode, int32_t resume, const float* x0_dev, float* x_trial_dev, void* stream);
/* closure() of lbfgs_ls.py:279, :67 and :134, turned inside out: consume loss_dev [B] and grad_dev [B][N] (DEVICE, packed),
 * evaluated at the current trial points, and write the next ones to x_trial_dev.  A problem that has finished is left alone:
 * its loss and gradient are not read, its row of x_trial_dev -- its accepted point -- is not written.  Enqueues only,
 * allocates nothing.                                                                                                     */
int  sfx_opt_tell(sfx_opt* h, const float* loss_dev, const float* grad_dev, float* x_trial_dev, void* stream);
/* Problems still running (HOST): the `while` of the caller's loop.  One 4-byte readback; synchronises the stream.        */
int  sfx_opt_active(sfx_opt* h, int32_t* n_active_host, void* stream);
/* What the reference leaves behind: the accepted point x_dev [B][N] (the parameters after step()) and grad_dev [B][N], the
 * gradient of each problem's most recent consumed evaluation (var.grad, fitting.py:191) -- DEVICE, may be NULL; per problem
 * (HOST, may be NULL): result -- mode 0 the value run_fitting returns (fitting.py:217; NaN for None), mode 1 the loss at entry
 * (lbfgs_ls.py:445) --, evaluations consumed since the last fresh begin, status (0 running, 1 finished).  Synchronises.   */
int  sfx_opt_get(sfx_opt* h, float* x_dev, float* grad_dev, float* result_host, int32_t* evals_host, int32_t* status_host);
/* Optimiser trace: records as sfx_batch_trace (types 0, 1, 2; the stage of a type-2 record is 0).  capacity > 0 attaches a
 * buffer of `capacity` records per problem, 0 detaches it; a fresh sfx_opt_begin empties it.
 * sfx_opt_get_trace: records [B][capacity][4] and the number written per problem (HOST; counts may exceed capacity).      */
int  sfx_opt_trace(sfx_opt* h, int32_t capacity);
int  sfx_opt_get_trace(sfx_opt* h, float* records, int32_t* counts);

/* ---- the same optimiser for problems of up to 32768 variables (csrc/opt_wide.hip, csrc/lbfgs_wide.h) ---------
 * B independent problems of N <= 32768 float32 variables each: the state machine of sfx_opt_* on a vector layer one workgroup
 * (1024 threads) wide, one workgroup per problem, one evaluation per launch; dot products accumulated in float64 and rounded
 * once, no atomics, a problem's bits depend on its own inputs only.  What a loss that couples frames needs -- one shape over
 * a clip, a temporal smoothness term, per-vertex offsets -- and what the reference's LBFGS (lbfgs_ls.py:256-445), which has no
 * size limit, takes as it is.  The contracts are those of sfx_opt_*, word for word.                                          */
typedef struct sfx_opt_wide sfx_opt_wide;
typedef struct sfx_opt_wide_cfg {
    int32_t B, N;
    int32_t n_groups; const int32_t* group_len; /* HOST, n_groups <= 256 lengths (read by sfx_opt_wide_create only): the tensors
                                                  of `params`, as sfx_opt_cfg.group_len; 0 groups = one group of N */
    int32_t maxiters; double ftol, gtol;       /* run_fitting (fitting.py:147-217); maxiters >= 1 */
    float   lr;
    double  tolerance_grad, tolerance_change;  /* negative = default 1e-5 / 1e-9; 0 is passed through */
    int32_t max_iter, max_eval, history_size;  /* 0 = defaults: maxiters, max_iter * 5 / 4, 100 */
    int32_t reuse_entry_eval;                  /* as sfx_opt_cfg.reuse_entry_eval (mode 0) */
} sfx_opt_wide_cfg;
/* Refused before any device memory is touched (-1): N outside 1..32768, B < 1, more than 256 groups, group lengths that do not
 * sum to N, history_size outside 0..400.  -3: no HIP device.  -2: out of device memory (nothing stays allocated).  Device
 * memory: 2 (history_size + 1) + 11 rows of N floats per problem (27.9 MB at N = 32768, history 100).                   */
int  sfx_opt_wide_create(const sfx_opt_wide_cfg* cfg, sfx_opt_wide** out);
void sfx_opt_wide_destroy(sfx_opt_wide* h);
/* As sfx_opt_begin: mode 0 the whole run_fitting loop, mode 1 ONE LBFGS.step; resume = 1 continues the optimiser of the previous
 * mode-1 run, 0 starts a fresh one and empties the trace.  x0_dev, x_trial_dev [B][N] (DEVICE, packed).  Enqueues only.   */
int  sfx_opt_wide_begin(sfx_opt_wide* h, int32_t mode, int32_t resume, const float* x0_dev, float* x_trial_dev, void* stream);
/* As sfx_opt_tell: consume loss_dev [B] and grad_dev [B][N] (DEVICE, packed) taken at the current trial points, write the next
 * ones to x_trial_dev.  A problem that has finished is left alone: its loss and gradient are not read, its row of x_trial_dev
 * -- its accepted point -- is not written.  Enqueues only, allocates nothing.                                              */
int  sfx_opt_wide_tell(sfx_opt_wide* h, const float* loss_dev, const float* grad_dev, float* x_trial_dev, void* stream);
/* Problems still running (HOST).  One readback of B status words; synchronises the stream.                                */
int  sfx_opt_wide_active(sfx_opt_wide* h, int32_t* n_active_host, void* stream);
/* As sfx_opt_get: accepted point x_dev [B][N] and gradient of the most recent consumed evaluation grad_dev [B][N] (DEVICE, may
 * be NULL); per problem (HOST, may be NULL) result, evaluations consumed since the last fresh begin, status.  Synchronises. */
int  sfx_opt_wide_get(sfx_opt_wide* h, float* x_dev, float* grad_dev, float* result_host, int32_t* evals_host, int32_t* status_host);
/* As sfx_opt_trace / sfx_opt_get_trace: records of types 0, 1, 2.                                                         */
int  sfx_opt_wide_trace(sfx_opt_wide* h, int32_t capacity);
int  sfx_opt_wide_get_trace(sfx_opt_wide* h, float* records, int32_t* counts);

/* ---- the objective on tensors the CALLER supplies (csrc/objective_ext.hip) -----------------------------------
 * Replaces `loss(body_model_output, camera=..., gt_joints=..., ...)` of the reference's closure (fitting.py:251-259) and what
 * `total_loss.backward()` walks behind it down to the loss's inputs, for B frames at once and for joints that came from
 * anywhere: SMPLifyLoss.forward (fitting.py:375-461 without the interpenetration lines :437-455, which the stand-alone
 * sfx_pen_* operators cover), with camera.py:93-117, utils.py:84-95 (GMoF) and prior.py:53-97, :100-231 inside it.
 * Stateless: no handle, no allocation, no synchronisation -- one launch that writes the loss of every frame AND the gradient of
 * that frame's loss with respect to every differentiable input.  All pointers are DEVICE pointers to contiguous fp32;
 * arithmetic is fp32.  One wavefront per frame, fixed-order reductions, no atomics: a frame's bits depend on its own inputs
 * only (not on B or its position in the batch).  A keypoint whose weight (joint_weights x confidence) is 0 contributes
 * exactly 0 to the loss and to every gradient, whatever its coordinates hold.
 * Refused (-1) before anything is launched: B < 1, K outside 1..512, an unknown prior form, the mixture form with D != 63 (or
 * an operand that is not 63 long) or M outside 1..32, a NULL required input.                                          */
enum {                              /* sfx_objective_cfg.prior_form: the pose prior of fitting.py:390-401                   */
    SFX_PRIOR_L2_EMBEDDING = 0,     /* |operand|^2: use_vposer, operand = pose_embedding (:395)                           */
    SFX_PRIOR_L2_TARGET = 1,        /* |operand - target|^2: the regression prior (:393, :397)                            */
    SFX_PRIOR_L2_BODY_POSE = 2,     /* |operand|^2: body_prior_type 'l2', operand = body_model_output.body_pose (:399-401); the
                                       same arithmetic as form 0 -- kept apart because the caller's operand differs         */
    SFX_PRIOR_MIXTURE = 3           /* MaxMixturePrior on operand = body_model_output.body_pose (:399-401, prior.py:100-231) */
};
typedef struct sfx_objective_cfg {
    float   rho;                    /* GMoF rho (cfg: 100)                                                                 */
    float   data_weight, body_pose_weight, shape_weight, bending_prior_weight, hand_prior_weight, expr_prior_weight;
    float   jaw_prior_weight[3];    /* the stage's weights as SMPLifyLoss holds them (fitting.py:341-359)                  */
    int32_t use_joints_conf;        /* weights = joint_weights * joints_conf (:380)                                        */
    int32_t use_hands, use_face;    /* off: the hand / expression + jaw terms are 0 and their gradients are zeros          */
    int32_t prior_form;             /* SFX_PRIOR_*                                                                          */
    /* SFX_PRIOR_MIXTURE: the module's buffers as prior.mixture_tables makes them (DEVICE): means [M][D], precisions [M][D][D]
     * (not symmetrised), nll_weights [M]; comp_const [M] or NULL with the semantics of sfx_batch_set_gmm_form (NULL = the
     * merged form).  D must be 63.                                                                                        */
    int32_t gmm_M, gmm_D;
    const float* gmm_means_dev; const float* gmm_precisions_dev; const float* gmm_nll_weights_dev; const float* gmm_comp_const_dev;
} sfx_objective_cfg;
typedef struct sfx_objective_in {
    int32_t B, K;                   /* frames, keypoints per frame                                                         */
    int32_t n_prior;                /* length of the pose-prior operand (latent size, or 63)                               */
    int32_t num_betas, num_expr;
    const float* joints_dev;        /* [B][K][3]   body_model_output.joints                                                */
    const float* cam_rot_dev;       /* [B][3][3]   camera.rotation                                                         */
    const float* cam_t_dev;         /* [B][3]      camera.translation                                                      */
    const float* focal_x_dev; const float* focal_y_dev;   /* [B]                                                           */
    const float* center_dev;        /* [B][2]                                                                              */
    const float* gt_joints_dev;     /* [B][K][2]                                                                           */
    const float* joints_conf_dev;   /* [B][K]      (NULL allowed without use_joints_conf)                                  */
    const float* joint_weights_dev; /* [B][K]                                                                              */
    const float* body_pose_dev;     /* [B][63]     full_pose[:, 3:66]: the angle prior's operand (:407-408)                 */
    const float* prior_dev;         /* [B][n_prior] the pose prior's operand, see SFX_PRIOR_*                              */
    const float* prior_target_dev;  /* [B][n_prior] regression_pose (SFX_PRIOR_L2_TARGET only, else NULL)                  */
    const float* betas_dev;         /* [B][num_betas]                                                                      */
    const float* expression_dev;    /* [B][num_expr]                      (use_face)                                       */
    const float* jaw_dev;           /* [B][3]                             (use_face)                                       */
    const float* lhand_dev; const float* rhand_dev;       /* [B][45] as ModelOutput carries them (use_hands)               */
} sfx_objective_in;
typedef struct sfx_objective_grads {  /* d loss[b] / d input, shaped like the input; any may be NULL (not wanted)            */
    float* d_joints_dev; float* d_cam_rot_dev; float* d_cam_t_dev; float* d_body_pose_dev; float* d_prior_dev;
    float* d_betas_dev; float* d_expression_dev; float* d_jaw_dev; float* d_lhand_dev; float* d_rhand_dev;
} sfx_objective_grads;
/* cfg, in and grads are HOST structures (read during the call) holding DEVICE pointers; grads may be NULL (loss only).
 * loss_dev [B].  The total is summed in the term order of fitting.py:457-460.                                             */
int  sfx_objective_eval(const sfx_objective_cfg* cfg, const sfx_objective_in* in, const sfx_objective_grads* grads,
                        float* loss_dev, void* stream);

/* SMPLifyCameraInitLoss.forward (fitting.py:499-520) in the same way: squared pixel residuals of the keypoints of
 * init_joints_idxs plus the depth term, with gradients to joints, rotation and translation.  init_count_dev [K]: how often
 * keypoint k appears in init_joints_idxs (index_select repeats a repeated index; 0 = not selected: contributes exactly 0).
 * use_conf reproduces the broadcast of :509-511 (oracle/objective.py:camera_init_loss): every residual is weighted by the SUM
 * of the selected keypoints' squared confidences (joints_conf_dev [B][K]).  est_tz_dev [B] = trans_estimation[:, 2]; NULL, or
 * depth_loss_weight <= 0: no depth term.  Refusals as sfx_objective_eval.                                                */
typedef struct sfx_camera_init_cfg {
    float   data_weight, depth_loss_weight;
    int32_t use_conf;
} sfx_camera_init_cfg;
int  sfx_camera_init_eval(const sfx_camera_init_cfg* cfg, int32_t B, int32_t K,
                          const float* joints_dev, const float* cam_rot_dev, const float* cam_t_dev,
                          const float* focal_x_dev, const float* focal_y_dev, const float* center_dev,
                          const float* gt_joints_dev, const float* init_count_dev, const float* joints_conf_dev /* or NULL */,
                          const float* est_tz_dev /* or NULL */, float* loss_dev, float* d_joints_dev /* [B][K][3] or NULL */,
                          float* d_cam_rot_dev /* [B][3][3] or NULL */, float* d_cam_t_dev /* [B][3] or NULL */, void* stream);

/* ---- evaluation of fitted meshes on the device (csrc/evaluate.hip) -----------------------------------------------------
 * Both entries are stateless like the two above: device pointers, sizes, a stream; no handle, no allocation, no
 * synchronisation.  B == 0 returns 0 before any pointer is looked at.  A refusal returns -1, sets the error text and
 * launches nothing.  Masks are uint8 [B][points] or NULL (every point valid); 0 takes the point out.
 *
 * Alignment and per-point error of B estimated point sets against their ground truth: ProcrustesAlignment
 * (smplifyx/utils.py:540-595), mpjpe / vertex_to_vertex_error (utils.py:597-614), PelvisAlignment (utils.py:650-668) and
 * ScaleAlignment (utils.py:729-772).
 *   est_dev, gt_dev   [B][N][3] float32
 *   mask_dev          a masked point is left out of every sum of its mesh and its error is exactly 0 (the reference's protocol
 *                     scores another vertex subset in every frame, eval.py:102-121)
 *   anchors           HOST int32 [n_anchors], 1 <= n_anchors <= SFX_ALIGN_MAX_ANCHORS, read by SFX_ALIGN_PELVIS only (NULL
 *                     otherwise): rows whose mean each set is moved by (the hip joints 2, 3 of the reference).  Read during
 *                     the call; an anchor outside 0 .. N-1 is refused.  Anchor rows are read whether masked or not.
 *   err_dev           [B][N] float32: Euclidean distance after alignment
 *   mean_dev          [B] or NULL: mean of err over the valid points (no valid point: NaN, the errors all 0)
 *   xform_dev         [B][13] float32 or NULL: scale, R row-major, t of the map  p -> scale R p + t  applied to the estimate.
 *                     NONE: 1, I, 0.  SCALE: R = I.  PELVIS: 1, I, t = -(mean of the estimate's anchor rows); the ground truth is
 *                     moved by the mean of its own anchor rows, which is not part of xform.
 * Centroids, the cross-covariance K = X1 X2^T, var1 and var2 are float64 sums over centred points (two passes) in a fixed
 * order without atomics; the 3x3 solve (csrc/procrustes3.h: R = V Z U^T with det R = +1, utils.py:575-581) and the
 * application of the transform are float64, only the stored values are rounded to float32.  A mesh's bits depend on its own
 * points only.  Where the reference divides by zero (one valid point, var1 = 0) the result is non-finite as the reference's. */
enum { SFX_ALIGN_NONE = 0, SFX_ALIGN_PROCRUSTES = 1, SFX_ALIGN_SCALE = 2, SFX_ALIGN_PELVIS = 3 };
#define SFX_ALIGN_MAX_ANCHORS 8
int  sfx_eval_align(int32_t mode, int32_t B, int32_t N, const float* est_dev, const float* gt_dev,
                    const unsigned char* mask_dev, const int32_t* anchors /* HOST */, int32_t n_anchors,
                    float* err_dev, float* mean_dev, float* xform_dev, void* stream);

/* The two nearest-neighbour queries of point_fscore (smplifyx/utils.py:622-648; the reference asks open3d) for B pairs of
 * point sets: for every valid point of a the distance to the nearest valid point of b, and the same for b against a.
 *   a_dev [B][Na][3], b_dev [B][Nb][3] float32; mask_a_dev [B][Na], mask_b_dev [B][Nb]
 *   thresh            HOST double [n_thresh], n_thresh <= SFX_NEAREST_MAX_THRESH (read during the call)
 *   dist_ab_dev [B][Na], dist_ba_dev [B][Nb]   float32 or NULL; 0 at masked points
 *   count_ab_dev, count_ba_dev [B][n_thresh]   int32: valid points whose distance is < thresh[t] (required when n_thresh > 0)
 *   valid_dev [B][2]                           int32 or NULL: valid points of a and of b
 * precision = count_ba / valid[1], recall = count_ab / valid[0] with a = the prediction (utils.py:633-636).
 * Brute force: squared distances from coordinate differences in float32.  A set with no valid point gives distances 0 and
 * counts 0 in both directions.  The counts are integers and do not depend on the order of the work.                      */
#define SFX_NEAREST_MAX_THRESH 8
int  sfx_eval_nearest(int32_t B, int32_t Na, int32_t Nb, const float* a_dev, const float* b_dev,
                      const unsigned char* mask_a_dev, const unsigned char* mask_b_dev,
                      int32_t n_thresh, const double* thresh /* HOST */, float* dist_ab_dev, float* dist_ba_dev,
                      int32_t* count_ab_dev, int32_t* count_ba_dev, int32_t* valid_dev, void* stream);

/* ---- differentiable nearest-point (chamfer) term between point sets (csrc/chamfer.hip, csrc/chamfer_math.h) ---------------
 * The 3D data term of a fit to a scan, a depth map or a reconstruction, for B pairs of point sets a [B][Na][3] and
 * b [B][Nb][3], float32 (by convention a is the mesh and b the cloud; nothing depends on that).  Both entries are stateless like
 * sfx_eval_*: device pointers, sizes, a stream; no handle, no allocation, no synchronisation; the caller supplies the scratch,
 * whose size the two macros below give.  B == 0 returns 0 before any pointer is looked at.  A refusal (a NULL required
 * pointer, Na or Nb outside 1 .. SFX_CHAMFER_MAX_POINTS, rho < 0 or not finite, scratch too small) returns -1, sets the error
 * text and launches nothing.
 *   mask_a_dev [B][Na], mask_b_dev [B][Nb]       uint8 or NULL (every point valid); 0 takes the point out as a query AND as a target
 *   weight_a_dev [B][Na], weight_b_dev [B][Nb]   float32 or NULL (1): scales the point's own query term, has no effect on the
 *                                                point as a target; a constant (no gradient)
 * Nearest target: j(i) = argmin over the valid j of s(i, j) = ((dx dx + dy dy) + dz dz), in float32 from the coordinate
 * differences, in exactly this association and with no fused multiply-add; ties go to the lowest index.  Index and squared
 * distance equal numpy's float32 argmin / min of the same expression bit for bit.
 * Direction a -> b: L_ab = sum over the valid i of w_a[i] rho(s_i);  rho(s) = s when rho == 0, rho^2 s / (s + rho^2) when
 * rho > 0 (the GMoF of smplifyx/utils.py:92-95 on the squared distance).  L_ba: the same with the roles swapped.
 * The per-point value w rho(s) is formed in float64 from the float32 s and stored as float32; a mesh's sum of a direction is
 * float64 in a fixed order (a thread's points in index order, the lanes of a wave, the waves in wave order) and is rounded to
 * float32 once.  No float atomics anywhere: a mesh's bits depend on its own points only, from run to run and in any batch.
 * A masked query has index -1, squared distance 0, value 0 and gradient 0.  A direction whose target set has no valid point
 * has every index -1 and loss 0.  Otherwise a query that finds no target nearer than +inf -- a non-finite coordinate, or
 * coordinates so far apart that s overflows -- has index -1, squared distance NaN, gradient 0 and makes that mesh's loss of
 * that direction NaN.
 *   idx_ab_dev [B][Na], idx_ba_dev [B][Nb]       int32: the nearest valid point of the other set, or -1
 *   dist2_ab_dev, dist2_ba_dev                   float32 or NULL: s at that point
 *   loss_dev [B][2]                              L_ab, L_ba
 *   valid_dev [B][2]                             int32 or NULL: valid (unmasked) points of a and of b
 * Gradient: d L_ab / d a_i = g_ab w_a[i] rho'(s_i) 2 (a_i - b_j(i)), and d L_ab / d b_j the negative of that summed over every i
 * with j(i) = j; rho'(s) = 1 when rho == 0, rho^4 / (s + rho^2)^2 when rho > 0; L_ba gives the same two terms with the roles
 * swapped.  s is formed again from the points (the same bits as the forward's).  The scatter goes through an inverted index
 * built per call from integers (counts, an exclusive scan, a fill, every entry moved to its rank): for every row the list of
 * the queries that chose it, in ascending query index.  A row is its gather term plus its list, in float64: the list is cut
 * into segments (one up to 32 entries, else 64 of equal length), each summed from 0 in list order, the segment sums added to
 * the gather term in segment order, rounded to float32 once (csrc/chamfer_math.h states the rule).  An index outside
 * 0 .. targets - 1 counts as -1.
 *   grad_dev [B][2]                              upstream d / d L_ab, d / d L_ba
 *   da_dev [B][Na][3], db_dev [B][Nb][3]         or NULL: not computed
 * Known limit: both directions are point-to-POINT; against a mesh that is point-to-vertex, not point-to-triangle
 * (sfx_p2m_forward below is the point-to-triangle term of the cloud -> surface direction).                                     */
#define SFX_CHAMFER_MAX_POINTS (1 << 26)
#define SFX_CHAMFER_FORWARD_SCRATCH_BYTES(B, Na, Nb)  ((int64_t)4 * (int64_t)(B) * ((int64_t)(Na) + (int64_t)(Nb)))
#define SFX_CHAMFER_BACKWARD_SCRATCH_BYTES(B, Na, Nb) ((int64_t)4 * (int64_t)(B) * (4 * ((int64_t)(Na) + (int64_t)(Nb)) + 2))
int  sfx_chamfer_forward(int32_t B, int32_t Na, int32_t Nb, const float* a_dev, const float* b_dev,
                         const unsigned char* mask_a_dev, const unsigned char* mask_b_dev,
                         const float* weight_a_dev, const float* weight_b_dev, float rho,
                         int32_t* idx_ab_dev, int32_t* idx_ba_dev, float* dist2_ab_dev, float* dist2_ba_dev,
                         float* loss_dev, int32_t* valid_dev, void* scratch_dev, int64_t scratch_bytes, void* stream);
int  sfx_chamfer_backward(int32_t B, int32_t Na, int32_t Nb, const float* a_dev, const float* b_dev,
                          const unsigned char* mask_a_dev, const unsigned char* mask_b_dev,
                          const float* weight_a_dev, const float* weight_b_dev, float rho,
                          const int32_t* idx_ab_dev, const int32_t* idx_ba_dev, const float* grad_dev,
                          float* da_dev, float* db_dev, void* scratch_dev, int64_t scratch_bytes, void* stream);

/* ---- differentiable point-to-triangle term from point clouds to mesh surfaces (csrc/p2m.hip, csrc/p2m_math.h) ------------
 * The point-to-SURFACE residual of a fit to a scan or a depth map: for B clouds p [B][Np][3] and B meshes v [B][Nv][3] of one
 * topology faces [F][3] (int32), float32, every cloud point against the nearest point of its mesh's triangles.  Only the cloud ->
 * surface direction; mesh -> cloud of a two-sided term is L_ab of sfx_chamfer_forward, and the caller adds the two.  Stateless
 * like sfx_chamfer_*: device pointers, sizes, a stream; no handle, no allocation, no synchronisation; the caller supplies the
 * scratch, whose size the two macros below give.  B == 0 returns 0 before any pointer is looked at.  A refusal (a NULL required
 * pointer, Np, Nv or F outside 1 .. SFX_P2M_MAX_POINTS, rho < 0 or not finite, scratch too small) returns -1, sets the error
 * text and launches nothing.
 *   mask_p_dev [B][Np]       uint8 or NULL: 0 takes the point out
 *   mask_f_dev [B][F]        uint8 or NULL: 0 takes the face out; a face that names a vertex outside 0 .. Nv - 1 is out as well
 *   weight_p_dev [B][Np]     float32 or NULL (1): scales the point's term; a constant (no gradient)
 * Closest point of triangle abc to p: the region test of Ericson, Real-Time Collision Detection 5.1.5, in float32 with no fused
 * multiply-add and the correctly rounded division, in exactly this association (csrc/p2m_math.h restates it):
 * dot(x, y) = (x0 y0 + x1 y1) + x2 y2;  ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c;  d1 = ab.ap, d2 = ac.ap,
 * d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp;  vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.  The first
 * condition that holds decides (v, w):  d1 <= 0 and d2 <= 0: (0, 0);  d3 >= 0 and d4 <= d3: (1, 0);  vc <= 0, d1 >= 0 and
 * d3 <= 0: (d1 / (d1 - d3), 0);  d6 >= 0 and d5 <= d6: (0, 1);  vb <= 0, d2 >= 0 and d6 <= 0: (0, d2 / (d2 - d6));  va <= 0,
 * d4 - d3 >= 0 and d5 - d6 >= 0: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w;  otherwise den = 1 / ((va + vb) + vc),
 * v = vb den, w = vc den.  u = (1 - v) - w;  q = (a + v ab) + w ac;  d = p - q;  s = dot(d, d).  A degenerate face can give a NaN
 * s; a NaN never wins.  Nearest face: the argmin of s over the candidate faces, replaced on strict <, so ties go to the lowest
 * face index.  face, s and the barycentrics equal a float32 numpy restatement of the above bit for bit.
 * L = sum over the valid points of w rho(s), rho as in sfx_chamfer_forward (rho == 0: s; rho > 0: the GMoF rho^2 s / (s + rho^2),
 * smplifyx/utils.py:92-95).  The per-point value is float64 from the float32 s, stored as float32; a mesh's sum is float64 in
 * the fixed order of sfx_chamfer_forward and is rounded to float32 once.  No float atomics anywhere.
 * A masked point has face -1, barycentrics 0, squared distance 0, value 0 and gradient 0.  A mesh with no candidate face at all
 * has every face -1 and loss 0.  Otherwise a point that finds no face nearer than +inf has face -1, barycentrics and squared
 * distance NaN, gradient 0 and makes that mesh's loss NaN.
 *   face_dev [B][Np]         int32: the nearest candidate face, or -1
 *   bary_dev [B][Np][3]      float32 or NULL: (u, v, w) of the closest point on it
 *   dist2_dev [B][Np]        float32 or NULL: s
 *   loss_dev [B]             L
 *   valid_dev [B]            int32 or NULL: valid (unmasked) points
 * Gradient at the faces given: with c = ((g w) rho'(s)) 2 in float64, d L / d p_i = c (p_i - q_i), the difference in float64
 * from the float32 p and q, and corner k of the face receives -(c bary_k)(p_i - q_i): the barycentrics minimise, so they carry
 * no derivative (envelope theorem).  s, q and the barycentrics are formed again from the points (the same bits as the forward's).
 * The scatter goes through the inverted index of sfx_chamfer_backward over the 3 Np entries e = 3 i + k and the Nv rows: for
 * every vertex its entries in ascending e, cut into segments (one up to 32 entries, else 64 of equal length), each summed from
 * 0 in list order, the segment sums added in segment order, float64, rounded to float32 once.  A point whose face is outside
 * 0 .. F - 1, or names a vertex outside the mesh, has no term.
 *   grad_dev [B]             upstream d / d L
 *   dp_dev [B][Np][3], dv_dev [B][Nv][3]         or NULL: not computed
 * Not built: point-to-plane, a spatial index or pruning (the search is brute force), a float64 kernel.                         */
#define SFX_P2M_MAX_POINTS (1 << 26)
#define SFX_P2M_FORWARD_SCRATCH_BYTES(B, Np, Nv)  ((int64_t)4 * (int64_t)(B) * (int64_t)(Np))
#define SFX_P2M_BACKWARD_SCRATCH_BYTES(B, Np, Nv) ((int64_t)4 * (int64_t)(B) * (9 * (int64_t)(Np) + 2 * (int64_t)(Nv) + 1))
int  sfx_p2m_forward(int32_t B, int32_t Np, int32_t Nv, int32_t F, const float* p_dev, const float* v_dev,
                     const int32_t* faces_dev, const unsigned char* mask_p_dev, const unsigned char* mask_f_dev,
                     const float* weight_p_dev, float rho, int32_t* face_dev, float* bary_dev, float* dist2_dev,
                     float* loss_dev, int32_t* valid_dev, void* scratch_dev, int64_t scratch_bytes, void* stream);
int  sfx_p2m_backward(int32_t B, int32_t Np, int32_t Nv, int32_t F, const float* p_dev, const float* v_dev,
                      const int32_t* faces_dev, const unsigned char* mask_p_dev, const float* weight_p_dev, float rho,
                      const int32_t* face_dev, const float* grad_dev, float* dp_dev, float* dv_dev,
                      void* scratch_dev, int64_t scratch_bytes, void* stream);

/* ---- fitted meshes drawn over their images on the device (csrc/raster.hip, csrc/host/render.hip) ------------------------
 * A batched software rasteriser for B triangle meshes of one topology, in place of render_mesh (smplifyx/utils.py:497-538:
 * pyrender's offscreen OpenGL).  Stateless like sfx_eval_*: device pointers, sizes, a stream; no handle, no allocation, no
 * synchronisation; the caller supplies the scratch.  B == 0 returns 0 before any pointer is looked at.  A refusal (a NULL
 * required pointer, n_lights outside 0 .. SFX_RENDER_MAX_LIGHTS, znear not > 0, V or F < 1, H or W < 1, H * W or B * H * W
 * beyond int32) returns -1, sets the error text and launches nothing.
 *
 * Camera: the fit camera itself (camera.PerspectiveCamera.forward): p_c = R p + t, x = fx X / Z + cx, y = fy Y / Z + cy, pixel
 * centres at (i + 0.5, j + 0.5), y down.  The reference reaches the same projection by a detour -- it rotates the mesh by 180
 * degrees about x, negates transl[0] and hands both to an OpenGL camera that looks down -z -- which is algebraically this
 * projection with R = I.
 * Vertices: screen = (x, y, Z) in float32, snapped to 1/256 pixel (rint).  A vertex is unusable when Z >= znear is false, a
 * component is not finite, or |x| or |y| exceeds 2^20 pixels.  A triangle with an unusable vertex is dropped whole (there is NO
 * near-plane clipping) and counted in dropped[b]; one whose snapped area is zero covers nothing.
 * Coverage: int64 edge functions on the snapped corners at the pixel centres, top-left fill rule, both windings
 * (csrc/raster_fixed.h): exact -- a manifold mesh has no cracks and no pixel hit twice along a shared edge.
 * Depth: perspective-correct, lambda_i = (float)e_i / (float)area2, depth = 1 / sum lambda_i / Z_i.  Visibility: the smallest
 * (bits(depth) << 32 | triangle) per pixel, so equal depths go to the lowest triangle id and an image depends neither on the
 * order of the work nor on the batch.
 * Shading: smooth vertex normals in camera space (for every vertex the un-normalised cross products of its usable incident
 * faces, summed in the order of the vertex -> face lists, then normalised; no float atomics); per pixel b_i = lambda_i depth /
 * Z_i, n = normalize(sum b_i n_i) turned towards the camera (n . p_c <= 0), shade = min(1, (1 / pi) sum_l I_l max(0, n . d_l)),
 * rgb = base * shade, stored as floor(255 c + 0.5).  d_l points from the surface TO light l in the camera's frame and is used
 * as given.  A covered pixel takes the mesh colour with alpha 255, an uncovered one the background with alpha 0
 * (utils.py:531-536).  pyrender's metallic-roughness shader is not reproduced.
 *   vf_offsets_dev [V + 1], vf_faces_dev [3 F]   the faces of every vertex (CSR), ascending face ids
 *   cam_rot_dev row-major R per mesh or NULL (identity); focal_dev (fx, fy), center_dev (cx, cy) per mesh
 *   vis_scratch_dev, vnormal_scratch_dev, snapped_scratch_dev    overwritten
 *   rgba_dev, depth_dev (+inf where empty), tri_dev (-1 where empty), screen_dev, dropped_dev    outputs, each may be NULL     */
#define SFX_RENDER_MAX_LIGHTS 8
typedef struct sfx_render_cfg {
    float base_rgb[3];
    int32_t n_lights;
    float light_dir[SFX_RENDER_MAX_LIGHTS][3];
    float light_intensity[SFX_RENDER_MAX_LIGHTS];
    float znear;
} sfx_render_cfg;
int  sfx_render_meshes(const sfx_render_cfg* cfg, int32_t B, int32_t V, int32_t F, int32_t H, int32_t W,
                       const float* verts_dev /* [B][V][3] */, const int32_t* faces_dev /* [F][3] */,
                       const int32_t* vf_offsets_dev /* [V+1] */, const int32_t* vf_faces_dev /* [3F] */,
                       const float* cam_rot_dev /* [B][9] or NULL = I */, const float* cam_t_dev /* [B][3] */,
                       const float* focal_dev /* [B][2] */, const float* center_dev /* [B][2] */,
                       const unsigned char* background_dev /* [B][H][W][3] or NULL = black */,
                       unsigned long long* vis_scratch_dev /* [B][H][W] */, float* vnormal_scratch_dev /* [B][V][3] */,
                       int32_t* snapped_scratch_dev /* [B][V][2] */,
                       unsigned char* rgba_dev /* [B][H][W][4] or NULL */, float* depth_dev /* [B][H][W] or NULL */,
                       int32_t* tri_dev /* [B][H][W] or NULL */, float* screen_dev /* [B][V][3] or NULL */,
                       int32_t* dropped_dev /* [B] or NULL */, void* stream);

/* Gaussian-mixture body pose prior (MaxMixturePrior, smplifyx/prior.py:100-231; body_prior_type 'gmm'):
 * used by the closure when use_vposer is off and the batch has no regression pose (fitting.py:399-401).
 * means [M][D], precisions [M][D][D], nll_weights [M] = the module's buffers; D = 63, M <= 8 (HOST). */
int  sfx_batch_set_gmm(sfx_batch* b, int32_t M, int32_t D, const float* means, const float* precisions,
                       const float* nll_weights);
/* The same prior in its per-component form (MaxMixturePrior(use_merged=False), prior.py:203-225):
 *   m* = argmin_m [ d_m^T P_m d_m + comp_const_m ],  value = d^T P d + comp_const (at m*) - log nll_weights_m*
 * comp_const [M] = 0.5 (log(det cov_m + epsilon) + D log 2 pi) (HOST); comp_const NULL = the merged form above.   */
int  sfx_batch_set_gmm_form(sfx_batch* b, int32_t M, int32_t D, const float* means, const float* precisions,
                            const float* nll_weights, const float* comp_const);

/* ---- float64 mode (sfx_batch_cfg.high_precision = 2); each of these refuses a batch of mode 0 or 1.
 * sfx_batch_set_stage_weights_f64: the batch's stage weights [n_stages] in double (sfx_batch_create widens the float ones).
 * sfx_batch_set_frames_f64: as sfx_batch_set_frames; camera (focal, center, data_weight = 1000 / H, est_tz) in double,
 *   keypoints, weights, masks and rotation must hold fp32 values (kept in fp32 tables, as the reference reads them).
 * sfx_batch_set_params_f64 / sfx_batch_get_params_f64: as sfx_batch_set_params / get_params in double; the regression
 *   pose must hold fp32 values.  body_pose = the embedding (no VPoser in this mode).
 * sfx_batch_closure_f64: as sfx_batch_closure, loss [B] and gradient [B][N] in double.
 * sfx_batch_get_grad_f64: as sfx_batch_get_grad in double.                                                    */
int  sfx_batch_set_stage_weights_f64(sfx_batch* b, const sfx_stage_weights_f64* stages /* [n_stages] */);
int  sfx_batch_set_frames_f64(sfx_batch* b, const double* keypoints, const double* joint_weights,
                              const double* cam_init_mask, const double* camera, const double* cam_rot);
int  sfx_batch_set_params_f64(sfx_batch* b, const double* cam_translation, const double* global_orient,
                              const double* betas, const double* lhand, const double* rhand,
                              const double* expression, const double* jaw, const double* leye,
                              const double* reye, const double* pose_embedding,
                              const double* regression_pose);
int  sfx_batch_get_params_f64(sfx_batch* b, double* cam_translation, double* global_orient,
                              double* betas, double* lhand, double* rhand, double* expression,
                              double* jaw, double* leye, double* reye, double* pose_embedding,
                              double* body_pose);
int  sfx_batch_closure_f64(sfx_batch* b, int32_t stage, double* loss_out, double* grad_out, void* stream);
int  sfx_batch_get_grad_f64(sfx_batch* b, int32_t stage, double* grad_out);

/* Final meshes / joints at the current parameters (dense LBS; DEVICE pointers, may be NULL). */
int  sfx_batch_forward(sfx_batch* b, float* vertices_out_dev /* [B][V][3] */,
                       float* joints_out_dev /* [B][K][3] */, void* stream);

/* ---- interpenetration term ---------------------------------------------
 * Replaces BVH(max_collisions) + FilterFaces(segm, parents, ign_part_pairs) +
 * DistanceFieldPenetrationLoss(sigma, penalize_outside) of the external mesh_intersection
 * package as the reference uses them (fitting.py:437-455, fit_single_frame.py:300-328), for a
 * batch of posed meshes.  faces [F][3]; segm / parents [F] per-face part labels of
 * smplx_parts_segm.pkl (NULL: no part filter); ign_pairs [n_ign][2] part pairs that never
 * collide; max_collisions = partners kept per triangle; max_batch = frames per call.            */
typedef struct sfx_pen sfx_pen;
int  sfx_pen_create(int32_t V, int32_t F, const int32_t* faces, const int32_t* segm, const int32_t* parents,
                    const int32_t* ign_pairs, int32_t n_ign, int32_t max_collisions, int32_t max_batch,
                    sfx_pen** out);
void sfx_pen_destroy(sfx_pen* h);
/* vertices [B][V][3] (DEVICE) -> loss [B] (DEVICE, unweighted: the caller multiplies by
 * coll_loss_weight) and d loss / d vertices [B][V][3] (DEVICE).  sigma = df_cone_height.        */
int  sfx_pen_eval(sfx_pen* h, int32_t B, const float* verts_dev, float sigma, int32_t penalize_outside,
                  float* loss_dev, float* dverts_dev, void* stream);
/* DistanceFieldPenetrationLoss(point2plane=...) (fit_single_frame.py:311-314, cmd_parser.py:239; every shipped cfg: False).
 * on: every Psi^2 of a pair (f, g) is weighted by (n_f . n_g)^2 -- the repulsion of a vertex measured along the other
 * triangle's normal (oracle/penetration.py, assumption A6) -- in all later evaluations of the handle.               */
int  sfx_pen_set_point2plane(sfx_pen* h, int32_t on);
/* DistanceFieldPenetrationLoss(...)(triangles, collision_idxs) stand-alone (fitting.py:451-455): loss and gradients for pairs the
 * CALLER supplies -- pairs_dev DEVICE int32 [B][n_pairs][2] triangle ids, each unordered pair once, rows with a negative id empty
 * (the package's -1 padding).  Outputs as sfx_pen_eval, plus dtri_dev DEVICE [B][F][3][3] or NULL: the gradient with respect to
 * every triangle CORNER (what autograd needs for the `triangles` tensor).  At most 8192 pairs per mesh.  Synchronises the stream. */
int  sfx_pen_eval_pairs(sfx_pen* h, int32_t B, const float* verts_dev, const int32_t* pairs_dev, int32_t n_pairs, float sigma,
                        int32_t penalize_outside, float* loss_dev, float* dverts_dev, float* dtri_dev, void* stream);
/* per frame (HOST [B][4]): ordered pairs kept, partners dropped by max_collisions / the pair list's capacity, grid entries
 * when they overflowed the buffer (0 = fine; then the frame reports no pairs), bucket walks cut short (0 on a sane mesh:
 * an entry looks at most 2048 entries ahead in its bucket; a mesh folded into a few cells by a diverged fit hits that). */
int  sfx_pen_stats(sfx_pen* h, int32_t B, int32_t* stats_host);
/* The pair list of mesh `mesh` of the most recent evaluation: HOST [cap][2] ordered pairs (receiving triangle, partner), receiver
 * ascending, partner ascending within a receiver, both orders of every colliding pair; *n_out = pairs in the list (the first
 * min(n, cap) are copied).  = collision_idxs after BVH and FilterFaces in the reference (fitting.py:445-450).                  */
int  sfx_pen_pairs(sfx_pen* h, int32_t mesh, int32_t cap, int32_t* pairs_host, int32_t* n_out);
/* Work the term has done since the last reset, counted on the device over every handle of the process (HOST [6]): grid
 * entries, ordered pairs kept, column evaluations (meshes that went through the broad phase), triangles that survived the
 * part culling, triangles that met more partners than the lists hold while they are collected (2 x max_collisions: their kept
 * partners are derived from the grid a second time -- 0 on a sane mesh), bucket walks cut short.  The benchmark's byte model of the step (bench.py
 * roofline_pen) divides the first two by the third.                                                                    */
int  sfx_pen_work_reset(void);
int  sfx_pen_work_get(int64_t* work_host);
/* Host side of the fitting loops (dense mode) since the last reset, HOST [4]: seconds the host thread spent enqueueing launches,
 * seconds it spent waiting for a batch's stage flags, wall seconds of the loops, rounds enqueued.  Wall time far above the kernels'
 * time with little waiting = the queue ran dry behind a slow host (bench.py reports this next to the kernels' times).          */
int  sfx_loop_host_stats(double* stats_host, int32_t reset);

/* Timing hooks for the roofline report: total duration (ms), number of TIMED launches and
 * frames processed by them, of the named kernel since the last reset, measured with HIP events
 * on the launch stream.  name: "lbs_dense", "tick" (k_tick_dense), "fit_rows", "closure",
 * "export", "lbfgs".  sfx_prof_enable(on): bit 0 = time launches; bit 1 = debug, run the
 * fitting loop with the stand-alone kernels; bits 8..23 = N: time every N-th launch of each
 * name only (an event pair costs two queue packets; 0/1 = every launch).                   */
int  sfx_prof_enable(int32_t on);
int  sfx_prof_get(const char* name, double* total_ms, int64_t* launches, double* units /* frames processed */);
void sfx_prof_reset(void);

/* Stand-alone operator (the parity tests of LBFGS.step's direction call it): direction of the device's blocked two-loop
 * recursion for a caller-supplied history (rows of 192 floats, zero padded; `count` pairs pushed in order, the window keeps the last history_size -- <= 0: 100, at most 400) and gradient
 * g[192]; d_out[192].  Host pointers.  Specification: optimizers/lbfgs_ls.py:312-341. */
int  sfx_lbfgs_two_loop(const float* S, const float* Y, int32_t count, int32_t history_size, const float* g, float* d_out);

/* tests / diagnostics: copy a device buffer of the dense path's most recent evaluation to the host, [B][per frame]:
 * "verts", "vposed", "pen_dverts" (V*3), "pen_dfeat", "feat" (512), "pen_dA", "A" (12*55), "pen_loss" (1).
 * n_out = number of floats the caller's buffer holds (checked).                                          */
int  sfx_batch_debug_read(sfx_batch* b, const char* name, float* out, int64_t n_out);

const char* sfx_last_error(void);
const char* sfx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SFX_H_ */
