// Internal structures shared by the host layer (host/) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#define SFX_J 55            // SMPL-X kinematic joints
#define SFX_POSE (3 * SFX_J)
#define SFX_NHAND 45
#define SFX_MAX_K 144       // mapped joints
#define SFX_MAX_ITEMS 240   // vertex items (21 + 68*3 = 225)
#define SFX_SMALL_ITEMS 32  // item capacity of the small closure variant (body-only: 11 items)
#define SFX_MAX_DYN 64      // dynamic-contour items (17 landmarks x 3 corners = 51)
#ifndef SFX_RIF_BIG
#define SFX_RIF_BIG 8        // 2-KiB blend-shape rows in flight per wavefront in the full-model closure (1 workgroup per CU:
#endif                       // the loads of 4 wavefronts are all the memory parallelism a frame gets)
#ifndef SFX_RIF_SMALL
#define SFX_RIF_SMALL 9      // ... in the body-only closure: 33 rows over 4 wavefronts in ONE pass (every pass is a ~1-us round trip to L2 / MALL: 4 -> 9 rows in flight made the needed-rows fit 14 % faster)
#endif
#ifndef SFX_SMALL_OCC
#define SFX_SMALL_OCC 1      // workgroups per CU the register budget of the persistent small kernel is sized for
#endif
#define SFX_KD_PAD 512      // padded blend-shape depth (20 + 486 = 506)
#define SFX_JPAD 56         // joints padded to an even MFMA depth
// K order of the dense blend-shape GEMM (lbs_dense.hip), shared with whoever must reproduce its sums bit for bit: chunks of
// SFX_DENSE_KC rows taken as 1, 2, ..., 15, 0, rows ascending inside a chunk
#define SFX_DENSE_KC 32
#define SFX_DENSE_KCHUNK(c) (((c) + 1) % (SFX_KD_PAD / SFX_DENSE_KC))
#define SFX_MAX_LEVELS 16
#define SFX_HIST 100        // L-BFGS history (optim_factory 'lbfgsls' default): slots of the ring unless history_size asks for more
#ifndef SFX_HIST_MAX
#define SFX_HIST_MAX 400    // largest history_size (the alphas of the two-loop recursion live in LDS: lbfgs_two_loop.h s_al)
#endif
#define SFX_HROWS (SFX_HIST + 8)   // ring of R slots + rows R..R+7 mirroring slots 0..7: any 8 consecutive members of the
#define SFX_HROWS_MAX (SFX_HIST_MAX + 8)   // window are 8 consecutive rows (lbfgs_two_loop.h lb_load); R = BatchCfgDev::hist_ring
#define SFX_NVAR_MAX 192    // optimiser vector length (182 / 88 / 6), padded to 3*64
#define SFX_FWD_N 6016      // floats per frame of saved forward state (FrameLDS prefix incl. the fp64 transforms + 96 + VPoser 1280)
#define SFX_NPAR_MAX 256    // canonical per-frame parameter block (182 with 12 hand components; 248 with all 45: forward only)
#define SFX_MAX_STAGES 8
#define SFX_MAX_GROUPS 12
#define SFX_NW 8             // nonzero skinning weights kept per vertex (needed-rows path)
// packed integer tables of the closure kernel (DevModel.meta)
#define MO_PAR 0
#define MO_LJ 56
#define MO_CS 112
#define MO_CL 168
#define MO_SK0 224
#define MO_SKL 280
#define MO_JT 424
#define MO_JS 568
#define MO_JI0 712
#define MO_JN 856
#define MO_IK 1000
#define MO_PRE 1240         // joint -> DFS pre-order position (subtree = contiguous pre-order range)
#define MO_SUB 1296         // joint -> subtree size
#define MO_ANC 1352         // [SFX_MAX_ROUNDS][56] 2^k-th ancestor of each joint (-1 past the root)
#define SFX_MAX_ROUNDS 5
#define SFX_META_N 1632

// Per-frame record (floats): keypoints, confidences, joint weights, camera-init mask, camera, camera rotation, regression
// pose -- packed by k_pack_fd (host/batch.hip) from the arrays the host fills, read by the closure workgroup in ONE 16-byte copy
#define FD_GT 0
#define FD_CONF (2 * SFX_MAX_K)
#define FD_JW (3 * SFX_MAX_K)
#define FD_CMASK (4 * SFX_MAX_K)
#define FD_CAM (5 * SFX_MAX_K)
#define FD_CAMR (FD_CAM + 8)
#define FD_REG (FD_CAMR + 12)
#define FD_N (FD_REG + 64)

// Canonical per-frame parameter block (floats).  cam_t | global_orient | betas | lhand |
// rhand | expression | jaw | leye | reye | body_pose param (dead, iff !use_vposer) | embedding
struct ParLayout {
    int cam_t, go, betas, lh, rh, expr, jaw, leye, reye, bodyp, emb;
    int NB, NE, NPCA, NEMB, has_bodyp, npar;
};

// Variable list of one optimisation stage kind: flat optimiser index -> canonical index.
struct VarList {
    int n;
    int ngroups;
    short idx[SFX_NVAR_MAX];
    short g_off[SFX_MAX_GROUPS], g_len[SFX_MAX_GROUPS], g_has[SFX_MAX_GROUPS];
};

struct StageW {       // per body stage
    float bpw, sw, bend, hpw, epw, jaw[3], hand_jw, face_jw, coll;
};
struct StageW64 {     // the same in double: the float64 mode (sfx_batch_cfg.high_precision = 2)
    double bpw, sw, bend, hpw, epw, jaw[3], hand_jw, face_jw, coll;
};

// The kernels take DevModel by value.  How the compiler groups their scalar argument loads -- and with it the SGPR spills and
// scratch of the persistent kernels (k_tick_dense, k_fit_rows, k_closure) -- follows the members' offsets, so the members that
// were dropped because nothing reads them (their tables are neither built nor uploaded any more) leave their bytes behind as
// gap*_: every live member stays at the offset the kernels were tuned with, and the kernels compile to the same code.  Closing
// the gaps was measured: other spill counts in eight kernels, scratch 68 -> 100 B in k_tick_dense, body fit -0.3 %.
struct DevModel {
    int V, gap0_, S, gap1_[2], K;     // S = NB+NE (blend-shape depth KD = S + 486 <= SFX_KD_PAD)
    int gap2_[3], n_dyn;
    int gap3_, n_rounds;              // ceil(log2(tree depth + 1)) pointer-jumping rounds
    int gap4_[SFX_MAX_LEVELS + 1];
    // constants
    const float* v_template;   // [V][3]
#ifdef SFX_LAB
    const float* dirs;         // [KD_PAD][3*Vpad]  k-major, coords interleaved (only the lab build's 32-frame dense GEMM reads it)
#else
    const void*  gap5_;
#endif
    const float* dirs_tiled;   // [Vpad/16][KD_PAD][48]  the same matrix, one contiguous block per 16-vertex tile (B operand of the dense and the adjoint GEMM)
    const float* dirsT;        // [V][3][KD_PAD] vertex-major (needed-rows path)
    const float* W;            // [V][J]
    const void*  gap6_;
    // dense skinning GEMM, compressed per 16-vertex tile to the joints that carry weight there
    const int*   tj_n;         // [ntile16] joints used by the tile, padded to a multiple of 4 (<= JPAD)
    const int*   tj_list;      // [ntile16][JPAD] joint ids (padding: joint 0 with zero weights)
    const float* tj_w;         // [ntile16][JPAD][16] weights, row = list slot, col = vertex in tile
    const int*   jv_start;     // [J+1] transposed CSR of lbs_weights: the vertices (ascending) skinned by joint j ...
    const int*   jv_vid;       // [nnz]
    const float* jv_w;         // [nnz] ... and their weights (adjoint of a gradient on every vertex, lbs_adjoint.hip)
    const int*   Wsp_j;        // [V][SFX_NW] joints of the nonzero weights (ascending), pad: j=0,w=0
    const float* Wsp_w;        // [V][SFX_NW]
    const float* J_template;   // [J][3]
    const float* J_dirs;       // [J][3][S]
    const void*  gap7_[4];
    const float* comp_l;       // [NPCA][45]
    const float* comp_r;
    const float* pose_mean;    // [165]
    const void*  gap8_[7];
    // mapped joints: their description (kinematic joint | vertex items, item owners) and the tree are in meta
    int n_items, n_static_items;
    int n_uniq;                // distinct vertices of the static items: the dense GEMM exports their v_posed and T
    const int* vslot;          // [Vpad] vertex -> index into the export arrays, or -1
    const int* item_uslot;     // [n_items] export index of a static item's vertex (-1: dynamic item, whose index comes with its LUT-row block: dynp_us)
    const int*   item_vid;     // [n_items] static vertex id (dynamic items: -1)
    const float* item_w;       // [n_items] static bary weight
    const float* item_vt;      // [n_items][3] v_template row of the item's vertex     } gathered copies for the static items:
    const int*   item_wj;      // [n_items][SFX_NW] = Wsp_j[item_vid]                  } one round trip at kernel entry
    const float* item_ww;      // [n_items][SFX_NW] = Wsp_w[item_vid]                  }
    const float* uniq_dirs;    // [ceil(n_uniq / 16) * 3][32][64][4] the blend-shape rows of the exported vertices as the B operands of
                               // closure_lds.h self_blend_offsets: per (tile of 16 export indices, coordinate) the 128 MFMA steps of
                               // the dense GEMM's K order, four steps per lane and 16-byte load (model_tables.h)
    const void*  gap9_[3];
    int Vpad;
    // per-joint lists of (item, skinning weight): static items, and dynamic items per LUT row
    const int *sj_start, *sj_item; const float* sj_w;      // [J+1], [..]
    const int *dj_start, *dj_item; const float* dj_w;      // [rows][J+1] (absolute offsets), [..]
    int n_dyn_items;
    // everything about the dynamic-contour items that depends on the LUT row, packed per row (one asynchronous copy into
    // the closure workgroup's LDS instead of four dependent global round trips): nd = n_dyn_items
    const int*   dynp_vid;     // [rows][nd]      vertex of item (n_static_items + q)
    const float* dynp_w;       // [rows][nd]      its barycentric weight
    const float* dynp_vt;      // [rows][nd][3]   its v_template row
    const int*   dynp_wj;      // [rows][nd][SFX_NW]  sparse skinning weights (Wsp_j / Wsp_w of the vertex)
    const float* dynp_ww;      // [rows][nd][SFX_NW]
    const int*   dynp_js;      // [rows][J+1]     per-joint adjoint lists of the row, offsets RELATIVE to the row's block ...
    const int*   dynp_ji;      // [rows][nd*SFX_NW]   ... items (absolute item ids), padded to nd * SFX_NW entries per row
    const float* dynp_jw;      // [rows][nd*SFX_NW]
    const int*   dynp_us;      // [rows][nd]      export index of the item's vertex in the dense GEMM's uvp (nullptr: no dynamic items)
    int n_sj;                  // entries of sj_item / sj_w
    const int*   meta;         // [SFX_META_N] the MO_* tables: tree, mapped joints, item owners
    // VPoser decoder
    int vp_latent, vp_hidden;
    const float *vp_w1, *vp_b1, *vp_w2, *vp_b2, *vp_w3, *vp_b3;      // [512][L], [512][512], [126][512]
    const float *vp_w1T, *vp_w2T, *vp_w3T;                          // [L][512], [512][512], [512][128]
    // the folded joint regressor before its rounding to fp32 (the float64 closure: J_regressor . v_shaped of a float64 model)
    const double* J_template64;  // [J][3]
    const double* J_dirs64;      // [J][3][S]
};

struct BatchCfgDev {
    int B, n_stages;
    int use_vposer, use_hands, use_face, use_conf, has_reg, use_conf_cam;
    int nbj;
    int maxiters, max_eval, lbfgs_max_iter;     // (run_fitting's step count | LBFGS max_eval | LBFGS max_iter)
    double ftol, gtol;
    float lr, rho, depth_w;
    int lbs_mode, reuse;
    float side_thsh; int lsh, rsh;     // side-view test: 2-D shoulder distance threshold, indices
    int pen;                           // interpenetration term enabled (dense mode)
    int kl[3], nil[3];                 // live keypoints / vertex items by stage class: body only, + hands, all (closure_body)
    double tol_grad, tol_change;       // LBFGS tolerance_grad / tolerance_change (lbfgs_ls.py defaults 1e-5 / 1e-9)
    int hist_cap;                      // LBFGS history_size (<= SFX_HIST_MAX)
    int hist_ring;                     // slots of the history ring: SFX_HIST, or history_size when that is larger (round 5)
    int proj64;                        // projection in fp64 in every stage (cfg float_dtype float64; the camera stage always is)
};

// Per-frame data pointers (all device).
struct BatchDev {
    BatchCfgDev cfg;
    ParLayout L;
    float* X;          // [B][NPAR_MAX] accepted parameters
    float* Xt;         // [B][NPAR_MAX] trial parameters (what the closure evaluates)
    float* gt;         // [B][K][2]
    float* conf;       // [B][K]
    float* jw;         // [B][K]
    float* cmask;      // [B][K]
    float* cam;        // [B][8] fx fy cx cy data_weight est_tz - -
    float* camR;       // [B][9]
    float* regpose;    // [B][63]  (or latent)
    float* fd;         // [B][FD_N] the seven arrays above packed per frame (k_pack_fd): what the closure workgroup loads
    float* f;          // [B] loss at Xt
    float* g;          // [B][NVAR_MAX] flat gradient at Xt
    float* bodypose;   // [B][63] decoded body pose (VPoser) scratch
    // dense path
    float* featR;      // [Bpad][KD_PAD]: one 2-KiB row of blend-shape coefficients per GEMM column (frame)
    float* AT;         // [12][JPAD][Bpad]
    float* verts;      // [B][V][3]
    float* joints;     // [B][K][3] (export)
    float* fullpose;   // [B][165]  (export)
    int Bpad;
    int*   slot;       // [B] frame -> operand column / vertex-buffer row (identity or compacted; -1: waiting in the queue)
    int nact;          // columns in use (frames the dense GEMM processes)
    const int* act;    // [nrun] frames the fused dense tick kernel works on (NULL: all B frames, block = frame)
    int nrun;          // length of act[]
    // optimiser state
    int*   stage;      // [B] current stage (-1 camera, 0.. body, n_stages = done)
    void*  opt;        // [B] OptState
    float* vec;        // [B][NVEC][NVAR_MAX] optimiser vectors
    float* hist;       // [B][2][hist_ring + 8][NVAR_MAX]
    int*   n_active;   // [1] frames not done
    float* stage_loss; // [B][1+MAX_STAGES]
    int*   stage_evals;     // [B][1+MAX_STAGES]
    int*   stage_ref_evals; // [B][1+MAX_STAGES]
    float* X0;         // [B][NPAR_MAX] first-orientation result (side-view second fit)
    float* gocam;      // [B][4] global_orient at the end of the camera stage
    float* stage_loss2;// [B][1+MAX_STAGES] second-orientation stage losses
    int*   try_both;   // [B]
    int*   orient_pass;// [B] 0 first fit, 1 second fit running, 2 done
    float* uvp;             // [B][n_uniq][3]  (slot-indexed) blend offsets (v_posed - v_template) of the item vertices, written by the dense GEMM
    float* pen_loss;        // [B] (slot-indexed) unweighted penetration loss of the pending evaluation
    float* pen_dverts;      // [B][V][3] (slot-indexed) its gradient with respect to the vertices
    int gmm_M;              // Gaussian-mixture body pose prior: components (0 = off) ...
    const float* gmm_mean;  // [M][64]
    const float* gmm_prec;  // [M][64][64] symmetrised precisions, rows padded
    const float* gmm_lognw; // [M] log nll_weights
    const float* gmm_csel;  // [M] constant of a component in the selection: -log nll_weights (merged form) | comp_const (per-component form)
    const float* gmm_cadd;  // [M] added to the selected component's value: 0 | -log nll_weights
    float gmm_scale;        // factor of the quadratic form: 0.5 | 1
    float* vposed;          // [B][V][3] (slot-indexed) v_posed of every vertex, written by the dense GEMM when the term is on
    float* adj_G;           // [Bpad][3*Vpad] (slot-indexed) d v_posed = T^T d verts: operand of the adjoint GEMM
    float* adj_part;        // [slices][KD_PAD][Bpad] its per-slice partial sums
    float* pen_dfeat;       // [B][KD_PAD] (slot-indexed) d pen_loss / d feat
    float* pen_dA;          // [B][J][12] (slot-indexed) d pen_loss / d A
    int*   pen_want;        // [B] (slot-indexed) 1 = the column's pending evaluation carries a collision weight
    int*   ext_n;           // [B] (slot-indexed) vertices with a nonzero penetration gradient (diagnostics)
    int*   pen_over;        // [B] (slot-indexed) 1 = the column's latest collision evaluation kept partners by arrival order somewhere
    int*   pen_flag;        // [B] (frame-indexed, sticky over a fit) the frame consumed such an evaluation: not reproducible run to run
    float* fwd;             // [B][SFX_FWD_N] forward state handed from the export pass to the adjoint pass
    long long* dbg;         // [64] phase timestamps of block 0 (NULL = off)
    float4* trace;          // [B][trace_cap] optimiser trace records (NULL = off), see sfx_batch_trace
    int*   trace_n;         // [B] records written
    int    trace_cap;
    int    trace_evals;     // 1: also one record (3, t, loss, |g|inf) per closure evaluation
    // float64 mode (sfx_batch_cfg.high_precision = 2): typed twins of X, Xt, f, g (NULL in modes 0 / 1; a float64 batch keeps
    // the fp32 ones allocated but never writes them) and the camera record -- fx fy cx cy data_weight est_tz - - -- in double
    double* X64;            // [B][NPAR_MAX]
    double* Xt64;           // [B][NPAR_MAX]
    double* f64;            // [B]
    double* g64;            // [B][NVAR_MAX]
    double* cam64;          // [B][8]
    // where the export pass WRITES the GEMM operands.  Everywhere but in the overlapped dense loop (host/fit_loop.hip DenseLoop) these are
    // featR / AT themselves; there the rest-tile GEMM of evaluation i still reads featR / AT while the tick kernel exports
    // evaluation i + 1, so the export goes to another set of buffers and the host rotates the sets after every tick launch
    float* featR_w;         // [Bpad][KD_PAD]
    float* AT_w;            // [12][JPAD][Bpad]
};

enum { VEC_XINIT = 0, VEC_D, VEC_G, VEC_PREVG, VEC_GPREV, VEC_BG0, VEC_BG1, VEC_LSG0, NVEC };

#define SFX_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    sfx_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); return -2; } } while (0)

void sfx_set_error(const char* fmt, ...);

// The one owner of device memory on the host side: a handle (sfx_model, sfx_batch, sfx_pen) or a function's scratch holds one,
// and whatever it handed out is freed when it goes out of scope -- an early return (SFX_CHECK) after it leaks nothing.
struct DevAlloc {
    std::vector<void*> ptrs;
    bool failed = false;        // sticky: any hipMalloc / hipMemcpy / hipMemset of this owner failed (checked once by the creator)
    DevAlloc() = default;
    DevAlloc(const DevAlloc&) = delete;
    DevAlloc& operator=(const DevAlloc&) = delete;
    ~DevAlloc() { clear(); }
    void clear() { for (void* p : ptrs) (void)hipFree(p); ptrs.clear(); }
    template <typename T> T* alloc(size_t count) {      // uninitialised; never a zero-byte request
        T* d = nullptr;
        if (hipMalloc((void**)&d, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) { failed = true; return nullptr; }
        ptrs.push_back(d);
        return d;
    }
    template <typename T> T* zeros(size_t count) {
        T* d = alloc<T>(count);
        if (d && hipMemset(d, 0, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) failed = true;
        return d;
    }
    template <typename T> T* up(const T* h, size_t count) {
        T* d = alloc<T>(count);
        if (d && count && hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) failed = true;
        return d;
    }
    template <typename T> T* up(const std::vector<T>& h) { return up(h.data(), h.size()); }
};

// kernel launchers (defined in the .hip files)
struct ClosureArgs {
    int stage_override;     // -2: use per-frame stage[]; otherwise stage for all frames
    int forward_only;       // 1: export joints / full_pose / featR / AT only
    int use_dense_verts;    // 1: the blend offsets of the item vertices come from the dense GEMM (BatchDev.uvp); 2: dense mode, but the
                            //    workgroup forms them itself from its column of BatchDev.featR (closure_lds.h self_blend_offsets: same bits)
    int export_dense;       // 1: write featR / AT for the dense kernel
    int from_X;             // 1: evaluate at X instead of Xt
    int keep_tables;        // 1: S.meta / S.fd are still valid from the previous evaluation of this workgroup
    int reuse_fwd;          // 1: forward state of this trial point was saved by the export pass
    const float* x_lds;     // the trial point in the workgroup's LDS (k_tick_dense: left there by the optimiser tick); NULL: read X / Xt
    int self_col;           // use_dense_verts = 2: the frame's GEMM column (BatchDev.slot), read by the caller next to the stage
};
// the 47-KB closure variant serves models whose keypoints need at most SFX_SMALL_ITEMS vertex rows
// when the VPoser decoder is not in the loop
static inline bool sfx_small_closure(const DevModel& M, const BatchDev& D) {
    return M.n_items <= SFX_SMALL_ITEMS && !D.cfg.use_vposer;
}
void launch_closure(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW* sw_dev,
                    const ClosureArgs& a, hipStream_t s);
// the float64 closure (body-only needed-rows path: FrameLDSSmall64)
void launch_closure64(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW64* sw_dev,
                      const ClosureArgs& a, hipStream_t s);
// d v_posed = T^T g of the interpenetration gradient, written by the kernel that forms g (k_pen_gather) when the caller is a
// fitting batch: operand of the adjoint GEMM (lbs_adjoint.hip).  adj_G == nullptr: stand-alone operator, nothing to do.
struct PenAdjPrep {
    const float* AT;        // [12][JPAD][Bpad] skinning transforms of the columns (BatchDev.AT)
    const int*   Wsp_j;     // [V][SFX_NW]
    const float* Wsp_w;     // [V][SFX_NW]
    const float* W;         // [V][J] (vertices with more than SFX_NW weights)
    float*       adj_G;     // [Bpad][3 * Vpad]
    int Bpad, Vpad;
};
void launch_pen_adjoint(const DevModel& M, const BatchDev& D, hipStream_t s);
// backward pass of the stand-alone LBS (lbs_backward.hip; sfx_lbs_backward): the adjoint GEMM's operand from a vertex gradient the
// caller supplies (D.pen_dverts -> D.adj_G), the reverse sweep with external upstream (result: the gradient of the parameter
// block, gc [B][SFX_NPAR_MAX]) and its scatter to the nine named gradients
struct LbsGradOut { float *go, *bp, *betas, *expr, *jaw, *leye, *reye, *lh, *rh; };      // device pointers, any may be NULL
void launch_adj_prep(const DevModel& M, const BatchDev& D, hipStream_t s);
void launch_closure_ext(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW* sw_dev, const ClosureArgs& a,
                        const float* djoints, int has_dverts, float* gc, hipStream_t s);
void launch_scatter_gc(const BatchDev& D, const float* gc, const LbsGradOut& o, hipStream_t s);
int sfx_adj_slices(const DevModel& M);
void launch_lbs_dense(const DevModel& M, const BatchDev& D, hipStream_t s);
// the same launch over the n_list tiles of an ascending device list (model_tables.h tile_key / tile_rest) instead of over all
void launch_lbs_dense_list(const DevModel& M, const BatchDev& D, const int* list_dev, int n_list, hipStream_t s);
#ifdef SFX_LAB
extern int g_lbs_dense_form;          // 16 (k_lbs_dense16, default) | 17 (k_lbs_dense16 at every size) | 32 (k_lbs_dense)
#endif
void launch_lbfgs_tick(const DevModel& M, const BatchDev& D, const VarList* vl_dev, int first_stage,
                       int last_stage, int init, int step_mode, hipStream_t s);
size_t sfx_optstate_size();
int debug_two_loop(const float* S, const float* Y, int cnt, int hist_cap, const float* g, float* d_out);   // lbfgs.hip (host pointers)
void launch_fit_rows(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW* sw_dev,
                     int first_stage, int last_stage, int max_ticks, hipStream_t s);
// has_eval: 0 export only | 1 loss + adjoint of the pending evaluation (blend offsets from D.uvp), tick, export | 2 the same with
// self-served blend offsets (nothing of the GEMM of the pending evaluation is read)
void launch_tick_dense(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW* sw_dev,
                       int first_stage, int last_stage, int has_eval, hipStream_t s);
// R <= SFX_TICK_ROUNDS self-served rounds (has_eval = 2) in one launch of k_tick_dense_multi (fused.hip): round r reads operand set
// r and exports to set r + 1, so `sets` names R + 1 of them, the first being the set of the pending evaluation.  Only where
// tick_dense_multi_ok: the launch shape of the eight-wavefront body-only kernel with a workgroup per CU.
#define SFX_TICK_ROUNDS 8
struct TickSets { float* featR[SFX_TICK_ROUNDS + 1]; float* AT[SFX_TICK_ROUNDS + 1]; };
bool tick_dense_multi_ok(const DevModel& M, const BatchDev& D);
void launch_tick_dense_multi(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW* sw_dev,
                             int first_stage, int last_stage, const TickSets& sets, int R, hipStream_t s);
// debug / tests: the self-served blend offsets of every column from the current D.featR, out [B][n_uniq][3] (device)
void launch_uvp_self(const DevModel& M, const BatchDev& D, float* out, hipStream_t s);

// the mesh rasteriser (raster.hip; sfx_render_meshes in host/render.hip): everything of one call, device pointers as the C ABI
// names them.  launch_raster_stage enqueues one kernel of the pipeline for the meshes b0 .. b0 + nb - 1, nb <= RS_GRID_Y.
struct RasterArgs {
    int B, V, F, H, W, n_lights;
    float base[3], light_dir[8][3], light_int[8], znear;      // (8 = SFX_RENDER_MAX_LIGHTS, asserted in raster.hip)
    const float* verts; const int* faces; const int* vf_off; const int* vf_faces;
    const float *rot, *trans, *focal, *center;
    const unsigned char* background;
    unsigned long long* vis; float* vnormal; int* snapped;
    unsigned char* rgba; float* depth; int* tri; float* screen; int* dropped;
};
enum { RS_STAGE_PROJECT = 0, RS_STAGE_VNORMALS, RS_STAGE_COVER, RS_STAGE_RESOLVE, RS_STAGES };
#define RS_GRID_Y 65535      // gridDim.y holds this many meshes
void launch_raster_stage(const RasterArgs& A, int stage, int b0, int nb, hipStream_t s);
