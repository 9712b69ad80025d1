// api.hip -- host layer of libsfx.so: the C ABI of include/sfx.h over the gfx950 kernels.
// Owns HBM residency of the model constants and of every batch's state; the hot loop
// (sfx_batch_fit) is a stream of kernel launches with no host arithmetic and one small
// device->host poll every POLL ticks.
#include "../../include/sfx.h"
#include "sfx_internal.h"
#include "column_pool.h"
#include "model_tables.h"
#include "vposer_pack.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

static thread_local char g_err[1024] = "";
void sfx_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
extern "C" const char* sfx_last_error(void) { return g_err; }
extern "C" const char* sfx_version(void) { return "sfx 0.1.0 (gfx950)"; }

// ---------------------------------------------------------------------------------------
// profiling: HIP-event timing of named kernels on the launch stream
struct ProfAcc { double ms = 0; int64_t n = 0, seen = 0; double units = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> pend; };
static int g_prof = 0;
static int g_prof_every = 1;  // time every N-th launch of a name (events cost a queue packet each)
static int g_unfused = 0;     // debug: run the fitting loop with the stand-alone kernels
static std::map<std::string, ProfAcc> g_acc;
static std::vector<hipEvent_t> g_ev_pool;
static std::mutex g_prof_mu;     // batches may be driven from several host threads (one stream each)

static hipEvent_t ev_get() {
    if (!g_ev_pool.empty()) { hipEvent_t e = g_ev_pool.back(); g_ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr; hipEventCreate(&e); return e;
}
static void prof_flush(ProfAcc& a) {
    for (auto& p : a.pend) {
        hipEventSynchronize(p.second);
        float ms = 0; hipEventElapsedTime(&ms, p.first, p.second);
        a.ms += ms; a.n += 1;
        g_ev_pool.push_back(p.first); g_ev_pool.push_back(p.second);
    }
    a.pend.clear();
}
struct ProfScope {
    const char* name; hipStream_t s; hipEvent_t e0 = nullptr, e1 = nullptr;
    ProfScope(const char* n, hipStream_t st, double units = 0) : name(n), s(st) {
        if (!g_prof) return;
        std::lock_guard<std::mutex> lk(g_prof_mu);
        auto& a = g_acc[name];
        if (a.seen++ % g_prof_every) return;
        a.units += units;
        e0 = ev_get(); e1 = ev_get();
        hipEventRecord(e0, s);
    }
    ~ProfScope() {
        if (!e0) return;
        hipEventRecord(e1, s);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        auto& a = g_acc[name]; a.pend.push_back({e0, e1});
        if (a.pend.size() > 4096) prof_flush(a);
    }
};
// bit 0: time launches with HIP events; bit 1: debug, stand-alone kernels; bits 8..23: time every
// N-th launch of each name only (0/1 = every launch)
extern "C" int sfx_prof_enable(int32_t on) {
    g_prof = on & 1; g_unfused = (on >> 1) & 1;
    const int every = (on >> 8) & 0xffff;
    g_prof_every = every > 1 ? every : 1;
    return 0;
}
extern "C" void sfx_prof_reset(void) { std::lock_guard<std::mutex> lk(g_prof_mu); for (auto& kv : g_acc) { prof_flush(kv.second); } g_acc.clear(); }
// Host side of the polled dense loops since the last reset (HOST [4]): seconds spent enqueueing, seconds spent waiting for a
// batch's stage flags (the GPU was ahead of the host exactly when this is ~0 while the loop's wall time exceeds the kernels'),
// wall seconds of the loops, rounds enqueued.
static double g_loop_host[4] = {0, 0, 0, 0};
extern "C" int sfx_loop_host_stats(double* out, int32_t reset) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (out) for (int i = 0; i < 4; ++i) out[i] = g_loop_host[i];
    if (reset) for (int i = 0; i < 4; ++i) g_loop_host[i] = 0.0;
    return 0;
}
extern "C" int sfx_prof_get(const char* name, double* total_ms, int64_t* launches, double* units) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto it = g_acc.find(name);
    if (it == g_acc.end()) { if (total_ms) *total_ms = 0; if (launches) *launches = 0; if (units) *units = 0; return 0; }
    prof_flush(it->second);
    if (total_ms) *total_ms = it->second.ms;
    if (launches) *launches = it->second.n;
    if (units) *units = it->second.units;
    return (int)std::min<int64_t>(it->second.n, 1 << 30);
}

// ---------------------------------------------------------------------------------------
struct sfx_pen;
extern "C" int sfx_pen_create(int32_t V, int32_t F, const int32_t* faces, const int32_t* segm, const int32_t* parents,
                              const int32_t* ign_pairs, int32_t n_ign, int32_t max_collisions, int32_t max_batch,
                              sfx_pen** out);
extern "C" void sfx_pen_destroy(sfx_pen* h);
extern "C" int sfx_pen_eval(sfx_pen* h, int32_t B, const float* verts_dev, float sigma, int32_t penalize_outside,
                            float* loss_dev, float* dverts_dev, void* stream);
extern "C" int sfx_pen_stats(sfx_pen* h, int32_t B, int32_t* stats_host);
extern "C" int sfx_pen_pairs(sfx_pen* h, int32_t mesh, int32_t cap, int32_t* pairs_host, int32_t* n_out);
int sfx_pen_eval_masked(sfx_pen* h, int32_t B, const float* verts_dev, float sigma, int32_t penalize_outside,
                        float* loss_dev, float* dverts_dev, const int* want_dev, const PenAdjPrep* prep, int* over_dev, void* stream);
int sfx_pen_capacity(const sfx_pen* h);          // meshes per call the handle's buffers hold (collide.hip)
void sfx_pen_note_batch(sfx_pen* h, int B);      // meshes of the evaluation a replayed graph performs
void sfx_pen_reuse(sfx_pen* h);                  // a handle taken from a model's idle slot: per-process settings of the lab build re-read
int sfx_pen_stats_from(const int* stats_dev, int n, int32_t* stats_host);
int sfx_pen_stats_stride(void);
const int* sfx_pen_stats_dev(const sfx_pen* h);

extern "C" void sfx_batch_destroy(sfx_batch* b);
// Who owns what: a model owns its constants (mem), the batch behind sfx_lbs_forward and the idle collision handle; a batch owns
// its state (mem), its trace, pinned poll buffers, events, capture stream, second stream, graphs, and the collision handle while it lives.  Each
// handle releases all of it in its destructor and nowhere else: sfx_*_destroy and every failing exit of sfx_*_create end there.
struct sfx_model {
    DevModel M{};
    DevAlloc mem;
    std::vector<int> faces_host, segm_host, parents_host, ign_host;   // interpenetration set-up
    int NB = 0, NE = 0, NPCA = 0;
    std::vector<int> meta_host;   // DevModel.meta
    const int *tile_key = nullptr, *tile_rest = nullptr;      // the dense GEMM's tiles by consumer (model_tables.h), owned by mem
    int n_key = 0, n_rest = 0;
    sfx_batch* fwd = nullptr;     // lazily created batch behind sfx_lbs_forward
    int fwd_B = 0;
    // The collision buffers of the interpenetration term (~45 MB per GEMM column: 11.5 GB for 256 columns) outlive the batch that
    // used them: a job is a sequence of batches on one model (driver.fit_frames per (gender, H, W) group, bench.py per step), and
    // returning 11 GB to the driver and asking for them again cost 10 ms on some boxes and 450 ms per batch on others (round 6:
    // `outside_loop_ms_per_step` of the --workload pen line, 402 against 239 frames/s for the same kernels).  ONE idle handle is
    // kept per model; it is reused when it holds at least the columns asked for, at the same max_collisions and part table.
    sfx_pen* pen_idle = nullptr;
    int pen_idle_cols = 0, pen_idle_cap = 0, pen_idle_gen = -1;
    int parts_gen = 0;            // bumped by sfx_model_set_parts: handles made for another part table are not reused
    std::mutex pen_mu;
    ~sfx_model() { sfx_batch_destroy(fwd); sfx_pen_destroy(pen_idle); }
};

// The fused dense loop keeps `ahead` batches of 8 rounds queued beyond the one whose stage flags the host is waiting for: the
// GPU only idles when the host thread stays away for longer than that much queued work.  Measured in round 4 (LAB_NOTES §4.6):
// the host's own enqueueing is 4-7 % of the loop (7 us per round of 2 launches, 43 us per round of 13), so a captured graph
// would save nothing on a quiet host; on a host whose 16 cores carry 32 spinning processes EVERY workload halves (body 509 ->
// 239, interpenetration 349 -> 182 frames/s: the polling thread waits milliseconds for a time slice), and a deeper queue buys
// back part of it where a round is two launches (body: 249 / 275 frames/s with 3 / 6 batches ahead) but HURTS where a round
// is thirteen (interpenetration, quiet host: 349 / 322 / 221 frames/s with 1 / 3 / 6 ahead -- hundreds of queued packets).
// Default: 3 batches ahead for the two-launch loops, 1 with the interpenetration term; SFX_POLL_AHEAD overrides.  The price of
// depth: decisions (retirement, admission, compaction, the end) lag by ahead x 8 rounds; finished frames only ever stay
// finished, and the surplus rounds at the end run on empty launches (0.1 % of a 256-frame fit at depth 3).
#define SFX_POLL_BUFS 8
#define SFX_OV_EVENTS 4      // events per ring of the overlapped dense loop: E_G of rounds i, i - 1, i - 2 are alive at once
#ifndef SFX_OV_MAX
#define SFX_OV_MAX 256       // ... and so do rounds at more columns than this: beyond a tick workgroup per CU both kernels fill the chip
#endif
#ifndef SFX_OV_SERIAL
#define SFX_OV_SERIAL 160    // rounds at this many active GEMM columns or fewer stay serial on one stream
#endif
// the self-served form of a round (DenseLoop::round_self; models that export at most SFX_OV_SELF_UNIQ vertices, no interpenetration term):
// rounds at more than SFX_OV_SELF_SERIAL and at most SFX_OV_SELF_MAX active columns; outside that band the rules above hold.
// The band is where the form won the sweep of LAB_NOTES 4.9 (frames/s with the form from n + 1 columns up to 160: n = 0: 620.1,
// 16: 631.6, 32: 635.7, 64: 637.3, 96: 628.5, 128: 616.2, 160 = the key / rest rule alone: 611.8; up to 192 instead of 160:
// +3.7): below 65 columns the GEMM's small workgroups take the CUs the tick chain needs next and the round turns serial again
#ifndef SFX_OV_SELF_SERIAL
#define SFX_OV_SELF_SERIAL 64
#endif
#ifndef SFX_OV_SELF_MAX
#define SFX_OV_SELF_MAX 192
#endif
#define SFX_OV_SELF_UNIQ 16  // one tile of exported vertices: three of the tick workgroup's wavefronts carry one MFMA chain each
struct sfx_batch {
    sfx_model* m = nullptr;
    BatchDev D{};
    DevAlloc mem;
    VarList* vl_dev = nullptr;    // [2]: camera, body
    StageW* sw_dev = nullptr;     // [n_stages]
    VarList vl_host[2];
    int* stage_host = nullptr;    // pinned, [SFX_POLL_BUFS][B]
    int* map_host = nullptr;      // pinned, [SFX_POLL_BUFS][3B]: slot[], running-frame list, newly admitted frames (one upload per batch in flight)
    int* act_dev = nullptr;       // [B] running frames of the fused dense loop
    int* act_new_dev = nullptr;   // [B] frames admitted at the latest poll (export-only launch)
    int slots = 0;                // GEMM columns of the fused dense loop (0: one per frame)
    hipEvent_t poll_ev[SFX_POLL_BUFS] = {};
    // the overlapped dense loop (DenseLoop): the second and third set of GEMM operand buffers (owned by mem; D.featR / D.AT
    // name the set of the most recent evaluation, whichever that is), the stream of the rest-tile GEMMs and the two rings of events that
    // order them against the tick kernels; stream and events are made by the first fit that overlaps
    float *featR_o[2] = {nullptr, nullptr}, *AT_o[2] = {nullptr, nullptr};      // [0] the next export's target, [1] the one after
    hipStream_t s2 = nullptr;
    hipEvent_t ov_ev[2][SFX_OV_EVENTS] = {};
    int K = 0;
    sfx_pen* pen = nullptr;       // interpenetration operator (cfg.interpenetration)
    float pen_sigma = 0.f; int pen_outside = 1;
    int pen_cols = 0, pen_cap = 0, pen_gen = -1;       // what b->pen was made for (returned to the model's idle slot on destroy)
    // the interpenetration step of a round of the fused loop as ONE captured graph per column count (twelve kernels; the count
    // only changes when the columns are compacted -- a handful of times per fit): one API call per round instead of twelve
    std::map<int, hipGraphExec_t> pen_graphs;
    int pen_graph_nodes = 0;       // kernel nodes of the most recently captured interpenetration step (sfx_batch_pen_launches)
    hipStream_t cap_stream = nullptr;   // capture happens on a stream of its own (the caller's may be the legacy NULL stream, which cannot capture)
    int* pen_stats_all = nullptr; // [B][stride] diagnostics of a CHUNKED evaluation (stand-alone call on a pooled batch), else unused
    bool pen_chunked = false;     // the most recent evaluation was chunked: sfx_batch_pen_stats reads pen_stats_all
    bool f64 = false;             // float64 mode (high_precision = 2): X, Xt, f, g hold doubles, closures run k_closure64
    StageW64* sw64_dev = nullptr; // [n_stages] its stage weights
    DevAlloc trace_mem;           // D.trace / D.trace_n (sfx_batch_trace)
    long long* dbg_buf = nullptr; // [64] clock buffer of the lab build (sfx_debug_clocks attaches it as D.dbg), owned by mem
    // sfx_lbs_backward (the model's forward batch only), allocated by its first call and owned by mem: the parameter block's
    // gradient, and -- first call with a vertex gradient -- what the adjoint of a gradient on every vertex needs.  They are NOT
    // attached to D: the forward keeps launching what it launched (a non-NULL D.vposed makes the dense GEMM write it).
    float* bwd_gc = nullptr;      // [B][SFX_NPAR_MAX]
    struct { float *vposed, *adj_G, *adj_part, *dfeat, *dA; int* want; } bwd = {};      // as BatchDev's members of the interpenetration term
    ~sfx_batch() {
        for (auto& kv : pen_graphs) hipGraphExecDestroy(kv.second);
        if (cap_stream) hipStreamDestroy(cap_stream);
        if (s2) { (void)hipStreamSynchronize(s2); hipStreamDestroy(s2); }      // (DenseLoop::run drains it on every way out: nothing is pending)
        for (auto& ring : ov_ev) for (hipEvent_t e : ring) if (e) hipEventDestroy(e);
        if (pen) {             // the collision buffers go back to the model's idle slot (see sfx_model)
            (void)hipDeviceSynchronize();
            std::lock_guard<std::mutex> lk(m->pen_mu);
            if (pen_gen == m->parts_gen && (!m->pen_idle || m->pen_idle_cols <= pen_cols)) {
                sfx_pen_destroy(m->pen_idle);
                m->pen_idle = pen; m->pen_idle_cols = pen_cols; m->pen_idle_cap = pen_cap; m->pen_idle_gen = pen_gen;
            } else sfx_pen_destroy(pen);
        }
        if (stage_host) hipHostFree(stage_host);
        if (map_host) hipHostFree(map_host);
        for (hipEvent_t e : poll_ev) if (e) hipEventDestroy(e);
    }
};

// The float64 mode's guards.  Float inputs to a float64 batch are widened; float OUTPUTS are refused, so that no result is
// silently rounded, and so is everything the mode does not have (the device optimiser, the dense path, the GMM prior).
static int refuse_f64(const sfx_batch* b, const char* fn) {
    if (b && b->f64) {
        sfx_set_error("%s: not available on a float64 batch (high_precision = 2): use the _f64 entry points", fn); return -1; }
    return 0;
}
static int need_f64(const sfx_batch* b, const char* fn) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (!b->f64) { sfx_set_error("%s: the batch is not in float64 mode (high_precision = 2)", fn); return -1; }
    return 0;
}
// values the float64 mode keeps in fp32 tables (keypoints, weights, masks, camera rotation, regression pose): exact or refused
static bool fp32_exact(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!((double)(float)v[i] == v[i]) && !std::isnan(v[i])) return false;
    return true;
}

extern "C" int sfx_model_create(const sfx_model_desc* d, sfx_model** out) {
    if (!d || !out) { sfx_set_error("null argument"); return -1; }
    if (d->J != SFX_J) { sfx_set_error("only J=55 (SMPL-X) is supported, got %d", d->J); return -1; }
    const int V = d->V, S = d->num_betas + d->num_expr, KD = S + 9 * (d->J - 1);
    if (KD > SFX_KD_PAD) { sfx_set_error("blend-shape depth %d unsupported", KD); return -1; }
    if (d->K > SFX_MAX_K) { sfx_set_error("K=%d > %d", d->K, SFX_MAX_K); return -1; }
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        sfx_set_error("no HIP device: libsfx has no CPU fallback"); return -3;
    }
    ModelTables T;
    if (int rc = sfx_build_model_tables(d, &T)) return rc;      // every refusal: before the first device allocation
    std::unique_ptr<sfx_model> m(new sfx_model());
    DevModel& M = m->M;
    DevAlloc& mem = m->mem;
    m->NB = d->num_betas; m->NE = d->num_expr; m->NPCA = d->num_pca;
    M.V = V; M.S = S; M.K = d->K; M.n_dyn = d->n_dyn; M.Vpad = T.Vpad; M.n_rounds = T.n_rounds;
    M.n_items = T.n_items; M.n_static_items = T.n_static_items; M.n_uniq = T.n_uniq; M.n_sj = T.n_sj; M.n_dyn_items = T.n_dyn_items;
    M.v_template = mem.up(d->v_template, (size_t)V * 3);
#ifdef SFX_LAB
    M.dirs = mem.up(T.dirs);
#endif
    M.dirsT = mem.up(T.dirsT); M.dirs_tiled = mem.up(T.dirs_tiled);
    M.Wsp_j = mem.up(T.Wsp_j); M.Wsp_w = mem.up(T.Wsp_w);
    M.jv_start = mem.up(T.jv_start); M.jv_vid = mem.up(T.jv_vid); M.jv_w = mem.up(T.jv_w);
    M.W = mem.up(d->lbs_weights, (size_t)V * SFX_J);
    M.tj_n = mem.up(T.tj_n); M.tj_list = mem.up(T.tj_list); M.tj_w = mem.up(T.tj_w);
    M.J_template = mem.up(T.J_template); M.J_dirs = mem.up(T.J_dirs);
    M.J_template64 = mem.up(T.J_template64); M.J_dirs64 = mem.up(T.J_dirs64);
    M.comp_l = mem.up(d->hands_comp_l, (size_t)d->num_pca * SFX_NHAND); M.comp_r = mem.up(d->hands_comp_r, (size_t)d->num_pca * SFX_NHAND);
    M.pose_mean = mem.up(d->pose_mean, SFX_POSE);
    M.sj_start = mem.up(T.sj_start); M.sj_item = mem.up(T.sj_item); M.sj_w = mem.up(T.sj_w);
    M.dj_start = mem.up(T.dj_start); M.dj_item = mem.up(T.dj_item); M.dj_w = mem.up(T.dj_w);
    M.dynp_vid = mem.up(T.dynp_vid); M.dynp_w = mem.up(T.dynp_w); M.dynp_vt = mem.up(T.dynp_vt);
    M.dynp_wj = mem.up(T.dynp_wj); M.dynp_ww = mem.up(T.dynp_ww);
    M.dynp_js = T.dynp_js.empty() ? nullptr : mem.up(T.dynp_js);
    M.dynp_ji = mem.up(T.dynp_ji); M.dynp_jw = mem.up(T.dynp_jw);
    M.item_vid = mem.up(T.item_vid); M.item_w = mem.up(T.item_w);
    M.item_vt = mem.up(T.item_vt); M.item_wj = mem.up(T.item_wj); M.item_ww = mem.up(T.item_ww);
    M.dynp_us = T.dynp_us.empty() ? nullptr : mem.up(T.dynp_us);
    M.vslot = mem.up(T.vslot); M.item_uslot = mem.up(T.item_uslot); M.uniq_dirs = mem.up(T.uniq_dirs);
    M.meta = mem.up(T.meta);
    m->tile_key = mem.up(T.tile_key); m->tile_rest = mem.up(T.tile_rest);
    m->n_key = (int)T.tile_key.size(); m->n_rest = (int)T.tile_rest.size();
    m->meta_host = std::move(T.meta); m->faces_host = std::move(T.faces);
    if (mem.failed) { (void)hipGetLastError(); sfx_set_error("out of device memory (model constants)"); return -2; }
    if (hipDeviceSynchronize() != hipSuccess) { sfx_set_error("model upload failed"); return -2; }
    *out = m.release();
    return 0;
}

extern "C" void sfx_model_destroy(sfx_model* m) { delete m; }

extern "C" int sfx_model_set_parts(sfx_model* m, const int32_t* segm, const int32_t* parents, const int32_t* ign_pairs,
                                   int32_t n_ign) {
    if (!m) { sfx_set_error("null argument"); return -1; }
    { std::lock_guard<std::mutex> lk(m->pen_mu); ++m->parts_gen; if (m->pen_idle) { sfx_pen_destroy(m->pen_idle); m->pen_idle = nullptr; } }
    if (!segm && !parents) {        // no FilterFaces module (fit_single_frame.py:316 without part_segm_fn): no pair is filtered by part
        m->segm_host.clear(); m->parents_host.clear(); m->ign_host.clear();
        return 0;
    }
    if (!segm || !parents) { sfx_set_error("null argument"); return -1; }
    const size_t F = m->faces_host.size() / 3;
    m->segm_host.assign(segm, segm + F);
    m->parents_host.assign(parents, parents + F);
    m->ign_host.clear();
    if (ign_pairs && n_ign > 0) m->ign_host.assign(ign_pairs, ign_pairs + (size_t)2 * n_ign);
    return 0;
}

extern "C" int sfx_model_set_vposer(sfx_model* m, int32_t latent, int32_t hidden, const float* w1, const float* b1,
                                    const float* w2, const float* b2, const float* w3, const float* b3) {
    if (!m) { sfx_set_error("null model"); return -1; }
    if (!vposer_shape_ok(latent, hidden)) return -1;
    auto v = [](const float* p, size_t n) { return std::vector<float>(p, p + n); };
    const int H = hidden, L = latent;
    VposerPack P;
    vposer_pack(L, H, w1, w2, w3, P);
    m->M.vp_latent = latent; m->M.vp_hidden = hidden;
    m->M.vp_w1 = m->mem.up(v(w1, (size_t)H * L)); m->M.vp_b1 = m->mem.up(v(b1, H));
    m->M.vp_w2 = m->mem.up(v(w2, (size_t)H * H)); m->M.vp_b2 = m->mem.up(v(b2, H));
    m->M.vp_w3 = m->mem.up(v(w3, (size_t)126 * H)); m->M.vp_b3 = m->mem.up(v(b3, 126));
    m->M.vp_w1T = m->mem.up(P.w1T); m->M.vp_w2T = m->mem.up(P.w2T); m->M.vp_w3T = m->mem.up(P.w3T);
    if (m->mem.failed) { (void)hipGetLastError(); m->M.vp_latent = 0; sfx_set_error("out of device memory (VPoser weights)"); return -2; }
    if (m->fwd) { sfx_batch_destroy(m->fwd); m->fwd = nullptr; }
    return 0;
}

// ---------------------------------------------------------------------------------------
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
    if (c->lbs_mode == 1 && !D.cfg.pen) {
        for (int i = 0; i < 2; ++i) {
            b->featR_o[i] = b->mem.zeros<float>((size_t)SFX_KD_PAD * D.Bpad);
            b->AT_o[i] = b->mem.zeros<float>((size_t)12 * SFX_JPAD * D.Bpad);
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
        {
            std::lock_guard<std::mutex> lk(m->pen_mu);
            if (m->pen_idle && m->pen_idle_cols >= pen_cols && m->pen_idle_cap == pen_cap && m->pen_idle_gen == m->parts_gen) {
                b->pen = m->pen_idle; b->pen_cols = m->pen_idle_cols;
                m->pen_idle = nullptr;
                sfx_pen_reuse(b->pen);
            } else if (m->pen_idle) { sfx_pen_destroy(m->pen_idle); m->pen_idle = nullptr; }      // too small / another table: make room first
        }
        if (!b->pen) {
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
static void pack_fd(sfx_batch* b, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_fd, dim3(b->D.cfg.B), dim3(128), 0, s, b->D, b->K);
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
        std::vector<float> c8((size_t)B * 8, 0.f);
        for (int i = 0; i < B; ++i) for (int q = 0; q < 6; ++q) c8[(size_t)i * 8 + q] = cam[(size_t)i * 6 + q];
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
        ClosureArgs a{}; a.stage_override = 0; a.forward_only = 1; a.from_X = 1;
        launch_closure(b->m->M, b->D, b->vl_dev, b->sw_dev, a, 0);
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
        std::vector<double> d8((size_t)B * 8, 0.0);
        for (int i = 0; i < B; ++i) for (int q = 0; q < 6; ++q) d8[(size_t)i * 8 + q] = cam[(size_t)i * 6 + q];
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
//   closure_lds.h self_blend_offsets on the current "feat": one launch of k_uvp_self into a scratch buffer)
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

// Stand-alone operator: the direction the device's blocked two-loop recursion (lbfgs_body.h lb_two_loop) computes from a history of `count`
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

extern "C" int sfx_batch_num_vars(sfx_batch* b, int32_t stage) {
    if (!b) return -1;
    return b->vl_host[stage < 0 ? 0 : 1].n;
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

// Upper bound on the rounds a fit can take (a guard against a loop that never ends, not a budget): an LBFGS.step costs at most
// max_eval evaluations in its iterations plus one line search that may run over -- the bracket phase up to 25 evaluations, the zoom
// phase up to LBFGS(max_iter) (lbfgs_ls.py:108) -- plus the entry evaluation; a side view is fitted from two orientations
// (fit_single_frame.py:527-551), accounted for as a factor of its own (the old bound let the `* 2` do both).
static long sfx_fit_tick_bound(const BatchCfgDev& c, int first_stage, int last_stage) {
    const long per_step = (long)c.max_eval + std::max(25, (int)c.lbfgs_max_iter) + 1;
    return (long)(last_stage - first_stage + 1) * c.maxiters * std::max(80L, per_step + 7) * 2 /* orientations */ * 2 /* slack */ + 64;
}

// want_ready: the fused tick kernel maintains pen_want[] itself (it knows every running frame's next stage when it exports
// the next trial point, and clears the flag of a frame that finishes): no launch for it inside the fitting loop
static int eval_penetration(sfx_batch* b, int stage_override, hipStream_t s, bool want_ready = false) {
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

static int eval_closure(sfx_batch* b, int stage_override, int from_X, hipStream_t s) {
    const DevModel& M = b->m->M; const BatchDev& D = b->D;
    ClosureArgs a{};
    a.stage_override = stage_override; a.from_X = from_X;
    // the camera stage asks for return_verts=False (fit_single_frame.py:485): the reference
    // still evaluates every vertex there, so dense mode does too.
    if (D.cfg.lbs_mode == 1) {
        ClosureArgs e = a; e.export_dense = 1; e.forward_only = 2;
        { ProfScope p("export", s); launch_closure(M, D, b->vl_dev, b->sw_dev, e, s); }
        { ProfScope p("lbs_dense", s, D.nact); launch_lbs_dense(M, D, s); }
        if (int rc = eval_penetration(b, stage_override, s)) return rc;
        a.use_dense_verts = 1;
    }
    ProfScope p("closure", s);
    launch_closure(M, D, b->vl_dev, b->sw_dev, a, s);
    return 0;
}

extern "C" int sfx_batch_closure(sfx_batch* b, int32_t stage, float* loss_out, float* grad_out, void* stream) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_batch_closure")) return -1;
    if (stage >= b->D.cfg.n_stages) { sfx_set_error("stage %d out of range", stage); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (int rc = eval_closure(b, stage < 0 ? -1 : stage, 1, s)) return rc;
    SFX_CHECK(hipStreamSynchronize(s));
    SFX_CHECK(hipGetLastError());
    const int B = b->D.cfg.B, N = b->vl_host[stage < 0 ? 0 : 1].n;
    if (loss_out) SFX_CHECK(hipMemcpy(loss_out, b->D.f, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (grad_out) {
        std::vector<float> g((size_t)B * SFX_NVAR_MAX);
        SFX_CHECK(hipMemcpy(g.data(), b->D.g, g.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < B; ++i) memcpy(grad_out + (size_t)i * N, &g[(size_t)i * SFX_NVAR_MAX], (size_t)N * 4);
    }
    return 0;
}

extern "C" int sfx_batch_closure_f64(sfx_batch* b, int32_t stage, double* loss_out, double* grad_out, void* stream) {
    if (need_f64(b, "sfx_batch_closure_f64")) return -1;
    if (stage >= b->D.cfg.n_stages) { sfx_set_error("stage %d out of range", stage); return -1; }
    hipStream_t s = (hipStream_t)stream;
    ClosureArgs a{};
    a.stage_override = stage < 0 ? -1 : stage; a.from_X = 1;
    { ProfScope p("closure", s); launch_closure64(b->m->M, b->D, b->vl_dev, b->sw64_dev, a, s); }
    SFX_CHECK(hipStreamSynchronize(s));
    SFX_CHECK(hipGetLastError());
    const int B = b->D.cfg.B, N = b->vl_host[stage < 0 ? 0 : 1].n;
    if (loss_out) SFX_CHECK(hipMemcpy(loss_out, b->D.f64, (size_t)B * 8, hipMemcpyDeviceToHost));
    if (grad_out) {
        std::vector<double> g((size_t)B * SFX_NVAR_MAX);
        SFX_CHECK(hipMemcpy(g.data(), b->D.g64, g.size() * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < B; ++i) memcpy(grad_out + (size_t)i * N, &g[(size_t)i * SFX_NVAR_MAX], (size_t)N * 8);
    }
    return 0;
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
    ClosureArgs a{}; a.stage_override = -1; a.forward_only = 1; a.from_X = 1;
    launch_closure(b->m->M, b->D, b->vl_dev, b->sw_dev, a, s);
    hipLaunchKernelGGL(k_guess_init, dim3((b->D.cfg.B + 63) / 64), dim3(64), 0, s, b->D, b->K, pd, n_pairs);
    pack_fd(b, s);          // (est_tz changed)
    SFX_CHECK(hipStreamSynchronize(s));
    SFX_CHECK(hipGetLastError());
    return 0;
}

// Measurement switches of the lab build (include/sfx_lab.h), read once by the first dense fit: diagnostics to stderr, polling
// cadence, the form of a dense round.  The product build has the defaults as constants.
struct DenseSwitches {
    bool dbg_nact = false, dbg_host = false;
    int rpb = 0, ahead = 0;                                                 // 0: the loop's own 8 rounds per batch, 3 / 1 batches ahead
    bool ov_on = true, self_on = true, self_in_serial = false;
    int ov_serial = SFX_OV_SERIAL, self_serial = SFX_OV_SELF_SERIAL, self_max = SFX_OV_SELF_MAX;
};
static const DenseSwitches& dense_switches() {
#ifdef SFX_LAB
    static const DenseSwitches w = [] {
        const auto num = [](const char* name, int unset) { const char* e = getenv(name); return e && *e ? atoi(e) : unset; };
        DenseSwitches v;
        v.dbg_nact = getenv("SFX_DEBUG_NACT") != nullptr; v.dbg_host = getenv("SFX_DEBUG_HOST") != nullptr;
        v.rpb = num("SFX_POLL_ROUNDS", 0); v.ahead = num("SFX_POLL_AHEAD", 0);
        v.ov_on = num("SFX_DENSE_OVERLAP", 1) != 0; v.self_on = num("SFX_DENSE_SELF", 1) != 0; v.self_in_serial = num("SFX_DENSE_SELF_SERIAL", 0) != 0;
        v.ov_serial = num("SFX_OVERLAP_SERIAL", SFX_OV_SERIAL); v.self_max = num("SFX_DENSE_SELF_MAX", SFX_OV_SELF_MAX);
        v.self_serial = num("SFX_OVERLAP_SERIAL", SFX_OV_SELF_SERIAL);      // (SFX_OVERLAP_SERIAL: whichever form is selected)
        return v;
    }();
#else
    static constexpr DenseSwitches w{};
#endif
    return w;
}

namespace {
// Dense fused loop, polled one batch of rounds AHEAD: while the host waits for the stage flags copied after rounds 8i .. 8i+7,
// rounds 8i+8 .. 8i+15 are already queued, so the GPU never idles on the host round trip.  A decision (all done / admission /
// compaction) therefore lags by 8 rounds: finished frames only ever stay finished, so that is safe; the surplus rounds at the
// end find nothing to do.  Frames beyond cfg.slots columns queue for the column of a frame that finishes (column_pool.h).
//
// A round is one GEMM and one tick launch, in one of three forms (round_serial, round_key_rest, round_self).  The two overlapped
// forms run over THREE sets of operand buffers: cur = D.featR / D.AT, nxt = b->featR_o[0] / AT_o[0], and the set the GEMM of the
// round before may still be reading, b->featR_o[1] / AT_o[1]; the host rotates them after every tick launch (the kernels take
// BatchDev by value and know no parity).  T(i) overwrites what the GEMM of round i-2 read, hence its wait, which never blocks in
// practice: with two sets T(i) had to wait for Gr(i-1) and then raced Gr(i) for the CUs -- a tick workgroup needs 300 to 512
// registers per SIMD free and starves behind the GEMM's small workgroups (measured: 99 instead of 46 us per tick launch at 256
// frames, no gain).  With three, T(i) is queued while Gr(i-1) drains and takes the CUs as they empty; Gr(i) fills what is left.
// A finished frame's workgroup copies its column of cur to nxt for as long as it is listed (fused.hip).  Admission and
// compaction exports write cur IN PLACE once s has waited for the latest Gr -- the columns of the frames that keep running hold
// their pending evaluation in cur only.  Two records and two waits per round; no other cross-stream traffic.
struct DenseLoop {
    sfx_batch* const b; const hipStream_t s; const int first_stage, last_stage;
    BatchDev& D = b->D; const DevModel& M = b->m->M; const int B = D.cfg.B;
    bool overlap = false, self_form = false;            // a second stream and operand sets to overlap on; the model may serve itself
    hipEvent_t last_G = nullptr, prev_G = nullptr;     // E_G of the latest overlapped round and of the one before (NULL: s has waited for it)
    hipEvent_t last_T = nullptr;                       // E_T of the latest self-served round (NULL: the latest round was of another form)
    long ov_i = 0, tick = 0;                           // overlapped rounds (their slot in the event rings), rounds
    ColumnPool pool;
    int upl = 0, rpb = 8;                              // next upload buffer, rounds per polled batch
    // how much of the loop's wall time the HOST spends enqueueing (its headroom against a busy box) and waiting for stage flags
    double host_enq_s = 0.0, host_wait_s = 0.0; long host_batches = 0;
    static inline long nact_hist[9] = {};              // rounds by active GEMM columns: <=32, <=64, ..., <=256, more (cumulative)
    void tick_kernel(const char* name, const BatchDev& Dx, int has_eval) {
        ProfScope p(name, s, Dx.nrun);
        launch_tick_dense(M, Dx, b->vl_dev, b->sw_dev, first_stage, last_stage, has_eval, s);
    }
    int join_s2() {                                     // before s writes operands in place: every Gr has read them
        if (last_G) SFX_CHECK(hipStreamWaitEvent(s, last_G, 0));
        last_G = prev_G = nullptr;
        return 0;
    }
    int upload(const std::vector<int>* fresh) {         // slot[], running list (+ admitted list) through pinned memory
        const std::vector<int>& run = pool.run;
        int* h = b->map_host + (size_t)upl * 3 * B; upl = (upl + 1) % SFX_POLL_BUFS;      // (at most one upload per processed batch, at most `ahead` + 1 batches in flight)
        memcpy(h, pool.col.data(), (size_t)B * sizeof(int));
        memcpy(h + B, run.data(), run.size() * sizeof(int));
        SFX_CHECK(hipMemcpyAsync(D.slot, h, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
        if (!run.empty()) SFX_CHECK(hipMemcpyAsync(b->act_dev, h + B, run.size() * sizeof(int), hipMemcpyHostToDevice, s));
        if (fresh && !fresh->empty()) {
            memcpy(h + 2 * B, fresh->data(), fresh->size() * sizeof(int));
            SFX_CHECK(hipMemcpyAsync(b->act_new_dev, h + 2 * B, fresh->size() * sizeof(int), hipMemcpyHostToDevice, s));
        }
        D.act = b->act_dev; D.nrun = (int)run.size();
        return 0;
    }
    // the tail of both overlapped forms: s waits for E_G(i-2), T(i) exports evaluation i + 1 to nxt, the operand sets rotate
    int tick_beside(hipEvent_t e_G, int has_eval) {
        if (prev_G) SFX_CHECK(hipStreamWaitEvent(s, prev_G, 0));
        prev_G = last_G; last_G = e_G;
        BatchDev Dt = D; Dt.featR_w = b->featR_o[0]; Dt.AT_w = b->AT_o[0];
        tick_kernel("tick", Dt, has_eval);
        float* const f = D.featR; D.featR = b->featR_o[0]; b->featR_o[0] = b->featR_o[1]; b->featR_o[1] = f;
        float* const a = D.AT; D.AT = b->AT_o[0]; b->AT_o[0] = b->AT_o[1]; b->AT_o[1] = a;
        D.featR_w = D.featR; D.AT_w = D.AT;
        return 0;
    }
    // Self-served form (models that export at most SFX_OV_SELF_UNIQ vertices: body-only keypoints).  The tick workgroup forms the
    // blend offsets of its keypoint vertices itself, from its column of cur with the GEMM's own chain of operations
    // (closure_lds.h self_blend_offsets: has_eval = 2), so the tick of evaluation i waits for no GEMM launch at all and the WHOLE
    // GEMM of every evaluation runs beside the tick chain:
    //     stream s :  wait E_G(i-2) | T(i) reads cur, exports evaluation i + 1 to nxt | record E_T(i)
    //     stream s2:  wait E_T(i-1) | G(i) all tiles, reads cur | record E_G(i)
    // Every evaluation still gets exactly one whole-mesh GEMM (it goes on writing D.uvp, which nobody reads in these rounds).
    // The first such round after anything else on s records its own E_T at its start.  E_T lives in ring 0, whose events the
    // key / rest form records and waits for at once: a wait holds the record it was enqueued behind, so slot k + 1 of this
    // round is free again when round i + 4 records it.
    int round_self() {
        const int k = (int)(ov_i++ % SFX_OV_EVENTS);
        if (!last_G || !last_T) { SFX_CHECK(hipEventRecord(b->ov_ev[0][k], s)); last_T = b->ov_ev[0][k]; }
        SFX_CHECK(hipStreamWaitEvent(b->s2, last_T, 0));
        { ProfScope p("lbs_dense", b->s2, D.nact); launch_lbs_dense(M, D, b->s2); }
        SFX_CHECK(hipEventRecord(b->ov_ev[1][k], b->s2));
        if (int rc = tick_beside(b->ov_ev[1][k], 2)) return rc;
        last_T = b->ov_ev[0][(k + 1) % SFX_OV_EVENTS];
        SFX_CHECK(hipEventRecord(last_T, s));
        return 0;
    }
    // GEMM beside tick.  Of the GEMM of evaluation i the tick kernel reads D.uvp only -- the blend offsets of the keypoint
    // vertices: the key tiles, a twentieth of the mesh body-only:
    //     stream s :  Gk(i) key tiles, reads cur | record E_K(i) | wait E_G(i-2) | T(i) reads uvp, exports evaluation i + 1 to nxt
    //     stream s2:  wait E_K(i) | Gr(i) every other tile, reads cur | record E_G(i)
    // Gr(i) waits for Gk(i), not only for T(i-1): beside Gk it would slow the round's critical path.  After a self-served round
    // the loop joins first: Gk(i) on s and G(i-1) on s2 both write the key tiles of D.verts.
    int round_key_rest() {
        if (last_T) { if (int rc = join_s2()) return rc; last_T = nullptr; }
        const int k = (int)(ov_i++ % SFX_OV_EVENTS);
        if (b->m->n_key) { ProfScope p("lbs_dense_key", s, D.nact); launch_lbs_dense_list(M, D, b->m->tile_key, b->m->n_key, s); }
        SFX_CHECK(hipEventRecord(b->ov_ev[0][k], s));
        SFX_CHECK(hipStreamWaitEvent(b->s2, b->ov_ev[0][k], 0));
        { ProfScope p("lbs_dense", b->s2, D.nact); launch_lbs_dense_list(M, D, b->m->tile_rest, b->m->n_rest, b->s2); }
        SFX_CHECK(hipEventRecord(b->ov_ev[1][k], b->s2));
        return tick_beside(b->ov_ev[1][k], 1);
    }
    // Everything on s: whole-grid GEMM, the interpenetration step (which needs every vertex before the tick), tick.
    int round_serial() {
        if (int rc = join_s2()) return rc;
        last_T = nullptr;
        { ProfScope p("lbs_dense", s, D.nact); launch_lbs_dense(M, D, s); }
        if (int rc = eval_penetration(b, -2, s, true)) return rc;
        tick_kernel("tick", D, (dense_switches().self_in_serial && !b->pen && M.n_uniq <= SFX_OV_SELF_UNIQ) ? 2 : 1);
        return 0;
    }
    // One polled batch: rpb rounds, each in the form its count of active columns selects, then the stage flags to poll buffer
    // `buf`.  Self-served at SFX_OV_SELF_SERIAL < columns <= SFX_OV_SELF_MAX: the band where the form won (LAB_NOTES 4.9).
    // Key / rest at SFX_OV_SERIAL < columns <= SFX_OV_MAX (LAB_NOTES "GEMM beside tick"): below, a short rest GEMM saves less
    // than it costs the tick kernel it runs beside (frames/s by threshold: 32: 581, 96: 597, 160: 605, 192: 603; serial loop
    // 563); above, 1 024 frames through the 512-column pool lost 6 % overlapped: two tick workgroups per CU and a GEMM that fills
    // the chip leave nothing to share.  The eight-wavefront tick kernel at every size (the four-wavefront one shares its CU with
    // GEMM workgroups and then takes 101 instead of 58 us per launch).
    int rounds(int buf) {
        const DenseSwitches& sw = dense_switches();
        if (sw.dbg_nact) nact_hist[std::min(8, (D.nact - 1) / 32)] += rpb;
        const auto h0 = std::chrono::steady_clock::now();
        for (int q = 0; q < rpb; ++q, ++tick) {
            const int rc = self_form && D.nact > sw.self_serial && D.nact <= sw.self_max ? round_self()
                         : overlap && D.nact > sw.ov_serial && D.nact <= SFX_OV_MAX      ? round_key_rest() : round_serial();
            if (rc) return rc;
        }
        SFX_CHECK(hipMemcpyAsync(b->stage_host + (size_t)buf * B, D.stage, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
        SFX_CHECK(hipEventRecord(b->poll_ev[buf], s));
        host_enq_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - h0).count(); ++host_batches;
        return 0;
    }
    // Wait for poll buffer `cur`; retire the frames that have finished, admit queued ones to their columns; once the queue is
    // dry, compact the columns whenever a slice has emptied.
    int poll(int cur, bool& done) {
        const auto w0 = std::chrono::steady_clock::now();
        SFX_CHECK(hipEventSynchronize(b->poll_ev[cur]));
        host_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
        std::vector<int> fresh;
        const bool changed = pool.retire(b->stage_host + (size_t)cur * B, last_stage, fresh);
        done = pool.run.empty();
        if (done || !changed) return 0;
        if (!fresh.empty()) {
            // admission: the new frames inherit the freed columns; only they need an export pass (one extra launch)
            if (int rc = join_s2()) return rc;
            if (int rc = upload(&fresh)) return rc;
            BatchDev Dn = D; Dn.act = b->act_new_dev; Dn.nrun = (int)fresh.size();
            tick_kernel("tick_admit", Dn, 0);
        } else if (ColumnPool::slice_emptied(D.nact, (int)pool.run.size())) {
            // The pending evaluation of every running frame lives in column slot[f] of featR / AT, so re-export after
            // remapping (queued behind the rounds already in flight, which still use the old mapping consistently).
            D.nact = pool.compact();
            if (int rc = join_s2()) return rc;
            if (int rc = upload(nullptr)) return rc;
            tick_kernel("tick", D, 0);
        } else if (int rc = upload(nullptr)) return rc;      // shorter running list: fewer workgroups per tick launch
        return 0;
    }
    int run(long max_ticks, bool& done) {
        const DenseSwitches& sw = dense_switches();
        overlap = sw.ov_on && !b->pen && b->featR_o[0] && b->featR_o[1] && b->AT_o[0] && b->AT_o[1];
        if (overlap && !b->s2) {
            int lo = 0, hi = 0;
            SFX_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));         // (lowest priority: the key tiles and the tick are the round's critical path)
            SFX_CHECK(hipStreamCreateWithPriority(&b->s2, hipStreamNonBlocking, lo));
            for (auto& ring : b->ov_ev) for (hipEvent_t& e : ring) SFX_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        self_form = overlap && sw.self_on && M.n_uniq <= SFX_OV_SELF_UNIQ;
        {
            // every way out of this block leaves both streams drained and the export pointed back at D.featR / D.AT
            struct OvDrain { sfx_batch* b; hipStream_t s;
                             ~OvDrain() { if (b->s2) (void)hipStreamSynchronize(b->s2); (void)hipStreamSynchronize(s); b->D.featR_w = b->D.featR; b->D.AT_w = b->D.AT; } } ov_drain{b, s};
            const int ncol = b->slots > 0 ? std::min(b->slots, B) : B;
            pool.reset(B, ncol);
            D.nact = ncol;
            if (int rc = upload(nullptr)) return rc;
            tick_kernel("tick", D, 0);
            const double wall0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
            rpb = std::max(1, std::min(64, sw.rpb > 0 ? sw.rpb : 8));
            const int ahead = std::max(1, std::min(SFX_POLL_BUFS - 1, sw.ahead > 0 ? sw.ahead : (b->pen ? 1 : 3)));
            long q_head = 0, q_next = 0;       // batches processed / queued
            for (; q_next < ahead; ++q_next) if (int rc = rounds((int)(q_next % SFX_POLL_BUFS))) return rc;
            while (!done && tick < max_ticks + (long)rpb * (ahead + 1)) {
                if (int rc = rounds((int)(q_next++ % SFX_POLL_BUFS))) return rc;
                if (int rc = poll((int)(q_head++ % SFX_POLL_BUFS), done)) return rc;
            }
            if (b->s2) SFX_CHECK(hipStreamSynchronize(b->s2));
            SFX_CHECK(hipStreamSynchronize(s));
            D.act = nullptr; D.nrun = 0;
            const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - wall0;
            {   // the host's side of this loop, accumulated for sfx_loop_host_stats (bench.py reports it next to the kernels' times)
                std::lock_guard<std::mutex> lk(g_prof_mu);
                g_loop_host[0] += host_enq_s; g_loop_host[1] += host_wait_s; g_loop_host[2] += wall; g_loop_host[3] += (double)host_batches * rpb;
            }
            if (sw.dbg_host)
                fprintf(stderr, "[sfx] host enqueue: %ld batches of rounds, %.1f us of host time per round, %.1f %% of the loop's %.1f ms wall time\n",
                        host_batches, 1e6 * host_enq_s / std::max(1L, host_batches * rpb), 100.0 * host_enq_s / std::max(wall, 1e-9), 1e3 * wall);
            if (sw.dbg_nact) {
                fprintf(stderr, "[sfx] rounds by active columns (<=32, <=64, ..., <=256, more), cumulative:");
                for (int i = 0; i < 9; ++i) fprintf(stderr, " %ld", nact_hist[i]);
                fprintf(stderr, "\n");
            }
        }
        SFX_CHECK(hipGetLastError());
        std::vector<int> id(B);         // restore the identity mapping for stand-alone calls
        for (int i = 0; i < B; ++i) id[i] = i;
        SFX_CHECK(hipMemcpyAsync(D.slot, id.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
        SFX_CHECK(hipStreamSynchronize(s));
        D.nact = B;
        return 0;
    }
};
}  // namespace

// The loops that wait for every poll: the needed-rows fused path (persistent per-frame workgroups; the host only re-launches
// frames that need more ticks) and the stand-alone kernels of sfx_batch_step / sfx_prof_enable bit 1
static int run_synced(sfx_batch* b, int first_stage, int last_stage, int step_mode, bool fused, long max_ticks, bool& done, hipStream_t s) {
    BatchDev& D = b->D; const DevModel& M = b->m->M;
    const int B = D.cfg.B, chunk = 512, POLL = D.cfg.lbs_mode == 1 ? 8 : 32;
    std::vector<int> hs(B);
    int* hp = b->stage_host ? b->stage_host : hs.data();
    for (long tick = 0; !done && tick < max_ticks;) {
        if (fused) {
            ProfScope p("fit_rows", s);
            launch_fit_rows(M, D, b->vl_dev, b->sw_dev, first_stage, last_stage, chunk, s);
            tick += chunk;
        } else for (int q = 0; q < POLL; ++q, ++tick) {
            if (int rc = eval_closure(b, -2, 0, s)) return rc;
            ProfScope p("lbfgs", s);
            launch_lbfgs_tick(M, D, b->vl_dev, first_stage, last_stage, 0, step_mode, s);
        }
        SFX_CHECK(hipMemcpyAsync(hp, D.stage, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
        SFX_CHECK(hipStreamSynchronize(s));
        done = true;
        for (int i = 0; i < B; ++i) if (hp[i] <= last_stage) { done = false; break; }
    }
    SFX_CHECK(hipGetLastError());
    return 0;
}

// tick loop shared by sfx_batch_fit (whole run_fitting) and sfx_batch_step (one LBFGS.step): the init tick, then the loop of the
// batch's kind -- the polled dense loop for a fused dense fit, run_synced for everything else
static int run_ticks(sfx_batch* b, int first_stage, int last_stage, int init, int step_mode, hipStream_t s) {
    BatchDev& D = b->D;
    const bool dense = D.cfg.lbs_mode == 1;
    const bool fused = !step_mode && !g_unfused;
    D.act = nullptr; D.nrun = 0;          // (a previous fit that ended on an error may have left its running list attached)
    if (init == 1 && D.pen_flag) SFX_CHECK(hipMemsetAsync(D.pen_flag, 0, (size_t)D.cfg.B * sizeof(int), s));
    launch_lbfgs_tick(b->m->M, D, b->vl_dev, first_stage, last_stage, init, step_mode, s);
    // bound on the rounds of the polled loops: one resident batch needs at most stages x maxiters LBFGS.step calls of
    // <= ~160 evaluations each; a job of B frames through a pool of `slots` columns needs that once per wave of the queue
    long max_ticks = sfx_fit_tick_bound(D.cfg, first_stage, last_stage);
    if (dense && b->slots > 0 && b->slots < D.cfg.B) max_ticks *= (D.cfg.B + b->slots - 1) / b->slots;
    bool done = false;
    const int rc = fused && dense ? DenseLoop{b, s, first_stage, last_stage}.run(max_ticks, done)
                                  : run_synced(b, first_stage, last_stage, step_mode, fused, max_ticks, done, s);
    if (rc) return rc;
    if (!done) { sfx_set_error("fit did not finish within %ld ticks", max_ticks); return -4; }
    return 0;
}

extern "C" int sfx_batch_fit(sfx_batch* b, int32_t first_stage, int32_t last_stage, void* stream) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_batch_fit")) return -1;
    if (first_stage < -1 || last_stage >= b->D.cfg.n_stages || last_stage < first_stage) {
        sfx_set_error("bad stage range [%d,%d]", first_stage, last_stage); return -1;
    }
    return run_ticks(b, first_stage, last_stage, 1, 0, (hipStream_t)stream);
}

extern "C" int sfx_batch_step(sfx_batch* b, int32_t stage, int32_t resume, float* loss_out, void* stream) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_batch_step")) return -1;
    if (stage < -1 || stage >= b->D.cfg.n_stages) { sfx_set_error("stage %d out of range", stage); return -1; }
    int rc = run_ticks(b, stage, stage, resume ? 2 : 1, 1, (hipStream_t)stream);
    if (rc) return rc;
    if (loss_out) {
        const int B = b->D.cfg.B;
        std::vector<float> l((size_t)B * (1 + SFX_MAX_STAGES));
        SFX_CHECK(hipMemcpy(l.data(), b->D.stage_loss, l.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < B; ++i) loss_out[i] = l[(size_t)i * (1 + SFX_MAX_STAGES) + stage + 1];
    }
    return 0;
}

// body_pose_prior = MaxMixturePrior (prior.py:100-231) for use_vposer=False fits without a regression
// prior (fitting.py:399-401).  means [M][D], precisions [M][D][D], nll_weights [M] (as the module's buffers)
extern "C" int sfx_batch_set_gmm_form(sfx_batch* b, int32_t M, int32_t Dm, const float* means, const float* precisions,
                                      const float* nll_weights, const float* comp_const);
extern "C" int sfx_batch_set_gmm(sfx_batch* b, int32_t M, int32_t Dm, const float* means, const float* precisions,
                                 const float* nll_weights) {
    return sfx_batch_set_gmm_form(b, M, Dm, means, precisions, nll_weights, nullptr);
}
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

extern "C" int sfx_batch_pen_stats(sfx_batch* b, int32_t* stats_host /* [B][4] */, int32_t* ext_n_host /* [B] or NULL */) {
    if (!b || !stats_host) { sfx_set_error("null argument"); return -1; }
    if (!b->pen) { sfx_set_error("batch was created without interpenetration"); return -1; }
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
    if (!b->pen) { sfx_set_error("batch was created without interpenetration"); return -1; }
    if (b->pen_chunked) { sfx_set_error("the pair lists of a pooled batch's stand-alone evaluation are overwritten chunk by chunk"); return -1; }
    return sfx_pen_pairs(b->pen, column, cap, pairs_host, n_out);
}

extern "C" int sfx_batch_pen_launches(sfx_batch* b) {
    if (!b) { sfx_set_error("null argument"); return -1; }
    return b->pen_graph_nodes;
}

extern "C" int sfx_batch_pen_flags(sfx_batch* b, int32_t* flags_host /* [B] */) {
    if (!b || !flags_host) { sfx_set_error("null argument"); return -1; }
    if (!b->pen) { sfx_set_error("batch was created without interpenetration"); return -1; }
    SFX_CHECK(hipDeviceSynchronize());
    SFX_CHECK(hipMemcpy(flags_host, b->D.pen_flag, (size_t)b->D.cfg.B * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sfx_batch_get_grad(sfx_batch* b, int32_t stage, float* grad_out) {
    if (!b || !grad_out) { sfx_set_error("null argument"); return -1; }
    if (refuse_f64(b, "sfx_batch_get_grad")) return -1;
    if (stage < -1 || stage >= b->D.cfg.n_stages) { sfx_set_error("stage %d out of range", stage); return -1; }
    const int B = b->D.cfg.B, n = b->vl_host[stage < 0 ? 0 : 1].n;
    std::vector<float> g((size_t)B * SFX_NVAR_MAX);
    SFX_CHECK(hipMemcpy(g.data(), b->D.g, g.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < B; ++i) memcpy(grad_out + (size_t)i * n, g.data() + (size_t)i * SFX_NVAR_MAX, (size_t)n * 4);
    return 0;
}

extern "C" int sfx_batch_get_grad_f64(sfx_batch* b, int32_t stage, double* grad_out) {
    if (need_f64(b, "sfx_batch_get_grad_f64")) return -1;
    if (!grad_out) { sfx_set_error("null argument"); return -1; }
    if (stage < -1 || stage >= b->D.cfg.n_stages) { sfx_set_error("stage %d out of range", stage); return -1; }
    const int B = b->D.cfg.B, n = b->vl_host[stage < 0 ? 0 : 1].n;
    std::vector<double> g((size_t)B * SFX_NVAR_MAX);
    SFX_CHECK(hipMemcpy(g.data(), b->D.g64, g.size() * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < B; ++i) memcpy(grad_out + (size_t)i * n, g.data() + (size_t)i * SFX_NVAR_MAX, (size_t)n * 8);
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

extern "C" int sfx_batch_forward(sfx_batch* b, float* verts_dev, float* joints_dev, void* stream) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (refuse_f64(b, "sfx_batch_forward")) return -1;
    hipStream_t s = (hipStream_t)stream;
    const DevModel& M = b->m->M; const BatchDev& D = b->D;
    if (D.cfg.lbs_mode == 0 && !verts_dev) {       // needed-rows batch, joints only: the forward the rows closure runs
        ClosureArgs a{}; a.stage_override = 0; a.forward_only = 1; a.from_X = 1;
        launch_closure(M, D, b->vl_dev, b->sw_dev, a, s);
        if (joints_dev) SFX_CHECK(hipMemcpyAsync(joints_dev, D.joints, (size_t)D.cfg.B * M.K * 3 * 4, hipMemcpyDeviceToDevice, s));
        SFX_CHECK(hipStreamSynchronize(s));
        SFX_CHECK(hipGetLastError());
        return 0;
    }
    ClosureArgs e{}; e.stage_override = 0; e.export_dense = 1; e.forward_only = 2; e.from_X = 1;
    launch_closure(M, D, b->vl_dev, b->sw_dev, e, s);
    { ProfScope p("lbs_dense", s, D.nact); launch_lbs_dense(M, D, s); }
    ClosureArgs a{}; a.stage_override = 0; a.forward_only = 1; a.from_X = 1; a.use_dense_verts = 1;
    launch_closure(M, D, b->vl_dev, b->sw_dev, a, s);
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
        ClosureArgs e{}; e.stage_override = 0; e.export_dense = 1; e.forward_only = 2; e.from_X = 1;
        launch_closure(M, D, b->vl_dev, b->sw_dev, e, s);
        { ProfScope p("lbs_dense", s, D.nact); launch_lbs_dense(M, D, s); }      // (writes v_posed of every vertex as well: D.vposed)
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
