// host.h -- what the units of the host layer (csrc/host/) share: the two handles of include/sfx.h with their ownership rules, the
// float64 mode's guards, the polled loop's constants, the profiler's scope and the few functions that cross units.
//   runtime.hip   error string, version, HIP-event profiler, host statistics of the polled loops, the float64 guards
//   model.hip     sfx_model_*: constants upload, part table, VPoser weights
//   batch.hip     sfx_batch_create / destroy, frame and parameter I/O with the _f64 forms, stage weights, GMM prior
//   eval.hip      one evaluation: the interpenetration step, closure and gradient readers, guess_init, forward, sfx_lbs_*
//   fit_loop.hip  DenseLoop, run_synced, run_ticks; sfx_batch_fit / step
//   inspect.hip   debug readers, the lab build's clocks, interpenetration diagnostics, trace, stats
//   render.hip    sfx_render_meshes: the stateless entry of the mesh rasteriser (csrc/raster.hip)
#pragma once
#include "../../../include/sfx.h"
#include "../sfx_internal.h"
#include "../collide_host.h"
#include "../operand_ring.h"
#include "idle_slot.h"

#include <map>
#include <vector>

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
    IdleSlot<sfx_pen, sfx_pen_destroy> pen_idle;      // taken by sfx_batch_create, given back by ~sfx_batch (idle_slot.h)
    int parts_gen = 0;            // bumped by sfx_model_set_parts: handles made for another part table are not reused
    ~sfx_model() { sfx_batch_destroy(fwd); pen_idle.drop(); }
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
// the multi-round form (DenseLoop::launch_multi: up to SFX_OV_MULTI_R self-served rounds per tick launch, their GEMMs beside the next
// launch) at 1 .. SFX_OV_MULTI_MAX active columns: in place of the serial rounds below the self-served band and of that band's
// lowest slice.  Swept in LAB_NOTES 4.14 (frames/s with the form up to n columns: 0: 636.5, 16: 647.6, 32: 657.2, 64: 673.5,
// 96: 677.2, 128: 677.6; at 128 columns with 2 / 4 / 8 rounds per launch: 624.4 / 659.5 / 677.6)
#ifndef SFX_OV_MULTI_MAX
#define SFX_OV_MULTI_MAX 96
#endif
#ifndef SFX_OV_MULTI_R
#define SFX_OV_MULTI_R SFX_TICK_ROUNDS
#endif
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
    // the overlapped dense loop (DenseLoop): the sets of GEMM operand buffers (owned by mem; set 0 is what D.featR / D.AT were
    // created as, and D.featR / D.AT name set ring.cur, the one of the most recent evaluation), the bookkeeping that hands them
    // out (operand_ring.h; it outlives a fit, like the buffers), the stream of the GEMMs beside the ticks and the two rings of
    // events that order them against the tick kernels; stream and events are made by the first fit that overlaps.
    // n_sets: 1 (no overlap: interpenetration, needed-rows), 3 (the single overlapped rounds) or OperandRing::kMaxSets (models the
    // multi-round form serves: body-only; 2 x SFX_TICK_ROUNDS + 1) -- (SFX_KD_PAD + 12 SFX_JPAD) x Bpad floats each, 1.2 MB at 256 frames
    float *op_f[OperandRing::kMaxSets] = {}, *op_a[OperandRing::kMaxSets] = {};
    int n_sets = 1;
    OperandRing ring;
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
    ~sfx_batch();                 // batch.hip
};

// The float64 mode's guards (runtime.hip).  Float inputs to a float64 batch are widened; float OUTPUTS are refused, so that no
// result is silently rounded, and so is everything the mode does not have (the device optimiser, the dense path, the GMM prior).
int refuse_f64(const sfx_batch* b, const char* fn);
int need_f64(const sfx_batch* b, const char* fn);
// values the float64 mode keeps in fp32 tables (keypoints, weights, masks, camera rotation, regression pose): exact or refused
bool fp32_exact(const double* v, size_t n);

// profiling: HIP-event timing of named kernels on the launch stream (runtime.hip).  With profiling off a scope is a load and a branch.
extern int g_prof;
extern int g_unfused;         // debug: run the fitting loop with the stand-alone kernels (sfx_prof_enable bit 1)
struct ProfScope {
    const char* name; hipStream_t s; hipEvent_t e0 = nullptr, e1 = nullptr;
    ProfScope(const char* n, hipStream_t st, double units = 0) : name(n), s(st) { if (g_prof) begin(units); }
    ~ProfScope() { if (e0) end(); }
    void begin(double units); void end();       // runtime.hip
};
// one polled dense loop's host side, added to what sfx_loop_host_stats reports: seconds enqueueing, waiting, wall; rounds
void loop_host_add(double enq_s, double wait_s, double wall_s, double rounds);

void pack_fd(sfx_batch* b, hipStream_t s);                                                        // batch.hip
void forward_at_X(sfx_batch* b, int stage, int use_dense_verts, hipStream_t s);                   // eval.hip
int eval_penetration(sfx_batch* b, int stage_override, hipStream_t s, bool want_ready = false);   // eval.hip
int eval_closure(sfx_batch* b, int stage_override, int from_X, hipStream_t s);                    // eval.hip
