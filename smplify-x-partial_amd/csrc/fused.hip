// fused.hip -- the fitting loop with as few launches as the data dependencies allow.
//
//  k_fit_rows   (needed-rows LBS): ONE workgroup per frame runs that frame's whole schedule
//               -- closure (256 threads) -> optimiser tick (wavefront 0) -> closure -> ... --
//               without returning to the host: no launch latency, no lock-step between frames;
//               workgroups of finished frames retire and queued frames take their CU.
//  k_tick_dense (dense LBS): between two launches of the batched MFMA GEMM (lbs_dense.hip) one
//               launch does [loss + adjoint of evaluation i] -> [optimiser tick] -> [pose
//               assembly / kinematic chain of evaluation i+1 and its export to the GEMM operands].
//  k_tick_dense_multi (dense LBS, body-only, few frames): up to SFX_TICK_ROUNDS such rounds in one launch -- the tick needs
//               nothing of the GEMM there (self-served blend offsets), so a workgroup walks its frame's rounds over a ring of
//               operand sets and the GEMMs follow behind the launch.
#include "closure_body.h"
#include "lbfgs_body.h"

#ifndef SFX_SETS_SMALL8
#define SFX_SETS_SMALL8 3      // register sets of the two-loop recursion in the body-only tick kernels with a workgroup per CU
#endif
#ifndef SFX_TICK_OCC
#define SFX_TICK_OCC 2
#endif

template <class LDS>
__global__ __launch_bounds__(LDS::kThreads, LDS::kBlocksPerCU)
void k_fit_rows(DevModel M, BatchDev D, const VarList* __restrict__ vls, const StageW* __restrict__ sws,
                int first_stage, int last_stage, int max_ticks) {
    __shared__ LDS S;
    __shared__ float gflat[SFX_NVAR_MAX];
    __shared__ float fval;
    __shared__ float s_al[SFX_HIST_MAX + 2 * LB_BS];
    __shared__ OptScal st;
    const int b = blockIdx.x;
    ClosureArgs a{};
    a.stage_override = -2;
    for (int it = 0; it < max_ticks; ++it) {
        if (D.stage[b] > last_stage) break;
        closure_body(S, M, D, vls, sws, a, b, gflat, &fval);
        a.keep_tables = 1;
        __syncthreads();
        // (one wavefront: sharing the dot products of the two-loop recursion between four was measured slower --
        //  a workgroup barrier per block of 8 history pairs costs more than the reductions it removes)
        if (threadIdx.x < 64)
            lbfgs_tick_body<2>(M, D, vls, first_stage, last_stage, 0, 0, b, threadIdx.x, s_al, st, S.T, &fval, gflat);      // (S.T: >= 2048 floats of closure scratch, dead between evaluations)
        __syncthreads();
    }
}

// (small variant, OCC = 2: two workgroups per CU -- batches of more than 256 frames then run two latency-bound frames per
//  CU; OCC = 1 is the same code with the whole register file, launched when every frame has a CU of its own: no spills,
//  73.8 instead of 76.2 us per launch)
// The overlapped loop (host/fit_loop.hip DenseLoop) rotates three sets of GEMM operand buffers: the export pass writes featR_w / AT_w while
// GEMMs in flight read featR / AT (the operands of the latest evaluation) and the third set.  A frame that has finished exports
// no more, so its column would go on cycling through the operands of its last three evaluations and D.verts would end on any
// of their meshes.  Its workgroup therefore copies the column from the set of the latest evaluation into the one that is
// written now -- in the launch it finishes in and in every later one that still lists it (the host retires a frame at least
// one polled batch of rounds after it finished): after two launches all three sets hold the operands of its last evaluation.
// Only the set nobody reads is written: the loop has waited for the GEMM that read it.  Elsewhere featR_w == featR: nothing to do.
__device__ __forceinline__ void copy_operand_column(const BatchDev& D, int slot, int nthreads) {
    if (D.featR_w == D.featR) return;
    const int t = threadIdx.x;
    if (t < SFX_KD_PAD / 4)
        reinterpret_cast<float4*>(D.featR_w + (size_t)slot * SFX_KD_PAD)[t] = reinterpret_cast<const float4*>(D.featR + (size_t)slot * SFX_KD_PAD)[t];
    for (int i = t; i < 12 * SFX_JPAD; i += nthreads) D.AT_w[(size_t)i * D.Bpad + slot] = D.AT[(size_t)i * D.Bpad + slot];
}

template <class LDS, int OCC>
__global__ __launch_bounds__(LDS::kThreads, OCC)
void k_tick_dense(DevModel M, BatchDev D, const VarList* __restrict__ vls, const StageW* __restrict__ sws,
                  int first_stage, int last_stage, int has_eval) {
    __shared__ LDS S;
    __shared__ float gflat[SFX_NVAR_MAX];
    __shared__ float fval;
    __shared__ float s_al[SFX_HIST_MAX + 2 * LB_BS];
    __shared__ OptScal st;
    // PF (a workgroup per CU: LDS to spare): the optimiser tick's working set -- its 8 vectors, X, Xt, the scalar state, both
    // variable lists -- is requested with the loss / adjoint pass's entry batch (LDS-DMA into memory of its own, waited for
    // by that entry's barrier) instead of at the tick's start, where it was a memory round trip of the frame's serial chain;
    // the pass that follows the tick takes the trial point and the stage from LDS instead of reading back what the tick
    // has just stored (two more round trips).  Same values either way.
    constexpr bool PF = (OCC == 1);
    constexpr int CTK = LDS::kThreads;
    __shared__ __align__(16) float s_pf[PF ? 2048 : 4];
    __shared__ __align__(16) VarList s_vl[PF ? 2 : 1];
    __shared__ int s_stage;
    static_assert(sizeof(VarList) % 4 == 0 && sizeof(OptScal) % 4 == 0 && (NVEC * SFX_NVAR_MAX) % 4 == 0, "dword / 16-byte LDS-DMA");
    const int b = D.act ? D.act[blockIdx.x] : blockIdx.x;      // (frames that finished or still wait in the queue are not launched)
    // self-served blend offsets (has_eval = 2): the frame's column addresses the A operand of closure_body's self_blend_offsets --
    // requested here, with the stage
    const int self_col = (has_eval == 2 && M.n_uniq > 0) ? D.slot[b] : 0;
    if (D.stage[b] > last_stage) {      // finished, and the host has not retired it yet: see copy_operand_column
        if (has_eval) copy_operand_column(D, D.slot[b], CTK);
        return;
    }
    const long long wc0 = D.dbg ? wall_clock64() : 0;      // debug: per-workgroup duration statistics (100 MHz clock)
    // debug clocks: stamps freeze after launch number dbg[61] of this kernel, so a mid-fit launch is what is read back
    if (D.dbg && blockIdx.x == 0 && threadIdx.x == 0) { D.dbg[62] += 1; if (D.dbg[62] <= D.dbg[61]) D.dbg[24] = clock64(); }
    if (has_eval) {
        ClosureArgs a{};
        a.stage_override = -2; a.use_dense_verts = has_eval == 2 ? 2 : 1; a.reuse_fwd = 1;      // (2: self-served blend offsets, sfx_internal.h)
        a.self_col = __builtin_amdgcn_readfirstlane(self_col);
        if constexpr (PF) {
            lds_fill_async16<CTK>(s_pf, D.vec + (size_t)b * NVEC * SFX_NVAR_MAX, NVEC * SFX_NVAR_MAX / 4);
            lds_fill_async16<CTK>(s_pf + NVEC * SFX_NVAR_MAX, D.X + (size_t)b * SFX_NPAR_MAX, SFX_NPAR_MAX / 4);
            lds_fill_async16<CTK>(s_pf + NVEC * SFX_NVAR_MAX + SFX_NPAR_MAX, D.Xt + (size_t)b * SFX_NPAR_MAX, SFX_NPAR_MAX / 4);
            lds_fill_async<CTK>(&st, &(reinterpret_cast<const OptState*>(D.opt) + b)->s, (int)(sizeof(OptScal) / 4));
            lds_fill_async<CTK>(s_vl, vls, (int)(2 * sizeof(VarList) / 4));
        }
        closure_body(S, M, D, vls, sws, a, b, gflat, &fval);
        __syncthreads();
        const long long wc1 = D.dbg ? wall_clock64() : 0;
        // (one wavefront: sharing the dot products of the two-loop recursion between four was measured slower --
        //  a workgroup barrier per block of 8 history pairs costs more than the reductions it removes)
        if (threadIdx.x < 64) {
            if constexpr (PF)
                lbfgs_tick_body<((LDS::kMaxItems <= SFX_SMALL_ITEMS) ? SFX_SETS_SMALL8 : 2), true>(M, D, s_vl, first_stage, last_stage, 0, 0, b, threadIdx.x, s_al, st, s_pf, &fval, gflat, &s_stage);
            else
                lbfgs_tick_body<2>(M, D, vls, first_stage, last_stage, 0, 0, b, threadIdx.x, s_al, st, S.T, &fval, gflat);      // (S.T: >= 2048 floats of closure scratch, dead between evaluations)
        }
        __syncthreads();
        if (D.dbg && threadIdx.x == 0) {       // debug: mean duration of the two segments over all workgroups (100 MHz ticks)
            const long long wc2 = wall_clock64();
            atomicAdd((unsigned long long*)&D.dbg[29], (unsigned long long)(wc1 - wc0));
            atomicAdd((unsigned long long*)&D.dbg[30], (unsigned long long)(wc2 - wc1));
        }
        if (D.dbg && b == 0 && threadIdx.x == 0 && D.dbg[62] <= D.dbg[61]) { D.dbg[25] = clock64(); for (int i = 0; i < 17; ++i) D.dbg[40 + i] = D.dbg[i]; }
        if ((PF ? s_stage : D.stage[b]) > last_stage) {          // finished in this launch: its column carries no collision weight any more
            if (D.pen_want && threadIdx.x == 0) D.pen_want[D.slot[b]] = 0;
            copy_operand_column(D, D.slot[b], CTK);
            return;
        }
    }
    const int stage_now = (PF && has_eval) ? s_stage : D.stage[b];
    // interpenetration: does the evaluation exported below carry a collision weight (fitting.py:437)?  Kept here, per column, by
    // the workgroup that knows the frame's stage (a memset and a launch of their own per round until round 4)
    if (D.pen_want && threadIdx.x == 0) {
        const int st_ = stage_now;
        D.pen_want[D.slot[b]] = (st_ >= 0 && st_ < D.cfg.n_stages) ? (sws[st_].coll > 0.f ? 1 : 0) : 0;
    }
    ClosureArgs e{};
    e.stage_override = -2; e.export_dense = 1; e.forward_only = 2; e.keep_tables = has_eval;
    if (PF && has_eval) { e.stage_override = stage_now; e.x_lds = s_pf + NVEC * SFX_NVAR_MAX + SFX_NPAR_MAX; }
    closure_body(S, M, D, vls, sws, e, b, nullptr, nullptr);
    if (D.dbg && b == 0 && threadIdx.x == 0 && D.dbg[62] <= D.dbg[61]) D.dbg[26] = clock64();
    if (D.dbg && threadIdx.x == 0) {
        const long long dt = wall_clock64() - wc0;
        atomicMax((unsigned long long*)&D.dbg[58], (unsigned long long)dt);
        atomicAdd((unsigned long long*)&D.dbg[59], (unsigned long long)dt);
        atomicAdd((unsigned long long*)&D.dbg[60], 1ull);
    }
}

// k_tick_dense_multi: up to SFX_TICK_ROUNDS rounds of the self-served form (has_eval = 2) of k_tick_dense<FrameLDSSmall8, 1> in ONE
// launch.  T(i+1) of a frame reads only what T(i) of the same workgroup wrote -- optimiser state, trial point, forward-state
// blob, its column of the operands -- so the workgroup loops over its frame's rounds and keeps its CU between them: no kernel
// boundary, no cold entry (the tables stay in LDS: keep_tables from the second round on) and no waiting for the slowest frame
// of every round.  Round r reads operand set r (blend offsets, column copy) and exports to set r + 1; the host launches the
// GEMMs of sets 1 .. R behind the launch, on the CUs the ticks do not hold (host/fit_loop.hip DenseLoop::launch_multi).  Between
// rounds: one workgroup barrier; the frame's state stays in LDS (forward state in S, the tick's working set in s_pf / st) and is
// written to global memory as between two launches, for the host and for whoever runs the frame's next round, but not read
// back.  No flags, no polling, nothing between workgroups.
// A frame that finishes in round r (or is found finished at entry: r = 0) copies its column of set r into EVERY later set of the
// launch and leaves the loop, so each GEMM behind this launch skins its last evaluation (copy_operand_column, generalised).
// The debug clocks stamp round 0.
__global__ __launch_bounds__(FrameLDSSmall8::kThreads, 1)
void k_tick_dense_multi(DevModel M, BatchDev D, const VarList* __restrict__ vls, const StageW* __restrict__ sws,
                        int first_stage, int last_stage, TickSets sets, int R) {
    using LDS = FrameLDSSmall8;
    constexpr int CTK = LDS::kThreads;
    __shared__ LDS S;
    __shared__ float gflat[SFX_NVAR_MAX];
    __shared__ float fval;
    __shared__ float s_al[SFX_HIST_MAX + 2 * LB_BS];
    __shared__ OptScal st;
    __shared__ __align__(16) float s_pf[2048];          // the optimiser tick's working set, prefetched (k_tick_dense: PF)
    __shared__ __align__(16) VarList s_vl[2];
    __shared__ int s_stage;
    __shared__ float* s_featR[SFX_TICK_ROUNDS + 1];       // the operand sets, indexed by round (a kernel argument indexed at run time would live in scratch)
    __shared__ float* s_AT[SFX_TICK_ROUNDS + 1];
    const int b = D.act ? D.act[blockIdx.x] : blockIdx.x;
    const int slot = D.slot[b];
    const int self_col = __builtin_amdgcn_readfirstlane(M.n_uniq > 0 ? slot : 0);
    const bool stamp = D.dbg && blockIdx.x == 0 && threadIdx.x == 0;
    if (stamp) { D.dbg[62] += 1; if (D.dbg[62] <= D.dbg[61]) D.dbg[24] = clock64(); }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q <= SFX_TICK_ROUNDS; ++q) { s_featR[q] = sets.featR[q]; s_AT[q] = sets.AT[q]; }
    }
    __syncthreads();
    // The optimiser tick's working set (k_tick_dense: PF) and the forward state of the pending evaluation come from global memory
    // in round 0 alone: requested here, waited for by the entry barrier of round 0's loss / adjoint pass.  In every later round
    // they are what the tick and the export pass of the round before left in s_pf / st and in S -- the tick writes back all it
    // changes there, the export pass saves what it leaves, so the bytes are those a reload would bring -- and the frame's stage
    // is the one that tick handed over in s_stage.
    int stage_now = D.stage[b];
    if (stage_now <= last_stage) {
        lds_fill_async16<CTK>(s_pf, D.vec + (size_t)b * NVEC * SFX_NVAR_MAX, NVEC * SFX_NVAR_MAX / 4);
        lds_fill_async16<CTK>(s_pf + NVEC * SFX_NVAR_MAX, D.X + (size_t)b * SFX_NPAR_MAX, SFX_NPAR_MAX / 4);
        lds_fill_async16<CTK>(s_pf + NVEC * SFX_NVAR_MAX + SFX_NPAR_MAX, D.Xt + (size_t)b * SFX_NPAR_MAX, SFX_NPAR_MAX / 4);
        lds_fill_async<CTK>(&st, &(reinterpret_cast<const OptState*>(D.opt) + b)->s, (int)(sizeof(OptScal) / 4));
        lds_fill_async<CTK>(s_vl, vls, (int)(2 * sizeof(VarList) / 4));
    }
    int r = 0;
    const bool live_at_entry = stage_now <= last_stage;
#pragma clang loop unroll(disable)
    for (bool live = live_at_entry; live && r < R; ++r) {
        if (r) __syncthreads();
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));                   // opaque per round: address arithmetic on it stays inside the round instead of being hoisted and spilled
        // forward state: in S from round 1 on; saved to D.fwd by the last export of the launch alone (the next launch, a
        // single-round tick after a form change, or a compaction's export may be the reader -- never one before that)
        const OperandSets ops{s_featR[r], s_featR[r + 1], s_AT[r + 1], t, r > 0, r + 1 == R};
        ClosureArgs a{};
        a.stage_override = stage_now; a.use_dense_verts = 2; a.reuse_fwd = 1; a.keep_tables = r > 0; a.self_col = self_col;
        closure_body(S, M, D, vls, sws, a, b, gflat, &fval, NoUpstream{}, ops);
        __syncthreads();
        if (t < 64)
            lbfgs_tick_body<SFX_SETS_SMALL8, true, false>(M, D, s_vl, first_stage, last_stage, 0, 0, b, t, s_al, st, s_pf, &fval, gflat, &s_stage, stage_now);
        __syncthreads();
        if (stamp && r == 0 && D.dbg[62] <= D.dbg[61]) { D.dbg[25] = clock64(); for (int i = 0; i < 17; ++i) D.dbg[40 + i] = D.dbg[i]; }
        stage_now = __builtin_amdgcn_readfirstlane(s_stage);
        if (stage_now > last_stage) { live = false; break; }      // finished in this round: set r holds its last evaluation
        ClosureArgs e{};
        e.stage_override = stage_now; e.export_dense = 1; e.forward_only = 2; e.keep_tables = 1;
        e.x_lds = s_pf + NVEC * SFX_NVAR_MAX + SFX_NPAR_MAX;
        closure_body(S, M, D, vls, sws, e, b, nullptr, nullptr, NoUpstream{}, ops);
        // the tick's working set to memory, every round (the host reads it after the fit, the next launch at its entry): here, by all
        // wavefronts next to the export's stores, whose acknowledgement the barrier at the loop's top waits for anyway -- at the
        // tick's end the tick wavefront waited for these stores alone, on the frame's chain
        tick_write_back<CTK>(D, b, s_pf, st, t);
        if (stamp && r == 0 && D.dbg[62] <= D.dbg[61]) D.dbg[26] = clock64();
    }
    if (r == R) return;                                  // every round exported
    if (live_at_entry) tick_write_back<CTK>(D, b, s_pf, st, (int)threadIdx.x);      // finished in round r: its last tick's working set
    // finished in round r > 0: the export of round r - 1 did not save its forward state (its reader was this workgroup); D.fwd is
    // to hold the state of the frame's last exported evaluation, and S still does -- nothing after an export pass writes there
    if (r > 0 && D.fwd) save_forward_state(S, D.fwd + (size_t)b * SFX_FWD_N, (int)threadIdx.x, false);
    const float4* const f0 = reinterpret_cast<const float4*>(s_featR[r] + (size_t)slot * SFX_KD_PAD);
    const float* const a0 = s_AT[r];
    for (int q = r + 1; q <= R; ++q) {
        if (threadIdx.x < SFX_KD_PAD / 4) reinterpret_cast<float4*>(s_featR[q] + (size_t)slot * SFX_KD_PAD)[threadIdx.x] = f0[threadIdx.x];
        for (int i = threadIdx.x; i < 12 * SFX_JPAD; i += CTK) s_AT[q][(size_t)i * D.Bpad + slot] = a0[(size_t)i * D.Bpad + slot];
    }
}

// debug / tests (sfx_batch_debug_read "uvp_self"): self_blend_offsets for every column of the current D.featR, one workgroup of four
// wavefronts per column -- what a tick workgroup launched with has_eval = 2 would use in place of that column's row of D.uvp
__global__ __launch_bounds__(256)
void k_uvp_self(DevModel M, BatchDev D, float* __restrict__ out) {
    const int col = blockIdx.x;
    self_blend_offsets(M.uniq_dirs, M.n_uniq, D.featR + (size_t)col * SFX_KD_PAD, out + (size_t)col * M.n_uniq * 3,
                       threadIdx.x >> 6, 4, threadIdx.x & 63);
}
void launch_uvp_self(const DevModel& M, const BatchDev& D, float* out, hipStream_t s) {
    if (D.cfg.B <= 0 || M.n_uniq <= 0) return;
    hipLaunchKernelGGL(k_uvp_self, dim3(D.cfg.B), dim3(256), 0, s, M, D, out);
}

void launch_fit_rows(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW* sw_dev,
                     int first_stage, int last_stage, int max_ticks, hipStream_t s) {
    if (sfx_small_closure(M, D))
        hipLaunchKernelGGL(k_fit_rows<FrameLDSSmall>, dim3(D.cfg.B), dim3(FrameLDSSmall::kThreads), 0, s, M, D, vl_dev, sw_dev, first_stage, last_stage, max_ticks);
    else
        hipLaunchKernelGGL(k_fit_rows<FrameLDS>, dim3(D.cfg.B), dim3(FrameLDS::kThreads), 0, s, M, D, vl_dev, sw_dev, first_stage, last_stage, max_ticks);
}
// The launch shapes of the body-only dense tick: a workgroup per CU while the grid fits the chip -- eight wavefronts
// (FrameLDSSmall8: same bits as four, closure_body.h; lab build, SFX_TICK_THREADS=256: the four-wavefront kernel of round 3, a
// measurement switch) -- and two four-wavefront workgroups per CU beyond.  launch_tick_dense and tick_dense_multi_ok both ask here.
enum TickShape { TICK_SMALL8, TICK_SMALL_CU, TICK_SMALL_OCC };
static TickShape tick_small_shape(int grid) {
    static const int n_cu = [] { hipDeviceProp_t p; int dev = 0; (void)hipGetDevice(&dev); return hipGetDeviceProperties(&p, dev) == hipSuccess ? p.multiProcessorCount : 256; }();
#ifdef SFX_LAB
    static const bool t256 = [] { const char* e = getenv("SFX_TICK_THREADS"); return e && atoi(e) == 256; }();
#else
    constexpr bool t256 = false;
#endif
    return grid > n_cu ? TICK_SMALL_OCC : t256 ? TICK_SMALL_CU : TICK_SMALL8;
}
bool tick_dense_multi_ok(const DevModel& M, const BatchDev& D) {
    return M.n_uniq > 0 && M.n_uniq <= FrameLDSSmall8::kMaxItems && sfx_small_closure(M, D) && tick_small_shape(D.act ? D.nrun : D.cfg.B) == TICK_SMALL8;
}
void launch_tick_dense_multi(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW* sw_dev,
                             int first_stage, int last_stage, const TickSets& sets, int R, hipStream_t s) {
    const int grid = D.act ? D.nrun : D.cfg.B;
    if (grid <= 0 || R <= 0) return;
    hipLaunchKernelGGL(k_tick_dense_multi, dim3(grid), dim3(FrameLDSSmall8::kThreads), 0, s, M, D, vl_dev, sw_dev, first_stage, last_stage, sets, R);
}
void launch_tick_dense(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW* sw_dev,
                       int first_stage, int last_stage, int has_eval, hipStream_t s) {
    const int grid = D.act ? D.nrun : D.cfg.B;
    if (grid <= 0) return;
    if (sfx_small_closure(M, D)) {
        switch (tick_small_shape(grid)) {
        case TICK_SMALL8:
            hipLaunchKernelGGL((k_tick_dense<FrameLDSSmall8, 1>), dim3(grid), dim3(FrameLDSSmall8::kThreads), 0, s, M, D, vl_dev, sw_dev, first_stage, last_stage, has_eval); break;
        case TICK_SMALL_CU:
            hipLaunchKernelGGL((k_tick_dense<FrameLDSSmall, 1>), dim3(grid), dim3(FrameLDSSmall::kThreads), 0, s, M, D, vl_dev, sw_dev, first_stage, last_stage, has_eval); break;
        case TICK_SMALL_OCC:
            hipLaunchKernelGGL((k_tick_dense<FrameLDSSmall, SFX_TICK_OCC>), dim3(grid), dim3(FrameLDSSmall::kThreads), 0, s, M, D, vl_dev, sw_dev, first_stage, last_stage, has_eval); break;
        }
    } else
        hipLaunchKernelGGL((k_tick_dense<FrameLDS, 1>), dim3(grid), dim3(FrameLDS::kThreads), 0, s, M, D, vl_dev, sw_dev, first_stage, last_stage, has_eval);
}
