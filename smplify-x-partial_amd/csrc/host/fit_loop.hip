// fit_loop.hip -- the hot loop of libsfx.so: sfx_batch_fit / sfx_batch_step are a stream of kernel launches with no host
// arithmetic and one small device->host poll every POLL ticks.  DenseLoop is the polled loop of a fused dense fit (four round
// forms over the column pool of column_pool.h and the operand sets of operand_ring.h), run_synced the loop of everything else,
// run_ticks chooses between them.
#include "host.h"
#include "../column_pool.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// Upper bound on the rounds a fit can take (a guard against a loop that never ends, not a budget): an LBFGS.step costs at most
// max_eval evaluations in its iterations plus one line search that may run over -- the bracket phase up to 25 evaluations, the zoom
// phase up to LBFGS(max_iter) (lbfgs_ls.py:108) -- plus the entry evaluation; a side view is fitted from two orientations
// (fit_single_frame.py:527-551), accounted for as a factor of its own (the old bound let the `* 2` do both).
static long sfx_fit_tick_bound(const BatchCfgDev& c, int first_stage, int last_stage) {
    const long per_step = (long)c.max_eval + std::max(25, (int)c.lbfgs_max_iter) + 1;
    return (long)(last_stage - first_stage + 1) * c.maxiters * std::max(80L, per_step + 7) * 2 /* orientations */ * 2 /* slack */ + 64;
}

// Measurement switches of the lab build (include/sfx_lab.h), read once by the first dense fit: diagnostics to stderr, polling
// cadence, the form of a dense round.  The product build has the defaults as constants.
struct DenseSwitches {
    bool dbg_nact = false, dbg_host = false;
    int rpb = 0, ahead = 0;                                                 // 0: the loop's own 8 rounds per batch, 3 / 1 batches ahead
    bool ov_on = true, self_on = true, self_in_serial = false;
    int ov_serial = SFX_OV_SERIAL, self_serial = SFX_OV_SELF_SERIAL, self_max = SFX_OV_SELF_MAX;
    int multi_max = SFX_OV_MULTI_MAX, multi_R = SFX_OV_MULTI_R;           // the multi-round form: up to this many columns, rounds per launch
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
        // the multi-round form stands where the serial rounds below the self-served band stood, so a given SFX_OVERLAP_SERIAL moves
        // it too (= 0: every round a self-served single launch, down to one column)
        v.multi_max = num("SFX_DENSE_MULTI", 1) != 0 ? num("SFX_DENSE_MULTI_MAX", getenv("SFX_OVERLAP_SERIAL") ? v.self_serial : SFX_OV_MULTI_MAX) : 0;
        v.multi_R = num("SFX_DENSE_MULTI_R", SFX_OV_MULTI_R);
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
// A round is one GEMM and one tick of every running frame, in one of four forms.  Three launch the tick of one round at a time
// (round_serial, round_key_rest, round_self); the fourth (launch_multi) launches the ticks of up to eight rounds as ONE kernel
// whose workgroups keep their CUs between rounds, and the GEMMs of those rounds behind it.  The form is chosen per polled batch.
// The overlapped forms run over SETS of operand buffers (b->op_f / op_a); b->ring (operand_ring.h) decides which set an export
// writes and which GEMM event s must have waited for first, and D.featR / D.AT always name its `cur`, the set of the latest
// export (the kernels take BatchDev by value and know no parity).
// Single overlapped rounds rotate THREE sets: T(i) overwrites what the GEMM of round i-2 read, hence its wait, which never blocks in
// practice: with two sets T(i) had to wait for Gr(i-1) and then raced Gr(i) for the CUs -- a tick workgroup needs 300 to 512
// registers per SIMD free and starves behind the GEMM's small workgroups (measured: 99 instead of 46 us per tick launch at 256
// frames, no gain).  With three, T(i) is queued while Gr(i-1) drains and takes the CUs as they empty; Gr(i) fills what is left.
// A finished frame's workgroup copies its column of cur to the set written for as long as it is listed (fused.hip).  Admission
// and compaction exports write cur IN PLACE once s has waited for the latest GEMM -- the columns of the frames that keep running
// hold their pending evaluation in cur only.  Two records and two waits per round or multi-round launch; no other cross-stream traffic.
struct DenseLoop {
    sfx_batch* const b; const hipStream_t s; const int first_stage, last_stage;
    BatchDev& D = b->D; const DevModel& M = b->m->M; const int B = D.cfg.B;
    bool overlap = false, self_form = false;            // a second stream and operand sets to overlap on; the model may serve itself
    OperandRing& ring = b->ring;
    long g_tok = OperandRing::kFree;                   // token of the newest GEMM event (its round's ov_i) s has not waited for
    hipEvent_t last_T = nullptr;                       // E_T of the latest self-served round (NULL: the latest round was of another form)
    long ov_i = 0, tick = 0;                           // overlapped rounds and multi-round launches (their slot in the event rings), rounds
    ColumnPool pool;
    int upl = 0, rpb = 8;                              // next upload buffer, rounds per polled batch
    int rot = 0;                                       // operand sets in the rotation of the latest batch's form (0: exports in place)
    int multi_R = 1;                                   // rounds per multi-round launch; the form rotates 2 multi_R + 1 operand sets
    // how much of the loop's wall time the HOST spends enqueueing (its headroom against a busy box) and waiting for stage flags
    double host_enq_s = 0.0, host_wait_s = 0.0; long host_batches = 0;
    static inline long nact_hist[9] = {};              // rounds by active GEMM columns: <=32, <=64, ..., <=256, more (cumulative)
    void tick_kernel(const char* name, const BatchDev& Dx, int has_eval) {
        ProfScope p(name, s, Dx.nrun);
        launch_tick_dense(M, Dx, b->vl_dev, b->sw_dev, first_stage, last_stage, has_eval, s);
    }
    hipEvent_t ev_G(long tok) const { return b->ov_ev[1][tok % SFX_OV_EVENTS]; }
    int wait_G(long tok) { if (tok != OperandRing::kFree) SFX_CHECK(hipStreamWaitEvent(s, ev_G(tok), 0)); return 0; }
    void point_at_cur() { D.featR = D.featR_w = b->op_f[ring.cur]; D.AT = D.AT_w = b->op_a[ring.cur]; }
    int join_s2() {                                     // before s writes operands in place: every GEMM has read them
        if (int rc = wait_G(g_tok)) return rc;
        g_tok = OperandRing::kFree; ring.joined();
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
    // the tail of both single overlapped forms: the GEMM of round k, E_G(k) behind it, reads cur; s waits for the reader of the
    // next set (E_G(k-2)), T(k) exports evaluation k + 1 to it, and it becomes cur
    int tick_beside(long k, int has_eval) {
        const OperandRing::Write w = ring.next_single();
        if (int rc = wait_G(w.wait)) return rc;
        ring.gemm_reads_cur(k); g_tok = k;
        BatchDev Dt = D; Dt.featR_w = b->op_f[w.set]; Dt.AT_w = b->op_a[w.set];
        tick_kernel("tick", Dt, has_eval);
        ring.exported(w.set); point_at_cur();
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
        const long i = ov_i++;
        const int k = (int)(i % SFX_OV_EVENTS);
        if (g_tok == OperandRing::kFree || !last_T) { SFX_CHECK(hipEventRecord(b->ov_ev[0][k], s)); last_T = b->ov_ev[0][k]; }
        SFX_CHECK(hipStreamWaitEvent(b->s2, last_T, 0));
        { ProfScope p("lbs_dense", b->s2, D.nact); launch_lbs_dense(M, D, b->s2); }
        SFX_CHECK(hipEventRecord(b->ov_ev[1][k], b->s2));
        if (int rc = tick_beside(i, 2)) return rc;
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
        const long i = ov_i++;
        const int k = (int)(i % SFX_OV_EVENTS);
        if (b->m->n_key) { ProfScope p("lbs_dense_key", s, D.nact); launch_lbs_dense_list(M, D, b->m->tile_key, b->m->n_key, s); }
        SFX_CHECK(hipEventRecord(b->ov_ev[0][k], s));
        SFX_CHECK(hipStreamWaitEvent(b->s2, b->ov_ev[0][k], 0));
        { ProfScope p("lbs_dense", b->s2, D.nact); launch_lbs_dense_list(M, D, b->m->tile_rest, b->m->n_rest, b->s2); }
        SFX_CHECK(hipEventRecord(b->ov_ev[1][k], b->s2));
        return tick_beside(i, 1);
    }
    // Everything on s: whole-grid GEMM, the interpenetration step (which needs every vertex before the tick), tick; the export
    // goes to cur in place.
    int round_serial() {
        if (int rc = join_s2()) return rc;
        last_T = nullptr;
        { ProfScope p("lbs_dense", s, D.nact); launch_lbs_dense(M, D, s); }
        if (int rc = eval_penetration(b, -2, s, true)) return rc;
        tick_kernel("tick", D, (dense_switches().self_in_serial && !b->pen && M.n_uniq <= SFX_OV_SELF_UNIQ) ? 2 : 1);
        return 0;
    }
    // Multi-round form (where the self-served form applies and the tick kernel has a CU per workgroup: tick_dense_multi_ok).
    // T(i+1) of a frame reads only what T(i) of the same workgroup wrote, so n <= multi_R rounds are ONE launch P whose workgroups
    // loop over their frame's rounds (fused.hip k_tick_dense_multi): no kernel boundary and no cold entry per round, no waiting
    // for the slowest frame of every round, and the workgroups never give their CUs to the GEMM's 655 small ones in between --
    // which is what made single self-served rounds serial again at few columns.  The n GEMMs run beside the NEXT launch:
    //     stream s :  wait E_G(b-2) | P(b): n rounds, reads cur, exports evaluations to the n sets behind it | record E_P(b)
    //     stream s2:  wait E_P(b)   | G x n, a whole-mesh GEMM per evaluation P(b) consumed (cur and all it wrote but the last), in order | record E_G(b)
    // The ring rotates 2 multi_R + 1 sets, so P(b) overwrites exactly what G(b-2) read.  Every evaluation still gets exactly one
    // whole-mesh GEMM, in order, and as in the other forms the evaluation left in cur is the one that has had none: admission and
    // compaction exports find the loop where a serial loop would be.  E_P takes the ring the other forms record E_T / E_K in.
    int launch_multi(int n) {
        const long i = ov_i++;
        const int k = (int)(i % SFX_OV_EVENTS);
        const OperandRing::Launch L = ring.next_multi(n, OperandRing::span(multi_R));
        if (int rc = wait_G(L.wait)) return rc;
        TickSets ts{};
        for (int q = 0; q <= n; ++q) { ts.featR[q] = b->op_f[L.set[q]]; ts.AT[q] = b->op_a[L.set[q]]; }
        { ProfScope p("tick_multi", s, (double)D.nrun * n); launch_tick_dense_multi(M, D, b->vl_dev, b->sw_dev, first_stage, last_stage, ts, n, s); }
        hipEvent_t const e_P = b->ov_ev[0][(k + 1) % SFX_OV_EVENTS];
        SFX_CHECK(hipEventRecord(e_P, s));
        SFX_CHECK(hipStreamWaitEvent(b->s2, e_P, 0));
        for (int q = 0; q < n; ++q) {
            BatchDev Dg = D; Dg.featR = ts.featR[q]; Dg.AT = ts.AT[q];
            ProfScope p("lbs_dense", b->s2, D.nact); launch_lbs_dense(M, Dg, b->s2);
        }
        SFX_CHECK(hipEventRecord(b->ov_ev[1][k], b->s2));
        g_tok = i;
        ring.launched_multi(L, i); point_at_cur();
        return 0;
    }
    // Entering a form that rotates another number of sets (joined): every set of its rotation must hold the last column of the
    // frames that have finished since the latest compaction -- their columns are still skinned, and their workgroups stop
    // copying them before a wider rotation has come round -- so cur goes to all of them, once.  Not before the first round of a
    // fit: nobody has finished.
    int spread_cur(int n_rot) {
        for (int i = 0; i < n_rot; ++i) {
            if (i == ring.cur) continue;
            SFX_CHECK(hipMemcpyAsync(b->op_f[i], b->op_f[ring.cur], (size_t)SFX_KD_PAD * D.Bpad * sizeof(float), hipMemcpyDeviceToDevice, s));
            SFX_CHECK(hipMemcpyAsync(b->op_a[i], b->op_a[ring.cur], (size_t)12 * SFX_JPAD * D.Bpad * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        return 0;
    }
    // One polled batch: rpb rounds, each in the form its count of active columns selects, then the stage flags to poll buffer
    // `buf`.  Multi-round launches at columns <= SFX_OV_MULTI_MAX (LAB_NOTES 4.14); entering a rotation of another size joins.
    // Self-served at SFX_OV_SELF_SERIAL < columns <= SFX_OV_SELF_MAX: the band where the form won (LAB_NOTES 4.9).
    // Key / rest at SFX_OV_SERIAL < columns <= SFX_OV_MAX (LAB_NOTES "GEMM beside tick"): below, a short rest GEMM saves less
    // than it costs the tick kernel it runs beside (frames/s by threshold: 32: 581, 96: 597, 160: 605, 192: 603; serial loop
    // 563); above, 1 024 frames through the 512-column pool lost 6 % overlapped: two tick workgroups per CU and a GEMM that fills
    // the chip leave nothing to share.  The eight-wavefront tick kernel at every size (the four-wavefront one shares its CU with
    // GEMM workgroups and then takes 101 instead of 58 us per launch).
    int rounds(int buf) {
        const DenseSwitches& sw = dense_switches();
        if (sw.dbg_nact) nact_hist[std::min(8, (D.nact - 1) / 32)] += rpb;
        const auto h0 = std::chrono::steady_clock::now();
        const bool multi = self_form && D.nact > 0 && D.nact <= sw.multi_max && OperandRing::span(multi_R) <= b->n_sets && tick_dense_multi_ok(M, D);
        const bool self = !multi && self_form && D.nact > sw.self_serial && D.nact <= sw.self_max;
        const bool key_rest = !multi && !self && overlap && D.nact > sw.ov_serial && D.nact <= SFX_OV_MAX;
        const int rot_new = multi ? OperandRing::span(multi_R) : (self || key_rest) ? 3 : 0;
        if (rot_new != rot && rot_new) {
            if (int rc = join_s2()) return rc;
            last_T = nullptr;
            if (tick > 0) if (int rc = spread_cur(rot_new)) return rc;
        }
        rot = rot_new;
        if (multi) for (int q = 0; q < rpb; q += multi_R) {
            const int n = std::min(multi_R, rpb - q);
            if (int rc = launch_multi(n)) return rc;
            tick += n;
        }
        else for (int q = 0; q < rpb; ++q, ++tick) {
            const int rc = self ? round_self() : key_rest ? round_key_rest() : round_serial();
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
        overlap = sw.ov_on && !b->pen && b->n_sets >= 3;
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
            ring.joined(); point_at_cur();      // (both streams are drained between fits)
            rot = 0;
            tick_kernel("tick", D, 0);
            const double wall0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
            rpb = std::max(1, std::min(64, sw.rpb > 0 ? sw.rpb : 8));
            const int ahead = std::max(1, std::min(SFX_POLL_BUFS - 1, sw.ahead > 0 ? sw.ahead : (b->pen ? 1 : 3)));
            multi_R = OperandRing::rounds_per_launch(sw.multi_R, (long)ahead * rpb);      // (a finished frame stays listed for `ahead` batches)
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
            // the host's side of this loop, accumulated for sfx_loop_host_stats (bench.py reports it next to the kernels' times)
            loop_host_add(host_enq_s, host_wait_s, wall, (double)host_batches * rpb);
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
