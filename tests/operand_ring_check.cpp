// CPU check of the dense loop's operand-set bookkeeping (csrc/operand_ring.h) on scripted sequences of round forms, driven as
// csrc/host/fit_loop.hip DenseLoop drives it: single self-served rounds, key / rest rounds, serial rounds, multi-round launches
// with R = 1, 3 and 8 (batches that R does not divide included), admission and compaction exports between them, several fits
// on one ring.  A model of the two streams runs beside the ring and after every step checks that
//   - no set is handed out for writing while a GEMM that reads it has not been waited for by the tick stream, and no wait names
//     an event whose slot in the ring of SFX_OV_EVENTS events has been recorded again;
//   - every exported evaluation is read by exactly one GEMM, in order;
//   - `cur` is the set of the latest export, and after a drain the export target is cur again;
//   - a frame that finishes and is retired by the host `lag` rounds later leaves its last column in every set a later GEMM reads
//     (also one that retired before the loop entered the multi-round form).
// Stand-alone: own main, no device.  Built and run by tests/test_operand_ring_host.py (host AddressSanitizer + UBSan).
#include "../smplify-x-partial_amd/csrc/operand_ring.h"
#include <algorithm>
#include <cstdio>
#include <vector>

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { if (++g_fail <= 40) printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)

enum Form { SELF, KEYREST, SERIAL, MULTI };
enum { EVENTS = 4, NSETS = OperandRing::kMaxSets };      // SFX_OV_EVENTS of host.h

struct Model {
    OperandRing ring;                        // (outlives a fit, like sfx_batch's)
    // the streams
    long ov_i = 0, g_tok = OperandRing::kFree, waited = -1;      // waited: s has waited for every GEMM token <= this
    std::vector<long> readers[NSETS];        // tokens of the GEMMs launched on each set's current content
    // the evaluations: content[set] = id of the evaluation the running frames' columns hold there
    long content[NSETS], next_eval = 0, latest_set = 0, last_gemm_eval = -1;
    std::vector<int> reads;                  // GEMM launches per evaluation id
    // one tracked frame: runs until round `fin`, is listed until round `delist`; colval[set] = the evaluation its column holds
    long fin = -1, delist = -1, round = 0, final_eval = -1, colval[NSETS];
    int rot = 0, multi_R = 1;               // sets in the rotation of the latest batch's form (0: in place)
    Model() { for (int i = 0; i < NSETS; ++i) { content[i] = -1; colval[i] = -1; } }

    bool listed() const { return delist < 0 || round < delist; }
    bool finished() const { return fin >= 0 && round >= fin; }
    void wait_G(long tok) {
        if (tok == OperandRing::kFree) return;
        CHECK(tok > ov_i - 1 - EVENTS);      // its event slot has not been recorded again
        waited = std::max(waited, tok);
    }
    void join() { wait_G(g_tok); g_tok = OperandRing::kFree; ring.joined(); }
    void gemm(int set, long tok) {           // a whole-mesh GEMM reads `set`, event `tok` behind it
        const long e = content[set];
        CHECK(e >= 0 && e == last_gemm_eval + 1);      // every evaluation once, in order
        last_gemm_eval = std::max(last_gemm_eval, e);
        if (e >= 0 && e < (long)reads.size()) ++reads[e];
        if (tok >= 0) readers[set].push_back(tok);      // (a serial round's GEMM runs on s itself, in order with its tick)
        if (final_eval >= 0 && !listed()) CHECK(colval[set] == final_eval);      // a retired frame's column: its last evaluation
    }
    // the export of one round lands in `set`.  In place (admission, compaction, the first tick of a fit) it completes a pending
    // evaluation no GEMM has read yet, or starts a new one; finished frames export nothing there.
    void write(int set, bool in_place) {
        for (long tok : readers[set]) CHECK(tok <= waited);
        readers[set].clear();
        const bool pending = in_place && content[set] >= 0 && reads[content[set]] == 0;
        if (!pending) { content[set] = next_eval++; reads.push_back(0); }
        if (listed() && !(in_place && finished())) colval[set] = finished() ? final_eval : content[set];
        latest_set = set;
    }
    void after_step() { CHECK(ring.cur == latest_set); }

    void export_in_place() {                  // first tick of a fit, admission, compaction: joined, writes cur
        join();
        CHECK(ring.cur == latest_set);
        write(ring.cur, true); after_step();
    }
    void tick_round() {                       // the tracked frame's tick of this round
        if (fin >= 0 && round == fin) final_eval = colval[latest_set];      // it finishes on the evaluation it has just consumed
    }
    void single(Form f) {
        if (f == SERIAL) {
            join();
            gemm(ring.cur, -2);
            tick_round();
            write(ring.cur, true);
        } else {
            const long i = ov_i++;
            gemm(ring.cur, i);
            const OperandRing::Write w = ring.next_single();
            CHECK(w.set != ring.cur && w.set < 3);
            wait_G(w.wait);
            ring.gemm_reads_cur(i); g_tok = i;
            tick_round();
            write(w.set, false); ring.exported(w.set);
        }
        ++round; after_step();
    }
    void multi(int n) {
        const long i = ov_i++;
        const OperandRing::Launch L = ring.next_multi(n, OperandRing::span(multi_R));
        CHECK(L.n == n && L.set[0] == ring.cur);
        for (int q = 1; q <= n; ++q) { CHECK(L.set[q] != ring.cur && L.set[q] < OperandRing::span(multi_R)); for (int p = 1; p < q; ++p) CHECK(L.set[p] != L.set[q]); }
        wait_G(L.wait);
        for (int q = 1; q <= n; ++q) { tick_round(); write(L.set[q], false); ++round; }
        for (int q = 0; q < n; ++q) gemm(L.set[q], i);      // behind the launch: the evaluations its rounds consumed
        g_tok = i; ring.launched_multi(L, i);
        after_step();
    }
    void batch(Form f, int rpb) {
        const bool m = f == MULTI;
        const int rot_new = m ? OperandRing::span(multi_R) : f == SERIAL ? 0 : 3;
        if (rot_new != rot && rot_new) {      // (DenseLoop::spread_cur: joined, cur is copied to every set of the rotation the loop enters)
            join();
            for (int s = 0; s < rot_new; ++s) if (s != ring.cur) { CHECK(readers[s].empty() || readers[s].back() <= waited); colval[s] = colval[ring.cur]; }
        }
        rot = rot_new;
        if (m) for (int q = 0; q < rpb; q += multi_R) multi(std::min(multi_R, rpb - q));
        else for (int q = 0; q < rpb; ++q) single(f);
    }
    void begin_fit(int want_R, int rpb, int ahead) {
        ov_i = 0; g_tok = OperandRing::kFree; waited = -1; rot = 0;      // both streams drained, a new DenseLoop
        for (auto& r : readers) r.clear();
        ring.joined();
        reads.assign(next_eval, 1); last_gemm_eval = next_eval - 1;      // (the last fit's pending evaluation is never skinned)
        if (content[ring.cur] >= 0) { content[ring.cur] = next_eval++; reads.push_back(0); }
        multi_R = OperandRing::rounds_per_launch(want_R, (long)ahead * rpb);
        CHECK(multi_R >= 1 && multi_R <= want_R && 2 * multi_R <= (long)ahead * rpb + 1);
        export_in_place();
    }
    void end_fit() {                          // every evaluation but the pending one has had exactly one GEMM
        for (size_t e = 0; e + 1 < reads.size(); ++e) CHECK(reads[e] == 1);
        CHECK(reads.empty() || reads.back() <= 1);
        join();
    }
};

struct Step { Form f; int batches; int event; };      // event after the batches: 0 none, 1 admission export, 2 compaction export

// one fit: the script's forms in turn; the tracked frame finishes at round `fin` and is delisted `ahead` batches after the batch it
// finished in, as the polled loop's lag has it
static void fit(Model& M, const char* name, const std::vector<Step>& script, int R, int rpb, int ahead, long fin) {
    M.begin_fit(R, rpb, ahead);
    M.round = 0; M.fin = fin; M.delist = fin < 0 ? -1 : (fin / rpb + 1 + ahead) * (long)rpb; M.final_eval = -1;
    for (const Step& st : script) {
        for (int k = 0; k < st.batches; ++k) M.batch(st.f, rpb);
        if (st.event) M.export_in_place();
    }
    M.end_fit();
    printf("%s: R %d (launches of %d), %d rounds per batch, %d ahead: %ld rounds, %ld evaluations, %ld event tokens\n",
           name, R, M.multi_R, rpb, ahead, M.round, M.next_eval, M.ov_i);
}

int main() {
    const std::vector<Step> down = {{KEYREST, 3, 0}, {SELF, 4, 2}, {SELF, 2, 2}, {MULTI, 5, 2}, {MULTI, 9, 0}};      // a resident job, compacting on its way down
    const std::vector<Step> pool = {{MULTI, 2, 1}, {MULTI, 1, 1}, {MULTI, 3, 1}, {MULTI, 2, 2}, {MULTI, 6, 0}};      // admissions between multi-round batches
    const std::vector<Step> mixed = {{SERIAL, 2, 0}, {SELF, 2, 0}, {KEYREST, 2, 0}, {SELF, 1, 1}, {MULTI, 3, 0}, {SERIAL, 2, 0}, {SELF, 3, 0}, {MULTI, 2, 2},
                                     {KEYREST, 1, 0}, {MULTI, 4, 0}};                                                 // every change of form, both ways
    const std::vector<Step> serial = {{SERIAL, 6, 2}, {SERIAL, 3, 0}};
    const struct { int R, rpb, ahead; } shapes[] = {{8, 8, 3}, {3, 7, 3}, {1, 7, 3}, {8, 8, 1}, {8, 3, 1}, {4, 8, 2}, {8, 64, 1}, {2, 1, 1}};
    for (const auto& sh : shapes) {
        Model M;                                 // one ring through all the fits of a shape: each starts where the last one ended
        for (long fin : {-1L, 0L, 5L, (long)sh.rpb * 4 + 2, (long)sh.rpb * 9 - 1, (long)sh.rpb * 13}) {
            fit(M, "down", down, sh.R, sh.rpb, sh.ahead, fin);
            fit(M, "pool", pool, sh.R, sh.rpb, sh.ahead, fin);
            fit(M, "mixed", mixed, sh.R, sh.rpb, sh.ahead, fin);
            fit(M, "serial", serial, sh.R, sh.rpb, sh.ahead, fin);
        }
    }
    // the launch size rule: 2 R sets must be written while a finished frame is still listed
    CHECK(OperandRing::rounds_per_launch(8, 24) == 8 && OperandRing::rounds_per_launch(8, 8) == 4 && OperandRing::rounds_per_launch(3, 21) == 3);
    CHECK(OperandRing::rounds_per_launch(8, 15) == 7 && OperandRing::span(8) == OperandRing::kMaxSets);
    CHECK(OperandRing::rounds_per_launch(0, 24) == 1 && OperandRing::rounds_per_launch(99, 1000) == OperandRing::kMaxRounds && OperandRing::rounds_per_launch(8, 1) == 1);
    printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
