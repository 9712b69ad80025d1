// operand_ring.h -- host bookkeeping of the dense loop's GEMM operand sets (host/fit_loop.hip DenseLoop asks, this decides): which
// set holds the latest export (`cur`), which sets a tick launch writes next, and which GEMM event stream s must have waited for
// before it may overwrite them.  A set is one featR / AT pair; the export pass of a tick launch writes a set, a whole-mesh
// GEMM on the second stream reads it.  GEMM events are named by tokens that grow with every launch; the second stream is in
// order, so having waited for a token means having waited for every smaller one.
//   single overlapped rounds (key / rest, self-served): three sets in rotation -- T(i) writes what G(i-2) read.
//   multi-round launches: `span` = 2 R + 1 sets in rotation -- P(b) reads cur and writes the n <= R sets behind it, G(b) reads
//   the n sets P(b)'s rounds read (cur and all it wrote but the last), so P(b+1) writes sets that only G(b-1) read: the GEMMs of
//   a launch run beside the next launch.  (With 2 R sets P(b+1) would overwrite the cur of P(b) and wait for G(b).)
//   in-place exports (first tick of a fit, admission, compaction, the tick of a serial round) write cur itself: joined first.
// In every form cur holds the one evaluation no GEMM has been launched for, as in the serial loop: a compaction finds the same
// GEMM to have been the last over the columns it drops.
// Host only, no device call: tests/operand_ring_check.cpp walks it alone.
#pragma once

struct OperandRing {
    static constexpr int kMaxRounds = 8, kMaxSets = 2 * kMaxRounds + 1;
    static constexpr long kFree = -1;      // no GEMM that s has not waited for reads the set
    int cur = 0;                           // the set of the latest export
    long reader[kMaxSets];                 // token of the latest GEMM event behind a read of the set
    OperandRing() { joined(); }
    // s has waited for the newest GEMM event (or both streams are drained)
    void joined() { for (long& r : reader) r = kFree; }
    // a GEMM launched now, event token e behind it, reads cur
    void gemm_reads_cur(long e) { reader[cur] = e; }

    // One single overlapped round: the set its tick launch exports to and the token s waits for first (kFree: none).
    struct Write { int set; long wait; };
    Write next_single() const { const int t = cur < 3 ? (cur + 1) % 3 : 0; return {t, reader[t]}; }
    void exported(int set) { reader[set] = kFree; cur = set; }

    // One multi-round launch of n rounds over a rotation of `span` >= 2 n + 1 sets: set[0] = cur is read by round 0, round q exports
    // to set[q + 1]; `wait` is the newest token among the readers of the sets written.
    struct Launch { int n; int set[kMaxRounds + 1]; long wait; };
    Launch next_multi(int n, int span) const {
        Launch L{n, {cur}, kFree};
        const int base = cur < span ? cur : span - 1;
        for (int q = 1; q <= n; ++q) {
            L.set[q] = (base + q) % span;
            if (reader[L.set[q]] > L.wait) L.wait = reader[L.set[q]];
        }
        return L;
    }
    // ... launched; the GEMMs of set[0 .. n - 1], the evaluations its rounds consumed, follow it in order, event token e behind the last
    void launched_multi(const Launch& L, long e) {
        for (int q = 0; q < L.n; ++q) reader[L.set[q]] = e;
        cur = L.set[L.n];
    }
    static int span(int R) { return 2 * R + 1; }
    // Rounds per launch: a frame that finishes goes on being listed for `lag_rounds` further rounds (the polling lag), in which
    // its workgroup copies its last column into every set written; all span - 1 = 2 R other sets must be among them, or a GEMM
    // behind a later launch would skin an older evaluation of a frame no workgroup is launched for any more.
    static int rounds_per_launch(int want, long lag_rounds) {
        long r = want < 1 ? 1 : (want > kMaxRounds ? kMaxRounds : want);
        if (2 * r > lag_rounds) r = lag_rounds / 2;
        return r < 1 ? 1 : (int)r;
    }
};
