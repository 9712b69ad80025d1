// column_pool.h -- host bookkeeping of the dense loop's column pool (continuous batching, cfg.slots; host/fit_loop.hip DenseLoop).
// `pool` GEMM columns; frames beyond the first `pool` wait in a queue (column -1, not in the running list) and take over the
// column of a frame that has finished.  Frames are independent and a column's arithmetic does not depend on its index: results
// equal those of a batch with one column per frame.  Host only, no device call: tests/column_pool_check.cpp walks it alone.
#pragma once
#include <vector>

struct ColumnPool {
    std::vector<int> col;        // frame -> column, -1 = queued or retired          (both: read by the upload, written here only)
    std::vector<int> run;        // running frames, ascending admission order
    int next_q = 0;              // head of the queue: frames next_q .. B - 1 wait
    void reset(int B, int pool) {
        col.assign(B, -1);
        run.clear(); run.reserve(B);
        for (int i = 0; i < pool; ++i) { col[i] = i; run.push_back(i); }
        next_q = pool;
    }
    // One poll.  stage[f] > last_stage: frame f has finished (a snapshot older than a frame's admission shows its start stage).
    // Survivors keep their order; each retired frame's column goes to the next queued frame; the admitted frames are appended
    // to the running list and returned in `fresh`.  True when a frame retired.
    bool retire(const int* stage, int last_stage, std::vector<int>& fresh) {
        fresh.clear();
        size_t w = 0;
        for (size_t r = 0; r < run.size(); ++r) {
            const int f = run[r];
            if (stage[f] <= last_stage) { run[w++] = f; continue; }
            const int c = col[f];
            col[f] = -1;
            if (next_q < (int)col.size()) { const int nf = next_q++; col[nf] = c; fresh.push_back(nf); }
        }
        const bool changed = w != run.size();
        run.resize(w);
        run.insert(run.end(), fresh.begin(), fresh.end());
        return changed;
    }
    // Queue dry: compact when a 32-frame MFMA slice has emptied, and also down to ONE 16-frame slice (the few-frames GEMM's
    // floor is 17.5 us there, 23 at two slices)
    static bool slice_emptied(int nact, int nrun) { return (nact + 31) / 32 != (nrun + 31) / 32 || (nact > 16 && nrun <= 16); }
    int compact() {              // running frame i takes column i; returns the new count of active columns
        int q = 0;
        for (int f : run) col[f] = q++;
        return q;
    }
};
