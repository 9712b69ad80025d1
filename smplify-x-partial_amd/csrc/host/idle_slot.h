// idle_slot.h -- the one owner of a model's idle collision handle.  The collision buffers of the interpenetration term (~45 MB
// per GEMM column: 11.5 GB for 256 columns) outlive the batch that used them: a job is a sequence of batches on one model
// (driver.fit_frames per (gender, H, W) group, bench.py per step), and returning 11 GB to the driver and asking for them again
// cost 10 ms on some boxes and 450 ms per batch on others (round 6: `outside_loop_ms_per_step` of the --workload pen line, 402
// against 239 frames/s for the same kernels).  ONE idle handle is kept per model; it is reused when it holds at least the
// columns asked for, at the same max_collisions (cap) and part table (generation).  Host only, no device call of its own: the
// handle type and its destroy function are the template's arguments, and tests/idle_slot_check.cpp walks it with counted dummies.
#pragma once
#include <mutex>

template <class H, void (*Destroy)(H*)>
class IdleSlot {
    H* h_ = nullptr;
    int cols_ = 0, cap_ = 0, gen_ = -1;
    mutable std::mutex mu_;
    void drop_locked() { if (h_) { Destroy(h_); h_ = nullptr; } }
public:
    IdleSlot() = default;
    IdleSlot(const IdleSlot&) = delete;
    IdleSlot& operator=(const IdleSlot&) = delete;
    ~IdleSlot() { drop(); }
    // The idle handle, now the caller's, if it holds at least `cols` columns at this cap and generation (*got_cols: how many it
    // holds).  Otherwise nullptr, and whatever was idle -- too small / another cap / another table -- is destroyed: room first.
    H* take(int cols, int cap, int gen, int* got_cols) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!h_ || cols_ < cols || cap_ != cap || gen_ != gen) { drop_locked(); return nullptr; }
        H* h = h_; h_ = nullptr;
        *got_cols = cols_;
        return h;
    }
    // A handle comes back: kept if it was made for the current part table and is not smaller than what is idle; the loser of the
    // two is destroyed either way.
    void give(H* h, int cols, int cap, int gen, int current_gen) {
        std::lock_guard<std::mutex> lk(mu_);
        if (gen != current_gen || (h_ && cols_ > cols)) { Destroy(h); return; }
        drop_locked();
        h_ = h; cols_ = cols; cap_ = cap; gen_ = gen;
    }
    void drop() { std::lock_guard<std::mutex> lk(mu_); drop_locked(); }
    const H* idle() const { std::lock_guard<std::mutex> lk(mu_); return h_; }      // (for the host test)
};
