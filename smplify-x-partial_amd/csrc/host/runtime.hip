// runtime.hip -- what every unit of the host layer leans on: the thread-local error string, the version, the HIP-event profiler
// behind ProfScope, the host statistics of the polled loops and the float64 mode's guards.
#include "host.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>

static thread_local char g_err[1024] = "";
void sfx_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
extern "C" const char* sfx_last_error(void) { return g_err; }
extern "C" const char* sfx_version(void) { return "sfx 0.1.0 (gfx950)"; }

int refuse_f64(const sfx_batch* b, const char* fn) {
    if (b && b->f64) {
        sfx_set_error("%s: not available on a float64 batch (high_precision = 2): use the _f64 entry points", fn); return -1; }
    return 0;
}
int need_f64(const sfx_batch* b, const char* fn) {
    if (!b) { sfx_set_error("null batch"); return -1; }
    if (!b->f64) { sfx_set_error("%s: the batch is not in float64 mode (high_precision = 2)", fn); return -1; }
    return 0;
}
bool fp32_exact(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!((double)(float)v[i] == v[i]) && !std::isnan(v[i])) return false;
    return true;
}

// ---------------------------------------------------------------------------------------
// profiling: HIP-event timing of named kernels on the launch stream
struct ProfAcc { double ms = 0; int64_t n = 0, seen = 0; double units = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> pend; };
int g_prof = 0;
static int g_prof_every = 1;  // time every N-th launch of a name (events cost a queue packet each)
int g_unfused = 0;
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
void ProfScope::begin(double units) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto& a = g_acc[name];
    if (a.seen++ % g_prof_every) return;
    a.units += units;
    e0 = ev_get(); e1 = ev_get();
    hipEventRecord(e0, s);
}
void ProfScope::end() {
    hipEventRecord(e1, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto& a = g_acc[name]; a.pend.push_back({e0, e1});
    if (a.pend.size() > 4096) prof_flush(a);
}
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
void loop_host_add(double enq_s, double wait_s, double wall_s, double rounds) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_loop_host[0] += enq_s; g_loop_host[1] += wait_s; g_loop_host[2] += wall_s; g_loop_host[3] += rounds;
}
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
