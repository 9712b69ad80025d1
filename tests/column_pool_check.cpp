// CPU check of the dense loop's column pool (csrc/column_pool.h) on scripted stage-flag snapshots: B frames through `pool`
// columns, driven as csrc/host/fit_loop.hip DenseLoop::poll drives it (retire, then admission / compaction by slice_emptied / nothing),
// with snapshots that lag behind the admissions as the polled loop's do.  After every poll: the frame -> column map and the
// running list against what the poll's retirements dictate; and the compaction rule's table.  Stand-alone: own main, no
// device.  Built and run by tests/test_column_pool_host.py (host AddressSanitizer + UBSan).
#include "../smplify-x-partial_amd/csrc/column_pool.h"
#include <algorithm>
#include <cstdio>
#include <set>

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { if (++g_fail <= 40) printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)

enum { LAST = 2, START = 0 };       // a frame runs while its stage flag is <= LAST; a queued or newly admitted frame shows START

// need[f]: polls between frame f's admission and the first snapshot taken after it has finished; the snapshot examined at poll p
// was taken `lag` polls earlier (frames admitted since then show START)
static void walk(const char* name, int B, int pool, const std::vector<int>& need, int lag) {
    ColumnPool P;
    P.reset(B, pool);
    int nact = pool, compactions = 0, polls = 0, retired_total = 0;
    std::vector<int> admitted_at(B, -1), order;               // poll of admission (-1: queued); frames in order of admission
    std::vector<bool> gone(B, false);
    for (int f = 0; f < pool; ++f) { admitted_at[f] = 0; order.push_back(f); }
    CHECK((int)P.run.size() == pool && (int)P.col.size() == B);
    for (int f = 0; f < B; ++f) CHECK(P.col[f] == (f < pool ? f : -1));
    std::vector<int> snap(B), fresh;
    while (!P.run.empty() && polls < 100000) {
        ++polls;
        for (int f = 0; f < B; ++f)        // retired frames go on showing LAST + 1
            snap[f] = (admitted_at[f] >= 0 && admitted_at[f] + need[f] <= polls - lag) ? LAST + 1 : (f % (LAST + 1));
        for (int f = 0; f < B; ++f) if (admitted_at[f] < 0 || admitted_at[f] > polls - lag) snap[f] = START;
        const std::vector<int> run0 = P.run, col0 = P.col;
        std::vector<int> survivors, freed;
        for (int f : run0) { if (snap[f] <= LAST) survivors.push_back(f); else { freed.push_back(col0[f]); gone[f] = true; } }
        const int queued = B - (int)order.size();
        const bool changed = P.retire(snap.data(), LAST, fresh);
        retired_total += (int)freed.size();
        CHECK(changed == !freed.empty());
        // admission: in queue order, exactly the freed columns in retirement order, the surplus stays vacant
        CHECK((int)fresh.size() == std::min(queued, (int)freed.size()));
        for (size_t i = 0; i < fresh.size(); ++i) {
            CHECK(fresh[i] == (int)order.size());
            CHECK(i < freed.size() && P.col[fresh[i]] == freed[i]);
            CHECK(admitted_at[fresh[i]] == -1);
            admitted_at[fresh[i]] = polls; order.push_back(fresh[i]);
        }
        // survivors keep their order and come before the admitted frames
        std::vector<int> expect = survivors;
        expect.insert(expect.end(), fresh.begin(), fresh.end());
        CHECK(P.run == expect);
        for (size_t i = fresh.size(); i < freed.size(); ++i)
            for (int f : P.run) CHECK(P.col[f] != freed[i]);
        // what DenseLoop::poll does with it
        const bool done = P.run.empty();
        if (!done && changed && fresh.empty() && ColumnPool::slice_emptied(nact, (int)P.run.size())) {
            nact = P.compact();
            ++compactions;
            CHECK(nact == (int)P.run.size());
            for (size_t i = 0; i < P.run.size(); ++i) CHECK(P.col[P.run[i]] == (int)i);
            CHECK(P.run == expect);
        }
        // the map: running frames hold distinct columns below nact, everybody else none
        std::set<int> held;
        const std::set<int> running(P.run.begin(), P.run.end());
        CHECK(running.size() == P.run.size());
        for (int f = 0; f < B; ++f) {
            const int c = P.col[f];
            if (running.count(f)) { CHECK(c >= 0 && c < nact); CHECK(held.insert(c).second); CHECK(!gone[f] && admitted_at[f] >= 0); }
            else CHECK(c == -1);
        }
        CHECK(done == (retired_total == B));                   // the loop ends exactly when everybody has retired
        // a snapshot that shows only retired frames as finished and every running one at START changes nothing
        const std::vector<int> run1 = P.run, col1 = P.col;
        for (int f = 0; f < B; ++f) snap[f] = gone[f] ? LAST + 1 : START;
        std::vector<int> none;
        CHECK(!P.retire(snap.data(), LAST, none));
        CHECK(none.empty() && P.run == run1 && P.col == col1);
    }
    CHECK(P.run.empty() && retired_total == B && (int)order.size() == B);
    for (int f = 0; f < B; ++f) { CHECK(order[f] == f); CHECK(P.col[f] == -1); }
    printf("%s: %d frames through %d columns, lag %d: %d polls, %d compactions, %d columns at the end\n", name, B, pool, lag, polls, compactions, nact);
}

int main() {
    const struct { const char* name; int B, pool; } shapes[] = {
        {"tiny", 5, 2}, {"resident", 32, 32}, {"three-waves", 70, 32}, {"half-wave", 48, 32}, {"slice-of-16", 40, 16}};
    for (const auto& sh : shapes)
        for (int lag : {0, 3}) {
            std::vector<int> need(sh.B);
            for (int f = 0; f < sh.B; ++f) need[f] = 1 + (f * 7) % 5 + (f % 11 == 3 ? 6 : 0);      // neighbours finish apart, some much later
            walk(sh.name, sh.B, sh.pool, need, lag);
        }
    {   // everybody at once: a whole wave retires in one poll, the last wave leaves columns vacant
        walk("lock-step", 70, 32, std::vector<int>(70, 2), 1);
    }
    {   // one fixed-seed random finishing order
        unsigned seed = 20240611u;
        std::vector<int> need(200);
        for (int& n : need) { seed = seed * 1664525u + 1013904223u; n = 1 + (int)((seed >> 16) % 23u); }
        walk("random", 200, 64, need, 3);
    }
    // the compaction rule: a 32-frame MFMA slice has emptied, or the columns fit ONE 16-frame slice for the first time
    const struct { int nact, nrun; bool compact; } rule[] = {
        {64, 33, false}, {64, 32, true}, {33, 32, true}, {32, 17, false}, {32, 16, true}, {17, 16, true}, {16, 9, false}, {16, 1, false}};
    for (const auto& r : rule) CHECK(ColumnPool::slice_emptied(r.nact, r.nrun) == r.compact);
    printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
