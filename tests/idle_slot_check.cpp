// CPU check of the owner of a model's idle collision handle (csrc/host/idle_slot.h), driven with counted dummy handles as
// csrc/host/batch.hip (sfx_batch_create takes, ~sfx_batch gives) and csrc/host/model.hip (sfx_model_set_parts drops) drive it.
// After every operation: which handle is idle, and how often each handle made so far has been destroyed; at the end every handle
// has been destroyed exactly once.  Stand-alone: own main, no device.  Built and run by tests/test_idle_slot_host.py (host
// AddressSanitizer + UBSan).
#include "../smplify-x-partial_amd/csrc/host/idle_slot.h"
#include <cstdio>
#include <vector>

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { if (++g_fail <= 40) printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)

struct Dummy { int id; };
static std::vector<int> g_destroyed;        // per handle made, in order of making
static Dummy* make() { g_destroyed.push_back(0); return new Dummy{(int)g_destroyed.size() - 1}; }
static void destroy(Dummy* d) { ++g_destroyed[d->id]; delete d; }
using Slot = IdleSlot<Dummy, destroy>;

// the slot holds `idle` (nullptr: nothing) and exactly the handles in `dead` (by id) have been destroyed, once each
static void expect(const Slot& S, const Dummy* idle, std::vector<int> dead) {
    CHECK(S.idle() == idle);
    std::vector<int> want(g_destroyed.size(), 0);
    for (int id : dead) want[id] = 1;
    CHECK(g_destroyed == want);
}

int main() {
    enum { CAP = 128, GEN = 3 };
    {
        Slot S;
        int got = -1;
        // take from empty
        CHECK(S.take(32, CAP, GEN, &got) == nullptr && got == -1);
        expect(S, nullptr, {});
        // give into empty
        Dummy* h0 = make();                                     // id 0: 64 columns
        S.give(h0, 64, CAP, GEN, GEN);
        expect(S, h0, {});
        // take exact
        CHECK(S.take(64, CAP, GEN, &got) == h0 && got == 64);
        expect(S, nullptr, {});
        S.give(h0, 64, CAP, GEN, GEN);
        // take larger-than-asked: the caller learns what the handle holds
        got = -1;
        CHECK(S.take(32, CAP, GEN, &got) == h0 && got == 64);
        expect(S, nullptr, {});
        S.give(h0, 64, CAP, GEN, GEN);
        // take too small: the idle one is destroyed (room first), the caller makes its own
        got = -1;
        CHECK(S.take(96, CAP, GEN, &got) == nullptr && got == -1);
        expect(S, nullptr, {0});
        Dummy* h1 = make();                                     // id 1: 96 columns
        S.give(h1, 96, CAP, GEN, GEN);
        expect(S, h1, {0});
        // cap mismatch
        CHECK(S.take(32, CAP / 2, GEN, &got) == nullptr);
        expect(S, nullptr, {0, 1});
        Dummy* h2 = make();                                     // id 2: 32 columns at CAP / 2
        S.give(h2, 32, CAP / 2, GEN, GEN);
        expect(S, h2, {0, 1});
        CHECK(S.take(32, CAP, GEN, &got) == nullptr);           // ... and the other way round
        expect(S, nullptr, {0, 1, 2});
        // stale generation: the part table changed after the idle handle was made (without a drop in between)
        Dummy* h3 = make();                                     // id 3
        S.give(h3, 64, CAP, GEN, GEN);
        CHECK(S.take(64, CAP, GEN + 1, &got) == nullptr);
        expect(S, nullptr, {0, 1, 2, 3});
        // give smaller than idle: the given one is destroyed
        Dummy *h4 = make(), *h5 = make();                       // ids 4 (64 columns), 5 (32 columns)
        S.give(h4, 64, CAP, GEN, GEN);
        S.give(h5, 32, CAP, GEN, GEN);
        expect(S, h4, {0, 1, 2, 3, 5});
        // give equal: the idle one is destroyed
        Dummy* h6 = make();                                     // id 6: 64 columns
        S.give(h6, 64, CAP, GEN, GEN);
        expect(S, h6, {0, 1, 2, 3, 4, 5});
        // give larger: the idle one is destroyed
        Dummy* h7 = make();                                     // id 7: 128 columns
        S.give(h7, 128, CAP, GEN, GEN);
        expect(S, h7, {0, 1, 2, 3, 4, 5, 6});
        CHECK(S.take(100, CAP, GEN, &got) == h7 && got == 128);
        S.give(h7, 128, CAP, GEN, GEN);
        // give with stale generation: destroyed, whatever is idle stays
        Dummy* h8 = make();                                     // id 8: made for generation GEN - 1, larger than the idle one
        S.give(h8, 256, CAP, GEN - 1, GEN);
        expect(S, h7, {0, 1, 2, 3, 4, 5, 6, 8});
        // ... also into an empty slot
        CHECK(S.take(128, CAP, GEN, &got) == h7);
        Dummy* h9 = make();                                     // id 9
        S.give(h9, 64, CAP, GEN - 1, GEN);
        expect(S, nullptr, {0, 1, 2, 3, 4, 5, 6, 8, 9});
        S.give(h7, 128, CAP, GEN, GEN);
        // drop, twice
        S.drop();
        expect(S, nullptr, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9});
        S.drop();
        expect(S, nullptr, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9});
        // destruction with one idle
        Dummy* h10 = make();                                    // id 10
        S.give(h10, 16, CAP, GEN, GEN);
        expect(S, h10, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9});
    }
    CHECK(g_destroyed.size() == 11);
    for (int n : g_destroyed) CHECK(n == 1);                    // every handle made: destroyed exactly once
    { Slot empty; }                                             // destruction with nothing idle
    printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
