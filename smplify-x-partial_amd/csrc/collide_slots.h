// collide_slots.h -- the layout of the interpenetration term's two diagnostic arrays: the per-mesh `stats` row (PenDev::stats,
// [B][PEN_STATS] int) and the process-wide `work` counters (PenDev::work, [PEN_WORK_SLOTS] unsigned long long).  Every index
// into either, on the device and on the host, is one of these names.  Plain C++ for host and device, no HIP header
// (tests/collide_slots_check.cpp compiles it alone).
#pragma once
#include <cstdint>

#ifdef PEN_COUNT
#define PEN_STATS 32            // diagnostic build: room for the walk counters and k_pen_g3's phase cycles
#else
#define PEN_STATS 16
#endif

// ---- the stats row of one mesh, rewritten by every evaluation
enum PenStat : int {
    PEN_ST_PAIRS     = 0,       // ordered pairs in the list (k_pen_list / pen_narrow; 0 from k_pen_g3 for a skipped or overflowed mesh)
    PEN_ST_DROPPED   = 1,       // partners dropped by the max_collisions cap
    PEN_ST_OVERFLOW  = 2,       // grid-entry overflow: the entries the mesh wanted (0 = they fitted); k_pen_list and k_pen_narrow skip such a mesh
    PEN_ST_CELLS     = 3,       // the constant PEN_CELLS, stored by k_pen_g3.  NO READER on the device, the host or in Python.
    PEN_ST_CLOCK0    = 4,       // the window sfx_pen_phase_clocks copies out: PEN_CLOCK_COLS slots from here (columns below)
    PEN_ST_WALKS_CUT = 13,      // bucket walks cut short at PEN_MAX_WALK entries (k_pen_walk counts; k_pen_narrow zeroes it at a hand-over)
    PEN_ST_ENTRIES   = 14,      // grid entries (k_pen_g3)
    PEN_ST_ONE_SIDED = 15,      // ordered pairs in the list that only one of the two triangles kept: they contribute nothing
    // -DPEN_COUNT only (stride 32)
    PEN_ST_CNT_WALKED  = 16,    // candidates of the pair tests: walked, ...
    PEN_ST_CNT_CELL    = 17,    // ... in the same cell, ...
    PEN_ST_CNT_PARTS   = 18,    // ... past the part mask, ...
    PEN_ST_CNT_BOXES   = 19,    // ... with overlapping boxes;
    PEN_ST_CNT_STEPS   = 20,    // wavefront steps of the walk
    PEN_ST_G3_CYCLES0  = 24,    // k_pen_g3's shader cycles per phase, PEN_G3_PHASES slots: init, part masks, histogram, scan, scatter, copy
};
// Columns of the clock window, [B][PEN_CLOCK_COLS] of sfx_pen_phase_clocks (column k = slot PEN_ST_CLOCK0 + k).  k_pen_g3 zeroes
// columns 0-8; only k_pen_narrow stamps, in the lab build (-DSFX_LAB: 100 MHz ticks since its start, at the ends of phases D-G),
// so columns 3-6 stay 0 in form 0 and for a handed-over mesh.  Columns 0-2 and 7-8 have no writer but that zeroing (their stamps went with k_pen_frame).
// Columns 9 and 10 are the two counts above: they lie in the window, not among the stamps.
enum PenClockCol : int {
    PEN_CLK_LIST = 3, PEN_CLK_EVAL = 4, PEN_CLK_SUMS = 5, PEN_CLK_VERTS = 6,      // end of D pair list, E pair evaluation, F triangle sums, G vertices + loss
    PEN_CLK_WALKS_CUT = PEN_ST_WALKS_CUT - PEN_ST_CLOCK0,      // = 9: a count
    PEN_CLK_ENTRIES   = PEN_ST_ENTRIES - PEN_ST_CLOCK0,        // = 10: a count
    PEN_CLOCK_COLS = 11,
};
constexpr int PEN_G3_PHASES = 6;

// ---- the work counters: sums since sfx_pen_work_reset over every handle of the process
constexpr int PEN_WORK_SLOTS = 16;
enum PenWork : int {
    PEN_WK_ENTRIES   = 0,       // grid entries
    PEN_WK_PAIRS     = 1,       // ordered pairs
    PEN_WK_COLUMNS   = 2,       // column evaluations (meshes that went through k_pen_g3's grid build)
    PEN_WK_SURVIVORS = 3,       // triangles that survived the part culling
    PEN_WK_LONG      = 4,       // triangles with more partners than the lists hold (2 x max_collisions)
    PEN_WK_WALKS_CUT = 5,       // bucket walks cut short
    PEN_WORK_PUBLIC  = 6,       // what sfx_pen_work_get returns: slots [0, 6); 6-7 are unused
    PEN_WK_DEBUG0    = 8,       // slots [8, 16): ONE of the two debug views below
};
constexpr int PEN_WORK_DEBUG = PEN_WORK_SLOTS - PEN_WK_DEBUG0;      // what sfx_debug_pen_phase_ticks returns
// The two views of work[8..15] exclude each other.  PenWorkNarrow is written by k_pen_narrow in the lab build (-DSFX_LAB) and
// read by sfx_debug_pen_phase_ticks.  PenWorkRank is written by k_pen_rank under -DPEN_RANKT, a diagnostic build read with the same
// call (tools/pen_rank_probe.py), in which sfx_debug_pen_phase_ticks therefore means nothing for k_pen_narrow.
enum PenWorkNarrow : int {      // 100 MHz ticks summed over k_pen_narrow's column evaluations
    PEN_WKN_ENTRY = 8, PEN_WKN_LIST = 9, PEN_WKN_EVAL = 10, PEN_WKN_SUMS = 11, PEN_WKN_VERTS = 12,      // until the pairs are read, then phases D-G
    PEN_WKN_EVALS = 13,         // number of such evaluations
    PEN_WKN_PAIRS = 14,         // their ordered pairs (15: unused)
};
enum PenWorkRank : int {        // -DPEN_RANKT: k_pen_rank's wavefronts that took more than 40 us
    PEN_WKR_WAVES = 8, PEN_WKR_T_RANK = 9, PEN_WKR_T_LONG = 10, PEN_WKR_T_REWALK = 11, PEN_WKR_N_LONG = 12, PEN_WKR_N_REWALK = 13,
    PEN_WKR_T_LOAD = 14, PEN_WKR_T_SHORT = 15,
};

namespace pen_slots_detail {
constexpr int always[] = {PEN_ST_PAIRS, PEN_ST_DROPPED, PEN_ST_OVERFLOW, PEN_ST_CELLS, PEN_ST_CLOCK0 + PEN_CLK_LIST, PEN_ST_CLOCK0 + PEN_CLK_EVAL,
                          PEN_ST_CLOCK0 + PEN_CLK_SUMS, PEN_ST_CLOCK0 + PEN_CLK_VERTS, PEN_ST_WALKS_CUT, PEN_ST_ENTRIES, PEN_ST_ONE_SIDED};
constexpr bool distinct_below(const int* v, int n, int bound) {
    for (int i = 0; i < n; ++i) { if (v[i] < 0 || v[i] >= bound) return false; for (int j = 0; j < i; ++j) if (v[i] == v[j]) return false; }
    return true;
}
}
static_assert(pen_slots_detail::distinct_below(pen_slots_detail::always, 11, 16), "the always-present stats slots are distinct and fit the stride of 16");
static_assert(PEN_ST_CNT_WALKED >= 16 && PEN_ST_CNT_STEPS < PEN_ST_G3_CYCLES0 && PEN_ST_G3_CYCLES0 + PEN_G3_PHASES <= 32, "the PEN_COUNT slots fit the stride of 32");
static_assert(PEN_ST_CLOCK0 + PEN_CLOCK_COLS <= 16, "the clock window lies in every build's row");
// "walks cut" lies inside the clock window, at a column where no stamp is written (today clock index 9; the stamps are 3-6)
static_assert(PEN_CLK_WALKS_CUT == 9 && PEN_CLK_ENTRIES == 10 && PEN_CLK_VERTS < PEN_CLK_WALKS_CUT && PEN_CLK_ENTRIES < PEN_CLOCK_COLS, "counts inside the clock window");
static_assert(PEN_WORK_PUBLIC <= PEN_WK_DEBUG0 && PEN_WORK_DEBUG == 8 && PEN_WKN_PAIRS < PEN_WORK_SLOTS && PEN_WKR_T_SHORT < PEN_WORK_SLOTS, "work slots");

// a stats row -> the four public figures of a mesh (sfx_pen_stats): pairs, dropped, entry overflow, walks cut.  One-sided pairs
// are in the list but contribute nothing: they count as dropped.
inline void pen_public_stats(const int* row, int32_t out[4]) {
    out[0] = row[PEN_ST_PAIRS] - row[PEN_ST_ONE_SIDED]; out[1] = row[PEN_ST_DROPPED] + row[PEN_ST_ONE_SIDED];
    out[2] = row[PEN_ST_OVERFLOW]; out[3] = row[PEN_ST_WALKS_CUT];
}
