// chamfer_index.h -- what the nearest-point terms share (csrc/chamfer.hip and csrc/p2m.hip).  Device bodies: the fixed-order
// float64 reduce of the per-point values, the four integer steps of the inverted index (count, exclusive scan, fill, rank
// placement) and the walk of a row's list that sums its entries' terms (ch_rows_body).  Host: what every entry refuses beside
// its sizes (ch_refuse) and the chunks of meshes a grid holds (ch_mesh_chunks).
// Each unit wraps the bodies in kernels of its own; the index bodies see a "side" S through these members only:
//   S.Nd, S.Nq          rows of the destination set, entries (queries) that may choose one
//   S.my                uint8 [Nq] or NULL: 0 takes the entry out
//   S.idx_in            int [Nq]: the row an entry chose; anything outside 0 .. Nd - 1 names no row
//   S.cnt [Nd], S.off [Nd + 1], S.list [Nq], S.sorted [Nq]
// After the four steps S.sorted holds, for every row r at S.off[r] .. S.off[r + 1] - 1, its entries in ascending order, whatever
// order the integer atomics of the fill landed in.  No float atomics.
#pragma once
#include "sfx_internal.h"
#include "wave_ops.h"
#include "chamfer_math.h"

#include <algorithm>
#include <cmath>

#define CH_RED_THREADS 1024
#define CH_RED_WAVES (CH_RED_THREADS / 64)
#define CH_ROW_THREADS 256
#define CH_GRID_Y 65535

// one workgroup of CH_RED_THREADS: the float64 sum of val[Nq] in a fixed order (a thread's points in index order, the lanes by
// wave_sum_dpp, the waves in wave order), rounded to float32 once; the number of valid (unmasked) queries beside it
__device__ __forceinline__ void ch_reduce_body(const float* val, const unsigned char* mq, int Nq, float* loss, int* valid) {
    __shared__ double red[CH_RED_WAVES];
    __shared__ int redn[CH_RED_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double acc = 0.0; int n = 0;
    for (int i = tid; i < Nq; i += CH_RED_THREADS) {
        acc += (double)val[i];
        n += (!mq || mq[i]) ? 1 : 0;
    }
    const double s = wave_sum_dpp(acc);
    const int c = wave_incl_scan_dpp(n);
    if (lane == 0) red[w] = s;
    if (lane == 63) redn[w] = c;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0; int m = 0;
        for (int k = 0; k < CH_RED_WAVES; ++k) { t += red[k]; m += redn[k]; }
        *loss = (float)t;
        if (valid) *valid = m;
    }
}

// the bucket of entry q, or -1: masked, without a target, or an index that names no row
template <class Side>
__device__ __forceinline__ int ch_bucket(const Side& S, int q) {
    if (S.my && !S.my[q]) return -1;
    const int t = S.idx_in[q];
    return ch_index_ok(t, S.Nd) ? t : -1;
}

// counts[row] += 1 for every entry with a row (integer atomics: the result has no order); one thread per entry
template <class Side>
__device__ __forceinline__ void ch_count_body(const Side& S, int q) {
    if (q >= S.Nq) return;
    const int t = ch_bucket(S, q);
    if (t >= 0) atomicAdd(&S.cnt[t], 1);
}

// one workgroup of CH_RED_THREADS: exclusive scan of the counts; zeroes them for the fill
template <class Side>
__device__ __forceinline__ void ch_scan_body(const Side& S) {
    __shared__ int wave_total[CH_RED_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int carry = 0;
    for (int base = 0; base < S.Nd; base += CH_RED_THREADS) {
        const int i = base + tid;
        const int c = i < S.Nd ? S.cnt[i] : 0;
        const int incl = wave_incl_scan_dpp(c);
        if (lane == 63) wave_total[w] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < CH_RED_WAVES; ++k) { const int t = wave_total[k]; before += k < w ? t : 0; total += t; }
        if (i < S.Nd) { S.off[i] = carry + before + incl - c; S.cnt[i] = 0; }       // (the counts become the fill's cursors)
        carry += total;
        __syncthreads();
    }
    if (tid == 0) S.off[S.Nd] = carry;
}

// every entry takes the next free place of its bucket (integer atomic cursor: any order)
template <class Side>
__device__ __forceinline__ void ch_fill_body(const Side& S, int q) {
    if (q >= S.Nq) return;
    const int t = ch_bucket(S, q);
    if (t >= 0) S.list[S.off[t] + atomicAdd(&S.cnt[t], 1)] = q;
}

// every entry moves to its rank inside its bucket (ch_rank): the buckets are now ascending, whatever the fill's order was
template <class Side>
__device__ __forceinline__ void ch_order_body(const Side& S, int q) {
    if (q >= S.Nq) return;
    const int t = ch_bucket(S, q);
    if (t < 0) return;
    const int o = S.off[t], len = S.off[t + 1] - o;
    S.sorted[o + ch_rank(S.list + o, len, q)] = q;
}

// One thread per row r of a destination set (live: r names a row; every lane of the row's wave calls): row += the terms of the
// entries sorted[off[r] .. off[r + 1] - 1].  term(x, q, acc) adds what entry q adds to the row into acc; x holds three floats
// of the row's own (chamfer: its point) that a long list's lanes receive by readlane instead of loading them again.  The
// order of the sum is the contract -- the same bits in every run and in any batch: up to CH_SERIAL_MAX entries are one
// segment, summed by the row's thread in list order and added to the row.  A longer list is cut into segments of ch_seg_len
// entries, at most 64; the lanes of the row's wave sum a segment each in list order, and the segment sums are added to the row
// in segment order.  A wave takes its long lists one after the other, lowest lane first.  Every sum is float64.
// (The sums are kept in scalars, not in row[]: with the array the compiler's schedule of both callers came out slower.)
template <class Term>
__device__ __forceinline__ void ch_rows_body(const int* off, const int* sorted, int r, bool live, const float (&x)[3], double (&row)[3],
                                             Term term) {
    const int lane = threadIdx.x & 63;
    double r0 = row[0], r1 = row[1], r2 = row[2];
    int o = 0, len = 0;
    if (live) {
        o = off[r]; len = off[r + 1] - o;
        if (len > 0 && len <= CH_SERIAL_MAX) {                            // one segment, walked by this thread
            double p[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < len; ++k) term(x, sorted[o + k], p);
            r0 += p[0]; r1 += p[1]; r2 += p[2];
        }
    }
    unsigned long long todo = __ballot(live && len > CH_SERIAL_MAX);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int lo = __builtin_amdgcn_readlane(o, src), ll = __builtin_amdgcn_readlane(len, src);
        const float t[3] = {__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[0]), src)),
                            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[1]), src)),
                            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[2]), src))};
        const int seg = ch_seg_len(ll), n_seg = (ll + seg - 1) / seg;     // (n_seg <= 64: a lane each)
        double p[3] = {0.0, 0.0, 0.0};
        const int k0 = min(ll, lane * seg), k1 = min(ll, k0 + seg);
        for (int k = k0; k < k1; ++k) term(t, sorted[lo + k], p);
        for (int l = 0; l < n_seg; ++l) {                                 // (l is wave-uniform)
            const double v0 = readlane_f64(p[0], l), v1 = readlane_f64(p[1], l), v2 = readlane_f64(p[2], l);
            if (lane == src) { r0 += v0; r1 += v1; r2 += v2; }
        }
    }
    row[0] = r0; row[1] = r1; row[2] = r2;
}

// ------------------------------------------------------------------------------------------------------------ host side
// what every entry refuses beside its sizes (those the unit checks itself, after B); 0 = fine.  n1, n2: the two sizes the
// scratch message names.
static inline int ch_refuse(const char* entry, int32_t B, float rho, const void* scratch, int64_t scratch_bytes, size_t need,
                            const char* n1, int32_t v1, const char* n2, int32_t v2) {
    if (B < 0) { sfx_set_error("%s: B = %d", entry, B); return -1; }
    if (!std::isfinite(rho) || rho < 0.f) { sfx_set_error("%s: rho = %g, a finite value >= 0 is needed", entry, (double)rho); return -1; }
    if (!scratch || scratch_bytes < 0 || (size_t)scratch_bytes < need) {
        sfx_set_error("%s: scratch of %lld bytes, %zu are needed for B = %d, %s = %d, %s = %d", entry,
                      scratch ? (long long)scratch_bytes : 0LL, need, B, n1, v1, n2, v2); return -1; }
    return 0;
}

// launch(nb) once per chunk of nb meshes from A.b0 on (gridDim.y holds 65 535 meshes); stops at the first that fails
template <class Args, class Launch>
static inline int ch_mesh_chunks(Args& A, int B, Launch launch) {
    for (int b0 = 0; b0 < B; b0 += CH_GRID_Y) {
        A.b0 = b0;
        if (const int rc = launch(std::min(B - b0, CH_GRID_Y))) return rc;
    }
    return 0;
}
