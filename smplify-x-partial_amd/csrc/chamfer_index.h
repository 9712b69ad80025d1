// chamfer_index.h -- the device bodies that the nearest-point terms share (csrc/chamfer.hip and csrc/p2m.hip): the fixed-order
// float64 reduce of the per-point values and the four integer steps of the inverted index (count, exclusive scan, fill, rank
// placement).  Each unit wraps them in kernels of its own; the bodies see a "side" S through these members only:
//   S.Nd, S.Nq          rows of the destination set, entries (queries) that may choose one
//   S.my                uint8 [Nq] or NULL: 0 takes the entry out
//   S.idx_in            int [Nq]: the row an entry chose; anything outside 0 .. Nd - 1 names no row
//   S.cnt [Nd], S.off [Nd + 1], S.list [Nq], S.sorted [Nq]
// After the four steps S.sorted holds, for every row r at S.off[r] .. S.off[r + 1] - 1, its entries in ascending order, whatever
// order the integer atomics of the fill landed in.  No float atomics.
#pragma once
#include "wave_ops.h"
#include "chamfer_math.h"

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
