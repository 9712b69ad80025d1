// chamfer_math.h -- the arithmetic and the serial bookkeeping of the chamfer term (csrc/chamfer.hip, sfx_chamfer_forward /
// sfx_chamfer_backward; the contract is in include/sfx.h), for the host and the device: no HIP runtime call, no global state.
// The kernels and tests/chamfer_math_check.cpp both include it.
//
//   squared distance    s = ((dx dx + dy dy) + dz dz) in float32 from the coordinate differences, in this association, without a
//                       fused multiply-add (the units that include this header are compiled with -ffp-contract=off)
//   robustifier         rho == 0: rho(s) = s, rho'(s) = 1;  rho > 0: the GMoF of smplifyx/utils.py:92-95 on the squared distance,
//                       rho(s) = r2 s / (s + r2), rho'(s) = r2^2 / (s + r2)^2, r2 = rho^2, all float64
//   per-point value     (float)(w rho(s)): float64 from the float32 s, rounded once
//   gradient factor     c = ((g w) rho'(s)) 2 in float64; a query q with target t adds c (q - t) to its own row and -c (q - t)
//                       to the row of t
//   inverted index      for every target the list of the queries whose nearest target it is, in ascending query index: integer
//                       counts, an exclusive scan, a fill.  ch_invert is the serial statement of it (a stable fill); the device
//                       fills a bucket in whatever order its integer atomics land and then places every entry at its rank
//                       (ch_rank: the entries of its bucket that are smaller), which gives the same lists
//   sum of a row        gather term G, then the row's list cut into segments of ch_seg_len(L) entries: each segment is summed
//                       from 0.0 in list order, the segment sums are added to G in segment order, the result is rounded to
//                       float32 once.  Lists of up to CH_SERIAL_MAX entries are one segment (one thread walks them), longer
//                       ones CH_SEGMENTS segments (the lanes of one wave, a segment each)
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CH_HD __host__ __device__ inline
#else
#define CH_HD inline
#endif

#define CH_SERIAL_MAX 32      // a list of up to this many entries is summed by one thread as one segment
#define CH_SEGMENTS 64        // a longer list: at most this many segments of equal length (the last may be shorter)

CH_HD float ch_dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// r2 = rho^2 in float64 (0: no robustifier)
CH_HD double ch_rho2(float rho) { return (double)rho * (double)rho; }

CH_HD double ch_rho(double s, double r2) { return r2 > 0.0 ? (r2 * s) / (s + r2) : s; }

CH_HD double ch_drho(double s, double r2) {
    if (!(r2 > 0.0)) return 1.0;
    const double d = s + r2;
    return (r2 * r2) / (d * d);
}

CH_HD float ch_point_value(float s, float w, double r2) { return (float)((double)w * ch_rho((double)s, r2)); }

CH_HD double ch_coef(float g, float w, float s, double r2) { return (((double)g * (double)w) * ch_drho((double)s, r2)) * 2.0; }

// a query takes part in the inverted index when its index names a target: -1 (masked, nothing found) and anything else outside
// 0 .. n_targets - 1 do not
CH_HD bool ch_index_ok(int idx, int n_targets) { return (unsigned)idx < (unsigned)n_targets; }

// entries of one bucket (any order) that are smaller than q: the place of q in the ascending list
CH_HD int ch_rank(const int* bucket, int len, int q) {
    int r = 0;
    for (int k = 0; k < len; ++k) r += bucket[k] < q;
    return r;
}

// entries per segment of a list of len entries (len >= 1)
CH_HD int ch_seg_len(int len) { return len <= CH_SERIAL_MAX ? len : (len + CH_SEGMENTS - 1) / CH_SEGMENTS; }

// The inverted index of idx[n_queries] over n_targets targets, serially: off[n_targets + 1] (exclusive scan of the counts) and
// list[off[n_targets]] with the queries of target t at off[t] .. off[t + 1] - 1 in ascending order.  Returns the entries.
inline int ch_invert(const int* idx, int n_queries, int n_targets, int* off, int* list) {
    for (int t = 0; t <= n_targets; ++t) off[t] = 0;
    for (int q = 0; q < n_queries; ++q)
        if (ch_index_ok(idx[q], n_targets)) ++off[idx[q] + 1];
    for (int t = 0; t < n_targets; ++t) off[t + 1] += off[t];
    const int total = off[n_targets];
    // stable fill without a second array: walking the queries backwards, off[t + 1] counts down from the end of bucket t to
    // its start, so a bucket's entries land in ascending order and off[t + 1] ends as the start of bucket t
    for (int q = n_queries - 1; q >= 0; --q)
        if (ch_index_ok(idx[q], n_targets)) list[--off[idx[q] + 1]] = q;
    for (int t = 0; t < n_targets; ++t) off[t] = off[t + 1];
    off[n_targets] = total;
    return total;
}
