// lbfgs_two_loop.h -- the history of the on-device L-BFGS (lbfgs_body.h) and the blocked two-loop recursion over it, on ONE
// wavefront: a lane's three elements of a (<= 192)-vector (Lane3), the per-frame optimiser state (OptState), the push of a
// curvature pair (lb_push_pair) and the recursion itself (lb_two_loop).  Replaces lbfgs_ls.py:312-341.
//
// Compile with -ffp-contract=off: the only fused multiply-adds are the explicit fmaf() of the axpy updates (ATen's
// add_(alpha) vector path) and of the lane partials of the two-loop recursion's dot products
// (a 64-lane summation tree that no ATen kernel shares anyway).
#pragma once
#include "sfx_internal.h"
#include "wave_ops.h"
#include "lbfgs_scalar.h"
// every multiply-add in this file is written out: no implicit contraction (see header comment)
#pragma clang fp contract(off)
#define LB_BS 8      // history pairs per block of the blocked two-loop recursion (one group of 8 lanes per member)
// single-wavefront synchronisation: order LDS/global accesses of the 64 lanes
#define LB_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)

// Band of the Gram matrix S^T Y used by the blocked two-loop recursion, one 16-float row per history slot:
// row[8 + k], k = 1..7, holds  syb: s_p . y_(k-th successor of p)   (loop 2 walks old -> new)
//                              syt: s_(k-th predecessor of p) . y_p  (loop 1 walks new -> old);
// row[0..8] stay ZERO, so a lane that reads row[8 + (c - m)] for a member c <= m of the block gets the "+0" of the
// in-block coupling without a mask.
#define LB_BROW 16
struct OptState {
    OptScal s;
    float ro[SFX_HROWS_MAX];             // (rows R..R+7 of all three mirror slots 0..7, as the history does; R: the ring's slots)
    float syb[SFX_HROWS_MAX * LB_BROW];
    float syt[SFX_HROWS_MAX * LB_BROW];
};

#define NE3 3     // elements per lane (NVAR_MAX / 64)

struct Lane3 { float v[NE3]; };

__device__ __forceinline__ float wsum(float v) { return wave_sum_dpp(v); }
__device__ __forceinline__ float wmax(float v) { return wave_max_dpp(v); }
// lane l owns elements 3l, 3l+1, 3l+2 of a (<=192)-vector: one 12-byte load per lane, 768
// contiguous bytes per wavefront instruction.  Rows are allocated NVAR_MAX long, so the wide
// load is always in bounds; elements >= N are masked to zero.
__device__ __forceinline__ Lane3 ld3(const float* p, int lane, int N) {
    Lane3 r;
    const float3 v = *reinterpret_cast<const float3*>(p + 3 * lane);
    r.v[0] = (3 * lane + 0 < N) ? v.x : 0.f;
    r.v[1] = (3 * lane + 1 < N) ? v.y : 0.f;
    r.v[2] = (3 * lane + 2 < N) ? v.z : 0.f;
    return r;
}
// history rows are written full width (elements >= N are zero in every vector derived from masked
// loads), so they can be read back without masks
__device__ __forceinline__ Lane3 ld3_raw(const float* base, unsigned row_off, int lane) {
    Lane3 r;      // 32-bit element offset: uniform base pointer + per-lane offset (saddr addressing)
    const float3 v = *reinterpret_cast<const float3*>(reinterpret_cast<const char*>(base) + (row_off * 4u + 12u * (unsigned)lane));
    r.v[0] = v.x; r.v[1] = v.y; r.v[2] = v.z;
    return r;
}
__device__ __forceinline__ void st3_full(float* p, const Lane3& a, int lane) {
    *reinterpret_cast<float3*>(p + 3 * lane) = make_float3(a.v[0], a.v[1], a.v[2]);
}
__device__ __forceinline__ void st3(float* p, const Lane3& a, int lane, int N) {
#pragma unroll
    for (int e = 0; e < NE3; ++e) { const int i = 3 * lane + e; if (i < N) p[i] = a.v[e]; }
}
__device__ __forceinline__ float dot3(const Lane3& a, const Lane3& b) {
    float p = a.v[0] * b.v[0];
    p = p + a.v[1] * b.v[1];
    p = p + a.v[2] * b.v[2];
    return wsum(p);
}
__device__ __forceinline__ float absmax3(const Lane3& a, int lane, int N) {
    float m = 0.f;
#pragma unroll
    for (int e = 0; e < NE3; ++e) if (3 * lane + e < N) m = fmaxf(m, fabsf(a.v[e]));
    return wmax(m);
}
__device__ __forceinline__ Lane3 axpy3(const Lane3& x, float a, const Lane3& d) {
    Lane3 r;
#pragma unroll
    for (int e = 0; e < NE3; ++e) r.v[e] = fmaf(a, d.v[e], x.v[e]);
    return r;
}

// ---------------------------------------------------------------------------------------------
// Two-loop recursion (lbfgs_ls.py:322-341) on ONE wavefront, in blocks of 8 history pairs.  A single wavefront issues
// one instruction every 4 cycles whatever its kind, so the recursion is priced in instructions: per block
//   * 16 row loads (8 s rows, 8 y rows; lane l owns elements 3l..3l+2) from CONTIGUOUS history slots -- one uniform
//     base and immediate offsets; only the block that wraps around the ring or sticks out of the window computes
//     clamped slots row by row;
//   * the 8 dot products against the running vector, 3 FMAs each;
//   * ONE recursive-halving reduction of all 8 (wave_sum8_groups: 17 instructions) that leaves the sum of member c in
//     the 8 lanes of group c;
//   * the in-block coupling  s_c . (q - sum_{m<c} al_m y_m)  resolved lane-parallel on those groups with the stored
//     band of S^T Y (one 64-byte row per step, zeros where c <= m): multiply, v_readlane (the broadcast the axpy
//     needs anyway), FMA per step;
//   * the 8 axpys.
// Same arithmetic in exact terms as the sequential recursion (the order of the updates is the reference's; only the
// summation tree of each dot product differs).  Two blocks of look-ahead in registers cover the history's
// L2 / MALL latency.
template <int CTRL>
__device__ __forceinline__ float lb_dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
// in: v[c] = this lane's partial of sum c.  out: every lane of group g (lanes 8g..8g+7) holds the wave-wide sum g.
__device__ __forceinline__ float wave_sum8_groups(const float (&v)[8], const int lane) {
    // halves (stride 32): lanes 0-31 keep a, lanes 32-63 keep b
    auto halves = [](float a_, float b_) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a_), __float_as_uint(b_), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]); };
    // rows of 16 (stride 16): rows 0, 2 keep a, rows 1, 3 keep b
    auto rows = [](float a_, float b_) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a_), __float_as_uint(b_), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]); };
    // operand order chosen so that sum g ends in group g: rows of AB = sums 0, 2, 4, 6 and of CD = 1, 3, 5, 7
    const float A = halves(v[0], v[4]), B = halves(v[2], v[6]), C = halves(v[1], v[5]), D = halves(v[3], v[7]);
    const float AB = rows(A, B), CD = rows(C, D);
    // stride 8: lanes 0-7 of a row keep AB, lanes 8-15 keep CD
    const float tA = AB + lb_dpp<0x128>(AB), tC = CD + lb_dpp<0x128>(CD);          // row_ror:8
    float t = (lane & 8) ? tC : tA;
    t = t + lb_dpp<0x141>(t);          // row_half_mirror: l <-> 7 - l
    t = t + lb_dpp<0xB1>(t);           // quad_perm [1,0,3,2]
    t = t + lb_dpp<0x4E>(t);           // quad_perm [2,3,0,1]
    return t;
}

#define LB_ROWB (SFX_NVAR_MAX * 4)      // bytes per history row
// a lane's 3 elements of a history row as (pair, single): the 12-byte load lands in an even-aligned register triple, so
// the pair feeds v_pk_fma_f32 as it is (left to itself the compiler pairs elements 1, 2 and copies every row)
typedef float lb_v2 __attribute__((ext_vector_type(2)));
struct LbRow { lb_v2 a; float b; };
struct LbSet { LbRow mine[8]; LbRow all[8]; float bnd[7]; float ro, al; bool valid; };      // ro / al as loaded: the consumer masks them with `valid`
typedef float lb_v3 __attribute__((ext_vector_type(3)));
__device__ __forceinline__ LbRow lb_ldrow(const char* p) {
#ifdef SFX_HIST_NT
    // history rows are read once per direction and never shared: non-temporal, so that they do not push the tables every
    // frame of the XCD reads (blend-shape rows, VPoser weights) out of the 4-MB L2
    const lb_v3 u = __builtin_nontemporal_load(reinterpret_cast<const lb_v3*>(p));
#else
    const float3 u = *reinterpret_cast<const float3*>(p);
#endif
    LbRow r; r.a.x = u.x; r.a.y = u.y; r.b = u.z; return r;
}
__device__ __forceinline__ float lb_dotpart(const LbRow& x, const LbRow& y) { return fmaf(x.b, y.b, fmaf(x.a.y, y.a.y, x.a.x * y.a.x)); }
__device__ __forceinline__ void lb_axpy(LbRow& y, const float a, const LbRow& x) {
    const lb_v2 aa = {a, a};
    y.a = __builtin_elementwise_fma(aa, x.a, y.a); y.b = fmaf(a, x.b, y.b);
}

// rows of the block whose member 0 is logical index `base`, members base + DIR * c: always 8 CONSECUTIVE rows (the ring
// is followed by a mirror of its first 8 slots).  Members outside the window [0, n) get ro = al = 0: their rows are
// other slots of the ring (stale pairs or the zeros of the allocation -- finite), their steps are exact no-ops.
// mine / all: the two history arrays in the order the loop uses them; tab: the band table of this direction.  The rows
// the block touches first (mine) are requested last: one s_waitcnt at the dot products covers the whole set.
template <int DIR>
__device__ __forceinline__ void lb_load(LbSet& X, const int base, const int n, const int head, const float* hMine,
                                        const float* hAll, const float* tab, const float* ro, const float* s_alp,
                                        const bool want_al, const int lane, const int R) {
    const int grp = lane >> 3;
    int p = head + base; p = p >= R ? p - R : p;
    if (DIR < 0 && p < 7) p += R;
    const float* tb = tab + p * LB_BROW + 8 + grp;
#pragma unroll
    for (int m = 0; m < 7; ++m) X.bnd[m] = tb[DIR * m * LB_BROW - m];
    const int ig = base + DIR * grp;
    const bool valid = ig >= 0 && ig < n;
    // ro / al are handed over as loaded and masked where they are used (lb_two_loop): a select right behind its load is a
    // wait for that load, and in front of the 16 row requests it cost the prologue of loop 2 two serial memory round trips
    X.valid = valid;
    X.ro = ro[p + DIR * grp];
    X.al = 0.f;
    if (want_al) X.al = s_alp[ig];
    const char* ra = reinterpret_cast<const char*>(hAll) + (size_t)p * LB_ROWB + 12 * lane;
    const char* rm = reinterpret_cast<const char*>(hMine) + (size_t)p * LB_ROWB + 12 * lane;
#pragma unroll
    for (int c = 0; c < 8; ++c) X.all[c] = lb_ldrow(ra + DIR * c * LB_ROWB);
#pragma unroll
    for (int c = 0; c < 8; ++c) X.mine[c] = lb_ldrow(rm + DIR * c * LB_ROWB);
}

// A new curvature pair (lbfgs_ls.py:312-320: the oldest one leaves when the window is full) with what the blocked
// recursion keeps per pair: ro, the band entries s_(k-th predecessor) . y_new -- the syt row of the new pair and entry k
// of the k-th predecessor's syb row -- and the mirror of slots 0..7 behind the ring.
__device__ __forceinline__ void lb_push_pair(float* hY, float* hS, OptState* gst, int& hist_n, int& hist_head, const Lane3& y,
                                             const Lane3& sv, const float ys, const int lane, const int hist_cap = SFX_HIST,
                                             const int R = SFX_HIST) {
    if (hist_n >= hist_cap) { hist_head = hist_head + 1 >= R ? 0 : hist_head + 1; hist_n -= 1; }      // (history_size <= R, the ring's slots: 100 unless history_size asks for more)
    int ph = hist_head + hist_n; ph = ph >= R ? ph - R : ph;
    st3_full(hY + (size_t)ph * SFX_NVAR_MAX, y, lane);
    st3_full(hS + (size_t)ph * SFX_NVAR_MAX, sv, lane);
    const float ro = 1.0f / ys;
    if (lane == 0) gst->ro[ph] = ro;
    if (ph < 8) {
        st3_full(hY + (size_t)(ph + R) * SFX_NVAR_MAX, y, lane);
        st3_full(hS + (size_t)(ph + R) * SFX_NVAR_MAX, sv, lane);
        if (lane == 0) gst->ro[ph + R] = ro;
    }
    hist_n += 1;
    const int n1 = __builtin_amdgcn_readfirstlane(hist_n), hd1 = __builtin_amdgcn_readfirstlane(hist_head);
    Lane3 SP[7];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const int i_ = n1 - 1 - k;
        int t_ = hd1 + (i_ >= 0 ? i_ : 0); t_ = t_ >= R ? t_ - R : t_;
        SP[k - 1] = ld3_raw(hS, (unsigned)t_ * SFX_NVAR_MAX, lane);
    }
    float eb[8];
    eb[0] = 0.f;
#pragma unroll
    for (int k = 1; k < 8; ++k) eb[k] = fmaf(SP[k - 1].v[2], y.v[2], fmaf(SP[k - 1].v[1], y.v[1], SP[k - 1].v[0] * y.v[0]));
    const float e = wave_sum8_groups(eb, lane);      // group k: s_(k-th predecessor) . y_new
    const int k = lane >> 3, i_ = n1 - 1 - k;
    int t_ = hd1 + (i_ >= 0 ? i_ : 0); t_ = t_ >= R ? t_ - R : t_;
    const float ev = (k >= 1 && i_ >= 0) ? e : 0.f;   // (no such predecessor: a finite 0)
    if ((lane & 7) == 0) {
        gst->syt[ph * LB_BROW + 8 + k] = ev;
        gst->syb[ph * LB_BROW + 8 + k] = 0.f;         // successors of the new pair do not exist yet
        if (ph < 8) { gst->syt[(ph + R) * LB_BROW + 8 + k] = ev; gst->syb[(ph + R) * LB_BROW + 8 + k] = 0.f; }
        if (k >= 1 && i_ >= 0) {
            gst->syb[t_ * LB_BROW + 8 + k] = ev;
            if (t_ < 8) gst->syb[(t_ + R) * LB_BROW + 8 + k] = ev;
        }
    }
}

template <int SETS>
__device__ __forceinline__ Lane3 lb_two_loop(const float* hS, const float* hY, const OptState* gst, float* s_al,
                                             const int n_, const int head_, const float hd, const Lane3 q_in, const int lane,
                                             const int R = SFX_HIST) {
    const int n = __builtin_amdgcn_readfirstlane(n_), head = __builtin_amdgcn_readfirstlane(head_);
    float* s_alp = s_al + 8;        // members below index 0 of the last block land in the padding
    const int grp = lane >> 3;
    const int nb = max(1, (n + 7) >> 3);        // block steps per loop (the old loops ran one step for an empty window too)
#define LB_RL(v, l) __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (l)))
    // SETS register sets of history rows: the block in use + (SETS - 1) blocks of look-ahead (3 where the registers are
    // there -- the tick kernels; 2 inside the persistent per-frame kernel, which would spill)
    static_assert(SETS == 2 || SETS == 3, "register sets");
    LbSet A, B, C;
    LbRow q; q.a.x = q_in.v[0]; q.a.y = q_in.v[1]; q.b = q_in.v[2];
    // ---- loop 1: newest -> oldest;  al_i = ro_i s_i . q;  q -= al_i y_i
    auto down = [&](const LbSet& X, const int base) {
        float part[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) part[c] = lb_dotpart(X.mine[c], q);
        float acc = wave_sum8_groups(part, lane);
        const float ro = X.valid ? X.ro : 0.f;
        float al[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            al[m] = LB_RL(acc * ro, 8 * m);
            if (m < 7) acc = fmaf(-al[m], X.bnd[m], acc);
        }
        s_alp[base - grp] = acc * ro;          // (members c <= m see zeros of the band: acc[c] is final after step c)
#pragma unroll
        for (int c = 0; c < 8; ++c) lb_axpy(q, -al[c], X.all[c]);
    };
#define LB_LD1(X, b_) lb_load<-1>(X, (b_), n, head, hS, hY, gst->syt, gst->ro, s_alp, false, lane, R)
    // The look-ahead loads are UNCONDITIONAL (a block past the end of the window re-reads block 0; it is never used): with
    // `if (i0 >= 16) load` the number of loads in flight at the next dot products depended on a branch, and the compiler then
    // waits for the shorter path's count -- vmcnt(0): every block paid its own memory round trip and the look-ahead bought
    // nothing (round 4, read off the ISA; the same holds for stores left pending by the pair push: gfx9 counts them in vmcnt).
    // (and the loads must stay where they are written: left alone, the compiler sinks the look-ahead loads of two steps into the
    //  third one, next to their use -- LB_PIN, an empty asm that memory operations do not cross)
#define LB_PIN() asm volatile("" ::: "memory")
    __builtin_amdgcn_s_waitcnt(0x0F70);      // (kept: without it the tick launch is 0.2 us slower, A/B in one session)
    {
        int i0 = n - 1, k = 0;
        // ONE exit per loop: with `if (i0 < 0) break` after every step the unified loop exit gave the header an edge from each
        // step, and the wait counts at the header and in the third step were those of the shortest such path -- vmcnt(8) and
        // vmcnt(23) where 48 loads may stay in flight: two steps out of three waited for the look-ahead of the step before
        // (round 4, read off the ISA).  Whole rounds of SETS steps in the loop, the 1 .. SETS - 1 left over behind it.
        if constexpr (SETS == 3) {
        LB_LD1(A, i0); LB_LD1(B, max(i0 - 8, 0));
        for (; k + 3 <= nb; k += 3) {
            LB_LD1(C, max(i0 - 16, 0)); LB_PIN(); down(A, i0); LB_PIN(); i0 -= 8;
            LB_LD1(A, max(i0 - 16, 0)); LB_PIN(); down(B, i0); LB_PIN(); i0 -= 8;
            LB_LD1(B, max(i0 - 16, 0)); LB_PIN(); down(C, i0); LB_PIN(); i0 -= 8;
        }
        if (k < nb) { down(A, i0); LB_PIN(); i0 -= 8; if (k + 1 < nb) { down(B, i0); LB_PIN(); } }
        } else {
        LB_LD1(A, i0);
        for (; k + 2 <= nb; k += 2) {
            LB_LD1(B, max(i0 - 8, 0)); LB_PIN(); down(A, i0); LB_PIN(); i0 -= 8;
            LB_LD1(A, max(i0 - 8, 0)); LB_PIN(); down(B, i0); LB_PIN(); i0 -= 8;
        }
        if (k < nb) { down(A, i0); LB_PIN(); }
        }
    }
#undef LB_LD1
    LB_SYNC();      // alphas (LDS) are read back below
    LbRow r; r.a = q.a * hd; r.b = q.b * hd;
    // ---- loop 2: oldest -> newest;  be_i = ro_i y_i . r;  r += (al_i - be_i) s_i
    auto up = [&](const LbSet& X) {
        float part[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) part[c] = lb_dotpart(X.mine[c], r);
        float acc = wave_sum8_groups(part, lane);
        const float ro = X.valid ? X.ro : 0.f, alv = X.valid ? X.al : 0.f;
        float cc[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            cc[m] = LB_RL(alv - acc * ro, 8 * m);
            if (m < 7) acc = fmaf(cc[m], X.bnd[m], acc);
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) lb_axpy(r, cc[c], X.all[c]);
    };
#define LB_LD2(X, b_) lb_load<1>(X, (b_), n, head, hY, hS, gst->syb, gst->ro, s_alp, true, lane, R)
    {
        int i0 = 0, k = 0;
        const int last = max(n - 1, 0);
        if constexpr (SETS == 3) {
        LB_LD2(A, i0); LB_LD2(B, min(i0 + 8, last));
        for (; k + 3 <= nb; k += 3) {
            LB_LD2(C, min(i0 + 16, last)); LB_PIN(); up(A); LB_PIN(); i0 += 8;
            LB_LD2(A, min(i0 + 16, last)); LB_PIN(); up(B); LB_PIN(); i0 += 8;
            LB_LD2(B, min(i0 + 16, last)); LB_PIN(); up(C); LB_PIN(); i0 += 8;
        }
        if (k < nb) { up(A); LB_PIN(); if (k + 1 < nb) { up(B); LB_PIN(); } }
        } else {
        LB_LD2(A, i0);
        for (; k + 2 <= nb; k += 2) {
            LB_LD2(B, min(i0 + 8, last)); LB_PIN(); up(A); LB_PIN(); i0 += 8;
            LB_LD2(A, min(i0 + 8, last)); LB_PIN(); up(B); LB_PIN(); i0 += 8;
        }
        if (k < nb) { up(A); LB_PIN(); }
        }
    }
#undef LB_LD2
#undef LB_PIN
#undef LB_RL
    Lane3 out; out.v[0] = r.a.x; out.v[1] = r.a.y; out.v[2] = r.b;
    return out;
}

#pragma clang fp contract(fast)
