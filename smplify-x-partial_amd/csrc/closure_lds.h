// closure_lds.h -- the per-frame LDS working set of the closure workgroup (FrameLDSBase and its variants) and the helpers that
// fill it: asynchronous global -> LDS copies and the self-served blend offsets of the dense path.
#pragma once
#include "closure_math.h"
// (contraction as in closure_math.h; vposer.h -- VposerLDS is a member of the working set -- is compiled under it too)
#pragma clang fp contract(on)
#include "vposer.h"

// an integer parked in a slot of the reduction scratch
__device__ __forceinline__ void red_put_int(float& r, int n) { r = __int_as_float(n); }
__device__ __forceinline__ void red_put_int(double& r, int n) { r = (double)n; }
__device__ __forceinline__ int red_get_int(float r) { return __float_as_int(r); }
__device__ __forceinline__ int red_get_int(double r) { return (int)r; }

// threads per closure workgroup: a property of the LDS variant (FrameLDSx::kThreads) -- 256 for the body-only working set
// (two or three workgroups share a CU), 512 for the full one (142 KB: the workgroup owns its CU, and what it does there is
// stream VPoser weights and adjoint rows through that CU's L2 port: 8 wavefronts keep 108 GB/s in flight, 4 keep 93)
#ifndef SFX_BIG_THREADS
#define SFX_BIG_THREADS 512
#endif
#define SFX_MAX_THREADS 512

struct EmptyLDS {};

// Asynchronous global -> LDS copies by the whole workgroup (LDS-DMA, `global_load_lds_dword[x4]`): no registers, and no wait
// until the next __syncthreads (which carries the vmcnt(0)).  Every table a closure workgroup needs at entry -- model
// tables, this frame's record, the forward state of the previous launch -- is requested back to back this way: ONE memory
// round trip instead of one per copy loop (the entry of k_tick_dense was 7.7 us body-only / 11 us with hands + face).
// The destination of one wave-instruction is a contiguous run of 64 dwords (or 64 x 16 bytes) starting at a wave-uniform
// LDS address; sources are per-lane.  tid: the caller's thread index where it is not to be threadIdx.x itself (OperandSets.t).
typedef __attribute__((address_space(3))) void* sfx_lds_vp;
typedef const __attribute__((address_space(1))) void* sfx_glb_vp;
template <int CT>
__device__ __forceinline__ void lds_fill_async(void* lds_dst, const void* gsrc, const int n_dwords, const int tid = threadIdx.x) {
    const int lane = tid & 63, wv = tid >> 6;
    const char* g = reinterpret_cast<const char*>(gsrc);
    char* l = reinterpret_cast<char*>(lds_dst);
    for (int base = wv * 64; base < n_dwords; base += CT) {
        const int i = base + lane;
        if (i < n_dwords) __builtin_amdgcn_global_load_lds((sfx_glb_vp)(g + 4 * (size_t)i), (sfx_lds_vp)(l + 4 * base), 4, 0, 0);
    }
}
// LDS-DMA completes in vmcnt order: the barrier that publishes DMA-filled LDS to the other wavefronts must be preceded by a
// wait for this wavefront's own copies.  The compiler emits that s_waitcnt in front of every such s_barrier today; the memory
// model does not oblige it to (a workgroup-scope release needs lgkmcnt only), so it is spelled out (CK: block_sync_lds_direct_load).
__device__ __forceinline__ void lds_dma_wait() { __builtin_amdgcn_s_waitcnt(0x0F70); }      // vmcnt(0); expcnt / lgkmcnt untouched
// the same in 16-byte units (both sides 16-byte aligned)
template <int CT>
__device__ __forceinline__ void lds_fill_async16(void* lds_dst, const void* gsrc, const int n16, const int tid = threadIdx.x) {
    const int lane = tid & 63, wv = tid >> 6;
    const char* g = reinterpret_cast<const char*>(gsrc);
    char* l = reinterpret_cast<char*>(lds_dst);
    for (int base = wv * 64; base < n16; base += CT) {
        const int i = base + lane;
        if (i < n16) __builtin_amdgcn_global_load_lds((sfx_glb_vp)(g + 16 * (size_t)i), (sfx_lds_vp)(l + 16 * base), 16, 0, 0);
    }
}

// Self-served blend offsets: what the dense GEMM (lbs_dense.hip) exports as BatchDev.uvp -- sum_k featR[column][k] dirs[k][vertex,
// coordinate] for the n_uniq exported vertices -- formed by the frame's own workgroup from its operand row `arow`, bit for bit:
// the GEMM's instruction (v_mfma_f32_16x16x4_f32), accumulator from zero, its K order (SFX_DENSE_KCHUNK, rows ascending inside
// a chunk, k = 4 ks + kq in lane group kq), no template added.  The rows of an MFMA tile are independent, so all 16 A rows carry
// this frame's operand and row 0 (lanes 0-15, register 0) is read; the B columns are the exported vertices, whose rows of dirsT
// the model keeps a second time in the order this chain consumes them (DevModel.uniq_dirs: one 16-byte load per lane and four
// steps; gathered from dirsT itself -- 4-byte loads at stride 16 over 16 rows -- the phase cost 9.4 us per launch, LAB_NOTES 4.9).
// One accumulator chain per (tile of 16 vertices, coordinate), dealt to the `nw` wavefronts that call (wavefront wv of them): 128
// dependent MFMAs, B operands fetched four chunks (32 steps) ahead.  out[u * 3 + c], LDS or global; any n_uniq (0: nothing).
typedef float sfx_f32x4 __attribute__((ext_vector_type(4)));
[[maybe_unused]] static __device__ __forceinline__ void self_blend_offsets(const float* __restrict__ uniq_dirs, const int n_uniq, const float* __restrict__ arow,
                                                                           float* out, const int wv, const int nw, const int lane) {
    constexpr int NCH = SFX_KD_PAD / SFX_DENSE_KC, KS = SFX_DENSE_KC / 4;      // 16 chunks of 8 MFMA steps
    constexpr int NG = 4, GS = NG * KS;                                         // chunks / steps per operand group
    static_assert(NCH % NG == 0 && KS % 4 == 0 && NCH * KS == 128, "operand groups; DevModel.uniq_dirs holds 128 steps per unit");
    const int jl = lane & 15, kq = lane >> 4;
    const int nunit = ((n_uniq + 15) / 16) * 3;
    for (int unit = wv; unit < nunit; unit += nw) {
        const int tile = unit / 3, co = unit - tile * 3;
        const int u = tile * 16 + jl;
        const float4* pb = reinterpret_cast<const float4*>(uniq_dirs) + (size_t)unit * (NCH * KS / 4) * 64 + lane;
        const float* pa = arow + kq;
        float a[NCH * KS];
        float4 bv[2][GS / 4];
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) a[c * KS + ks] = pa[SFX_DENSE_KCHUNK(c) * SFX_DENSE_KC + ks * 4];
#define SELF_LOAD(g, buf) _Pragma("unroll") for (int q = 0; q < GS / 4; ++q) bv[buf][q] = pb[((g) * (GS / 4) + q) * 64];
        sfx_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        SELF_LOAD(0, 0)
#pragma unroll
        for (int g = 0; g < NCH / NG; ++g) {
            if (g + 1 < NCH / NG) { SELF_LOAD(g + 1, (g + 1) & 1) }
            __builtin_amdgcn_sched_barrier(0);      // (keep the next group's loads in front of this group's chain: left alone, the scheduler sinks them to 8 steps ahead)
#pragma unroll
            for (int q = 0; q < GS / 4; ++q) {
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g * GS + 4 * q + 0], bv[g & 1][q].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g * GS + 4 * q + 1], bv[g & 1][q].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g * GS + 4 * q + 2], bv[g & 1][q].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g * GS + 4 * q + 3], bv[g & 1][q].w, acc, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#undef SELF_LOAD
        if (kq == 0 && u < n_uniq) out[u * 3 + co] = acc[0];
    }
}

// Per-frame working set of the closure workgroup.  MAXI = item capacity, VP = VPoser activations
// present.  Two variants are instantiated: <240, true> (any model / configuration, 86 KB) and
// <32, false> (body-only keypoints without VPoser, 47 KB -> three workgroups per CU, or one next
// to two 48-KB GEMM workgroups).
// TH (round 4): threads of the workgroup when not the variant's default -- the body-only set on 512 threads where a workgroup owns
// its CU (k_tick_dense at <= 256 frames): two wavefronts per SIMD cover each other's LDS round trips in the barrier-separated
// passes.  The same bits as on 256 threads: every sum across wavefronts either has its terms in the first four wavefronts on
// both (threads >= 256 hold no keypoint, parameter or item of this variant: they add zeros) or is dealt to kRowWaves = 4
// wavefronts whatever the thread count (the adjoint's row streams), and the layout -- the forward-state blob two launches
// hand each other -- does not depend on TH.
// Real (the float64 mode, sfx_batch_cfg.high_precision = 2: double): the closure's working precision -- parameters,
// rotations, blend-shape sums, item vertices and transforms, losses and the whole reverse sweep.  The copies of model
// tables (vt, iw, ww, sjw, djw) stay fp32: the model is fp32 and widening it is exact.
template <int MAXI, bool VP, int TH, class Real>
struct __align__(16) FrameLDSBase {
    using real_t = Real;
    static constexpr int kMaxItems = MAXI;
    static constexpr int kBlocksPerCU = (MAXI <= SFX_SMALL_ITEMS && !VP) ? SFX_SMALL_OCC : 1;    // register budget of the fused kernels
    static constexpr int kThreads = TH ? TH : ((MAXI <= SFX_SMALL_ITEMS && !VP) ? 256 : SFX_BIG_THREADS);
    static constexpr int kRowWaves = (MAXI <= SFX_SMALL_ITEMS && !VP) ? 4 : kThreads / 64;        // wavefronts that stream adjoint rows
    // scratch T: the item transforms, and (reverse sweep) one 512-float partial per row-streaming wavefront
    static constexpr int kScratch = (MAXI * 12 > kRowWaves * 512) ? MAXI * 12 : kRowWaves * 512;
    Real  feat[SFX_KD_PAD];        // first: read as float4
    Real  x[SFX_NPAR_MAX];
    Real  full_pose[168];
    Real  R[SFX_J * 9];
    Real  Jr[SFX_J * 3];
    Real  G[SFX_J * 12];
    Real  A[SFX_J * 12];
    // the part of the forward whose ROUNDING NOISE decides when the line search stalls is carried in fp64 (see
    // "forward precision" below): skinning transforms and posed kinematic joints; saved with the prefix above
    fwd_t Ad[SFX_J * 12];
    fwd_t Gt[SFX_J * 3 + 3];      // (+3: keeps the saved prefix a multiple of 16 bytes in either precision)
    Real  vp[MAXI * 3];            // v_posed of the items (template + blend offsets), for the reverse sweep
    Real  vpo[MAXI * 3];           // the blend offsets alone (small numbers: fp32 sums of them carry ~1e-10 m)
    float vt[MAXI * 3];            // v_template rows of the items
    alignas(16) Real T[kScratch]; // item transforms [MAXI][12]; reused as scratch (>= 2048 floats) by the reverse sweep and, between
                                   // evaluations, as the working set of the optimiser tick (float4 accesses)
    fwd_t cd[2 * SFX_J * 12];     // kinematic chain in fp64: the two buffers of the pointer-jumping rounds
    fwd_t Jd[SFX_J * 3];          // rest joints, fp64
    fwd_t jd[SFX_MAX_K * 3];      // mapped joints, fp64 (what the projection reads)
    Real  dvert[MAXI * 3];
    Real  dvp[MAXI * 3];
    int   rl[MAXI * 3];            // compacted list of the blend-shape rows the adjoint streams (row = vertex * 3 + coordinate) ...
    Real  rc[MAXI * 3];            // ... and their coefficients (d v_posed), nonzero entries only
    int   ivid[MAXI];
    int   uslot[MAXI];             // static items: index of the item's vertex in the dense GEMM's export (BatchDev.uvp)
    float iw[MAXI];
    int   wj[MAXI * SFX_NW];       // sparse skinning weights of the items
    float ww[MAXI * SFX_NW];
    int   sjs[SFX_J + 1];          // per-joint lists of the static items (adjoint of the skinning: dA), copied from the
    int   sji[MAXI * SFX_NW];      //   model's CSR when it fits (M.n_sj <= MAXI * SFX_NW): two dependent global round trips
    float sjw[MAXI * SFX_NW];      //   per evaluation otherwise
    static constexpr int kMaxDyn = (MAXI > SFX_SMALL_ITEMS) ? SFX_MAX_DYN : 1;
    int   djs[SFX_J + 1];          // the same for the dynamic-contour items of this frame's LUT row (DevModel.dynp_*)
    int   dji[kMaxDyn * SFX_NW];
    float djw[kMaxDyn * SFX_NW];
    Real  joints[SFX_MAX_K * 3];
    Real  dj[SFX_MAX_K * 3];
    Real  dA[SFX_J * 12];
    Real  dG[SFX_J * 12];
    Real  drel[SFX_J * 3];
    Real  dJ[SFX_J * 3];
    Real  dR[SFX_J * 9];
    Real  dfeat[SFX_KD_PAD];
    Real  dpose[168];
    Real  gc[SFX_NPAR_MAX];
    Real  red[SFX_MAX_THREADS];
    Real  lh45[SFX_NHAND], rh45[SFX_NHAND];    // } contiguous: saved / reloaded as one run of 2 * SFX_NHAND + 1 dwords
    int   lut_row;                             // }
    typename std::conditional<VP, VposerLDS, EmptyLDS>::type V;   // VPoser activations (use_vposer only)
    alignas(16) float fd[FD_N]; // this frame's keypoints / weights / camera / regression pose (image of BatchDev.fd)
    alignas(16) int meta[SFX_META_N];     // tree / joint-map tables (one coalesced load instead of
                                // dependent global loads inside every level of the chain)
};
template <int MAXI, bool VP, int TH = 0>
struct FrameLDSx : FrameLDSBase<MAXI, VP, TH, float> {};
using FrameLDS = FrameLDSx<SFX_MAX_ITEMS, true>;
using FrameLDSSmall = FrameLDSx<SFX_SMALL_ITEMS, false>;
using FrameLDSSmall8 = FrameLDSx<SFX_SMALL_ITEMS, false, 512>;      // the same set on eight wavefronts (k_tick_dense, a workgroup per CU)
// the body-only set in double (float64 mode, needed-rows path): one workgroup per CU
struct FrameLDSSmall64 : FrameLDSBase<SFX_SMALL_ITEMS, false, 0, double> {};
static_assert(sizeof(FrameLDSSmall64) + 4096 <= 160 * 1024, "float64 closure working set: LDS of one workgroup");

#pragma clang fp contract(fast)
