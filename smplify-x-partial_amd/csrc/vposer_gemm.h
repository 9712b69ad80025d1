// vposer_gemm.h -- the tile product of the stand-alone VPoser kernels (vposer_batch.hip: decoder, vposer_encode.hip: encoder):
// 16 frames x K from LDS times a weight matrix streamed from global memory through v_mfma_f32_16x16x4_f32.  The layout of the
// operands and of the accumulators is described at the top of vposer_batch.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// C[16][N] = A[16][K] (LDS, row stride LDA) x W[K][N] (global, row stride LDW; K a multiple of 4), by all wavefronts of the
// workgroup: wavefront w owns the 16 * NC columns from 16 * NC * w (NC = 4: float4 weight loads, see the header; NC = 1: one
// 16-column MFMA tile).  epi(frame, column, value) is called once per output element by the lane that holds it.
// KC > 0: K = KC, a multiple of 64 -- the operands of the NEXT eight k steps are requested before this chunk's MFMAs are issued
// (eight 16-byte weight loads in flight per lane: a wavefront waits for memory once per 8 KiB, not once per row).  KC = 0: K =
// `kdyn` at run time (the latent: at most 15 steps), a plain loop.  Either way an output element is one chain over ascending k.
template <int NC, int KC, int LDA, int LDW, int N, class Epi>
__device__ __forceinline__ void vpb_gemm(const float* A, const float* __restrict__ W, const int kdyn, Epi epi) {
    static_assert(NC == 1 || NC == 4, "columns per lane");
    static_assert(KC % 64 == 0, "whole pairs of chunks of eight k steps");
    typedef typename std::conditional<NC == 4, float4, float>::type wvec;
    constexpr int U = 8;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int n0 = wv * 16 * NC;
    if (n0 < N) {                // (wavefront-uniform)
        f32x4 acc[NC];
#pragma unroll
        for (int s = 0; s < NC; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* pa = A + m * LDA + q;
        const wvec* pw = reinterpret_cast<const wvec*>(W + (size_t)q * LDW + n0 + NC * m);
        auto step = [&](const float a, const wvec& w) {
            if constexpr (NC == 4) {
                acc[0] = MFMA(a, w.x, acc[0]); acc[1] = MFMA(a, w.y, acc[1]);
                acc[2] = MFMA(a, w.z, acc[2]); acc[3] = MFMA(a, w.w, acc[3]);
            } else {
                acc[0] = MFMA(a, w, acc[0]);
            }
        };
        if constexpr (KC > 0) {
            wvec w_a[U], w_b[U];       // two register sets used in turn: no copies between them, so each wait counts only its own set's loads
            float a_a[U], a_b[U];
            auto load = [&](wvec (&w)[U], float (&a)[U], const int k0) {
#pragma unroll
                for (int u = 0; u < U; ++u) { w[u] = pw[(size_t)(k0 + 4 * u) * (LDW / NC)]; a[u] = pa[k0 + 4 * u]; }
            };
            load(w_a, a_a, 0);
#pragma unroll 1
            for (int k0 = 0; k0 < KC; k0 += 8 * U) {
                load(w_b, a_b, k0 + 4 * U);
                __builtin_amdgcn_sched_barrier(0);      // (the scheduler otherwise sinks the requests below the MFMAs that hide them)
#pragma unroll
                for (int u = 0; u < U; ++u) step(a_a[u], w_a[u]);
                load(w_a, a_a, k0 + 8 * U < KC ? k0 + 8 * U : 0);      // (unconditional -- the last trip asks for chunk 0 again, unused: a branch here makes every wait of the second set a full one)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < U; ++u) step(a_b[u], w_b[u]);
            }
        } else {
            for (int k = 0; k < kdyn; k += 4) step(pa[k], pw[(size_t)k * (LDW / NC)]);
        }
        // accumulator s, register e of lane (m, q) = C[4 q + e][n0 + NC m + s]
#pragma unroll
        for (int s = 0; s < NC; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) epi(4 * q + e, n0 + NC * m + s, acc[s][e]);
    }
}
