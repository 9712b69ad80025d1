// lbs_backward.hip -- device side of sfx_lbs_backward: the backward pass of the stand-alone LBS (autograd through
// smplx.SMPLX.forward / smplx.lbs.lbs in the reference's ecosystem) for upstream gradients the CALLER supplies,
//     L = sum(dvertices * vertices) + sum(djoints * joints),   dL / d(the nine inputs of sfx_lbs_forward).
// Everything heavy already exists: the adjoint GEMM and its finish (lbs_adjoint.hip) take a gradient on every vertex back to feat
// and to the skinning transforms, the reverse sweep of closure_body.h takes d joints, d feat and d A back to the parameters.  This
// file adds the three pieces between them:
//   k_adj_prep     d v_posed = T(v)^T g(v) for every vertex of every column: the adjoint GEMM's operand (adj_G) for a gradient
//                  that comes from outside (inside a fit k_pen_gather writes it for the interpenetration term)
//   k_closure_ext  closure_body with an external upstream (ExtUpstream): forward of the keypoints, then the reverse sweep only
//   k_scatter_gc   the parameter block's gradient -> the nine outputs
#include "closure_body.h"

// ---- k_adj_prep ---------------------------------------------------------------------------------------------------------
// Traffic per column: g in (V x 12 B) and adj_G out (Vpad x 12 B), both once, both in 16-byte accesses; the sparse skinning rows
// of a vertex (64 B, PenAdjPrep's Wsp_j / Wsp_w) are read once per PREP_CG columns and kept in registers; the columns' rotation
// blocks (55 x 9 floats out of AT) sit in LDS.  A workgroup = 256 consecutive vertices x PREP_CG columns, thread = vertex.
// g is [B][V][3] with V x 12 B no multiple of 16: a column's row does not start on a 16-byte boundary, so the tile's span is
// staged through LDS from the enclosing ALIGNED run of float4 (coalesced, every byte once) and read back per vertex at stride
// 3 (conflict-free); results go the same way out, to rows of adj_G that are aligned (3 Vpad and the tile start are multiples
// of 4 floats).  Each (column, vertex) is computed on its own, in the order of pen_vertex_out (ascending weight slots, zero
// weights skipped): a column's result does not depend on which other columns are present.
#define PREP_T 256
#define PREP_CG 4
__global__ __launch_bounds__(PREP_T)
void k_adj_prep(PenAdjPrep ap, const float* __restrict__ g, const int V, const int B) {
    __shared__ __align__(16) float s_in[PREP_T * 3 + 8];
    __shared__ __align__(16) float s_out[PREP_T * 3];
    __shared__ __align__(16) float s_A[PREP_CG][SFX_J][12];      // rows of the 3 x 3 block: [r][c] at r * 4 + c
    const int t = threadIdx.x;
    const int v0 = blockIdx.x * PREP_T, b0 = blockIdx.y * PREP_CG;
    const int nb = min(PREP_CG, B - b0);
    const int nv = min(PREP_T, V - v0);                        // vertices of this tile (> 0 by the grid)
    const int nvp = min(PREP_T, ap.Vpad - v0);                 // ... and rows of adj_G it owns (padding rows: zeros)
    const size_t total = (size_t)B * V * 3;
    const bool aligned = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    for (int i = t; i < nb * SFX_J * 12; i += PREP_T) {
        const int cb = i / (SFX_J * 12), r = i % (SFX_J * 12), j = r / 12, e = r % 12;
        s_A[cb][j][e] = ap.AT[((size_t)e * SFX_JPAD + j) * ap.Bpad + b0 + cb];
    }
    const int v = v0 + t;
    const bool vok = t < nv;
    int wj[SFX_NW]; float ww[SFX_NW];
    {
        const int vc = vok ? v : V - 1;
        const int4* pj = reinterpret_cast<const int4*>(ap.Wsp_j + (size_t)vc * SFX_NW);
        const float4* pw = reinterpret_cast<const float4*>(ap.Wsp_w + (size_t)vc * SFX_NW);
        static_assert(SFX_NW == 8, "two 16-byte loads per table");
        const int4 j0 = pj[0], j1 = pj[1]; const float4 w0 = pw[0], w1 = pw[1];
        wj[0] = j0.x; wj[1] = j0.y; wj[2] = j0.z; wj[3] = j0.w; wj[4] = j1.x; wj[5] = j1.y; wj[6] = j1.z; wj[7] = j1.w;
        ww[0] = w0.x; ww[1] = w0.y; ww[2] = w0.z; ww[3] = w0.w; ww[4] = w1.x; ww[5] = w1.y; ww[6] = w1.z; ww[7] = w1.w;
    }
    for (int cb = 0; cb < nb; ++cb) {
        const int b = b0 + cb;
        const size_t f0 = ((size_t)b * V + v0) * 3;            // first float of the tile's span in g
        const size_t a0 = f0 & ~(size_t)3;
        const int sh = (int)(f0 - a0), n4 = (sh + 3 * nv + 3) >> 2;      // <= 193 float4
        __syncthreads();                                       // (first trip: s_A is complete; later: s_in has been read)
        if (t < n4) {
            const size_t i0 = a0 + 4 * (size_t)t;
            float4 x;
            if (aligned && i0 + 4 <= total) x = *reinterpret_cast<const float4*>(g + i0);
            else {                                             // the tensor's last, partial float4 (or a base that is not 16-byte aligned)
                x.x = i0 < total ? g[i0] : 0.f; x.y = i0 + 1 < total ? g[i0 + 1] : 0.f;
                x.z = i0 + 2 < total ? g[i0 + 2] : 0.f; x.w = i0 + 3 < total ? g[i0 + 3] : 0.f;
            }
            reinterpret_cast<float4*>(s_in)[t] = x;
        }
        __syncthreads();
        float o0 = 0.f, o1 = 0.f, o2 = 0.f;
        if (vok) {
            const float g0 = s_in[sh + 3 * t], g1 = s_in[sh + 3 * t + 1], g2 = s_in[sh + 3 * t + 2];
            if (g0 != 0.f || g1 != 0.f || g2 != 0.f) {         // d v_posed(v) = T(v)[:3,:3]^T g(v),  T(v) = sum_j W[v][j] A_j
                float T[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                auto add = [&](const int j, const float w) {
                    const float4* a = reinterpret_cast<const float4*>(s_A[cb][j]);
                    const float4 r0 = a[0], r1 = a[1], r2 = a[2];
                    T[0] += w * r0.x; T[1] += w * r0.y; T[2] += w * r0.z;
                    T[4] += w * r1.x; T[5] += w * r1.y; T[6] += w * r1.z;
                    T[8] += w * r2.x; T[9] += w * r2.y; T[10] += w * r2.z;
                };
                if (wj[0] >= 0) {
#pragma unroll
                    for (int q = 0; q < SFX_NW; ++q) if (ww[q] != 0.f) add(wj[q], ww[q]);
                } else {                                       // more than SFX_NW nonzero weights: the full row of lbs_weights
                    for (int j = 0; j < SFX_J; ++j) { const float w = ap.W[(size_t)v * SFX_J + j]; if (w != 0.f) add(j, w); }
                }
                o0 = T[0] * g0 + T[4] * g1 + T[8] * g2;
                o1 = T[1] * g0 + T[5] * g1 + T[9] * g2;
                o2 = T[2] * g0 + T[6] * g1 + T[10] * g2;
            }
        }
        s_out[3 * t] = o0; s_out[3 * t + 1] = o1; s_out[3 * t + 2] = o2;
        __syncthreads();
        if (4 * t < 3 * nvp)                                   // (3 nvp is a multiple of 4: Vpad and the tile start are multiples of 16)
            reinterpret_cast<float4*>(ap.adj_G + (size_t)b * 3 * ap.Vpad + (size_t)v0 * 3)[t] = reinterpret_cast<const float4*>(s_out)[t];
    }
}

void launch_adj_prep(const DevModel& M, const BatchDev& D, hipStream_t s) {
    if (D.nact <= 0) return;
    PenAdjPrep ap{D.AT, M.Wsp_j, M.Wsp_w, M.W, D.adj_G, D.Bpad, M.Vpad};
    hipLaunchKernelGGL(k_adj_prep, dim3((M.V + PREP_T - 1) / PREP_T, (D.nact + PREP_CG - 1) / PREP_CG), dim3(PREP_T), 0, s,
                       ap, (const float*)D.pen_dverts, M.V, D.nact);
}

// ---- reverse sweep with external upstream ----------------------------------------------------------------------------------
template <class LDS>
__global__ __launch_bounds__(LDS::kThreads)
void k_closure_ext(DevModel M, BatchDev D, const VarList* __restrict__ vls, const StageW* __restrict__ sws,
                   ClosureArgs args, ExtUpstream ext) {
    __shared__ LDS S;
    closure_body(S, M, D, vls, sws, args, blockIdx.x, nullptr, nullptr, ext);
}

void launch_closure_ext(const DevModel& M, const BatchDev& D, const VarList* vl_dev, const StageW* sw_dev, const ClosureArgs& a,
                        const float* djoints, int has_dverts, float* gc, hipStream_t s) {
    const ExtUpstream ext{djoints, has_dverts, gc};
    if (sfx_small_closure(M, D)) hipLaunchKernelGGL(k_closure_ext<FrameLDSSmall>, dim3(D.cfg.B), dim3(FrameLDSSmall::kThreads), 0, s, M, D, vl_dev, sw_dev, a, ext);
    else hipLaunchKernelGGL(k_closure_ext<FrameLDS>, dim3(D.cfg.B), dim3(FrameLDS::kThreads), 0, s, M, D, vl_dev, sw_dev, a, ext);
}

// ---- parameter block -> the nine gradients (NULL: not wanted) ----------------------------------------------------------------
__global__ void k_scatter_gc(ParLayout L, const float* __restrict__ gc, LbsGradOut o) {
    const int b = blockIdx.x, t = threadIdx.x;
    const float* x = gc + (size_t)b * SFX_NPAR_MAX;
    auto cp = [&](const int off, const int n, float* dst) { if (dst && t < n) dst[(size_t)b * n + t] = x[off + t]; };
    cp(L.go, 3, o.go); cp(L.emb, 63, o.bp); cp(L.betas, L.NB, o.betas); cp(L.expr, L.NE, o.expr);
    cp(L.jaw, 3, o.jaw); cp(L.leye, 3, o.leye); cp(L.reye, 3, o.reye); cp(L.lh, L.NPCA, o.lh); cp(L.rh, L.NPCA, o.rh);
}

void launch_scatter_gc(const BatchDev& D, const float* gc, const LbsGradOut& o, hipStream_t s) {
    hipLaunchKernelGGL(k_scatter_gc, dim3(D.cfg.B), dim3(64), 0, s, D.L, gc, o);
}
