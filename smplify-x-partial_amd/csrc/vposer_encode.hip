// vposer_encode.hip -- the stand-alone VPoser-v1 encoder and its backward for whole batches of poses (sfx_vposer_encoder_*:
// `vposer.encode(full_pose_prior)` of fit_single_frame.py:245, the pose prior `vposer.encode(body_pose).mean.pow(2).sum()` of code
// that optimises the pose itself, and what autograd walks behind them).
//
// The mirror image of vposer_batch.hip: a workgroup owns a TILE of 16 poses and streams the weights once per tile through the
// fp32 matrix cores with the same tile product (vposer_gemm.h; operand and accumulator layout: the header of vposer_batch.hip).
// The two eval-mode batch norms are folded into the linear layers behind them on the host (vposer_pack.h), so the device runs
//   front end -> W1' (kin -> 512) -> leaky_relu(0.2) -> W2' (512 -> 512) -> leaky_relu(0.2) -> head (512 -> 128)
// with mu in head columns 0 .. L-1 and logvar in columns 64 .. 64+L-1; mean = mu, sigma = softplus(logvar).
// Front end, one thread per (frame, joint): a 63-wide first layer takes the pose as it is (kin = 64, column 63 zero); a 189-wide
// one takes the nine entries of each joint's rotation matrix, row-major, by plain Rodrigues with the first-order form I + K(aa)
// below 1e-6 rad -- vposer._aa_to_matrot, NOT the rodrigues_fwd of closure_body.h, whose epsilon rule is smplx's (kin = 192).
//
// The backward is stateless: it takes the poses again, re-evaluates the forward, overwrites the head output with its gradient
// (d mu = dmean, d logvar = dsigma * sigmoid(logvar)), runs the three transposed products -- the two hidden gradients overwrite h2
// and h1 element by element in the epilogues that read their leaky' masks from them -- and ends with the adjoint of the front end.
//
// An output element is ONE accumulator element of ONE wavefront, summed over k in ascending order from zero: a frame's result
// depends on its own pose only -- not on B, on the tile it falls in or on its row there.  No cross-row reduction, no atomics.
// Rows of a tail tile beyond B are fed zeros and store nothing.
//
// LDS per workgroup (all kernels): h1 [16][514] + h2 [16][514] + u [16][194] floats = 78 208 B: two workgroups (16 wavefronts)
// per CU.  u is the pose operand x [16][194] until the first product has read it, then the head output o [16][130] (never live
// together), and in the backward of the 189-wide form finally d x.  Row strides are = 2 mod 32 dwords.
// The 2 L softplus / sigmoid values of a frame are evaluated in double: sigma's float32 rounding is then the only error the
// activation adds, and the cost is nil next to the products.
#include "../../include/sfx.h"
#include "vposer.h"
#include "vposer_pack.h"
#include "vposer_gemm.h"

#include <memory>

#define VPE_T 512            // 8 wavefronts
#define VPE_F 16             // frames per tile = MFMA rows
#define VPE_LDH (VP_H + 2)   // row strides (floats) of the LDS operands: = 2 mod 32
#define VPE_LDX 194
#define VPE_LDO 130

struct VpeWeights {
    int latent;
    const float *w1T, *b1, *w2T, *b2, *whT, *bh;      // [kin][512], [512], [512][512], [512], [512][128], [128]
    const float *w1p, *w2, *wh;                       // [512][kin] (columns >= n_in zero), [512][512], [128][512]
};

struct alignas(16) VpeLDS {
    float h1[VPE_F * VPE_LDH], h2[VPE_F * VPE_LDH];
    float u[VPE_F * VPE_LDX];       // x [16][VPE_LDX] | o [16][VPE_LDO]
};
static_assert(VPE_LDX >= VPE_LDO && VPE_LDX % 32 == 2 && VPE_LDO % 32 == 2 && VPE_LDH % 32 == 2, "operand strides");
static_assert(sizeof(VpeLDS) == 78208 && 2 * sizeof(VpeLDS) <= 160 * 1024, "two workgroups per CU");

// R (row-major) of an axis-angle vector as vposer._aa_to_matrot forms it: I + sin K + (1 - cos) K K with K of the unit axis;
// I + K(aa) below 1e-6 rad.  1 - cos is formed as 2 sin^2(angle / 2): the same number without the cancellation.
// G != nullptr: also daa = d sum(G * R) / d aa.
__device__ __forceinline__ void vpe_rodrigues(const float aa[3], float R[9], const float* G, float daa[3]) {
    // the angle is formed in double, as _aa_to_matrot forms it: the 1e-6 test then takes the host encoder's branch for every float32 pose
    const double thd = sqrt((double)aa[0] * aa[0] + (double)aa[1] * aa[1] + (double)aa[2] * aa[2]);
    const float th = (float)thd;
    // v = vee(G - G^T): the gradient of sum(G * K(w)) with respect to w
    float v[3] = {0.f, 0.f, 0.f};
    if (G) { v[0] = G[7] - G[5]; v[1] = G[2] - G[6]; v[2] = G[3] - G[1]; }
    if (thd < 1e-6) {
        R[0] = 1.f;    R[1] = -aa[2]; R[2] = aa[1];
        R[3] = aa[2];  R[4] = 1.f;    R[5] = -aa[0];
        R[6] = -aa[1]; R[7] = aa[0];  R[8] = 1.f;
        if (G) { daa[0] = v[0]; daa[1] = v[1]; daa[2] = v[2]; }
        return;
    }
    const float inv = 1.f / th;
    const float u[3] = {aa[0] * inv, aa[1] * inv, aa[2] * inv};
    const float n2 = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    const float s = sinf(th), sh = sinf(0.5f * th), omc = 2.f * sh * sh;
    // K K = u u^T - (u . u) I
    R[0] = 1.f + omc * (u[0] * u[0] - n2); R[1] = -s * u[2] + omc * u[0] * u[1];  R[2] = s * u[1] + omc * u[0] * u[2];
    R[3] = s * u[2] + omc * u[1] * u[0];   R[4] = 1.f + omc * (u[1] * u[1] - n2); R[5] = -s * u[0] + omc * u[1] * u[2];
    R[6] = -s * u[1] + omc * u[2] * u[0];  R[7] = s * u[0] + omc * u[2] * u[1];   R[8] = 1.f + omc * (u[2] * u[2] - n2);
    if (G) {
        const float c = cosf(th), tr = G[0] + G[4] + G[8];
        // (G + G^T) u and u^T G u
        const float gu[3] = {2.f * G[0] * u[0] + (G[1] + G[3]) * u[1] + (G[2] + G[6]) * u[2],
                             (G[1] + G[3]) * u[0] + 2.f * G[4] * u[1] + (G[5] + G[7]) * u[2],
                             (G[2] + G[6]) * u[0] + (G[5] + G[7]) * u[1] + 2.f * G[8] * u[2]};
        const float ugu = 0.5f * (gu[0] * u[0] + gu[1] * u[1] + gu[2] * u[2]);
        const float g_s = v[0] * u[0] + v[1] * u[1] + v[2] * u[2], g_omc = ugu - n2 * tr;
        const float dth = c * g_s + s * g_omc;                     // d sin = cos, d (1 - cos) = sin
        float du[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) du[i] = s * v[i] + omc * (gu[i] - 2.f * tr * u[i]);
        const float duu = du[0] * u[0] + du[1] * u[1] + du[2] * u[2];
        // u = aa / th, th = |aa|:  d aa = (du - (du . u) u) / th + dth u
#pragma unroll
        for (int i = 0; i < 3; ++i) daa[i] = (du[i] - duu * u[i]) * inv + dth * u[i];
    }
}

__device__ __forceinline__ float vpe_softplus(const float x) {       // log1p(exp(-|x|)) + max(x, 0), in double
    const double d = (double)x;
    return (float)(log1p(exp(-fabs(d))) + fmax(d, 0.0));
}
__device__ __forceinline__ float vpe_sigmoid(const float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }

// poses of the tile from f0 (rows beyond B: zeros) -> S.h1, S.h2 (after leaky_relu), S.u = o (mu | logvar, the rest zero).
// KIN = 64: the pose itself; KIN = 192: rotation matrices.
template <int KIN>
__device__ __forceinline__ void vpe_forward_tile(VpeLDS& S, const VpeWeights& W, const float* __restrict__ pose, const int B, const int f0) {
    static_assert(KIN == 64 || KIN == 192, "63 or 189 inputs, padded");
    const int t = threadIdx.x;
    if constexpr (KIN == 64) {
        for (int i = t; i < VPE_F * 64; i += VPE_T) {
            const int f = i >> 6, k = i & 63;
            S.u[f * VPE_LDX + k] = (k < 63 && f0 + f < B) ? pose[(size_t)(f0 + f) * 63 + k] : 0.f;
        }
    } else {
        if (t < VPE_F * 21) {
            const int f = t / 21, j = t - 21 * f;
            float* px = &S.u[f * VPE_LDX + 9 * j];
            if (f0 + f < B) {
                const float* pp = pose + (size_t)(f0 + f) * 63 + 3 * j;
                const float aa[3] = {pp[0], pp[1], pp[2]};
                float R[9];
                vpe_rodrigues(aa, R, nullptr, nullptr);
#pragma unroll
                for (int i = 0; i < 9; ++i) px[i] = R[i];
            } else {
#pragma unroll
                for (int i = 0; i < 9; ++i) px[i] = 0.f;
            }
        } else if (t >= 448 && t < 448 + VPE_F * 3) {       // columns 189 .. 191
            const int i = t - 448, f = i / 3;
            S.u[f * VPE_LDX + 189 + (i - 3 * f)] = 0.f;
        }
    }
    __syncthreads();
    vpb_gemm<4, KIN, VPE_LDX, VP_H, VP_H>(S.u, W.w1T, 0, [&](int f, int c, float v) { S.h1[f * VPE_LDH + c] = leaky(v + W.b1[c]); });
    __syncthreads();
    vpb_gemm<4, VP_H, VPE_LDH, VP_H, VP_H>(S.h1, W.w2T, 0, [&](int f, int c, float v) { S.h2[f * VPE_LDH + c] = leaky(v + W.b2[c]); });
    __syncthreads();
    vpb_gemm<1, VP_H, VPE_LDH, VPE_HEAD, VPE_HEAD>(S.h2, W.whT, 0, [&](int f, int c, float v) { S.u[f * VPE_LDO + c] = v + W.bh[c]; });
    __syncthreads();
}

template <int KIN>
__global__ __launch_bounds__(VPE_T)
void k_vposer_encode16(VpeWeights W, int B, const float* __restrict__ pose, float* __restrict__ mean, float* __restrict__ sigma) {
    __shared__ VpeLDS S;
    const int f0 = blockIdx.x * VPE_F, L = W.latent;
    vpe_forward_tile<KIN>(S, W, pose, B, f0);
    for (int i = threadIdx.x; i < VPE_F * L; i += VPE_T) {
        const int f = i / L, c = i - f * L;
        if (f0 + f < B) {
            mean[(size_t)(f0 + f) * L + c] = S.u[f * VPE_LDO + c];
            if (sigma) sigma[(size_t)(f0 + f) * L + c] = vpe_softplus(S.u[f * VPE_LDO + VPE_LV + c]);
        }
    }
}

// dpose = d (sum(dmean * mean) + sum(dsigma * sigma)) / d pose, the forward re-evaluated at pose (stateless); dmean or dsigma
// may be nullptr (= zeros)
template <int KIN>
__global__ __launch_bounds__(VPE_T)
void k_vposer_encode16_bwd(VpeWeights W, int B, const float* __restrict__ pose, const float* __restrict__ dmean,
                           const float* __restrict__ dsigma, float* __restrict__ dpose) {
    __shared__ VpeLDS S;
    const int f0 = blockIdx.x * VPE_F, t = threadIdx.x, L = W.latent;
    vpe_forward_tile<KIN>(S, W, pose, B, f0);
    for (int i = t; i < VPE_F * VPE_HEAD; i += VPE_T) {       // d o over o, element by element (rows beyond B: zeros)
        const int f = i >> 7, c = i & 127;
        float* po = &S.u[f * VPE_LDO + c];
        float d = 0.f;
        if (f0 + f < B) {
            if (c < L) { if (dmean) d = dmean[(size_t)(f0 + f) * L + c]; }
            else if (c >= VPE_LV && c < VPE_LV + L) { if (dsigma) d = dsigma[(size_t)(f0 + f) * L + c - VPE_LV] * vpe_sigmoid(*po); }
        }
        *po = d;
    }
    __syncthreads();
    // d h2 = head^T d o, d h1 = W2'^T d pre2, d x = W1'^T d pre1; d pre = d h * leaky'(h), in place over h
    vpb_gemm<4, VPE_HEAD, VPE_LDO, VP_H, VP_H>(S.u, W.wh, 0, [&](int f, int c, float v) {
        float& h = S.h2[f * VPE_LDH + c]; h = v * (h > 0.f ? 1.f : 0.2f); });
    __syncthreads();
    vpb_gemm<4, VP_H, VPE_LDH, VP_H, VP_H>(S.h2, W.w2, 0, [&](int f, int c, float v) {
        float& h = S.h1[f * VPE_LDH + c]; h = v * (h > 0.f ? 1.f : 0.2f); });
    __syncthreads();
    if constexpr (KIN == 64) {
        vpb_gemm<1, VP_H, VPE_LDH, 64, 64>(S.h1, W.w1p, 0, [&](int f, int c, float v) {
            if (f0 + f < B && c < 63) dpose[(size_t)(f0 + f) * 63 + c] = v; });
    } else {
        vpb_gemm<4, VP_H, VPE_LDH, 192, 192>(S.h1, W.w1p, 0, [&](int f, int c, float v) { S.u[f * VPE_LDX + c] = v; });
        __syncthreads();
        if (t < VPE_F * 21) {
            const int f = t / 21, j = t - 21 * f;
            if (f0 + f < B) {
                const float* pp = pose + (size_t)(f0 + f) * 63 + 3 * j;
                const float* pg = &S.u[f * VPE_LDX + 9 * j];
                const float aa[3] = {pp[0], pp[1], pp[2]};
                float G[9], R[9], daa[3];
#pragma unroll
                for (int i = 0; i < 9; ++i) G[i] = pg[i];
                vpe_rodrigues(aa, R, G, daa);
                float* out = dpose + (size_t)(f0 + f) * 63 + 3 * j;
                out[0] = daa[0]; out[1] = daa[1]; out[2] = daa[2];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// The handle owns its weights through one DevAlloc and is released by its destructor only: sfx_vposer_encoder_destroy and every
// failing exit of sfx_vposer_encoder_create end there.
struct sfx_vposer_encoder {
    VpeWeights W{};
    int kin = 0;
    DevAlloc mem;
};

extern "C" int sfx_vposer_encoder_create(int32_t latent, int32_t hidden, int32_t n_in,
        const float* bn1_w, const float* bn1_b, const float* bn1_mean, const float* bn1_var, const float* fc1_w, const float* fc1_b,
        const float* bn2_w, const float* bn2_b, const float* bn2_mean, const float* bn2_var, const float* fc2_w, const float* fc2_b,
        const float* mu_w, const float* mu_b, const float* logvar_w, const float* logvar_b, sfx_vposer_encoder** out) {
    if (!out) { sfx_set_error("null argument"); return -1; }
    VposerEncPack P;                                       // every refusal: before the first device call
    if (!vposer_pack_encoder(latent, hidden, n_in, bn1_w, bn1_b, bn1_mean, bn1_var, fc1_w, fc1_b, bn2_w, bn2_b, bn2_mean, bn2_var,
                             fc2_w, fc2_b, mu_w, mu_b, logvar_w, logvar_b, P)) return -1;
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        sfx_set_error("no HIP device: libsfx has no CPU fallback"); return -3;
    }
    std::unique_ptr<sfx_vposer_encoder> e(new sfx_vposer_encoder());
    VpeWeights& W = e->W;
    DevAlloc& mem = e->mem;
    W.latent = latent; e->kin = P.kin;
    W.w1T = mem.up(P.w1T); W.w2T = mem.up(P.w2T); W.whT = mem.up(P.whT);
    W.b1 = mem.up(P.b1); W.b2 = mem.up(P.b2); W.bh = mem.up(P.bh);
    W.w1p = mem.up(P.w1p); W.w2 = mem.up(P.w2); W.wh = mem.up(P.wh);
    if (mem.failed) { (void)hipGetLastError(); sfx_set_error("out of device memory (VPoser encoder weights)"); return -2; }
    *out = e.release();
    return 0;
}

extern "C" void sfx_vposer_encoder_destroy(sfx_vposer_encoder* e) { delete e; }

// Both calls only enqueue on the stream: no synchronisation, no device allocation, no scratch outside the workgroups' LDS.
extern "C" int sfx_vposer_encode(sfx_vposer_encoder* e, int32_t B, const float* pose_dev, float* mean_dev, float* sigma_dev,
                                 void* stream) {
    if (!e) { sfx_set_error("null vposer encoder"); return -1; }
    if (B < 0) { sfx_set_error("sfx_vposer_encode: B=%d", B); return -1; }
    if (B == 0) return 0;
    if (!pose_dev || !mean_dev) { sfx_set_error("sfx_vposer_encode: null argument"); return -1; }
    const dim3 grid((B + VPE_F - 1) / VPE_F), block(VPE_T);
    if (e->kin == 64) hipLaunchKernelGGL(k_vposer_encode16<64>, grid, block, 0, (hipStream_t)stream, e->W, B, pose_dev, mean_dev, sigma_dev);
    else hipLaunchKernelGGL(k_vposer_encode16<192>, grid, block, 0, (hipStream_t)stream, e->W, B, pose_dev, mean_dev, sigma_dev);
    SFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sfx_vposer_encode_backward(sfx_vposer_encoder* e, int32_t B, const float* pose_dev, const float* dmean_dev,
                                          const float* dsigma_dev, float* dpose_dev, void* stream) {
    if (!e) { sfx_set_error("null vposer encoder"); return -1; }
    if (B < 0) { sfx_set_error("sfx_vposer_encode_backward: B=%d", B); return -1; }
    if (B == 0) return 0;
    if (!dmean_dev && !dsigma_dev) { sfx_set_error("sfx_vposer_encode_backward: dmean and dsigma both null"); return -1; }
    if (!pose_dev || !dpose_dev) { sfx_set_error("sfx_vposer_encode_backward: null argument"); return -1; }
    const dim3 grid((B + VPE_F - 1) / VPE_F), block(VPE_T);
    if (e->kin == 64) hipLaunchKernelGGL(k_vposer_encode16_bwd<64>, grid, block, 0, (hipStream_t)stream, e->W, B, pose_dev, dmean_dev,
                                         dsigma_dev, dpose_dev);
    else hipLaunchKernelGGL(k_vposer_encode16_bwd<192>, grid, block, 0, (hipStream_t)stream, e->W, B, pose_dev, dmean_dev, dsigma_dev,
                            dpose_dev);
    SFX_CHECK(hipGetLastError());
    return 0;
}
