// vposer_batch.hip -- the stand-alone VPoser-v1 decoder and its backward for whole batches of latents
// (sfx_vposer_*: `vposer.decode(pose_embedding, output_type='aa')` outside the fit loop, reference call sites fitting.py:72,197,
// 236, fit_single_frame.py:265,515,607,620,654, render_pkl.py:97, and what autograd walks behind it).
//
// The in-loop decoder (vposer.h) is one workgroup per frame and streams the 1.37 MB of weights once per frame.  Here a
// workgroup owns a TILE of 16 latents and streams the weights once per tile through the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32: A[l&15][k=l>>4], B[k=l>>4][l&15], C[row 4(l>>4)+e][col l&15]):
//   A operand = the tile's activations [16 frames][K], read from LDS (row stride = 2 mod 32 dwords: the 32 lanes of a
//               ds_read_b32 group -- 16 frames x 2 k -- fall on 32 different banks);
//   B operand = the weights [K][N], streamed from global memory; the workgroup's 8 wavefronts split the N output columns.
//               A wavefront with 64 columns loads ONE float4 per lane and k, W[k][n0 + 4m .. 4m+3], and element s of it feeds
//               accumulator s: MFMA column m of accumulator s is output column n0 + 4m + s (any assignment of columns to MFMA
//               column slots is valid as long as the epilogue knows it), so a wavefront reads 256 contiguous bytes per k row.
// Forward products stream the transposed copies ([in][out]: w1T, w2T, w3T), the backward's transposed products the original
// [out][in] layouts (w2 as it is; w3 with two zero rows appended, w1 with zero columns up to 64, so that no k step or column
// tile needs a bounds test).  Bias, leaky_relu(0.2) / its derivative and the write of the next product's A operand happen in
// the epilogues; the 6-D -> axis-angle step and its adjoint are vposer.h's vposer_joint, one thread per (frame, joint).
//
// An output element is ONE accumulator element of ONE wavefront, summed over k in ascending order from zero: a frame's result
// depends on its own latent only -- not on B, on the tile it falls in or on its row there.  No cross-row reduction, no atomics.
// Rows of a tail tile beyond B are fed zeros and store nothing.
//
// LDS per workgroup (both kernels): z [16][66] + h1 [16][514] + h2 [16][514] + o [16][130] floats = 78 336 B: two workgroups
// (16 wavefronts) per CU.  The backward keeps no second set: d o overwrites o (per thread, after it read its six values), and
// the two hidden gradients overwrite h2 and h1 element by element in the epilogues that read their leaky' masks from them.
#include "../../include/sfx.h"
#include "vposer.h"
#include "vposer_pack.h"
#include "vposer_gemm.h"      // vpb_gemm: the tile product, shared with vposer_encode.hip

#include <memory>

#define VPB_T 512            // 8 wavefronts
#define VPB_F 16             // frames per tile = MFMA rows
#define VPB_LDH (VP_H + 2)   // row strides (floats) of the LDS operands: = 2 mod 32
#define VPB_LDZ 66
#define VPB_LDO 130
#define VPB_LP 64            // latent columns of the padded w1 (latent <= 60)

struct VpbWeights {
    int latent;
    const float *w1T, *b1, *w2T, *b2, *w3T, *b3;      // [L][512], [512], [512][512], [512], [512][128], [128] (126, 127 zero)
    const float *w1p, *w2, *w3p;                      // [512][64] (columns >= L zero), [512][512], [128][512] (rows 126, 127 zero)
};

struct alignas(16) VpbLDS {
    float z[VPB_F * VPB_LDZ];
    float h1[VPB_F * VPB_LDH], h2[VPB_F * VPB_LDH];
    float o[VPB_F * VPB_LDO];
};
static_assert(2 * sizeof(VpbLDS) <= 160 * 1024, "two workgroups per CU");

// latents of the tile from f0 (rows beyond B: zeros) -> S.h1, S.h2 (after leaky_relu), S.o (columns 126, 127 zero)
__device__ __forceinline__ void vpb_forward_tile(VpbLDS& S, const VpbWeights& W, const float* __restrict__ z, const int B, const int f0) {
    const int L = W.latent;
    for (int i = threadIdx.x; i < VPB_F * L; i += VPB_T) {
        const int f = i / L, k = i - f * L;
        S.z[f * VPB_LDZ + k] = f0 + f < B ? z[(size_t)(f0 + f) * L + k] : 0.f;
    }
    __syncthreads();
    vpb_gemm<4, 0, VPB_LDZ, VP_H, VP_H>(S.z, W.w1T, L, [&](int f, int c, float v) { S.h1[f * VPB_LDH + c] = leaky(v + W.b1[c]); });
    __syncthreads();
    vpb_gemm<4, VP_H, VPB_LDH, VP_H, VP_H>(S.h1, W.w2T, 0, [&](int f, int c, float v) { S.h2[f * VPB_LDH + c] = leaky(v + W.b2[c]); });
    __syncthreads();
    vpb_gemm<1, VP_H, VPB_LDH, 128, 128>(S.h2, W.w3T, 0, [&](int f, int c, float v) { S.o[f * VPB_LDO + c] = v + W.b3[c]; });
    __syncthreads();
}

__global__ __launch_bounds__(VPB_T)
void k_vposer_decode16(VpbWeights W, int B, const float* __restrict__ z, float* __restrict__ body) {
    __shared__ VpbLDS S;
    const int f0 = blockIdx.x * VPB_F, t = threadIdx.x;
    vpb_forward_tile(S, W, z, B, f0);
    if (t < VPB_F * 21) {
        const int f = t / 21, j = t - 21 * f;
        if (f0 + f < B) {
            float aa[3];
            vposer_joint(&S.o[f * VPB_LDO + 6 * j], aa, nullptr, nullptr);
            float* out = body + (size_t)(f0 + f) * 63 + 3 * j;
            out[0] = aa[0]; out[1] = aa[1]; out[2] = aa[2];
        }
    }
}

// dz = d sum(dbody * body_pose) / d z, the forward re-evaluated at z (stateless)
__global__ __launch_bounds__(VPB_T)
void k_vposer_decode16_bwd(VpbWeights W, int B, const float* __restrict__ z, const float* __restrict__ dbody, float* __restrict__ dz) {
    __shared__ VpbLDS S;
    const int f0 = blockIdx.x * VPB_F, t = threadIdx.x, L = W.latent;
    vpb_forward_tile(S, W, z, B, f0);
    if (t < VPB_F * 21) {        // d o over o: a thread's six values, read before they are written (rows beyond B: zeros)
        const int f = t / 21, j = t - 21 * f;
        float* po = &S.o[f * VPB_LDO + 6 * j];
        float da[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (f0 + f < B) {
            const float* pd = dbody + (size_t)(f0 + f) * 63 + 3 * j;
            const float a[6] = {po[0], po[1], po[2], po[3], po[4], po[5]}, daa[3] = {pd[0], pd[1], pd[2]};
            float aa[3];
            vposer_joint(a, aa, daa, da);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) po[i] = da[i];
    }
    __syncthreads();
    // d h2 = W3^T d o, d h1 = W2^T d pre2, d z = W1^T d pre1; d pre = d h * leaky'(h), in place over h
    vpb_gemm<4, 128, VPB_LDO, VP_H, VP_H>(S.o, W.w3p, 0, [&](int f, int c, float v) {
        float& h = S.h2[f * VPB_LDH + c]; h = v * (h > 0.f ? 1.f : 0.2f); });
    __syncthreads();
    vpb_gemm<4, VP_H, VPB_LDH, VP_H, VP_H>(S.h2, W.w2, 0, [&](int f, int c, float v) {
        float& h = S.h1[f * VPB_LDH + c]; h = v * (h > 0.f ? 1.f : 0.2f); });
    __syncthreads();
    vpb_gemm<1, VP_H, VPB_LDH, VPB_LP, VPB_LP>(S.h1, W.w1p, 0, [&](int f, int c, float v) {
        if (f0 + f < B && c < L) dz[(size_t)(f0 + f) * L + c] = v; });
}

// ---------------------------------------------------------------------------------------
// The handle owns its weights through one DevAlloc and is released by its destructor only: sfx_vposer_destroy and every failing
// exit of sfx_vposer_create end there.
struct sfx_vposer {
    VpbWeights W{};
    DevAlloc mem;
};

extern "C" int sfx_vposer_create(int32_t latent, int32_t hidden, const float* w1, const float* b1, const float* w2, const float* b2,
                                 const float* w3, const float* b3, sfx_vposer** out) {
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !out) { sfx_set_error("null argument"); return -1; }
    if (!vposer_shape_ok(latent, hidden)) return -1;       // every refusal: before the first device allocation
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        sfx_set_error("no HIP device: libsfx has no CPU fallback"); return -3;
    }
    const int H = hidden, L = latent;
    VposerPack P;
    vposer_pack(L, H, w1, w2, w3, P);
    std::vector<float> w1p((size_t)H * VPB_LP, 0.f), w3p((size_t)128 * H, 0.f), b3p(128, 0.f);
    for (int o = 0; o < H; ++o) for (int i = 0; i < L; ++i) w1p[(size_t)o * VPB_LP + i] = w1[(size_t)o * L + i];
    std::copy(w3, w3 + (size_t)VP_O * H, w3p.begin());
    std::copy(b3, b3 + VP_O, b3p.begin());
    std::unique_ptr<sfx_vposer> v(new sfx_vposer());
    VpbWeights& W = v->W;
    DevAlloc& mem = v->mem;
    W.latent = L;
    W.w1T = mem.up(P.w1T); W.w2T = mem.up(P.w2T); W.w3T = mem.up(P.w3T);
    W.b1 = mem.up(b1, (size_t)H); W.b2 = mem.up(b2, (size_t)H); W.b3 = mem.up(b3p);
    W.w1p = mem.up(w1p); W.w2 = mem.up(w2, (size_t)H * H); W.w3p = mem.up(w3p);
    if (mem.failed) { (void)hipGetLastError(); sfx_set_error("out of device memory (VPoser weights)"); return -2; }
    *out = v.release();
    return 0;
}

extern "C" void sfx_vposer_destroy(sfx_vposer* v) { delete v; }

// Both calls only enqueue on the stream: no synchronisation, no device allocation, no scratch outside the workgroups' LDS.
extern "C" int sfx_vposer_decode(sfx_vposer* v, int32_t B, const float* z_dev, float* body_pose_dev, void* stream) {
    if (!v) { sfx_set_error("null vposer"); return -1; }
    if (B < 0) { sfx_set_error("sfx_vposer_decode: B=%d", B); return -1; }
    if (B == 0) return 0;
    if (!z_dev || !body_pose_dev) { sfx_set_error("sfx_vposer_decode: null argument"); return -1; }
    hipLaunchKernelGGL(k_vposer_decode16, dim3((B + VPB_F - 1) / VPB_F), dim3(VPB_T), 0, (hipStream_t)stream, v->W, B, z_dev, body_pose_dev);
    SFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sfx_vposer_decode_backward(sfx_vposer* v, int32_t B, const float* z_dev, const float* dbody_dev, float* dz_dev,
                                          void* stream) {
    if (!v) { sfx_set_error("null vposer"); return -1; }
    if (B < 0) { sfx_set_error("sfx_vposer_decode_backward: B=%d", B); return -1; }
    if (B == 0) return 0;
    if (!z_dev || !dbody_dev || !dz_dev) { sfx_set_error("sfx_vposer_decode_backward: null argument"); return -1; }
    hipLaunchKernelGGL(k_vposer_decode16_bwd, dim3((B + VPB_F - 1) / VPB_F), dim3(VPB_T), 0, (hipStream_t)stream, v->W, B, z_dev,
                       dbody_dev, dz_dev);
    SFX_CHECK(hipGetLastError());
    return 0;
}
