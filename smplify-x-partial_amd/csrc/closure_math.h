// closure_math.h -- scalar and wavefront-level math of the closure kernels (closure_body.h) and of the stand-alone objective
// (objective_ext.hip): projection, Rodrigues forward / reverse, GMoF, the fixed-order sums.  No LDS layout, no model tables.
#pragma once
#include "sfx_internal.h"
#include "wave_ops.h"
// contraction only inside one source expression (decided by the front end): the stand-alone
// closure kernel and the fused fit kernels then round identically, so optimizer.step() driven from
// the host and sfx_batch_fit walk the same trajectory bit for bit
#pragma clang fp contract(on)

// Precision of the keypoint forward (rotations, rest joints, kinematic chain, keypoint skinning: fwd_t) and of the
// projection up to the pixel residual (proj_t); see "forward precision" in closure_body.  Measured on the 64 + 64
// reference fits of the benchmark configuration (LAB_NOTES.md §3.1; evaluations per frame / signed mean final-loss
// difference to the reference's fp32 run; the reference: 2 362 in fp32, 4 098 and -2.1 % in fp64):
//   fwd fp64, proj fp64 : 3 221 / -1.7 %   gradient noise 0.13 x torch fp32's: keeps working where the reference stalls
//   fwd fp64, proj fp32 : 2 482 / -0.4 %   <- built: never noisier than the reference, closest to it in loss and in work
//   fwd fp32, proj fp32 : 2 233 / +0.6 %   noise ~ torch's (pointer-jumping chain 1.3 x): stops a little early
#ifdef SFX_FWD_FP32
typedef float fwd_t;
#else
typedef double fwd_t;
#endif
#ifdef SFX_PROJ_FP64
typedef double proj_t;
#else
typedef float proj_t;
#endif

// camera.py:93-117: p_cam = R p + t, pixel = f p_cam.xy / p_cam.z + c; residual gt - pixel, all in T.
// O: the closure's working precision (float; double in the float64 mode)
template <class T, class O>
__device__ __forceinline__ void project_residual(const fwd_t* pj, const float* Rc, const O* ct, O fx, O fy, O cx,
                                                 O cy, float gtx, float gty, O& pcx, O& pcy, O& pcz, O& rx,
                                                 O& ry) {
    const T p[3] = {(T)pj[0], (T)pj[1], (T)pj[2]};
    const T pxd = (T)Rc[0] * p[0] + (T)Rc[1] * p[1] + (T)Rc[2] * p[2] + (T)ct[0];
    const T pyd = (T)Rc[3] * p[0] + (T)Rc[4] * p[1] + (T)Rc[5] * p[2] + (T)ct[1];
    const T pzd = (T)Rc[6] * p[0] + (T)Rc[7] * p[1] + (T)Rc[8] * p[2] + (T)ct[2];
    pcx = (O)pxd; pcy = (O)pyd; pcz = (O)pzd;
    rx = (O)((T)gtx - ((T)fx * (pxd / pzd) + (T)cx));
    ry = (O)((T)gty - ((T)fy * (pyd / pzd) + (T)cy));
}
__device__ __forceinline__ void sincos_t(double a, double* s, double* c) { sincos(a, s, c); }
__device__ __forceinline__ void sincos_t(float a, float* s, float* c) { *s = sinf(a); *c = cosf(a); }
// the closure's math at its working precision (float: the fp32 library calls of the fp32 closure, unchanged)
__device__ __forceinline__ float r_sqrt(float a) { return sqrtf(a); }
__device__ __forceinline__ double r_sqrt(double a) { return sqrt(a); }
__device__ __forceinline__ float r_sin(float a) { return sinf(a); }
__device__ __forceinline__ double r_sin(double a) { return sin(a); }
__device__ __forceinline__ float r_cos(float a) { return cosf(a); }
__device__ __forceinline__ double r_cos(double a) { return cos(a); }
__device__ __forceinline__ float r_exp(float a) { return expf(a); }
__device__ __forceinline__ double r_exp(double a) { return exp(a); }
// batch_rodrigues' 1e-8 (a Python float: rounded to the tensor's dtype)
template <class Real> __device__ __forceinline__ Real rodrigues_eps() { return (Real)1e-8; }
template <> __device__ __forceinline__ float rodrigues_eps<float>() { return 1e-8f; }

__device__ __forceinline__ float wave_sum(float v) { return wave_sum_dpp(v); }
__device__ __forceinline__ double wave_sum(double v) { return wave_sum_dpp(v); }
template <int CTRL>
__device__ __forceinline__ float lb_quad(float x) {       // DPP quad permutation of x (all lanes of the quad active)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double lb_quad(double x) {     // the same in fp64: both halves take the same permutation
    const long long u = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)u, CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// fixed-order block reduction: DPP sum per wavefront, then the CT/64 partials in order
// (2 barriers instead of a 9-barrier LDS tree); result in all threads
template <int CT, class Real>
__device__ __forceinline__ Real block_sum(Real v, Real* red) {
    const Real w = wave_sum_dpp(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    Real r = red[0];
#pragma unroll
    for (int i = 1; i < CT / 64; ++i) r += red[i];
    __syncthreads();
    return r;
}

// smplx.lbs.batch_rodrigues: angle = ||theta + 1e-8||, R = I + sin K + (1-cos) K K
__device__ __forceinline__ void rodrigues_fwd(const float* th, float* R) {
    const float ex = th[0] + 1e-8f, ey = th[1] + 1e-8f, ez = th[2] + 1e-8f;
    const float a = sqrtf(ex * ex + ey * ey + ez * ez);
    const float dx = th[0] / a, dy = th[1] / a, dz = th[2] / a;
    const float s = sinf(a), c = cosf(a);
    const float K[9] = {0.f, -dz, dy, dz, 0.f, -dx, -dy, dx, 0.f};
    const float omc = 1.f - c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float kk = K[i * 3 + 0] * K[0 * 3 + j] + K[i * 3 + 1] * K[1 * 3 + j] + K[i * 3 + 2] * K[2 * 3 + j];
            R[i * 3 + j] = ((i == j) ? 1.f : 0.f) + s * K[i * 3 + j] + omc * kk;
        }
}

// the same in fp64 (forward precision, see closure_body): R row-major
template <class Tin>
__device__ __forceinline__ void rodrigues_fwd_d(const Tin* th, fwd_t* R) {
    const fwd_t t0 = th[0], t1 = th[1], t2 = th[2];
    const fwd_t ex = t0 + (fwd_t)1e-8, ey = t1 + (fwd_t)1e-8, ez = t2 + (fwd_t)1e-8;
    const fwd_t a = sqrt(ex * ex + ey * ey + ez * ez);
    const fwd_t dx = t0 / a, dy = t1 / a, dz = t2 / a;
    fwd_t s, c;
    sincos_t(a, &s, &c);
    const fwd_t K[9] = {0, -dz, dy, dz, 0, -dx, -dy, dx, 0};
    const fwd_t omc = (fwd_t)1 - c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const fwd_t kk = K[i * 3 + 0] * K[0 * 3 + j] + K[i * 3 + 1] * K[1 * 3 + j] + K[i * 3 + 2] * K[2 * 3 + j];
            R[i * 3 + j] = ((i == j) ? (fwd_t)1 : (fwd_t)0) + s * K[i * 3 + j] + omc * kk;
        }
}

// reverse of rodrigues_fwd: dth += J^T dR
template <class Real>
__device__ __forceinline__ void rodrigues_bwd(const Real* th, const Real* dR, Real* dth) {
    const Real eps = rodrigues_eps<Real>();
    const Real ex = th[0] + eps, ey = th[1] + eps, ez = th[2] + eps;
    const Real a = r_sqrt(ex * ex + ey * ey + ez * ez);
    const Real inv = 1.f / a;
    const Real d[3] = {th[0] * inv, th[1] * inv, th[2] * inv};
    const Real s = r_sin(a), c = r_cos(a), omc = 1.f - c;
    const Real K[9] = {0.f, -d[2], d[1], d[2], 0.f, -d[0], -d[1], d[0], 0.f};
    Real KK[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            KK[i * 3 + j] = K[i * 3 + 0] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
    Real dRK = 0.f, dRKK = 0.f;
#pragma unroll
    for (int e = 0; e < 9; ++e) { dRK += dR[e] * K[e]; dRKK += dR[e] * KK[e]; }
    Real da = c * dRK + s * dRKK;
    // dK = s dR + (1-c) (dR K^T + K^T dR)
    Real dK[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Real t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t1 += dR[i * 3 + k] * K[j * 3 + k];     // dR K^T
                t2 += K[k * 3 + i] * dR[k * 3 + j];     // K^T dR
            }
            dK[i * 3 + j] = s * dR[i * 3 + j] + omc * (t1 + t2);
        }
    const Real dd[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    const Real ddth = dd[0] * th[0] + dd[1] * th[1] + dd[2] * th[2];
    da -= ddth * inv * inv;
    dth[0] += dd[0] * inv + da * ex * inv;
    dth[1] += dd[1] * inv + da * ey * inv;
    dth[2] += dd[2] * inv + da * ez * inv;
}

template <class Real>
__device__ __forceinline__ Real gmof_grad(Real r, Real rho2) {
    // d/dr [ rho^2 r^2 / (r^2 + rho^2) ] = 2 r rho^4 / (r^2 + rho^2)^2
    const Real den = r * r + rho2;
    return 2.f * r * (rho2 / den) * (rho2 / den);
}

#pragma clang fp contract(fast)
