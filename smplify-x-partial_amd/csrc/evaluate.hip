// evaluate.hip -- scoring of fitted meshes on the device: sfx_eval_align and sfx_eval_nearest (include/sfx.h).
//
// Replaces, for B pairs of point sets that already sit in device memory:
//   ProcrustesAlignment.__call__        smplifyx/utils.py:540-595
//   mpjpe / vertex_to_vertex_error      smplifyx/utils.py:597-614
//   PelvisAlignment                     smplifyx/utils.py:650-668
//   ScaleAlignment                      smplifyx/utils.py:729-772
//   point_fscore (its two nearest-neighbour queries and the threshold counts)      smplifyx/utils.py:622-648
//
// k_eval_align: one workgroup of EV_ALIGN_THREADS per mesh, three passes over the two point sets (250 KB at V = 10 475: they
//   stay in L2 between the passes).
//     pass 1   number of valid points, centroids of both sets
//     pass 2   (Procrustes, scale) centred sums: K = X1 X2^T, var1 = sum |X1|^2, var2 = sum |X2|^2
//     solve    thread 0: R from K (procrustes3.h), scale, t; through LDS to every thread
//     pass 3   e_i = | s R p_i + t - (q_i - o) |, stored as float; their sum for the mean
//   Every sum is float64 and has a fixed order: a thread adds its points i = tid, tid + T, .. in order, the 64 lanes of a wave are
//   added by wave_sum_dpp, the waves' totals in wave order.  No atomics: a mesh's bits depend on its own points only.
// k_eval_nearest: brute force.  A workgroup keeps EV_NN_QPT x 256 query points in registers (EV_NN_QPT per thread) and walks the
//   other set in tiles of EV_NN_TILE points staged in LDS as float4; every lane reads the same LDS address (a broadcast, one
//   ds_read_b128 per target and EV_NN_QPT distance updates).  The squared distance is formed from the coordinate differences.
//   A masked target is staged as +inf and can never be the minimum.  Counts below the thresholds and the valid counts are
//   integers: one atomicAdd per wave and threshold (the result does not depend on the order).
#include "../../include/sfx.h"
#include "sfx_internal.h"
#include "wave_ops.h"
#include "procrustes3.h"

#define EV_ALIGN_THREADS 1024
#define EV_ALIGN_WAVES (EV_ALIGN_THREADS / 64)
#define EV_MAX_POINTS (1 << 26)      // points per set: every index and every i + stride stays inside int32
#define EV_NN_THREADS 256
#define EV_NN_QPT 2
#define EV_NN_TILE 1024
#define EV_GRID_Y 65535

struct AlignArgs {
    int mode, N, n_anchors;
    int anchors[SFX_ALIGN_MAX_ANCHORS];
    const float* est; const float* gt; const unsigned char* mask;
    float* err; float* mean; float* xform;
};

// sums of NV values over the workgroup, in a fixed order, returned in every thread
template <int NV>
__device__ __forceinline__ void ev_block_sum(double (&v)[NV], double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = wave_sum_dpp(v[i]);
        if (lane == 0) red[w * NV + i] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double s = 0.0;
        for (int k = 0; k < EV_ALIGN_WAVES; ++k) s += red[k * NV + i];
        v[i] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(EV_ALIGN_THREADS)
void k_eval_align(const AlignArgs A) {
    __shared__ double red[EV_ALIGN_WAVES * 11];
    __shared__ double xf[16];                    // scale, R (9), t (3), o (3): the offset taken from the ground truth
    const int N = A.N, tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * N;
    const float* est = A.est + base * 3;
    const float* gt = A.gt + base * 3;
    const unsigned char* mask = A.mask ? A.mask + base : nullptr;

    // ---- pass 1: valid count and centroids
    double s1[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < N; i += EV_ALIGN_THREADS) {
        if (mask && !mask[i]) continue;
        s1[0] += (double)est[i * 3]; s1[1] += (double)est[i * 3 + 1]; s1[2] += (double)est[i * 3 + 2];
        s1[3] += (double)gt[i * 3]; s1[4] += (double)gt[i * 3 + 1]; s1[5] += (double)gt[i * 3 + 2];
        s1[6] += 1.0;
    }
    ev_block_sum<7>(s1, red);
    const double n = s1[6];
    const double mu1[3] = {s1[0] / n, s1[1] / n, s1[2] / n}, mu2[3] = {s1[3] / n, s1[4] / n, s1[5] / n};

    // ---- pass 2: centred sums (utils.py:560-572, :756-761)
    double s2[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool centred = A.mode == SFX_ALIGN_PROCRUSTES || A.mode == SFX_ALIGN_SCALE;
    if (centred) {
        for (int i = tid; i < N; i += EV_ALIGN_THREADS) {
            if (mask && !mask[i]) continue;
            const double x[3] = {(double)est[i * 3] - mu1[0], (double)est[i * 3 + 1] - mu1[1], (double)est[i * 3 + 2] - mu1[2]};
            const double y[3] = {(double)gt[i * 3] - mu2[0], (double)gt[i * 3 + 1] - mu2[1], (double)gt[i * 3 + 2] - mu2[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) s2[r * 3 + c] += x[r] * y[c];
            s2[9] += x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
            s2[10] += y[0] * y[0] + y[1] * y[1] + y[2] * y[2];
        }
        ev_block_sum<11>(s2, red);
    }

    // ---- the transform: s R p + t for the estimate, q - o for the ground truth
    if (tid == 0) {
        double scale = 1.0, R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0};
        if (A.mode == SFX_ALIGN_PROCRUSTES) {
            procrustes3_rotation(s2, R, nullptr);
            double tr = 0.0;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) tr += R[r * 3 + c] * s2[c * 3 + r];
            scale = tr / s2[9];                                                       // utils.py:584
            for (int r = 0; r < 3; ++r)
                t[r] = mu2[r] - scale * (R[r * 3] * mu1[0] + R[r * 3 + 1] * mu1[1] + R[r * 3 + 2] * mu1[2]);
        } else if (A.mode == SFX_ALIGN_SCALE) {
            scale = sqrt(s2[10] / s2[9]);                                             // utils.py:763
            for (int r = 0; r < 3; ++r) t[r] = mu2[r] - scale * mu1[r];
        } else if (A.mode == SFX_ALIGN_PELVIS) {
            for (int k = 0; k < A.n_anchors; ++k) {
                const int a = A.anchors[k];                                           // (checked on the host: 0 <= a < N)
                for (int r = 0; r < 3; ++r) { t[r] -= (double)est[a * 3 + r]; o[r] += (double)gt[a * 3 + r]; }
            }
            for (int r = 0; r < 3; ++r) { t[r] /= (double)A.n_anchors; o[r] /= (double)A.n_anchors; }
        }
        xf[0] = scale;
        for (int i = 0; i < 9; ++i) xf[1 + i] = R[i];
        for (int i = 0; i < 3; ++i) { xf[10 + i] = t[i]; xf[13 + i] = o[i]; }
        if (A.xform) {
            float* out = A.xform + (size_t)blockIdx.x * 13;
            for (int i = 0; i < 13; ++i) out[i] = (float)xf[i];
        }
    }
    __syncthreads();
    double T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = xf[i];

    // ---- pass 3: the errors
    double acc[1] = {0.0};
    float* err = A.err + base;
    for (int i = tid; i < N; i += EV_ALIGN_THREADS) {
        float e32 = 0.f;
        if (!mask || mask[i]) {
            const double p[3] = {(double)est[i * 3], (double)est[i * 3 + 1], (double)est[i * 3 + 2]};
            double d2 = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double a = T[0] * (T[1 + r * 3] * p[0] + T[2 + r * 3] * p[1] + T[3 + r * 3] * p[2]) + T[10 + r];
                const double d = a - ((double)gt[i * 3 + r] - T[13 + r]);
                d2 += d * d;
            }
            const double e = sqrt(d2);
            acc[0] += e;
            e32 = (float)e;
        }
        err[i] = e32;
    }
    if (A.mean) {                                   // (uniform over the workgroup)
        ev_block_sum<1>(acc, red);
        if (tid == 0) A.mean[blockIdx.x] = (float)(acc[0] / n);                       // no valid point: 0 / 0
    }
}

extern "C" int sfx_eval_align(int32_t mode, int32_t B, int32_t N, const float* est_dev, const float* gt_dev,
                              const unsigned char* mask_dev, const int32_t* anchors, int32_t n_anchors,
                              float* err_dev, float* mean_dev, float* xform_dev, void* stream) {
    if (B == 0) return 0;
    if (B < 0) { sfx_set_error("sfx_eval_align: B = %d", B); return -1; }
    if (N < 1 || N > EV_MAX_POINTS) { sfx_set_error("sfx_eval_align: N = %d points, supported 1..%d", N, EV_MAX_POINTS); return -1; }
    if (mode < SFX_ALIGN_NONE || mode > SFX_ALIGN_PELVIS) { sfx_set_error("sfx_eval_align: mode %d (0 .. 3: SFX_ALIGN_*)", mode); return -1; }
    if (!est_dev || !gt_dev || !err_dev) { sfx_set_error("sfx_eval_align: a required pointer is NULL"); return -1; }
    AlignArgs A{};
    A.mode = mode; A.N = N;
    if (mode == SFX_ALIGN_PELVIS) {
        if (!anchors || n_anchors < 1 || n_anchors > SFX_ALIGN_MAX_ANCHORS) {
            sfx_set_error("sfx_eval_align: %d anchors, supported 1..%d", anchors ? n_anchors : 0, SFX_ALIGN_MAX_ANCHORS); return -1; }
        for (int k = 0; k < n_anchors; ++k) {
            if (anchors[k] < 0 || anchors[k] >= N) { sfx_set_error("sfx_eval_align: anchor %d outside the %d points", anchors[k], N); return -1; }
            A.anchors[k] = anchors[k];
        }
        A.n_anchors = n_anchors;
    }
    A.est = est_dev; A.gt = gt_dev; A.mask = mask_dev; A.err = err_dev; A.mean = mean_dev; A.xform = xform_dev;
    hipLaunchKernelGGL(k_eval_align, dim3(B), dim3(EV_ALIGN_THREADS), 0, (hipStream_t)stream, A);
    SFX_CHECK(hipGetLastError());
    return 0;
}

struct NearestArgs {
    int Na, Nb, n_thresh, b0;
    double thresh[SFX_NEAREST_MAX_THRESH];
    const float* a; const float* b; const unsigned char* ma; const unsigned char* mb;
    float* dab; float* dba; int* cab; int* cba; int* valid;
};

__global__ __launch_bounds__(EV_NN_THREADS)
void k_eval_nearest(const NearestArgs A) {
    __shared__ float4 tile[EV_NN_TILE];
    const int dir = blockIdx.z, tid = threadIdx.x;
    const int Nq = dir ? A.Nb : A.Na, Nt = dir ? A.Na : A.Nb;
    const int q0 = blockIdx.x * (EV_NN_THREADS * EV_NN_QPT);
    if (q0 >= Nq) return;                                   // (the whole workgroup: the grid is sized for the larger set)
    const size_t mesh = (size_t)A.b0 + blockIdx.y;
    const float* Q = (dir ? A.b : A.a) + mesh * Nq * 3;
    const float* T = (dir ? A.a : A.b) + mesh * Nt * 3;
    const unsigned char* mq = dir ? A.mb : A.ma;
    const unsigned char* mt = dir ? A.ma : A.mb;
    if (mq) mq += mesh * Nq;
    if (mt) mt += mesh * Nt;

    const float INF = __int_as_float(0x7f800000);
    float qx[EV_NN_QPT], qy[EV_NN_QPT], qz[EV_NN_QPT], best[EV_NN_QPT];
    bool have[EV_NN_QPT];
#pragma unroll
    for (int k = 0; k < EV_NN_QPT; ++k) {
        const int i = q0 + k * EV_NN_THREADS + tid;
        have[k] = i < Nq && (!mq || mq[i]);
        qx[k] = have[k] ? Q[i * 3] : 0.f; qy[k] = have[k] ? Q[i * 3 + 1] : 0.f; qz[k] = have[k] ? Q[i * 3 + 2] : 0.f;
        best[k] = INF;
    }
    for (int t0 = 0; t0 < Nt; t0 += EV_NN_TILE) {
        __syncthreads();                                    // (the previous tile has been read by every wave)
        for (int j = tid; j < EV_NN_TILE; j += EV_NN_THREADS) {
            const int g = t0 + j;
            float4 p = make_float4(INF, INF, INF, 0.f);
            if (g < Nt && (!mt || mt[g])) { p.x = T[g * 3]; p.y = T[g * 3 + 1]; p.z = T[g * 3 + 2]; }
            tile[j] = p;
        }
        __syncthreads();
        const int nt = min(EV_NN_TILE, Nt - t0);
#pragma unroll 8
        for (int j = 0; j < nt; ++j) {
            const float4 p = tile[j];
#pragma unroll
            for (int k = 0; k < EV_NN_QPT; ++k) {
                const float dx = qx[k] - p.x, dy = qy[k] - p.y, dz = qz[k] - p.z;
                best[k] = fminf(best[k], dx * dx + dy * dy + dz * dz);
            }
        }
    }
    float* dist = dir ? A.dba : A.dab;
    int* cnt = dir ? A.cba : A.cab;
    const int lane = tid & 63;
    int n_have = 0;
#pragma unroll
    for (int k = 0; k < EV_NN_QPT; ++k) {
        const int i = q0 + k * EV_NN_THREADS + tid;
        const bool found = have[k] && best[k] < INF;        // no valid target at all: distance 0, counted nowhere
        const float d = found ? sqrtf(best[k]) : 0.f;
        if (dist && i < Nq) dist[mesh * Nq + i] = d;
        n_have += __popcll(__ballot(have[k]));
        for (int t = 0; t < A.n_thresh; ++t) {
            const int c = __popcll(__ballot(found && (double)d < A.thresh[t]));
            if (lane == 0 && c) atomicAdd(&cnt[mesh * A.n_thresh + t], c);
        }
    }
    if (A.valid && lane == 0 && n_have) atomicAdd(&A.valid[mesh * 2 + dir], n_have);
}

extern "C" int sfx_eval_nearest(int32_t B, int32_t Na, int32_t Nb, const float* a_dev, const float* b_dev,
                                const unsigned char* mask_a_dev, const unsigned char* mask_b_dev,
                                int32_t n_thresh, const double* thresh, float* dist_ab_dev, float* dist_ba_dev,
                                int32_t* count_ab_dev, int32_t* count_ba_dev, int32_t* valid_dev, void* stream) {
    if (B == 0) return 0;
    if (B < 0) { sfx_set_error("sfx_eval_nearest: B = %d", B); return -1; }
    if (Na < 1 || Nb < 1 || Na > EV_MAX_POINTS || Nb > EV_MAX_POINTS) {
        sfx_set_error("sfx_eval_nearest: Na = %d, Nb = %d points, supported 1..%d", Na, Nb, EV_MAX_POINTS); return -1; }
    if (n_thresh < 0 || n_thresh > SFX_NEAREST_MAX_THRESH) {
        sfx_set_error("sfx_eval_nearest: %d thresholds, supported 0..%d", n_thresh, SFX_NEAREST_MAX_THRESH); return -1; }
    if (!a_dev || !b_dev) { sfx_set_error("sfx_eval_nearest: a required pointer is NULL"); return -1; }
    if (n_thresh > 0 && (!thresh || !count_ab_dev || !count_ba_dev)) {
        sfx_set_error("sfx_eval_nearest: thresholds without the threshold array or the count outputs"); return -1; }
    NearestArgs A{};
    A.Na = Na; A.Nb = Nb; A.n_thresh = n_thresh;
    for (int t = 0; t < n_thresh; ++t) A.thresh[t] = thresh[t];
    A.a = a_dev; A.b = b_dev; A.ma = mask_a_dev; A.mb = mask_b_dev; A.dab = dist_ab_dev; A.dba = dist_ba_dev;
    A.cab = n_thresh > 0 ? count_ab_dev : nullptr; A.cba = n_thresh > 0 ? count_ba_dev : nullptr; A.valid = valid_dev;
    hipStream_t s = (hipStream_t)stream;
    if (n_thresh > 0) {
        SFX_CHECK(hipMemsetAsync(count_ab_dev, 0, sizeof(int32_t) * (size_t)B * n_thresh, s));
        SFX_CHECK(hipMemsetAsync(count_ba_dev, 0, sizeof(int32_t) * (size_t)B * n_thresh, s));
    }
    if (valid_dev) SFX_CHECK(hipMemsetAsync(valid_dev, 0, sizeof(int32_t) * (size_t)B * 2, s));
    const int per = EV_NN_THREADS * EV_NN_QPT, tiles = (std::max(Na, Nb) + per - 1) / per;
    for (int b0 = 0; b0 < B; b0 += EV_GRID_Y) {             // (gridDim.y holds 65 535 meshes)
        A.b0 = b0;
        hipLaunchKernelGGL(k_eval_nearest, dim3(tiles, std::min(B - b0, EV_GRID_Y), 2), dim3(EV_NN_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
    }
    return 0;
}
