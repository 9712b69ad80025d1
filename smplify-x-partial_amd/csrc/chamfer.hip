// chamfer.hip -- the differentiable nearest-point (chamfer) term between B pairs of point sets on the device:
// sfx_chamfer_forward and sfx_chamfer_backward (include/sfx.h holds the contract; csrc/chamfer_math.h the arithmetic).
// Compiled with -ffp-contract=off (csrc/units.txt): the squared distance is float32 without a fused multiply-add, so index and
// distance equal numpy's float32 argmin / min bit for bit.
//
// Forward
//   k_chamfer_nearest   the structure of k_eval_nearest (csrc/evaluate.hip): CH_NN_QPT x 256 queries of one set in registers, the
//                       other set walked in tiles of CH_NN_TILE points staged in LDS as float4, one broadcast LDS read per
//                       target.  Beside the running minimum it keeps the running index, replaced on strict < (the lowest index
//                       wins a tie), and counts the valid targets it staged.  A masked target is staged as +inf and is never
//                       nearer than anything.  Writes index, squared distance and the per-point value w rho(s).
//                       grid (query tiles, meshes, 2 directions)
//   k_chamfer_reduce    one workgroup per (mesh, direction): float64 sum of the per-point values in a fixed order (a thread's
//                       points in index order, the lanes by wave_sum_dpp, the waves in wave order: ev_block_sum of evaluate.hip),
//                       rounded to float32 once; the number of valid queries beside it
// Backward: scatter-add without float atomics, through an inverted index built per call (integers only)
//   k_chamfer_count     counts[target] += 1 for every query with a target (integer atomics: the result has no order)
//   k_chamfer_scan      one workgroup per (mesh, destination set): exclusive scan of the counts; zeroes them for the fill
//   k_chamfer_fill      every query takes the next free place of its bucket (integer atomic cursor: any order)
//   k_chamfer_order     every query moves to its rank inside its bucket (ch_rank): the buckets are now ascending, whatever the
//                       fill's order was
//   k_chamfer_rows      one thread per output row: its gather term, then its list by ch_rows_body, which states the order of
//                       the sum.  Every sum is float64 in a fixed order and is rounded to float32 once.
// No kernel uses a float atomic; a mesh's bits depend on its own points only.  The bodies of the reduce, of the four index
// steps and of the walk of a row's list are in csrc/chamfer_index.h, which csrc/p2m.hip (the point-to-triangle term) uses too;
// so are what both units' entries refuse alike and their loop over chunks of meshes.
#include "../../include/sfx.h"
#include "sfx_internal.h"
#include "wave_ops.h"
#include "chamfer_math.h"
#include "chamfer_index.h"

#define CH_NN_THREADS 256
#define CH_NN_QPT 2
#define CH_NN_TILE 1024

typedef float ch_f2 __attribute__((ext_vector_type(2)));
static_assert(CH_NN_QPT == 2, "k_chamfer_nearest packs the two queries of a thread");

struct ChamferArgs {
    int Na, Nb, b0, want;                       // want: bit 0 = da, bit 1 = db (backward)
    double r2;
    const float* a; const float* b; const unsigned char* ma; const unsigned char* mb; const float* wa; const float* wb;
    int* iab; int* iba; float* sab; float* sba;
    float* val;                                 // forward scratch [B][Na + Nb]: per-point values, a's queries first
    float* loss; int* valid;
    const float* grad; float* da; float* db;
    int* cnt; int* off; int* list; int* sorted; // backward scratch (sfx_chamfer_backward lays it out)
};

// ------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(CH_NN_THREADS)
void k_chamfer_nearest(const ChamferArgs A) {
    __shared__ float4 tile[CH_NN_TILE];
    __shared__ int wave_targets[CH_NN_THREADS / 64];
    const int dir = blockIdx.z, tid = threadIdx.x;
    const int Nq = dir ? A.Nb : A.Na, Nt = dir ? A.Na : A.Nb;
    const int q0 = blockIdx.x * (CH_NN_THREADS * CH_NN_QPT);
    if (q0 >= Nq) return;                                   // (the whole workgroup: the grid is sized for the larger set)
    const size_t mesh = (size_t)A.b0 + blockIdx.y;
    const float* Q = (dir ? A.b : A.a) + mesh * Nq * 3;
    const float* T = (dir ? A.a : A.b) + mesh * Nt * 3;
    const unsigned char* mq = dir ? A.mb : A.ma;
    const unsigned char* mt = dir ? A.ma : A.mb;
    const float* wq = dir ? A.wb : A.wa;
    if (mq) mq += mesh * Nq;
    if (mt) mt += mesh * Nt;
    if (wq) wq += mesh * Nq;

    const float INF = __int_as_float(0x7f800000);
    float qx[CH_NN_QPT], qy[CH_NN_QPT], qz[CH_NN_QPT], best[CH_NN_QPT];
    int bi[CH_NN_QPT];
    bool have[CH_NN_QPT];
#pragma unroll
    for (int k = 0; k < CH_NN_QPT; ++k) {
        const int i = q0 + k * CH_NN_THREADS + tid;
        have[k] = i < Nq && (!mq || mq[i]);
        qx[k] = have[k] ? Q[(size_t)i * 3] : 0.f; qy[k] = have[k] ? Q[(size_t)i * 3 + 1] : 0.f; qz[k] = have[k] ? Q[(size_t)i * 3 + 2] : 0.f;
        best[k] = INF; bi[k] = -1;
    }
    int staged = 0;                                         // valid targets this thread staged
    for (int t0 = 0; t0 < Nt; t0 += CH_NN_TILE) {
        __syncthreads();                                    // (the previous tile has been read by every wave)
        for (int j = tid; j < CH_NN_TILE; j += CH_NN_THREADS) {
            const int g = t0 + j;
            float4 p = make_float4(INF, INF, INF, 0.f);
            if (g < Nt && (!mt || mt[g])) { p.x = T[(size_t)g * 3]; p.y = T[(size_t)g * 3 + 1]; p.z = T[(size_t)g * 3 + 2]; ++staged; }
            tile[j] = p;
        }
        __syncthreads();
        const int nt = min(CH_NN_TILE, Nt - t0);
#pragma unroll 8
        for (int j = 0; j < nt; ++j) {
            const float4 p = tile[j];
            // both queries of the thread side by side (packed float32 adds and multiplies: the same IEEE operations per half)
            const ch_f2 dx = ch_f2{qx[0], qx[1]} - p.x, dy = ch_f2{qy[0], qy[1]} - p.y, dz = ch_f2{qz[0], qz[1]} - p.z;
            const ch_f2 s2 = (dx * dx + dy * dy) + dz * dz;
            const float s[CH_NN_QPT] = {s2.x, s2.y};
#pragma unroll
            for (int k = 0; k < CH_NN_QPT; ++k) {
                const bool nearer = s[k] < best[k];         // strict: the lowest index keeps a tie; false for +inf and NaN
                best[k] = nearer ? s[k] : best[k];
                bi[k] = nearer ? t0 + j : bi[k];
            }
        }
    }
    // valid targets of this mesh and direction (every workgroup counts them for itself: integers, no order)
    {
        const int incl = wave_incl_scan_dpp(staged);
        if ((tid & 63) == 63) wave_targets[tid >> 6] = incl;
    }
    __syncthreads();
    int n_targets = 0;
#pragma unroll
    for (int w = 0; w < CH_NN_THREADS / 64; ++w) n_targets += wave_targets[w];

    int* idx = (dir ? A.iba : A.iab) + mesh * Nq;
    float* dist2 = dir ? A.sba : A.sab;
    float* val = A.val + mesh * ((size_t)A.Na + A.Nb) + (dir ? A.Na : 0);
    const float QNAN = __int_as_float(0x7fc00000);
#pragma unroll
    for (int k = 0; k < CH_NN_QPT; ++k) {
        const int i = q0 + k * CH_NN_THREADS + tid;
        if (i >= Nq) continue;
        int oi = -1; float os = 0.f, ov = 0.f;
        if (have[k]) {
            if (bi[k] >= 0) { oi = bi[k]; os = best[k]; ov = ch_point_value(best[k], wq ? wq[i] : 1.f, A.r2); }
            else if (n_targets > 0) { os = QNAN; ov = QNAN; }     // valid targets, none nearer than +inf: non-finite coordinates
        }
        idx[i] = oi;
        if (dist2) dist2[mesh * Nq + i] = os;
        val[i] = ov;
    }
}

__global__ __launch_bounds__(CH_RED_THREADS)
void k_chamfer_reduce(const ChamferArgs A) {
    const int dir = blockIdx.x;
    const size_t mesh = (size_t)A.b0 + blockIdx.y;
    const int Nq = dir ? A.Nb : A.Na;
    const float* val = A.val + mesh * ((size_t)A.Na + A.Nb) + (dir ? A.Na : 0);
    const unsigned char* mq = dir ? A.mb : A.ma;
    if (mq) mq += mesh * Nq;
    ch_reduce_body(val, mq, Nq, A.loss + mesh * 2 + dir, A.valid ? A.valid + mesh * 2 + dir : nullptr);
}

// ----------------------------------------------------------------------------------------------------------- backward
// Destination set X = blockIdx.z (0: a, 1: b).  Its rows receive a gather term from X's own queries (direction X) and scatter
// terms from the queries of the other set Y (direction 1 - X) whose nearest target they are.  Per mesh the scratch holds, for
// both destination sets one behind the other (a first): counts [Na + Nb], offsets [Na + Nb + 2], list and sorted [Nb + Na].
struct ChamferSide {
    int Nd, Nq;                      // rows of the destination set, queries of the other set
    const float* X; const float* Y;  // this mesh's destination and query points
    const unsigned char* mx; const unsigned char* my; const float* wx; const float* wy;
    const int* idx_own; const int* idx_in;      // X's own nearest targets (into Y); Y's nearest targets (into X)
    int* cnt; int* off; int* list; int* sorted;
    float* out; float g_own, g_in;
};

__device__ __forceinline__ ChamferSide chamfer_side(const ChamferArgs& A, size_t mesh, int set) {
    ChamferSide S;
    const size_t Na = A.Na, Nb = A.Nb;
    S.Nd = set ? A.Nb : A.Na; S.Nq = set ? A.Na : A.Nb;
    const float* a = A.a + mesh * Na * 3; const float* b = A.b + mesh * Nb * 3;
    const unsigned char* ma = A.ma ? A.ma + mesh * Na : nullptr; const unsigned char* mb = A.mb ? A.mb + mesh * Nb : nullptr;
    const float* wa = A.wa ? A.wa + mesh * Na : nullptr; const float* wb = A.wb ? A.wb + mesh * Nb : nullptr;
    const int* iab = A.iab + mesh * Na; const int* iba = A.iba + mesh * Nb;
    S.X = set ? b : a; S.Y = set ? a : b; S.mx = set ? mb : ma; S.my = set ? ma : mb; S.wx = set ? wb : wa; S.wy = set ? wa : wb;
    S.idx_own = set ? iba : iab; S.idx_in = set ? iab : iba;
    S.cnt = A.cnt + mesh * (Na + Nb) + (set ? Na : 0);
    S.off = A.off + mesh * (Na + Nb + 2) + (set ? Na + 1 : 0);
    S.list = A.list + mesh * (Na + Nb) + (set ? Nb : 0);
    S.sorted = A.sorted + mesh * (Na + Nb) + (set ? Nb : 0);
    float* out = set ? A.db : A.da;
    S.out = out ? out + mesh * (size_t)S.Nd * 3 : nullptr;
    S.g_own = A.grad[mesh * 2 + set]; S.g_in = A.grad[mesh * 2 + 1 - set];
    return S;
}

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_chamfer_count(const ChamferArgs A) {
    const int set = blockIdx.z;
    if (!(A.want >> set & 1)) return;
    ch_count_body(chamfer_side(A, (size_t)A.b0 + blockIdx.y, set), blockIdx.x * CH_ROW_THREADS + threadIdx.x);
}

__global__ __launch_bounds__(CH_RED_THREADS)
void k_chamfer_scan(const ChamferArgs A) {
    const int set = blockIdx.x;
    if (!(A.want >> set & 1)) return;
    ch_scan_body(chamfer_side(A, (size_t)A.b0 + blockIdx.y, set));
}

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_chamfer_fill(const ChamferArgs A) {
    const int set = blockIdx.z;
    if (!(A.want >> set & 1)) return;
    ch_fill_body(chamfer_side(A, (size_t)A.b0 + blockIdx.y, set), blockIdx.x * CH_ROW_THREADS + threadIdx.x);
}

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_chamfer_order(const ChamferArgs A) {
    const int set = blockIdx.z;
    if (!(A.want >> set & 1)) return;
    ch_order_body(chamfer_side(A, (size_t)A.b0 + blockIdx.y, set), blockIdx.x * CH_ROW_THREADS + threadIdx.x);
}

// what query q of the other set (target: the row at x) adds to that row: -c (y_q - x)
__device__ __forceinline__ void chamfer_scatter_term(const ChamferSide& S, double r2, int q, const float (&x)[3], double (&p)[3]) {
    const float x0 = x[0], x1 = x[1], x2 = x[2];
    const float y0 = S.Y[(size_t)q * 3], y1 = S.Y[(size_t)q * 3 + 1], y2 = S.Y[(size_t)q * 3 + 2];
    const float s = ch_dist2(y0, y1, y2, x0, x1, x2);
    const double c = ch_coef(S.g_in, S.wy ? S.wy[q] : 1.f, s, r2);
    p[0] += -(c * ((double)y0 - (double)x0)); p[1] += -(c * ((double)y1 - (double)x1)); p[2] += -(c * ((double)y2 - (double)x2));
}

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_chamfer_rows(const ChamferArgs A) {
    const int set = blockIdx.z;
    if (!(A.want >> set & 1)) return;
    const ChamferSide S = chamfer_side(A, (size_t)A.b0 + blockIdx.y, set);
    if ((int)(blockIdx.x * CH_ROW_THREADS) >= S.Nd) return;             // (the whole workgroup)
    const int r = blockIdx.x * CH_ROW_THREADS + threadIdx.x;
    const bool live = r < S.Nd;
    float x[3] = {0.f, 0.f, 0.f};
    double row[3] = {0.0, 0.0, 0.0};
    if (live) {
        x[0] = S.X[(size_t)r * 3]; x[1] = S.X[(size_t)r * 3 + 1]; x[2] = S.X[(size_t)r * 3 + 2];
        const int t = (!S.mx || S.mx[r]) ? S.idx_own[r] : -1;
        if (ch_index_ok(t, S.Nq)) {                                       // the gather term: c (x - y_t)
            const float x0 = x[0], x1 = x[1], x2 = x[2];
            const float y0 = S.Y[(size_t)t * 3], y1 = S.Y[(size_t)t * 3 + 1], y2 = S.Y[(size_t)t * 3 + 2];
            const float s = ch_dist2(x0, x1, x2, y0, y1, y2);
            const double c = ch_coef(S.g_own, S.wx ? S.wx[r] : 1.f, s, A.r2);
            row[0] = c * ((double)x0 - (double)y0); row[1] = c * ((double)x1 - (double)y1); row[2] = c * ((double)x2 - (double)y2);
        }
    }
    ch_rows_body(S.off, S.sorted, r, live, x, row, [&](const float (&t)[3], int q, double (&p)[3]) { chamfer_scatter_term(S, A.r2, q, t, p); });
    if (live && S.out) { S.out[(size_t)r * 3] = (float)row[0]; S.out[(size_t)r * 3 + 1] = (float)row[1]; S.out[(size_t)r * 3 + 2] = (float)row[2]; }
}

// ---------------------------------------------------------------------------------------------------------- the entries
// what both entries refuse, in the order B, sizes, rho, scratch; 0 = fine
static int chamfer_refuse(const char* entry, int32_t B, int32_t Na, int32_t Nb, float rho, const void* scratch,
                          int64_t scratch_bytes, size_t need) {
    if (B >= 0 && (Na < 1 || Nb < 1 || Na > SFX_CHAMFER_MAX_POINTS || Nb > SFX_CHAMFER_MAX_POINTS)) {
        sfx_set_error("%s: Na = %d, Nb = %d points, supported 1..%d", entry, Na, Nb, SFX_CHAMFER_MAX_POINTS); return -1; }
    return ch_refuse(entry, B, rho, scratch, scratch_bytes, need, "Na", Na, "Nb", Nb);
}

extern "C" int sfx_chamfer_forward(int32_t B, int32_t Na, int32_t Nb, const float* a_dev, const float* b_dev,
                                   const unsigned char* mask_a_dev, const unsigned char* mask_b_dev,
                                   const float* weight_a_dev, const float* weight_b_dev, float rho,
                                   int32_t* idx_ab_dev, int32_t* idx_ba_dev, float* dist2_ab_dev, float* dist2_ba_dev,
                                   float* loss_dev, int32_t* valid_dev, void* scratch_dev, int64_t scratch_bytes, void* stream) {
    if (B == 0) return 0;
    if (chamfer_refuse("sfx_chamfer_forward", B, Na, Nb, rho, scratch_dev, scratch_bytes,
                       B > 0 ? SFX_CHAMFER_FORWARD_SCRATCH_BYTES(B, Na, Nb) : 0)) return -1;
    if (!a_dev || !b_dev || !idx_ab_dev || !idx_ba_dev || !loss_dev) { sfx_set_error("sfx_chamfer_forward: a required pointer is NULL"); return -1; }
    ChamferArgs A{};
    A.Na = Na; A.Nb = Nb; A.r2 = ch_rho2(rho);
    A.a = a_dev; A.b = b_dev; A.ma = mask_a_dev; A.mb = mask_b_dev; A.wa = weight_a_dev; A.wb = weight_b_dev;
    A.iab = idx_ab_dev; A.iba = idx_ba_dev; A.sab = dist2_ab_dev; A.sba = dist2_ba_dev;
    A.val = (float*)scratch_dev; A.loss = loss_dev; A.valid = valid_dev;
    hipStream_t s = (hipStream_t)stream;
    const int per = CH_NN_THREADS * CH_NN_QPT, tiles = (std::max(Na, Nb) + per - 1) / per;
    return ch_mesh_chunks(A, B, [&](int nb) {
        hipLaunchKernelGGL(k_chamfer_nearest, dim3(tiles, nb, 2), dim3(CH_NN_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_chamfer_reduce, dim3(2, nb), dim3(CH_RED_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        return 0;
    });
}

extern "C" int sfx_chamfer_backward(int32_t B, int32_t Na, int32_t Nb, const float* a_dev, const float* b_dev,
                                    const unsigned char* mask_a_dev, const unsigned char* mask_b_dev,
                                    const float* weight_a_dev, const float* weight_b_dev, float rho,
                                    const int32_t* idx_ab_dev, const int32_t* idx_ba_dev, const float* grad_dev,
                                    float* da_dev, float* db_dev, void* scratch_dev, int64_t scratch_bytes, void* stream) {
    if (B == 0) return 0;
    if (chamfer_refuse("sfx_chamfer_backward", B, Na, Nb, rho, scratch_dev, scratch_bytes,
                       B > 0 ? SFX_CHAMFER_BACKWARD_SCRATCH_BYTES(B, Na, Nb) : 0)) return -1;
    if (!a_dev || !b_dev || !idx_ab_dev || !idx_ba_dev || !grad_dev) { sfx_set_error("sfx_chamfer_backward: a required pointer is NULL"); return -1; }
    if (!da_dev && !db_dev) return 0;                        // nothing asked for
    ChamferArgs A{};
    A.Na = Na; A.Nb = Nb; A.r2 = ch_rho2(rho); A.want = (da_dev ? 1 : 0) | (db_dev ? 2 : 0);
    A.a = a_dev; A.b = b_dev; A.ma = mask_a_dev; A.mb = mask_b_dev; A.wa = weight_a_dev; A.wb = weight_b_dev;
    A.iab = const_cast<int32_t*>(idx_ab_dev); A.iba = const_cast<int32_t*>(idx_ba_dev);      // (only ever read here)
    A.grad = grad_dev; A.da = da_dev; A.db = db_dev;
    const size_t n = (size_t)Na + Nb, Bz = (size_t)B;
    A.cnt = (int*)scratch_dev; A.off = A.cnt + Bz * n; A.list = A.off + Bz * (n + 2); A.sorted = A.list + Bz * n;
    hipStream_t s = (hipStream_t)stream;
    SFX_CHECK(hipMemsetAsync(A.cnt, 0, sizeof(int) * Bz * n, s));
    const int tiles = (std::max(Na, Nb) + CH_ROW_THREADS - 1) / CH_ROW_THREADS;
    return ch_mesh_chunks(A, B, [&](int nb) {
        hipLaunchKernelGGL(k_chamfer_count, dim3(tiles, nb, 2), dim3(CH_ROW_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_chamfer_scan, dim3(2, nb), dim3(CH_RED_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_chamfer_fill, dim3(tiles, nb, 2), dim3(CH_ROW_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_chamfer_order, dim3(tiles, nb, 2), dim3(CH_ROW_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_chamfer_rows, dim3(tiles, nb, 2), dim3(CH_ROW_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        return 0;
    });
}
