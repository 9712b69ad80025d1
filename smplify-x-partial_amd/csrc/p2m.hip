// p2m.hip -- the differentiable point-to-triangle term from B point clouds to the surfaces of B meshes of one topology, on the
// device: sfx_p2m_forward and sfx_p2m_backward (include/sfx.h holds the contract; csrc/p2m_math.h the arithmetic).  Compiled
// with -ffp-contract=off (csrc/units.txt): the closest point is float32 without a fused multiply-add, so face, squared distance
// and barycentrics equal a float32 numpy restatement of the contract bit for bit.
//
// Forward
//   k_p2m_nearest   the structure of k_chamfer_nearest: P2M_QPT x 256 points of one cloud in registers, the faces walked in tiles
//                   of P2M_TILE staged in LDS, four broadcast float4 reads per face.  Staging gathers a face's three vertices
//                   through `faces` (a mesh's vertices stay in L2) and stores a, b, c, ab = b - a, ac = c - a: the contract's
//                   own subtractions, formed once per face and workgroup.  b and c are staged beside the differences because
//                   d3 .. d6 are dot products with p - b and p - c.  A face that is masked or names a vertex outside the mesh is
//                   staged as NaN: its s is NaN and never nearer.  The running (s, face) is replaced on strict < (the lowest face
//                   wins a tie); the barycentrics are formed once, for the winner, from its vertices.  The candidate faces a
//                   workgroup staged are counted: none at all gives face -1 / 0, some but none nearer than +inf face -1 / NaN.
//                   grid (point tiles, meshes)
//   k_p2m_reduce    ch_reduce_body of csrc/chamfer_index.h, one workgroup per mesh
// Backward: per point its own row c (p - q); per vertex the sum over the corners that name it, through the inverted index of
// csrc/chamfer_index.h over the 3 Np entries e = 3 i + k (no float atomics)
//   k_p2m_corners   corner[e] = the vertex of corner k of point i's face, -1 where the point has no term
//   k_p2m_count / _scan / _fill / _order     the four integer steps
//   k_p2m_point_rows    dp
//   k_p2m_vertex_rows   dv: the row's list in ascending e by ch_rows_body of csrc/chamfer_index.h, float64, rounded once
// s, q and the barycentrics are formed again from the points with the header: the same bits as the forward's.
#include "../../include/sfx.h"
#include "sfx_internal.h"
#include "wave_ops.h"
#include "chamfer_math.h"
#include "chamfer_index.h"
#include "p2m_math.h"

#define P2M_THREADS 256
#define P2M_QPT 2
#define P2M_TILE 256

struct P2mArgs {
    int Np, Nv, F, b0, want;                    // want: bit 0 = dp, bit 1 = dv (backward)
    double r2;
    const float* p; const float* v; const int* faces;
    const unsigned char* mp; const unsigned char* mf; const float* wp;
    int* face; float* bary; float* dist2;
    float* val;                                 // forward scratch [B][Np]: per-point values
    float* loss; int* valid;
    const float* grad; float* dp; float* dv;
    int* corner; int* cnt; int* off; int* list; int* sorted;    // backward scratch (sfx_p2m_backward lays it out)
};

// the three vertex ids of face f when all of them name a vertex
__device__ __forceinline__ bool p2m_face_ids(const int* faces, int f, int Nv, int (&id)[3]) {
    id[0] = faces[(size_t)f * 3]; id[1] = faces[(size_t)f * 3 + 1]; id[2] = faces[(size_t)f * 3 + 2];
    return ch_index_ok(id[0], Nv) && ch_index_ok(id[1], Nv) && ch_index_ok(id[2], Nv);
}

// ------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(P2M_THREADS)
void k_p2m_nearest(const P2mArgs A) {
    __shared__ float4 tile[P2M_TILE * 4];       // per face: (a, b.x) (b.yz, c.xy) (c.z, ab) (ac, -)
    __shared__ int wave_faces[P2M_THREADS / 64];
    const int tid = threadIdx.x;
    const int q0 = blockIdx.x * (P2M_THREADS * P2M_QPT);
    const size_t mesh = (size_t)A.b0 + blockIdx.y;
    const float* P = A.p + mesh * A.Np * 3;
    const float* V = A.v + mesh * A.Nv * 3;
    const unsigned char* mp = A.mp ? A.mp + mesh * A.Np : nullptr;
    const unsigned char* mf = A.mf ? A.mf + mesh * A.F : nullptr;
    const float* wp = A.wp ? A.wp + mesh * A.Np : nullptr;

    const float INF = __int_as_float(0x7f800000), QNAN = __int_as_float(0x7fc00000);
    float q[P2M_QPT][3], best[P2M_QPT];
    int bi[P2M_QPT];
    bool have[P2M_QPT];
#pragma unroll
    for (int k = 0; k < P2M_QPT; ++k) {
        const int i = q0 + k * P2M_THREADS + tid;
        have[k] = i < A.Np && (!mp || mp[i]);
#pragma unroll
        for (int c = 0; c < 3; ++c) q[k][c] = have[k] ? P[(size_t)i * 3 + c] : 0.f;
        best[k] = INF; bi[k] = -1;
    }
    int staged = 0;                                         // candidate faces this thread staged
    for (int t0 = 0; t0 < A.F; t0 += P2M_TILE) {
        __syncthreads();                                    // (the previous tile has been read by every wave)
        for (int j = tid; j < P2M_TILE; j += P2M_THREADS) {
            const int f = t0 + j;
            float a[3] = {QNAN, QNAN, QNAN}, b[3] = {QNAN, QNAN, QNAN}, c[3] = {QNAN, QNAN, QNAN};
            int id[3];
            if (f < A.F && (!mf || mf[f]) && p2m_face_ids(A.faces, f, A.Nv, id)) {
#pragma unroll
                for (int x = 0; x < 3; ++x) { a[x] = V[(size_t)id[0] * 3 + x]; b[x] = V[(size_t)id[1] * 3 + x]; c[x] = V[(size_t)id[2] * 3 + x]; }
                ++staged;
            }
            tile[j * 4] = make_float4(a[0], a[1], a[2], b[0]);
            tile[j * 4 + 1] = make_float4(b[1], b[2], c[0], c[1]);
            tile[j * 4 + 2] = make_float4(c[2], b[0] - a[0], b[1] - a[1], b[2] - a[2]);
            tile[j * 4 + 3] = make_float4(c[0] - a[0], c[1] - a[1], c[2] - a[2], 0.f);
        }
        __syncthreads();
        const int nt = min(P2M_TILE, A.F - t0);
#pragma unroll 2
        for (int j = 0; j < nt; ++j) {
            const float4 r0 = tile[j * 4], r1 = tile[j * 4 + 1], r2 = tile[j * 4 + 2], r3 = tile[j * 4 + 3];
            const float a[3] = {r0.x, r0.y, r0.z}, b[3] = {r0.w, r1.x, r1.y}, c[3] = {r1.z, r1.w, r2.x};
            const float ab[3] = {r2.y, r2.z, r2.w}, ac[3] = {r3.x, r3.y, r3.z};
#pragma unroll
            for (int k = 0; k < P2M_QPT; ++k) {
                const float s = p2m_closest_staged(q[k], a, b, c, ab, ac).s;
                const bool nearer = s < best[k];            // strict: the lowest face keeps a tie; false for +inf and NaN
                best[k] = nearer ? s : best[k];
                bi[k] = nearer ? t0 + j : bi[k];
            }
        }
    }
    // candidate faces of this mesh (every workgroup counts them for itself: integers, no order)
    {
        const int incl = wave_incl_scan_dpp(staged);
        if ((tid & 63) == 63) wave_faces[tid >> 6] = incl;
    }
    __syncthreads();
    int n_faces = 0;
#pragma unroll
    for (int w = 0; w < P2M_THREADS / 64; ++w) n_faces += wave_faces[w];

#pragma unroll
    for (int k = 0; k < P2M_QPT; ++k) {
        const int i = q0 + k * P2M_THREADS + tid;
        if (i >= A.Np) continue;
        int of = -1; float os = 0.f, ov = 0.f, ob[3] = {0.f, 0.f, 0.f};
        if (have[k]) {
            if (bi[k] >= 0) {                               // the winner once more, from its vertices: the barycentrics
                int id[3];
                p2m_face_ids(A.faces, bi[k], A.Nv, id);     // (a candidate: its ids name vertices)
                const P2mHit h = p2m_closest(q[k], V + (size_t)id[0] * 3, V + (size_t)id[1] * 3, V + (size_t)id[2] * 3);
                of = bi[k]; os = best[k]; ob[0] = h.u; ob[1] = h.v; ob[2] = h.w;
                ov = ch_point_value(best[k], wp ? wp[i] : 1.f, A.r2);
            } else if (n_faces > 0) { os = QNAN; ov = QNAN; ob[0] = ob[1] = ob[2] = QNAN; }    // candidates, none nearer than +inf
        }
        A.face[mesh * A.Np + i] = of;
        if (A.dist2) A.dist2[mesh * A.Np + i] = os;
        if (A.bary) { float* o = A.bary + (mesh * A.Np + i) * 3; o[0] = ob[0]; o[1] = ob[1]; o[2] = ob[2]; }
        A.val[mesh * A.Np + i] = ov;
    }
}

__global__ __launch_bounds__(CH_RED_THREADS)
void k_p2m_reduce(const P2mArgs A) {
    const size_t mesh = (size_t)A.b0 + blockIdx.x;
    ch_reduce_body(A.val + mesh * A.Np, A.mp ? A.mp + mesh * A.Np : nullptr, A.Np, A.loss + mesh, A.valid ? A.valid + mesh : nullptr);
}

// ----------------------------------------------------------------------------------------------------------- backward
// Per mesh the scratch holds corner [3 Np], counts [Nv], offsets [Nv + 1], list and sorted [3 Np].
struct P2mSide {
    int Nd, Nq;                      // vertex rows; corner entries
    const unsigned char* my;         // (none: a point without a term has corner -1)
    const int* idx_in;               // corner [3 Np]
    int* cnt; int* off; int* list; int* sorted;
    const float* P; const float* V; const int* face; const float* wp; float g;
};

__device__ __forceinline__ P2mSide p2m_side(const P2mArgs& A, size_t mesh) {
    P2mSide S;
    const size_t Np = A.Np, Nv = A.Nv;
    S.Nd = A.Nv; S.Nq = 3 * A.Np; S.my = nullptr;
    S.idx_in = A.corner + mesh * 3 * Np;
    S.cnt = A.cnt + mesh * Nv; S.off = A.off + mesh * (Nv + 1);
    S.list = A.list + mesh * 3 * Np; S.sorted = A.sorted + mesh * 3 * Np;
    S.P = A.p + mesh * Np * 3; S.V = A.v + mesh * Nv * 3; S.face = A.face + mesh * Np;
    S.wp = A.wp ? A.wp + mesh * Np : nullptr; S.g = A.grad[mesh];
    return S;
}

// the vertex ids of point i's face when the point has a term: unmasked, a face inside 0 .. F - 1 whose ids name vertices
__device__ __forceinline__ bool p2m_point_ids(const P2mArgs& A, size_t mesh, int i, int (&id)[3]) {
    if (A.mp && !A.mp[mesh * A.Np + i]) return false;
    const int f = A.face[mesh * A.Np + i];
    return ch_index_ok(f, A.F) && p2m_face_ids(A.faces, f, A.Nv, id);
}

// point i against its face: the hit and the factor c
__device__ __forceinline__ double p2m_point_coef(const P2mSide& S, const int (&id)[3], int i, double r2, P2mHit& h) {
    h = p2m_closest(S.P + (size_t)i * 3, S.V + (size_t)id[0] * 3, S.V + (size_t)id[1] * 3, S.V + (size_t)id[2] * 3);
    return ch_coef(S.g, S.wp ? S.wp[i] : 1.f, h.s, r2);
}

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_p2m_corners(const P2mArgs A) {
    const size_t mesh = (size_t)A.b0 + blockIdx.y;
    const int e = blockIdx.x * CH_ROW_THREADS + threadIdx.x;
    if (e >= 3 * A.Np) return;
    int id[3];
    const bool ok = p2m_point_ids(A, mesh, e / 3, id);
    A.corner[mesh * 3 * A.Np + e] = ok ? id[e % 3] : -1;
}

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_p2m_count(const P2mArgs A) { ch_count_body(p2m_side(A, (size_t)A.b0 + blockIdx.y), blockIdx.x * CH_ROW_THREADS + threadIdx.x); }

__global__ __launch_bounds__(CH_RED_THREADS)
void k_p2m_scan(const P2mArgs A) { ch_scan_body(p2m_side(A, (size_t)A.b0 + blockIdx.x)); }

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_p2m_fill(const P2mArgs A) { ch_fill_body(p2m_side(A, (size_t)A.b0 + blockIdx.y), blockIdx.x * CH_ROW_THREADS + threadIdx.x); }

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_p2m_order(const P2mArgs A) { ch_order_body(p2m_side(A, (size_t)A.b0 + blockIdx.y), blockIdx.x * CH_ROW_THREADS + threadIdx.x); }

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_p2m_point_rows(const P2mArgs A) {
    const size_t mesh = (size_t)A.b0 + blockIdx.y;
    const int i = blockIdx.x * CH_ROW_THREADS + threadIdx.x;
    if (i >= A.Np) return;
    const P2mSide S = p2m_side(A, mesh);
    double row[3] = {0.0, 0.0, 0.0};
    int id[3];
    if (p2m_point_ids(A, mesh, i, id)) {
        P2mHit h;
        const double c = p2m_point_coef(S, id, i, A.r2, h);
        p2m_point_term(S.P + (size_t)i * 3, h, c, row);
    }
    float* o = A.dp + (mesh * A.Np + i) * 3;
    o[0] = (float)row[0]; o[1] = (float)row[1]; o[2] = (float)row[2];
}

// what entry e = 3 i + k adds to the row of its vertex: -(c bary_k)(p_i - q_i)
__device__ __forceinline__ void p2m_scatter_term(const P2mArgs& A, const P2mSide& S, int e, double (&acc)[3]) {
    const int i = e / 3;
    int id[3];
    p2m_face_ids(A.faces, S.face[i], A.Nv, id);             // (an entry of a list: its point has a term)
    P2mHit h;
    const double c = p2m_point_coef(S, id, i, A.r2, h);
    p2m_corner_term(S.P + (size_t)i * 3, h, e % 3, c, acc);
}

__global__ __launch_bounds__(CH_ROW_THREADS)
void k_p2m_vertex_rows(const P2mArgs A) {
    const size_t mesh = (size_t)A.b0 + blockIdx.y;
    const P2mSide S = p2m_side(A, mesh);
    const int r = blockIdx.x * CH_ROW_THREADS + threadIdx.x;
    const bool live = r < S.Nd;
    const float none[3] = {0.f, 0.f, 0.f};                              // (a corner's term reads nothing of its vertex)
    double row[3] = {0.0, 0.0, 0.0};
    ch_rows_body(S.off, S.sorted, r, live, none, row, [&](const float (&)[3], int e, double (&acc)[3]) { p2m_scatter_term(A, S, e, acc); });
    if (live) { float* out = A.dv + (mesh * A.Nv + r) * 3; out[0] = (float)row[0]; out[1] = (float)row[1]; out[2] = (float)row[2]; }
}

// ---------------------------------------------------------------------------------------------------------- the entries
// what both entries refuse, in the order B, sizes, rho, scratch; 0 = fine
static int p2m_refuse(const char* entry, int32_t B, int32_t Np, int32_t Nv, int32_t F, float rho, const void* scratch,
                      int64_t scratch_bytes, size_t need) {
    if (B >= 0 && (Np < 1 || Np > SFX_P2M_MAX_POINTS || Nv < 1 || Nv > SFX_P2M_MAX_POINTS || F < 1 || F > SFX_P2M_MAX_POINTS)) {
        sfx_set_error("%s: Np = %d points, Nv = %d vertices, F = %d faces, supported 1..%d each", entry, Np, Nv, F, SFX_P2M_MAX_POINTS); return -1; }
    return ch_refuse(entry, B, rho, scratch, scratch_bytes, need, "Np", Np, "Nv", Nv);
}

extern "C" int sfx_p2m_forward(int32_t B, int32_t Np, int32_t Nv, int32_t F, const float* p_dev, const float* v_dev,
                               const int32_t* faces_dev, const unsigned char* mask_p_dev, const unsigned char* mask_f_dev,
                               const float* weight_p_dev, float rho, int32_t* face_dev, float* bary_dev, float* dist2_dev,
                               float* loss_dev, int32_t* valid_dev, void* scratch_dev, int64_t scratch_bytes, void* stream) {
    if (B == 0) return 0;
    if (p2m_refuse("sfx_p2m_forward", B, Np, Nv, F, rho, scratch_dev, scratch_bytes,
                   B > 0 ? SFX_P2M_FORWARD_SCRATCH_BYTES(B, Np, Nv) : 0)) return -1;
    if (!p_dev || !v_dev || !faces_dev || !face_dev || !loss_dev) { sfx_set_error("sfx_p2m_forward: a required pointer is NULL"); return -1; }
    P2mArgs A{};
    A.Np = Np; A.Nv = Nv; A.F = F; A.r2 = ch_rho2(rho);
    A.p = p_dev; A.v = v_dev; A.faces = faces_dev; A.mp = mask_p_dev; A.mf = mask_f_dev; A.wp = weight_p_dev;
    A.face = face_dev; A.bary = bary_dev; A.dist2 = dist2_dev;
    A.val = (float*)scratch_dev; A.loss = loss_dev; A.valid = valid_dev;
    hipStream_t s = (hipStream_t)stream;
    const int per = P2M_THREADS * P2M_QPT, tiles = (Np + per - 1) / per;
    return ch_mesh_chunks(A, B, [&](int nb) {
        hipLaunchKernelGGL(k_p2m_nearest, dim3(tiles, nb), dim3(P2M_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_p2m_reduce, dim3(nb), dim3(CH_RED_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        return 0;
    });
}

extern "C" int sfx_p2m_backward(int32_t B, int32_t Np, int32_t Nv, int32_t F, const float* p_dev, const float* v_dev,
                                const int32_t* faces_dev, const unsigned char* mask_p_dev, const float* weight_p_dev, float rho,
                                const int32_t* face_dev, const float* grad_dev, float* dp_dev, float* dv_dev,
                                void* scratch_dev, int64_t scratch_bytes, void* stream) {
    if (B == 0) return 0;
    if (p2m_refuse("sfx_p2m_backward", B, Np, Nv, F, rho, scratch_dev, scratch_bytes,
                   B > 0 ? SFX_P2M_BACKWARD_SCRATCH_BYTES(B, Np, Nv) : 0)) return -1;
    if (!p_dev || !v_dev || !faces_dev || !face_dev || !grad_dev) { sfx_set_error("sfx_p2m_backward: a required pointer is NULL"); return -1; }
    if (!dp_dev && !dv_dev) return 0;                        // nothing asked for
    P2mArgs A{};
    A.Np = Np; A.Nv = Nv; A.F = F; A.r2 = ch_rho2(rho); A.want = (dp_dev ? 1 : 0) | (dv_dev ? 2 : 0);
    A.p = p_dev; A.v = v_dev; A.faces = faces_dev; A.mp = mask_p_dev; A.wp = weight_p_dev;
    A.face = const_cast<int32_t*>(face_dev);                 // (only ever read here)
    A.grad = grad_dev; A.dp = dp_dev; A.dv = dv_dev;
    const size_t n3 = (size_t)3 * Np, nv = (size_t)Nv, Bz = (size_t)B;
    A.corner = (int*)scratch_dev; A.cnt = A.corner + Bz * n3; A.off = A.cnt + Bz * nv; A.list = A.off + Bz * (nv + 1); A.sorted = A.list + Bz * n3;
    hipStream_t s = (hipStream_t)stream;
    if (dv_dev) SFX_CHECK(hipMemsetAsync(A.cnt, 0, sizeof(int) * Bz * nv, s));
    const int point_tiles = (Np + CH_ROW_THREADS - 1) / CH_ROW_THREADS, entry_tiles = (int)((n3 + CH_ROW_THREADS - 1) / CH_ROW_THREADS);
    const int vertex_tiles = (Nv + CH_ROW_THREADS - 1) / CH_ROW_THREADS;
    return ch_mesh_chunks(A, B, [&](int nb) {
        if (dp_dev) {
            hipLaunchKernelGGL(k_p2m_point_rows, dim3(point_tiles, nb), dim3(CH_ROW_THREADS), 0, s, A);
            SFX_CHECK(hipGetLastError());
        }
        if (!dv_dev) return 0;
        hipLaunchKernelGGL(k_p2m_corners, dim3(entry_tiles, nb), dim3(CH_ROW_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_p2m_count, dim3(entry_tiles, nb), dim3(CH_ROW_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_p2m_scan, dim3(nb), dim3(CH_RED_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_p2m_fill, dim3(entry_tiles, nb), dim3(CH_ROW_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_p2m_order, dim3(entry_tiles, nb), dim3(CH_ROW_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_p2m_vertex_rows, dim3(vertex_tiles, nb), dim3(CH_ROW_THREADS), 0, s, A);
        SFX_CHECK(hipGetLastError());
        return 0;
    });
}
