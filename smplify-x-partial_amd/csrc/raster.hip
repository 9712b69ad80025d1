// raster.hip -- fitted meshes drawn over their images on the device: the kernels behind sfx_render_meshes (include/sfx.h, where the
// geometry and coverage contract is written down; the entry itself is host/render.hip).
//
// Replaces render_mesh (smplifyx/utils.py:497-538: trimesh + pyrender's offscreen OpenGL, one context per frame on the host) for B
// meshes of one topology that already sit in device memory.  The camera is the fit camera exactly as
// camera.PerspectiveCamera.forward has it: p_c = R p + t, x = fx X / Z + cx, y = fy Y / Z + cy, pixel centres at (i + 0.5, j + 0.5),
// y down.  The reference's detour -- the mesh rotated by 180 degrees about x, transl[0] negated, an OpenGL camera looking down -z --
// is algebraically this projection with R = I.
//
//   k_rs_project   one thread per (mesh, vertex): screen = (x, y, Z), the position snapped to 1/256 pixel, or the unusable mark
//   k_rs_vnormals  one thread per (mesh, vertex): the un-normalised cross products of the vertex's usable faces in camera space,
//                  gathered in the order of the vertex -> face lists (fixed order, no float atomics), normalised
//   (clear)        the visibility buffer, uint64 [B][H][W], to all-ones by hipMemsetAsync
//   k_rs_cover     one lane per triangle.  A body triangle covers a handful of pixels: the lane walks its clipped box and issues one
//                  64-bit atomicMin of (bits(depth) << 32 | triangle) per covered pixel (a native global_atomic_umin_x2, no
//                  compare-and-swap loop).  The pixel's key is read first and the atomic skipped when it is already smaller: the
//                  key only ever decreases, so a stale read costs a wasted atomic, never a wrong result.  A triangle whose box
//                  holds more than RS_LANE_MAX pixels (a mesh at the camera, one triangle across the image) goes to a per-wave
//                  list in LDS that the whole wavefront then walks 64 pixels at a time: no lane loops over more than
//                  RS_LANE_MAX pixels alone.
//   k_rs_resolve   one thread per pixel: the winning triangle's edge values and depth again through the SAME functions as the
//                  cover kernel (rs_fetch, rs_covers, rs_depth: same bits), perspective-correct barycentrics, shading,
//                  compositing; writes rgba, depth, tri.
// The unit is compiled with -ffp-contract=off (units.txt): no multiply-add is fused, so a function gives the same bits wherever
// it is inlined.  Coverage is integer (raster_fixed.h); depth and shading are float32.
#include "../../include/sfx.h"
#include "sfx_internal.h"
#include "raster_fixed.h"

#define RS_THREADS 256
#define RS_WAVES (RS_THREADS / 64)
#define RS_LANE_MAX 256                 // pixels of a clipped box one lane walks alone
#define RS_EMPTY 0xffffffffffffffffull

static_assert(SFX_RENDER_MAX_LIGHTS == 8, "RasterArgs holds 8 lights");

struct RsCam { float R[9], t[3], fx, fy, cx, cy; };

__device__ __forceinline__ RsCam rs_load_cam(const RasterArgs& A, int b) {
    RsCam c;
    for (int i = 0; i < 9; ++i) c.R[i] = A.rot ? A.rot[(size_t)b * 9 + i] : (i % 4 == 0 ? 1.f : 0.f);
    for (int i = 0; i < 3; ++i) c.t[i] = A.trans[(size_t)b * 3 + i];
    c.fx = A.focal[(size_t)b * 2]; c.fy = A.focal[(size_t)b * 2 + 1];
    c.cx = A.center[(size_t)b * 2]; c.cy = A.center[(size_t)b * 2 + 1];
    return c;
}

// one coordinate of p_c = R p + t: the one expression every kernel evaluates (same bits everywhere)
__device__ __forceinline__ float rs_cam_coord(const RsCam& c, const float* v, int k) {
    return c.R[k * 3] * v[0] + c.R[k * 3 + 1] * v[1] + c.R[k * 3 + 2] * v[2] + c.t[k];
}

// A triangle as cover and resolve see it: corners, oriented edges, clipped box, camera-space depth (FULL: position) per corner.
struct RsFace { RsTri t; RsBox box; int vi[3]; float p[3][3]; };

// false: nothing to draw -- a corner index outside the mesh or an unusable corner (`unusable`), or zero snapped area
template <bool FULL>
__device__ __forceinline__ bool rs_fetch(const RasterArgs& A, const RsCam& cam, int b, int f, RsFace& T, bool& unusable) {
    int32_t x[3], y[3];
    unusable = false;
    for (int i = 0; i < 3; ++i) {
        T.vi[i] = A.faces[(size_t)f * 3 + i];
        if ((unsigned)T.vi[i] >= (unsigned)A.V) { unusable = true; return false; }
    }
    for (int i = 0; i < 3; ++i) {
        const int2 s = *reinterpret_cast<const int2*>(A.snapped + ((size_t)b * A.V + T.vi[i]) * 2);
        x[i] = s.x; y[i] = s.y;
        unusable = unusable || s.x == RS_UNUSABLE;
    }
    if (unusable) return false;
    T.t = rs_setup(x, y);
    if (T.t.area2 == 0) return false;
    T.box = rs_box(x, y, A.W, A.H);
    for (int i = 0; i < 3; ++i) {
        const float* v = A.verts + ((size_t)b * A.V + T.vi[i]) * 3;
        if (FULL) { T.p[i][0] = rs_cam_coord(cam, v, 0); T.p[i][1] = rs_cam_coord(cam, v, 1); }
        T.p[i][2] = rs_cam_coord(cam, v, 2);
    }
    return true;
}

// lambda_i = e_i / area2 and the perspective-correct depth 1 / sum lambda_i / Z_i
__device__ __forceinline__ float rs_depth(const RsFace& T, const rs_i64 e[3], float lam[3]) {
    const float a = (float)T.t.area2;
    for (int i = 0; i < 3; ++i) lam[i] = (float)e[i] / a;
    const float s = lam[0] / T.p[0][2] + lam[1] / T.p[1][2] + lam[2] / T.p[2][2];
    return 1.0f / s;
}

__device__ __forceinline__ void rs_plot(const RsFace& T, int f, int px, int py, unsigned long long* vis, int W) {
    rs_i64 e[3];
    if (!rs_covers(T.t, px, py, e)) return;
    float lam[3];
    const float d = rs_depth(T, e, lam);
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)f;
    unsigned long long* p = vis + (size_t)py * W + px;
    if (*p > key) atomicMin(p, key);
}

__global__ __launch_bounds__(RS_THREADS)
void k_rs_project(const RasterArgs A, int b0) {
    const int v = blockIdx.x * RS_THREADS + threadIdx.x, b = b0 + blockIdx.y;
    if (v >= A.V) return;
    const RsCam cam = rs_load_cam(A, b);
    const size_t o = (size_t)b * A.V + v;
    const float* p = A.verts + o * 3;
    const float X = rs_cam_coord(cam, p, 0), Y = rs_cam_coord(cam, p, 1), Z = rs_cam_coord(cam, p, 2);
    const float x = X / Z * cam.fx + cam.cx, y = Y / Z * cam.fy + cam.cy;
    if (A.screen) { A.screen[o * 3] = x; A.screen[o * 3 + 1] = y; A.screen[o * 3 + 2] = Z; }
    int2 s = make_int2(RS_UNUSABLE, 0);
    if (rs_usable(x, y, Z, A.znear)) s = make_int2(rs_snap(x), rs_snap(y));
    *reinterpret_cast<int2*>(A.snapped + o * 2) = s;
}

__global__ __launch_bounds__(RS_THREADS)
void k_rs_vnormals(const RasterArgs A, int b0) {
    const int v = blockIdx.x * RS_THREADS + threadIdx.x, b = b0 + blockIdx.y;
    if (v >= A.V) return;
    const RsCam cam = rs_load_cam(A, b);
    const size_t base = (size_t)b * A.V;
    const int lo = max(A.vf_off[v], 0), hi = min(A.vf_off[v + 1], 3 * A.F);
    float n[3] = {0.f, 0.f, 0.f};
    for (int k = lo; k < hi; ++k) {
        const int f = A.vf_faces[k];
        if ((unsigned)f >= (unsigned)A.F) continue;
        float p[3][3];
        bool ok = true;
        for (int i = 0; i < 3; ++i) {
            const int vi = A.faces[(size_t)f * 3 + i];
            ok = ok && (unsigned)vi < (unsigned)A.V;
            if (!ok) break;
            ok = A.snapped[(base + vi) * 2] != RS_UNUSABLE;
            if (!ok) break;
            const float* q = A.verts + (base + vi) * 3;
            for (int c = 0; c < 3; ++c) p[i][c] = rs_cam_coord(cam, q, c);
        }
        if (!ok) continue;                      // a dropped triangle shades nothing
        const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
        const float wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
        n[0] += uy * wz - uz * wy; n[1] += uz * wx - ux * wz; n[2] += ux * wy - uy * wx;
    }
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const float inv = len > 0.f ? 1.0f / len : 0.f;
    for (int c = 0; c < 3; ++c) A.vnormal[(base + v) * 3 + c] = n[c] * inv;
}

__global__ __launch_bounds__(RS_THREADS)
void k_rs_cover(const RasterArgs A, int b0) {
    __shared__ int big[RS_WAVES][64];
    __shared__ int nbig[RS_WAVES];
    const int b = b0 + blockIdx.y, f = blockIdx.x * RS_THREADS + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) nbig[w] = 0;
    __syncthreads();
    const RsCam cam = rs_load_cam(A, b);
    unsigned long long* vis = A.vis + (size_t)b * A.H * A.W;
    RsFace T;
    bool unusable;
    if (f < A.F) {
        if (rs_fetch<false>(A, cam, b, f, T, unusable)) {
            const rs_i64 npx = rs_box_pixels(T.box);
            if (npx > RS_LANE_MAX) {
                big[w][atomicAdd(&nbig[w], 1)] = f;             // (at most one entry per lane: 64 per wave)
            } else if (npx > 0) {
                for (int py = T.box.y0; py <= T.box.y1; ++py)
                    for (int px = T.box.x0; px <= T.box.x1; ++px) rs_plot(T, f, px, py, vis, A.W);
            }
        } else if (unusable && A.dropped) {
            atomicAdd(&A.dropped[b], 1);
        }
    }
    __syncthreads();
    // the large triangles of this wavefront, every lane on each of them
    const int n = nbig[w];
    for (int k = 0; k < n; ++k) {
        const int fb = big[w][k];
        if (!rs_fetch<false>(A, cam, b, fb, T, unusable)) continue;     // (it was drawable when it was listed)
        const int bw = T.box.x1 - T.box.x0 + 1;
        const int total = (int)rs_box_pixels(T.box);                    // <= H * W < 2^31
        for (int i = lane; i < total; i += 64) rs_plot(T, fb, T.box.x0 + i % bw, T.box.y0 + i / bw, vis, A.W);
    }
}

__global__ __launch_bounds__(RS_THREADS)
void k_rs_resolve(const RasterArgs A, int b0) {
    const int HW = A.H * A.W, pix = blockIdx.x * RS_THREADS + threadIdx.x, b = b0 + blockIdx.y;
    if (pix >= HW) return;
    const size_t o = (size_t)b * HW + pix;
    const unsigned long long key = A.vis[o];
    unsigned char* rgba = A.rgba ? A.rgba + o * 4 : nullptr;
    const int f = (int)(unsigned)(key & 0xffffffffull), px = pix % A.W, py = pix / A.W;
    if (key == RS_EMPTY || (unsigned)f >= (unsigned)A.F) {
        if (rgba) {
            uchar4 c = make_uchar4(0, 0, 0, 0);
            if (A.background) { const unsigned char* g = A.background + o * 3; c.x = g[0]; c.y = g[1]; c.z = g[2]; }
            *reinterpret_cast<uchar4*>(rgba) = c;
        }
        if (A.depth) A.depth[o] = __int_as_float(0x7f800000);
        if (A.tri) A.tri[o] = -1;
        return;
    }
    if (A.tri) A.tri[o] = f;
    if (A.depth) A.depth[o] = __uint_as_float((unsigned)(key >> 32));
    if (!rgba) return;
    const RsCam cam = rs_load_cam(A, b);
    RsFace T;
    bool unusable;
    rs_i64 e[3];
    float lam[3];
    rs_fetch<true>(A, cam, b, f, T, unusable);          // drawable: it won this pixel
    rs_covers(T.t, px, py, e);
    const float d = rs_depth(T, e, lam);
    float n[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < 3; ++i) {
        const float bi = lam[i] * d / T.p[i][2];
        const float* vn = A.vnormal + ((size_t)b * A.V + T.vi[i]) * 3;
        for (int c = 0; c < 3; ++c) { n[c] += bi * vn[c]; p[c] += bi * T.p[i][c]; }
    }
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const float inv = len > 0.f ? 1.0f / len : 0.f;
    for (int c = 0; c < 3; ++c) n[c] *= inv;
    if (n[0] * p[0] + n[1] * p[1] + n[2] * p[2] > 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }      // towards the camera
    float s = 0.f;
    for (int l = 0; l < A.n_lights; ++l)
        s += A.light_int[l] * fmaxf(0.f, n[0] * A.light_dir[l][0] + n[1] * A.light_dir[l][1] + n[2] * A.light_dir[l][2]);
    const float shade = fminf(1.f, s * 0.318309886183790672f);
    unsigned char c8[3];
    for (int c = 0; c < 3; ++c) c8[c] = (unsigned char)floorf(255.f * fminf(1.f, fmaxf(0.f, A.base[c] * shade)) + 0.5f);
    *reinterpret_cast<uchar4*>(rgba) = make_uchar4(c8[0], c8[1], c8[2], 255);
}

// one stage of the pipeline for the meshes b0 .. b0 + nb - 1 (nb <= RS_GRID_Y); host/render.hip runs them in order after the clear
void launch_raster_stage(const RasterArgs& A, int stage, int b0, int nb, hipStream_t s) {
    const int gv = (A.V + RS_THREADS - 1) / RS_THREADS, gf = (A.F + RS_THREADS - 1) / RS_THREADS;
    const int gp = (int)(((size_t)A.H * A.W + RS_THREADS - 1) / RS_THREADS);
    switch (stage) {
    case RS_STAGE_PROJECT:  hipLaunchKernelGGL(k_rs_project, dim3(gv, nb), dim3(RS_THREADS), 0, s, A, b0); break;
    case RS_STAGE_VNORMALS: hipLaunchKernelGGL(k_rs_vnormals, dim3(gv, nb), dim3(RS_THREADS), 0, s, A, b0); break;
    case RS_STAGE_COVER:    hipLaunchKernelGGL(k_rs_cover, dim3(gf, nb), dim3(RS_THREADS), 0, s, A, b0); break;
    case RS_STAGE_RESOLVE:  hipLaunchKernelGGL(k_rs_resolve, dim3(gp, nb), dim3(RS_THREADS), 0, s, A, b0); break;
    }
}
