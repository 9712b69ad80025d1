// raster_fixed.h -- the integer half of the mesh rasteriser (csrc/raster.hip, sfx_render_meshes), for the host and the device: no
// HIP runtime call, no global state.  Everything that decides WHICH pixels a triangle covers lives here and is integer, so
// coverage is exact: the host check (tests/raster_fixed_check.cpp) and the device agree with a numpy int64 oracle bit for bit.
//
//   snap        a screen position in pixels -> int32 in 1/256 pixel, rint(x * 256).  x * 256 is exact in float32; positions are
//               bounded by RS_MAX_PX = 2^20 pixels (rs_usable), so the snapped value stays inside +-2^28.
//   orientation area2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) of the snapped corners.  0: the triangle covers nothing.  Negative:
//               every edge function and every edge direction is negated, which is the triangle with its winding reversed -- both
//               windings are drawn, and the three edge values keep belonging to the corners 0, 1, 2 the caller numbered.
//   edge        edge i runs from corner (i + 1) % 3 to corner (i + 2) % 3 (opposite corner i):
//               e_i(p) = dx_i (p_y - y_j) - dy_i (p_x - x_j), evaluated at pixel centres p = (256 i + 128, 256 j + 128).
//               e_0 + e_1 + e_2 = area2 at every p; the differences stay below 2^29, every product below 2^58.
//   fill rule   p is covered when every e_i > 0, or e_i = 0 on a top or left edge (y down: top is dy = 0, dx > 0; left is
//               dy < 0).  Of an edge shared by two triangles exactly one side owns the pixel centres on it.
//   box         the pixels whose centres lie inside the corners' bounding box, clipped to the image.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_HD __host__ __device__ inline
#else
#include <math.h>
#define RS_HD inline
#endif

#define RS_SUB 256                      // sub-pixel positions per pixel
#define RS_HALF 128                     // a pixel centre
#define RS_MAX_PX 1048576.0f            // 2^20: a vertex further out than this (either axis) is unusable
#define RS_UNUSABLE INT32_MIN           // snapped x of an unusable vertex

typedef long long rs_i64;

// A projected vertex can take part in coverage: in front of the near plane, finite, inside +-RS_MAX_PX.  (Written so that a NaN
// anywhere fails.)
RS_HD bool rs_usable(float x, float y, float z, float znear) {
    return z >= znear && z <= 3.0e38f && fabsf(x) <= RS_MAX_PX && fabsf(y) <= RS_MAX_PX;
}

RS_HD int32_t rs_snap(float x) { return (int32_t)rintf(x * (float)RS_SUB); }

struct RsTri {
    int32_t xj[3], yj[3];               // start corner of edge i
    int32_t dx[3], dy[3];               // its direction, already negated for a negative area2
    rs_i64 area2;                       // > 0 after orientation; 0: nothing to draw
    int32_t sign;                       // +1 / -1: what the edge values are multiplied by
};

// Corners (x[i], y[i]) in 1/256 pixel, |.| <= 2^28.
RS_HD RsTri rs_setup(const int32_t x[3], const int32_t y[3]) {
    RsTri t;
    const rs_i64 a = (rs_i64)(x[1] - x[0]) * (rs_i64)(y[2] - y[0]) - (rs_i64)(y[1] - y[0]) * (rs_i64)(x[2] - x[0]);
    t.sign = a < 0 ? -1 : 1;
    t.area2 = a < 0 ? -a : a;
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        t.xj[i] = x[j]; t.yj[i] = y[j];
        t.dx[i] = t.sign * (x[k] - x[j]); t.dy[i] = t.sign * (y[k] - y[j]);
    }
    return t;
}

// e_i at the centre of pixel (px, py); px, py must lie inside the triangle's box (rs_box), which bounds the differences.
RS_HD rs_i64 rs_edge(const RsTri& t, int i, int32_t px, int32_t py) {
    const int32_t cx = px * RS_SUB + RS_HALF, cy = py * RS_SUB + RS_HALF;
    return (rs_i64)t.dx[i] * (rs_i64)(cy - t.yj[i]) - (rs_i64)t.dy[i] * (rs_i64)(cx - t.xj[i]);
}

RS_HD bool rs_top_left(const RsTri& t, int i) { return t.dy[i] < 0 || (t.dy[i] == 0 && t.dx[i] > 0); }

// The three edge values at pixel (px, py) and whether its centre is covered.
RS_HD bool rs_covers(const RsTri& t, int32_t px, int32_t py, rs_i64 e[3]) {
    bool in = true;
    for (int i = 0; i < 3; ++i) {
        e[i] = rs_edge(t, i, px, py);
        in = in && (e[i] > 0 || (e[i] == 0 && rs_top_left(t, i)));
    }
    return in;
}

struct RsBox { int32_t x0, y0, x1, y1; };      // pixels x0 .. x1, y0 .. y1 inclusive; empty when x1 < x0 or y1 < y0

// Pixels whose centres 256 i + 128 lie in [min, max] of the corners, clipped to W x H.  (v >> 8 is the floor of v / 256 for
// negative v as well: arithmetic shift.)
RS_HD RsBox rs_box(const int32_t x[3], const int32_t y[3], int32_t W, int32_t H) {
    int32_t xmin = x[0], xmax = x[0], ymin = y[0], ymax = y[0];
    for (int i = 1; i < 3; ++i) {
        xmin = x[i] < xmin ? x[i] : xmin; xmax = x[i] > xmax ? x[i] : xmax;
        ymin = y[i] < ymin ? y[i] : ymin; ymax = y[i] > ymax ? y[i] : ymax;
    }
    RsBox b;
    b.x0 = (xmin - RS_HALF + RS_SUB - 1) >> 8; b.x1 = (xmax - RS_HALF) >> 8;
    b.y0 = (ymin - RS_HALF + RS_SUB - 1) >> 8; b.y1 = (ymax - RS_HALF) >> 8;
    b.x0 = b.x0 < 0 ? 0 : b.x0; b.y0 = b.y0 < 0 ? 0 : b.y0;
    b.x1 = b.x1 > W - 1 ? W - 1 : b.x1; b.y1 = b.y1 > H - 1 ? H - 1 : b.y1;
    return b;
}

// pixels of a box (0 when empty); a box never holds more than W * H < 2^31
RS_HD rs_i64 rs_box_pixels(const RsBox& b) {
    return (b.x1 < b.x0 || b.y1 < b.y0) ? 0 : (rs_i64)(b.x1 - b.x0 + 1) * (rs_i64)(b.y1 - b.y0 + 1);
}
