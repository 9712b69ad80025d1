"""The numpy oracle of the mesh rasteriser's contract (include/sfx.h, sfx_render_meshes; csrc/raster.hip, csrc/raster_fixed.h),
float64 for everything that is float on the device and int64 / Python integers for everything that is integer there, written
independently of the C code: whole boxes at a time, floor division instead of shifts, no shared helper.

  project            p_c = R p + t, x = X / Z fx + cx, y = Y / Z fy + cy in a chosen dtype
  snap               float32 screen positions -> 1/256 pixel (rint), and which vertices are usable
  triangle_coverage  the int64 edge functions of one triangle over a block of pixels, the top-left fill rule, both windings
  coverage_mask      the pixels of an image one triangle covers, by brute force over the WHOLE image (no bounding box)
  rasterize          every triangle of a mesh: hits per pixel, the nearest triangle, its depth and barycentrics, the second-nearest
                     depth (for the near-tie test), the same depth formula in float32 (for the tolerance), dropped triangles
  vertex_normals     smooth normals in camera space from the usable faces
  shade              the colour of every covered pixel
  icosphere          a subdivided icosahedron (2 subdivisions: 162 vertices, 320 faces), a closed manifold
Shared by tests/test_raster_fixed_host.py (CPU) and tests/test_gpu_render.py."""
import numpy as np

SUB, HALF = 256, 128
MAX_PX = 2.0 ** 20
BASE_RGB = (0.4, 0.4, 0.7)
LIGHTS = tuple(((0.5 * np.cos(phi), -0.5 * np.sin(phi), -np.cos(np.pi / 6.0)), 1.0)
               for phi in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0)) + (((0.0, 0.0, -1.0), 1.0),)


def icosphere(subdivisions=2, radius=1.0):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.stack(v) * radius, np.asarray(f, np.int64)


def camera_points(verts, t, R=None, dtype=np.float64):
    verts = np.asarray(verts, dtype)
    R = np.eye(3, dtype=dtype) if R is None else np.asarray(R, dtype)
    t = np.asarray(t, dtype)
    # (the sum order of the device: R0 x + R1 y + R2 z + t -- immaterial in float64, the float32 twin is the error yardstick)
    return ((R[None, :, 0] * verts[:, 0:1] + R[None, :, 1] * verts[:, 1:2]) + R[None, :, 2] * verts[:, 2:3]) + t[None]


def project(verts, t, focal, center, R=None, dtype=np.float64):
    """screen [V, 3] = (x, y, Z) of the fit camera in `dtype`."""
    pc = camera_points(verts, t, R, dtype)
    f, c = np.asarray(focal, dtype).reshape(2), np.asarray(center, dtype).reshape(2)
    with np.errstate(all="ignore"):
        x = pc[:, 0] / pc[:, 2] * f[0] + c[0]
        y = pc[:, 1] / pc[:, 2] * f[1] + c[1]
    return np.stack([x, y, pc[:, 2]], 1).astype(dtype)


def snap(screen, znear=0.05):
    """(sx, sy int64 [V] in 1/256 pixel, usable bool [V]) of float32 screen positions."""
    s = np.asarray(screen, np.float32)
    with np.errstate(all="ignore"):
        usable = np.isfinite(s).all(1) & (s[:, 2] >= np.float32(znear)) & (np.abs(s[:, 0]) <= MAX_PX) & (np.abs(s[:, 1]) <= MAX_PX)
        q = np.rint(np.where(usable[:, None], s[:, :2], 0).astype(np.float32) * np.float32(SUB))
    return q[:, 0].astype(np.int64), q[:, 1].astype(np.int64), usable


def triangle_coverage(x, y, px, py):
    """One triangle with snapped corners x[3], y[3] (Python integers) over the pixels px [w] x py [h] (int64 arrays).
    Returns (area2 > 0, e [3][h, w] int64 oriented edge values with e[i] opposite corner i, inside [h, w]); None for zero area."""
    x, y = [int(a) for a in x], [int(a) for a in y]
    area2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if area2 == 0:
        return None
    sgn = 1 if area2 > 0 else -1
    cx = (np.asarray(px, np.int64) * SUB + HALF)[None, :]
    cy = (np.asarray(py, np.int64) * SUB + HALF)[:, None]
    inside = np.ones((cy.shape[0], cx.shape[1]), bool)
    e = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        dx, dy = sgn * (x[k] - x[j]), sgn * (y[k] - y[j])
        ei = dx * (cy - y[j]) - dy * (cx - x[j])
        top_left = dy < 0 or (dy == 0 and dx > 0)       # y down: a left edge runs upwards, a top edge to the right
        inside &= (ei > 0) | ((ei == 0) & top_left)
        e.append(ei)
    return sgn * area2, e, inside


def coverage_mask(x, y, H, W):
    """bool [H, W]: the pixel centres one triangle covers, every pixel of the image tested."""
    r = triangle_coverage(x, y, np.arange(W), np.arange(H))
    return np.zeros((H, W), bool) if r is None else r[2]


def pixel_box(x, y, H, W):
    """(x0, y0, x1, y1) inclusive: pixels whose centres lie in the corners' bounding box, clipped to the image."""
    x0 = max(0, -((-(min(x) - HALF)) // SUB)); x1 = min(W - 1, (max(x) - HALF) // SUB)
    y0 = max(0, -((-(min(y) - HALF)) // SUB)); y1 = min(H - 1, (max(y) - HALF) // SUB)
    return int(x0), int(y0), int(x1), int(y1)


def rasterize(screen, faces, H, W, znear=0.05):
    """A mesh from its float32 screen positions [V, 3].  Returns a dict of [H, W] arrays:
    hits (triangles covering the pixel), tri (the nearest, -1: none; equal float64 depths go to the lowest id), depth (float64,
    inf: none), second (the nearest depth among the OTHER triangles covering the pixel, inf: none), depth32 (the nearest
    triangle's depth by the same formula in float32 numpy), lam [H, W, 3] (its e_i / area2); and dropped (triangles with an
    unusable vertex)."""
    screen = np.asarray(screen, np.float32)
    faces = np.asarray(faces, np.int64)
    sx, sy, usable = snap(screen, znear)
    Z = screen[:, 2].astype(np.float64)
    out = dict(hits=np.zeros((H, W), np.int32), tri=np.full((H, W), -1, np.int64), depth=np.full((H, W), np.inf),
               second=np.full((H, W), np.inf), depth32=np.full((H, W), np.inf, np.float32), lam=np.zeros((H, W, 3)), dropped=0)
    for f, (a, b, c) in enumerate(faces):
        if not (usable[a] and usable[b] and usable[c]):
            out["dropped"] += 1
            continue
        x, y = [int(sx[a]), int(sx[b]), int(sx[c])], [int(sy[a]), int(sy[b]), int(sy[c])]
        x0, y0, x1, y1 = pixel_box(x, y, H, W)
        if x1 < x0 or y1 < y0:
            continue
        r = triangle_coverage(x, y, np.arange(x0, x1 + 1), np.arange(y0, y1 + 1))
        if r is None or not r[2].any():
            continue
        area2, e, inside = r
        lam = [ei / float(area2) for ei in e]
        z = [Z[a], Z[b], Z[c]]
        d = 1.0 / (lam[0] / z[0] + lam[1] / z[1] + lam[2] / z[2])
        a32 = np.float32(area2)
        l32 = [ei.astype(np.float32) / a32 for ei in e]
        d32 = np.float32(1.0) / (l32[0] / screen[a, 2] + l32[1] / screen[b, 2] + l32[2] / screen[c, 2])
        sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        out["hits"][sl] += inside
        best, second = out["depth"][sl], out["second"][sl]
        wins = inside & (d < best)                      # (ascending f: an equal depth keeps the earlier triangle)
        loses = inside & ~wins
        second[wins] = best[wins]
        second[loses] = np.minimum(second[loses], d[loses])
        best[wins] = d[wins]
        out["tri"][sl][wins] = f
        out["depth32"][sl][wins] = d32[wins]
        for i in range(3):
            out["lam"][sl][..., i][wins] = lam[i][wins]
    return out


def vertex_normals(cam_pts, faces, usable=None):
    """Unit normals [V, 3]: the un-normalised cross products of every vertex's faces summed (faces with an unusable vertex left
    out), normalised; 0 where the sum is 0."""
    p, faces = np.asarray(cam_pts, np.float64), np.asarray(faces, np.int64)
    keep = np.ones(len(faces), bool) if usable is None else np.asarray(usable)[faces].all(1)
    with np.errstate(all="ignore"):
        fn = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    fn[~keep] = 0.0
    n = np.zeros_like(p)
    for i in range(3):
        np.add.at(n, faces[:, i], fn)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0)


def shade(ras, cam_pts, faces, usable=None, base_rgb=BASE_RGB, lights=LIGHTS):
    """uint8 [H, W, 3] mesh colour of every covered pixel of `ras` (0 elsewhere), from float64 camera-space points."""
    p, faces = np.asarray(cam_pts, np.float64), np.asarray(faces, np.int64)
    vn = vertex_normals(p, faces, usable)
    tri = ras["tri"]
    cov = tri >= 0
    f = faces[tri[cov]]                                 # [n, 3]
    lam, depth = ras["lam"][cov], ras["depth"][cov]
    bary = lam * depth[:, None] / p[f][:, :, 2]         # [n, 3]
    n = (bary[:, :, None] * vn[f]).sum(1)
    pos = (bary[:, :, None] * p[f]).sum(1)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0)
    n = np.where(((n * pos).sum(1) > 0)[:, None], -n, n)
    s = np.zeros(len(n))
    for d, inten in lights:
        s += inten * np.maximum(0.0, n @ np.asarray(d, np.float64))
    sh = np.minimum(1.0, s / np.pi)
    col = np.clip(np.asarray(base_rgb, np.float64)[None] * sh[:, None], 0.0, 1.0)
    img = np.zeros(tri.shape + (3,), np.uint8)
    img[cov] = np.floor(255.0 * col + 0.5).astype(np.uint8)
    return img
