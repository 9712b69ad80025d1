"""The numpy oracle of the point-to-triangle term's contract (include/sfx.h, sfx_p2m_forward / sfx_p2m_backward; csrc/p2m.hip,
csrc/p2m_math.h), the meshes and clouds the tests run it on and the yardstick of their float comparisons.  Plain numpy: nothing
of the package beyond the synthetic model's faces, nothing of the reference tree.

Exact parts (bit for bit): the closest point of a triangle in the dtype of the inputs (closest: the contract's region test with
np.select over the conditions in order), the nearest face with the lowest index of a tie (nearest_face), and, in rows_exact,
the gradient rows in the device's own float64 order.
Float parts: loss and gradients by the formulas of the contract in a dtype of the caller's choice at GIVEN face indices; a test
evaluates them in float64 (the reference) and in float32 (the yardstick): bound = chamfer_common.bound."""
import functools

import numpy as np

import chamfer_common as CC

bound = CC.bound
QUERIES, TILE = 512, 256        # points per workgroup (P2M_THREADS x P2M_QPT) and faces per LDS tile (P2M_TILE) of csrc/p2m.hip
SHAPES = ((1, 1), (3, 2), (QUERIES - 1, TILE - 1), (QUERIES, TILE), (QUERIES + 1, TILE + 1), (2 * QUERIES + 1, 2 * TILE + 1),
          (2 * TILE + 1, QUERIES + 1))          # (Np, F)


# ---- the closest point of a triangle ----------------------------------------------------------------------------------------------
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _parts(p, a, b, c):
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    return ab, ac, (d1, d2, d3, d4, d5, d6), (va, vb, vc), conds


def region(p, a, b, c):
    """1 .. 7: the condition of the contract that decides (7: the face's interior, and whatever a NaN leaves)."""
    with np.errstate(all="ignore"):
        conds = _parts(p, a, b, c)[4]
    return np.select(conds, [1, 2, 3, 4, 5, 6], 7)


def closest(p, a, b, c):
    """(s, u, v, w, q) of the contract for arrays [..., 3] of one dtype, in that dtype."""
    assert p.dtype == a.dtype == b.dtype == c.dtype
    with np.errstate(all="ignore"):
        ab, ac, (d1, d2, d3, d4, d5, d6), (va, vb, vc), conds = _parts(p, a, b, c)
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        den = one / ((va + vb) + vc)
        w6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, one - w6], vb * den)
        w = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), w6], vc * den)
        u = (one - v) - w
        q = (a + v[..., None] * ab) + w[..., None] * ac
        d = p - q
        s = _dot(d, d)
    assert s.dtype == p.dtype and u.dtype == p.dtype
    return s, u, v, w, q


# ---- exact: the nearest face --------------------------------------------------------------------------------------------------------
def candidates(faces, Nv, mf=None):
    ok = ((faces >= 0) & (faces < Nv)).all(1)
    return ok if mf is None else ok & np.asarray(mf, bool)


def nearest_face(p, v, faces, mp=None, mf=None):
    """One mesh: (face int32 [Np], s [Np], bary [Np, 3]) in the dtype of p, brute force.  -1 / 0 / 0 at a masked point and when
    no face is a candidate; -1 / NaN / NaN where candidates exist and none is nearer than +inf.  A NaN counts as +inf; the first
    of equal minima wins."""
    Np = len(p)
    mp = np.ones(Np, bool) if mp is None else np.asarray(mp, bool)
    cand = candidates(faces, len(v), mf)
    face, s, bary = np.full(Np, -1, np.int32), np.zeros(Np, p.dtype), np.zeros((Np, 3), p.dtype)
    if not cand.any():
        return face, s, bary
    f = np.where(cand[:, None], faces, 0)
    tri = v[f]                                                  # [F, 3, 3]
    d, u, vv, w, _ = closest(p[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
    d = d.copy()
    d[:, ~cand] = np.inf
    d[np.isnan(d)] = np.inf
    j = np.argmin(d, 1)                                         # the first of equal minima
    rows = np.arange(Np)
    m = d[rows, j]
    found = m < np.inf
    face[:] = np.where(found, j, -1)
    s[:] = np.where(found, m, np.nan)
    bary[:] = np.where(found[:, None], np.stack([u[rows, j], vv[rows, j], w[rows, j]], 1), np.nan)
    face[~mp] = -1
    s[~mp] = 0
    bary[~mp] = 0
    return face, s, bary


def tied(p, v, faces):
    """How many points of one mesh have more than one face at their minimum (in the dtype of p)."""
    tri = v[faces]
    d = closest(p[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])[0]
    d = np.where(np.isnan(d), np.inf, d)
    return int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())


def nearest_face_batch(p, v, faces, mp=None, mf=None):
    out = [nearest_face(p[k], v[k], faces, None if mp is None else mp[k], None if mf is None else mf[k]) for k in range(len(p))]
    return [np.stack(o) for o in zip(*out)]


# ---- the formulas of the contract in a chosen dtype, at given faces ----------------------------------------------------------------
def term(p, v, faces, face, w, g, rho, dtype):
    """One mesh in `dtype`: (loss, dp [Np, 3], dv [Nv, 3]) at the given faces (-1: no term)."""
    p, v = p.astype(dtype), v.astype(dtype)
    ok = face >= 0
    tri = v[faces[np.where(ok, face, 0)]]
    s, u, vv, ww, q = closest(p, tri[:, 0], tri[:, 1], tri[:, 2])
    w = np.ones(len(p), dtype) if w is None else w.astype(dtype)
    val = np.where(ok, w * CC.rho_fn(s, rho), 0).astype(dtype)
    coef = np.where(ok, dtype(g) * w * CC.drho_fn(s, rho) * 2, 0).astype(dtype)
    dp = (coef[:, None] * (p - q)).astype(dtype)
    dv = np.zeros((len(v), 3), dtype)
    for k, bk in enumerate((u, vv, ww)):
        np.add.at(dv, faces[face[ok], k], -(bk[ok, None] * dp[ok]))
    return val.sum(dtype=dtype), dp, dv


# ---- exact: the gradient rows in the device's order -----------------------------------------------------------------------------------
def rows_exact(p, v, faces, face, mp, w, g, rho, sequential=False):
    """(dp float32 [Np, 3], dv float32 [Nv, 3]) of one mesh as sfx_p2m_backward forms them: s, q and the barycentrics in float32,
    c and the differences in float64; a vertex's row is its corner entries e = 3 i + k in ascending e, cut into segments by
    chamfer_common.seg_len (sequential: one segment whatever the length), rounded once."""
    Np, Nv, F = len(p), len(v), len(faces)
    has = (face >= 0) & (face < F)
    if mp is not None:
        has &= np.asarray(mp, bool)
    f = faces[np.where(has, face, 0)]
    has &= ((f >= 0) & (f < Nv)).all(1)
    f = np.where(has[:, None], f, 0)
    s, u, vv, ww, q = closest(p, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    assert s.dtype == np.float32
    wt = np.ones(Np, np.float32) if w is None else w
    coef = np.array([CC._coef(g, wt[i], s[i], rho) for i in range(Np)])
    diff = p.astype(np.float64) - q.astype(np.float64)
    dp = np.where(has[:, None], coef[:, None] * diff, 0.0).astype(np.float32)
    bary = np.stack([u, vv, ww], 1).astype(np.float64)
    corner = np.where(has[:, None], f, Nv).reshape(-1)          # entry e = 3 i + k
    order = np.argsort(corner, kind="stable")
    starts = np.searchsorted(corner[order], np.arange(Nv + 1))
    dv = np.zeros((Nv, 3), np.float32)
    for r in range(Nv):
        lst = order[starts[r]:starts[r + 1]]
        row = np.zeros(3)
        if len(lst):
            step = len(lst) if sequential else CC.seg_len(len(lst))
            for k0 in range(0, len(lst), step):
                acc = np.zeros(3)
                for e in lst[k0:k0 + step]:
                    i, k = divmod(int(e), 3)
                    acc = acc + -((coef[i] * bary[i, k]) * diff[i])
                row = row + acc
        dv[r] = row.astype(np.float32)
    return dp, dv


# ---- meshes and clouds ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_mesh(F):
    """(vertices float32 [Nv, 3], faces int32 [F, 3]): the first F triangles of a bumpy height field, 1 cm spacing,
    z = 0.004 sin(0.9 x) cos(0.7 y) with x, y in grid units."""
    n = int(np.ceil(np.sqrt((F + 1) // 2))) + 1                 # n x n cells of two triangles
    ix, iy = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    z = 0.004 * np.sin(0.9 * ix) * np.cos(0.7 * iy)
    v = np.stack([0.01 * ix, 0.01 * iy, z], -1).reshape(-1, 3).astype(np.float32)
    vid = lambda i, j: i * (n + 1) + j
    faces = []
    for i in range(n):
        for j in range(n):
            faces.append((vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)))
            faces.append((vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)))
    faces = np.int32(faces[:F])
    assert len(faces) == F
    return v, faces


@functools.lru_cache(maxsize=None)
def grid_case(B, Np, F, seed=0):
    """B copies of grid_mesh(F), each moved a little, and points scattered 1 cm about the used part of the surface."""
    rng = np.random.RandomState(3000 * seed + 7 * Np + F + B)
    v0, faces = grid_mesh(F)
    v = (v0[None] + 0.0005 * rng.normal(size=(B,) + v0.shape)).astype(np.float32)
    used = v0[np.unique(faces)]
    pick = rng.randint(0, len(used), size=(B, Np))
    p = (used[pick] + 0.01 * rng.normal(size=(B, Np, 3))).astype(np.float32)
    return p, v, faces


@functools.lru_cache(maxsize=None)
def lattice_case(Np=600, F=700, Nv=120):
    """An integer-lattice triangle soup (coordinates in -3 .. 3, float32 exact): many ties, degenerate faces included."""
    rng = np.random.RandomState(5)
    v = rng.randint(-3, 4, size=(1, Nv, 3)).astype(np.float32)
    faces = rng.randint(0, Nv, size=(F, 3)).astype(np.int32)
    faces[::50, 1] = faces[::50, 0]                             # (two corners the same vertex)
    p = rng.randint(-3, 4, size=(1, Np, 3)).astype(np.float32)
    return p, v, faces


@functools.lru_cache(maxsize=None)
def soup_case(B, Np, F, seed=0):
    """Body-scale random soup: F triangles with ~2 cm edges about centres ~ N(0, diag(.25, .5, .12)) m over Nv = 3 F // 2 + 3
    shared vertices, points 1 cm about random face centres."""
    rng = np.random.RandomState(4000 * seed + 7 * Np + F + B)
    centre = rng.normal(size=(F, 3)) * [0.25, 0.5, 0.12]
    Nv = 3 * F // 2 + 3
    faces = rng.randint(0, Nv, size=(F, 3)).astype(np.int32)
    v = np.zeros((B, Nv, 3))
    v[:] = rng.normal(size=(Nv, 3)) * [0.25, 0.5, 0.12]
    own = rng.rand(F) < 0.7                                     # most faces get corners of their own, ~2 cm apart
    k = 0
    for f in np.nonzero(own)[0]:
        if k + 3 > Nv:
            break
        faces[f] = (k, k + 1, k + 2)
        v[:, k:k + 3] = centre[f] + 0.02 * rng.normal(size=(B, 3, 3))
        k += 3
    v = v.astype(np.float32)
    pick = rng.randint(0, F, size=(B, Np))
    p = (v[np.arange(B)[:, None], faces[pick, 0]] + 0.01 * rng.normal(size=(B, Np, 3))).astype(np.float32)
    return p, v, faces


@functools.lru_cache(maxsize=None)
def long_list_case():
    """(p [2, 130, 3], v [2, 70, 3], faces [F, 3], face [2, 130], counts [2, 70]): the vertex rows of chamfer_common
    .LONG_LIST_ROWS as corner entries.  Every point of a mesh is given a face that names the mesh's 130-entry vertex; the two
    other corners of the 130 faces take the other rows with their counts, and rows 22 .. 27 of the first wave take what is left
    (17 or 18 each: short lists).  `face` is handed to the backward as the forward's result would be: the backward forms each
    point's term against the face it is given."""
    rng = np.random.RandomState(23)
    Nv, Np = CC.LONG_LIST_NROWS, 130
    tri, counts = [], np.zeros((2, Nv), int)
    for m, rows in enumerate(CC.LONG_LIST_ROWS):
        hub = [r for r, c in rows.items() if c == Np][0]
        rest = {r: c for r, c in rows.items() if r != hub}
        left = 2 * Np - sum(rest.values())
        rest.update({22 + k: left // 6 + (k < left % 6) for k in range(6)})
        slots = np.repeat(sorted(rest), [rest[r] for r in sorted(rest)])    # (no row holds 130 of them: a pair is two vertices)
        tri.append(np.stack([np.roll((hub, slots[i], slots[i + Np]), i % 3) for i in range(Np)]))
        counts[m] = np.bincount(tri[m].reshape(-1), minlength=Nv)
    faces, face = np.unique(np.concatenate(tri), axis=0, return_inverse=True)
    face = face.reshape(2, Np).astype(np.int32)
    v = (0.1 * rng.normal(size=(2, Nv, 3))).astype(np.float32)
    centre = np.stack([v[m][faces[face[m]]].mean(1) for m in range(2)])
    p = (centre + 0.02 * rng.normal(size=(2, Np, 3))).astype(np.float32)
    return p, v, faces.astype(np.int32), face, counts


def masks_and_weights(B, Np, F, seed=3):
    rng = np.random.RandomState(seed + Np + F)
    mp, mf = rng.rand(B, Np) > 0.3, rng.rand(B, F) > 0.3
    mp[:, 0] = True; mf[:, 0] = True
    return mp, mf, rng.uniform(0.2, 2.0, size=(B, Np)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def synthetic_faces():
    from smplifyx_amd import synthetic
    return np.ascontiguousarray(np.asarray(synthetic.make_synthetic_model(0)["f"], np.int64).astype(np.int32))


def sample_on_faces(rng, v, faces, n):
    """n points inside random faces of one mesh by uniform barycentrics: (points float64 [n, 3], face ids)."""
    f = rng.randint(0, len(faces), size=n)
    r1, r2 = np.sqrt(rng.rand(n)), rng.rand(n)
    bary = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], 1)
    tri = v.astype(np.float64)[faces[f]]
    return (bary[:, :, None] * tri).sum(1), f


# ---- the cases of the host check ---------------------------------------------------------------------------------------------------
def body_scale_triangles(n, seed, dtype=np.float32):
    """(p, a, b, c) [n, 3]: triangles with 0.5 - 4 cm edges at body-scale positions, the point at affine coordinates in
    -0.7 .. 1.7 of the triangle's plane (every region is hit) and up to ~2 cm off it."""
    rng = np.random.RandomState(seed)
    a = rng.normal(size=(n, 3)) * [0.25, 0.5, 0.12]
    size = rng.uniform(0.005, 0.04, size=(n, 1))
    b, c = a + size * rng.normal(size=(n, 3)), a + size * rng.normal(size=(n, 3))
    al, be = rng.uniform(-0.7, 1.7, size=(2, n, 1))
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = a + al * (b - a) + be * (c - a) + rng.normal(size=(n, 1)) * 0.01 * nrm
    return tuple(x.astype(dtype) for x in (p, a, b, c))


def lattice_triangles(n, seed):
    rng = np.random.RandomState(seed)
    return tuple(rng.randint(-3, 4, size=(n, 3)).astype(np.float32) for _ in range(4))


def special_triangles():
    """Points exactly on an edge, on a vertex and in the plane (float32-exact coordinates)."""
    a, b, c = np.float32([0, 0, 0]), np.float32([2, 0, 0]), np.float32([0, 2, 0])
    pts = [a, b, c, (a + b) / 2, (a + c) / 2, (b + c) / 2, np.float32([0.5, 0.5, 0]), np.float32([0.5, 0.25, 0]),
           np.float32([3, 3, 0]), np.float32([-1, -1, 0]), np.float32([1, -1, 0]), np.float32([-1, 1, 0]), np.float32([0.5, 0.5, 1])]
    p = np.stack(pts).astype(np.float32)
    n = len(p)
    return p, np.tile(a, (n, 1)), np.tile(b, (n, 1)), np.tile(c, (n, 1))
