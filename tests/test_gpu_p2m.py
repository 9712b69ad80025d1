"""GPU tests of the point-to-triangle term: sfx_p2m_forward / sfx_p2m_backward (csrc/p2m.hip) through engine.point_mesh_eval,
engine.point_mesh_backward and pointcloud.PointToMeshLoss, against the numpy oracle of tests/p2m_common.py.

Exact comparisons (bit for bit): nearest face, squared distance and barycentrics against the float32 oracle; the gradient rows
against the oracle's restatement of the device's float64 order; one mesh in any batch; one call and the next.
Float comparisons: the formulas of the contract in float64 numpy AT THE FACES THE DEVICE RETURNED are the reference, the same
formulas in float32 numpy the yardstick: |device - f64| <= max(10 x |f32 - f64|, 2^-22 x max|f64|) (p2m_common.bound).  Faces
are not compared across precisions: float32 and float64 disagree on some nearest faces (printed).
Shapes: the forward kernel holds 512 points per workgroup and stages 256 faces per LDS tile, so each size minus one, exact and
plus one, more than one tile either way, and the smallest there are (p2m_common.SHAPES)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chamfer_common as CC
import helpers as H
import p2m_common as PC
from smplifyx_amd import _capi, engine, pointcloud

pytestmark = pytest.mark.gpu

KINDS = dict(grid=PC.grid_case, soup=PC.soup_case)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    return torch.device("cuda:0")


def cuda(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(bits(x), bits(y))


def device_eval(p, v, faces, mp=None, mf=None, w=None, rho=0.0):
    out = engine.point_mesh_eval(cuda(p), cuda(v), faces, cuda(mp, torch.bool), cuda(w), cuda(mf, torch.bool), rho)
    return {k: host(t) for k, t in out.items()}


def device_grad(p, v, faces, fwd, g, mp=None, w=None, rho=0.0, want=("points", "vertices")):
    f = dict(face=cuda(fwd["face"], torch.int32))
    dp, dv = engine.point_mesh_backward(cuda(p), cuda(v), faces, f, cuda(g), want, cuda(mp, torch.bool), cuda(w), rho)
    return (None if dp is None else host(dp)), (None if dv is None else host(dv))


@functools.lru_cache(maxsize=None)
def exact_reference(kind, B, Np, F, masked=False):
    """The float32 oracle of one seeded case, computed once: face, dist2, bary."""
    p, v, faces = KINDS[kind](B, Np, F)
    mp = mf = None
    if masked:
        mp, mf, _ = PC.masks_and_weights(B, Np, F)
    return PC.nearest_face_batch(p, v, faces, mp, mf)


def assert_exact(out, ref):
    assert np.array_equal(out["face"], ref[0])
    assert same_bits(out["dist2"], ref[1]) and same_bits(out["bary"], ref[2])


# ---- 1. face, squared distance and barycentrics, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Np,F", PC.SHAPES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_face_distance_and_barycentrics_are_the_oracles(gpu, kind, Np, F, B):
    p, v, faces = KINDS[kind](B, Np, F)
    out = device_eval(p, v, faces)
    assert_exact(out, exact_reference(kind, B, Np, F))
    assert np.array_equal(out["valid"], np.full(B, Np, np.int32))
    assert kind == "soup" or (out["face"] >= 0).all()         # (a soup's random faces may be degenerate: NaN, never nearer)
    mp, mf, w = PC.masks_and_weights(B, Np, F)
    masked = device_eval(p, v, faces, mp, mf, w)
    assert_exact(masked, exact_reference(kind, B, Np, F, True))
    assert np.array_equal(masked["valid"], mp.sum(1).astype(np.int32))
    shared = device_eval(p, v, faces, None, mf[0])            # a face mask [F] serves the whole batch
    ref = PC.nearest_face_batch(p, v, faces, None, np.tile(mf[0], (B, 1)))
    assert_exact(shared, ref)


def test_ties_go_to_the_lowest_face(gpu):
    """Neighbouring triangles share edges and vertices, so a point nearest to one of those has the same float32 distance to
    several faces; on the integer lattice most points do."""
    p, v, faces = PC.grid_case(1, 3000, 1012)
    tied = PC.tied(p[0], v[0], faces)
    assert tied > 100, tied
    assert_exact(device_eval(p, v, faces), PC.nearest_face_batch(p, v, faces))
    lp, lv, lfaces = PC.lattice_case()
    ltied = PC.tied(lp[0], lv[0], lfaces)
    assert ltied > 200, ltied
    assert_exact(device_eval(lp, lv, lfaces), PC.nearest_face_batch(lp, lv, lfaces))
    print("tied float32 minima: grid %d of 3000 points, lattice %d of %d" % (tied, ltied, lp.shape[1]))


# ---- 2. loss and gradients against float64 --------------------------------------------------------------------------------------
def check_against_float64(label, p, v, faces, out, grads, g, w, rho):
    for k in range(len(p)):
        wk = None if w is None else w[k]
        ref = PC.term(p[k], v[k], faces, out["face"][k], wk, g[k], rho, np.float64)
        f32 = PC.term(p[k], v[k], faces, out["face"][k], wk, g[k], rho, np.float32)
        H.check_bound(label, "loss", abs(float(out["loss"][k]) - ref[0]), PC.bound(f32[0], ref[0]))
        for name, got, r, f in (("dp", grads[0], ref[1], f32[1]), ("dv", grads[1], ref[2], f32[2])):
            H.check_bound(label, name, np.abs(got[k].astype(np.float64) - r).max(), PC.bound(f, r))


@pytest.mark.parametrize("with_masks_and_weights", [False, True])
@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("Np,F", PC.SHAPES)
def test_loss_and_gradients_against_float64(gpu, Np, F, robust, with_masks_and_weights):
    B = 3
    for kind in sorted(KINDS):
        p, v, faces = KINDS[kind](B, Np, F)
        ref = exact_reference(kind, B, Np, F)
        rho = float(np.float32(np.sqrt(np.median(ref[1])))) if robust else 0.0
        mp = mf = w = None
        if with_masks_and_weights:
            mp, mf, w = PC.masks_and_weights(B, Np, F)
        g = np.random.RandomState(Np).uniform(0.5, 1.5, size=B).astype(np.float32)
        out = device_eval(p, v, faces, mp, mf, w, rho)
        grads = device_grad(p, v, faces, out, g, mp, w, rho)
        label = "p2m %s rho %s %s" % (kind, "> 0" if robust else "= 0", "masked, weighted" if with_masks_and_weights else "plain")
        check_against_float64(label, p, v, faces, out, grads, g, w, rho)
        if robust and Np > 3:                                 # both regimes of rho occur
            s = out["dist2"][out["face"] >= 0]
            assert (s > rho * rho).any() and (s[s > 0] < rho * rho).any()
        if not with_masks_and_weights and not robust:
            f64 = PC.nearest_face_batch(p.astype(np.float64), v.astype(np.float64), faces)
            print("%s Np %d F %d: largest |s32 - s64| %.2e, %d of %d faces differ between float32 and float64"
                  % (kind, Np, F, np.abs(out["dist2"] - f64[1]).max(), int((out["face"] != f64[0]).sum()), out["face"].size))


# ---- 3. gradient rows in the device's own order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.0, 0.01])
def test_gradient_rows_in_the_devices_own_order(gpu, rho):
    """Every row of dp and dv, bit for bit (p2m_common.rows_exact restates csrc/p2m_math.h over csrc/chamfer_math.h), with a
    point mask, a face mask and weights.  Then the two meshes of p2m_common.long_list_case: a wave of vertex rows that holds two
    long lists beside short lists and empty rows, and a partly filled wave with one more (chamfer_common.LONG_LIST_ROWS)."""
    Np, F = 513, 257
    p, v, faces = PC.grid_case(1, Np, F)
    mp, mf, w = PC.masks_and_weights(1, Np, F)
    g = np.float32([0.75])
    out = device_eval(p, v, faces, mp, mf, w, rho)
    dp, dv = device_grad(p, v, faces, out, g, mp, w, rho)
    rp, rv = PC.rows_exact(p[0], v[0], faces, out["face"][0], mp[0], w[0], g[0], rho)
    assert same_bits(dp[0], rp) and same_bits(dv[0], rv)
    assert np.abs(dv).max() > 0 and np.all(bits(dp[0][~mp[0]]) == 0)
    only_p = device_grad(p, v, faces, out, g, mp, w, rho, want=("points",))
    only_v = device_grad(p, v, faces, out, g, mp, w, rho, want=("vertices",))
    assert only_p[1] is None and only_v[0] is None and same_bits(only_p[0], dp) and same_bits(only_v[1], dv)
    p, v, faces, face, counts = PC.long_list_case()
    w = PC.masks_and_weights(2, p.shape[1], len(faces))[2]
    g = np.float32([0.75, 1.5])
    dp, dv = device_grad(p, v, faces, dict(face=face), g, None, w, rho)
    for m in range(2):
        assert all(counts[m][r] == c for r, c in CC.LONG_LIST_ROWS[m].items())
        rp, rv = PC.rows_exact(p[m], v[m], faces, face[m], None, w[m], g[m], rho)
        assert same_bits(dp[m], rp) and same_bits(dv[m], rv)


def test_a_vertex_that_collects_more_than_2048_entries(gpu):
    """A fan of 24 faces around vertex 0 with 2 049 points above it: every point's face names vertex 0, so its row sums 2 049
    corner entries -- the long-list path (64 segments).  Equal to the oracle's restatement of that order bit for bit, and from
    call to call; the plain ascending sum is printed beside it."""
    rng = np.random.RandomState(9)
    n, Np = 24, 2049
    ang = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0, 0, 0]], np.stack([0.05 * np.cos(ang), 0.05 * np.sin(ang), np.zeros(n)], 1)])[None].astype(np.float32)
    faces = np.int32([(0, 1 + i, 1 + (i + 1) % n) for i in range(n)])
    p = (np.array([0, 0, 0.03]) + 0.01 * rng.normal(size=(1, Np, 3))).astype(np.float32)
    g = np.float32([1.0])
    for rho in (0.0, 0.05):
        out = device_eval(p, v, faces, rho=rho)
        assert (out["face"] >= 0).all()
        dp, dv = device_grad(p, v, faces, out, g, rho=rho)
        dp2, dv2 = device_grad(p, v, faces, device_eval(p, v, faces, rho=rho), g, rho=rho)
        assert same_bits(dp, dp2) and same_bits(dv, dv2)
        rp, rv = PC.rows_exact(p[0], v[0], faces, out["face"][0], None, None, 1.0, rho)
        assert same_bits(dp[0], rp) and same_bits(dv[0], rv)
        plain = PC.rows_exact(p[0], v[0], faces, out["face"][0], None, None, 1.0, rho, sequential=True)[1]
        print("rho %g: row of vertex 0 %s, as one ascending sum %s" % (rho, dv[0, 0].tolist(), plain[0].tolist()))
        assert np.abs(dv[0, 0]).max() > 0


# ---- 4. sentinels ---------------------------------------------------------------------------------------------------------------------
def test_sentinels_of_the_contract(gpu):
    Np, F = 513, 257
    p, v, faces = PC.grid_case(3, Np, F)
    plain = device_eval(p, v, faces)
    # a masked point: face -1, distance 0, barycentrics 0, value 0, gradient 0
    mp = np.ones((3, Np), bool)
    mp[:, ::3] = False
    out = device_eval(p, v, faces, mp)
    assert np.all(out["face"][~mp] == -1) and np.all(bits(out["dist2"][~mp]) == 0) and np.all(bits(out["bary"][~mp]) == 0)
    assert np.array_equal(out["face"][mp], plain["face"][mp]) and (out["loss"] < plain["loss"]).all()
    g = np.ones(3, np.float32)
    dp, dv = device_grad(p, v, faces, out, g, mp)
    assert np.all(bits(dp[~mp]) == 0) and np.abs(dp[mp]).max() > 0
    # the masked call equals the call on the compacted cloud, bit for bit
    sub = device_eval(p[1:2][:, mp[1]], v[1:2], faces)
    assert same_bits(sub["loss"], out["loss"][1:2]) and same_bits(sub["dist2"][0], out["dist2"][1][mp[1]])
    # no candidate face at all in mesh 1: every face -1, loss 0, gradients 0; the other meshes keep their bits
    mf = np.ones((3, F), bool)
    mf[1] = False
    out = device_eval(p, v, faces, None, mf)
    assert np.all(out["face"][1] == -1) and bits(out["loss"])[1] == 0 and np.all(bits(out["dist2"][1]) == 0)
    assert out["valid"].tolist() == [Np] * 3
    for k in (0, 2):
        assert same_bits(out["loss"][k:k + 1], plain["loss"][k:k + 1]) and np.array_equal(out["face"][k], plain["face"][k])
    dp, dv = device_grad(p, v, faces, out, g)
    assert np.all(bits(dp[1]) == 0) and np.all(bits(dv[1]) == 0)
    # one NaN coordinate in a point of mesh 2: nothing is nearer than +inf -- face -1, distance NaN, that mesh's loss NaN,
    # gradient rows 0; everything else keeps its bits
    bad = p.copy()
    bad[2, 77, 1] = np.nan
    out = device_eval(bad, v, faces)
    assert out["face"][2, 77] == -1 and np.isnan(out["dist2"][2, 77]) and np.isnan(out["bary"][2, 77]).all() and np.isnan(out["loss"][2])
    assert same_bits(out["loss"][:2], plain["loss"][:2]) and np.array_equal(np.delete(out["face"][2], 77), np.delete(plain["face"][2], 77))
    dp, dv = device_grad(bad, v, faces, out, g)
    assert np.all(dp[2, 77] == 0) and np.isfinite(dp).all() and np.isfinite(dv).all()
    # a NaN vertex: its faces are never nearer than anything, the others still serve
    vbad = v.copy()
    vbad[0, faces[5, 0]] = np.nan
    out = device_eval(p, vbad, faces)
    touched = (faces == faces[5, 0]).any(1)
    assert np.isfinite(out["loss"]).all() and not touched[out["face"][0]].any() and (out["face"][0] >= 0).all()
    assert_exact(out, PC.nearest_face_batch(p, vbad, faces))


# ---- 5. batch independence, reproducibility, autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Np,F", [(513, 257), (1025, 513)])
def test_a_mesh_does_not_depend_on_its_batch_and_runs_repeat(gpu, Np, F):
    p, v, faces = PC.soup_case(3, Np, F)
    mp, mf, w = PC.masks_and_weights(3, Np, F)
    g = np.float32([1.0, 0.25, 1.5])
    rho = 0.01
    whole = device_eval(p, v, faces, mp, mf, w, rho)
    grads = device_grad(p, v, faces, whole, g, mp, w, rho)
    again = device_eval(p, v, faces, mp, mf, w, rho)
    grads2 = device_grad(p, v, faces, again, g, mp, w, rho)
    for k in whole:
        assert same_bits(whole[k], again[k]), k
    assert same_bits(grads[0], grads2[0]) and same_bits(grads[1], grads2[1])
    for k in range(3):
        s = slice(k, k + 1)
        alone = device_eval(p[s], v[s], faces, mp[s], mf[s], w[s], rho)
        for name in whole:
            assert same_bits(whole[name][s], alone[name]), (name, k)
        dp, dv = device_grad(p[s], v[s], faces, alone, g[s], mp[s], w[s], rho)
        assert same_bits(grads[0][s], dp) and same_bits(grads[1][s], dv), k


def test_autograd_is_the_engine_call(gpu):
    Np, F = 513, 257
    p, v, faces = PC.grid_case(3, Np, F)
    mp, mf, w = PC.masks_and_weights(3, Np, F)
    rho = 0.01
    ft = torch.as_tensor(faces)
    args = (cuda(mp, torch.bool), cuda(w), cuda(mf, torch.bool))
    fwd = engine.point_mesh_eval(cuda(p), cuda(v), ft, *args, rho)
    up = torch.tensor([2.0, 0.5, 1.0], device=gpu)
    vt, pt = cuda(v).requires_grad_(), cuda(p).requires_grad_()
    module = pointcloud.PointToMeshLoss(ft, rho, reduction="sum")
    loss = module(vt, pt, *args)
    assert tuple(loss.shape) == (3,) and torch.equal(loss.detach(), fwd["loss"])
    (loss * up).sum().backward()
    dp, dv = engine.point_mesh_backward(cuda(p), cuda(v), ft, fwd, up, ("points", "vertices"), args[0], args[1], rho)
    assert torch.equal(pt.grad, dp) and torch.equal(vt.grad, dv)
    # only the input that needs a gradient gets one; the mean divides by the valid points
    vt, pt = cuda(v).requires_grad_(), cuda(p)
    mean = pointcloud.PointToMeshLoss(ft, rho)(vt, pt, *args)
    assert torch.equal(mean, fwd["loss"] / fwd["valid"].clamp(min=1).to(torch.float32))
    mean.sum().backward()
    assert vt.grad is not None and pt.grad is None
    # float64 containers: values and gradients come back in float64, holding the float32 results
    v64, p64 = cuda(v, torch.float64).requires_grad_(), cuda(p, torch.float64).requires_grad_()
    l64 = module(v64, p64, *args)
    assert l64.dtype == torch.float64 and torch.equal(l64, fwd["loss"].double())
    (l64 * up.double()).sum().backward()
    assert v64.grad.dtype == torch.float64 and torch.equal(v64.grad, dv.double()) and torch.equal(p64.grad, dp.double())
    with pytest.raises(RuntimeError, match="first derivatives only"):
        module(cuda(v).requires_grad_(), cuda(p)).sum().backward(create_graph=True)


# ---- 6. resolution: the reason for the term ---------------------------------------------------------------------------------------------
def _body(synth_model, gpu, B):
    from smplifyx_amd import smplx, utils as U
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False)
    bm = smplx.create(synth_model, joint_mapper=U.JointMapper(H.joint_map_for(cfg)), num_betas=cfg["num_betas"],
                      num_expression_coeffs=cfg["num_expression_coeffs"], num_pca_comps=cfg["num_pca_comps"],
                      use_face_contour=cfg["use_face_contour"], create_body_pose=True, batch_size=B, differentiable=True).to(gpu)
    return bm, cfg


def test_points_on_the_surface_have_no_distance_to_it_but_a_distance_to_its_vertices(gpu, synth_model):
    """2 048 noise-free points inside the faces of the synthetic model at random parameters.  Point-to-triangle: what is left is
    the float32 rounding of the sampled coordinates, ~1e-7 m, squared -- below 1e-10 m^2 with margin.  Point-to-vertex (ChamferLoss
    column 1): the vertex spacing, squared -- above 1e-7 m^2.  The numpy oracle on the template gave 4.7e-16 and 8.9e-5."""
    B = 2
    bm, cfg = _body(synth_model, gpu, B)
    rng = np.random.RandomState(21)
    P = H.random_params(rng, B, scale=0.3, npca=cfg["num_pca_comps"])
    bm.reset_params(global_orient=P["global_orient"], body_pose=P["pose_embedding"], betas=P["betas"])
    with torch.no_grad():
        verts = bm().vertices.contiguous()
    faces = PC.synthetic_faces()
    pts = np.stack([PC.sample_on_faces(rng, host(verts[k]), faces, 2048)[0] for k in range(B)]).astype(np.float32)
    surface = pointcloud.PointToMeshLoss(faces)(verts, cuda(pts))
    vertex = pointcloud.ChamferLoss()(verts, cuda(pts))[:, 1]
    print("mean squared distance of points sampled on the surface: point-to-triangle %s m^2, point-to-vertex %s m^2"
          % (host(surface).tolist(), host(vertex).tolist()))
    assert (surface < 1e-10).all() and (vertex > 1e-7).all()


# ---- 7. a fit ------------------------------------------------------------------------------------------------------------------------------
def _closest_torch(p, a, b, c):
    """The contract's closest point in torch ops, differentiable (every unselected quotient gets a denominator of 1)."""
    dot = lambda x, y: (x * y).sum(-1)
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    r = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
         (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    first, taken = [], torch.zeros_like(r[0])
    for cond in r:
        first.append(cond & ~taken)
        taken = taken | cond
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    safe = lambda num, den, m: torch.where(m, num, zero) / torch.where(m, den, one)
    v3, w5, w6 = safe(d1, d1 - d3, first[2]), safe(d2, d2 - d6, first[4]), safe(d4 - d3, (d4 - d3) + (d5 - d6), first[5])
    den = safe(one, (va + vb) + vc, ~taken)
    v = torch.where(first[1], one, zero) + v3 + torch.where(first[5], 1 - w6, zero) + torch.where(~taken, vb * den, zero)
    w = torch.where(first[3], one, zero) + w5 + w6 + torch.where(~taken, vc * den, zero)
    d = p - (a + v[..., None] * ab + w[..., None] * ac)
    return dot(d, d)


def test_a_fit_to_a_partial_cloud_by_the_per_sample_optimiser(gpu, synth_model):
    """B = 2 on the synthetic model: differentiable SMPL-X + a torch translation + PointToMeshLoss over faces[:4096], driven by
    LBFGS(per_sample=True).  The cloud: 512 points sampled inside those faces at other parameters plus 2 mm of noise; frame 1
    keeps the half with y > 0.  At the entry point loss and parameter gradients agree, within the float32 yardstick, with the
    same closure whose term is torch float64 ops doing their own brute force over the 4 096 faces; after the step every frame's
    loss is strictly below its entry loss."""
    from smplifyx_amd.optimizers.lbfgs_ls import LBFGS
    B, NP, NF, rho = 2, 512, 4096, 0.05
    bm, cfg = _body(synth_model, gpu, B)
    rng = np.random.RandomState(4)
    P = H.random_params(rng, B, scale=0.3, npca=cfg["num_pca_comps"])
    start = dict(global_orient=P["global_orient"], body_pose=P["pose_embedding"], betas=P["betas"])
    bm.reset_params(**start)
    faces = PC.synthetic_faces()[:NF]
    ft = torch.as_tensor(faces.astype(np.int64), device=gpu)
    with torch.no_grad():
        tgt = bm(global_orient=torch.tensor(P["global_orient"] + 0.1, device=gpu),
                 body_pose=torch.tensor(P["pose_embedding"] * 0.5, device=gpu)).vertices
    pts = np.stack([PC.sample_on_faces(rng, host(tgt[k]), faces, NP)[0] for k in range(B)])
    cloud = cuda(pts + [0.02, -0.01, 0.03] + 0.002 * rng.normal(size=pts.shape)).contiguous()
    seen = torch.ones(B, NP, dtype=torch.bool, device=gpu)
    seen[1] = cloud[1, :, 1] > 0                              # frame 1: a partial observation
    assert 0.2 * NP < int(seen[1].sum()) < 0.8 * NP
    transl = torch.zeros(B, 3, device=gpu, requires_grad=True)
    params = [bm.global_orient, bm.body_pose, bm.betas, transl]
    module = pointcloud.PointToMeshLoss(ft, rho, reduction="sum")

    def device_term(v):
        return module(v, cloud, point_mask=seen)

    def torch_term(v, dtype=torch.float32):
        v, p = v.to(dtype), cloud.to(dtype)
        tri = v[:, ft]                                        # [B, F, 3, 3]
        with torch.no_grad():                                 # its own brute force: the nearest face of every point
            s_all = _closest_torch(p[:, :, None, :], tri[:, None, :, 0], tri[:, None, :, 1], tri[:, None, :, 2])
            idx = torch.where(torch.isnan(s_all), torch.full_like(s_all, float("inf")), s_all).min(2).indices
        near = torch.gather(tri, 1, idx[..., None, None].expand(-1, -1, 3, 3))
        s = _closest_torch(p, near[:, :, 0], near[:, :, 1], near[:, :, 2])
        r2 = rho * rho
        return (r2 * s / (s + r2) * seen.to(dtype)).sum(1)

    v0 = bm().vertices + transl[:, None, :]                   # the three terms on ONE forward of the model

    def entry(term):
        per = term(v0)
        grads = torch.autograd.grad(per.sum(), params, retain_graph=True)
        return per.detach().double().cpu().numpy(), [g.double().cpu().numpy().reshape(B, -1) for g in grads]

    l_dev, g_dev = entry(device_term)
    l_64, g_64 = entry(lambda v: torch_term(v, torch.float64).to(torch.float32))
    l_32, g_32 = entry(torch_term)
    print("entry loss per frame: device %s, torch float64 %s, torch float32 %s" % (l_dev.tolist(), l_64.tolist(), l_32.tolist()))
    for k in range(B):
        H.check_bound("p2m fit entry", "loss", abs(l_dev[k] - l_64[k]), PC.bound(l_32[k], l_64[k]))
        for name, gd, g6, g3 in zip(("global_orient", "body_pose", "betas", "transl"), g_dev, g_64, g_32):
            H.check_bound("p2m fit entry", "d " + name, np.abs(gd[k] - g6[k]).max(), PC.bound(g3[k], g6[k]))

    bm.reset_params(**start)
    with torch.no_grad():
        transl.zero_()
        before = device_term(bm().vertices + transl[:, None, :]).clone()

    def closure():
        for q in params:
            q.grad = None
        per = device_term(bm().vertices + transl[:, None, :])
        per.sum().backward()
        return per
    first = LBFGS(params, line_search_fn="strong_Wolfe", per_sample=True, lr=1.0, max_iter=10).step(closure)
    with torch.no_grad():
        after = device_term(bm().vertices + transl[:, None, :])
    assert tuple(first.shape) == (B,) and torch.equal(first, before), (first, before)
    assert (after < first).all(), (first, after)
    print("p2m fit, loss after / before one LBFGS step of 10 iterations, per frame: %s" % np.round(host(after / before), 4).tolist())


# ---- 8. the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_library_refuses_without_launching_and_skips_faces_that_name_no_vertex(gpu):
    lib = _capi.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert lib.sfx_p2m_forward(0, 5, 5, 2, *[None] * 6, 0.0, *[None] * 6, 0, None) == 0
    assert lib.sfx_p2m_backward(0, 5, 5, 2, *[None] * 5, 0.0, *[None] * 5, 0, None) == 0
    x = cuda(np.zeros((1, 5, 3)))
    faces = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32, device=gpu)
    face = torch.full((1, 5), 7, dtype=torch.int32, device=gpu)
    loss = torch.full((1,), 7.0, device=gpu)
    d = torch.full((1, 5, 3), 7.0, device=gpu)
    scratch = torch.zeros(1024, dtype=torch.int32, device=gpu)
    nf, nb = engine.p2m_forward_scratch_bytes(1, 5, 5), engine.p2m_backward_scratch_bytes(1, 5, 5)

    def fwd(B=1, Np=5, Nv=5, F=2, p=ptr(x), rho=0.0, sc=ptr(scratch), n=nf, fc=ptr(faces)):
        return lib.sfx_p2m_forward(B, Np, Nv, F, p, ptr(x), fc, None, None, None, rho, ptr(face), None, None, ptr(loss), None, sc, n, None)

    def bwd(B=1, Np=5, Nv=5, F=2, p=ptr(x), rho=0.0, sc=ptr(scratch), n=nb, fc=ptr(faces), g=ptr(loss)):
        return lib.sfx_p2m_backward(B, Np, Nv, F, p, ptr(x), fc, None, None, rho, ptr(face), g, ptr(d), ptr(d), sc, n, None)
    for call, name in ((fwd, b"sfx_p2m_forward"), (bwd, b"sfx_p2m_backward")):
        for kw in (dict(p=None), dict(fc=None), dict(Np=0), dict(Nv=0), dict(F=0), dict(Np=(1 << 26) + 1), dict(rho=-0.5),
                   dict(rho=float("nan")), dict(sc=None), dict(n=(nf if call is fwd else nb) - 1), dict(B=-1)):
            assert call(**kw) == -1, (name, kw)
            assert name in lib.sfx_last_error(), (name, kw, lib.sfx_last_error())
    assert bwd(g=None) == -1 and b"sfx_p2m_backward" in lib.sfx_last_error()
    torch.cuda.synchronize()
    assert torch.all(face == 7) and torch.all(loss == 7.0) and torch.all(d == 7.0)      # nothing was written
    # a face that names a vertex outside 0 .. Nv - 1 is no candidate (the engine refuses such faces; the library skips them)
    p, v, good = PC.grid_case(1, 64, 9)
    bad = good.copy()
    bad[::2, 1] = v.shape[1]
    bad[1, 2] = -1
    ok = PC.candidates(bad, v.shape[1])
    assert ok.any() and not ok.all()
    pt, vt, bt = cuda(p), cuda(v), cuda(bad, torch.int32)
    of, ob, os_ = torch.empty(1, 64, dtype=torch.int32, device=gpu), torch.empty(1, 64, 3, device=gpu), torch.empty(1, 64, device=gpu)
    ol = torch.empty(1, device=gpu)
    n = engine.p2m_forward_scratch_bytes(1, 64, v.shape[1])
    assert lib.sfx_p2m_forward(1, 64, v.shape[1], 9, ptr(pt), ptr(vt), ptr(bt), None, None, None, 0.0, ptr(of), ptr(ob), ptr(os_),
                               ptr(ol), None, ptr(scratch), n, None) == 0
    ref = PC.nearest_face_batch(p, v, bad)
    assert np.array_equal(host(of), ref[0]) and same_bits(host(os_), ref[1]) and same_bits(host(ob), ref[2])
    assert ok[host(of)[0]].all()
    # backward at a face that names no vertex, or outside 0 .. F - 1: no term, nothing read out of bounds
    assert ok[3] and not ok[0]
    given = torch.tensor([[3, 0, 9, -1] * 16], dtype=torch.int32, device=gpu)
    dp, dv = torch.empty(1, 64, 3, device=gpu), torch.empty(1, v.shape[1], 3, device=gpu)
    nbk = engine.p2m_backward_scratch_bytes(1, 64, v.shape[1])
    big = torch.zeros(nbk // 4, dtype=torch.int32, device=gpu)
    up = torch.ones(1, device=gpu)
    assert lib.sfx_p2m_backward(1, 64, v.shape[1], 9, ptr(pt), ptr(vt), ptr(bt), None, None, 0.0, ptr(given), ptr(up),
                                ptr(dp), ptr(dv), ptr(big), nbk, None) == 0
    rp, rv = PC.rows_exact(p[0], v[0], bad, host(given)[0], None, None, 1.0, 0.0)
    assert same_bits(host(dp)[0], rp) and same_bits(host(dv)[0], rv)
    assert np.all(np.abs(host(dp)[0][0::4]).max(1) > 0) and np.all(bits(host(dp)[0][np.arange(64) % 4 != 0]) == 0)
