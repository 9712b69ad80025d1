"""GPU tests of the chamfer term: sfx_chamfer_forward / sfx_chamfer_backward (csrc/chamfer.hip) through engine.chamfer_eval,
engine.chamfer_backward and pointcloud.ChamferLoss, against the numpy oracle of tests/chamfer_common.py.

Exact comparisons (bit for bit): nearest index and squared distance against float32 numpy; the gradient rows against the
oracle's restatement of the device's float64 order; one mesh in any batch; one call and the next.
Float comparisons: the formulas of the contract in float64 numpy AT THE INDICES THE DEVICE RETURNED are the reference, the
same formulas in float32 numpy the yardstick: |device - f64| <= max(10 x |f32 - f64|, 2^-22 x max|f64|), per mesh and
quantity (chamfer_common.bound).  Bounds and observed maxima go through helpers.check_bound into the session summary.
Shapes: the forward kernel holds 512 queries per workgroup and stages 1 024 targets per LDS tile, so each size minus one, exact
and plus one, more than one tile either way, and the smallest sets there are (chamfer_common.SHAPES)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chamfer_common as CC
import helpers as H
from smplifyx_amd import _capi, engine, pointcloud

pytestmark = pytest.mark.gpu

KINDS = dict(normal=CC.normal_clouds, body=CC.body_clouds)


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
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


def device_eval(a, b, ma=None, mb=None, wa=None, wb=None, rho=0.0):
    out = engine.chamfer_eval(cuda(a), cuda(b), cuda(ma, torch.bool), cuda(mb, torch.bool), cuda(wa), cuda(wb), rho)
    return {k: host(v) for k, v in out.items()}


def device_grad(a, b, fwd, g, ma=None, mb=None, wa=None, wb=None, rho=0.0, want=("a", "b")):
    f = dict(idx_ab=cuda(fwd["idx_ab"], torch.int32), idx_ba=cuda(fwd["idx_ba"], torch.int32))
    da, db = engine.chamfer_backward(cuda(a), cuda(b), f, cuda(g), want, cuda(ma, torch.bool), cuda(mb, torch.bool), cuda(wa), cuda(wb), rho)
    return (None if da is None else host(da)), (None if db is None else host(db))


@functools.lru_cache(maxsize=None)
def exact_reference(kind, B, Na, Nb):
    """The float32 oracle of one seeded set, computed once: idx_ab, idx_ba, dist2_ab, dist2_ba."""
    a, b = KINDS[kind](B, Na, Nb)
    return CC.nearest_batch(a, b)


def median_rho(ref):
    """rho near the median nearest distance of a set, so that points lie on both sides of the GMoF's knee."""
    return float(np.float32(np.sqrt(np.median(np.r_[ref[2].reshape(-1), ref[3].reshape(-1)]))))


# ---- 1. index and squared distance, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Na,Nb", CC.SHAPES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_index_and_squared_distance_are_numpys(gpu, kind, Na, Nb, B):
    a, b = KINDS[kind](B, Na, Nb)
    iab, iba, sab, sba = exact_reference(kind, B, Na, Nb)
    out = device_eval(a, b)
    assert np.array_equal(out["idx_ab"], iab) and np.array_equal(out["idx_ba"], iba)
    assert same_bits(out["dist2_ab"], sab) and same_bits(out["dist2_ba"], sba)
    assert np.array_equal(out["valid"], np.tile(np.int32([Na, Nb]), (B, 1)))


def test_ties_go_to_the_lowest_index(gpu):
    """An integer lattice: float32 is exact and most queries have several targets at the minimum."""
    a, b = CC.lattice_clouds()
    d = CC.dist2(a[0], b[0])
    tied = ((d == d.min(1, keepdims=True)).sum(1) > 1).sum()
    assert tied > 500, tied                                  # of 600 queries
    iab, iba, sab, sba = CC.nearest_batch(a, b)
    out = device_eval(a, b)
    assert np.array_equal(out["idx_ab"], iab) and np.array_equal(out["idx_ba"], iba)
    assert same_bits(out["dist2_ab"], sab) and same_bits(out["dist2_ba"], sba)
    print("lattice: %d of %d queries of a have a tied minimum" % (tied, a.shape[1]))


# ---- 2. loss and gradients against float64 --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def argmin_agrees_in_float64(kind, B, Na, Nb):
    """Disagreements between the float64 and the float32 argmin on a seeded set (the float64 reference is evaluated at the
    device's indices; where the two argmins agree no query is left to a tie that float32 decided)."""
    a, b = KINDS[kind](B, Na, Nb)
    i32 = exact_reference(kind, B, Na, Nb)
    i64 = CC.nearest_batch(a.astype(np.float64), b.astype(np.float64))
    return int((i32[0] != i64[0]).sum() + (i32[1] != i64[1]).sum())


def check_against_float64(label, a, b, out, grads, g, wa, wb, rho):
    B = len(a)
    for k in range(B):
        w_a, w_b = (None if wa is None else wa[k]), (None if wb is None else wb[k])
        ref = CC.term(a[k], b[k], out["idx_ab"][k], out["idx_ba"][k], w_a, w_b, g[k], rho, np.float64)
        f32 = CC.term(a[k], b[k], out["idx_ab"][k], out["idx_ba"][k], w_a, w_b, g[k], rho, np.float32)
        for d in range(2):
            H.check_bound(label, "loss", abs(float(out["loss"][k, d]) - ref[0][d]), CC.bound(f32[0][d], ref[0][d]))
        for name, got, r, f in (("da", grads[0], ref[1], f32[1]), ("db", grads[1], ref[2], f32[2])):
            H.check_bound(label, name, np.abs(got[k].astype(np.float64) - r).max(), CC.bound(f, r))


@pytest.mark.parametrize("with_masks_and_weights", [False, True])
@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("Na,Nb", CC.SHAPES)
def test_loss_and_gradients_against_float64(gpu, Na, Nb, robust, with_masks_and_weights):
    B = 3
    for kind in sorted(KINDS):
        a, b = KINDS[kind](B, Na, Nb)
        assert argmin_agrees_in_float64(kind, B, Na, Nb) == 0
        rho = median_rho(exact_reference(kind, B, Na, Nb)) if robust else 0.0
        assert (rho > 0) == robust or Na * Nb == 1
        ma = mb = wa = wb = None
        if with_masks_and_weights:
            ma, mb, wa, wb = CC.masks_and_weights(B, Na, Nb)
        g = np.random.RandomState(Na).uniform(0.5, 1.5, size=(B, 2)).astype(np.float32)
        out = device_eval(a, b, ma, mb, wa, wb, rho)
        if with_masks_and_weights:
            ref = CC.nearest_batch(a, b, ma, mb)
            assert np.array_equal(out["idx_ab"], ref[0]) and np.array_equal(out["idx_ba"], ref[1])
            assert same_bits(out["dist2_ab"], ref[2]) and same_bits(out["dist2_ba"], ref[3])
            assert np.array_equal(out["valid"], np.stack([ma.sum(1), mb.sum(1)], 1))
        grads = device_grad(a, b, out, g, ma, mb, wa, wb, rho)
        label = "chamfer %s rho %s %s" % (kind, "> 0" if robust else "= 0", "masked, weighted" if with_masks_and_weights else "plain")
        check_against_float64(label, a, b, out, grads, g, wa, wb, rho)
        if robust and Na > 2:                                 # both regimes of rho occur
            s = np.r_[out["dist2_ab"].reshape(-1), out["dist2_ba"].reshape(-1)]
            assert (s > rho * rho).any() and (s[s > 0] < rho * rho).any()


@pytest.mark.parametrize("rho", [0.0, 0.02])
def test_gradient_rows_in_the_devices_own_order(gpu, rho):
    """Every row of da and db, bit for bit: the gather term, then the row's list in ascending query index (chamfer_common
    .rows_exact restates csrc/chamfer_math.h), with masks and weights.  Then the two meshes of chamfer_common.long_list_clouds: a
    wave that holds two long lists beside short lists and empty rows, and a partly filled wave with one more (LONG_LIST_ROWS)."""
    a, b = CC.body_clouds(1, 513, 1025)
    ma, mb, wa, wb = CC.masks_and_weights(1, 513, 1025)
    g = np.float32([[0.75, 1.25]])
    out = device_eval(a, b, ma, mb, wa, wb, rho)
    da, db = device_grad(a, b, out, g, ma, mb, wa, wb, rho)
    assert same_bits(da[0], CC.rows_exact(a[0], b[0], out["idx_ab"][0], out["idx_ba"][0], wa[0], wb[0], g[0, 0], g[0, 1], rho))
    assert same_bits(db[0], CC.rows_exact(b[0], a[0], out["idx_ba"][0], out["idx_ab"][0], wb[0], wa[0], g[0, 1], g[0, 0], rho))
    only_a = device_grad(a, b, out, g, ma, mb, wa, wb, rho, want=("a",))
    only_b = device_grad(a, b, out, g, ma, mb, wa, wb, rho, want=("b",))
    assert only_a[1] is None and only_b[0] is None and same_bits(only_a[0], da) and same_bits(only_b[1], db)
    a, b, counts = CC.long_list_clouds()
    wa, wb = CC.masks_and_weights(2, a.shape[1], b.shape[1])[2:]
    g = np.float32([[0.75, 1.25], [1.5, 0.5]])
    out = device_eval(a, b, None, None, wa, wb, rho)
    da, db = device_grad(a, b, out, g, None, None, wa, wb, rho)
    for m in range(2):
        assert np.bincount(out["idx_ba"][m], minlength=a.shape[1]).tolist() == counts[m].tolist()
        assert same_bits(da[m], CC.rows_exact(a[m], b[m], out["idx_ab"][m], out["idx_ba"][m], wa[m], wb[m], g[m, 0], g[m, 1], rho))
        assert same_bits(db[m], CC.rows_exact(b[m], a[m], out["idx_ba"][m], out["idx_ab"][m], wb[m], wa[m], g[m, 1], g[m, 0], rho))


# ---- 3. masks and weights -------------------------------------------------------------------------------------------------------
def test_masked_points_are_out_and_zero_weights_still_serve_as_targets(gpu):
    Na, Nb = 513, 1025
    a, b = CC.body_clouds(3, Na, Nb)
    ma, mb, _, _ = CC.masks_and_weights(3, Na, Nb)
    out = device_eval(a, b, ma, mb)
    # a masked point is never a target and contributes exactly 0
    for idx, m_q, m_t, s in ((out["idx_ab"], ma, mb, out["dist2_ab"]), (out["idx_ba"], mb, ma, out["dist2_ba"])):
        assert np.all(idx[~m_q] == -1) and np.all(bits(s[~m_q]) == 0)
        hit = idx[m_q]
        assert np.all(hit >= 0)
        for k in range(3):
            assert m_t[k][idx[k][m_q[k]]].all()
    g = np.ones((3, 2), np.float32)
    da, db = device_grad(a, b, out, g, ma, mb)
    # a masked query has gradient 0; as nobody's target either, its whole row is +0
    assert np.all(bits(da[~ma]) == 0) and np.all(bits(db[~mb]) == 0)
    # the masked call equals the call on the compacted sets, bit for bit (one mesh)
    k = 1
    sub = device_eval(a[k:k + 1][:, ma[k]], b[k:k + 1][:, mb[k]])
    assert same_bits(sub["loss"], out["loss"][k:k + 1])
    assert same_bits(sub["dist2_ab"][0], out["dist2_ab"][k][ma[k]]) and same_bits(sub["dist2_ba"][0], out["dist2_ba"][k][mb[k]])
    # weight 0: exactly 0 as a query, unchanged as a target
    wa = np.ones((3, Na), np.float32)
    zero = np.zeros((3, Na), bool)
    zero[:, ::3] = True
    wa[zero] = 0.0
    w = device_eval(a, b, None, None, wa, None)
    plain = device_eval(a, b)
    assert np.array_equal(w["idx_ab"], plain["idx_ab"]) and np.array_equal(w["idx_ba"], plain["idx_ba"])      # still targets
    assert same_bits(w["dist2_ba"], plain["dist2_ba"]) and same_bits(w["loss"][:, 1], plain["loss"][:, 1])
    assert (w["loss"][:, 0] < plain["loss"][:, 0]).all()
    kept = device_eval(a, b, ~zero, None)                     # the same queries by a mask: the same sum of the a -> b direction
    assert same_bits(w["loss"][:, 0], kept["loss"][:, 0])
    dwa, dwb = device_grad(a, b, w, g, None, None, wa, None)
    gather_only = device_grad(a, b, w, np.float32([[1, 0]] * 3), None, None, wa, None)[0]
    assert np.all(gather_only[zero] == 0)                     # no term of its own
    assert np.isin(np.arange(Na), plain["idx_ba"][0]).any() and np.abs(dwa[zero]).max() > 0       # but the cloud still pulls on it


def test_an_all_masked_target_set_gives_zero_loss_and_a_nan_stays_in_its_mesh(gpu):
    Na, Nb = 513, 1025
    a, b = CC.body_clouds(3, Na, Nb)
    mb = np.ones((3, Nb), bool)
    mb[1] = False
    out = device_eval(a, b, None, mb)
    assert np.all(out["idx_ab"][1] == -1) and np.all(out["idx_ba"][1] == -1)
    assert np.all(bits(out["loss"][1]) == 0) and out["valid"][1].tolist() == [Na, 0]
    plain = device_eval(a, b)
    for k in (0, 2):
        assert same_bits(out["loss"][k], plain["loss"][k]) and np.array_equal(out["idx_ab"][k], plain["idx_ab"][k])
    da, db = device_grad(a, b, out, np.ones((3, 2), np.float32), None, mb)
    assert np.all(bits(da[1]) == 0) and np.all(bits(db[1]) == 0)
    # one NaN coordinate in a query of a: that mesh's a -> b loss is NaN, everything else keeps its bits
    bad = a.copy()
    bad[2, 77, 1] = np.nan
    out = device_eval(bad, b)
    assert np.isnan(out["loss"][2, 0]) and out["idx_ab"][2, 77] == -1
    assert same_bits(out["loss"][:2], plain["loss"][:2])
    assert np.array_equal(out["idx_ab"][:2], plain["idx_ab"][:2]) and np.array_equal(out["idx_ba"][:2], plain["idx_ba"][:2])
    assert np.isfinite(out["loss"][2, 1])                     # as a target the point is never nearer than anything
    da, db = device_grad(bad, b, out, np.float32([[1, 0]] * 3))
    assert np.all(da[2, 77] == 0) and np.isfinite(da).all() and np.isfinite(db).all()


# ---- 4. batch independence and reproducibility ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Na,Nb", [(513, 1025), (2049, 513)])
def test_a_mesh_does_not_depend_on_its_batch_and_runs_repeat(gpu, Na, Nb):
    a, b = CC.body_clouds(3, Na, Nb)
    ma, mb, wa, wb = CC.masks_and_weights(3, Na, Nb)
    g = np.float32([[1.0, 0.5], [0.25, 2.0], [1.5, 1.0]])
    rho = 0.02
    whole = device_eval(a, b, ma, mb, wa, wb, rho)
    grads = device_grad(a, b, whole, g, ma, mb, wa, wb, rho)
    again = device_eval(a, b, ma, mb, wa, wb, rho)
    grads2 = device_grad(a, b, again, g, ma, mb, wa, wb, rho)
    for k in whole:
        assert same_bits(whole[k], again[k]), k
    assert same_bits(grads[0], grads2[0]) and same_bits(grads[1], grads2[1])
    for k in range(3):
        s = slice(k, k + 1)
        alone = device_eval(a[s], b[s], ma[s], mb[s], wa[s], wb[s], rho)
        for name in whole:
            assert same_bits(whole[name][s], alone[name]), (name, k)
        da, db = device_grad(a[s], b[s], alone, g[s], ma[s], mb[s], wa[s], wb[s], rho)
        assert same_bits(grads[0][s], da) and same_bits(grads[1][s], db), k


def test_one_bucket_holding_every_point(gpu):
    """Every one of 2 049 cloud points is nearest to the same vertex: that vertex's row is its gather term plus 2 049 scatter
    terms -- the long-list path (64 segments).  Equal to the oracle's restatement of that order bit for bit, to the plain
    ascending float64 sum rounded once, and from call to call."""
    rng = np.random.RandomState(9)
    Na, Nb = 513, 2049
    a = (rng.normal(size=(1, Na, 3)) + [100.0, 0.0, 0.0]).astype(np.float32)
    a[0, 7] = 0.0
    b = (0.1 * rng.normal(size=(1, Nb, 3))).astype(np.float32)
    g = np.float32([[1.0, 1.0]])
    for rho in (0.0, 0.1):
        out = device_eval(a, b, rho=rho)
        assert np.all(out["idx_ba"] == 7)
        da, db = device_grad(a, b, out, g, rho=rho)
        da2, db2 = device_grad(a, b, device_eval(a, b, rho=rho), g, rho=rho)
        assert same_bits(da, da2) and same_bits(db, db2)
        segmented = CC.rows_exact(a[0], b[0], out["idx_ab"][0], out["idx_ba"][0], None, None, 1.0, 1.0, rho)
        plain = CC.rows_exact(a[0], b[0], out["idx_ab"][0], out["idx_ba"][0], None, None, 1.0, 1.0, rho, sequential=True)
        assert same_bits(da[0], segmented)
        assert same_bits(da[0], plain)
        assert same_bits(db[0], CC.rows_exact(b[0], a[0], out["idx_ba"][0], out["idx_ab"][0], None, None, 1.0, 1.0, rho))
        assert np.abs(da[0, 7]).max() > 0


# ---- 5. autograd ----------------------------------------------------------------------------------------------------------------
def test_autograd_is_the_engine_call(gpu):
    Na, Nb = 513, 1025
    a, b = CC.body_clouds(3, Na, Nb)
    ma, mb, wa, wb = CC.masks_and_weights(3, Na, Nb)
    rho = 0.02
    args = (cuda(ma, torch.bool), cuda(mb, torch.bool), cuda(wa), cuda(wb))
    fwd = engine.chamfer_eval(cuda(a), cuda(b), *args, rho)
    for col in range(2):
        v, p = cuda(a).requires_grad_(), cuda(b).requires_grad_()
        loss = pointcloud.ChamferLoss(rho, reduction="sum")(v, p, *args)
        assert tuple(loss.shape) == (3, 2) and torch.equal(loss.detach(), fwd["loss"])
        loss[:, col].sum().backward()
        unit = torch.zeros(3, 2, device=gpu)
        unit[:, col] = 1.0
        da, db = engine.chamfer_backward(cuda(a), cuda(b), fwd, unit, ("a", "b"), *args, rho)
        assert torch.equal(v.grad, da) and torch.equal(p.grad, db)
    # an upstream weight scales the unit gradient as the formula says: g enters c = ((g w) rho') 2 in float64
    up = torch.tensor([[2.0, 0.5], [1.0, 4.0], [0.25, 8.0]], device=gpu)
    v, p = cuda(a).requires_grad_(), cuda(b).requires_grad_()
    (pointcloud.ChamferLoss(rho, reduction="sum")(v, p, *args) * up).sum().backward()
    da, db = engine.chamfer_backward(cuda(a), cuda(b), fwd, up, ("a", "b"), *args, rho)
    assert torch.equal(v.grad, da) and torch.equal(p.grad, db)
    ones = engine.chamfer_backward(cuda(a), cuda(b), fwd, torch.tensor([[1.0, 0.0]] * 3, device=gpu), ("a",), *args, rho)[0]
    scaled = engine.chamfer_backward(cuda(a), cuda(b), fwd, torch.tensor([[2.0, 0.0], [1.0, 0.0], [0.25, 0.0]], device=gpu), ("a",), *args, rho)[0]
    assert torch.equal(scaled, ones * torch.tensor([2.0, 1.0, 0.25], device=gpu).reshape(3, 1, 1))      # (powers of two: exact)
    # only the input that needs a gradient gets one
    v, p = cuda(a).requires_grad_(), cuda(b)
    pointcloud.ChamferLoss(rho)(v, p)[:, 1].sum().backward()
    assert v.grad is not None and p.grad is None


def test_mean_is_sum_over_valid_and_float64_round_trips(gpu):
    Na, Nb = 513, 1025
    a, b = CC.body_clouds(3, Na, Nb)
    ma, mb, _, _ = CC.masks_and_weights(3, Na, Nb)
    ma[2] = False                                             # no valid vertex: the count is clamped to 1
    args = (cuda(ma, torch.bool), cuda(mb, torch.bool))
    fwd = engine.chamfer_eval(cuda(a), cuda(b), *args)
    total = pointcloud.ChamferLoss(reduction="sum")(cuda(a), cuda(b), *args)
    mean = pointcloud.ChamferLoss(reduction="mean")(cuda(a), cuda(b), *args)
    assert host(fwd["valid"]).tolist() == [[int(ma[k].sum()), int(mb[k].sum())] for k in range(3)]
    assert torch.equal(mean, total / fwd["valid"].clamp(min=1).to(torch.float32))
    assert torch.all(mean[2] == 0) and torch.isfinite(mean).all()
    # float64 containers: values and gradients come back in float64, holding the float32 results
    v64, p64 = cuda(a, torch.float64).requires_grad_(), cuda(b, torch.float64).requires_grad_()
    l64 = pointcloud.ChamferLoss(0.02)(v64, p64, *args)
    v32, p32 = cuda(a).requires_grad_(), cuda(b).requires_grad_()
    l32 = pointcloud.ChamferLoss(0.02)(v32, p32, *args)
    assert l64.dtype == torch.float64 and torch.equal(l64, l32.double())
    l64.sum().backward()
    l32.sum().backward()
    assert v64.grad.dtype == torch.float64 and torch.equal(v64.grad, v32.grad.double()) and torch.equal(p64.grad, p32.grad.double())


def test_second_derivatives_are_refused(gpu):
    a, b = CC.body_clouds(1, 513, 1025)
    v = cuda(a).requires_grad_()
    loss = pointcloud.ChamferLoss(0.02)(v, cuda(b)).sum()
    with pytest.raises(RuntimeError, match="first derivatives only"):
        loss.backward(create_graph=True)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
def test_a_fit_to_a_partial_cloud_by_the_per_sample_optimiser(gpu, synth_model):
    """B = 2 on the synthetic model: differentiable SMPL-X + a torch translation + ChamferLoss, driven by
    LBFGS(per_sample=True).  The cloud: 2 048 of the model's own vertices at other parameters plus 2 mm of noise; frame 1 keeps
    the half with y > 0 only and is fitted with the points -> mesh column alone.  At the entry point loss and parameter
    gradients agree with the same closure whose term is torch ops (cdist, min, gather) within the float32 yardstick; after the
    step every frame's loss is below its entry loss.  The reduction both paths reach is printed, not asserted."""
    from smplifyx_amd import smplx, utils as U
    from smplifyx_amd.optimizers.lbfgs_ls import LBFGS
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False)
    B, NP, rho = 2, 2048, 0.05
    bm = smplx.create(synth_model, joint_mapper=U.JointMapper(H.joint_map_for(cfg)), num_betas=cfg["num_betas"],
                      num_expression_coeffs=cfg["num_expression_coeffs"], num_pca_comps=cfg["num_pca_comps"],
                      use_face_contour=cfg["use_face_contour"], create_body_pose=True, batch_size=B, differentiable=True).to(gpu)
    rng = np.random.RandomState(4)
    P = H.random_params(rng, B, scale=0.3, npca=cfg["num_pca_comps"])
    start = dict(global_orient=P["global_orient"], body_pose=P["pose_embedding"], betas=P["betas"])
    bm.reset_params(**start)
    with torch.no_grad():
        tgt = bm(global_orient=torch.tensor(P["global_orient"] + 0.1, device=gpu),
                 body_pose=torch.tensor(P["pose_embedding"] * 0.5, device=gpu)).vertices
        pick = torch.as_tensor(rng.choice(tgt.shape[1], NP, replace=False), device=gpu)
        cloud = (tgt[:, pick] + torch.tensor([0.02, -0.01, 0.03], device=gpu)
                 + 0.002 * torch.as_tensor(rng.normal(size=(B, NP, 3)), dtype=torch.float32, device=gpu)).contiguous()
    seen = torch.ones(B, NP, dtype=torch.bool, device=gpu)
    seen[1] = cloud[1, :, 1] > 0                              # frame 1: a partial observation
    assert 0.2 * NP < int(seen[1].sum()) < 0.8 * NP
    col_w = torch.tensor([[1.0, 1.0], [0.0, 1.0]], device=gpu)        # frame 1: points -> mesh alone
    transl = torch.zeros(B, 3, device=gpu, requires_grad=True)
    params = [bm.global_orient, bm.body_pose, bm.betas, transl]
    chamfer = pointcloud.ChamferLoss(rho, reduction="sum")

    def device_term(v):
        return chamfer(v, cloud, point_mask=seen)

    def torch_term(v, dtype=torch.float32):
        v, p = v.to(dtype), cloud.to(dtype)
        r2 = rho * rho
        with torch.no_grad():       # the indices only; cdist in its default mode (its non-matmul mode was seen to return wrong,
            d = torch.cdist(v, p).masked_fill(~seen[:, None, :], float("inf"))      # unrepeatable distances at this size)
        cols = []
        for idx, q, t, m in ((d.min(2).indices, v, p, None), (d.min(1).indices, p, v, seen)):
            s = ((q - torch.gather(t, 1, idx[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
            val = r2 * s / (s + r2)
            cols.append((val if m is None else val * m.to(dtype)).sum(1))
        return torch.stack(cols, 1)

    def evaluate(term, v=None):
        v = bm().vertices + transl[:, None, :] if v is None else v
        return (term(v) * col_w.to(transl.dtype)).sum(1)

    # the entry point: the three terms on ONE forward of the model, so that they differ in the term alone
    v0 = bm().vertices + transl[:, None, :]

    def entry(term):
        per = evaluate(term, v0)
        grads = torch.autograd.grad(per.sum(), params, retain_graph=True)
        return per.detach().double().cpu().numpy(), [g.double().cpu().numpy().reshape(B, -1) for g in grads]

    l_dev, g_dev = entry(device_term)
    l_64, g_64 = entry(lambda v: torch_term(v, torch.float64).to(torch.float32))
    l_32, g_32 = entry(torch_term)
    print("entry loss per frame: device %s, torch float64 %s, torch float32 %s" % (l_dev.tolist(), l_64.tolist(), l_32.tolist()))
    for k in range(B):
        H.check_bound("chamfer fit entry", "loss", abs(l_dev[k] - l_64[k]), CC.bound(l_32[k], l_64[k]))
        for name, gd, g6, g3 in zip(("global_orient", "body_pose", "betas", "transl"), g_dev, g_64, g_32):
            H.check_bound("chamfer fit entry", "d " + name, np.abs(gd[k] - g6[k]).max(), CC.bound(g3[k], g6[k]))

    reached = {}
    for name, term in (("device", device_term), ("torch", torch_term)):
        bm.reset_params(**start)
        with torch.no_grad():
            transl.zero_()
            before = evaluate(term).clone()

        def closure():
            for p in params:
                p.grad = None
            per = evaluate(term)
            per.sum().backward()
            return per
        first = LBFGS(params, line_search_fn="strong_Wolfe", per_sample=True, lr=1.0, max_iter=10).step(closure)
        with torch.no_grad():
            after = evaluate(term)
        reached[name] = host(after / before)
        if name == "device":
            assert tuple(first.shape) == (B,) and torch.equal(first, before), (first, before)
            assert (after < first).all(), (first, after)
    print("chamfer fit, loss after / before one LBFGS step of 10 iterations, per frame: device %s, torch %s"
          % (np.round(reached["device"], 4).tolist(), np.round(reached["torch"], 4).tolist()))


# ---- 7. the C ABI's refusals ------------------------------------------------------------------------------------------------------
def test_library_refuses_without_launching(gpu):
    lib = _capi.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.sfx_chamfer_forward(0, 5, 5, None, None, *[None] * 4, 0.0, *[None] * 7, 0, None) == 0
    assert lib.sfx_chamfer_backward(0, 5, 5, None, None, *[None] * 4, 0.0, *[None] * 6, 0, None) == 0
    x = cuda(np.zeros((1, 5, 3)))
    idx = torch.full((1, 5), 7, dtype=torch.int32, device=gpu)
    loss = torch.full((1, 2), 7.0, device=gpu)
    d = torch.full((1, 5, 3), 7.0, device=gpu)
    scratch = torch.zeros(1024, dtype=torch.int32, device=gpu)
    nf, nb = engine.chamfer_forward_scratch_bytes(1, 5, 5), engine.chamfer_backward_scratch_bytes(1, 5, 5)

    def fwd(B=1, Na=5, Nb=5, a=p(x), rho=0.0, sc=p(scratch), n=nf):
        return lib.sfx_chamfer_forward(B, Na, Nb, a, p(x), None, None, None, None, rho, p(idx), p(idx), None, None, p(loss), None, sc, n, None)

    def bwd(B=1, Na=5, Nb=5, a=p(x), rho=0.0, sc=p(scratch), n=nb, g=p(loss)):
        return lib.sfx_chamfer_backward(B, Na, Nb, a, p(x), None, None, None, None, rho, p(idx), p(idx), g, p(d), p(d), sc, n, None)
    for call, name in ((fwd, b"sfx_chamfer_forward"), (bwd, b"sfx_chamfer_backward")):
        for kw in (dict(a=None), dict(Na=0), dict(Nb=(1 << 26) + 1), dict(rho=-0.5), dict(rho=float("nan")), dict(sc=None),
                   dict(n=(nf if call is fwd else nb) - 1), dict(B=-1)):
            assert call(**kw) == -1, (name, kw)
            assert name in lib.sfx_last_error(), (name, kw, lib.sfx_last_error())
    assert bwd(g=None) == -1 and b"sfx_chamfer_backward" in lib.sfx_last_error()
    torch.cuda.synchronize()
    assert torch.all(idx == 7) and torch.all(loss == 7.0) and torch.all(d == 7.0)      # nothing was written
