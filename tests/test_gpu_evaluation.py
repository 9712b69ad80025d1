"""GPU tests of the device evaluation: sfx_eval_align / sfx_eval_nearest (csrc/evaluate.hip) through engine.align_errors,
engine.nearest_distances and evaluation.compute_v2v(device=True), against this package's numpy evaluation code.

The yardstick of every float comparison: the numpy code runs on the float32-rounded inputs once in float32 and once in float64;
the device is compared with the float64 result and must stay within  max(10 x max|f32 - f64|, 2^-22 x max|coordinate|).  The
bound is formed from the reference side only; observed maxima go through helpers.check_bound into the session summary.
The reference always gets its points as columns ([3, N]): evaluation._cols takes a [N, 3] array with N = 2 or 3 for columns."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers as H
from smplifyx_amd import _capi, engine, evaluation as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "evaluation.npz"))
MODES = ("none", "procrustes", "scale", "pelvis")
MIRROR = np.array([1.0, 1.0, -1.0], np.float32)
SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1025)        # 4: coplanar; the wave (64), workgroup (1024) and query-tile (256) edges


def cuda(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---- the reference side -------------------------------------------------------------------------------------------------
def numpy_errors(mode, est, gt, anchors=(2, 3)):
    """[N] errors of one mesh by evaluation.py's own code, in the dtype of the inputs ([N, 3])."""
    if mode == "none":
        return E.mpjpe(est, gt)
    if mode == "pelvis":
        gt_al, est_al = E.PelvisAlignment(list(anchors))(gt, est)
        return E.mpjpe(est_al, gt_al)
    align = E.ProcrustesAlignment() if mode == "procrustes" else E.ScaleAlignment()
    return E.vertex_to_vertex_error(align(est.T, gt.T).T, gt)


def numpy_xform(mode, est, gt, anchors=(2, 3)):
    """[13] scale, R, t of the map applied to the estimate (include/sfx.h), restating evaluation.py's lines in the inputs' dtype."""
    scale, R, t = np.ones((), est.dtype), np.eye(3, dtype=est.dtype), np.zeros(3, est.dtype)
    mu1, mu2 = est.mean(0), gt.mean(0)
    X1, X2 = (est - mu1).T, (gt - mu2).T
    if mode == "procrustes":
        K = X1 @ X2.T
        U, _, Vh = np.linalg.svd(K)
        Z = np.eye(3)
        Z[-1, -1] *= np.sign(np.linalg.det(U @ Vh))
        R = Vh.T @ Z @ U.T
        scale = np.trace(R @ K) / np.sum(X1 ** 2)
        t = mu2 - scale * (R @ mu1)
    elif mode == "scale":
        scale = np.sqrt(np.sum(X2 ** 2) / np.sum(X1 ** 2))
        t = mu2 - scale * mu1
    elif mode == "pelvis":
        t = -est[list(anchors)].mean(0)
    return np.concatenate([np.reshape(scale, 1), np.reshape(R, 9), t]).astype(np.float64)


def bound_of(ref32, ref64, coord):
    return max(10.0 * float(np.max(np.abs(np.asarray(ref32, np.float64) - ref64))), 2.0 ** -22 * float(coord))


def check_mesh(label, mode, est, gt, err, mean, xform, anchors=(2, 3)):
    """One mesh of a device result (numpy [N], scalar, [13]) against the float64 reference on est / gt (float32 [N, 3])."""
    e64, g64 = est.astype(np.float64), gt.astype(np.float64)
    coord = max(np.abs(est).max(), np.abs(gt).max())
    r64, r32 = numpy_errors(mode, e64, g64, anchors), numpy_errors(mode, est, gt, anchors)
    H.check_bound(label, mode + " err", np.abs(err - r64).max(), bound_of(r32, r64, coord))
    H.check_bound(label, mode + " mean", abs(float(mean) - r64.mean()), bound_of(r32.mean(), r64.mean(), coord))
    if xform is not None:
        x64, x32 = numpy_xform(mode, e64, g64, anchors), numpy_xform(mode, est, gt, anchors)
        H.check_bound(label, mode + " xform", np.abs(xform - x64).max(), bound_of(x32, x64, coord))


def run_modes(label, est, gt, modes=MODES, anchors=(2, 3)):
    """est, gt: float32 [B, N, 3]; every mode in one batched call each, every mesh checked."""
    out = {}
    for mode in modes:
        err, mean, xf = engine.align_errors(cuda(est), cuda(gt), mode=mode, anchors=anchors, return_transform=True)
        assert err.shape == est.shape[:2] and mean.shape == est.shape[:1] and xf.shape == (est.shape[0], 13)
        assert err.is_cuda and err.dtype == torch.float32
        err, mean, xf = host(err), host(mean), host(xf)
        for b in range(est.shape[0]):
            check_mesh(label, mode, est[b], gt[b], err[b], mean[b], xf[b], anchors)
        out[mode] = (err, mean, xf)
    return out


def random_rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def synthetic_pair(N, seed, coplanar=False):
    """gt ~ N(0, 1) + (0.3, -1.2, 2.5); est = 1.7 R gt + t + 0.02 noise (coplanar: both sets in a plane); float32 [N, 3]."""
    rng = np.random.RandomState(seed)
    gt, noise = rng.normal(size=(N, 3)), rng.normal(size=(N, 3))
    if coplanar:
        gt[:, 2] = 0.0
        noise[:, 2] = 0.0
    R = random_rotation(rng)
    est = 1.7 * (gt + np.array([0.3, -1.2, 2.5]) + 0.02 / 1.7 * noise) @ R.T + rng.normal(size=3)
    return est.astype(np.float32), (gt + np.array([0.3, -1.2, 2.5])).astype(np.float32)


def brute_nearest(a, b):
    """Distance of every point of a to the nearest point of b, by coordinate differences, in the inputs' dtype."""
    d = a[:, None, :] - b[None, :, :]
    return np.sqrt((d * d).sum(-1).min(1))


def host_fscore(pred, gt, thresh):
    """evaluation.point_fscore with the brute-force distances (the k-d tree's package may be absent)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    gt_to_pred, pred_to_gt = brute_nearest(gt, pred), brute_nearest(pred, gt)
    recall = (pred_to_gt < thresh).sum() / len(pred_to_gt)
    precision = (gt_to_pred < thresh).sum() / len(gt_to_pred)
    f = 2 * recall * precision / (recall + precision) if recall + precision > 0.0 else 0.0
    return {"fscore": f, "precision": precision, "recall": recall}


def assert_margin(dist, thresholds, rel=1e-3):
    """A condition on the INPUTS: no float64 nearest distance within `rel` (relative) of a threshold, so that float32
    distances must give the same counts."""
    for t in thresholds:
        gap = np.abs(np.asarray(dist) / t - 1.0).min()
        assert gap > rel, (t, gap)


# ---- alignment -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["j", "v"])
def test_golden_sets_all_modes(tag):
    est, gt = G[tag + "_est"].astype(np.float32), G[tag + "_gt"].astype(np.float32)
    out = run_modes("eval golden " + tag, np.stack([est, est * MIRROR]), np.stack([gt, gt]))
    # the reflection branch: the mirrored estimate still gets a proper rotation
    for b in range(2):
        R = out["procrustes"][2][b, 1:10].reshape(3, 3).astype(np.float64)
        assert abs(np.linalg.det(R) - 1.0) <= 1e-6, (b, np.linalg.det(R))


@pytest.mark.parametrize("N", SIZES)
def test_synthetic_sizes_plain_and_mirrored(N):
    est, gt = synthetic_pair(N, 100 + N, coplanar=(N == 4))
    out = run_modes("eval synthetic", np.stack([est, est * MIRROR]), np.stack([gt, gt]), anchors=(0, 2))
    for b in range(2):
        R = out["procrustes"][2][b, 1:10].reshape(3, 3).astype(np.float64)
        assert abs(np.linalg.det(R) - 1.0) <= 1e-6
    # Procrustes recovers the similarity up to the injected noise
    assert out["procrustes"][1][0] < 0.1 and abs(out["procrustes"][2][0, 0] - 1.0 / 1.7) < 0.05


@pytest.mark.parametrize("N", [1, 2])
def test_degenerate_sizes_return_and_are_finite_where_the_reference_is(N):
    est, gt = synthetic_pair(N, 7 + N)
    for mode in MODES:
        anchors = tuple(range(N))
        err, mean, xf = engine.align_errors(cuda(est[None]), cuda(gt[None]), mode=mode, anchors=anchors, return_transform=True)
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            ref = numpy_errors(mode, est.astype(np.float64), gt.astype(np.float64), anchors)
        assert np.array_equal(np.isfinite(host(err)[0]), np.isfinite(ref)), (mode, host(err), ref)
        assert bool(np.isfinite(host(mean)[0])) == bool(np.isfinite(ref).all()), (mode, host(mean), ref)
        if mode in ("none", "pelvis"):
            assert np.isfinite(ref).all() and np.isfinite(host(xf)).all()


def test_real_size_meshes():
    est0, gt0 = synthetic_pair(10475, 5)
    est1, gt1 = synthetic_pair(10475, 6)
    run_modes("eval V=10475", np.stack([est0, est1 * MIRROR]), np.stack([gt0, gt1]), modes=("procrustes", "pelvis"))


def test_masks_per_mesh():
    est, gt = G["v_est"].astype(np.float32), G["v_gt"].astype(np.float32)
    rng = np.random.RandomState(3)
    masks = rng.uniform(size=(3, 400)) < 0.5
    masks[:, [2, 3]] = True                                  # the pelvis anchors stay in every subset
    masks[2] = False                                         # a mesh with no valid point
    E3, G3 = np.stack([est, est * MIRROR, est]), np.stack([gt, gt, gt])
    for mode in MODES:
        for mdtype in (torch.bool, torch.uint8):
            err, mean, xf = engine.align_errors(cuda(E3), cuda(G3), mode=mode, mask=cuda(masks, mdtype), return_transform=True)
            err, mean, xf = host(err), host(mean), host(xf)
            assert np.all(err[~masks] == 0.0)
            assert np.isnan(mean[2]) and np.all(err[2] == 0.0)
            for b in range(2):
                keep = np.flatnonzero(masks[b])
                anchors = tuple(int(np.searchsorted(keep, a)) for a in (2, 3))
                check_mesh("eval masked", mode, E3[b][keep], G3[b][keep], err[b][keep], mean[b], xf[b], anchors)     # (mean: over the valid points)
                # the same subset gathered and scored on its own
                e1, m1, x1 = engine.align_errors(cuda(E3[b][keep][None]), cuda(G3[b][keep][None]), mode=mode, anchors=anchors,
                                                 return_transform=True)
                check_mesh("eval gathered", mode, E3[b][keep], G3[b][keep], host(e1)[0], host(m1)[0], host(x1)[0], anchors)


def test_batch_independence_and_the_empty_batch():
    pairs = [synthetic_pair(257, 40 + b) for b in range(5)]
    est, gt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    est[1] *= MIRROR
    masks = np.random.RandomState(9).uniform(size=(5, 257)) < 0.7
    masks[:, :2] = True
    for mode in MODES:
        whole = engine.align_errors(cuda(est), cuda(gt), mode=mode, mask=cuda(masks, torch.bool), anchors=(0, 1), return_transform=True)
        for b in range(5):
            alone = engine.align_errors(cuda(est[b:b + 1]), cuda(gt[b:b + 1]), mode=mode, mask=cuda(masks[b:b + 1], torch.bool),
                                        anchors=(0, 1), return_transform=True)
            for w, a in zip(whole, alone):
                assert torch.equal(w[b:b + 1], a), (mode, b)
    nn = engine.nearest_distances(cuda(est), cuda(gt), [0.05, 0.2], mask_a=cuda(masks, torch.bool))
    for b in range(5):
        alone = engine.nearest_distances(cuda(est[b:b + 1]), cuda(gt[b:b + 1]), [0.05, 0.2], mask_a=cuda(masks[b:b + 1], torch.bool))
        for k in nn:
            assert torch.equal(nn[k][b:b + 1], alone[k]), (k, b)
    # B = 0: returns at once, before any pointer is looked at
    lib = _capi.load()
    assert lib.sfx_eval_align(1, 0, 5, None, None, None, None, 0, None, None, None, None) == 0
    assert lib.sfx_eval_nearest(0, 5, 5, None, None, None, None, 0, None, None, None, None, None, None, None) == 0
    e, m = engine.align_errors(cuda(np.zeros((0, 5, 3))), cuda(np.zeros((0, 5, 3))))
    assert e.shape == (0, 5) and m.shape == (0,)
    assert engine.nearest_distances(cuda(np.zeros((0, 5, 3))), cuda(np.zeros((0, 4, 3))), [0.1])["count_ab"].shape == (0, 1)


def test_library_refuses_without_launching():
    lib = _capi.load()
    x, e = cuda(np.zeros((1, 5, 3))), cuda(np.full((1, 5), 7.0))
    p = lambda t: C.c_void_p(t.data_ptr())
    anchors = _capi.i32([2, 5])
    assert lib.sfx_eval_align(3, 1, 5, p(x), p(x), None, _capi.iptr(anchors), 2, p(e), None, None, None) == -1
    assert b"anchor 5 outside the 5 points" in lib.sfx_last_error()
    assert lib.sfx_eval_align(3, 1, 5, p(x), p(x), None, None, 0, p(e), None, None, None) == -1
    assert lib.sfx_eval_align(4, 1, 5, p(x), p(x), None, None, 0, p(e), None, None, None) == -1
    assert lib.sfx_eval_align(1, 1, 0, p(x), p(x), None, None, 0, p(e), None, None, None) == -1
    assert lib.sfx_eval_align(1, 1, 5, p(x), p(x), None, None, 0, None, None, None, None) == -1
    th = _capi.f64([0.1])
    assert lib.sfx_eval_nearest(1, 5, 5, p(x), p(x), None, None, 1, _capi.dptr(th), None, None, None, None, None, None) == -1
    assert lib.sfx_eval_nearest(1, 5, 5, p(x), p(x), None, None, 9, _capi.dptr(th), None, None, None, None, None, None) == -1
    assert lib.sfx_eval_nearest(1, 5, 0, p(x), p(x), None, None, 0, None, None, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert torch.all(e == 7.0)                               # nothing was written


# ---- nearest neighbours ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Na,Nb", [(1, 1), (65, 257), (400, 400), (1025, 513)])
def test_nearest_distances_against_brute_force(Na, Nb):
    rng = np.random.RandomState(Na + Nb)
    a = (rng.normal(size=(2, Na, 3)) + [0.3, -1.2, 2.5]).astype(np.float32)
    b = (rng.normal(size=(2, Nb, 3)) + [0.3, -1.2, 2.5]).astype(np.float32)
    th = [0.1, 0.3, 1.0]
    nn = engine.nearest_distances(cuda(a), cuda(b), th)
    assert nn["dist_ab"].shape == (2, Na) and nn["dist_ba"].shape == (2, Nb) and nn["count_ab"].shape == (2, 3)
    assert nn["count_ab"].dtype == torch.int32 and nn["valid"].dtype == torch.int32
    assert np.array_equal(host(nn["valid"]), [[Na, Nb]] * 2)
    coord = max(np.abs(a).max(), np.abs(b).max())
    for m in range(2):
        for key, ckey, p, q in (("dist_ab", "count_ab", a[m], b[m]), ("dist_ba", "count_ba", b[m], a[m])):
            r64, r32 = brute_nearest(p.astype(np.float64), q.astype(np.float64)), brute_nearest(p, q)
            bound = bound_of(r32, r64, coord)
            d = host(nn[key])[m]
            H.check_bound("eval nearest", "%s %dx%d" % (key, Na, Nb), np.abs(d - r64).max(), bound)
            # counts: exact wherever no float64 distance lies within the bound of the threshold
            for k, t in enumerate(th):
                lo, hi = (r64 < t - bound).sum(), (r64 < t + bound).sum()
                assert lo <= int(host(nn[ckey])[m, k]) <= hi
                assert int(host(nn[ckey])[m, k]) == int((d.astype(np.float64) < t).sum())


def test_a_set_against_itself_is_exactly_zero():
    gt = G["v_gt"].astype(np.float32)
    x = cuda(np.stack([gt, gt[::-1]]))
    nn = engine.nearest_distances(x, x.clone(), [1e-6])
    assert torch.all(nn["dist_ab"] == 0.0) and torch.all(nn["dist_ba"] == 0.0)
    assert np.array_equal(host(nn["count_ab"]), [[400], [400]]) and np.array_equal(host(nn["count_ba"]), [[400], [400]])
    f = E.point_fscore(x[0], x[0].clone(), 1e-6)
    assert f["fscore"].is_cuda and f["fscore"].dtype == torch.float64
    assert float(f["fscore"]) == 1.0 and float(f["precision"]) == 1.0 and float(f["recall"]) == 1.0


def test_counts_equal_the_float64_counts_on_the_golden_set():
    est, gt = G["v_est"].astype(np.float32).astype(np.float64), G["v_gt"].astype(np.float32).astype(np.float64)
    aligned = E.ProcrustesAlignment()(est.T, gt.T).T                       # float64 Procrustes on the host
    th = [0.05, 0.1, 0.2]
    d_ab, d_ba = brute_nearest(aligned, gt), brute_nearest(gt, aligned)
    assert_margin(np.concatenate([d_ab, d_ba]), th)
    want_ab, want_ba = [int((d_ab < t).sum()) for t in th], [int((d_ba < t).sum()) for t in th]
    assert sorted(zip(want_ab, want_ba))[0] in ((133, 134), (134, 133)) and want_ab[1:] == [371, 400] and want_ba[1:] == [371, 400]
    nn = engine.nearest_distances(cuda(aligned[None]), cuda(gt[None]), th, return_distances=False)
    assert set(nn) == {"count_ab", "count_ba", "valid"}
    assert host(nn["count_ab"])[0].tolist() == want_ab and host(nn["count_ba"])[0].tolist() == want_ba
    assert host(nn["valid"])[0].tolist() == [400, 400]


def test_masked_targets_are_never_chosen():
    # a: one query at the origin.  b: its nearest target (0.01 away) is masked, the second nearest is 5 away
    a = np.zeros((1, 1, 3), np.float32)
    b = np.array([[[0.01, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, 0.0, -7.0]]], np.float32)
    mb = np.array([[False, True, True]])
    nn = engine.nearest_distances(cuda(a), cuda(b), [1.0, 6.0], mask_b=cuda(mb, torch.bool))
    assert host(nn["dist_ab"]).tolist() == [[5.0]]
    assert host(nn["dist_ba"]).tolist() == [[0.0, 5.0, 7.0]]              # 0 at the masked point
    assert host(nn["count_ab"]).tolist() == [[0, 1]] and host(nn["count_ba"]).tolist() == [[0, 1]]
    assert host(nn["valid"]).tolist() == [[1, 2]]
    # the same in a larger set, across tile and workgroup edges: every second target masked
    rng = np.random.RandomState(11)
    A2, B2 = rng.normal(size=(1, 700, 3)).astype(np.float32), rng.normal(size=(1, 1300, 3)).astype(np.float32)
    ma, mb = rng.uniform(size=(1, 700)) < 0.5, np.arange(1300)[None] % 2 == 0
    nn = engine.nearest_distances(cuda(A2), cuda(B2), [0.2], mask_a=cuda(ma, torch.uint8), mask_b=cuda(mb, torch.bool))
    r_ab = brute_nearest(A2[0][ma[0]].astype(np.float64), B2[0][mb[0]].astype(np.float64))
    r_ba = brute_nearest(B2[0][mb[0]].astype(np.float64), A2[0][ma[0]].astype(np.float64))
    d_ab, d_ba = host(nn["dist_ab"])[0], host(nn["dist_ba"])[0]
    assert np.all(d_ab[~ma[0]] == 0.0) and np.all(d_ba[~mb[0]] == 0.0)
    bound = 2.0 ** -22 * max(np.abs(A2).max(), np.abs(B2).max())
    H.check_bound("eval nearest", "masked dist_ab", np.abs(d_ab[ma[0]] - r_ab).max(), bound)
    H.check_bound("eval nearest", "masked dist_ba", np.abs(d_ba[mb[0]] - r_ba).max(), bound)
    assert host(nn["valid"]).tolist() == [[int(ma.sum()), int(mb.sum())]]
    # a set with no valid point: distances 0, counts 0, and the F = 0 branch
    nn = engine.nearest_distances(cuda(A2), cuda(B2), [0.2], mask_b=cuda(np.zeros((1, 1300), bool), torch.bool))
    assert torch.all(nn["dist_ab"] == 0.0) and torch.all(nn["dist_ba"] == 0.0)
    assert host(nn["count_ab"]).tolist() == [[0]] and host(nn["count_ba"]).tolist() == [[0]] and host(nn["valid"]).tolist() == [[700, 0]]
    assert float(E._fscore_from_counts(nn)[0]) == 0.0


# ---- compute_v2v -------------------------------------------------------------------------------------------------------------
def test_compute_v2v_device_against_the_host_path(monkeypatch):
    try:
        import scipy.spatial                                   # noqa: F401
    except ImportError:
        monkeypatch.setattr(E, "point_fscore", host_fscore)
    est32 = np.stack([G["v_est"], G["v_est"] * MIRROR]).astype(np.float32)
    gt32 = np.stack([G["v_gt"], G["v_gt"]]).astype(np.float32)
    vids = np.arange(0, 400, 2)
    th_pro, th_pel = [0.05, 0.1], [0.3, 2.0]        # (chosen on the CPU for the margin asserted below)

    def alignments():
        return {"procrustes": E.ProcrustesAlignmentMPJPE(fscore_thresholds=th_pro), "pelvis": E.PelvisAlignmentMPJPE(fscore_thresholds=th_pel)}

    ref = E.compute_v2v(est32.astype(np.float64), gt32.astype(np.float64), alignments(), vids=vids)
    ref32 = E.compute_v2v(est32, gt32, alignments(), vids=vids)
    # the margin condition on these inputs (float64): procrustes-aligned and pelvis-aligned estimate against the ground truth as given
    for b in range(2):
        e, g = est32[b][vids].astype(np.float64), gt32[b][vids].astype(np.float64)
        for aligned, th in ((E.ProcrustesAlignment()(e.T, g.T).T, th_pro), (E.PelvisAlignment()(g, e)[1], th_pel)):
            assert_margin(np.concatenate([brute_nearest(aligned, g), brute_nearest(g, aligned)]), th)
    out = E.compute_v2v(cuda(est32), cuda(gt32), alignments(), vids=vids, device=True)
    assert set(out) == set(ref) and set(out["point"]) == set(ref["point"]) and set(out["fscore"]) == set(ref["fscore"])
    coord = max(np.abs(est32).max(), np.abs(gt32).max())
    for name in ref["point"]:
        p = out["point"][name]
        assert torch.is_tensor(p) and p.is_cuda and tuple(p.shape) == ref["point"][name].shape == (2, 200)
        H.check_bound("eval compute_v2v", name + " point", np.abs(host(p) - ref["point"][name]).max(),
                      bound_of(ref32["point"][name], ref["point"][name], coord))
        assert set(out["fscore"][name]) == set(ref["fscore"][name]) == set(th_pro if name == "procrustes" else th_pel)
        for t, f in out["fscore"][name].items():
            assert torch.is_tensor(f) and f.is_cuda and f.dtype == torch.float64 and tuple(f.shape) == (2,)
            assert np.abs(host(f) - ref["fscore"][name][t]).max() <= 1e-12, (name, t, host(f), ref["fscore"][name][t])
    # the pelvis quirk is live: its F-score is not the one of the two aligned sets
    assert not np.allclose(ref["fscore"]["pelvis"][th_pel[0]], 1.0)
    # masks: the masked-out points hold 0 and the rest equals a call on the gathered subset
    masks = np.random.RandomState(5).uniform(size=(2, 200)) < 0.6
    masks[:, [2, 3]] = True
    outm = E.compute_v2v(cuda(est32), cuda(gt32), alignments(), vids=vids, masks=cuda(masks, torch.bool), device=True)
    for b in range(2):
        keep = vids[masks[b]]
        one = {"procrustes": E.ProcrustesAlignmentMPJPE()}
        r64 = E.compute_v2v(est32[b:b + 1].astype(np.float64), gt32[b:b + 1].astype(np.float64), one, vids=keep)["point"]["procrustes"][0]
        r32 = E.compute_v2v(est32[b:b + 1], gt32[b:b + 1], one, vids=keep)["point"]["procrustes"][0]
        p = host(outm["point"]["procrustes"])[b]
        assert np.all(p[~masks[b]] == 0.0)
        H.check_bound("eval compute_v2v", "masked point", np.abs(p[masks[b]] - r64).max(), bound_of(r32, r64, coord))
        # the documented average: the sum over the valid count
        H.check_bound("eval compute_v2v", "masked mean", abs(p.astype(np.float64).sum() / masks[b].sum() - r64.mean()), bound_of(r32, r64, coord))
