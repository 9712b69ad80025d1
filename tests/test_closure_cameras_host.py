"""CPU tests of the per-frame camera fixture (tests/camera_common.py) the GPU closure tests stand on: its rotation convention
against the drop-in's own camera, the preconditions the GPU tests rely on, and the reference gradient under a rotated,
fx != fy, off-centre camera against central differences of its own loss."""
import numpy as np
import pytest
import torch

import camera_common as CC
import test_gpu_parity as T

EPS = 2.0 ** -52


@pytest.mark.parametrize("which", ["body", "full"])
def test_fixture_projection_is_the_dropin_cameras(synth_model, which):
    """oracle.objective.project == smplifyx_amd.camera.PerspectiveCamera.forward == the fixture's own re-projection on the four
    cameras, in float64: the rotation convention of the fixture (p = R j + t, R row-major) is the drop-in camera's, which copies
    the reference's einsum.  Bound: 8 ulp of float64 on the forward-error scale of each pixel coordinate,
    f (sum_j |R_aj p_j| + |t_a|) / z + |c| -- the three restatements differ in the order of a 4-term sum, a division and a
    multiply-add (a transposed rotation moves frame 3's pixels by hundreds)."""
    from oracle import objective as obj
    from smplifyx_amd.camera import PerspectiveCamera
    cs = CC.shared_set(synth_model, which)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    j, R, t = cs["joints"], cs["R"].astype(np.float64), np.asarray(cs["frames"]["cam_t"], np.float64)
    uv_o = obj.project(t64(j), t64(R), t64(t), t64(cs["focal"][:, 0]), t64(cs["focal"][:, 1]), t64(cs["center"])).numpy()
    cam = PerspectiveCamera(rotation=t64(R), translation=t64(t), focal_length_x=t64(cs["focal"][:, 0]),
                            focal_length_y=t64(cs["focal"][:, 1]), center=t64(cs["center"]), batch_size=CC.B, dtype=torch.float64)
    with torch.no_grad():
        uv_c = cam(t64(j)).numpy()
    uv_f, p = CC.project_np(j, R, t, cs["focal"], cs["center"])
    mag = np.einsum("nab,nkb->nka", np.abs(R), np.abs(j)) + np.abs(t)[:, None, :]
    scale = cs["focal"][:, None, :] * mag[..., :2] / p[..., 2:3] + np.abs(cs["center"])[:, None, :]
    for a, b in ((uv_o, uv_c), (uv_f, uv_c)):
        assert np.all(np.abs(a - b) <= 8 * EPS * scale), float((np.abs(a - b) / scale).max() / EPS)
    # the convention is visible: the transposed rotation is another camera in every rotated frame
    uv_t, _ = CC.project_np(j, np.swapaxes(R, 1, 2), t, cs["focal"], cs["center"])
    assert np.all(np.abs(uv_t - uv_c)[1:].reshape(3, -1).max(1) > 50.0) and np.array_equal(uv_t[0], uv_f[0])


def test_cameras_share_no_field(synth_model):
    """No two frames share a value of any camera field except fx (and the image height, so data_weight) of frames 0 and 1, whose
    fy, centre and rotation differ: a record read from another frame's slot changes the projection.  The rotations are float32
    numbers (what the float64 batch asks for), orthonormal to float32 rounding."""
    cs = CC.shared_set(synth_model, "body")
    cols = dict(fy=cs["focal"][:, 1], cx=cs["center"][:, 0], cy=cs["center"][:, 1])
    for name, v in cols.items():
        assert len(set(v.tolist())) == CC.B, name
    assert len(set(cs["focal"][:, 0].tolist())) == CC.B - 1 and cs["focal"][0, 0] == cs["focal"][1, 0]
    assert len(set(cs["data_weight"].tolist())) == CC.B - 1 and cs["data_weight"][0] == cs["data_weight"][1]      # H = 600 twice
    assert len({(f, w) for f, w in zip(cs["focal"][:, 1], cs["data_weight"])}) == CC.B
    R = cs["R"]
    assert R.dtype == np.float32 and np.array_equal(R[0], np.eye(3, dtype=np.float32))
    for a in range(CC.B):
        assert np.abs(R[a].astype(np.float64) @ R[a].astype(np.float64).T - np.eye(3)).max() < 4 * 2.0 ** -24
        assert a == 0 or np.abs(R[a] - R[a].T).max() > 0.1                    # a transposed rotation is another rotation
        for b in range(a + 1, CC.B):
            assert np.abs(R[a] - R[b]).max() > 0.1 and np.abs(R[a] - R[b].T).max() > 0.1
    assert cs["focal"][1, 0] != cs["focal"][1, 1] and cs["focal"][2, 0] != cs["focal"][2, 1]         # a swapped pair shows
    # frame 3 turns the image axes into each other: x' = -y, y' = x
    assert np.abs(R[3].astype(np.float64) - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])).max() < 1e-7


@pytest.mark.parametrize("which", ["body", "full"])
def test_preconditions_of_the_gpu_tests(synth_model, which):
    """What tests/test_gpu_closure_cameras.py relies on, so that it holds without a GPU:
      every joint of every frame is well in front of its camera (p_cam.z > 5 m: no pole of the projection nearby);
      at the truth the re-projected frames' residual is the keypoint noise, at most 5 px on every live keypoint;
      dropped detections stay (0, 0, 0) and the confidences are the frames' own."""
    cs = CC.shared_set(synth_model, which)
    fr = cs["frames"]
    _, p = CC.project_np(cs["joints"], cs["R"], fr["cam_t"], cs["focal"], cs["center"])
    assert p[..., 2].min() > 5.0, p[..., 2].min()
    cfg = CC.cfg_for(which)
    old = T.synth_frames(synth_model, cfg, CC.B)
    assert np.array_equal(fr["keypoints"][..., 2], old["keypoints"][..., 2])
    dropped = np.all(old["keypoints"] == 0, axis=2)
    assert dropped.any() and np.array_equal(dropped, ~cs["live"]) and np.all(fr["keypoints"][dropped] == 0)
    assert not np.any(np.all(fr["keypoints"][~dropped] == 0, axis=1))
    tr = fr["truth"]
    n = lambda k: np.zeros((CC.B, k), np.float32)
    truth = dict(global_orient=tr["global_orient"], pose_embedding=tr["body_pose"], betas=tr["betas"], cam_translation=fr["cam_t"],
                 expression=n(10), jaw_pose=n(3), leye_pose=n(3), reye_pose=n(3), left_hand_pose=n(12), right_hand_pose=n(12))
    res, live = CC.residuals(synth_model, cfg, cs, truth)
    seen = cs["live"]
    # (keypoints are float32: half an ulp of a coordinate below 4096 px is 1.2e-4 px; cam_t is float32 too)
    assert np.abs(res - cs["noise"])[seen].max() < 2e-3, np.abs(res - cs["noise"])[seen].max()
    assert 0.5 < np.abs(res[seen]).max() <= 5.0, np.abs(res[seen]).max()
    assert live.sum() >= 0.5 * live.size


@pytest.mark.parametrize("pts,rho,side,scope", CC.RHO_CASES)
def test_rho_cases_sit_where_the_gpu_test_says(synth_model, pts, rho, side, scope):
    """The robustifier rho^2 r^2 / (r^2 + rho^2) is exercised on both of its ends only when residuals lie on both sides of rho.
    'both': a tenth at least of the live residual components on either side of rho -- over the four frames (scope 'set': rho = 30
    at the far points, where camera 2's short focal keeps its own frame below 26 px, and rho = 3 at the near points, where a
    frame has one to fifteen components above) or in every frame under its own camera (scope 'frame': rho = 12 / rho = 1, added
    for that).  'below a fifth': every live component below rho / 5, the near-quadratic end."""
    cs = CC.shared_set(synth_model, "body")
    cfg = CC.cfg_for("body", rho=rho)
    res, live = CC.residuals(synth_model, cfg, cs, CC.points(cs, pts))
    per = [np.abs(res[i][live[i]]).ravel() for i in range(CC.B)]
    assert min(r.size for r in per) >= 20
    for r in per if scope == "frame" else [np.concatenate(per)]:
        if side == "both":
            above = float((r > rho).mean())
            assert 0.1 <= above <= 0.9, (pts, rho, scope, above, np.percentile(r, [0, 10, 50, 90, 100]))
        else:
            assert r.max() < rho / 5, (pts, rho, r.max())
    if side == "both":
        assert sum(bool((r > rho).any() and (r < rho).any()) for r in per) >= 3                     # (three frames of four at least)


# central differences of the float64 oracle's loss: step per parameter block (the blocks' curvature scales differ by orders:
# a metre of camera translation, a radian of a joint, a unit of shape)
FD_STEP = dict(cam_translation=1e-4, global_orient=1e-5, betas=1e-4, body_pose=1e-5, pose_embedding=1e-5, left_hand_pose=1e-4,
               right_hand_pose=1e-4, expression=1e-4, jaw_pose=1e-5, leye_pose=1e-5, reye_pose=1e-5)
FD_LOG = {}
LOSS_ULPS = 32


@pytest.mark.parametrize("which,stage", [("body", -1), ("body", 2), ("full", 2)])
def test_reference_gradient_under_camera_2_matches_central_differences(synth_model, which, stage):
    """The reference the GPU tests compare with is autograd of the oracle; under a rotated, fx != fy, off-centre camera it has
    never been checked against anything.  Here: camera 2 (rotation vector (0.5, 0.9, -0.4), f = (1400, 1650), centre (960, 200)),
    the far point of its frame, the camera stage and the last body stage; three coordinates (first, middle, last) of every
    block against D(h) = (f(x + h e) - f(x - h e)) / 2h.
      truncation: D(h) - f' = c h^2 + O(h^4), so t = |D(h) - D(h/2)| = 3/4 |c| h^2 is observed, and D(h/2) is off by t / 3;
      roundoff:   a loss value is a sum of some fifty to a few hundred non-negative terms, each a few roundings deep: within
                  32 ulp of |f| in any summation order, so D(h/2) carries at most r = 2 * 32 eps |f| / h (observed: 5 ulp,
                  camera stage, t_z, where r is all of the bound).
      bound:      |D(h/2) - g| <= t + r -- three times the observed truncation error of D(h/2), plus the roundoff of the
                  difference itself.  Nothing in it comes from g.  No coordinate uses more than a tenth of it.
    Observed, relative to the largest entry of the block's gradient (printed per block; LAB_NOTES.md 3.6): |D(h/2) - g| <=
    5e-11 in the camera stage and <= 3.2e-8 in the body stage (the jaw of the body cfg, whose gradient is the smallest), with
    t + r at 1e-9 and 5.2e-6 there; in the blocks that carry the gradient (pose, shape, orientation) |D(h/2) - g| <= 1.1e-10
    under t + r <= 1e-8.  A dead coordinate (body_pose) has D = g = 0 exactly."""
    cs = CC.shared_set(synth_model, which)
    cfg = CC.cfg_for(which)
    P = CC.points(cs, "far")
    i = 2
    ff = CC.frame_fit(synth_model, cfg, cs, i, torch.float64)
    lo, go, _ = T._oracle_closure_at(ff, i, P, stage, torch.float64)
    blocks = CC.H.gradient_blocks(ff, stage)
    CC.H.assert_blocks_tile(blocks, go.size)
    if stage < 0:
        ps, fn = [ff.cam_t, ff.bm.global_orient], ff.camera_objective
    else:
        ps = [p for p in ff.bm.parameters() if p.requires_grad] + [ff.pose_embedding]
        w = dict(ff.stages[stage]); w["data_weight"] = ff.data_weight
        w["bending_prior_weight"] = 3.17 * w["body_pose_weight"]
        jw = ff.jw.clone()
        if ff.use_hands: jw[:, ff.nb:ff.nb + 42] = w["hand_weight"]
        if ff.use_face: jw[:, ff.nb + 42:] = w["face_weight"]
        jw[:, ff.low] = 0
        fn = lambda: ff.body_terms(stage, w, jw)["total"]
    x0 = torch.cat([p.detach().reshape(-1) for p in ps]).numpy().copy()

    def f(x):
        o = 0
        with torch.no_grad():
            for p in ps:
                p.copy_(torch.as_tensor(x[o:o + p.numel()], dtype=torch.float64).view_as(p)); o += p.numel()
            return float(fn())
    assert f(x0) == lo
    D = lambda q, h: (f(x0 + h * np.eye(1, x0.size, q)[0]) - f(x0 - h * np.eye(1, x0.size, q)[0])) / (2 * h)
    for name, a, b in blocks:
        h = FD_STEP[name]
        gmax = np.abs(go[a:b]).max()
        for q in sorted({a, (a + b) // 2, b - 1}):
            d1, d2 = D(q, h), D(q, h / 2)
            t, r = abs(d1 - d2), 2 * LOSS_ULPS * EPS * abs(lo) / h
            err = abs(d2 - go[q])
            if gmax > 0:
                e = FD_LOG.setdefault((which, stage, name), [0.0, 0.0])
                e[0], e[1] = max(e[0], err / gmax), max(e[1], (t + r) / gmax)
            else:
                assert d1 == 0.0 and d2 == 0.0 and go[q] == 0.0, (name, q)
            assert err <= t + r, (which, stage, name, q, d2, go[q], err, t, r)
    print("\n".join("central differences %-5s stage %2d %-16s |D(h/2) - g| / max|g_b| %.1e   bound t + r %.1e" % (k + tuple(v))
                    for k, v in sorted(FD_LOG.items()) if k[:2] == (which, stage)))
