"""The fitting closure under per-frame cameras on the MI355X: rotation, fx != fy, off-centre principal points, per-frame
data weights (tests/camera_common.py: four cameras that share no field), and under loss settings no shipped cfg has.

Every other closure test of the suite runs with R = I, fx = fy = 5000, the centre at (W/2, H/2), one data_weight, rho = 100,
use_joints_conf and depth_loss_weight = 100: closure_math.h project_residual (Rc row-major, fx and fy apart), the adjoint through
the transpose and (fx, fy) in closure_body.h, the camera record of host/batch.hip (and its float64 twin) and the focal of
host/eval.hip k_guess_init have never seen anything else.

Bounds of every closure comparison (camera_common.bounds, helpers.check_closure_blocks):
  loss, whole gradient   max(helpers.CLOSURE_*_TOL, 10 x the float32 oracle's own error against the float64 oracle at the same
                         point, camera and setting)
  per block              max(CLOSURE_GRAD_TOL, 10 x the float32 oracle's error in the block); a block whose reference is exactly
                         zero is exactly zero on the device
  float64 batch          the same scaled by helpers.F64_UNIT_RATIO (floors 7.5e-15 on the loss; on the gradient 1e-14, the bound
                         of test_gpu_float64.py, which is the tighter of the two)
No frame, stage or block is left out.  B = 4 everywhere; the oracle results are cached per (settings, camera, point set, frame,
stage) in camera_common -- not in test_gpu_parity's session cache, whose key knows neither the camera nor rho."""
import numpy as np
import pytest
import torch

import camera_common as CC
import helpers as H
import test_gpu_parity as T
from test_gpu_parity import gpu      # noqa: F401  (the GPU fixture of the parity tests)

pytestmark = pytest.mark.gpu

F64_LOSS_FLOOR = H.CLOSURE_LOSS_TOL * H.F64_UNIT_RATIO
F64_GRAD_FLOOR = min(1e-14, H.CLOSURE_GRAD_TOL * H.F64_UNIT_RATIO)


def _stages(fb):
    return (-1, 0, fb.n_stages - 1)


def _compare(label, model, cfg, cs, P, pts, fb, stages, unit_ratio=1.0, loss_floor=H.CLOSURE_LOSS_TOL, grad_floor=H.CLOSURE_GRAD_TOL):
    """The batch's closure at every stage of `stages` against the oracle under each frame's own camera; returns
    {stage: (loss, grad, oracle loss, oracle grad)}."""
    out = {}
    for stage in stages:
        loss, grad = fb.closure(stage)
        lo, go, lo32, go32, blocks = CC.oracle_set(model, cfg, cs, P, stage, pts)
        H.assert_blocks_tile(blocks, fb.num_vars(stage))
        assert grad.shape == go.shape
        for i in range(len(lo)):
            lt, gt = CC.bounds(lo[i], go[i], lo32[i], go32[i], unit_ratio, loss_floor, grad_floor)
            H.check_closure(label, stage, loss[i], lo[i], grad[i], go[i], loss_tol=lt, grad_tol=gt)
        H.check_closure_blocks(label, stage, grad, go, go32, blocks, floor=grad_floor, unit_ratio=unit_ratio)
        out[stage] = (loss, grad, lo, go)
    return out


# ---------------------------------------------------------------- (a) parity under the four cameras
@pytest.mark.parametrize("which,mode", [("body", "rows"), ("body", "dense"), ("full", "dense")])
def test_closure_under_per_frame_cameras(gpu, synth_model, which, mode):
    """Camera stage, first and last body stage at the far and the near points: frame 0 is the control (the camera of every
    other test); frame 3 (R = Rz(pi/2)) changes sign under a transposed rotation, frames 1 and 2 have fx != fy, and no frame can
    borrow another frame's record unnoticed."""
    cfg, cs = CC.cfg_for(which), CC.shared_set(synth_model, which)
    dm = T._dm(synth_model, cfg)
    for pts in ("far", "near"):
        P = CC.points(cs, pts)
        fb = CC.device_batch(dm, cfg, cs, P, mode)
        _compare("cam-%s-%s-%s" % (pts, which, mode), synth_model, cfg, cs, P, pts, fb, _stages(fb))
        fb.close()
    dm.close()


# ---------------------------------------------------------------- (b) the float64 batch
def test_float64_closure_under_per_frame_cameras(gpu, synth_model):
    """precision="float64" (rows, body cfg): the double camera record D.cam64 next to the float rotation, camera stage and last
    body stage, both point sets.  The rotations are float32 numbers widened, the same values the oracle gets."""
    cfg = CC.cfg_for("body", float_dtype="float64")
    cs = CC.shared_set(synth_model, "body")
    dm = T._dm(synth_model, cfg)
    for pts in ("far", "near"):
        P = CC.points(cs, pts)
        fb = CC.device_batch(dm, cfg, cs, P, "rows", precision="float64")
        assert fb.float64
        got = _compare("cam-f64-%s-body-rows" % pts, synth_model, cfg, cs, P, pts, fb, (-1, fb.n_stages - 1),
                       unit_ratio=H.F64_UNIT_RATIO, loss_floor=F64_LOSS_FLOOR, grad_floor=F64_GRAD_FLOOR)
        assert all(l.dtype == np.float64 and g.dtype == np.float64 for l, g, _, _ in got.values())
        fb.close()
    dm.close()


# ---------------------------------------------------------------- (c) batch composition, bitwise
@pytest.mark.parametrize("which,mode,slots", [("body", "rows", 0), ("body", "dense", 0), ("body", "dense", 2), ("full", "dense", 0)])
def test_frame_in_the_batch_equals_the_frame_alone_bitwise(gpu, synth_model, which, mode, slots):
    """Each frame's loss and gradient from the batch of four is, bit for bit, what the frame gives alone (B = 1) under its own
    camera: with four different records a frame that read another's -- in part -- cannot be.  (slots = 2: the library rounds a
    column pool up to 32 columns, so four frames are resident whatever is asked; the case pins that an asked-for pool does not
    reach the closure.  Frames that do queue: test_fit_through_a_column_pool_keeps_each_frames_camera.)"""
    cfg, cs = CC.cfg_for(which), CC.shared_set(synth_model, which)
    dm = T._dm(synth_model, cfg)
    P = CC.points(cs, "far")
    fb = CC.device_batch(dm, cfg, cs, P, mode, slots=slots)
    stages = _stages(fb)
    full = [fb.closure(s) for s in stages]
    fb.close()
    for i in range(CC.B):
        fb = CC.device_batch(dm, cfg, CC.subset(cs, [i]), {k: v[i:i + 1] for k, v in P.items()}, mode)
        for s, (l4, g4) in zip(stages, full):
            l1, g1 = fb.closure(s)
            assert np.isfinite(l1[0]) and np.any(g1[0] != 0)
            assert l4[i] == l1[0] and np.array_equal(g4[i], g1[0]), (i, s, l4[i], l1[0], np.abs(g4[i] - g1[0]).max())
        fb.close()
    # ... and the records do differ: the control's camera on frame 2's keypoints is another loss
    wrong = CC.subset(cs, [2])
    for k in ("R", "focal", "center", "data_weight"):
        wrong[k] = cs[k][[0]]
    fb = CC.device_batch(dm, cfg, wrong, {k: v[2:3] for k, v in P.items()}, mode)
    assert all(fb.closure(s)[0][0] != l4[2] for s, (l4, _) in zip(stages, full))
    fb.close(); dm.close()


# ---------------------------------------------------------------- (d) guess_init
@pytest.mark.parametrize("mode", ["rows", "dense"])
def test_guess_init_uses_each_frames_focal(gpu, synth_model, mode):
    """fb.guess_init under the four cameras: cam_translation[:, 2] = fx_b * mean|d3D| / mean|d2D| (fitting.py:87-102) with frame
    b's own fx, x and y exactly zero.  Bound: the float32 oracle's own rounding -- the largest relative difference of its float32
    run to its float64 run over the four frames, not below 2**-24 (half an ulp: what one correctly rounded float32 result is
    off by) -- times the project's usual 10."""
    from oracle import objective as obj
    cfg, cs = CC.cfg_for("body"), CC.shared_set(synth_model, "body")
    fr = cs["frames"]
    dm = T._dm(synth_model, cfg)
    P = dict(global_orient=fr["reg_global"], pose_embedding=fr["reg_pose"], cam_translation=np.zeros((CC.B, 3), np.float32),
             est_tz=np.zeros(CC.B, np.float32))
    fb = CC.device_batch(dm, cfg, cs, P, mode)
    fb.guess_init(cfg["body_tri_idxs"])
    got = fb.get_params()["cam_translation"]
    fb.close(); dm.close()
    want = {}
    for dtype in (torch.float64, torch.float32):
        est = []
        for i in range(CC.B):
            ff = CC.frame_fit(synth_model, cfg, cs, i, dtype)          # (its constructor runs guess_init_depth with focal = fx_i)
            with torch.no_grad():
                out = ff.bm(body_pose=ff._body_pose(), return_verts=False, return_full_pose=False)
                again = obj.guess_init_depth(out.joints, ff.gt, cfg["body_tri_idxs"], float(cs["focal"][i, 0]))
            assert float(again) == float(ff.init_t[0, 2])
            est.append(float(ff.init_t[0, 2]))
        want[dtype] = np.array(est)
    w64, w32 = want[torch.float64], want[torch.float32]
    yard = max(float(np.abs(w32 - w64).max() / np.abs(w64).min()), 2.0 ** -24)
    bound = 10.0 * yard             # 10 x max(the float32 oracle's error against its float64 run, 2**-24); 3e-6 where this was written
    assert np.all(got[:, :2] == 0)
    for i in range(CC.B):
        H.check_bound("cam-guess-init-%s" % mode, "t_z frame %d (fx %g)" % (i, cs["focal"][i, 0]), abs(got[i, 2] - w64[i]) / abs(w64[i]), bound)
    # the depth follows the focal: with frame 0's focal on every frame the estimates of frames 2 and 3 are 3.6 and 2.1 times off
    assert np.all(np.abs(w64 * (cs["focal"][0, 0] / cs["focal"][:, 0]) - w64)[2:] > 0.5 * w64[2:])


# ---------------------------------------------------------------- (e) loss settings
def _setting(name):
    """(cfg overrides, point set) of one loss setting no shipped cfg has."""
    if name.startswith("rho"):
        pts, rho = {"rho30": ("far", 30.0), "rho3": ("near", 3.0), "rho1000": ("far", 1000.0), "rho12": ("far", 12.0),
                    "rho1": ("near", 1.0)}[name]
        assert (pts, rho) in [c[:2] for c in CC.RHO_CASES]          # (the sides of rho are asserted on the CPU)
        return dict(rho=rho), pts
    return dict(noconf=dict(use_joints_conf=False), depth0=dict(depth_loss_weight=0.0), depth17=dict(depth_loss_weight=17.0),
                camconf_off=dict(use_conf_for_camera_init=False), camconf_on=dict(use_conf_for_camera_init=True),
                ign_none=dict(joints_to_ign=[-1]), thr0=dict(confidence_threshold=0.0),
                # (the synthetic detector's confidences are U(0.3, 1) or 0 for a dropped keypoint: under use_joints_conf the
                #  threshold 0 changes no weight.  Two more values that do: without the confidences a dropped keypoint at (0, 0)
                #  carries its full weight, and 0.6 takes out four detections in ten)
                thr0_noconf=dict(confidence_threshold=0.0, use_joints_conf=False), thr06=dict(confidence_threshold=0.6))[name], "far"


SETTING_NAMES = ("rho30", "rho3", "rho1000", "rho12", "rho1", "noconf", "depth0", "depth17", "camconf_off", "camconf_on", "ign_none",
                 "thr0", "thr0_noconf", "thr06")
_SETTING_RUNS = {}


def _run_setting(model, name):
    """{stage: (loss, grad, oracle loss, oracle grad)} of one setting: body cfg, dense, the three stages, every comparison
    asserted; evaluated once per session."""
    if name not in _SETTING_RUNS:
        over, pts = _setting(name)
        cfg, cs = CC.cfg_for("body", **over), CC.shared_set(model, "body")
        for k, v in over.items():
            assert CC.cfg_for("body").get(k) != v or name == "camconf_on", (k, v)      # (camconf_on, the shipped value: the pair's control)
        dm = T._dm(model, cfg)
        P = CC.points(cs, pts)
        fb = CC.device_batch(dm, cfg, cs, P, "dense")
        _SETTING_RUNS[name] = _compare("cam-set-%s" % name, model, cfg, cs, P, pts, fb, _stages(fb))
        fb.close(); dm.close()
        if name == "ign_none":          # the setting reaches the weights: the joints the cfg ignores carry weight now
            ign = CC.cfg_for("body")["joints_to_ign"]
            assert np.all(T._jw(cfg, cs["frames"])[:, ign] == 1) and np.all(T._jw(CC.cfg_for("body"), cs["frames"])[:, ign] == 0)
    return _SETTING_RUNS[name]


@pytest.mark.parametrize("name", SETTING_NAMES)
def test_loss_settings_under_per_frame_cameras(gpu, synth_model, name):
    """C.rho on both ends of the robustifier (rho = 30 / 12 at the far points, 3 / 1 at the near points: residuals on both sides;
    rho = 1000: every residual below rho / 5), C.use_conf off, C.depth_w = 0 (its branch) and 17, the camera-init confidences
    both ways, no ignored joint, no confidence threshold (and one of 0.6) -- body cfg, dense, camera stage, first and last body
    stage, under the four cameras."""
    _run_setting(synth_model, name)


def test_depth_weight_moves_only_the_depth_gradient_by_the_oracles_amount(gpu, synth_model):
    """depth_loss_weight 0 against 17 in the camera stage: the gradient of cam_translation[2] changes by the oracle's amount,
    2 * 17^2 * (t_z - est_z), and no other entry changes at all.  Bound on the change: the two float32 entries it is the
    difference of carry half an ulp each from their last addition, the term itself three roundings (a difference, two products):
    2**-24 * (|g_0| + |g_17| + 3 |change|), times 4."""
    (l0, g0, lo0, go0), (l17, g17, lo17, go17) = _run_setting(synth_model, "depth0")[-1], _run_setting(synth_model, "depth17")[-1]
    cs = CC.shared_set(synth_model, "body")
    P = CC.points(cs, "far")
    for i in range(CC.B):
        want = go17[i, 2] - go0[i, 2]
        assert abs(want - 2 * 17.0 ** 2 * (float(P["cam_translation"][i, 2]) - float(P["est_tz"][i]))) <= 1e-12 * abs(want)
        assert abs(want) > 50.0
        change = float(g17[i, 2]) - float(g0[i, 2])
        bound = 4 * 2.0 ** -24 * (abs(float(g0[i, 2])) + abs(float(g17[i, 2])) + 3 * abs(want))
        H.check_bound("cam-set-depth", "d grad t_z frame %d" % i, abs(change - want) / abs(want), bound / abs(want))
        keep = [q for q in range(g0.shape[1]) if q != 2]
        assert np.array_equal(g0[i, keep], g17[i, keep]), i
        assert l17[i] > l0[i]


# ---------------------------------------------------------------- (f) the drop-in path
def test_dropin_closure_uses_the_cameras_rotation_and_both_focals(gpu, synth_model):
    """FittingMonitor.create_fitting_closure with a PerspectiveCamera that has camera 2's rotation (requires_grad off), fx = 1400,
    fy = 1650 and centre (960, 200): the camera-init loss and the first body stage -- the returned loss and the .grad of the
    optimised tensors against the oracle under the same camera, within the bounds of this file.  (Before FrameBatch.set_frames
    took (fx, fy) pairs the closure handed focal_length_x over for both: every v residual was computed with fy = 1400.)"""
    from smplifyx_amd import fitting, prior, smplx, utils
    from smplifyx_amd.camera import create_camera
    cfg, cs = CC.cfg_for("body"), CC.shared_set(synth_model, "body")
    i, dev, dtype = 2, torch.device("cuda"), torch.float32
    P = CC.points(cs, "far")
    fr = cs["frames"]
    K = fr["keypoints"].shape[1]
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    model_params = dict(model_path=synth_model, joint_mapper=utils.JointMapper(H.joint_map_for(cfg)), create_global_orient=True,
                        create_body_pose=True, create_betas=True, create_left_hand_pose=True, create_right_hand_pose=True,
                        create_expression=True, create_jaw_pose=True, create_leye_pose=True, create_reye_pose=True,
                        create_transl=False, dtype=dtype)
    bm = smplx.create(gender="neutral", **model_params,
                      **{k: v for k, v in cfg.items() if k not in model_params and k != "gender"}).to(dev)
    camera = create_camera(rotation=t(cs["R"][i:i + 1]), translation=t(P["cam_translation"][i:i + 1]),
                           focal_length_x=t(cs["focal"][i:i + 1, 0]), focal_length_y=t(cs["focal"][i:i + 1, 1]),
                           center=t(cs["center"][i:i + 1]), batch_size=1, dtype=dtype).to(dev)
    camera.rotation.requires_grad = False
    assert float(camera.focal_length_x) != float(camera.focal_length_y)
    pose_embedding = t(P["pose_embedding"][i:i + 1]).requires_grad_(True)
    bm.reset_params(body_pose=pose_embedding, **{k: t(P[k][i:i + 1]) for k in P if k not in ("pose_embedding", "cam_translation", "est_tz")})
    kd = t(fr["keypoints"][i:i + 1])
    gt_joints, joints_conf = kd[:, :, :2], kd[:, :, 2].reshape(1, -1)
    joint_weights = t(T._jw(cfg, CC.subset(cs, [i])["frames"]))
    init_idxs = [int(k) for k in np.flatnonzero(T._cmask(cfg, CC.subset(cs, [i])["frames"])[0])]
    init_t = t([[0.0, 0.0, float(P["est_tz"][i])]])
    mk = lambda n: prior.create_prior(prior_type=n, dtype=dtype)
    camera_loss = fitting.create_loss("camera_init", joints_conf=joints_conf, use_conf=cfg["use_conf_for_camera_init"],
                                      trans_estimation=init_t, init_joints_idxs=torch.tensor(init_idxs, device=dev),
                                      depth_loss_weight=cfg.get("depth_loss_weight", 1e2), dtype=dtype).to(dev)
    loss = fitting.create_loss(loss_type="smplify", joint_weights=joint_weights, rho=cfg["rho"], use_joints_conf=True,
                               use_face=False, use_hands=False, body_pose_prior=mk("l2"), shape_prior=mk("l2"),
                               angle_prior=mk("angle"), interpenetration=False, dtype=dtype,
                               regression_pose=t(fr["reg_pose"][i:i + 1]), num_stages=3).to(dev)
    data_weight = float(cs["data_weight"][i])

    def flat(ps):
        return torch.cat([(p.grad.reshape(-1) if p.grad is not None else torch.zeros(p.numel(), device=dev)) for p in ps]).cpu().numpy()
    with fitting.FittingMonitor(**cfg) as monitor:
        camera_loss.reset_loss_weights({"data_weight": data_weight})
        camera.translation.requires_grad = True
        bm.global_orient.requires_grad = True
        fit_camera = monitor.create_fitting_closure(None, bm, camera, gt_joints, camera_loss, create_graph=False, use_vposer=False,
                                                    pose_embedding=pose_embedding, return_full_pose=False, return_verts=False)
        lc = float(fit_camera(stage=0))
        gc = flat([camera.translation, bm.global_orient])
        final_params = [p for p in bm.parameters() if p.requires_grad] + [pose_embedding]
        w = {"data_weight": data_weight, "body_pose_weight": torch.tensor(float(cfg["body_pose_prior_weights"][0]), device=dev),
             "shape_weight": torch.tensor(float(cfg["shape_weights"][0]), device=dev)}
        w["bending_prior_weight"] = 3.17 * w["body_pose_weight"]
        loss.reset_loss_weights(w)
        closure = monitor.create_fitting_closure(None, bm, camera=camera, gt_joints=gt_joints, joints_conf=joints_conf,
                                                 joint_weights=joint_weights, loss=loss, create_graph=False, use_vposer=False,
                                                 pose_embedding=pose_embedding, return_verts=True, return_full_pose=True)
        lb = float(closure(stage=0))
        gb = flat(final_params)
    for stage, l, g in ((-1, lc, gc), (0, lb, gb)):
        lo, go, lo32, go32, blocks = CC.oracle_closure(synth_model, cfg, cs, i, P, stage, "far")
        assert g.shape == go.shape, (stage, g.shape, go.shape)
        lt, gt = CC.bounds(lo, go, lo32, go32)
        H.check_closure("cam-dropin-body", stage, l, lo, g, go, loss_tol=lt, grad_tol=gt)
        H.check_closure_blocks("cam-dropin-body", stage, g, go, go32, blocks)


# ---------------------------------------------------------------- (g) one fit, bitwise
def _fit_job(synth_model, n):
    """n frames (the four synthetic frames in turn, later rounds 0.37 px further off each) seen through cameras 0, 2, 3 in turn
    with R = I and the centre at (W/2, H/2), as driver.fit_frames sets them: keypoints, H, W, focal [n], reg_pose, reg_global."""
    cs = CC.shared_set(synth_model, "body")
    fr = cs["frames"]
    f_idx = np.arange(n) % CC.B
    c_idx = np.array([0, 2, 3])[np.arange(n) % 3]
    Hs, Ws, fx = cs["H"][c_idx], 2.0 * cs["center"][c_idx, 0], cs["focal"][c_idx, 0]
    uv, p = CC.project_np(cs["joints"][f_idx], np.tile(np.eye(3), (n, 1, 1)), np.asarray(fr["cam_t"], np.float64)[f_idx],
                          np.stack([fx, fx], 1), np.stack([Ws * 0.5, Hs * 0.5], 1))
    assert p[..., 2].min() > 5.0
    kp = np.concatenate([uv + cs["noise"][f_idx] + 0.37 * (np.arange(n) // CC.B)[:, None, None], fr["keypoints"][f_idx][..., 2:3]], -1)
    kp[~cs["live"][f_idx]] = 0.0
    return dict(keypoints=kp.astype(np.float32), H=Hs, W=Ws, focal=fx, reg_pose=fr["reg_pose"][f_idx], reg_global=fr["reg_global"][f_idx])


def _fit_cfg():
    cfg = CC.cfg_for("body", maxiters=5)
    cfg["use_camera_prior"] = False
    return cfg


def _same(a, b, rows_a, rows_b, what):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k])[rows_a], np.asarray(b[k])[rows_b]
        assert np.array_equal(x, y, equal_nan=True), (what, k)


def test_fit_with_per_frame_image_size_and_focal_is_shard_invariant_bitwise(gpu, synth_model):
    """driver.fit_frames (dense, maxiters 5) with H, W and focal given as [B] from cameras 0, 2 and 3: every returned array
    equals, bit for bit, what each frame gives fitted alone with its own numbers -- test_shard_invariance_bitwise for cameras
    that differ.  (fit_frames has no rotation argument: R = I.)"""
    from smplifyx_amd import driver
    cfg = _fit_cfg()
    dm = T._dm(synth_model, cfg)
    job = _fit_job(synth_model, 3)
    jw = H.base_joint_weights(cfg, job["keypoints"].shape[1])
    kw = dict(lbs_mode="dense", reuse_entry_eval=True)
    res = driver.fit_frames(dm, cfg, job["keypoints"], jw, job["H"], job["W"], job["focal"], reg_pose=job["reg_pose"],
                            reg_global=job["reg_global"], **kw)
    assert np.all(np.isfinite(res["stage_loss"])) and np.all(res["stage_evals"] > 0)
    assert len(set(res["cam_translation"][:, 2].tolist())) == 3
    for i in range(3):
        one = driver.fit_frames(dm, cfg, job["keypoints"][i:i + 1], jw, float(job["H"][i]), float(job["W"][i]), float(job["focal"][i]),
                                reg_pose=job["reg_pose"][i:i + 1], reg_global=job["reg_global"][i:i + 1], **kw)
        _same(res, one, slice(i, i + 1), slice(0, 1), "frame %d alone" % i)
    dm.close()


def test_fit_through_a_column_pool_keeps_each_frames_camera(gpu, synth_model):
    """36 frames through a pool of 32 GEMM columns (the smallest pool the library forms: four frames queue and take over the
    columns of frames that finish), cameras 0, 2, 3 in turn so that a frame's column and its index part ways: bit for bit the
    resident run, in the queue's predicted-cost order and in the given one -- a record read by column where the frame index is
    meant (or kept on chip from the column's previous frame) cannot be."""
    from smplifyx_amd import driver
    cfg = _fit_cfg()
    dm = T._dm(synth_model, cfg)
    n = 36
    job = _fit_job(synth_model, n)
    jw = H.base_joint_weights(cfg, job["keypoints"].shape[1])
    run = lambda **kw: driver.fit_frames(dm, cfg, job["keypoints"], jw, job["H"], job["W"], job["focal"], reg_pose=job["reg_pose"],
                                         reg_global=job["reg_global"], lbs_mode="dense", reuse_entry_eval=True, **kw)
    resident = run(slots=0)
    assert np.isfinite(resident["stage_loss"]).mean() > 0.9
    for order in ("given", "auto"):
        _same(resident, run(slots=32, order=order), slice(None), slice(None), "pool of 32, order %s" % order)
    dm.close()
