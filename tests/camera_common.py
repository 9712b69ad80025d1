"""Per-frame cameras for the closure tests: four cameras no two of which share a rotation, a focal pair, a centre or a data
weight, the synthetic frames re-projected through them, and the oracle / device closures under them.

Every other closure-vs-oracle test of the suite sets R = I, fx = fy = 5000, the centre at (W/2, H/2) and one data_weight for the
whole batch: a transposed or mis-strided rotation, a swapped focal pair or a camera record read from another frame's slot is
invisible there.  Shared by tests/test_closure_cameras_host.py (CPU: the fixture's own preconditions) and
tests/test_gpu_closure_cameras.py (MI355X)."""
import hashlib

import numpy as np
import torch

import helpers as H

# rotation vector | fx, fy | centre | image height (data_weight = 1000 / H).  Frame 0 is the control (the camera of every other
# test); frame 3 turns the image axes into each other (R = Rz(pi/2): a transposed R changes sign); 1 and 2 are generic.  No two
# frames share a value of any field except fx of frames 0 and 1.
CAMERAS = (dict(rotvec=(0.0, 0.0, 0.0), fx=5000.0, fy=5000.0, center=(400.0, 300.0), H=600),
           dict(rotvec=(0.15, -0.2, 0.1), fx=5000.0, fy=4600.0, center=(352.5, 311.25), H=600),
           dict(rotvec=(0.5, 0.9, -0.4), fx=1400.0, fy=1650.0, center=(960.0, 200.0), H=1080),
           dict(rotvec=(0.0, 0.0, np.pi / 2), fx=2400.0, fy=2400.0, center=(17.0, 1033.0), H=2160))
B = len(CAMERAS)
# (point set, rho, where the live residual components lie, over the set or in every frame) of the loss-settings test; the
# sides are asserted on the CPU (tests/test_closure_cameras_host.py)
RHO_CASES = (("far", 30.0, "both", "set"), ("near", 3.0, "both", "set"), ("far", 1000.0, "below a fifth", "frame"),
             ("far", 12.0, "both", "frame"), ("near", 1.0, "both", "frame"))


def project_np(j, R, t, focal, center):
    """uv [n, K, 2] and camera-space points [n, K, 3] of joints j [n, K, 3] (float64): p = R j + t, uv = f p_xy / p_z + c."""
    p = np.einsum("nab,nkb->nka", np.asarray(R, np.float64), np.asarray(j, np.float64)) + np.asarray(t, np.float64)[:, None, :]
    uv = np.asarray(focal, np.float64)[:, None, :] * p[..., :2] / p[..., 2:3] + np.asarray(center, np.float64)[:, None, :]
    return uv, p


def camera_set(model, cfg, frames):
    """The B = 4 cameras and `frames` (synthetic.make_frames, 4 frames) re-projected through them:
      R [4, 3, 3] float32 (rounded first: the same float32 values, widened, go to the oracle and to the device -- the float64
      batch refuses a rotation that is no float32 number), focal [4, 2] = (fx, fy), center [4, 2], H [4], data_weight [4]
      (float64), frames (a copy with new keypoints; the scalar H / W / focal of the uniform camera are left out), joints [4, K, 3]
      (the truth joints, float64) and noise [4, K, 2] (the frame's own keypoint noise).
    A keypoint of the new frames is the projection of the frame's truth joint through its camera plus the noise the frame had
    (old keypoint minus old projection); dropped detections stay (0, 0, 0)."""
    from oracle.fit_frame import rotvec_to_mat
    kp = np.asarray(frames["keypoints"])
    assert kp.shape[0] == B, kp.shape
    R = np.stack([rotvec_to_mat(c["rotvec"]) for c in CAMERAS]).astype(np.float32)
    focal = np.array([[c["fx"], c["fy"]] for c in CAMERAS], np.float64)
    center = np.array([c["center"] for c in CAMERAS], np.float64)
    Hs = np.array([c["H"] for c in CAMERAS], np.float64)
    j = np.asarray(H.oracle_joints_fn(model, cfg)(frames["truth"]), np.float64)
    cam_t = np.asarray(frames["cam_t"], np.float64)
    eye = np.tile(np.eye(3), (B, 1, 1))
    old_uv, _ = project_np(j, eye, cam_t, np.full((B, 2), frames["focal"]), np.tile([frames["W"] * 0.5, frames["H"] * 0.5], (B, 1)))
    live = ~np.all(kp == 0, axis=2)
    noise = np.where(live[..., None], kp[..., :2].astype(np.float64) - old_uv, 0.0)
    uv, _ = project_np(j, R, cam_t, focal, center)
    new = np.concatenate([uv + noise, kp[..., 2:3].astype(np.float64)], -1)
    new[~live] = 0.0
    fr = {k: v for k, v in frames.items() if k not in ("H", "W", "focal")}
    fr["keypoints"] = new.astype(np.float32)
    return dict(R=R, focal=focal, center=center, H=Hs, data_weight=1000.0 / Hs, frames=fr, joints=j, noise=noise, live=live)


_SETS = {}


def cfg_for(which, **over):
    """'body' / 'full': cfg_files/fit_smplx_combined_coco25.yaml without / with hands and face; `over` changes loss settings."""
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", **(dict(use_hands=False, use_face=False) if which == "body" else {}))
    cfg.update(over)
    return cfg


def shared_set(model, which):
    """camera_set of the 4 synthetic frames of cfg `which`, made once per session; shared and not to be written to.  (The frames
    do not depend on the loss settings: one set serves every variation of a cfg.)"""
    import test_gpu_parity as T
    if which not in _SETS:
        cfg = cfg_for(which)
        cs = camera_set(model, cfg, T.synth_frames(model, cfg, B))
        for v in list(cs.values()) + [cs["frames"]["keypoints"]]:          # (the arrays made here; the others are the frames' own)
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SETS[which] = (model, cs)
    assert _SETS[which][0] is model
    return _SETS[which][1]


def subset(cs, idx):
    """The camera set of frames `idx` only (a batch of its own)."""
    idx = list(idx)
    out = {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in cs.items() if k != "frames"}
    out["frames"] = {k: (v[idx] if isinstance(v, np.ndarray) else
                         ({n: a[idx] for n, a in v.items()} if isinstance(v, dict) else v)) for k, v in cs["frames"].items()}
    return out


def frame_fit(model, cfg, cs, i, dtype):
    """oracle.fit_frame.FrameFit of frame i under its own camera: built as helpers.oracle_frame_fit builds one (regression
    prior), then cam_R / fx / fy / center / data_weight -- plain attributes that oracle.objective.project and the two objectives
    read -- are overwritten."""
    from oracle.fit_frame import FrameFit
    fr = cs["frames"]
    K = fr["keypoints"].shape[1]
    assert not cfg.get("use_vposer")
    ff = FrameFit(H.oracle_model(model, cfg, dtype), fr["keypoints"][i:i + 1], float(cs["H"][i]), 2.0 * float(cs["center"][i, 0]),
                  float(cs["focal"][i, 0]), cfg, H.base_joint_weights(cfg, K), reg_pose=fr["reg_pose"][i],
                  reg_global=fr["reg_global"][i], dtype=dtype)
    ff.cam_R = torch.tensor(cs["R"][i:i + 1].astype(np.float64), dtype=dtype)
    ff.fx = torch.tensor(cs["focal"][i:i + 1, 0], dtype=dtype)
    ff.fy = torch.tensor(cs["focal"][i:i + 1, 1], dtype=dtype)
    ff.center = torch.tensor(cs["center"][i:i + 1], dtype=dtype)
    ff.data_weight = torch.tensor(float(cs["data_weight"][i]), dtype=dtype)
    return ff


# what an oracle result of this file depends on beside the model, the camera and the point: the cfg keys the oracle reads that the
# tests change (float_dtype is not one: the oracle's dtype is an argument, and the float64 batch shares the float32 batch's entry)
SETTINGS = ("use_hands", "use_face", "format", "use_face_contour", "use_vposer", "rho", "use_joints_conf",
            "depth_loss_weight", "use_conf_for_camera_init", "joints_to_ign", "confidence_threshold", "body_pose_prior_weights",
            "shape_weights", "data_weights", "init_joints_idxs")
_ORACLE = {}


def _settings(cfg):
    return tuple((k, repr(cfg.get(k))) for k in SETTINGS)


def _digest(model, cfg, cs, params, i):
    h = hashlib.sha1()
    for a in (model["v_template"], model["weights"], cs["frames"]["keypoints"][i], cs["frames"]["reg_pose"][i],
              cs["frames"]["reg_global"][i], cs["R"][i], cs["focal"][i], cs["center"][i], cs["data_weight"][i]):
        h.update(np.ascontiguousarray(np.asarray(a)).tobytes())
    h.update(repr(_settings(cfg)).encode())
    for k in sorted(params):
        h.update(k.encode()); h.update(np.ascontiguousarray(np.asarray(params[k])[i:i + 1]).tobytes())
    return h.hexdigest()


def oracle_closure(model, cfg, cs, i, params, stage, pts=None):
    """(loss64, grad64, loss32, grad32, blocks) of the oracle under frame i's camera at row i of `params` (with est_tz), float64
    and float32.  `pts` names the point set and caches the result for the session, so that the rows and the dense test of one
    cfg share one CPU evaluation; the key holds the camera and every setting of SETTINGS, and so does the digest a cached entry
    is checked against (test_gpu_parity's session cache holds neither: it is not used here)."""
    import test_gpu_parity as T
    out = []
    for dtype in (torch.float64, torch.float32):
        k = dig = None
        if pts is not None:
            cam = tuple(np.concatenate([cs["R"][i].ravel(), cs["focal"][i], cs["center"][i], cs["data_weight"][i:i + 1]]).tolist())
            k = (_settings(cfg), cam, str(pts), int(i), int(stage), dtype)
            dig = _digest(model, cfg, cs, params, i)
            if k in _ORACLE:
                assert _ORACLE[k][0] == dig, ("oracle cache key reused for another model, frame, camera, setting or point", k)
                out.append(_ORACLE[k][1:])
                continue
        lo, go, ff = T._oracle_closure_at(frame_fit(model, cfg, cs, i, dtype), i, params, stage, dtype)
        go.setflags(write=False)
        blocks = tuple(H.gradient_blocks(ff, stage))
        if k is not None:
            _ORACLE[k] = (dig, lo, go, blocks)
        out.append((lo, go, blocks))
    (lo, go, blocks), (lo32, go32, _) = out
    return lo, go, lo32, go32, blocks


def oracle_set(model, cfg, cs, params, stage, pts=None):
    """oracle_closure of every frame: (loss64 [B], grad64 [B, N], loss32 [B], grad32 [B, N], blocks)."""
    rows = [oracle_closure(model, cfg, cs, i, params, stage, pts) for i in range(cs["R"].shape[0])]
    return (np.array([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows]),
            np.stack([r[3] for r in rows]), rows[0][4])


def bounds(lo, go, lo32, go32, unit_ratio=1.0, loss_floor=H.CLOSURE_LOSS_TOL, grad_floor=H.CLOSURE_GRAD_TOL):
    """(loss bound, whole-gradient bound) of one frame: max(the project's closure bound, 10 x the float32 oracle's own error
    against the float64 oracle at the same point, camera and setting [x unit_ratio: the arithmetic under test])."""
    le, ge = H.closure_errors(lo32, lo, go32, go)
    return max(loss_floor, 10.0 * le * unit_ratio), max(grad_floor, 10.0 * ge * unit_ratio)


def device_batch(dm, cfg, cs, params, mode, precision="mixed", slots=0):
    """FrameBatch of the camera set's frames under their cameras at `params` (with est_tz)."""
    import test_gpu_parity as T
    from smplifyx_amd import engine
    fr = cs["frames"]
    n = fr["keypoints"].shape[0]
    fb = engine.FrameBatch(dm, n, cfg, lbs_mode=mode, reuse_entry_eval=False, has_regression_pose=True, slots=slots,
                           precision=precision)
    fb.set_frames(fr["keypoints"], T._jw(cfg, fr), T._cmask(cfg, fr), cs["focal"], cs["center"], cs["data_weight"],
                  est_tz=params["est_tz"], cam_rot=cs["R"])
    fb.set_params(regression_pose=fr["reg_pose"], **{k: v for k, v in params.items() if k != "est_tz"})
    return fb


def points(cs, pts):
    """The point set `pts` ('far' / 'near': test_gpu_parity.far_points / near_points, B = 4) with est_tz."""
    import test_gpu_parity as T
    P, est = T.far_points(cs["frames"], B, 11) if pts == "far" else T.near_points(cs["frames"], B)
    P["est_tz"] = est
    return P


def residuals(model, cfg, cs, params):
    """[4, K, 2] data residual gt - projection (float64 oracle, each frame under its camera) at `params`, and the mask of the
    live components: keypoints that are detected and carry weight in cfg (helpers.base_joint_weights, confidence threshold)."""
    import test_gpu_parity as T
    fr = cs["frames"]
    res = []
    for i in range(cs["R"].shape[0]):
        ff = frame_fit(model, cfg, cs, i, torch.float64)
        with torch.no_grad():
            for k, v in params.items():
                if k in ("est_tz",):
                    continue
                t = ff.pose_embedding if k == "pose_embedding" else ff.cam_t if k == "cam_translation" else getattr(ff.bm, k)
                t.copy_(torch.tensor(v[i:i + 1], dtype=torch.float64))
            out = ff.bm(return_verts=False, body_pose=ff._body_pose(), return_full_pose=False)
            res.append((ff.gt - ff._project(out.joints))[0].numpy())
    live = cs["live"] & (T._jw(cfg, fr) > 0)
    return np.stack(res), live
