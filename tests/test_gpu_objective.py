"""GPU tests of the differentiable losses: create_loss(..., differentiable=True) over sfx_objective_eval / sfx_camera_init_eval
(csrc/objective_ext.hip, engine.objective_eval / camera_init_eval, fitting._differentiable_*).

Parity (tests 1, 2).  Reference: fp64 autograd of oracle.objective.project + smplify_terms / camera_init_loss (oracle/prior_gmm.py
for the mixture, tables of tests/golden/gmm.npz; the per-component form restated in tests/objective_common.py on the same
tables and pinned against tests/golden/gmm_unmerged.npz by tests/test_objective_host.py), one frame at a time.  Error measure: |l - l64| / |l64| for a frame's loss and
||g - g64|| / ||g64|| per frame and gradient block (joints, rotation, translation, body_pose, prior operand, betas, expression,
jaw, each hand).  Yardstick: the SAME oracle in torch.float32 against its fp64 run at the same points, largest over the frames.
Bound: max(10 x yardstick, helpers.CLOSURE_LOSS_TOL / CLOSURE_GRAD_TOL) -- the margin and the floors helpers.py states for
every closure comparison of the suite.  Every block's fp64 norm is >= 0.1 (asserted) so that no ratio is formed against
noise; a block whose reference is exactly zero (a term switched off) must be exactly zero on the device.  The weights are fp32
numbers (the loss module keeps them in fp32 buffers), so both oracles and the device read the same values.

The parity runs go through the public surface (a hand-built ModelOutput whose fields are leaves, a PerspectiveCamera, the loss
module, per_frame=True, backward): the kernel, the engine wrapper, the autograd function and the stage logic are all under the
bound.  Shapes: B = 3; K = 26 (fewer keypoints than lanes), 136 (two passes and a partial third), 64 (exactly one pass).

Observed on MI355X (the session summary prints every comparison next to its bound): loss <= 2.0e-7; d joints
1.05e-6, d rotation 1.5e-6, d translation 1.6e-6 (yardsticks 7e-7 .. 2.6e-6), prior operand 3.1e-7, every other block <= 1.1e-7;
every comparison at <= 0.18 x its bound; the smallest fp64 block norm is 2e2.  Camera-init loss: <= 1.0e-6 everywhere.
"""
import types

import numpy as np
import pytest
import torch

import helpers as H
from oracle import objective as O
from oracle.fit_frame import rotvec_to_mat
from oracle.prior_gmm import MaxMixtureRef
from objective_common import _PerComponentRef, _gmm

pytestmark = pytest.mark.gpu

BLOCKS = ("joints", "rotation", "translation", "body_pose", "prior", "betas", "expression", "jaw_pose", "left_hand_pose",
          "right_hand_pose")
KINDS = ("body", "full", "k64")
FORMS = ("embedding", "target_last", "target_early", "l2_body_pose", "gmm_merged", "gmm_unmerged")
FACTOR = 10.0
MIN_NORM = 0.1
RHO = 100.0
NUM_STAGES = 3
# the stage's weights, rounded to fp32 once: what the module's buffers hold
WEIGHTS = {k: float(np.float32(v)) for k, v in dict(data_weight=1000.0 / 600, body_pose_weight=20.0, shape_weight=75.0,
                                                    bending_prior_weight=3.17 * 20.0, hand_prior_weight=57.4,
                                                    expr_prior_weight=10.0).items()}
JAW_W = (100.0, 1000.0, 1000.0)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    return torch.device("cuda:0")


def _cfg(kind):
    if kind == "body":
        return H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False)
    return H.load_cfg("fit_smplx_combined_halpe.yaml")


# ---------------------------------------------------------------------------------------------------------------------------
# inputs (numpy float32), shared by the tests
_INPUTS = {}


def inputs(model, kind, B=3, seed=3):
    key = (kind, B, seed)
    if key in _INPUTS:
        return _INPUTS[key]
    cfg = _cfg(kind)
    rng = np.random.RandomState(seed)
    P = H.random_params(rng, B, scale=0.5, npca=cfg["num_pca_comps"])
    bm = H.oracle_model(model, cfg, torch.float64)
    J = []
    for i in range(B):
        bm.reset_params(**{k: v[i:i + 1] for k, v in P.items() if k != "pose_embedding"})
        with torch.no_grad():
            J.append(bm(return_verts=False, body_pose=torch.tensor(P["pose_embedding"][i:i + 1], dtype=torch.float64)).joints[0].numpy())
    joints = np.stack(J).astype(np.float32)
    jw = H.base_joint_weights(cfg, joints.shape[1])
    if kind == "k64":
        joints, jw = joints[:, :64], jw[:64]
    K = joints.shape[1]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    I = dict(joints=f32(joints),
             rotation=f32(np.stack([rotvec_to_mat(0.2 * rng.normal(size=3)) for _ in range(B)])),
             translation=f32(np.concatenate([0.3 * rng.normal(size=(B, 2)), rng.uniform(3.0, 5.0, size=(B, 1))], 1)),
             focal_x=f32(np.full(B, 5000.0)), focal_y=f32(np.full(B, 4800.0)), center=f32(np.tile([400.0, 300.0], (B, 1))),
             joint_weights=f32(np.tile(jw, (B, 1))))
    with torch.no_grad():
        d = lambda n: torch.tensor(I[n], dtype=torch.float64)
        proj = O.project(d("joints"), d("rotation"), d("translation"), d("focal_x"), d("focal_y"), d("center")).numpy()
        depth = (torch.einsum("bij,bkj->bki", d("rotation"), d("joints")) + d("translation")[:, None])[..., 2]
    assert float(depth.min()) > 1.0, "every keypoint is in front of the camera"
    # residuals between 5 and 300 px, either sign: both regimes of GMoF at rho = 100
    I["gt_joints"] = f32(proj + rng.uniform(5.0, 300.0, size=proj.shape) * rng.choice([-1.0, 1.0], size=proj.shape))
    conf = rng.uniform(0.0, 1.0, size=(B, K))
    conf[:, [2, 7, K - 1]] = 0.0        # missing detections: exact zeros, one of them in the last (partial) pass
    conf[0, 11] = 0.0
    I["joints_conf"] = f32(conf)
    mix, poses = _gmm()
    I.update(body_pose=f32(0.3 * rng.normal(size=(B, 63))), embedding=f32(rng.normal(size=(B, 32))),
             target=f32(rng.normal(size=(B, 32))), pose63=f32(np.resize(poses, (B, 63)) + 0.05 * rng.normal(size=(B, 63))),
             betas=f32(P["betas"]), expression=f32(P["expression"]), jaw_pose=f32(P["jaw_pose"]),
             left_hand_pose=f32(0.3 * rng.normal(size=(B, 45))), right_hand_pose=f32(0.3 * rng.normal(size=(B, 45))))
    I["_cfg"], I["_K"], I["_B"] = cfg, K, B
    _INPUTS[key] = I
    return I


def _form_kw(form, I, i, dtype):
    """(operand name, smplify_terms keywords of the pose prior) of one frame."""
    t = lambda a: torch.tensor(a[i:i + 1], dtype=dtype)
    mix, _ = _gmm()
    if form == "embedding":
        return "embedding", dict(use_vposer=True, regression_pose=None, stage=0)
    if form == "target_last":
        return "embedding", dict(use_vposer=True, regression_pose=t(I["target"]), stage=NUM_STAGES - 1)
    if form == "target_early":
        return "embedding", dict(use_vposer=True, regression_pose=t(I["target"]), stage=0)
    if form == "l2_body_pose":
        return "pose63", dict(use_vposer=False, regression_pose=None, body_pose_prior=None)
    ref = MaxMixtureRef if form == "gmm_merged" else _PerComponentRef
    return "pose63", dict(use_vposer=False, regression_pose=None, body_pose_prior=ref(mix["means"], mix["covars"], mix["weights"], dtype))


def oracle(I, form, hands, face, dtype):
    """(loss [B], {block: [B, ...]}) by autograd of the oracle in `dtype`, one frame at a time."""
    B = I["_B"]
    losses, grads = [], {b: [] for b in BLOCKS}
    w = {k: torch.tensor(v, dtype=dtype) for k, v in WEIGHTS.items()}
    w["jaw_prior_weight"] = torch.tensor(JAW_W, dtype=dtype)
    for i in range(B):
        t = lambda a: torch.tensor(a[i:i + 1], dtype=dtype)
        op, kw = _form_kw(form, I, i, dtype)
        leaf = {b: t(I[op if b == "prior" else b]).requires_grad_(True) for b in BLOCKS}
        proj = O.project(leaf["joints"], leaf["rotation"], leaf["translation"], t(I["focal_x"]), t(I["focal_y"]), t(I["center"]))
        full_pose = torch.cat([torch.zeros(1, 3, dtype=dtype), leaf["body_pose"], torch.zeros(1, 99, dtype=dtype)], 1)
        out = types.SimpleNamespace(body_pose=leaf["prior"], betas=leaf["betas"], full_pose=full_pose, expression=leaf["expression"],
                                    jaw_pose=leaf["jaw_pose"], left_hand_pose=leaf["left_hand_pose"], right_hand_pose=leaf["right_hand_pose"])
        total = O.smplify_terms(out, proj, t(I["gt_joints"]), t(I["joints_conf"]), t(I["joint_weights"]), w, leaf["prior"],
                                num_stages=NUM_STAGES, use_joints_conf=True, use_hands=hands, use_face=face, rho=RHO, **kw)["total"]
        g = torch.autograd.grad(total, [leaf[b] for b in BLOCKS], allow_unused=True)
        losses.append(float(total.detach()))
        for b, gi in zip(BLOCKS, g):
            grads[b].append((gi if gi is not None else torch.zeros_like(leaf[b])).double().numpy()[0])
    return np.array(losses), {b: np.stack(v) for b, v in grads.items()}


_REF = {}


def reference(model, kind, form, hands=True, face=True):
    """fp64 reference and fp32 yardstick of one case (computed once, left unchanged)."""
    key = (kind, form, hands, face)
    if key not in _REF:
        I = inputs(model, kind)
        l64, g64 = oracle(I, form, hands, face, torch.float64)
        l32, g32 = oracle(I, form, hands, face, torch.float32)
        yard = {"loss": float(np.max(np.abs(l32 - l64) / np.abs(l64)))}
        for b in BLOCKS:
            n = np.linalg.norm(g64[b].reshape(len(l64), -1), axis=1)
            e = np.linalg.norm((g32[b] - g64[b]).reshape(len(l64), -1), axis=1)
            yard[b] = float(np.max(e[n > 0] / n[n > 0])) if (n > 0).any() else None
        _REF[key] = dict(I=I, loss=l64, grads=g64, yard=yard)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the device side, through the public surface
def _priors():
    from smplifyx_amd import prior
    return lambda t: prior.create_prior(prior_type=t, dtype=torch.float32)


def make_loss(gpu, form, I=None, hands=True, face=True, differentiable=True, **over):
    from smplifyx_amd import fitting, prior
    mk = _priors()
    bpp = mk("l2")
    if form in ("gmm_merged", "gmm_unmerged"):
        mix, _ = _gmm()
        bpp = prior.MaxMixturePrior(gmm=mix, num_gaussians=8, dtype=torch.float32, use_merged=form == "gmm_merged")
    reg = None
    if form in ("target_last", "target_early"):
        reg = torch.tensor(I["target"], device=gpu)
    kw = dict(rho=RHO, use_joints_conf=True, use_face=face, use_hands=hands, body_pose_prior=bpp, shape_prior=mk("l2"),
              angle_prior=mk("angle"), expr_prior=mk("l2"), jaw_prior=mk("l2"), left_hand_prior=mk("l2"), right_hand_prior=mk("l2"),
              interpenetration=False, dtype=torch.float32, regression_pose=reg, num_stages=NUM_STAGES, differentiable=differentiable)
    kw.update(over)
    loss = fitting.create_loss(loss_type="smplify", **kw).to(gpu)
    w = dict(WEIGHTS)
    if not hands:
        w.pop("hand_prior_weight")
    if not face:
        w.pop("expr_prior_weight")
    else:
        w["jaw_prior_weight"] = list(JAW_W)
    loss.reset_loss_weights(w)
    return loss


def make_camera(gpu, I, sl=slice(None), dtype=torch.float32):
    from smplifyx_amd.camera import create_camera
    t = lambda n: torch.tensor(I[n][sl], dtype=dtype)
    B = I["rotation"][sl].shape[0]
    cam = create_camera(rotation=t("rotation"), translation=t("translation"), focal_length_x=t("focal_x"), focal_length_y=t("focal_y"),
                        center=t("center"), batch_size=B, dtype=dtype)
    return cam.to(gpu)


def make_output(gpu, I, form, sl=slice(None), dtype=torch.float32):
    """A hand-built ModelOutput whose fields are leaves: (output, {block: leaf}, pose_embedding or None, use_vposer)."""
    from smplifyx_amd import smplx
    vp = form in ("embedding", "target_last", "target_early")
    leaf = {b: torch.tensor(I[("embedding" if vp else "pose63") if b == "prior" else b][sl], dtype=dtype, device=gpu).requires_grad_(True)
            for b in BLOCKS if b not in ("rotation", "translation")}
    B = leaf["joints"].shape[0]
    z = lambda n: torch.zeros(B, n, dtype=dtype, device=gpu)
    full_pose = torch.cat([z(3), leaf["body_pose"], z(99)], 1)
    out = smplx.ModelOutput(joints=leaf["joints"], full_pose=full_pose, betas=leaf["betas"],
                            body_pose=leaf["body_pose"] if vp else leaf["prior"], expression=leaf["expression"],
                            jaw_pose=leaf["jaw_pose"], left_hand_pose=leaf["left_hand_pose"], right_hand_pose=leaf["right_hand_pose"])
    return out, leaf, (leaf["prior"] if vp else None), vp


def device_eval(gpu, I, form, hands=True, face=True, sl=slice(None), stage=None, upstream=None, dtype=torch.float32):
    """(loss [B] tensor, {block: grad tensor}) of the differentiable loss at the inputs' rows `sl`, upstream ones (or given)."""
    if stage is None:
        stage = NUM_STAGES - 1 if form == "target_last" else 0
    loss = make_loss(gpu, form, I, hands, face)
    if form in ("target_last", "target_early"):
        loss.regression_pose = torch.tensor(I["target"][sl], device=gpu)
    cam = make_camera(gpu, I, sl, dtype)
    out, leaf, emb, vp = make_output(gpu, I, form, sl, dtype)
    t = lambda n: torch.tensor(I[n][sl], dtype=dtype, device=gpu)
    per = loss(out, camera=cam, gt_joints=t("gt_joints"), joints_conf=t("joints_conf"), joint_weights=t("joint_weights"),
               body_model_faces=None, use_vposer=vp, pose_embedding=emb, stage=stage, per_frame=True)
    assert per.requires_grad and per.dtype == dtype and tuple(per.shape) == (leaf["joints"].shape[0],)
    (per.sum() if upstream is None else (per * upstream).sum()).backward()
    leaf["rotation"], leaf["translation"] = cam.rotation, cam.translation
    grads = {b: (leaf[b].grad if leaf[b].grad is not None else torch.zeros_like(leaf[b])) for b in BLOCKS}
    return per.detach(), grads


def _check(label, R, per, grads, expect_dead=(), blocks=BLOCKS):
    l64, g64, yard = R["loss"], R["grads"], R["yard"]
    l = per.double().cpu().numpy()
    B = len(l64)
    for i in range(B):
        err, bound = abs(l[i] - l64[i]) / abs(l64[i]), max(FACTOR * yard["loss"], H.CLOSURE_LOSS_TOL)
        print("%-34s frame %d loss %14.6f  device %.2e  yardstick %.2e  bound %.2e" % (label, i, l64[i], err, yard["loss"], bound))
        H.check_bound(label, "loss", err, bound)
    for b in blocks:
        g = grads[b].double().cpu().numpy().reshape(B, -1)
        ref = g64[b].reshape(B, -1)
        assert g.shape == ref.shape and np.isfinite(g).all(), (label, b)
        if b in expect_dead:
            assert not ref.any() and not g.any(), (label, b, "a term that is switched off has an exactly zero gradient")
            print("%-34s %-16s reference exactly zero: device exactly zero" % (label, b))
            continue
        bound = max(FACTOR * yard[b], H.CLOSURE_GRAD_TOL)
        for i in range(B):
            nrm = float(np.linalg.norm(ref[i]))
            err = float(np.linalg.norm(g[i] - ref[i]) / nrm)
            print("%-34s frame %d %-16s |g64| %9.3e  device %.2e  yardstick %.2e  bound %.2e" % (label, i, b, nrm, err, yard[b], bound))
            assert nrm >= MIN_NORM, (label, b, i, nrm)
            H.check_bound(label, "d " + b, err, bound)


# ------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_loss_and_gradient_blocks_match_fp64_autograd_of_the_oracle(gpu, synth_model, kind, form):
    R = reference(synth_model, kind, form)
    per, grads = device_eval(gpu, R["I"], form)
    _check("objective %s %s" % (kind, form), R, per, grads)


def test_the_target_form_is_the_last_stages_only(gpu, synth_model):
    """fitting.py:391-395: with VPoser the regression prior acts at the last stage; before it the prior is |embedding|^2 --
    target_early's reference IS the embedding form's (asserted on the oracle), and the two device runs agree bit for bit."""
    a, b = reference(synth_model, "body", "embedding"), reference(synth_model, "body", "target_early")
    assert np.array_equal(a["loss"], b["loss"]) and all(np.array_equal(a["grads"][k], b["grads"][k]) for k in BLOCKS)
    c = reference(synth_model, "body", "target_last")
    assert not np.array_equal(a["grads"]["prior"], c["grads"]["prior"])
    pa, ga = device_eval(gpu, a["I"], "embedding")
    pb, gb = device_eval(gpu, a["I"], "target_early")
    assert torch.equal(pa, pb) and all(torch.equal(ga[k], gb[k]) for k in BLOCKS)


def test_hands_and_face_off(gpu, synth_model):
    for hands, face in ((False, False), (True, False), (False, True)):
        R = reference(synth_model, "full", "embedding", hands, face)
        per, grads = device_eval(gpu, R["I"], "embedding", hands, face)
        dead = (() if hands else ("left_hand_pose", "right_hand_pose")) + (() if face else ("expression", "jaw_pose"))
        _check("objective full hands=%d face=%d" % (hands, face), R, per, grads, expect_dead=dead)


# ------------------------------------------------------------------------------------------------------ 2. camera-init loss
def _camera_oracle(I, idxs, use_conf, est, dtype):
    B = I["_B"]
    losses, grads = [], {b: [] for b in BLOCKS[:3]}
    for i in range(B):
        t = lambda a: torch.tensor(a[i:i + 1], dtype=dtype)
        leaf = {b: t(I[b]).requires_grad_(True) for b in BLOCKS[:3]}
        proj = O.project(leaf["joints"], leaf["rotation"], leaf["translation"], t(I["focal_x"]), t(I["focal_y"]), t(I["center"]))
        total = O.camera_init_loss(proj, t(I["gt_joints"]), idxs, torch.tensor(WEIGHTS["data_weight"], dtype=dtype),
                                   torch.tensor(100.0, dtype=dtype), leaf["translation"][:, 2], t(est) if est is not None else None,
                                   joints_conf=t(I["joints_conf"]), use_conf=use_conf)
        g = torch.autograd.grad(total, [leaf[b] for b in BLOCKS[:3]])
        losses.append(float(total.detach()))
        for b, gi in zip(BLOCKS[:3], g):
            grads[b].append(gi.double().numpy()[0])
    return np.array(losses), {b: np.stack(v) for b, v in grads.items()}


@pytest.mark.parametrize("with_est", [True, False])
@pytest.mark.parametrize("use_conf", [True, False])
@pytest.mark.parametrize("kind", ["body", "full"])
def test_camera_init_loss_matches_the_oracle(gpu, synth_model, kind, use_conf, with_est):
    from smplifyx_amd import fitting, smplx
    I = inputs(synth_model, kind)
    B, K = I["_B"], I["_K"]
    idxs = [k for k in I["_cfg"]["init_joints_idxs"] if k < K]
    assert len(idxs) >= 4
    est = np.stack([np.zeros(B), np.zeros(B), I["translation"][:, 2] + 0.7], 1).astype(np.float32) if with_est else None
    est_z = est[:, 2] if with_est else None
    l64, g64 = _camera_oracle(I, idxs, use_conf, est_z, torch.float64)
    l32, g32 = _camera_oracle(I, idxs, use_conf, est_z, torch.float32)
    yard = {"loss": float(np.max(np.abs(l32 - l64) / np.abs(l64)))}
    for b in BLOCKS[:3]:
        n = np.linalg.norm(g64[b].reshape(B, -1), axis=1)
        yard[b] = float(np.max(np.linalg.norm((g32[b] - g64[b]).reshape(B, -1), axis=1) / n))
    t = lambda n: torch.tensor(I[n], device=gpu)
    loss = fitting.create_loss("camera_init", init_joints_idxs=torch.tensor(idxs), trans_estimation=torch.tensor(est) if with_est else None,
                               data_weight=WEIGHTS["data_weight"], depth_loss_weight=1e2, joints_conf=t("joints_conf"),
                               use_conf=use_conf, differentiable=True).to(gpu)
    cam = make_camera(gpu, I)
    joints = t("joints").requires_grad_(True)
    per = loss(smplx.ModelOutput(joints=joints), camera=cam, gt_joints=t("gt_joints"), per_frame=True)
    assert tuple(per.shape) == (B,) and per.requires_grad
    per.sum().backward()
    grads = dict(joints=joints.grad, rotation=cam.rotation.grad, translation=cam.translation.grad)
    label = "camera-init %s conf=%d est=%d" % (kind, use_conf, with_est)
    _check(label, dict(loss=l64, grads=g64, yard=yard), per.detach(), grads, blocks=BLOCKS[:3])
    # keypoints outside init_joints_idxs: exactly zero rows
    rest = [k for k in range(K) if k not in idxs]
    assert not joints.grad[:, rest].any() and joints.grad[:, idxs].abs().amax(-1).min() > 0
    # the 0-d form is the sum of the frames (the reference's reduction)
    cam2 = make_camera(gpu, I)
    total = loss(smplx.ModelOutput(joints=t("joints")), camera=cam2, gt_joints=t("gt_joints"))
    assert total.dim() == 0 and torch.equal(total, per.detach().sum())


# --------------------------------------------------------------------------------------------------- 3. zero weight is exact
def test_zero_weight_keypoints_contribute_exactly_nothing(gpu, synth_model):
    """conf 0 (a missing detection) or joint weight 0: the rows of d joints are exactly 0, and the loss and every other
    gradient do not change by a bit when those keypoints' detections and 3-D positions are replaced by anything else."""
    I = dict(inputs(synth_model, "full"))
    dead = (I["joints_conf"] * I["joint_weights"]) == 0
    assert dead.sum() >= 3 * I["_B"]
    per, grads = device_eval(gpu, I, "embedding")
    gj = grads["joints"].cpu().numpy()
    assert not gj[dead].any() and (np.abs(gj[~dead]).max(axis=-1) > 0).all()
    J = dict(I)
    J["gt_joints"], J["joints"] = I["gt_joints"].copy(), I["joints"].copy()
    J["gt_joints"][dead] = 0.0
    J["joints"][dead] = [7.0, -3.0, 1.0]
    per2, grads2 = device_eval(gpu, J, "embedding")
    assert torch.equal(per, per2) and all(torch.equal(grads[b], grads2[b]) for b in BLOCKS)


# ------------------------------------------------------------------------------------------------- 4. batch independence
@pytest.mark.parametrize("form", ["gmm_merged", "target_last"])
def test_a_frame_does_not_depend_on_its_batch_bitwise(gpu, synth_model, form):
    """Frame 3 of B = 5 (the first wavefront of the second workgroup) against the same frame evaluated alone."""
    I = inputs(synth_model, "full", B=5, seed=8)
    per5, g5 = device_eval(gpu, I, form)
    per1, g1 = device_eval(gpu, I, form, sl=slice(3, 4))
    assert torch.equal(per5[3:4], per1), (per5[3].item(), per1.item())
    for b in BLOCKS:
        assert g1[b].abs().max() > 0 and torch.equal(g5[b][3:4], g1[b]), b


def test_camera_init_frame_does_not_depend_on_its_batch_bitwise(gpu, synth_model):
    from smplifyx_amd import engine
    I = inputs(synth_model, "full", B=5, seed=8)
    K = I["_K"]
    t = lambda n, sl: torch.tensor(I[n][sl], device=gpu)
    count = torch.zeros(K, device=gpu)
    count[[0, 5, 6, 11, 12, 70, 135]] = 1.0
    run = lambda sl: engine.camera_init_eval(*[t(n, sl) for n in ("joints", "rotation", "translation", "focal_x", "focal_y", "center", "gt_joints")],
                                             count, joints_conf=t("joints_conf", sl), est_tz=t("translation", sl)[:, 2].contiguous() + 0.5,
                                             data_weight=1.5, depth_loss_weight=100.0, use_conf=True)
    l5, g5 = run(slice(None))
    l1, g1 = run(slice(3, 4))
    assert torch.equal(l5[3:4], l1) and all(torch.equal(g5[k][3:4], g1[k]) and g1[k].abs().max() > 0 for k in g1)


# ---------------------------------------------------------------------------------------------------- 6. upstream scaling
def test_upstream_weights_scale_the_unit_gradients_bitwise(gpu, synth_model):
    I = inputs(synth_model, "full")
    per, unit = device_eval(gpu, I, "embedding")
    wts = torch.tensor([0.37, -2.5, 11.0], device=gpu)
    per_w, scaled = device_eval(gpu, I, "embedding", upstream=wts)
    assert torch.equal(per, per_w)
    for b in BLOCKS:
        assert torch.equal(scaled[b], unit[b] * wts.reshape([-1] + [1] * (unit[b].dim() - 1))), b


# ------------------------------------------------------------------------------------- 5. two adjoints agree, 7. optimiser
def _model(model, cfg, gpu, **kw):
    from smplifyx_amd import smplx, utils as U
    return smplx.create(model, joint_mapper=U.JointMapper(H.joint_map_for(cfg)), num_betas=cfg["num_betas"],
                        num_expression_coeffs=cfg["num_expression_coeffs"], num_pca_comps=cfg["num_pca_comps"],
                        use_face_contour=cfg["use_face_contour"], create_body_pose=not cfg.get("use_vposer"), **kw).to(gpu)



def _stage_loss(gpu, cfg, w, differentiable):
    from smplifyx_amd import fitting
    mk = _priors()
    loss = fitting.create_loss(loss_type="smplify", rho=cfg["rho"], use_joints_conf=True, use_face=cfg["use_face"],
                               use_hands=cfg["use_hands"], body_pose_prior=mk("l2"), shape_prior=mk("l2"), angle_prior=mk("angle"),
                               expr_prior=mk("l2"), jaw_prior=mk("l2"), left_hand_prior=mk("l2"), right_hand_prior=mk("l2"),
                               interpenetration=False, dtype=torch.float32, num_stages=len(cfg["body_pose_prior_weights"]),
                               differentiable=differentiable).to(gpu)
    loss.reset_loss_weights(w)
    return loss


@pytest.mark.parametrize("which_stage", ["first", "last"])
def test_the_reference_shaped_closure_and_the_engine_closure_agree(gpu, synth_model, which_stage):
    """One frame of the shipped VPoser cfg (fit_smplx_smplifyx.yaml: hands, face, contour, 5 stages) at a far point, two ways:
    (A) the reference's closure body written out -- vposer.decode, body_model(...), loss(...), backward() -- over the three
    differentiable=True objects: autograd chains sfx_vposer_decode_backward, sfx_lbs_backward and the fused loss;
    (B) create_fitting_closure with the default objects: closure_body.h's own adjoint.
    Each within CLOSURE_LOSS_TOL / CLOSURE_GRAD_TOL of the fp64 oracle (whole variable vector, reference order), the two within
    twice that of each other."""
    import test_gpu_parity as T
    from smplifyx_amd import fitting, synthetic, vposer
    from smplifyx_amd.camera import create_camera
    cfg = H.load_cfg("fit_smplx_smplifyx.yaml")
    assert cfg["use_vposer"] and cfg["use_hands"] and cfg["use_face"]
    n_st = len(cfg["body_pose_prior_weights"])
    stage = 0 if which_stage == "first" else n_st - 1
    frames = T.synth_frames(synth_model, cfg, 3)
    frames = {k: (v[:2] if isinstance(v, np.ndarray) else v) for k, v in frames.items()}
    P, est = T.far_points(frames, 2, 5, nemb=32)
    Q = dict(P); Q["est_tz"] = est
    lo, go, _, blocks = T._oracle_closure_blocks(synth_model, cfg, frames, 0, Q, stage, key=(T._cfg_key(cfg), "far", 2, 5))
    # the stage's weights and joint weights, as fit_single_frame.py:553-574 sets them (oracle.fit_frame does the same)
    ff = H.oracle_frame_fit(synth_model, cfg, frames, 0, dtype=torch.float32)
    st = ff.stages[stage]
    w = dict(data_weight=1000.0 / frames["H"], body_pose_weight=float(st["body_pose_weight"]), shape_weight=float(st["shape_weight"]),
             bending_prior_weight=3.17 * float(st["body_pose_weight"]), hand_prior_weight=float(st["hand_prior_weight"]),
             expr_prior_weight=float(st["expr_prior_weight"]), jaw_prior_weight=[float(v) for v in st["jaw_prior_weight"]])
    jw = ff.jw.clone()
    jw[:, ff.nb:ff.nb + 42] = st["hand_weight"]
    jw[:, ff.nb + 42:] = st["face_weight"]
    jw[:, ff.low] = 0
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=gpu)
    kd = t(frames["keypoints"][:1])
    gt, conf, jw = kd[:, :, :2].contiguous(), kd[:, :, 2].reshape(1, -1).contiguous(), jw.to(gpu)
    vpw = synthetic.make_synthetic_vposer(0)
    names = [k for k in P if k not in ("pose_embedding", "cam_translation")]

    def objects(differentiable):
        bm = _model(synth_model, cfg, gpu, vposer=vpw, differentiable=differentiable)
        bm.reset_params(**{k: P[k][:1] for k in names})
        cam = create_camera(focal_length_x=float(frames["focal"]), focal_length_y=float(frames["focal"]), dtype=torch.float32).to(gpu)
        cam.rotation.requires_grad = False
        with torch.no_grad():
            cam.translation[:] = t(P["cam_translation"][:1])
            cam.center[:] = t([frames["W"] * 0.5, frames["H"] * 0.5])
        emb = t(P["pose_embedding"][:1]).requires_grad_(True)
        return bm, cam, emb, _stage_loss(gpu, cfg, w, differentiable)

    # (A) the reference-shaped closure
    bm, cam, emb, loss = objects(True)
    vp = vposer.VPoser(vpw, differentiable=True)
    params = [p for p in bm.parameters() if p.requires_grad] + [emb]
    faces = bm.faces_tensor.view(-1)

    def closure():
        for p in params:
            p.grad = None
        body_pose = vp.decode(emb, output_type="aa").view(1, -1)
        out = bm(return_verts=True, body_pose=body_pose, return_full_pose=True)
        total = loss(out, camera=cam, gt_joints=gt, body_model_faces=faces, joints_conf=conf, joint_weights=jw,
                     pose_embedding=emb, use_vposer=True, stage=stage)
        total.backward()
        return total
    la = closure()
    assert la.dim() == 0
    ga = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params]).cpu().numpy()
    # (B) the engine's closure
    bm2, cam2, emb2, loss2 = objects(False)
    params2 = [p for p in bm2.parameters() if p.requires_grad] + [emb2]
    with fitting.FittingMonitor(**cfg) as monitor:
        c = monitor.create_fitting_closure(None, bm2, camera=cam2, gt_joints=gt, joints_conf=conf, joint_weights=jw, loss=loss2,
                                           use_vposer=True, vposer=vp, pose_embedding=emb2, return_verts=True, return_full_pose=True)
        lb = c(stage=stage)
        if c._fb is not None:
            c._fb.close()
    gb = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params2]).cpu().numpy()
    assert [tuple(p.shape) for p in params] == [tuple(p.shape) for p in params2] and ga.shape == go.shape == gb.shape
    H.assert_blocks_tile(blocks, ga.size)
    label = "objective two-adjoints"
    ea = H.check_closure(label + " autograd", stage, float(la), lo, ga, go)
    eb = H.check_closure(label + " engine", stage, float(lb), lo, gb, go)
    dl = abs(float(la) - float(lb)) / abs(lo)
    dg = float(np.linalg.norm(ga.astype(np.float64) - gb) / np.linalg.norm(go))
    print("stage %d: oracle loss %.6f; autograd path %.2e / %.2e, engine path %.2e / %.2e, between them %.2e / %.2e" %
          ((stage, lo) + ea + eb + (dl, dg)))
    H.check_bound(label, "loss, the two paths", dl, 2 * H.CLOSURE_LOSS_TOL)
    H.check_bound(label, "gradient, the two paths", dg, 2 * H.CLOSURE_GRAD_TOL)


def test_driven_by_the_per_sample_optimiser(gpu, synth_model):
    """LBFGS(per_sample=True).step(closure), B = 3, closure = differentiable model + differentiable loss, per_frame=True:
    step returns the entry losses, and every frame's loss afterwards is strictly lower."""
    from smplifyx_amd.optimizers.lbfgs_ls import LBFGS
    I = inputs(synth_model, "body")
    cfg, B = I["_cfg"], I["_B"]
    bm = _model(synth_model, cfg, gpu, batch_size=B, differentiable=True)
    rng = np.random.RandomState(4)
    P = H.random_params(rng, B, scale=0.3, npca=cfg["num_pca_comps"])
    bm.reset_params(global_orient=P["global_orient"], body_pose=P["pose_embedding"], betas=P["betas"])
    loss = make_loss(gpu, "l2_body_pose", hands=False, face=False)
    cam = make_camera(gpu, I)
    cam.rotation.requires_grad = False
    t = lambda n: torch.tensor(I[n], device=gpu)
    with torch.no_grad():        # detections: the model's own projection at other parameters, so that there is something to fit
        tgt = bm(return_verts=False, global_orient=torch.tensor(P["global_orient"] + 0.1, device=gpu),
                 body_pose=torch.tensor(P["pose_embedding"] * 0.5, device=gpu))
        gt = cam(tgt.joints).contiguous()
    conf, jw = t("joints_conf"), t("joint_weights")
    params = [bm.global_orient, bm.body_pose, bm.betas, cam.translation]

    def evaluate():
        out = bm(return_verts=False, return_full_pose=True)
        return loss(out, camera=cam, gt_joints=gt, joints_conf=conf, joint_weights=jw, use_vposer=False, stage=0, per_frame=True)

    def closure():
        for p in list(bm.parameters()) + list(cam.parameters()):
            p.grad = None
        per = evaluate()
        per.sum().backward()
        return per
    with torch.no_grad():
        before = evaluate().clone()
    opt = LBFGS(params, line_search_fn="strong_Wolfe", per_sample=True, lr=1.0, max_iter=10)
    entry = opt.step(closure)
    with torch.no_grad():
        after = evaluate()
    assert tuple(entry.shape) == (B,) and torch.equal(entry, before), (entry, before)
    assert (after < entry).all(), (entry, after)


# ------------------------------------------------------------------------------------------------ 8. interpenetration
def test_interpenetration_is_composed_from_the_stand_alone_modules(gpu):
    """total(w) - total(0) = w x pen_distance(triangles, filter(search_tree(triangles))) called directly, and the vertices'
    gradient of that difference is the direct call's -- on a self-colliding pose of the synthetic surface mesh (the recipe of
    test_gpu_dropin.test_create_loss_with_interpenetration_objects)."""
    from smplifyx_amd import synthetic
    from smplifyx_amd.mesh_intersection.bvh_search_tree import BVH
    import smplifyx_amd.mesh_intersection.loss as collisions_loss
    from smplifyx_amd.mesh_intersection.filter_faces import FilterFaces
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False, interpenetration=True)
    cfg["df_cone_height"] = 1e-2
    model = synthetic.make_synthetic_model(0, surface=True)
    parts = synthetic.make_synthetic_parts(model)
    K = len(H.joint_map_for(cfg))
    frames = synthetic.make_frames(1, H.oracle_joints_fn(model, cfg), K, focal=5000.0)
    rng = np.random.RandomState(3)
    pose = (frames["reg_pose"][:1] + 0.3 * rng.normal(size=(1, 63))).astype(np.float32)      # bent enough to collide
    # float64 containers: the total is then summed in double, so that total(w) - total(0) keeps the term's own digits beside a
    # data term many orders larger (the device arithmetic is fp32 either way)
    bm = _model(model, cfg, gpu, differentiable=True, dtype=torch.float64)
    bm.reset_params(global_orient=frames["reg_global"][:1], body_pose=pose)
    search_tree = BVH(max_collisions=cfg["max_collisions"])
    pen_distance = collisions_loss.DistanceFieldPenetrationLoss(sigma=cfg["df_cone_height"], point2plane=False, vectorized=True,
                                                                penalize_outside=cfg["penalize_outside"])
    filter_faces = FilterFaces(faces_segm=parts["segm"], faces_parents=parts["parents"], ign_part_pairs=cfg["ign_part_pairs"]).to(gpu)
    I = inputs(model, "body", B=1, seed=6)
    cam = make_camera(gpu, I)
    t = lambda n: torch.tensor(I[n], device=gpu)
    faces = bm.faces_tensor.view(-1)
    CW = 0.75

    def total(cw):
        loss = make_loss(gpu, "l2_body_pose", hands=False, face=False, interpenetration=True, search_tree=search_tree,
                         pen_distance=pen_distance, tri_filtering_module=filter_faces)
        loss.reset_loss_weights({"coll_loss_weight": cw})
        out = bm(return_verts=True, return_full_pose=True)
        out.vertices.retain_grad()
        v = loss(out, camera=cam, gt_joints=t("gt_joints"), body_model_faces=faces, joints_conf=t("joints_conf"),
                 joint_weights=t("joint_weights"), use_vposer=False, stage=0)
        v.backward()
        dv = out.vertices.grad
        return v.detach(), (dv.clone() if dv is not None else torch.zeros_like(out.vertices)), out.vertices.detach()
    l1, dv1, verts = total(CW)
    l0, dv0, _ = total(0.0)
    v = verts.clone().requires_grad_(True)
    triangles = torch.index_select(v, 1, faces).view(1, -1, 3, 3)
    with torch.no_grad():
        idx = search_tree(triangles)
    idx = filter_faces(idx)
    n_pairs = int(idx.ge(0).all(-1).sum())
    assert n_pairs > 0, "no colliding pair survives the filter: the pose of this test no longer collides -- the test checks nothing"
    direct = pen_distance(triangles, idx).sum()
    direct.backward()
    print("pairs kept %d; direct term %.6e; total(w) - total(0) = %.6e" % (n_pairs, float(direct), float(l1 - l0)))
    assert float(direct) > 0
    assert l1.dtype == torch.float64 and float(l0) > 0
    assert abs(float(l1 - l0) - CW * float(direct)) <= 1e-6 * abs(CW * float(direct))
    want = CW * v.grad
    assert torch.allclose(dv1 - dv0, want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
    assert (dv1 - dv0).abs().max() > 0


# ----------------------------------------------------------------------------------------------------------- 9. surface
def test_float64_containers(gpu, synth_model):
    I = inputs(synth_model, "full")
    per, g = device_eval(gpu, I, "embedding")
    per64, g64 = device_eval(gpu, I, "embedding", dtype=torch.float64)
    assert per64.dtype == torch.float64 and torch.equal(per64, per.double())
    for b in BLOCKS:
        assert g64[b].dtype == torch.float64 and torch.equal(g64[b], g[b].double()), b


class _OwnPrior(torch.nn.Module):
    """A caller's prior: one value per frame, not a class of this package."""

    def forward(self, x, *args):
        return (x ** 4).sum(-1) + x.abs().sum(-1)


def test_a_callers_own_prior_module_is_added_in_torch(gpu, synth_model):
    I = inputs(synth_model, "full")
    base, gb = device_eval(gpu, I, "embedding")
    loss = make_loss(gpu, "embedding", I, shape_prior=_OwnPrior(), expr_prior=_OwnPrior())
    ref = make_loss(gpu, "embedding", I)
    ref.reset_loss_weights({"shape_weight": 0.0, "expr_prior_weight": 0.0})
    res = []
    for m in (loss, ref):
        cam = make_camera(gpu, I)
        out, leaf, emb, vp = make_output(gpu, I, "embedding")
        t = lambda n: torch.tensor(I[n], device=gpu)
        per = m(out, camera=cam, gt_joints=t("gt_joints"), joints_conf=t("joints_conf"), joint_weights=t("joint_weights"),
                use_vposer=True, pose_embedding=emb, stage=0, per_frame=True)
        per.sum().backward()
        res.append((per.detach(), leaf))
    (per, leaf), (per0, leaf0) = res
    b, e = torch.tensor(I["betas"], device=gpu, requires_grad=True), torch.tensor(I["expression"], device=gpu, requires_grad=True)
    own = _OwnPrior()
    extra = own(b) * WEIGHTS["shape_weight"] ** 2 + own(e) * WEIGHTS["expr_prior_weight"] ** 2
    extra.sum().backward()
    assert float(extra.min()) > 0
    assert torch.allclose(per, per0 + extra.detach(), rtol=1e-6, atol=0)
    assert torch.allclose(leaf["betas"].grad, b.grad, rtol=1e-6) and torch.allclose(leaf["expression"].grad, e.grad, rtol=1e-6)
    for k in ("joints", "prior", "body_pose", "jaw_pose", "left_hand_pose"):      # the fused terms are untouched
        assert torch.equal(leaf[k].grad, leaf0[k].grad) and torch.equal(leaf[k].grad, gb[k]), k


def test_wrong_shapes_are_value_errors(gpu, synth_model):
    from smplifyx_amd import engine, fitting, smplx
    I = inputs(synth_model, "body")
    B, K = I["_B"], I["_K"]
    loss = make_loss(gpu, "embedding", I, hands=False, face=False)
    cam = make_camera(gpu, I)
    t = lambda n: torch.tensor(I[n], device=gpu)

    def call(out, emb, gt=None, conf=None):
        return loss(out, camera=cam, gt_joints=t("gt_joints") if gt is None else gt, joints_conf=t("joints_conf") if conf is None else conf,
                    joint_weights=t("joint_weights"), use_vposer=True, pose_embedding=emb, stage=0)
    out, leaf, emb, _ = make_output(gpu, I, "embedding")
    assert torch.isfinite(call(out, emb))
    with pytest.raises(ValueError, match="gt_joints"):           # K of the detections differs from the joints'
        call(out, emb, gt=t("gt_joints")[:, :K - 1].contiguous())
    with pytest.raises(ValueError, match="joints_conf"):
        call(out, emb, conf=torch.ones(B, K + 1, device=gpu))
    big = engine.OBJECTIVE_MAX_K + 1
    assert engine.OBJECTIVE_MAX_K >= 144
    out_big = smplx.ModelOutput(joints=torch.zeros(B, big, 3, device=gpu), betas=leaf["betas"], body_pose=leaf["body_pose"],
                                full_pose=out.full_pose)
    with pytest.raises(ValueError, match="supported 1.."):
        call(out_big, emb, gt=torch.zeros(B, big, 2, device=gpu), conf=torch.ones(B, big, device=gpu))
    cam_loss = fitting.create_loss("camera_init", init_joints_idxs=[0, 1, K + 3], differentiable=True).to(gpu)
    with pytest.raises(ValueError, match="init_joints_idxs"):
        cam_loss(out, camera=cam, gt_joints=t("gt_joints"))
    # the library refuses by itself what the wrappers check first: error code and text
    import ctypes as C
    from smplifyx_amd import _capi
    lib = _capi.load()
    a, c = _capi.ObjectiveIn(), _capi.ObjectiveCfg()
    buf = torch.zeros(4096, device=gpu)
    for name in _capi.OBJECTIVE_INPUTS:
        setattr(a, name + "_dev", buf.data_ptr())
    a.n_prior, a.num_betas, a.num_expr = 32, 10, 10
    for Bk, Kk, word in ((0, 26, "B = 0"), (1, 0, "K = 0"), (1, big, "K = %d" % big)):
        a.B, a.K = Bk, Kk
        assert lib.sfx_objective_eval(C.byref(c), C.byref(a), None, C.c_void_p(buf.data_ptr()), None) == -1
        assert word in lib.sfx_last_error().decode()
    a.B, a.K, a.n_prior = 1, 26, 62
    c.prior_form, c.gmm_M, c.gmm_D = 3, 8, 62
    c.gmm_means_dev = c.gmm_precisions_dev = c.gmm_nll_weights_dev = buf.data_ptr()
    assert lib.sfx_objective_eval(C.byref(c), C.byref(a), None, C.c_void_p(buf.data_ptr()), None) == -1
    assert "mixture dimension 62" in lib.sfx_last_error().decode()


def test_second_derivatives_are_refused(gpu, synth_model):
    I = inputs(synth_model, "body")
    loss = make_loss(gpu, "embedding", I, hands=False, face=False)
    cam = make_camera(gpu, I)
    out, leaf, emb, _ = make_output(gpu, I, "embedding")
    t = lambda n: torch.tensor(I[n], device=gpu)
    total = loss(out, camera=cam, gt_joints=t("gt_joints"), joints_conf=t("joints_conf"), joint_weights=t("joint_weights"),
                 use_vposer=True, pose_embedding=emb, stage=0)
    with pytest.raises(RuntimeError, match="first derivatives only"):
        total.backward(create_graph=True)


def test_the_default_objects_are_unchanged(gpu, synth_model):
    """differentiable=False: no graph, and forward IS _standalone_loss (the parent commit's forward), for both losses."""
    from smplifyx_amd import fitting
    I = inputs(synth_model, "body")
    cfg, K = I["_cfg"], I["_K"]
    bm = _model(synth_model, cfg, gpu)
    rng = np.random.RandomState(2)
    P = H.random_params(rng, 1, scale=0.3, npca=cfg["num_pca_comps"])
    bm.reset_params(global_orient=P["global_orient"], body_pose=P["pose_embedding"], betas=P["betas"])
    cam = make_camera(gpu, I, slice(0, 1))
    t = lambda n: torch.tensor(I[n][:1], device=gpu)
    out = bm(return_verts=True, return_full_pose=True)
    loss = make_loss(gpu, "l2_body_pose", hands=False, face=False, differentiable=False)
    assert loss.differentiable is False
    v = loss(out, camera=cam, gt_joints=t("gt_joints"), joints_conf=t("joints_conf"), joint_weights=t("joint_weights"),
             use_vposer=False, pose_embedding=bm.body_pose, stage=0)
    ref = fitting._standalone_loss(loss, out, cam, t("gt_joints"), t("joints_conf"), t("joint_weights"), False, bm.body_pose, 0)
    assert v.dim() == 0 and not v.requires_grad and v.grad_fn is None and torch.equal(v, ref) and float(v) > 0
    cam_loss = fitting.create_loss("camera_init", init_joints_idxs=torch.tensor([0, 5, 6, 11, 12]), trans_estimation=None,
                                   joints_conf=t("joints_conf"), use_conf=True).to(gpu)
    assert cam_loss.differentiable is False
    vc = cam_loss(out, camera=cam, gt_joints=t("gt_joints"))
    refc = fitting._standalone_loss(cam_loss, out, cam, t("gt_joints"), None, None, False, None, 0)
    assert not vc.requires_grad and torch.equal(vc, refc) and float(vc) > 0


def test_weights_reset_between_evaluations_are_the_ones_used(gpu, synth_model):
    """reset_loss_weights replaces the weight buffers; the loss keeps a read-back of them so that an evaluation pays no
    synchronisation per weight.  Many resets of SUBSETS of the weights, each followed by an evaluation, against a module built
    afresh with the same weights: the same bits (a read-back keyed by the buffers' addresses went stale here)."""
    I = inputs(synth_model, "body")
    rng = np.random.RandomState(12)
    loss = make_loss(gpu, "embedding", I, hands=False, face=False)
    cam = make_camera(gpu, I)
    t = lambda n: torch.tensor(I[n], device=gpu)
    gt, conf, jw = t("gt_joints"), t("joints_conf"), t("joint_weights")

    def value(m):
        out, leaf, emb, _ = make_output(gpu, I, "embedding")
        with torch.no_grad():
            return m(out, camera=cam, gt_joints=gt, joints_conf=conf, joint_weights=jw, use_vposer=True, pose_embedding=emb, stage=0)
    current = {k: WEIGHTS[k] for k in ("data_weight", "body_pose_weight", "shape_weight", "bending_prior_weight")}
    names = sorted(current)
    seen = set()
    for step in range(120):
        sub = [n for n in names if rng.rand() < 0.5] or [names[step % 4]]
        new = {n: float(np.float32(rng.uniform(0.1, 30.0))) for n in sub}
        loss.reset_loss_weights(new)
        current.update(new)
        got = value(loss)
        fresh = make_loss(gpu, "embedding", I, hands=False, face=False)
        fresh.reset_loss_weights(current)
        want = value(fresh)
        assert torch.equal(got, want), (step, sub, float(got), float(want))
        seen.add(float(got))
    assert len(seen) == 120


def test_host_tensors_are_refused_not_copied(gpu, synth_model):
    """Every tensor the loss reads must be on the device: a CPU joints_conf, joint_weights, regression target or camera is a
    RuntimeError naming the missing CPU fallback, not a silent copy per evaluation."""
    I = inputs(synth_model, "body")
    t = lambda n: torch.tensor(I[n], device=gpu)

    def call(loss, cam, **over):
        out, leaf, emb, _ = make_output(gpu, I, "embedding")
        kw = dict(camera=cam, gt_joints=t("gt_joints"), joints_conf=t("joints_conf"), joint_weights=t("joint_weights"),
                  use_vposer=True, pose_embedding=emb, stage=NUM_STAGES - 1)
        kw.update(over)
        return loss(out, **kw)
    loss = make_loss(gpu, "embedding", I, hands=False, face=False)
    assert torch.isfinite(call(loss, make_camera(gpu, I)))
    for name in ("joints_conf", "joint_weights", "gt_joints"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(loss, make_camera(gpu, I), **{name: torch.tensor(I[name])})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(loss, make_camera(gpu, I), pose_embedding=torch.tensor(I["embedding"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(loss, make_camera(gpu, I).cpu())
    reg = make_loss(gpu, "target_last", I, hands=False, face=False)
    reg.regression_pose = torch.tensor(I["target"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(reg, make_camera(gpu, I))
    # detections made for ONE frame are not spread over a batch without a word
    with pytest.raises(ValueError, match="gt_joints"):
        call(loss, make_camera(gpu, I), gt_joints=t("gt_joints")[:1].contiguous())
    # a row of joint weights and a camera made for one frame serve the batch (fit_single_frame.py:285-287, camera.py:35)
    a = call(loss, make_camera(gpu, I, slice(0, 1)), joint_weights=t("joint_weights")[:1].contiguous())
    I1 = dict(I)
    for k in ("rotation", "translation", "focal_x", "focal_y", "center"):
        I1[k] = np.repeat(I[k][:1], I["_B"], 0)
    assert torch.equal(a, call(loss, make_camera(gpu, I1)))
