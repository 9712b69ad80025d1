"""GPU tests of the stand-alone VPoser decoder (sfx_vposer_*, engine.VPoserDecoder, smplifyx_amd.vposer.VPoser): the tile kernels
k_vposer_decode16 / k_vposer_decode16_bwd of csrc/vposer_batch.hip.

Inputs.  Weights synthetic.make_synthetic_vposer(0, latent=L), L = 32 and 12 (12: a hard-coded 32 would show).  Draws:
RandomState(13), z = normal(37, L) as float32, then dbody = normal(37, 63).  B in {1, 16, 17, 37} as leading rows: a tile with 15
empty rows, exactly one tile, a full tile plus a one-row tile, two full tiles plus five rows.

Reference and yardstick (as tests/test_gpu_lbs_backward.py).  Reference: oracle.vposer.VPoserRef in float64 with torch
autograd.  Error measure: ||x - x64|| / ||x64||, per frame and over the batch.  Yardstick: the SAME oracle in float32 against its
float64 run at the same points, computed here.  Bound: 10 x the yardstick of the same quantity -- the margin tests/helpers.py
states for its own bounds, applied to the reference's own rounding because the device sums in another order.  Over the batch the
yardstick is the float32 oracle's error over the same B rows.  Per frame it is the float32 oracle's WORST single frame among the
37 draws, one number per quantity and L: one frame's float32 error is a draw from a distribution (it can come out several times
below its neighbours' by luck), the worst of 37 is the level of the reference's own per-frame rounding, and it does not depend
on anything the device computes.  Every float64 norm is >= 0.1 (asserted), so no relative error is measured against noise.

Conditions on the inputs, asserted on the float64 run, so that no kink decides a comparison: every hidden pre-activation of both
layers has |value| >= 1e-5 (a leaky_relu sign that differs between precisions changes dz by ~1/512 relative, which no rounding
bound covers; float32 sums of 512 O(1) terms are off by ~1e-6), and every decoded joint angle is < 1.5 rad (both precisions
take the same quaternion branch).  At these draws: min |pre-activation| 3.3e-5 (L = 32) / 4.5e-5 (L = 12), max angle 1.46 / 1.37 rad.

Observed on MI355X (the session summary prints every comparison next to its bound): body_pose <= 6.6e-7 over a batch and <= 1.0e-6
for a single frame (yardsticks of the same run 3.8e-7 .. 5.5e-7 and 5.4e-7 / 6.4e-7); dz <= 8.9e-7 and <= 1.7e-6 (yardsticks
4.2e-7 .. 7.0e-7 and 6.2e-7 / 1.2e-6): every comparison at about 1 .. 2 x its own yardstick.  In-loop against stand-alone decoder 7.1e-7;
the latent chain through the differentiable model 9.8e-7 at a yardstick of 7.4e-7.
"""
import numpy as np
import pytest
import torch

import helpers as H
from smplifyx_amd import synthetic

pytestmark = pytest.mark.gpu

LATENTS = (32, 12)
BATCHES = (1, 16, 17, 37)
N = 37
FACTOR = 10.0
MIN_NORM = 0.1


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    return torch.device("cuda:0")


def _rel(a, ref):
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / np.linalg.norm(ref))


def _rel_rows(a, ref):
    a = np.asarray(a, np.float64)
    return np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)


def _oracle(w, z, dbody, dtype):
    from oracle.vposer import VPoserRef
    vp = VPoserRef(w, dtype)
    zt = torch.tensor(z, dtype=dtype, requires_grad=True)
    body = vp.decode(zt).reshape(z.shape[0], 63)
    (body * torch.tensor(dbody, dtype=dtype)).sum().backward()
    return body.detach().double().numpy(), zt.grad.double().numpy()


_REF = {}


def reference(L):
    """Weights, draws, float64 reference, float32 yardsticks of one latent size (computed once, never modified)."""
    if L not in _REF:
        w = synthetic.make_synthetic_vposer(0, latent=L)
        rng = np.random.RandomState(13)
        z = rng.normal(size=(N, L)).astype(np.float32)
        dbody = rng.normal(size=(N, 63)).astype(np.float32)
        b64, g64 = _oracle(w, z, dbody, torch.float64)
        b32, g32 = _oracle(w, z, dbody, torch.float32)
        # the conditions of the module docstring, on the float64 run
        f = lambda k: np.asarray(w[k], np.float64)
        p1 = z.astype(np.float64) @ f("fc1_w").T + f("fc1_b")
        p2 = np.where(p1 > 0, p1, 0.2 * p1) @ f("fc2_w").T + f("fc2_b")
        min_pre = float(min(np.abs(p1).min(), np.abs(p2).min()))
        max_angle = float(np.linalg.norm(b64.reshape(N, 21, 3), axis=-1).max())
        print("L=%d: min |pre-activation| %.2e, max joint angle %.3f rad" % (L, min_pre, max_angle))
        assert min_pre >= 1e-5, (L, min_pre)
        assert max_angle < 1.5, (L, max_angle)
        norms = dict(body=np.linalg.norm(b64, axis=1), dz=np.linalg.norm(g64, axis=1))
        for k, v in norms.items():
            assert v.min() >= MIN_NORM, (L, k, float(v.min()))
        yard = dict(body_frame=float(_rel_rows(b32, b64).max()), dz_frame=float(_rel_rows(g32, g64).max()))
        for B in BATCHES:
            yard["body", B] = _rel(b32[:B], b64[:B])
            yard["dz", B] = _rel(g32[:B], g64[:B])
        print("L=%d: yardstick body_pose batch(37) %.2e worst frame %.2e; dz batch(37) %.2e worst frame %.2e; min fp64 norms %.2f / %.2f"
              % (L, yard["body", N], yard["body_frame"], yard["dz", N], yard["dz_frame"], norms["body"].min(), norms["dz"].min()))
        for a in (z, dbody, b64, g64):
            a.setflags(write=False)
        _REF[L] = dict(w=w, z=z, dbody=dbody, b64=b64, g64=g64, yard=yard)
    return _REF[L]


_DEC = {}


def decoder(L, gpu):
    from smplifyx_amd import engine
    if L not in _DEC:
        _DEC[L] = engine.VPoserDecoder(reference(L)["w"])
    return _DEC[L]


def _check(label, what, got, ref, y_batch, y_frame):
    assert got.shape == ref.shape and np.isfinite(got).all()
    per = _rel_rows(got, ref)
    whole = _rel(got, ref)
    print("%-22s %-10s batch %.2e (yardstick %.2e, bound %.2e)  worst frame %.2e (yardstick %.2e, bound %.2e)"
          % (label, what, whole, y_batch, FACTOR * y_batch, per.max(), y_frame, FACTOR * y_frame))
    H.check_bound(label, what + " batch", whole, FACTOR * y_batch)
    H.check_bound(label, what + " worst frame", float(per.max()), FACTOR * y_frame)


@pytest.mark.parametrize("L", LATENTS)
@pytest.mark.parametrize("B", BATCHES)
def test_decode_matches_the_float64_oracle(gpu, L, B):
    R = reference(L)
    body = decoder(L, gpu).decode(torch.tensor(R["z"][:B], device=gpu))
    assert body.shape == (B, 63) and body.dtype == torch.float32
    _check("vposer-decode L=%d" % L, "B=%d" % B, body.cpu().numpy(), R["b64"][:B], R["yard"]["body", B], R["yard"]["body_frame"])


@pytest.mark.parametrize("L", LATENTS)
@pytest.mark.parametrize("B", BATCHES)
def test_decode_backward_matches_float64_autograd_of_the_oracle(gpu, L, B):
    R = reference(L)
    t = lambda a: torch.tensor(a[:B], device=gpu)
    dz = decoder(L, gpu).decode_backward(t(R["z"]), t(R["dbody"]))
    assert dz.shape == (B, L) and dz.dtype == torch.float32
    _check("vposer-backward L=%d" % L, "B=%d" % B, dz.cpu().numpy(), R["g64"][:B], R["yard"]["dz", B], R["yard"]["dz_frame"])


@pytest.mark.parametrize("L", LATENTS)
def test_a_frame_does_not_depend_on_its_batch_bitwise(gpu, L):
    """Frame i of the B = 37 call = the same latent decoded alone (row 0 of a one-row tile) = its value when the 37 rows are
    passed in reversed order (another tile and another row), for decode and decode_backward."""
    R = reference(L)
    dec = decoder(L, gpu)
    z, db = torch.tensor(R["z"], device=gpu), torch.tensor(R["dbody"], device=gpu)
    body, dz = dec.decode(z), dec.decode_backward(z, db)
    assert torch.isfinite(body).all() and torch.isfinite(dz).all() and body.abs().max() > 0 and dz.abs().max() > 0
    body_r, dz_r = dec.decode(z.flip(0)), dec.decode_backward(z.flip(0), db.flip(0))
    assert torch.equal(body_r.flip(0), body), float((body_r.flip(0) - body).abs().max())
    assert torch.equal(dz_r.flip(0), dz), float((dz_r.flip(0) - dz).abs().max())
    for i in range(N):
        b1, g1 = dec.decode(z[i:i + 1]), dec.decode_backward(z[i:i + 1], db[i:i + 1])
        assert torch.equal(b1[0], body[i]), (i, float((b1[0] - body[i]).abs().max()))
        assert torch.equal(g1[0], dz[i]), (i, float((g1[0] - dz[i]).abs().max()))


@pytest.mark.parametrize("L", LATENTS)
@pytest.mark.parametrize("B", (1, 17))
def test_nothing_is_stored_beyond_B(gpu, L, B):
    R = reference(L)
    dec = decoder(L, gpu)
    z, db = torch.tensor(R["z"][:B], device=gpu), torch.tensor(R["dbody"][:B], device=gpu)
    sentinel = -12345.5
    body = torch.full([B + 1, 63], sentinel, device=gpu)
    dz = torch.full([B + 1, L], sentinel, device=gpu)
    dec.decode(z, out=body[:B])
    dec.decode_backward(z, db, out=dz[:B])
    assert (body[B] == sentinel).all() and (dz[B] == sentinel).all()
    assert torch.equal(body[:B], dec.decode(z)) and torch.equal(dz[:B], dec.decode_backward(z, db))
    assert (body[:B] != sentinel).all() and (dz[:B] != sentinel).all()
    # B = 0: no launch, empty results
    assert dec.decode(z[:0]).shape == (0, 63) and dec.decode_backward(z[:0], db[:0]).shape == (0, L)


def test_torch_surface(gpu):
    from smplifyx_amd.vposer import VPoser
    R = reference(32)
    B = 17
    vp = VPoser(R["w"]).to(gpu).eval()
    assert vp.latentD == 32
    db = torch.tensor(R["dbody"][:B], device=gpu)
    z = torch.tensor(R["z"][:B], device=gpu, requires_grad=True)
    out = vp.decode(z, output_type="aa")
    assert out.shape == (B, 1, 21, 3) and out.dtype == torch.float32 and out.requires_grad
    assert out.view(B, -1).shape == (B, 63)
    (out * db.view(B, 1, 21, 3)).sum().backward()
    ref = decoder(32, gpu).decode_backward(z.detach(), db)
    assert z.grad is not None and z.grad.dtype == torch.float32 and torch.equal(z.grad, ref)
    assert torch.equal(out.detach().view(B, 63), decoder(32, gpu).decode(z.detach()))
    with torch.no_grad():
        assert not vp.decode(z).requires_grad
    z64 = torch.tensor(R["z"][:B], device=gpu, dtype=torch.float64, requires_grad=True)
    o64 = vp.decode(z64)
    assert o64.dtype == torch.float64
    (o64 * db.double().view(B, 1, 21, 3)).sum().backward()
    assert z64.grad.dtype == torch.float64 and torch.equal(z64.grad, ref.double())
    with pytest.raises(ValueError, match="matrot"):
        vp.decode(z, output_type="matrot")
    dec = decoder(32, gpu)
    with pytest.raises(ValueError, match="z"):
        dec.decode(torch.zeros(3, 31, device=gpu))
    with pytest.raises(ValueError, match="dbody"):
        dec.decode_backward(z.detach(), db[:B - 1])
    vp.close()


def test_refused_outputs_and_devices(gpu):
    """`out` is written through a raw pointer with B and the width the call works out: anything but a contiguous float32
    tensor of exactly that shape is a ValueError.  The handle lives on one device: a latent elsewhere is refused, not
    dereferenced."""
    L, B = 12, 2
    R = reference(L)
    dec = decoder(L, gpu)
    z, db = torch.tensor(R["z"][:B], device=gpu), torch.tensor(R["dbody"][:B], device=gpu)
    for call, n in ((lambda out: dec.decode(z, out=out), 63), (lambda out: dec.decode_backward(z, db, out=out), L)):
        for bad in (torch.empty(B, n - 1, device=gpu), torch.empty(B + 1, n, device=gpu), torch.empty(B * n, device=gpu),
                    torch.empty(B, n, dtype=torch.float64, device=gpu), torch.empty(n, B, device=gpu).t(), torch.empty(B, n)):
            with pytest.raises(ValueError, match="out: a contiguous float32"):
                call(bad)
        mine = torch.empty(B, n, device=gpu)
        assert call(mine) is mine
    assert dec.device_index == gpu.index
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="decoder's weights on cuda:0"):
            dec.decode(z.to("cuda:1"))
        with pytest.raises(ValueError, match="decoder's weights on cuda:0"):
            dec.decode_backward(z.to("cuda:1"), db.to("cuda:1"))


def test_agrees_with_the_in_loop_decoder(gpu, synth_model):
    """A use_vposer FrameBatch decodes its accepted latents with the closure workgroup (csrc/vposer.h, sfx_batch_get_params);
    the stand-alone decode of the same latents is another fp32 evaluation with another summation tree.  Each is within test
    1's bound of the float64 oracle, so they differ by at most 2 x 10 x the yardstick."""
    import test_gpu_parity as T
    from smplifyx_amd import engine
    R = reference(32)
    B = 3
    cfg = H.load_cfg("fit_smplx_combined_vposer_coco25.yaml", use_hands=False, use_face=False)
    dm = T._dm(synth_model, cfg, vposer=R["w"])
    fb = engine.FrameBatch(dm, B, cfg, lbs_mode="rows", has_regression_pose=False)
    K = dm.K
    fb.set_frames(np.zeros((B, K, 3), np.float32), np.ones((B, K), np.float32), np.zeros((B, K), np.float32), 5000.0,
                  np.tile([400.0, 300.0], (B, 1)).astype(np.float32), 1000.0 / 600)
    fb.set_params(pose_embedding=R["z"][:B].copy(), global_orient=np.zeros((B, 3), np.float32),
                  cam_translation=np.tile([0.0, 0.0, 20.0], (B, 1)).astype(np.float32))
    inloop = fb.get_params()["body_pose"]
    alone = decoder(32, gpu).decode(torch.tensor(R["z"][:B], device=gpu)).cpu().numpy()
    ref = R["b64"][:B]
    assert np.isfinite(inloop).all() and np.abs(inloop).max() > 0
    y_batch = _rel(_oracle(R["w"], R["z"][:B], R["dbody"][:B], torch.float32)[0], ref)
    whole = float(np.linalg.norm(inloop.astype(np.float64) - alone) / np.linalg.norm(ref))
    per = np.linalg.norm(inloop.astype(np.float64) - alone, axis=1) / np.linalg.norm(ref, axis=1)
    print("in-loop vs stand-alone: batch %.2e (bound %.2e), worst frame %.2e (bound %.2e)"
          % (whole, 2 * FACTOR * y_batch, per.max(), 2 * FACTOR * R["yard"]["body_frame"]))
    H.check_bound("vposer in-loop vs alone", "batch", whole, 2 * FACTOR * y_batch)
    H.check_bound("vposer in-loop vs alone", "worst frame", float(per.max()), 2 * FACTOR * R["yard"]["body_frame"])
    fb.close()
    dm.close()


def _body_cfg():
    return H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False)


def _module(model, cfg, gpu, **kw):
    from smplifyx_amd import smplx, utils as U
    jm = U.JointMapper(H.joint_map_for(cfg))
    return smplx.create(model, joint_mapper=jm, num_betas=cfg["num_betas"], num_expression_coeffs=cfg["num_expression_coeffs"],
                        num_pca_comps=cfg["num_pca_comps"], use_face_contour=cfg["use_face_contour"], **kw).to(gpu)


def test_latent_gradient_through_decode_and_the_differentiable_model(gpu, synth_model):
    """pose_embedding -> VPoser.decode -> SMPLX(differentiable=True)(body_pose=...) -> sum(dj * joints) + sum(dv * vertices):
    pose_embedding.grad against float64 autograd of VPoserRef + the oracle body model; bound 10 x the float32 oracle's own
    error for this chain (computed here), relative 2-norm over the whole gradient."""
    from oracle.vposer import VPoserRef
    from smplifyx_amd.vposer import VPoser
    R = reference(32)
    B = 2
    cfg = _body_cfg()
    rng = np.random.RandomState(17)
    P = H.random_params(rng, B, scale=0.5, npca=cfg["num_pca_comps"])
    P.pop("pose_embedding")
    V, K = np.asarray(synth_model["v_template"]).shape[0], len(H.joint_map_for(cfg))
    dv = rng.normal(size=(B, V, 3)).astype(np.float32)
    dj = rng.normal(size=(B, K, 3)).astype(np.float32)
    z = R["z"][:B]

    def oracle(dtype):
        vp, bm = VPoserRef(R["w"], dtype), H.oracle_model(synth_model, cfg, dtype)
        zt = torch.tensor(z, dtype=dtype, requires_grad=True)
        loss = 0
        for i in range(B):
            bm.reset_params(**{k: v[i:i + 1] for k, v in P.items()})
            o = bm(return_verts=True, body_pose=vp.decode(zt[i:i + 1]).view(1, -1))
            loss = loss + (torch.as_tensor(dv[i:i + 1], dtype=dtype) * o.vertices).sum() + (torch.as_tensor(dj[i:i + 1], dtype=dtype) * o.joints).sum()
        loss.backward()
        return zt.grad.double().numpy()

    g64, g32 = oracle(torch.float64), oracle(torch.float32)
    yard = _rel(g32, g64)
    assert np.linalg.norm(g64, axis=1).min() >= MIN_NORM
    vp = VPoser(R["w"]).to(gpu).eval()
    bm = _module(synth_model, cfg, gpu, batch_size=B, differentiable=True)
    bm.reset_params(**P)
    zt = torch.tensor(z, device=gpu, requires_grad=True)
    out = bm(return_verts=True, body_pose=vp.decode(zt, output_type="aa").view(B, -1))
    ((out.vertices * torch.tensor(dv, device=gpu)).sum() + (out.joints * torch.tensor(dj, device=gpu)).sum()).backward()
    assert zt.grad is not None and zt.grad.shape == (B, 32) and torch.isfinite(zt.grad).all()
    err = _rel(zt.grad.cpu().numpy(), g64)
    print("latent chain: |g64| %.3e  device %.2e  yardstick %.2e  bound %.2e" % (np.linalg.norm(g64), err, yard, FACTOR * yard))
    H.check_bound("vposer latent chain", "d pose_embedding", err, FACTOR * yard)
    vp.close()


def test_guess_init_with_the_vposer_object(gpu, synth_model):
    from smplifyx_amd import fitting
    from smplifyx_amd.vposer import VPoser
    R = reference(32)
    cfg = _body_cfg()
    vp = VPoser(R["w"]).to(gpu).eval()
    bm = _module(synth_model, cfg, gpu, batch_size=1)
    K = len(H.joint_map_for(cfg))
    j2d = torch.tensor(np.random.RandomState(19).uniform(100, 500, size=(1, K, 2)).astype(np.float32), device=gpu)
    z = torch.tensor(R["z"][:1], device=gpu, requires_grad=True)
    t_vp = fitting.guess_init(bm, j2d, cfg["body_tri_idxs"], use_vposer=True, vposer=vp, pose_embedding=z, model_type="smplx",
                              focal_length=5000.0)
    body = vp.decode(z.detach(), output_type="aa").view(1, -1)
    t_aa = fitting.guess_init(bm, j2d, cfg["body_tri_idxs"], use_vposer=False, pose_embedding=body, model_type="smplx",
                              focal_length=5000.0)
    assert t_vp.shape == (1, 3) and torch.isfinite(t_vp).all() and float(t_vp[0, 2]) > 0
    assert torch.equal(t_vp, t_aa)
    vp.close()


def test_fitting_closure_takes_its_weights_from_the_vposer_object(gpu, synth_model):
    """create_fitting_closure(use_vposer=True, vposer=VPoser(w)) on a model created WITHOUT vposer= evaluates (it used to end in
    'use_vposer without sfx_model_set_vposer') and equals the closure on a model created with vposer=w, bit for bit."""
    import test_gpu_dropin as D
    from smplifyx_amd import fitting, prior
    from smplifyx_amd.vposer import VPoser
    R = reference(32)
    cfg = H.load_cfg("fit_smplx_combined_vposer_coco25.yaml", use_hands=False, use_face=False)
    cfg["use_camera_prior"] = False
    K = len(H.joint_map_for(cfg))
    rng = np.random.RandomState(23)
    kd = torch.tensor(np.concatenate([rng.uniform(100, 500, size=(1, K, 2)), rng.uniform(0.5, 1.0, size=(1, K, 1))], -1).astype(np.float32),
                      device=gpu)
    gt_joints, joints_conf = kd[:, :, :2], kd[:, :, 2].reshape(1, -1)
    joint_weights = torch.tensor(H.base_joint_weights(cfg, K), device=gpu).unsqueeze(0)
    mk = lambda t: prior.create_prior(prior_type=t, dtype=torch.float32)
    vals = []
    for model_vposer, closure_vposer in ((None, VPoser(R["w"])), (R["w"], None)):
        bm, camera = D._setup(synth_model, cfg, vposer=model_vposer)
        assert not hasattr(bm, "body_pose")
        with torch.no_grad():
            camera.translation[:] = torch.tensor([[0.0, 0.0, 20.0]], device=gpu)
            camera.center[:] = torch.tensor([400.0, 300.0], device=gpu)
        pose_embedding = torch.tensor(R["z"][:1], device=gpu, requires_grad=True)
        loss = fitting.create_loss(loss_type="smplify", joint_weights=joint_weights, rho=cfg["rho"], use_joints_conf=True,
                                   use_face=False, use_hands=False, body_pose_prior=mk("l2"), shape_prior=mk("l2"),
                                   angle_prior=mk("angle"), interpenetration=False, dtype=torch.float32).to(gpu)
        w = {"data_weight": 1000.0 / 600, "body_pose_weight": torch.tensor(cfg["body_pose_prior_weights"][0], device=gpu),
             "shape_weight": torch.tensor(cfg["shape_weights"][0], device=gpu)}
        w["bending_prior_weight"] = 3.17 * w["body_pose_weight"]
        loss.reset_loss_weights(w)
        with fitting.FittingMonitor(**cfg) as monitor:
            closure = monitor.create_fitting_closure(None, bm, camera=camera, gt_joints=gt_joints, joints_conf=joints_conf,
                                                     joint_weights=joint_weights, loss=loss, use_vposer=True, vposer=closure_vposer,
                                                     pose_embedding=pose_embedding, return_verts=False, return_full_pose=False)
            v = float(closure(stage=0))
            vals.append((v, pose_embedding.grad.detach().cpu().numpy().copy(), bm.global_orient.grad.detach().cpu().numpy().copy()))
            if closure._fb is not None:
                closure._fb.close()
        assert bm.device_model.vposer_latent == 32
    (va, ga, oa), (vb, gb, ob) = vals
    assert np.isfinite(va) and np.isfinite(ga).all() and np.abs(ga).max() > 0
    assert va == vb and np.array_equal(ga, gb) and np.array_equal(oa, ob)
