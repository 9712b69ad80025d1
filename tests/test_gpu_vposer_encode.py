"""GPU tests of the stand-alone VPoser encoder (sfx_vposer_encoder_*, engine.VPoserEncoder, smplifyx_amd.vposer.VPoser with
differentiable=True): the tile kernels k_vposer_encode16 / k_vposer_encode16_bwd of csrc/vposer_encode.hip.

Configurations (L, n_in, seed): (32, 63, 16), (32, 189, 24), (12, 189, 24) -- L = 12 shows a hard-coded 32, 189 exercises the
Rodrigues front end.  Weights synthetic.make_synthetic_vposer(0, latent=L, encoder_inputs=n_in).  Draws, in this order from
RandomState(seed), all float32: pose = 0.3 * normal(37, 63), dmean = normal(37, L), dsigma = normal(37, L).  B in {1, 16, 17, 37}
as leading rows: a tile with 15 empty rows, exactly one tile, a full tile plus a one-row tile, two full tiles plus five rows.

Reference and yardstick (the method of tests/test_gpu_vposer_batch.py).  Reference: oracle.vposer.VPoserEncoderRef in float64
with torch autograd of sum(dmean * mean) + sum(dsigma * sigma); for 189 inputs a plain torch Rodrigues written here goes in front
(the angles are far from zero).  Error measure: ||x - x64|| / ||x64||, per frame and over the batch.  Yardstick: the SAME oracle
in float32 against its float64 run at the same points, computed here; over the batch it is the float32 oracle's error over the
same B rows, per frame the float32 oracle's WORST single frame among the 37 draws.  Bound: 10 x the yardstick of the same
quantity (mean, sigma, dpose), the project's rule.

Conditions on the inputs, asserted on the float64 run, so that no kink decides a comparison: every hidden pre-activation of both
layers has |value| >= 1e-5, every joint angle lies in (0.01, 3) rad, every per-frame float64 norm is >= 0.1.  Other seeds fail
the first condition, which is why each configuration has its own seed.

The small-angle test replaces one frame's joints 0..4 by exact zeros and joints 5..9 by vectors of norm 5e-7 (the first-order
branch I + K(aa) of vposer._aa_to_matrot); its references are vposer.encode_stats (forward) and float64 autograd of a torch
restatement with the same branch (backward), its yardsticks that restatement in float32.
"""
import numpy as np
import pytest
import torch

import helpers as H
from smplifyx_amd import synthetic

pytestmark = pytest.mark.gpu

CONFIGS = ((32, 63, 16), (32, 189, 24), (12, 189, 24))
IDS = ["L%d-in%d" % (c[0], c[1]) for c in CONFIGS]
BATCHES = (1, 16, 17, 37)
N = 37
FACTOR = 10.0
MIN_NORM = 0.1
QUANTITIES = ("mean", "sigma", "dpose")


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


def _skew(a):
    z = torch.zeros_like(a[:, 0])
    return torch.stack([z, -a[:, 2], a[:, 1], a[:, 2], z, -a[:, 0], -a[:, 1], a[:, 0], z], -1).view(-1, 3, 3)


def _matrot_plain(pose):
    """[B, 63] axis-angle -> [B, 189] row-major rotation matrices: I + sin K + (1 - cos) K K, K of the unit axis."""
    a = pose.reshape(-1, 3)
    ang = a.norm(dim=1, keepdim=True)
    K = _skew(a / ang)
    s, c = torch.sin(ang)[:, :, None], torch.cos(ang)[:, :, None]
    R = torch.eye(3, dtype=pose.dtype)[None] + s * K + (1 - c) * (K @ K)
    return R.reshape(pose.shape[0], 189)


def _matrot_branch(pose):
    """The same with the first-order branch of vposer._aa_to_matrot: I + K(aa) where the angle is below 1e-6.  The plain form
    is evaluated at a stand-in for those rows, so that no 0 / 0 reaches autograd."""
    a = pose.reshape(-1, 3)
    small = (a.detach().norm(dim=1) < 1e-6)[:, None]
    safe = torch.where(small, torch.tensor([0.3, -0.2, 0.1], dtype=pose.dtype).expand_as(a), a)
    plain = _matrot_plain(safe.reshape(-1, 63)).reshape(-1, 3, 3)
    first = torch.eye(3, dtype=pose.dtype)[None] + _skew(a)
    return torch.where(small[:, :, None], first, plain).reshape(pose.shape[0], 189)


def _oracle(w, pose, dmean, dsigma, dtype, front=_matrot_plain):
    """(mean, sigma, dpose) of VPoserEncoderRef in `dtype`, as float64 arrays."""
    from oracle.vposer import VPoserEncoderRef
    enc = VPoserEncoderRef(w, dtype)
    p = torch.tensor(pose, dtype=dtype, requires_grad=True)
    q = enc.encode(front(p) if w["enc_fc1_w"].shape[1] == 189 else p)
    ((torch.tensor(dmean, dtype=dtype) * q.mean).sum() + (torch.tensor(dsigma, dtype=dtype) * q.stddev).sum()).backward()
    return dict(mean=q.mean.detach().double().numpy(), sigma=q.stddev.detach().double().numpy(), dpose=p.grad.double().numpy())


def _pre_activations(w, pose):
    """Hidden pre-activations of both layers in float64 (numpy, the unfolded network)."""
    from smplifyx_amd import vposer
    f = lambda k: np.asarray(w[k], np.float64)
    x = np.asarray(pose, np.float64)
    if w["enc_fc1_w"].shape[1] == 189:
        x = vposer._aa_to_matrot(x)
    bn = lambda x, n: (x - f(n + "_mean")) / np.sqrt(f(n + "_var") + vposer.BN_EPS) * f(n + "_w") + f(n + "_b")
    p1 = bn(x, "enc_bn1") @ f("enc_fc1_w").T + f("enc_fc1_b")
    p2 = bn(np.where(p1 > 0, p1, 0.2 * p1), "enc_bn2") @ f("enc_fc2_w").T + f("enc_fc2_b")
    return p1, p2


def _conditions(label, w, pose, r64):
    p1, p2 = _pre_activations(w, pose)
    min_pre = float(min(np.abs(p1).min(), np.abs(p2).min()))
    assert min_pre >= 1e-5, (label, min_pre)
    norms = {k: np.linalg.norm(r64[k], axis=1) for k in QUANTITIES}
    for k, v in norms.items():
        assert v.min() >= MIN_NORM, (label, k, float(v.min()))
    return min_pre, norms


_REF = {}


def reference(cfg):
    """Weights, draws, float64 reference, float32 yardsticks of one configuration (computed once, never modified)."""
    if cfg not in _REF:
        L, n_in, seed = cfg
        w = synthetic.make_synthetic_vposer(0, latent=L, encoder_inputs=n_in)
        rng = np.random.RandomState(seed)
        pose = (0.3 * rng.normal(size=(N, 63))).astype(np.float32)
        dmean = rng.normal(size=(N, L)).astype(np.float32)
        dsigma = rng.normal(size=(N, L)).astype(np.float32)
        r64 = _oracle(w, pose, dmean, dsigma, torch.float64)
        r32 = _oracle(w, pose, dmean, dsigma, torch.float32)
        # the conditions of the module docstring, on the float64 run
        min_pre, norms = _conditions(cfg, w, pose, r64)
        ang = np.linalg.norm(pose.astype(np.float64).reshape(N, 21, 3), axis=-1)
        print("L=%d n_in=%d: min |pre-activation| %.2e, joint angles %.3f .. %.3f rad, min fp64 norms mean %.2f sigma %.2f dpose %.2f"
              % (L, n_in, min_pre, ang.min(), ang.max(), norms["mean"].min(), norms["sigma"].min(), norms["dpose"].min()))
        assert 0.01 < ang.min() and ang.max() < 3.0, (cfg, float(ang.min()), float(ang.max()))
        yard = {}
        for k in QUANTITIES:
            yard[k, "frame"] = float(_rel_rows(r32[k], r64[k]).max())
            for B in BATCHES:
                yard[k, B] = _rel(r32[k][:B], r64[k][:B])
            print("L=%d n_in=%d: yardstick %-5s batch(37) %.2e worst frame %.2e" % (L, n_in, k, yard[k, N], yard[k, "frame"]))
        for a in (pose, dmean, dsigma) + tuple(r64.values()):
            a.setflags(write=False)
        _REF[cfg] = dict(w=w, pose=pose, dmean=dmean, dsigma=dsigma, r64=r64, yard=yard)
    return _REF[cfg]


_ENC = {}


def encoder(cfg, gpu):
    from smplifyx_amd import engine
    if cfg not in _ENC:
        _ENC[cfg] = engine.VPoserEncoder(reference(cfg)["w"])
    return _ENC[cfg]


def _check(label, what, got, ref, y_batch, y_frame):
    assert got.shape == ref.shape and np.isfinite(got).all()
    per = _rel_rows(got, ref)
    whole = _rel(got, ref)
    print("%-26s %-12s batch %.2e (yardstick %.2e, bound %.2e)  worst frame %.2e (yardstick %.2e, bound %.2e)"
          % (label, what, whole, y_batch, FACTOR * y_batch, per.max(), y_frame, FACTOR * y_frame))
    H.check_bound(label, what + " batch", whole, FACTOR * y_batch)
    H.check_bound(label, what + " worst frame", float(per.max()), FACTOR * y_frame)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("B", BATCHES)
def test_encode_matches_the_float64_oracle(gpu, cfg, B):
    R = reference(cfg)
    mean, sigma = encoder(cfg, gpu).encode(torch.tensor(R["pose"][:B], device=gpu))
    for k, t in (("mean", mean), ("sigma", sigma)):
        assert t.shape == (B, cfg[0]) and t.dtype == torch.float32
        _check("vposer-encode L=%d in=%d" % cfg[:2], "%s B=%d" % (k, B), t.cpu().numpy(), R["r64"][k][:B], R["yard"][k, B], R["yard"][k, "frame"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("B", BATCHES)
def test_encode_backward_matches_float64_autograd_of_the_oracle(gpu, cfg, B):
    R = reference(cfg)
    t = lambda a: torch.tensor(a[:B], device=gpu)
    dpose = encoder(cfg, gpu).encode_backward(t(R["pose"]), t(R["dmean"]), t(R["dsigma"]))
    assert dpose.shape == (B, 63) and dpose.dtype == torch.float32
    _check("vposer-encode-bwd L=%d in=%d" % cfg[:2], "dpose B=%d" % B, dpose.cpu().numpy(), R["r64"]["dpose"][:B],
           R["yard"]["dpose", B], R["yard"]["dpose", "frame"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_an_absent_gradient_is_an_explicit_zero_bitwise(gpu, cfg):
    R = reference(cfg)
    enc = encoder(cfg, gpu)
    pose, dm, ds = (torch.tensor(R[k], device=gpu) for k in ("pose", "dmean", "dsigma"))
    zero = torch.zeros_like(dm)
    only_mean, only_sigma = enc.encode_backward(pose, dm, None), enc.encode_backward(pose, None, ds)
    assert torch.isfinite(only_mean).all() and only_mean.abs().max() > 0 and only_sigma.abs().max() > 0
    assert torch.equal(only_mean, enc.encode_backward(pose, dm, zero))
    assert torch.equal(only_sigma, enc.encode_backward(pose, zero, ds))
    assert not torch.equal(only_mean, only_sigma)
    with pytest.raises(ValueError, match="at least one"):
        enc.encode_backward(pose, None, None)
    # sigma not wanted (sigma_dev = NULL): the mean alone is the same mean
    mean, none = enc.encode(pose, out_mean=torch.full([N, cfg[0]], -1.0, device=gpu), out_sigma=False)
    assert none is None and torch.equal(mean, enc.encode(pose)[0])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_a_frame_does_not_depend_on_its_batch_bitwise(gpu, cfg):
    """Frame i of the B = 37 call = the same pose encoded alone (row 0 of a one-row tile) = its value when the 37 rows are passed
    in reversed order (another tile and another row), for encode and encode_backward."""
    R = reference(cfg)
    enc = encoder(cfg, gpu)
    pose, dm, ds = (torch.tensor(R[k], device=gpu) for k in ("pose", "dmean", "dsigma"))
    (mean, sigma), dpose = enc.encode(pose), enc.encode_backward(pose, dm, ds)
    for t in (mean, sigma, dpose):
        assert torch.isfinite(t).all() and t.abs().max() > 0
    (mean_r, sigma_r), dpose_r = enc.encode(pose.flip(0)), enc.encode_backward(pose.flip(0), dm.flip(0), ds.flip(0))
    assert torch.equal(mean_r.flip(0), mean) and torch.equal(sigma_r.flip(0), sigma)
    assert torch.equal(dpose_r.flip(0), dpose), float((dpose_r.flip(0) - dpose).abs().max())
    for i in range(N):
        (m1, s1), g1 = enc.encode(pose[i:i + 1]), enc.encode_backward(pose[i:i + 1], dm[i:i + 1], ds[i:i + 1])
        assert torch.equal(m1[0], mean[i]) and torch.equal(s1[0], sigma[i]), i
        assert torch.equal(g1[0], dpose[i]), (i, float((g1[0] - dpose[i]).abs().max()))


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("B", (1, 17))
def test_nothing_is_stored_beyond_B(gpu, cfg, B):
    R = reference(cfg)
    L = cfg[0]
    enc = encoder(cfg, gpu)
    pose, dm, ds = (torch.tensor(R[k][:B], device=gpu) for k in ("pose", "dmean", "dsigma"))
    sentinel = -12345.5
    mean, sigma = torch.full([B + 1, L], sentinel, device=gpu), torch.full([B + 1, L], sentinel, device=gpu)
    dpose = torch.full([B + 1, 63], sentinel, device=gpu)
    enc.encode(pose, out_mean=mean[:B], out_sigma=sigma[:B])
    enc.encode_backward(pose, dm, ds, out=dpose[:B])
    assert (mean[B] == sentinel).all() and (sigma[B] == sentinel).all() and (dpose[B] == sentinel).all()
    m, s = enc.encode(pose)
    assert torch.equal(mean[:B], m) and torch.equal(sigma[:B], s) and torch.equal(dpose[:B], enc.encode_backward(pose, dm, ds))
    assert (mean[:B] != sentinel).all() and (sigma[:B] != sentinel).all() and (dpose[:B] != sentinel).all()
    # B = 0: no launch (a grid of zero workgroups would be a HIP error), nothing written, empty results
    mean.fill_(sentinel), sigma.fill_(sentinel), dpose.fill_(sentinel)
    m0, s0 = enc.encode(pose[:0], out_mean=mean[:0], out_sigma=sigma[:0])
    g0 = enc.encode_backward(pose[:0], dm[:0], ds[:0], out=dpose[:0])
    assert m0.shape == (0, L) and s0.shape == (0, L) and g0.shape == (0, 63)
    torch.cuda.synchronize()
    assert (mean == sentinel).all() and (sigma == sentinel).all() and (dpose == sentinel).all()
    # ... and the entry points return 0 for B = 0 before they look at any pointer
    import ctypes as C
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    assert enc._lib.sfx_vposer_encode(enc._h, 0, None, None, None, stream) == 0
    assert enc._lib.sfx_vposer_encode_backward(enc._h, 0, None, None, None, None, stream) == 0
    torch.cuda.synchronize()


def test_the_small_angle_branch(gpu):
    """Joints 0..4 of frame 1 exactly zero, joints 5..9 of norm 5e-7: the first-order branch, forward and backward."""
    from smplifyx_amd import vposer
    cfg = CONFIGS[1]
    R = reference(cfg)
    B = 3
    pose = R["pose"][:B].copy()
    dirs = np.random.RandomState(31).normal(size=(5, 3))
    pose[1, :15] = 0.0
    pose[1, 15:30] = (5e-7 * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32).reshape(-1)
    ang = np.linalg.norm(pose[1].astype(np.float64).reshape(21, 3), axis=1)
    assert (ang[:5] == 0).all() and (np.abs(ang[5:10] - 5e-7) < 1e-8).all() and (ang[10:] > 0.01).all()
    dm, ds = R["dmean"][:B], R["dsigma"][:B]
    r64 = _oracle(R["w"], pose, dm, ds, torch.float64, front=_matrot_branch)
    r32 = _oracle(R["w"], pose, dm, ds, torch.float32, front=_matrot_branch)
    mu, sg = vposer.encode_stats(R["w"], pose)
    assert _rel(r64["mean"], mu) < 1e-12 and _rel(r64["sigma"], sg) < 1e-12      # the restatement is the host encoder
    min_pre, norms = _conditions("small-angle", R["w"], pose, r64)
    print("small-angle: min |pre-activation| %.2e" % min_pre)
    enc = encoder(cfg, gpu)
    t = lambda a: torch.tensor(a, device=gpu)
    mean, sigma = enc.encode(t(pose))
    dpose = enc.encode_backward(t(pose), t(dm), t(ds))
    refs = dict(mean=mu, sigma=sg, dpose=r64["dpose"])
    for k, got in (("mean", mean), ("sigma", sigma), ("dpose", dpose)):
        _check("vposer-encode small angle", k, got.cpu().numpy(), refs[k], _rel(r32[k], r64[k]), float(_rel_rows(r32[k], r64[k]).max()))
    # the gradient of a small-angle joint is that of I + K(aa), not zero
    assert np.abs(dpose.cpu().numpy()[1, :30]).min() > 0


def test_torch_surface(gpu):
    from smplifyx_amd.vposer import VPoser
    cfg = CONFIGS[0]
    R = reference(cfg)
    B, L = 17, cfg[0]
    enc = encoder(cfg, gpu)
    vp = VPoser(R["w"], differentiable=True).to(gpu).eval()
    pose = torch.tensor(R["pose"][:B], device=gpu)
    mean, sigma = enc.encode(pose)
    Pin = pose.clone().requires_grad_(True)
    q = vp.encode(Pin)
    assert isinstance(q, torch.distributions.Normal)
    assert q.mean.shape == (B, L) and q.scale.shape == (B, L) and q.mean.requires_grad and q.scale.requires_grad
    assert q.mean.dtype == torch.float32 and torch.equal(q.mean.detach(), mean) and torch.equal(q.scale.detach(), sigma)
    (q.mean ** 2).sum().backward()
    assert Pin.grad is not None and Pin.grad.dtype == torch.float32
    assert torch.equal(Pin.grad, enc.encode_backward(pose, 2 * mean, None))
    # both outputs at once
    Pin2 = pose.clone().requires_grad_(True)
    q2 = vp.encode(Pin2)
    dm, ds = torch.tensor(R["dmean"][:B], device=gpu), torch.tensor(R["dsigma"][:B], device=gpu)
    ((q2.mean * dm).sum() + (q2.scale * ds).sum()).backward()
    assert torch.equal(Pin2.grad, enc.encode_backward(pose, dm, ds))
    # float64 in and out
    P64 = pose.double().requires_grad_(True)
    q64 = vp.encode(P64)
    assert q64.mean.dtype == torch.float64 and q64.scale.dtype == torch.float64 and torch.equal(q64.mean.detach(), mean.double())
    (q64.mean ** 2).sum().backward()
    assert P64.grad.dtype == torch.float64 and torch.equal(P64.grad, Pin.grad.double())
    with torch.no_grad():
        qn = vp.encode(Pin)
        assert not qn.mean.requires_grad and not qn.scale.requires_grad and torch.equal(qn.mean, mean)
    # the shapes the reference passes
    for shape in ((B, 1, 21, 3), (B, 21, 3)):
        qs = vp.encode(pose.view(*shape))
        assert qs.mean.shape == (B, L) and torch.equal(qs.mean, mean) and torch.equal(qs.scale, sigma)
    with pytest.raises(ValueError, match="63 values"):
        vp.encode(torch.zeros(B, 62, device=gpu))
    # a default object on the same CUDA input: the host numbers, without a graph
    from smplifyx_amd import vposer
    q0 = VPoser(R["w"]).to(gpu).eval().encode(Pin)
    mu, sg = vposer.encode_stats(R["w"], R["pose"][:B])
    assert not q0.mean.requires_grad and q0.mean.device.type == "cuda"
    assert np.array_equal(q0.mean.cpu().numpy(), mu.astype(np.float32)) and np.array_equal(q0.scale.cpu().numpy(), sg.astype(np.float32))
    # weights without an encoder: the host path's error
    with pytest.raises(ValueError, match="carry no encoder"):
        VPoser(synthetic.make_synthetic_vposer(0), differentiable=True).encode(pose)
    with pytest.raises(ValueError, match="pose"):
        enc.encode(torch.zeros(3, 62, device=gpu))
    with pytest.raises(ValueError, match="dmean"):
        enc.encode_backward(pose, dm[:B - 1], None)
    assert enc.device_index == gpu.index
    if torch.cuda.device_count() > 1:       # the handle lives on one device: a pose elsewhere is refused, not dereferenced
        with pytest.raises(ValueError, match="weights on cuda:0"):
            enc.encode(pose.to("cuda:1"))
    vp.close()
    assert vp._encoders == {}


def test_forward_is_encode_rsample_decode(gpu):
    from smplifyx_amd.vposer import VPoser
    cfg = CONFIGS[0]
    R = reference(cfg)
    B, L = 5, cfg[0]
    vp = VPoser(R["w"], differentiable=True).to(gpu).eval()
    Pin = torch.tensor(R["pose"][:B], device=gpu, requires_grad=True)
    torch.manual_seed(1234)
    out = vp(Pin.view(B, 1, 21, 3))
    assert sorted(out) == ["mean", "pose_aa", "std"]
    assert out["pose_aa"].shape == (B, 1, 21, 3) and out["mean"].shape == (B, L) and out["std"].shape == (B, L)
    torch.manual_seed(1234)
    with torch.no_grad():
        q = vp.encode(Pin)
        eps = torch.empty(q.mean.shape, dtype=q.mean.dtype, device=gpu).normal_()
        by_hand = vp.decode(q.mean + q.scale * eps)
    assert eps.abs().max() > 0
    assert torch.equal(out["mean"].detach(), q.mean) and torch.equal(out["std"].detach(), q.scale)
    assert torch.equal(out["pose_aa"].detach(), by_hand), float((out["pose_aa"].detach() - by_hand).abs().max())
    out["pose_aa"].sum().backward()
    assert Pin.grad is not None and torch.isfinite(Pin.grad).all() and (Pin.grad != 0).all()
    with pytest.raises(ValueError, match="matrot"):
        vp(Pin, output_type="matrot")
    with pytest.raises(NotImplementedError):
        VPoser(R["w"])(Pin)
    vp.close()


def _body_cfg():
    return H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False)


def _module(model, cfg, gpu, **kw):
    from smplifyx_amd import smplx, utils as U
    jm = U.JointMapper(H.joint_map_for(cfg))
    return smplx.create(model, joint_mapper=jm, num_betas=cfg["num_betas"], num_expression_coeffs=cfg["num_expression_coeffs"],
                        num_pca_comps=cfg["num_pca_comps"], use_face_contour=cfg["use_face_contour"], **kw).to(gpu)


def test_pose_prior_gradient_through_encode_and_the_differentiable_model(gpu, synth_model):
    """body_pose (a leaf) -> sum(dj * joints) of SMPLX(differentiable=True) + sum(encode(body_pose).mean ** 2): body_pose.grad
    against float64 autograd of the oracle body model + VPoserEncoderRef; bound 10 x the float32 oracles' own error of the same
    sum (computed here), relative 2-norm over the whole gradient."""
    from oracle.vposer import VPoserEncoderRef
    from smplifyx_amd.vposer import VPoser
    R = reference(CONFIGS[0])
    B = 2
    cfg = _body_cfg()
    rng = np.random.RandomState(17)
    P = H.random_params(rng, B, scale=0.5, npca=cfg["num_pca_comps"])
    P.pop("pose_embedding")
    K = len(H.joint_map_for(cfg))
    dj = rng.normal(size=(B, K, 3)).astype(np.float32)
    pose = R["pose"][:B]

    def oracle(dtype):
        enc, bm = VPoserEncoderRef(R["w"], dtype), H.oracle_model(synth_model, cfg, dtype)
        bp = torch.tensor(pose, dtype=dtype, requires_grad=True)
        loss = (enc.encode(bp).mean ** 2).sum()
        for i in range(B):
            bm.reset_params(**{k: v[i:i + 1] for k, v in P.items()})
            o = bm(return_verts=True, body_pose=bp[i:i + 1])
            loss = loss + (torch.as_tensor(dj[i:i + 1], dtype=dtype) * o.joints).sum()
        loss.backward()
        return bp.grad.double().numpy()

    g64, g32 = oracle(torch.float64), oracle(torch.float32)
    yard = _rel(g32, g64)
    assert np.linalg.norm(g64, axis=1).min() >= MIN_NORM
    vp = VPoser(R["w"], differentiable=True).to(gpu).eval()
    bm = _module(synth_model, cfg, gpu, batch_size=B, differentiable=True)
    bm.reset_params(**P)
    bp = torch.tensor(pose, device=gpu, requires_grad=True)
    out = bm(return_verts=True, body_pose=bp)
    prior = (vp.encode(bp).mean ** 2).sum()
    ((out.joints * torch.tensor(dj, device=gpu)).sum() + prior).backward()
    assert bp.grad is not None and bp.grad.shape == (B, 63) and torch.isfinite(bp.grad).all()
    # both terms reach the leaf
    g_prior = encoder(CONFIGS[0], gpu).encode_backward(bp.detach(), 2 * vp.encode(bp.detach()).mean, None)
    assert g_prior.abs().max() > 0 and (bp.grad - g_prior).abs().max() > 0
    err = _rel(bp.grad.cpu().numpy(), g64)
    print("pose-prior chain: |g64| %.3e  device %.2e  yardstick %.2e  bound %.2e" % (np.linalg.norm(g64), err, yard, FACTOR * yard))
    H.check_bound("vposer pose-prior chain", "d body_pose", err, FACTOR * yard)
    vp.close()
