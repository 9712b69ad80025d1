"""GPU tests of the differentiable SMPL-X forward (sfx_lbs_backward, DeviceModel.lbs_backward, smplx.SMPLX(differentiable=True)):
the gradient of sum(dvertices * vertices) + sum(djoints * joints) with respect to the nine inputs of the stand-alone LBS.

Parity (test 1).  Reference: fp64 autograd of the oracle (oracle/body_model.py: SMPLXRef through helpers.oracle_model).  Error
measure: ||g_dev - g64|| / ||g64|| per input block and for the concatenation of the nine.  Yardstick: the reference
precision's own rounding, i.e. the SAME oracle run with torch.float32 autograd at the same points against its fp64 run,
computed here.  Bound: 10 x that yardstick, per block and whole -- the factor is the margin tests/helpers.py states for its
own bounds (~10 x observed maxima); it is applied to the reference's error because the device's vertex arithmetic is fp32 with
other summation trees.  Every block's fp64 norm is >= 0.1 (asserted), so that no relative error is measured against noise --
with one exception that the inputs force: under the body-only joint map with a gradient on the joints alone, the 26 body
keypoints hardly depend on the jaw and the hands (fp64 norms 0.027 / 0.041 / 0.049 for jaw_pose / left_hand_pose /
right_hand_pose at these inputs).  Those three blocks are named below, and they are still held to the same relative bound,
which asks more of them than leaving them out would.

Observed on MI355X (the session summary prints every comparison next to its bound): the nine together <= 3.5e-7 (yardstick of
the same run 1.8e-7 .. 4.7e-7), per block <= 2.2e-6 (yardstick 1.5e-7 .. 4.5e-6), every block at 0.1 .. 1.4 x its own yardstick.
On helpers.dense_weights_model (the "dense-weights" case): the nine together <= 2.8e-7 (yardstick 2.5e-7 .. 5.9e-7), per block
<= 2.1e-6 (yardstick 1.9e-7 .. 3.1e-6), every block at 0.1 .. 2.1 x its own yardstick.
"""

import numpy as np
import pytest
import torch

import helpers as H
import test_gpu_parity as T

pytestmark = pytest.mark.gpu

NAMES = ("global_orient", "body_pose", "betas", "expression", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose",
         "right_hand_pose")
CASES = ("both", "vertices", "joints")
FACTOR = 10.0
MIN_NORM = 0.1
# the blocks below MIN_NORM (see the module docstring): body keypoints alone barely move with the jaw or the fingers
WEAK_BLOCKS = {("body", "joints", "jaw_pose"), ("body", "joints", "left_hand_pose"), ("body", "joints", "right_hand_pose")}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    return torch.device("cuda:0")


def _cfg(kind):
    """'full': fit_smplx_combined_halpe.yaml as shipped (hands + face + contour, K = 136: the big LDS variant of the sweep);
    'body': the same without hands and face (the small variant)."""
    if kind == "full":
        return H.load_cfg("fit_smplx_combined_halpe.yaml")
    return H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False)


def _inputs(B, seed, npca):
    rng = np.random.RandomState(seed)
    P = H.random_params(rng, B, scale=0.5, npca=npca)
    P["body_pose"] = P.pop("pose_embedding")
    return {k: P[k] for k in NAMES}, rng


def _oracle_grads(model, cfg, use_pca, P, dv, dj, dtype):
    """{case: [B x {name: grad}]} by autograd of the oracle in `dtype`: one forward per mesh, one backward per case."""
    bm = H.oracle_model(model, cfg, dtype)
    if not use_pca:         # the 45 axis-angle values themselves (SMPLXRef.use_pca=False; helpers.oracle_model does not pass it on)
        bm.use_pca = False
        bm.left_hand_pose = torch.nn.Parameter(torch.zeros([1, 45], dtype=dtype))
        bm.right_hand_pose = torch.nn.Parameter(torch.zeros([1, 45], dtype=dtype))
    B = dv.shape[0]
    out = {c: [] for c in CASES}
    ps = [getattr(bm, n) for n in NAMES]
    for i in range(B):
        bm.reset_params(**{k: v[i:i + 1] for k, v in P.items()})
        o = bm(return_verts=True)
        lv = (torch.as_tensor(dv[i:i + 1], dtype=dtype) * o.vertices).sum()
        lj = (torch.as_tensor(dj[i:i + 1], dtype=dtype) * o.joints).sum()
        for c, loss in (("both", lv + lj), ("vertices", lv), ("joints", lj)):
            g = torch.autograd.grad(loss, ps, retain_graph=True, allow_unused=True)
            out[c].append({n: (gi if gi is not None else torch.zeros_like(p)).double().numpy()[0] for n, gi, p in zip(NAMES, g, ps)})
    return {c: {n: np.stack([f[n] for f in out[c]]) for n in NAMES} for c in CASES}


def _rel(a, ref):
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / np.linalg.norm(ref))


def _cat(g):
    return np.concatenate([np.asarray(g[n], np.float64).reshape(-1) for n in NAMES])


_REF = {}


def reference(model, kind, use_pca, weights="base"):
    """Inputs, upstream gradients, fp64 reference gradients and the fp32 yardstick of one configuration (computed once).
    weights: "base", the model as given, or "dense", helpers.dense_weights_model of it."""
    key = (kind, use_pca, weights)
    if key not in _REF:
        if weights != "base":
            assert weights == "dense"
            model = H.dense_weights_model(model)
        cfg = _cfg(kind)
        npca = cfg["num_pca_comps"] if use_pca else 45
        P, rng = _inputs(3, 5, npca)
        V = np.asarray(model["v_template"]).shape[0]
        K = len(H.joint_map_for(cfg))
        dv = rng.normal(size=(3, V, 3)).astype(np.float32)
        dj = rng.normal(size=(3, K, 3)).astype(np.float32)
        g64 = _oracle_grads(model, cfg, use_pca, P, dv, dj, torch.float64)
        g32 = _oracle_grads(model, cfg, use_pca, P, dv, dj, torch.float32)
        yard = {}
        for c in CASES:
            y = {n: _rel(g32[c][n], g64[c][n]) for n in NAMES}
            y["whole"] = _rel(_cat(g32[c]), _cat(g64[c]))
            yard[c] = y
        _REF[key] = dict(cfg=cfg, P=P, dv=dv, dj=dj, g64=g64, yard=yard, K=K, V=V, model=model)
    return _REF[key]


def _dm(model, cfg, use_pca=True):
    return T._dm(model, cfg, use_pca=use_pca)


def _device_grads(dm, P, dv, dj, gpu):
    t = lambda a: torch.tensor(a, device=gpu) if a is not None else None
    g = dm.lbs_backward(*[t(P[n]) for n in NAMES], dvertices=t(dv), djoints=t(dj))
    assert tuple(g) == NAMES
    return g


# (the base model's cases keep the ids they had before the model became a parameter)
@pytest.mark.parametrize("kind,use_pca,weights", [
    pytest.param("full", True, "base", id="full-True"), pytest.param("body", True, "base", id="body-True"),
    pytest.param("full", False, "base", id="full-False"), pytest.param("full", True, "dense", id="full-True-dense-weights")])
def test_backward_matches_fp64_autograd_of_the_oracle(gpu, synth_model, kind, use_pca, weights):
    """weights = "dense": helpers.dense_weights_model -- 5 437 vertices with more than SFX_NW weights (k_adj_prep's full-row
    branch, wj[0] == -1), per-joint vertex lists of 2 433 .. 5 019 entries in k_adj_finish's d A (the base model's: 59 .. 3 443),
    keypoint vertices with 12."""
    R = reference(synth_model, kind, use_pca, weights)
    dm = _dm(R["model"], R["cfg"], use_pca)
    assert dm.K == R["K"] and dm.V == R["V"]
    label = "lbs-backward %s%s%s" % (kind, "" if use_pca else " no-pca", "" if weights == "base" else " dense-weights")
    for case in CASES:
        g = _device_grads(dm, R["P"], R["dv"] if case != "joints" else None, R["dj"] if case != "vertices" else None, gpu)
        g = {n: g[n].cpu().numpy() for n in NAMES}
        g64, yard = R["g64"][case], R["yard"][case]
        for n in NAMES:
            assert g[n].shape == g64[n].shape and np.isfinite(g[n]).all()
            nrm = float(np.linalg.norm(g64[n]))
            err = _rel(g[n], g64[n])
            print("%-28s %-9s %-16s |g64| %9.3e  device %.2e  yardstick %.2e  bound %.2e" % (label, case, n, nrm, err, yard[n], FACTOR * yard[n]))
            assert nrm >= MIN_NORM or (kind, case, n) in WEAK_BLOCKS, (label, case, n, nrm)
            H.check_bound(label, "%s d %s" % (case, n), err, FACTOR * yard[n])
        err = _rel(_cat(g), _cat(g64))
        print("%-28s %-9s %-16s device %.2e  yardstick %.2e  bound %.2e" % (label, case, "whole", err, yard["whole"], FACTOR * yard["whole"]))
        H.check_bound(label, "%s whole" % case, err, FACTOR * yard["whole"])
    dm.close()


def test_linearity_in_the_upstream(gpu, synth_model):
    """g(dv, dj) = g(dv, NULL) + g(NULL, dj) to fp32 rounding: the bound is test 1's (10 x the reference's own fp32 rounding of
    the combined gradient), the measure the same relative 2-norm, with the fp64 reference's norms as denominators."""
    R = reference(synth_model, "full", True)
    dm = _dm(synth_model, R["cfg"])
    both = _device_grads(dm, R["P"], R["dv"], R["dj"], gpu)
    gv = _device_grads(dm, R["P"], R["dv"], None, gpu)
    gj = _device_grads(dm, R["P"], None, R["dj"], gpu)
    yard, g64 = R["yard"]["both"], R["g64"]["both"]
    diff = {n: both[n].double().cpu().numpy() - (gv[n].double() + gj[n].double()).cpu().numpy() for n in NAMES}
    for n in NAMES:
        err = float(np.linalg.norm(diff[n]) / np.linalg.norm(g64[n]))
        print("linearity %-16s %.2e (bound %.2e)" % (n, err, FACTOR * yard[n]))
        H.check_bound("lbs-backward linearity", n, err, FACTOR * yard[n])
    err = float(np.linalg.norm(_cat(diff)) / np.linalg.norm(_cat(g64)))
    H.check_bound("lbs-backward linearity", "whole", err, FACTOR * yard["whole"])
    dm.close()


def test_a_frame_does_not_depend_on_its_batch_bitwise(gpu, synth_model):
    """70 frames: two 64-column tiles of the adjoint GEMM, the second partial; 130 frames: three tiles, hence the other launch
    shape (512 reduction indices per wavefront).  Frames at the tile edges give the same bits as the same frames alone."""
    cfg = _cfg("full")
    dm = _dm(synth_model, cfg)
    P, rng = _inputs(130, 7, cfg["num_pca_comps"])
    dv = rng.normal(size=(130, dm.V, 3)).astype(np.float32)
    dj = rng.normal(size=(130, dm.K, 3)).astype(np.float32)
    cut = lambda d, sl: {k: v[sl] for k, v in d.items()}
    g70 = _device_grads(dm, cut(P, slice(0, 70)), dv[:70], dj[:70], gpu)
    g130 = _device_grads(dm, P, dv, dj, gpu)
    for g, frames in ((g70, (0, 63, 64, 69)), (g130, (0, 64, 129))):
        for f in frames:
            g1 = _device_grads(dm, cut(P, slice(f, f + 1)), dv[f:f + 1], dj[f:f + 1], gpu)
            for n in NAMES:
                assert torch.isfinite(g1[n]).all() and g1[n].abs().max() > 0
                assert torch.equal(g[n][f], g1[n][0]), (n, f, float((g[n][f] - g1[n][0]).abs().max()))
    dm.close()


def _module(model, cfg, gpu, **kw):
    from smplifyx_amd import smplx, utils as U
    jm = U.JointMapper(H.joint_map_for(cfg))
    return smplx.create(model, joint_mapper=jm, num_betas=cfg["num_betas"], num_expression_coeffs=cfg["num_expression_coeffs"],
                        num_pca_comps=cfg["num_pca_comps"], use_face_contour=cfg["use_face_contour"], **kw).to(gpu)


def test_torch_surface(gpu, synth_model):
    cfg = _cfg("full")
    B = 2
    P, rng = _inputs(B, 9, cfg["num_pca_comps"])
    t = lambda a: torch.tensor(a, device=gpu)
    bm = _module(synth_model, cfg, gpu, batch_size=B, differentiable=True)
    bm.reset_params(**P)
    out = bm(return_verts=True)
    assert out.vertices.requires_grad and out.joints.requires_grad
    assert not out.betas.requires_grad and not out.body_pose.requires_grad and not out.left_hand_pose.requires_grad
    w = t(rng.normal(size=tuple(out.vertices.shape)).astype(np.float32))
    u = t(rng.normal(size=tuple(out.joints.shape)).astype(np.float32))
    # a second forward at other parameters between the forward and the backward of the first: the gradient is the first one's
    with torch.no_grad():
        other = bm(return_verts=True, body_pose=t(P["body_pose"]) + 0.3, betas=t(P["betas"]) - 1.0)
    assert not torch.equal(other.vertices, out.vertices)
    ((out.vertices * w).sum() + (out.joints * u).sum()).backward()
    ref = bm.device_model.lbs_backward(*[t(P[n]) for n in NAMES], dvertices=w, djoints=u)
    for n in NAMES:
        g = getattr(bm, n).grad
        assert g is not None and g.dtype == torch.float32 and torch.equal(g, ref[n].reshape(g.shape)), n
    # the caller's tensors take the gradient when they are passed in; joints only: the vertices' upstream stays None
    bp = t(P["body_pose"]).requires_grad_(True)
    be = t(P["betas"]).requires_grad_(True)
    for p in bm.parameters():
        p.grad = None
    out2 = bm(return_verts=True, body_pose=bp, betas=be)
    (out2.joints * u).sum().backward()
    ref2 = bm.device_model.lbs_backward(*[t(P[n]) for n in NAMES], djoints=u)
    assert torch.equal(bp.grad, ref2["body_pose"]) and torch.equal(be.grad, ref2["betas"])
    assert bm.body_pose.grad is None and bm.betas.grad is None
    assert torch.equal(bm.global_orient.grad, ref2["global_orient"])
    # float64 containers: cast in and out, float64 gradients of the same values
    bm64 = _module(synth_model, cfg, gpu, batch_size=B, differentiable=True, dtype=torch.float64)
    bm64.reset_params(**P)
    o64 = bm64(return_verts=True)
    assert o64.vertices.dtype == torch.float64 and o64.joints.dtype == torch.float64
    ((o64.vertices * w.double()).sum() + (o64.joints * u.double()).sum()).backward()
    for n in NAMES:
        g = getattr(bm64, n).grad
        assert g.dtype == torch.float64 and torch.equal(g, ref[n].reshape(g.shape).double()), n
    # the default constructor: no graph, and the forward's bits are those of the engine forward (as before)
    plain = _module(synth_model, cfg, gpu, batch_size=B)
    plain.reset_params(**P)
    op = plain(return_verts=True)
    assert not op.vertices.requires_grad and not op.joints.requires_grad
    v, j, _ = plain.device_model.lbs_forward(*[t(P[n]) for n in NAMES])
    assert torch.equal(op.vertices, v) and torch.equal(op.joints, j)
    assert torch.equal(out.vertices.detach(), v) and torch.equal(out.joints.detach(), j)


def test_memory_and_errors(gpu, synth_model):
    """The buffers of the backward are allocated by its first call, not at model creation or by the forward: free device memory
    (measured as test_a_refused_model_keeps_no_device_memory measures it) does not move across forward calls or a joints-only
    backward, and drops by the size of the adjoint's buffers at the first backward with a vertex gradient."""
    from smplifyx_amd import _capi
    import ctypes as C
    import gc
    gc.collect()
    cfg = _cfg("full")
    B = 32
    P, rng = _inputs(B, 11, cfg["num_pca_comps"])
    t = lambda a: torch.tensor(a, device=gpu)
    dm = _dm(synth_model, cfg)
    ins = [t(P[n]) for n in NAMES]
    dv = t(rng.normal(size=(B, dm.V, 3)).astype(np.float32))
    dj = t(rng.normal(size=(B, dm.K, 3)).astype(np.float32))
    free = lambda: (torch.cuda.synchronize(), torch.cuda.mem_get_info()[0])[1]
    v0, j0, _ = dm.lbs_forward(*ins)
    f_fwd = free()
    dm.lbs_forward(*ins)
    slack = 4 << 20         # torch's own small-block pool
    assert abs(f_fwd - free()) <= slack
    dm.lbs_backward(*ins, djoints=dj)
    f_j = free()
    assert f_fwd - f_j <= slack, "a joints-only backward allocates the parameter block's gradient only"
    dm.lbs_backward(*ins, dvertices=dv, djoints=dj)
    f_v = free()
    Vpad, Bpad = (dm.V + 15) // 16 * 16, (B + 127) // 128 * 128
    slices = 2 * ((3 * Vpad + 1023) // 1024)
    expect = 4 * (B * dm.V * 3 + Bpad * 3 * Vpad + slices * 512 * Bpad)      # v_posed, the GEMM operand, its partial sums
    print("free after forward / joints-only backward / full backward: %.1f / %.1f / %.1f MB; adjoint buffers %.1f MB" %
          (f_fwd / 2 ** 20, f_j / 2 ** 20, f_v / 2 ** 20, expect / 2 ** 20))
    assert expect > 8 * slack
    assert f_j - f_v >= expect - slack, "the adjoint's buffers were not there before the first backward that needs them"
    dm.lbs_backward(*ins, dvertices=dv, djoints=dj)
    assert abs(f_v - free()) <= slack
    # both upstream gradients missing: loud, at both layers; the model keeps working
    with pytest.raises(ValueError, match="upstream"):
        dm.lbs_backward(*ins)
    outs = [torch.empty_like(x) for x in ins]
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = dm._lib.sfx_lbs_backward(dm._h, B, *[p(x) for x in ins], None, None, *[p(x) for x in outs], None)
    assert rc == -1 and "both NULL" in dm._lib.sfx_last_error().decode()
    with pytest.raises(_capi.SfxError):
        _capi.check(rc)
    v1, j1, _ = dm.lbs_forward(*ins)
    assert torch.equal(v0, v1) and torch.equal(j0, j1)
    dm.close()


def test_forward_refuses_what_backward_refuses(gpu, synth_model):
    """lbs_forward hands the library nine pointers and B: a tensor of another width or batch is a ValueError naming it, as in
    lbs_backward (one code path), not a read past its end.  What it always took still passes, with the same bits: any dtype,
    body_pose as [B][21][3], inputs left out (None)."""
    cfg = _cfg("body")
    B = 2
    P, _ = _inputs(B, 5, cfg["num_pca_comps"])
    t = lambda a: torch.tensor(a, device=gpu)
    dm = _dm(synth_model, cfg)
    ins = [t(P[n]) for n in NAMES]
    dj = torch.ones(B, dm.K, 3, device=gpu)
    for i, name, bad in ((2, "betas", torch.zeros(B, dm.num_betas + 1, device=gpu)), (2, "betas", ins[2][:1]),
                         (8, "right_hand_pose", torch.zeros(B, dm.num_pca - 1, device=gpu)), (4, "jaw_pose", torch.zeros(B, 1, 3, device=gpu)),
                         (1, "body_pose", torch.zeros(B, 62, device=gpu))):
        wrong = ins[:i] + [bad] + ins[i + 1:]
        with pytest.raises(ValueError, match=name + ": shape"):
            dm.lbs_forward(*wrong)
        with pytest.raises(ValueError, match=name + ": shape"):
            dm.lbs_backward(*wrong, djoints=dj)
    with pytest.raises(ValueError, match="no CPU fallback"):
        dm.lbs_forward(*[x.cpu() for x in ins])
    v, j, fp = dm.lbs_forward(*ins)
    assert torch.isfinite(v).all() and v.abs().max() > 0
    v2, j2, fp2 = dm.lbs_forward(*[x.double() for x in ins[:1]], ins[1].reshape(B, 21, 3), *[x.double() for x in ins[2:]])
    assert torch.equal(v, v2) and torch.equal(j, j2) and torch.equal(fp, fp2)
    zeros = [torch.zeros_like(x) for x in ins]
    vz, jz, _ = dm.lbs_forward(*ins[:3], *zeros[3:])
    vn, jn, _ = dm.lbs_forward(*ins[:3], *[None] * 6)
    assert torch.equal(vz, vn) and torch.equal(jz, jn)
    dm.close()
