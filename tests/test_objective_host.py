"""CPU tests of the differentiable losses' surface (create_loss(differentiable=True), sfx_objective_eval / sfx_camera_init_eval):
what can be checked without a GPU -- the C ABI's declarations and bindings, the flag, and the loud refusal of CPU tensors.  The
arithmetic is tests/test_gpu_objective.py's."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sfx_objective_eval", "sfx_camera_init_eval")


def test_header_declares_and_capi_binds_the_two_entry_points():
    from smplifyx_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "sfx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _capi.SYMBOLS, name
    # each says which reference lines it replaces, as the other entry points do
    assert "fitting.py:375-461" in hdr and "fitting.py:499-520" in hdr
    # the structures the header declares and the bindings mirror: same fields, same order
    for struct, cls in (("sfx_objective_cfg", _capi.ObjectiveCfg), ("sfx_objective_in", _capi.ObjectiveIn),
                        ("sfx_objective_grads", _capi.ObjectiveGrads), ("sfx_camera_init_cfg", _capi.CameraInitCfg)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
        fields = re.findall(r"\b([A-Za-z_0-9]+)\s*(?:\[\d+\])?\s*[,;]", body)
        assert fields == [n for n, _ in cls._fields_], (struct, fields, [n for n, _ in cls._fields_])
    # the unit is built: named once in the list build.sh compiles and links from, with no flags of its own
    csrc = os.path.join(ROOT, "smplify-x-partial_amd", "csrc")
    assert open(os.path.join(csrc, "units.txt")).read().splitlines().count("objective_ext") == 1
    assert "units.txt" in open(os.path.join(csrc, "build.sh")).read()


def test_create_loss_stores_the_flag():
    from smplifyx_amd import fitting
    for kind, kw in (("smplify", {}), ("camera_init", dict(init_joints_idxs=[0, 1, 2]))):
        assert fitting.create_loss(kind, **kw).differentiable is False
        assert fitting.create_loss(kind, differentiable=True, **kw).differentiable is True


def test_cpu_tensors_are_refused_with_the_missing_fallback_named():
    from smplifyx_amd import fitting, prior, smplx
    from smplifyx_amd.camera import create_camera
    K = 5
    out = smplx.ModelOutput(joints=torch.zeros(1, K, 3, requires_grad=True), betas=torch.zeros(1, 10), body_pose=torch.zeros(1, 63),
                            full_pose=torch.zeros(1, 165))
    camera = create_camera(dtype=torch.float32)
    gt = torch.zeros(1, K, 2)
    mk = lambda t: prior.create_prior(prior_type=t)
    loss = fitting.create_loss("smplify", differentiable=True, use_hands=False, use_face=False, interpenetration=False,
                               body_pose_prior=mk("l2"), shape_prior=mk("l2"), angle_prior=mk("angle"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss(out, camera=camera, gt_joints=gt, joints_conf=torch.ones(1, K), joint_weights=torch.ones(1, K),
             pose_embedding=torch.zeros(1, 32), use_vposer=True)
    cam_loss = fitting.create_loss("camera_init", differentiable=True, init_joints_idxs=[0, 1, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cam_loss(out, camera=camera, gt_joints=gt)


def test_per_component_restatement_matches_the_references_golden():
    """The per-component oracle of tests/objective_common.py, the reference of the GPU parity test's 'gmm_unmerged' cases,
    against the REAL reference's module (tests/golden/gmm_unmerged.npz, fp64 run)."""
    import numpy as np
    from objective_common import GOLD, _PerComponentRef, _gmm
    mix, _ = _gmm()
    u = np.load(os.path.join(GOLD, "gmm_unmerged.npz"))
    pr = _PerComponentRef(mix["means"], mix["covars"], mix["weights"], torch.float64)
    x = torch.tensor(u["poses"], dtype=torch.float64, requires_grad=True)
    v = pr(x)
    v.sum().backward()
    assert np.allclose(v.detach().numpy(), u["val_f64"], rtol=1e-10, atol=0)
    assert np.linalg.norm(x.grad.numpy() - u["grad_f64"]) <= 1e-10 * np.linalg.norm(u["grad_f64"])


def test_weight_read_back_follows_every_reset():
    """fitting._loss_scalars caches the read-back of the weight buffers; reset_loss_weights replaces buffers, the old ones are
    freed and their addresses reused.  Random resets of subsets interleaved with read-backs: never a stale value."""
    import numpy as np
    from smplifyx_amd import fitting
    names = ["data_weight", "body_pose_weight", "shape_weight", "bending_prior_weight", "hand_prior_weight", "expr_prior_weight",
             "jaw_prior_weight", "coll_loss_weight"]
    rng = np.random.RandomState(0)
    for trial in range(20):
        loss = fitting.create_loss("smplify", differentiable=True, interpenetration=True)
        for step in range(200):
            sub = [n for n in names if n != "jaw_prior_weight" and rng.rand() < 0.4]
            loss.reset_loss_weights({n: float(rng.rand()) for n in sub})
            got = fitting._loss_scalars(loss, names)
            for n in names:
                want = getattr(loss, n).double().reshape(-1).tolist()
                assert got[n] == want, (trial, step, n, got[n], want)
    # a buffer changed IN PLACE is seen as well
    loss.data_weight.fill_(7.0)
    assert fitting._loss_scalars(loss, names)["data_weight"] == [7.0]
