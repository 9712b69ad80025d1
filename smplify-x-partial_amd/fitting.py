"""Drop-in for smplifyx/fitting.py: guess_init (:36-110), FittingMonitor (:113-275),
create_loss / SMPLifyLoss / SMPLifyCameraInitLoss (:278-520).

The objects keep the reference's constructor kwargs, attributes and call conventions, but the
arithmetic of the closure (LBS, projection, losses, adjoint) and of the optimiser runs in
libsfx.so (the loss modules' stand-alone forward evaluates the same device objective without backward): `create_fitting_closure` binds a one-frame `engine.FrameBatch` to the caller's
tensors; the closure it returns evaluates loss + gradients on the GPU and stores them in the
parameters' `.grad`; `run_fitting` executes the whole step loop on device.  By default there is no
autograd graph; `create_loss(..., differentiable=True)` makes the two losses functions of TENSORS with a graph (one fused
device kernel for value and gradient: csrc/objective_ext.hip), so that the reference's closure body -- body_model(...), loss(...),
total_loss.backward() -- runs as written over differentiable=True objects.  There is no CPU fallback.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _capi as capi
from . import engine
from . import utils


@torch.no_grad()
def guess_init(model, joints_2d, edge_idxs, focal_length=5000, pose_embedding=None, vposer=None,
               use_vposer=True, dtype=torch.float32, model_type="smpl", **kwargs):
    """Initial camera translation (0, 0, f * mean|d3D| / mean|d2D|) over limb pairs."""
    if use_vposer:
        body_pose = vposer.decode(pose_embedding, output_type="aa").view(1, -1)
    else:
        body_pose = pose_embedding
    output = model(body_pose=body_pose, return_verts=False, return_full_pose=False)
    j3 = output.joints
    j2 = joints_2d.to(device=j3.device)
    d3 = torch.stack([j3[:, e[0]] - j3[:, e[1]] for e in edge_idxs], dim=1)
    d2 = torch.stack([j2[:, e[0]] - j2[:, e[1]] for e in edge_idxs], dim=1)
    h2 = d2.pow(2).sum(dim=-1).sqrt().mean(dim=1)
    h3 = d3.pow(2).sum(dim=-1).sqrt().mean(dim=1)
    est_d = focal_length * (h3 / h2)
    z = torch.zeros([j3.shape[0]], device=j3.device, dtype=dtype)
    return torch.stack([z, z.clone(), est_d], dim=1)


def create_loss(loss_type="smplify", **kwargs):
    if loss_type == "smplify":
        return SMPLifyLoss(**kwargs)
    elif loss_type == "camera_init":
        return SMPLifyCameraInitLoss(**kwargs)
    raise ValueError("Unknown loss type: {}".format(loss_type))


class SMPLifyLoss(nn.Module):
    """Weights / flags of the body objective (fitting.py:287-373).  Evaluated by the engine."""

    def __init__(self, search_tree=None, pen_distance=None, tri_filtering_module=None, rho=100,
                 body_pose_prior=None, shape_prior=None, expr_prior=None, angle_prior=None, jaw_prior=None,
                 use_joints_conf=True, use_face=True, use_hands=True, left_hand_prior=None, right_hand_prior=None,
                 interpenetration=True, dtype=torch.float32, data_weight=1.0, body_pose_weight=0.0,
                 shape_weight=0.0, bending_prior_weight=0.0, hand_prior_weight=0.0, expr_prior_weight=0.0,
                 jaw_prior_weight=0.0, coll_loss_weight=0.0, reduction="sum", regression_pose=None, num_stages=3,
                 differentiable=False, **kwargs):
        super().__init__()
        # differentiable=False (default): forward evaluates the device objective at the parameters a ModelOutput remembers and
        # returns a tensor without a graph.  True: forward is a function of the tensors it is given (joints, camera, prior
        # operands) with an autograd graph -- see _differentiable_smplify.
        self.differentiable = bool(differentiable)
        self.use_joints_conf, self.rho = use_joints_conf, rho
        self.angle_prior, self.body_pose_prior, self.shape_prior = angle_prior, body_pose_prior, shape_prior
        self.interpenetration = interpenetration
        # fit_single_frame.py:300-328: BVH / DistanceFieldPenetrationLoss / FilterFaces (smplifyx_amd.mesh_intersection holders)
        self.search_tree, self.pen_distance, self.tri_filtering_module = search_tree, pen_distance, tri_filtering_module
        self.use_hands = use_hands
        if use_hands:
            self.left_hand_prior, self.right_hand_prior = left_hand_prior, right_hand_prior
        self.use_face = use_face
        if use_face:
            self.expr_prior, self.jaw_prior = expr_prior, jaw_prior
        reg = lambda n, v: self.register_buffer(n, torch.tensor(v, dtype=dtype))
        reg("data_weight", data_weight); reg("body_pose_weight", body_pose_weight); reg("shape_weight", shape_weight)
        reg("bending_prior_weight", bending_prior_weight)
        if use_hands:
            reg("hand_prior_weight", hand_prior_weight)
        if use_face:
            reg("expr_prior_weight", expr_prior_weight); reg("jaw_prior_weight", jaw_prior_weight)
        if interpenetration:
            reg("coll_loss_weight", coll_loss_weight)
        self.regression_pose = regression_pose
        self.num_stages = num_stages

    def reset_loss_weights(self, loss_weight_dict):
        for key in loss_weight_dict:
            if hasattr(self, key):
                cur = getattr(self, key)
                v = loss_weight_dict[key]
                if torch.is_tensor(v):
                    new = v.clone().detach()
                else:
                    new = torch.tensor(v, dtype=cur.dtype, device=cur.device)
                setattr(self, key, new)

    def forward(self, body_model_output, camera, gt_joints, joints_conf, body_model_faces=None, joint_weights=None,
                use_vposer=False, pose_embedding=None, stage=0, per_frame=False, **kwargs):
        """differentiable=True: the loss as a function of the given tensors, with a graph (_differentiable_smplify); a 0-d sum
        over the batch like the reference, or with per_frame=True the [B] losses of the frames.  Otherwise:
        Stand-alone evaluation (fitting.py:375-461; keyword set of :251-259): the total loss of the DEVICE objective
        (csrc/closure_body.h, no backward) at the parameters `body_model_output` was made from -- a ModelOutput of this
        package's SMPLX.forward, which remembers them.  `stage` matters only for the latent regression prior
        (fitting.py:391-395: last stage).  Returns a 0-d tensor like the reference; it carries no autograd graph."""
        if self.differentiable:
            return _differentiable_smplify(self, body_model_output, camera, gt_joints, joints_conf, body_model_faces, joint_weights,
                                           use_vposer, pose_embedding, stage, per_frame)
        return _standalone_loss(self, body_model_output, camera, gt_joints, joints_conf, joint_weights, use_vposer,
                                pose_embedding, stage)


class SMPLifyCameraInitLoss(nn.Module):
    def __init__(self, init_joints_idxs, trans_estimation=None, reduction="sum", data_weight=1.0,
                 depth_loss_weight=1e2, dtype=torch.float32, joints_conf=None, use_conf=False, differentiable=False, **kwargs):
        super().__init__()
        self.dtype = dtype
        self.differentiable = bool(differentiable)      # as SMPLifyLoss
        if trans_estimation is not None:
            te = trans_estimation.clone().detach() if torch.is_tensor(trans_estimation) else torch.tensor(trans_estimation, dtype=dtype)
            self.register_buffer("trans_estimation", te.to(dtype))
        else:
            self.trans_estimation = trans_estimation
        self.register_buffer("data_weight", torch.tensor(data_weight, dtype=dtype))
        idx = init_joints_idxs.clone().detach().long() if torch.is_tensor(init_joints_idxs) else torch.tensor(init_joints_idxs, dtype=torch.long)
        self.register_buffer("init_joints_idxs", idx)
        self.register_buffer("depth_loss_weight", torch.tensor(depth_loss_weight, dtype=dtype))
        self.joints_conf = joints_conf
        self.use_conf = use_conf

    def reset_loss_weights(self, loss_weight_dict):
        for key in loss_weight_dict:
            if hasattr(self, key):
                cur = getattr(self, key)
                setattr(self, key, torch.tensor(loss_weight_dict[key], dtype=cur.dtype, device=cur.device))

    def forward(self, body_model_output, camera, gt_joints, body_model=None, per_frame=False, **kwargs):
        """Stand-alone evaluation (fitting.py:499-520) of the device camera-initialisation loss at the parameters
        `body_model_output` was made from (see SMPLifyLoss.forward); differentiable=True: a function of the joints and the
        camera's rotation and translation, with a graph (_differentiable_camera_init)."""
        if self.differentiable:
            return _differentiable_camera_init(self, body_model_output, camera, gt_joints, per_frame)
        return _standalone_loss(self, body_model_output, camera, gt_joints, None, None, False,
                                kwargs.get("pose_embedding"), 0)


def _np(t):
    return t.detach().to("cpu", torch.float32).numpy()


# ---- create_loss(..., differentiable=True): the losses as functions of tensors, fused on the device -------------------------
class _FusedLoss(torch.autograd.Function):
    """loss [B] of a device objective (engine.objective_eval / camera_init_eval) of the given tensors.  The gradients come from
    the SAME launch as the loss and are saved, as mesh_intersection.loss._ConeFieldLoss does; backward only scales each frame's
    rows by that frame's upstream.  First derivatives only: backward(create_graph=True) is refused."""

    @staticmethod
    def forward(ctx, call, *tensors):
        loss, grads = call(*[t.detach() for t in tensors])
        ctx.save_for_backward(*grads)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        if torch.is_grad_enabled():       # autograd records the backward pass only under create_graph=True
            raise RuntimeError("backward(create_graph=True): the differentiable loss has first derivatives only -- its gradient "
                               "is computed by the device kernel together with the value, there is no graph of it to differentiate")
        out = [None]
        for g, need in zip(ctx.saved_tensors, ctx.needs_input_grad[1:]):
            out.append(g * dloss.reshape([-1] + [1] * (g.dim() - 1)) if need else None)
        return tuple(out)


def _need_cuda(t, what):
    if not torch.is_tensor(t):
        raise TypeError("%s: a torch tensor is needed, got %s" % (what, type(t).__name__))
    if t.device.type != "cuda":
        raise RuntimeError("%s is on %s: the differentiable loss is one fused device kernel (csrc/objective_ext.hip) and has "
                           "no CPU fallback -- move the model, the camera and the data to the GPU" % (what, t.device))


def _rows(name, t, shape, dev, one_serves_all=False):
    """`t` as a float32 contiguous tensor of `shape` on `dev`, graph kept (cast, made contiguous).  Every tensor must be on the
    device already (RuntimeError: nothing is copied from the host behind the caller's back, evaluation after evaluation).  The
    shape must be `shape` itself; one_serves_all: a tensor made for ONE frame (a camera, a row of joint weights, a regression
    target) is broadcast over the batch.  A shape that does not fit is the caller's mistake: ValueError."""
    if t is None:
        return None
    _need_cuda(t, name)
    if t.device != dev:
        raise ValueError("%s: on %s, body_model_output.joints on %s" % (name, t.device, dev))
    fits = tuple(t.shape) == tuple(shape)
    if not fits and one_serves_all:
        lead = t.dim() - len(shape) + 1           # a missing or a 1-long batch dimension, the rest as asked
        fits = lead in (0, 1) and tuple(t.shape[lead:]) == tuple(shape[1:]) and (lead == 0 or t.shape[0] == 1)
    if not fits:
        raise ValueError("%s: shape %s, expected %s%s (B and K are those of body_model_output.joints)"
                         % (name, tuple(t.shape), tuple(shape), " or one frame's" if one_serves_all else ""))
    return t.to(torch.float32).expand(shape).contiguous()


def _loss_scalars(loss, names):
    """{name: [floats]} of the loss's weight buffers, read back once per set of tensors (reset_loss_weights replaces them):
    a fused evaluation must not pay one device synchronisation per weight.  The cache HOLDS the tensors it was read from and
    compares identity and version counter: an address reused by a later tensor cannot be mistaken for them."""
    ts = [getattr(loss, n, None) for n in names]
    cached = loss.__dict__.get("_scalars")
    same = cached is not None and len(cached[0]) == len(ts) and all(
        a is t and v == getattr(t, "_version", 0) for (a, v), t in zip(cached[0], ts))
    if not same:
        vals = {n: (torch.as_tensor(t).detach().cpu().double().reshape(-1).tolist() if t is not None else [0.0]) for n, t in zip(names, ts)}
        cached = ([(t, getattr(t, "_version", 0)) for t in ts], vals)
        loss.__dict__["_scalars"] = cached
    return cached[1]


def _mixture_tables(loss, gmm, dev):
    """The mixture's tables on the device, as sfx_objective_cfg takes them (engine.FrameBatch.set_gmm's, kept as tensors)."""
    cached = loss.__dict__.get("_mixture")
    if cached is None or cached[0] is not gmm or cached[1] != dev:
        t = lambda x: x.detach().to(dev, torch.float32).contiguous()
        cc = gmm.component_constants()         # None: the merged form (the table FrameBatch.set_gmm sends as well)
        tables = dict(means=t(gmm.means), precisions=t(gmm.precisions), nll_weights=t(gmm.nll_weights.reshape(-1)),
                      comp_const=t(cc) if cc is not None else None)
        cached = (gmm, dev, tables)
        loss.__dict__["_mixture"] = cached
    return cached[2]


def _per_frame_term(v, B, dev):
    """A prior module's result as [B] when it holds one row per frame, else its 0-d sum (L2Prior-like modules return a scalar)."""
    v = torch.as_tensor(v, device=dev)
    if v.dim() >= 1 and v.shape[0] == B:
        return v.reshape(B, -1).sum(1)
    return v.sum().reshape(1) if B == 1 else v.sum()


def _finish(fused, extras, per_frame, dtype):
    """fused [B] + the terms evaluated in torch -> the [B] losses (per_frame) or their 0-d sum like the reference, in the
    containers' dtype (float64 containers: the fp32 device values are added up in double)."""
    per = fused.to(dtype)
    scalars = []
    for e in extras:
        if e.dim() == 1:
            per = per + e.to(per.dtype)
        else:
            scalars.append(e)
    if per_frame:
        if scalars:
            raise ValueError("per_frame=True: a prior module of the caller's returned one number for the whole batch; return one "
                             "value per frame ([B, ...]) so that the loss can be split")
        return per.to(dtype)
    total = per.sum()
    for e in scalars:
        total = total + e.to(total.dtype)
    return total.to(dtype)


def _differentiable_smplify(loss, out, camera, gt_joints, joints_conf, body_model_faces, joint_weights, use_vposer,
                            pose_embedding, stage, per_frame):
    """SMPLifyLoss.forward of differentiable=True (fitting.py:375-461) as a function of TENSORS: body_model_output.joints, the
    camera's rotation / translation (parameters) and focal lengths / center (buffers), and the prior operands -- from
    `body_model_output._graph` when this package's differentiable SMPLX made it (its echoed fields are detached), else from the
    output's own fields (a hand-built ModelOutput whose fields carry graphs).  Data term, L2Prior / SMPLifyAnglePrior /
    MaxMixturePrior terms and the gradient of their sum come from ONE launch (engine.objective_eval); any other prior module is
    called in torch on the same tensors and added with its weight; the interpenetration term is composed from the stand-alone
    search_tree / tri_filtering_module / pen_distance modules (:437-455)."""
    from . import prior as P
    joints = out.joints
    _need_cuda(joints, "body_model_output.joints")
    if joints.dim() != 3 or joints.shape[2] != 3:
        raise ValueError("body_model_output.joints: shape %s, expected (B, K, 3)" % (tuple(joints.shape),))
    B, K = int(joints.shape[0]), int(joints.shape[1])
    if K < 1 or K > engine.OBJECTIVE_MAX_K:
        raise ValueError("body_model_output.joints: K = %d keypoints, supported 1..%d" % (K, engine.OBJECTIVE_MAX_K))
    dev, dtype = joints.device, joints.dtype
    for name, t in (("camera.translation", camera.translation), ("gt_joints", gt_joints)):
        _need_cuda(t, name)
    graph = getattr(out, "_graph", None) or {}
    model = getattr(out, "_model", None)

    def field(name):
        t = graph.get(name)
        t = t if t is not None else getattr(out, name, None)
        if t is None:
            raise ValueError("body_model_output.%s is None: the loss reads it (fitting.py:399-435)" % name)
        return t

    names = ["data_weight", "body_pose_weight", "shape_weight", "bending_prior_weight", "hand_prior_weight", "expr_prior_weight",
             "jaw_prior_weight", "coll_loss_weight"]
    w = _loss_scalars(loss, names)
    s = lambda n: w[n][0]
    weights = dict(data_weight=s("data_weight"), body_pose_weight=s("body_pose_weight"))
    extras = []
    is_l2 = lambda m: type(m) is P.L2Prior

    # pose prior (fitting.py:390-401)
    reg, mixture, target = loss.regression_pose, None, None
    if use_vposer or reg is not None:
        if pose_embedding is None:
            raise ValueError("pose_embedding is needed (use_vposer, or a regression prior: fitting.py:390-397)")
        operand = pose_embedding
        form = "target" if reg is not None and (not use_vposer or stage + 1 == loss.num_stages) else "embedding"
        if form == "target":
            target = reg.detach().reshape(reg.shape[0], -1)
    else:
        operand, bpp = field("body_pose"), loss.body_pose_prior
        form = "body_pose"
        if type(bpp) is P.MaxMixturePrior:
            form, mixture = "mixture", _mixture_tables(loss, bpp, dev)
        elif not is_l2(bpp):
            weights["body_pose_weight"] = 0.0
            if bpp is not None:
                extras.append(_per_frame_term(bpp(operand, field("betas")), B, dev) * s("body_pose_weight") ** 2)
    operand = operand.reshape(operand.shape[0], -1)
    n = int(operand.shape[1])

    betas = field("betas")
    if is_l2(loss.shape_prior):
        weights["shape_weight"] = s("shape_weight")
    elif loss.shape_prior is not None:
        extras.append(_per_frame_term(loss.shape_prior(betas), B, dev) * s("shape_weight") ** 2)
    # the angle prior's operand (:407): full_pose[:, 3:66] is the body_pose input of the model
    if graph.get("body_pose") is not None:
        body_pose = graph["body_pose"]
    elif getattr(out, "full_pose", None) is not None:
        body_pose = out.full_pose[:, 3:66]
    else:
        body_pose = field("body_pose")
    if type(loss.angle_prior) is P.SMPLifyAnglePrior:
        weights["bending_prior_weight"] = s("bending_prior_weight")
    elif loss.angle_prior is not None:
        extras.append(_per_frame_term(loss.angle_prior(body_pose), B, dev) * s("bending_prior_weight"))

    lh = rh = expr = jaw = None
    use_hands = use_face = False
    jaw_w = (0.0, 0.0, 0.0)
    if loss.use_hands and (loss.left_hand_prior is not None or loss.right_hand_prior is not None):
        if graph.get("left_hand_pose") is not None and model is not None:     # PCA coefficients -> the 45 values, in torch
            lh45, rh45 = model.hand_pose_45(graph["left_hand_pose"], "left"), model.hand_pose_45(graph["right_hand_pose"], "right")
        else:
            lh45, rh45 = field("left_hand_pose"), field("right_hand_pose")
        if is_l2(loss.left_hand_prior) and is_l2(loss.right_hand_prior):
            use_hands, lh, rh = True, lh45, rh45
            weights["hand_prior_weight"] = s("hand_prior_weight")
        else:
            for m, h in ((loss.left_hand_prior, lh45), (loss.right_hand_prior, rh45)):
                if m is not None:
                    extras.append(_per_frame_term(m(h), B, dev) * s("hand_prior_weight") ** 2)
    if loss.use_face:
        if is_l2(loss.expr_prior) or is_l2(loss.jaw_prior):
            use_face, expr, jaw = True, field("expression"), field("jaw_pose")
        if is_l2(loss.expr_prior):
            weights["expr_prior_weight"] = s("expr_prior_weight")
        elif loss.expr_prior is not None:
            extras.append(_per_frame_term(loss.expr_prior(field("expression")), B, dev) * s("expr_prior_weight") ** 2)
        jw3 = w["jaw_prior_weight"] * 3 if len(w["jaw_prior_weight"]) == 1 else w["jaw_prior_weight"]
        if is_l2(loss.jaw_prior):
            jaw_w = tuple(jw3[:3])
        elif getattr(loss, "jaw_prior", None) is not None:
            jp = field("jaw_pose")
            extras.append(_per_frame_term(loss.jaw_prior(jp.mul(torch.tensor(jw3[:3], dtype=jp.dtype, device=dev))), B, dev))

    if loss.use_joints_conf and joints_conf is None:
        raise ValueError("use_joints_conf=True needs joints_conf (fitting.py:380)")
    if joint_weights is None:
        joint_weights = torch.ones([1, K], dtype=torch.float32, device=dev)
    fixed = dict(focal_x=_rows("camera.focal_length_x", camera.focal_length_x.detach(), (B,), dev, True),
                 focal_y=_rows("camera.focal_length_y", camera.focal_length_y.detach(), (B,), dev, True),
                 center=_rows("camera.center", camera.center.detach(), (B, 2), dev, True),
                 gt_joints=_rows("gt_joints", gt_joints.detach(), (B, K, 2), dev),
                 joint_weights=_rows("joint_weights", joint_weights.detach(), (B, K), dev, True),
                 joints_conf=_rows("joints_conf", joints_conf.detach(), (B, K), dev) if loss.use_joints_conf else None,
                 prior_target=_rows("regression_pose", target, (B, n), dev, True))
    diff = dict(joints=_rows("body_model_output.joints", joints, (B, K, 3), dev),
                rotation=_rows("camera.rotation", camera.rotation, (B, 3, 3), dev, True),
                translation=_rows("camera.translation", camera.translation, (B, 3), dev, True),
                body_pose=_rows("body_pose", body_pose.reshape(body_pose.shape[0], -1), (B, 63), dev),
                prior=_rows("the pose prior's operand", operand, (B, n), dev),
                betas=_rows("betas", betas, (B, betas.shape[-1]), dev),
                expression=_rows("expression", expr, (B, expr.shape[-1]), dev) if expr is not None else None,
                jaw_pose=_rows("jaw_pose", jaw, (B, 3), dev), left_hand_pose=_rows("left_hand_pose", lh, (B, 45), dev),
                right_hand_pose=_rows("right_hand_pose", rh, (B, 45), dev))
    order = [k for k in engine.OBJECTIVE_GRADS if diff[k] is not None]

    def call(*tensors):
        kw = dict(zip(order, tensors))
        value, grads = engine.objective_eval(kw["joints"], kw["rotation"], kw["translation"], fixed["focal_x"], fixed["focal_y"],
                                             fixed["center"], fixed["gt_joints"], fixed["joint_weights"], kw["body_pose"],
                                             kw["prior"], kw["betas"], joints_conf=fixed["joints_conf"],
                                             prior_target=fixed["prior_target"], expression=kw.get("expression"),
                                             jaw_pose=kw.get("jaw_pose"), left_hand_pose=kw.get("left_hand_pose"),
                                             right_hand_pose=kw.get("right_hand_pose"), weights=weights, jaw_prior_weight=jaw_w,
                                             rho=float(loss.rho), use_joints_conf=bool(loss.use_joints_conf), use_hands=use_hands,
                                             use_face=use_face, prior_form=form, mixture=mixture)
        return value, tuple(grads[k] for k in order)

    fused = _FusedLoss.apply(call, *[diff[k] for k in order])

    # interpenetration (fitting.py:437-455), composed from the stand-alone modules, which are differentiable themselves
    if getattr(loss, "interpenetration", False) and s("coll_loss_weight") > 0:
        if out.vertices is None:
            raise ValueError("the interpenetration term reads every vertex: body_model(return_verts=True)")
        if body_model_faces is None:
            if model is None:
                raise ValueError("body_model_faces is needed for the interpenetration term (fitting.py:253)")
            body_model_faces = model.faces_tensor.view(-1)
        triangles = torch.index_select(out.vertices, 1, body_model_faces.to(dev)).view(B, -1, 3, 3)
        with torch.no_grad():
            collision_idxs = loss.search_tree(triangles)
        if loss.tri_filtering_module is not None:
            collision_idxs = loss.tri_filtering_module(collision_idxs)
        if collision_idxs.ge(0).sum().item() > 0:
            extras.append(_per_frame_term(loss.pen_distance(triangles, collision_idxs), B, dev) * s("coll_loss_weight"))
    return _finish(fused, extras, per_frame, dtype)


def _differentiable_camera_init(loss, out, camera, gt_joints, per_frame):
    """SMPLifyCameraInitLoss.forward of differentiable=True (fitting.py:499-520): a function of body_model_output.joints and the
    camera's rotation and translation, value and gradient from one launch (engine.camera_init_eval)."""
    joints = out.joints
    _need_cuda(joints, "body_model_output.joints")
    if joints.dim() != 3 or joints.shape[2] != 3:
        raise ValueError("body_model_output.joints: shape %s, expected (B, K, 3)" % (tuple(joints.shape),))
    B, K = int(joints.shape[0]), int(joints.shape[1])
    if K < 1 or K > engine.OBJECTIVE_MAX_K:
        raise ValueError("body_model_output.joints: K = %d keypoints, supported 1..%d" % (K, engine.OBJECTIVE_MAX_K))
    dev, dtype = joints.device, joints.dtype
    for name, t in (("camera.translation", camera.translation), ("gt_joints", gt_joints)):
        _need_cuda(t, name)
    w = _loss_scalars(loss, ["data_weight", "depth_loss_weight"])
    idx = loss.init_joints_idxs
    cached = loss.__dict__.get("_init_count")
    if cached is None or cached[0] is not idx or cached[1] != (K, dev):
        host = idx.detach().cpu().reshape(-1)
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= K):
            raise ValueError("init_joints_idxs reach %d, the joints hold K = %d keypoints" % (int(host.max()), K))
        cached = (idx, (K, dev), torch.bincount(host, minlength=K).to(dev, torch.float32))
        loss.__dict__["_init_count"] = cached
    use_conf = bool(loss.use_conf)
    if use_conf and loss.joints_conf is None:
        raise ValueError("use_conf=True needs joints_conf (fitting.py:510)")
    est = loss.trans_estimation
    fixed = dict(focal_x=_rows("camera.focal_length_x", camera.focal_length_x.detach(), (B,), dev, True),
                 focal_y=_rows("camera.focal_length_y", camera.focal_length_y.detach(), (B,), dev, True),
                 center=_rows("camera.center", camera.center.detach(), (B, 2), dev, True),
                 gt_joints=_rows("gt_joints", gt_joints.detach(), (B, K, 2), dev),
                 joints_conf=_rows("joints_conf", loss.joints_conf.detach(), (B, K), dev) if use_conf else None,
                 est_tz=_rows("trans_estimation", est.detach().reshape(-1, 3)[:, 2], (B,), dev, True) if est is not None else None)
    order = ("joints", "rotation", "translation")

    def call(j, r, t):
        value, grads = engine.camera_init_eval(j, r, t, fixed["focal_x"], fixed["focal_y"], fixed["center"], fixed["gt_joints"],
                                               cached[2], joints_conf=fixed["joints_conf"], est_tz=fixed["est_tz"],
                                               data_weight=w["data_weight"][0], depth_loss_weight=w["depth_loss_weight"][0],
                                               use_conf=use_conf)
        return value, tuple(grads[k] for k in order)

    fused = _FusedLoss.apply(call, _rows("body_model_output.joints", joints, (B, K, 3), dev),
                             _rows("camera.rotation", camera.rotation, (B, 3, 3), dev, True),
                             _rows("camera.translation", camera.translation, (B, 3), dev, True))
    return _finish(fused, [], per_frame, dtype)


class _NoMonitor(object):
    """Tolerances of a closure that is only evaluated (stand-alone loss): never used by an optimiser."""
    maxiters, ftol, gtol, steps = 1, 0.0, 0.0, 0


def _standalone_loss(loss, out, camera, gt_joints, joints_conf, joint_weights, use_vposer, pose_embedding, stage):
    bm, inputs = getattr(out, "_model", None), getattr(out, "_inputs", None)
    if bm is None or inputs is None:
        raise RuntimeError("the stand-alone loss evaluates the device objective at the PARAMETERS a ModelOutput was made "
                           "from: pass the output of this package's SMPLX.forward (it remembers them); there is no CPU forward")
    if joint_weights is None:
        joint_weights = torch.ones_like(gt_joints[..., 0])
    pe = pose_embedding if pose_embedding is not None else inputs["body_pose"]
    c = EngineClosure(_NoMonitor(), None, bm, camera, gt_joints, loss, joints_conf, joint_weights, bool(use_vposer), None,
                      pe, return_verts=True)
    try:
        return c(stage=stage, backward=False, inputs=inputs)
    finally:
        if c._fb is not None:
            c._fb.close()


class EngineClosure(object):
    """What create_fitting_closure returns: callable like the reference's `fitting_func`
    (fitting.py:232-273) and the handle run_fitting / LBFGS.step use to reach the device engine."""

    def __init__(self, monitor, optimizer, body_model, camera, gt_joints, loss, joints_conf, joint_weights,
                 use_vposer, vposer, pose_embedding, return_verts):
        self.monitor, self.optimizer, self.body_model, self.camera = monitor, optimizer, body_model, camera
        self.gt_joints, self.loss, self.joints_conf, self.joint_weights = gt_joints, loss, joints_conf, joint_weights
        self.use_vposer, self.vposer, self.pose_embedding = use_vposer, vposer, pose_embedding
        self.is_camera = isinstance(loss, SMPLifyCameraInitLoss)
        self.return_verts = return_verts
        self._fb, self._fb_stage = None, None
        self._stepped = False

    # ---- engine batch bound to the caller's tensors ------------------------------------------
    def _batch(self, stage):
        if self._fb is not None and self._fb_stage == stage:
            return self._fb
        if self._fb is not None:
            self._fb.close()
        bm, loss, cam = self.body_model, self.loss, self.camera
        dm = bm.device_model
        if self.use_vposer and not dm.vposer_latent and getattr(self.vposer, "weights", None) is not None:
            # the reference hands the decoder to the closure as an object (vposer=); a model made without smplx.create(vposer=)
            # gets its in-loop copy of the weights from it (a model that has weights keeps them)
            dm.set_vposer(self.vposer.weights)
        K = dm.K
        opt = self.optimizer
        w = capi.StageWeights()
        pen_cfg = {}
        has_reg = False
        use_hands = use_face = False
        if not self.is_camera:
            f = lambda n: float(getattr(loss, n)) if hasattr(loss, n) else 0.0
            w.body_pose_weight, w.shape_weight = f("body_pose_weight"), f("shape_weight")
            w.bending_prior_weight = f("bending_prior_weight")
            use_hands = bool(loss.use_hands and loss.left_hand_prior is not None)
            use_face = bool(loss.use_face)
            w.hand_prior_weight = f("hand_prior_weight")
            w.expr_prior_weight = f("expr_prior_weight")
            jw = getattr(loss, "jaw_prior_weight", torch.zeros(3)).detach().cpu().reshape(-1)
            jw = jw.expand(3) if jw.numel() == 1 else jw
            for q in range(3):
                w.jaw_prior_weight[q] = float(jw[q])
            if getattr(loss, "interpenetration", False) and float(getattr(loss, "coll_loss_weight", 0.0)) > 0:
                # fitting.py:437-455 with the objects of fit_single_frame.py:300-328 (smplifyx_amd.mesh_intersection)
                st, pd, tf = loss.search_tree, loss.pen_distance, loss.tri_filtering_module
                if not (hasattr(st, "max_collisions") and hasattr(pd, "sigma")):
                    raise TypeError("create_loss(search_tree=, pen_distance=): pass smplifyx_amd.mesh_intersection's BVH and "
                                    "DistanceFieldPenetrationLoss (the external CUDA package's objects cannot run here)")
                if not self.return_verts:
                    raise ValueError("the interpenetration term reads every vertex: create_fitting_closure(return_verts=True)")
                pen_cfg = dict(interpenetration=True, max_collisions=st.max_collisions, df_cone_height=pd.sigma,
                               penalize_outside=pd.penalize_outside, point2plane=bool(getattr(pd, "point2plane", False)))
                w.coll_loss_weight = float(loss.coll_loss_weight)
                # the part filter belongs to THIS loss: a loss without a FilterFaces module filters nothing, whatever an earlier
                # loss on the same model had set (fit_single_frame.py:316-328 builds the module only with a part_segm_fn)
                if tf is not None and getattr(dm, "_parts_from", None) is not tf:
                    dm.set_parts(tf.faces_segm, tf.faces_parents, tf.ign_part_pairs)
                    dm._parts_from = tf
                elif tf is None and getattr(dm, "_parts_from", None) is not None:
                    dm.clear_parts()
                    dm._parts_from = None
            reg = loss.regression_pose
            has_reg = reg is not None and (not self.use_vposer or stage + 1 == loss.num_stages)
        cfg = dict(use_vposer=self.use_vposer, use_hands=use_hands, use_face=use_face,
                   use_joints_conf=bool(getattr(loss, "use_joints_conf", False)),
                   use_conf_for_camera_init=bool(getattr(loss, "use_conf", False)),
                   high_precision=getattr(bm, "dtype", torch.float32) == torch.float64,
                   lbfgs_tolerance_grad=getattr(opt, "tolerance_grad", None), lbfgs_tolerance_change=getattr(opt, "tolerance_change", None),
                   lbfgs_max_eval=getattr(opt, "max_eval", 0), lbfgs_history_size=getattr(opt, "history_size", 0),
                   lbfgs_max_iter=getattr(opt, "max_iter", 0),      # (optim_factory.py:15 passes maxiters; a caller's own LBFGS may not)
                   maxiters=self.monitor.maxiters, ftol=self.monitor.ftol, gtol=self.monitor.gtol,
                   lr=getattr(opt, "lr", 1.0), rho=getattr(loss, "rho", 100),
                   depth_loss_weight=(float(getattr(loss, "depth_loss_weight", 0.0))
                                      if getattr(loss, "trans_estimation", None) is not None else 0.0))
        cfg.update(pen_cfg)
        fb = engine.FrameBatch(dm, 1, cfg, lbs_mode="dense" if self.return_verts else "rows",
                               reuse_entry_eval=False, has_regression_pose=has_reg, stages=[w], num_body_joints=K)
        if (not self.is_camera and not self.use_vposer and not has_reg
                and hasattr(getattr(loss, "body_pose_prior", None), "nll_weights")):
            fb.set_gmm(loss.body_pose_prior)         # body_prior_type 'gmm' (fitting.py:399-401)
        gt = _np(self.gt_joints).reshape(1, K, 2)
        if self.is_camera:
            conf = _np(loss.joints_conf).reshape(1, K) if loss.joints_conf is not None else np.ones((1, K), np.float32)
            jwts = np.ones((1, K), np.float32)
            cmask = np.zeros((1, K), np.float32)
            cmask[0, _np(loss.init_joints_idxs).astype(np.int64)] = 1
            est = _np(loss.trans_estimation)[:, 2] if loss.trans_estimation is not None else np.zeros(1, np.float32)
        else:
            conf = _np(self.joints_conf).reshape(1, K) if self.joints_conf is not None else np.ones((1, K), np.float32)
            jwts = _np(self.joint_weights).reshape(1, K)
            cmask = np.zeros((1, K), np.float32)
            est = np.zeros(1, np.float32)
        kp = np.concatenate([gt, conf[..., None]], -1)
        focal = np.stack([_np(cam.focal_length_x).reshape(1), _np(cam.focal_length_y).reshape(1)], 1)      # [1, 2]: (fx, fy)
        fb.set_frames(kp, jwts, cmask, focal, _np(cam.center), float(loss.data_weight), est_tz=est,
                      cam_rot=_np(cam.rotation).reshape(1, 9))
        self._fb, self._fb_stage = fb, stage
        self._stepped = False
        return fb

    def _push(self, fb, inputs=None):
        bm = self.body_model
        if inputs is not None:      # stand-alone loss: the tensors a ModelOutput was made from
            g = lambda n: _np(inputs[n]) if inputs.get(n) is not None else None
        else:
            g = lambda n: _np(getattr(bm, n)) if hasattr(bm, n) else None
        reg = None
        if not self.is_camera and self.loss.regression_pose is not None:
            reg = _np(self.loss.regression_pose)
        fb.set_params(regression_pose=reg, cam_translation=_np(self.camera.translation), global_orient=g("global_orient"),
                      betas=g("betas"), left_hand_pose=g("left_hand_pose"), right_hand_pose=g("right_hand_pose"),
                      expression=g("expression"), jaw_pose=g("jaw_pose"), leye_pose=g("leye_pose"),
                      reye_pose=g("reye_pose"), pose_embedding=_np(self.pose_embedding))

    @torch.no_grad()
    def _pull(self, fb):
        p = fb.get_params()
        bm = self.body_model
        tgt = dict(global_orient=bm.global_orient)
        if not self.is_camera:
            for n in ("betas", "left_hand_pose", "right_hand_pose", "expression", "jaw_pose", "leye_pose", "reye_pose"):
                if hasattr(bm, n):
                    tgt[n] = getattr(bm, n)
            self.pose_embedding.copy_(torch.as_tensor(p["pose_embedding"]).to(self.pose_embedding))
        else:
            self.camera.translation.copy_(torch.as_tensor(p["cam_translation"]).to(self.camera.translation))
        for n, t in tgt.items():
            t.copy_(torch.as_tensor(p[n]).to(t))

    def _var_params(self):
        """Tensors in the order of the engine's flat variable vector for this closure."""
        bm = self.body_model
        if self.is_camera:
            return [self.camera.translation, bm.global_orient]
        ps = [p for p in bm.parameters() if p.requires_grad] + [self.pose_embedding]
        return ps

    def _check_params(self, params):
        want = self._var_params()
        if len(params) != len(want) or any(a is not b for a, b in zip(params, want)):
            raise NotImplementedError("the device engine optimises [camera.translation, global_orient] (camera stage) "
                                      "or body_model.parameters() + [pose_embedding] (body stages); got another set")

    # ---- the reference's fitting_func(stage=0, backward=True) ------------------------------------
    def __call__(self, stage=0, backward=True, inputs=None):
        fb = self._batch(stage)
        self._push(fb, inputs)
        loss, grad = fb.closure(-1 if self.is_camera else 0)
        if backward:
            self._set_grads(grad)
        self.monitor.steps += 1
        dev = self.body_model.faces_tensor.device
        return torch.tensor(float(loss[0]), dtype=torch.float32, device=dev)

    def _set_grads(self, grad):
        o = 0
        ps = self._var_params()
        # (the device leaves the dead body_pose parameter out of its variable vector when it would not fit: use_pca=False)
        dead_on_device = sum(p.numel() for p in ps) == grad.shape[1]
        for p in ps:
            n = p.numel()
            if self._is_dead(p):
                p.grad = None
                o += n if dead_on_device else 0
                continue
            p.grad = torch.as_tensor(grad[0, o:o + n]).reshape(p.shape).to(p)
            o += n

    def _is_dead(self, p):
        return (not self.use_vposer) and hasattr(self.body_model, "body_pose") and p is self.body_model.body_pose

    def run_stage(self, stage):
        fb = self._batch(stage)
        self._push(fb)
        fb.fit(first_stage=-1 if self.is_camera else 0, last_stage=-1 if self.is_camera else 0)
        self._pull(fb)
        st = fb.stats()
        slot = 0 if self.is_camera else 1
        self.monitor.steps += int(st["stage_evals"][0, slot])
        v = float(st["stage_loss"][0, slot])
        return None if np.isnan(v) else v

    def step(self, stage):
        fb = self._batch(stage)
        self._push(fb)
        loss = fb.step(-1 if self.is_camera else 0, resume=self._stepped)
        self._stepped = True
        self._pull(fb)
        self._set_grads(fb.last_grad(-1 if self.is_camera else 0))      # var.grad after step()
        dev = self.body_model.faces_tensor.device
        return torch.tensor(float(loss[0]), dtype=torch.float32, device=dev)


class FittingMonitor(object):
    def __init__(self, summary_steps=1, visualize=False, maxiters=100, ftol=2e-09, gtol=1e-05,
                 body_color=(1.0, 1.0, 0.9, 1.0), model_type="smpl", **kwargs):
        self.maxiters, self.ftol, self.gtol = maxiters, ftol, gtol
        self.visualize, self.summary_steps = visualize, summary_steps
        self.body_color, self.model_type = body_color, model_type
        if visualize:       # fitting.py:126-138: the mesh viewer; outside the fitting path, so nothing is drawn
            import warnings
            warnings.warn("FittingMonitor(visualize=True): no mesh viewer in this engine; the fit itself is unaffected")

    def __enter__(self):
        self.steps = 0
        return self

    def __exit__(self, exception_type, exception_value, traceback):
        pass

    def run_fitting(self, optimizer, closure, params, body_model, stage, use_vposer=True, pose_embedding=None,
                    vposer=None, **kwargs):
        """The whole step loop (fitting.py:174-217) on device for the 'lbfgsls' optimiser; returns the
        step-entry loss of the last step, like the reference.  Any other optimiser (torch.optim objects of
        optim_factory) is driven from the host with the same stopping rules, each closure evaluation on
        the device.  A closure the caller wrote (any callable) with this package's LBFGS runs the same host loop
        over optimizer.step, whose line searches run on the device."""
        if not isinstance(closure, EngineClosure):
            # a closure the caller wrote, with this package's LBFGS: the reference's host loop over optimizer.step, each step's
            # line searches on the device (optimizers/lbfgs_ls.py)
            if not (hasattr(optimizer, "_bind") and getattr(optimizer, "_closure", None) is None and callable(closure)):
                raise TypeError("run_fitting needs the closure returned by create_fitting_closure, or -- with optimizers.lbfgs_ls."
                                "LBFGS -- any callable that zeroes the gradients, calls backward and returns the loss")
            if optimizer.per_sample:
                raise NotImplementedError("run_fitting drives ONE problem, like the reference; for a batch of independent problems "
                                          "run the whole loop on the device: engine.BatchOptimizer(...).begin(x0, mode='fit')")
            step_closure = closure
        elif hasattr(optimizer, "_bind"):
            closure._check_params(list(params))
            return closure.run_stage(stage)
        else:
            step_closure = lambda: closure(stage=stage)
        params = list(params)
        prev_loss = None
        for n in range(self.maxiters):
            loss = optimizer.step(step_closure)
            if torch.isnan(loss).sum() > 0 or torch.isinf(loss).sum() > 0:
                break
            if n > 0 and prev_loss is not None and self.ftol > 0:
                if utils.rel_change(prev_loss, loss.item()) <= self.ftol:
                    break
            if all(torch.abs(var.grad.view(-1).max()).item() < self.gtol for var in params if var.grad is not None):
                break
            prev_loss = loss.item()
        return prev_loss

    def create_fitting_closure(self, optimizer, body_model, camera=None, gt_joints=None, loss=None,
                               joints_conf=None, joint_weights=None, return_verts=True, return_full_pose=False,
                               use_vposer=False, vposer=None, pose_embedding=None, create_graph=False, **kwargs):
        if not hasattr(self, "steps"):
            self.steps = 0
        c = EngineClosure(self, optimizer, body_model, camera, gt_joints, loss, joints_conf, joint_weights,
                          use_vposer, vposer, pose_embedding, return_verts)
        if optimizer is not None and hasattr(optimizer, "_bind"):
            optimizer._bind(c)
        return c
